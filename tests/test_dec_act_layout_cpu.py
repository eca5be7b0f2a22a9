"""The LDS map of an image workgroup of the fused decoder launch (svgp_mnist_decoder_fwd_bwd_data_pre[_aji | _tail]): d2, d1 and a2
are kept at a padded pixel stride, paid for inside the unchanged footprint by two aliases of arrays that are never live together (d1 in
the d3 block, dh0 on h0).  Checked on svgp_mnist_decoder_fused_lds_array / _fused_lds_index, the host entries that evaluate the
constexpr functions the kernel takes its pointers and index maps from, and on the bank model of tools/lds_bank_model.py; no GPU.

The bounds of the bank model are those of the table the strides were chosen from (mean and maximum number of distinct dwords on the
busiest bank per service group): d2 gathers <= 2.3 (3), d1 gathers <= 3.7 (4) -- <= 3 at stride 9 or 11 --, a2 gathers <= 1.4 (2);
on the packed strides the same functions must return 7.2 (9), 7.1 (8) and 3.0 (4), which is the guard that the model sees the problem."""
import ctypes as C
import itertools
import os
import sys

import pytest

import svgp_vae_amd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import lds_bank_model as M  # noqa: E402

NAMES = M.ARRAYS                    # dense, weff, z, h0, a1, a2, d3, d2, d1, dh0, red
PACKED = dict(z=64, h0=128, a1=512, a2=1568, d3=784, d2=1568, d1=512, dh0=128, red=16)      # packed elements of each array
LS = (1, 4, 16, 64)


@pytest.fixture(scope="module")
def lib():
    return svgp_vae_amd.load_library()


def _array(lib, L, which):
    o, s, f, l = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7)
    n = lib.svgp_mnist_decoder_fused_lds_array(L, which, C.byref(o), C.byref(s), C.byref(f), C.byref(l))
    return dict(extent=n, offset=o.value, stride=s.value, first=f.value, last=l.value)


def _arrays(lib, L):
    return {name: _array(lib, L, w) for w, name in enumerate(NAMES)}


def test_refusals(lib):
    null = C.POINTER(C.c_int)()
    assert lib.svgp_mnist_decoder_fused_lds_array(16, 5, null, null, null, null) == _array(lib, 16, 5)["extent"]     # NULLs are skipped
    for L, which in ((0, 5), (65, 5), (16, -1), (16, len(NAMES))):
        assert lib.svgp_mnist_decoder_fused_lds_array(L, which, null, null, null, null) == -1
    assert lib.svgp_mnist_decoder_fused_lds_index(0, 0) == -1                   # the dense weights have no element map
    for which, name in enumerate(NAMES):
        if name in PACKED:
            assert lib.svgp_mnist_decoder_fused_lds_index(which, -1) == -1
            assert lib.svgp_mnist_decoder_fused_lds_index(which, PACKED[name]) == -1
            assert lib.svgp_mnist_decoder_fused_lds_index(which, PACKED[name] - 1) >= 0
    assert lib.svgp_mnist_decoder_fused_lds_index(1, 2176) == -1 and lib.svgp_mnist_decoder_fused_lds_index(len(NAMES), 0) == -1


def test_index_map_is_injective_and_inside_its_block(lib):
    a = _arrays(lib, 16)
    for which, name in enumerate(NAMES):
        if name not in PACKED:
            continue
        places = [lib.svgp_mnist_decoder_fused_lds_index(which, e) for e in range(PACKED[name])]
        assert len(set(places)) == len(places), name
        assert min(places) == 0 and max(places) < a[name]["extent"], (name, max(places), a[name]["extent"])
        s = a[name]["stride"]
        if s >= 8:          # pixel * 8 + channel -> pixel * stride + channel: the copy-outs' remap i -> (i >> 3) * S + (i & 7)
            assert places == [(e >> 3) * s + (e & 7) for e in range(PACKED[name])], name
        else:
            assert places == list(range(PACKED[name])), name
    # the weight image: the map of svgp_mnist_decoder_weff_lds_offset, the three layers back to back
    for layer, first, n in ((0, 0, 1024), (1, 1024, 1024), (2, 2048, 128)):
        for e in (0, 1, n // 2 + 3, n - 1):
            assert lib.svgp_mnist_decoder_fused_lds_index(1, first + e) == lib.svgp_mnist_decoder_weff_lds_offset(layer, e)
    assert a["weff"]["extent"] == lib.svgp_mnist_decoder_weff_lds_offset(2, 128)


def test_only_d2_d1_a2_are_padded_and_the_global_copies_stay_packed(lib):
    a = _arrays(lib, 16)
    assert {n: a[n]["stride"] for n in ("h0", "a1", "dh0")} == dict(h0=8, a1=8, dh0=8)
    assert a["d3"]["stride"] == 1 and a["z"]["stride"] == a["red"]["stride"] == a["dense"]["stride"] == a["weff"]["stride"] == 0
    for n in ("a2", "d2", "d1"):
        assert a[n]["stride"] > 8 and a[n]["extent"] == PACKED[n] // 8 * a[n]["stride"], (n, a[n])
    for n in ("z", "h0", "a1", "d3", "dh0", "red"):
        assert a[n]["extent"] == PACKED[n], n


@pytest.mark.parametrize("L", LS)
def test_live_arrays_share_no_byte_and_the_two_aliases_are_never_live_together(lib, L):
    a = _arrays(lib, L)
    total = lib.svgp_mnist_decoder_fused_lds_bytes(L)
    for n, v in a.items():
        assert v["extent"] > 0 and 0 <= v["offset"] and (v["offset"] + v["extent"]) * 8 <= total, (n, v, total)
        assert 1 <= v["first"] <= v["last"] <= 14, (n, v)         # inside one trip of the image loop: the same order for every image
    shared = set()
    for x, y in itertools.combinations(NAMES, 2):
        bytes_overlap = a[x]["offset"] < a[y]["offset"] + a[y]["extent"] and a[y]["offset"] < a[x]["offset"] + a[x]["extent"]
        live_overlap = a[x]["first"] <= a[y]["last"] and a[y]["first"] <= a[x]["last"]
        assert not (bytes_overlap and live_overlap), (x, y, a[x], a[y])
        if bytes_overlap:
            shared.add((x, y))
    assert shared == {("d3", "d1"), ("h0", "dh0")}, shared
    assert a["d1"]["offset"] >= a["d3"]["offset"] and a["d1"]["offset"] + a["d1"]["extent"] <= a["d3"]["offset"] + a["d3"]["extent"]
    assert (a["dh0"]["offset"], a["dh0"]["extent"]) == (a["h0"]["offset"], a["h0"]["extent"])
    # what the intervals say, spelled out: d3 is dead (last read: UpC3 data reverse, stamp 8) before d1 is born (UpC2 data reverse,
    # stamp 10), h0 (copy-out, 7) before dh0 (UpC1 data reverse, 12)
    assert a["d3"]["last"] == 8 and a["d1"]["first"] == 10 and a["h0"]["last"] == 7 and a["dh0"]["first"] == 12


@pytest.mark.parametrize("L", LS)
def test_alignment_of_the_16_byte_reads(lib, L):
    a = _arrays(lib, L)
    assert a["a2"]["stride"] % 2 == 0 and a["a2"]["offset"] % 2 == 0        # tap_operand_group's activation reads of UpC3's forward
    assert a["h0"]["offset"] % 2 == 0 and a["a1"]["offset"] % 2 == 0        # ... of UpC1's and UpC2's
    assert a["weff"]["offset"] == L * 128 + 128 + 32 and a["weff"]["offset"] % 2 == 0      # We1 where dec_fwd_bwd_we_offset puts it
    assert a["dense"]["offset"] == 0 and a["dense"]["extent"] == a["weff"]["offset"]
    assert a["z"]["offset"] == a["weff"]["offset"] + a["weff"]["extent"]
    which = NAMES.index("a2")
    for p in range(196):
        for c in range(0, 8, 2):
            i = lib.svgp_mnist_decoder_fused_lds_index(which, p * 8 + c)
            assert (a["a2"]["offset"] + i) % 2 == 0 and lib.svgp_mnist_decoder_fused_lds_index(which, p * 8 + c + 1) == i + 1


def test_footprint_is_unchanged(lib):
    assert lib.svgp_mnist_decoder_fused_lds_bytes(16) == 77744
    for L in LS:            # the packed sum, whatever the strides: two workgroups per compute unit depend on it at L = 16
        assert lib.svgp_mnist_decoder_fused_lds_bytes(L) == (L * 128 + 128 + 32 + 2230 + 64 + 128 + 512 + 1568 + 784 + 1568 + 512 + 128 + 16) * 8


def _mean_max(degrees):
    return sum(degrees) / len(degrees), max(degrees)


def test_bank_model_bounds_of_the_padded_gathers(lib):
    lay = M.library_layout(lib, 16)
    (_, f2), (_, f1), (_, fa) = M.PADDED
    d2, d1, a2 = f2(lay), f1(lay), fa(lay)
    assert (len(d2), len(d1), len(a2)) == (256, 64, 784)
    print("d2 gathers: mean %.3f max %d;  d1: %.3f %d;  a2: %.3f %d" % (_mean_max(d2) + _mean_max(d1) + _mean_max(a2)))
    assert _mean_max(d2)[1] <= 3 and _mean_max(d2)[0] <= 2.3
    assert _mean_max(d1)[1] <= (3 if lay.stride["d1"] in (9, 11) else 4) and _mean_max(d1)[0] <= 3.7
    assert _mean_max(a2)[1] <= 2 and _mean_max(a2)[0] <= 1.4


def test_bank_model_sees_the_problem_on_the_packed_strides(lib):
    lay = M.packed_layout(lib, 16)
    (_, f2), (_, f1), (_, fa) = M.PADDED
    got = [_mean_max(f(lay)) for f in (f2, f1, fa)]
    print(got)
    for (mean, mx), (want_mean, want_max) in zip(got, ((7.2, 9), (7.1, 8), (3.0, 4))):
        assert round(mean, 1) == want_mean and mx == want_max, got
    # ... and the same through with_strides on the library's own map: only the stride matters to a gather
    lay8 = M.with_strides(M.library_layout(lib, 16), d2=8, d1=8, a2=8)
    assert [_mean_max(f(lay8)) for f in (f2, f1, fa)] == got


def test_bank_model_covers_the_groups_the_padding_does_not_touch(lib):
    """the separation of where the remaining conflicts sit: every other access group of an image is in the table, and none of those
    the padding does not reach changes between the two layouts"""
    packed, padded = M.table(M.packed_layout(lib, 16)), M.table(M.library_layout(lib, 16))
    assert [r[0] for r in packed] == [r[0] for r in padded] and len(packed) == len(M.PADDED) + len(M.OTHERS)
    names = " | ".join(r[0] for r in packed)
    for needle in ("bwd_data_valu", "B operands", "stores", "dense", "z-bar"):
        assert needle in names, needle
    touched = ("a2", "d2", "d1")
    for p, q in zip(packed, padded):
        if not any(t in p[0] for t in touched):
            assert p == q, (p, q)
    # the padding pays: fewer passes beyond one per group over the whole image, not only in the three gathers
    assert sum(r[4] for r in padded) < sum(r[4] for r in packed) - 2000
