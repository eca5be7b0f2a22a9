"""The LDS image of the decoder's effective weights in the fused launch (svgp_mnist_decoder_fwd_bwd_data_pre[_aji | _tail]): the four
parity classes of each up-convolution sit a padded stride apart, so that the lanes of one 16-byte read -- neighbouring output
pixels, hence different classes -- use disjoint banks.  Checked on svgp_mnist_decoder_weff_lds_offset, the host entry that evaluates
the constexpr function the kernel stages with; no GPU.

The banking rule is the one of ds_read_b128 on gfx950: bank of byte address a = (a / 4) mod 64, conflicts only within a 16-lane
group, equal addresses broadcast.  What a group reads for one (tap, ci):
  UpC1, UpC2 (8 -> 8 channels, a lane = output pixel x channel pair): per class the 4 pairs of that (tap, ci), 64 contiguous bytes;
  UpC3 (8 -> 1, a lane = output pixel): per class the 16 bytes (ci, ci + 1) of that tap.
Lanes of one class read the same addresses; the classes must not share a bank."""
import itertools

import pytest

import svgp_vae_amd

LAYERS = [(8, 8), (8, 8), (8, 1)]           # (CIN, COUT) of UpC1, UpC2, UpC3
BANKS = 64


@pytest.fixture(scope="module")
def offset():
    lib = svgp_vae_amd.load_library()
    return lambda layer, e: int(lib.svgp_mnist_decoder_weff_lds_offset(layer, e))


def _packed(cin, cout):
    return lambda cls, tap, ci, co: ((cls * 4 + tap) * cin + ci) * cout + co


def _banks(first_double, n_doubles):
    return {(a // 4) % BANKS for a in range(first_double * 8, (first_double + n_doubles) * 8, 4)}


def _group_reads(layer, cin, cout, tap, ci, at):
    """[(first double, doubles)] per class of what one lane group reads for (tap, ci); `at` maps a packed index to its place.

    This is a model of UpConv3::fwd_valu (csrc/vae_dev.hpp), not derived from it: item `it` = thread index, channel group
    cg = it % NCG (NCG = COUT / 2 = 4, or 1 for COUT = 1), output pixel p = it / NCG, class = parity of the pixel, and per (tap, ci)
    one 16-byte read at wc + tap * CIN * COUT + ci * COUT (+ 2 cg), or for COUT = 1 one per pair (ci, ci + 1).  So 16 lanes hold
    whole pixels with all their channel groups, and what can differ between lanes is the class and cg.  If that item order or the
    read width changes, this model has to change with it."""
    e = _packed(cin, cout)
    if cout == 1:
        return [(at(layer, e(cls, tap, ci & ~1, 0)), 2) for cls in range(4)]
    return [(at(layer, e(cls, tap, ci, 0)), cout) for cls in range(4)]


def test_map_is_injective_and_inside_each_layer_block(offset):
    start = 0
    for layer, (cin, cout) in enumerate(LAYERS):
        n = 16 * cin * cout
        end = offset(layer, n)
        places = [offset(layer, e) for e in range(n)]
        assert len(set(places)) == n, layer
        assert min(places) == start and max(places) < end, (layer, start, min(places), max(places), end)
        assert offset(layer, -1) == -1 and offset(layer, n + 1) == -1
        # within a class the packed order is kept: only the class stride moved
        nwc = 4 * cin * cout
        for cls in range(4):
            assert places[cls * nwc:(cls + 1) * nwc] == list(range(places[cls * nwc], places[cls * nwc] + nwc)), (layer, cls)
        start = end
    assert offset(3, 0) == -1 and offset(-1, 0) == -1


def test_every_16_byte_read_is_aligned(offset):
    """the image starts an even count of doubles into a 16-byte aligned LDS block: every channel pair (UpC1, UpC2) and every
    (ci, ci + 1) pair (UpC3) must start at an even offset, and its second element follow"""
    lib = svgp_vae_amd.load_library()
    for L in (1, 8, 16, 64):            # doubles in front of the image: L * 128 dense weights + 128 + 32 biases
        assert (L * 128 + 128 + 32) % 2 == 0
        assert lib.svgp_mnist_decoder_fused_lds_bytes(L) % 16 == 0
    for layer, (cin, cout) in enumerate(LAYERS):
        e = _packed(cin, cout)
        for cls, tap, ci in itertools.product(range(4), range(4), range(cin)):
            if cout == 1:
                if ci % 2 == 0:
                    o = offset(layer, e(cls, tap, ci, 0))
                    assert o % 2 == 0 and offset(layer, e(cls, tap, ci + 1, 0)) == o + 1
            else:
                for co in range(0, cout, 2):
                    o = offset(layer, e(cls, tap, ci, co))
                    assert o % 2 == 0 and offset(layer, e(cls, tap, ci, co + 1)) == o + 1


def test_the_four_classes_of_a_read_use_disjoint_banks(offset):
    for layer, (cin, cout) in enumerate(LAYERS):
        for tap, ci in itertools.product(range(4), range(cin)):
            sets = [_banks(*r) for r in _group_reads(layer, cin, cout, tap, ci, offset)]
            assert all(len(s) == (4 if cout == 1 else 16) for s in sets)
            for x, y in itertools.combinations(range(4), 2):
                assert not (sets[x] & sets[y]), (layer, tap, ci, x, y)


def test_the_packed_layout_does_not_have_that_property():
    """guards the check above: with the classes 4 * CIN * COUT doubles apart (ws.dec_weff) every class lands on the same banks"""
    for layer, (cin, cout) in enumerate(LAYERS):
        sets = [_banks(*r) for r in _group_reads(layer, cin, cout, 0, 0, lambda _, e: e)]
        assert sets[0] == sets[1] == sets[2] == sets[3]


def test_an_image_workgroup_still_fits_twice_on_a_compute_unit(offset):
    lib = svgp_vae_amd.load_library()
    total = lib.svgp_mnist_decoder_fused_lds_bytes(16)
    assert 0 < total <= 81920, total
    # the image is what grew: everything else of dec_fwd_bwd_lds(16) is the activations, the dense weights and the biases
    other = 16 * 128 + 128 + 32 + 64 + 128 + 512 + 1568 + 784 + 1568 + 512 + 128 + 16
    assert total == (other + offset(2, 16 * 8 * 1)) * 8
    assert lib.svgp_mnist_decoder_fused_lds_bytes(0) == -1 and lib.svgp_mnist_decoder_fused_lds_bytes(65) == -1
