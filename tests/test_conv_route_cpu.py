"""Which kernels a convolution call runs (csrc/conv_taps.hip: conv_fwd_plan / conv_wgrad_plan, read back as text through
svgp_conv_route), pinned without a GPU for every layer shape the project uses: the CASES of tests/test_gpu_conv.py and the 16
layers of the SPRITES networks, forward, data gradient and fused weight gradient, at n = 3 and 500 frames, 64 and 1024
weight-gradient workgroups, with and without an activation, float64 and float32.

A route has one line per launch, zero fill of the partials or partial-sum job: the kernel family with the template values of the
instance (flags as 0 / 1), the by-value scalars, grid, LDS bytes, class (-1: one launch for every class) and descriptor form (as
given / taps in grid order).  Table notation: `lds=<N>e` is N elements of the call's type (N * 8 or N * 4 bytes in the route);
`{out}` in a template list is the ACT flag: 1 when the call has the layer output (ELU' applied in the kernel), else 0.  A key names
only the parameters the route depends on."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

import svgp_vae_amd
from svgp_vae_amd import _lib
from svgp_vae_amd.conv import ConvLayer
from svgp_vae_amd.sprites import DEC_UP, ENC_STRIDES
from tests.test_gpu_conv import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sprites.py SpritesStepEngine, Lc = 16: encoder, decoder, representation network as (Hi, Ci, Co, k, stride, padding, up)
SPRITES = [(h, ci, 16, 3, s, "same", False) for h, ci, s in zip((64, 64, 32, 32, 16, 16), (3, 16, 16, 16, 16, 16), ENC_STRIDES)] + \
          [(h, 16, 16 if i < 6 else 3, 3, 1, "same", u) for i, (h, u) in enumerate(zip((8, 16, 16, 32, 32, 64, 64), DEC_UP))] + \
          [(h, ci, 16, 2, 2, "same", False) for h, ci in zip((64, 32, 16), (3, 16, 16))]
LAYERS = list(dict.fromkeys([c[:7] for c in CASES] + SPRITES))          # a route does not depend on the activation flag
FAMILIES = ["conv16_thin_fwd", "conv16_fwd_roll", "conv16_fwd", "convS_fwd_ring", "convS_fwd", "conv_taps_fwd",
            "convS_wgrad_ring", "convS_wgrad", "conv_taps_wgrad", "conv16_wgrad_grid", "conv16_wgrad_roll", "conv16_wgrad"]
# kernel families that no CASES entry reaches in any pass (each would need a case at the smallest shape that reaches it, or a
# note that a ConvLayer cannot reach it): none
UNREACHED_BY_CASES = []


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(svgp_vae_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _route(ds, pas, out=0, nwg=1, part_stride=1, elem=8, cap=4096):
    arr, buf = (_lib.ConvDesc * len(ds))(*ds), C.create_string_buffer(cap)
    _lib.call("svgp_conv_route", arr, len(ds), pas, out, nwg, part_stride, elem, buf, cap)
    return buf.value.decode().splitlines()


def _layer(key):
    Hi, Ci, Co, k, s, pad, up = key
    return ConvLayer(Hi, Ci, Co, k=k, stride=s, padding=pad, up=up)


def _routes(key, kind):
    """{(n, nwg, out, elem): route} of one layer and pass over the whole parameter set (nwg, out: weight gradient only)."""
    lay, res = _layer(key), {}
    for n, elem in itertools.product((3, 500), (8, 4)):
        if kind == "wgrad":
            for nwg, out in itertools.product((64, 1024), (0, 1)):
                res[(n, nwg, out, elem)] = _route(lay.descs_fwd(n, act=0), 1, out, nwg, lay.n_wf, elem)
        else:
            res[(n, None, None, elem)] = _route(lay.descs_fwd(n) if kind == "fwd" else lay.descs_bwd_data(n), 0, elem=elem)
    return res


def _expected(key, kind, n, nwg, out, elem):
    table = ROUTES[key][kind]
    vals = {"n": n, "nwg": nwg, "out": out, "elem": elem}
    names = re.findall(r"(\w+)=", next(iter(table)))
    tkey = " ".join(f"{m}={vals[m]}" for m in names) or "any"
    lines = [ln.replace("{out}", str(out)) for ln in table[tkey]]
    return tkey, [re.sub(r"lds=(\d+)e", lambda m: f"lds={int(m.group(1)) * elem}", ln) for ln in lines]


def _families(lines):
    return {re.match(r"\w+", ln).group(0) for ln in lines} & set(FAMILIES)


def _default(key, kind, elem=8, out=1):          # the route at the shapes of tests/test_gpu_conv.py: n = 3, nwg = 64
    return _routes(key, kind)[(3, 64, out, elem) if kind == "wgrad" else (3, None, None, elem)]


def test_every_plan_equals_the_table():
    assert set(ROUTES) == set(LAYERS)
    bad, used = [], set()
    for key in LAYERS:
        for kind in ("fwd", "bwd_data", "wgrad"):
            for (n, nwg, out, elem), got in _routes(key, kind).items():
                tkey, want = _expected(key, kind, n, nwg, out, elem)
                used.add((key, kind, tkey))
                if got != want:
                    bad.append((key, kind, n, nwg, out, elem, got, want))
    assert not bad, f"{len(bad)} routes differ from the table, the first: {bad[0]}"
    assert used == {(key, kind, tkey) for key in ROUTES for kind in ROUTES[key] for tkey in ROUTES[key][kind]}


def test_spot_checks_of_the_launch_trace():
    """The parent's launches (kernel stub, grid, LDS bytes of the calls at n = 3, nwg = 64, float64), as the issue lists them."""
    f, w = (lambda key: _default(key, "fwd")), (lambda key: _default(key, "wgrad"))
    sums = lambda r: [re.match(r"sum_partials ng=\d+ len=(\d+) ", ln).group(1) for ln in r]
    r = f((64, 3, 16, 3, 1, "same", False))
    assert len(r) == 1 and r[0].startswith("convS_fwd_ring<3,3,1,3,1> ") and " grid=(18,1,1) " in r[0]
    r = w((64, 3, 16, 3, 1, "same", False))
    assert r[0].startswith("convS_wgrad_ring<3,3,1,3,1,0> ") and " grid=(64,1,1) " in r[0] and sums(r[1:]) == ["432", "16"]
    r = f((64, 16, 16, 3, 2, "same", False))
    assert len(r) == 1 and r[0].startswith("conv16_fwd_roll<3,3,2,1,1> ") and " grid=(6,1,1) " in r[0]
    r = w((64, 16, 16, 3, 2, "same", False))
    assert r[0].startswith("conv16_wgrad_grid<3,3,2,2,1> ") and " lds=76032 " in r[0] and sums(r[1:]) == ["2304", "16"]
    r = f((64, 16, 3, 3, 1, "same", False))
    assert len(r) == 1 and r[0].startswith("conv16_thin_fwd<3,3,3> ") and " grid=(23,1,1) " in r[0]
    r = w((64, 16, 3, 3, 1, "same", False))
    assert [ln.split()[0] for ln in r] == ["elu_bwd_colsum", "sum_partials", "convS_wgrad_ring<3,3,1,3,0,1>", "sum_partials"]
    assert sums(r[1::2]) == ["3", "432"]
    r = f((20, 5, 7, 3, 1, "same", False))
    assert len(r) == 1 and r[0].startswith("conv_taps_fwd<0,0> ") and " grid=(6,1,3) lds=23616 " in r[0]
    r = w((20, 5, 7, 3, 1, "same", False))
    assert any(ln.startswith("conv_taps_wgrad ") and " grid=(64,1,1) lds=41024 " in ln for ln in r)
    r = f((37, 16, 5, 3, 1, "valid", False))
    assert len(r) == 1 and r[0].startswith("conv16_fwd_roll<3,3,1,1,0> ") and " grid=(18,1,1) " in r[0]
    r = w((37, 16, 5, 3, 1, "valid", False))
    assert r[0].startswith("conv16_wgrad_roll<9,1> ") and " lds=27648 " in r[0]
    r = f((6, 16, 16, 3, 1, "same", False))
    assert len(r) == 1 and r[0].startswith("conv16_fwd<9> ") and " grid=(3,1,1) " in r[0]
    r = w((6, 16, 16, 3, 1, "same", False))
    assert r[0].startswith("conv16_wgrad<9> ") and " lds=16384 " in r[0]


def test_the_kernels_the_comments_of_test_gpu_conv_name():
    """tests/test_gpu_conv.py says which kernel a group of CASES is there for; here that is checked."""
    for c in CASES:
        key = c[:7]
        fwd, wg = _default(key, "fwd"), _default(key, "wgrad")
        for elem in (8, 4):
            assert _families(_default(key, "fwd", elem)) == _families(fwd) and _families(_default(key, "wgrad", elem)) == _families(wg)
        if c[1] == 16:          # "16 input channels = the direct kernels (k_conv16_*)"
            assert _families(fwd) <= {"conv16_thin_fwd", "conv16_fwd_roll", "conv16_fwd"}, (key, fwd)
        if c[1] == 16 and c[2] == 3:        # "k_conv16_thin_fwd (16 -> 3) at widths that are not multiples of its 14-column segments"
            assert _families(fwd) == {"conv16_thin_fwd"}, (key, fwd)
    thin = [c for c in CASES if c[1] == 16 and c[2] == 3]
    assert {c[5] for c in thin} == {"same", "valid"} and {c[7] for c in thin} == {True, False}
    assert any(_layer(c[:7]).Ho % 14 and _layer(c[:7]).Ho % 16 for c in thin)
    # "k_conv16_wgrad_grid (16 -> 16, width a multiple of 16): three 16-pixel segments"
    key = (48, 16, 16, 3, 1, "same", False)
    assert key in [c[:7] for c in CASES]
    assert _families(_default(key, "wgrad")) == {"conv16_wgrad_grid"} and " nseg=3 " in _default(key, "fwd")[0] + " "
    # the cases the odd-row-block test selects (its -k expression) all take k_conv16_wgrad_grid, except the 3 -> 16 layer
    for key in [(64, 16, 16, 3, 2, "same", False), (16, 16, 16, 3, 1, "same", False), (32, 16, 16, 3, 1, "same", True),
                (32, 16, 16, 2, 2, "same", False), (48, 16, 16, 3, 1, "same", False)]:
        assert key in [c[:7] for c in CASES] and _families(_default(key, "wgrad")) == {"conv16_wgrad_grid"}, key
    # widths that are no multiple of 16, fewer than 16 output channels, narrow images: the rolling and the non-rolling forms both run
    c16 = set().union(*[_families(_default(c[:7], k)) for c in CASES if c[1] == 16 for k in ("fwd", "bwd_data", "wgrad")])
    assert {"conv16_fwd_roll", "conv16_fwd", "conv16_wgrad_roll", "conv16_wgrad", "conv16_wgrad_grid"} <= c16


def test_kernel_families_no_case_reaches():
    reached = set()
    for c in CASES:
        for kind in ("fwd", "bwd_data", "wgrad"):
            for (n, nwg, out, elem), r in _routes(c[:7], kind).items():
                if n == 3 and nwg in (None, 64):            # the shapes test_gpu_conv.py runs
                    reached |= _families(r)
    missing = [f for f in FAMILIES if f not in reached]
    print("kernel families no CASES entry reaches:", missing or "none")
    assert missing == UNREACHED_BY_CASES


def test_route_text_that_does_not_fit_is_refused():
    ds = _layer(LAYERS[0]).descs_fwd(3)
    with pytest.raises(svgp_vae_amd.SvgpError, match="route text"):
        _route(ds, 0, cap=16)
    with pytest.raises(svgp_vae_amd.SvgpError, match="bad argument"):
        _route(ds, 2)
    with pytest.raises(svgp_vae_amd.SvgpError, match="bad argument"):
        _route(ds, 0, elem=2)


def _dump_hook_routes():
    """(child interpreter) every route at n = 3, nwg = 64, float64, as JSON on stdout"""
    print(json.dumps([[list(key), kind, _default(key, kind)] for key in LAYERS for kind in ("fwd", "bwd_data", "wgrad")]))


@pytest.mark.parametrize("rows", [3, 5])
def test_row_count_hook_changes_only_the_rows_per_wave(rows):
    """SVGP_CONV_ROWS (the library's test hook, read once per process, hence the child interpreter): the k_conv16_wgrad_grid routes
    keep everything but RW, which becomes min(rows, ceil(Hs / 4)); tests/test_gpu_conv.py relies on that for its odd row blocks.
    Every other route may differ from the unhooked one only in what follows from the rows per wave: RW, R, strips, ntask, grid."""
    r = subprocess.run([sys.executable, "-c", "from tests import test_conv_route_cpu as t; t._dump_hook_routes()"],
                       env=dict(os.environ, SVGP_CONV_ROWS=str(rows)), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    changed = 0
    for key, kind, hooked in json.loads(r.stdout.splitlines()[-1]):
        plain = _default(tuple(key), kind)
        if kind != "wgrad" or _families(plain) != {"conv16_wgrad_grid"}:
            loose = lambda lines: [re.sub(r" (RW|R|strips|ntask)=\d+| grid=\(\d+,", " *", ln) for ln in lines]
            assert loose(hooked) == loose(plain), (key, kind, hooked, plain)
            continue
        mask = lambda lines: [re.sub(r" RW=\d+", " RW=*", ln) for ln in lines]
        assert mask(hooked) == mask(plain), (key, hooked, plain)
        Hs = _layer(tuple(key)).descs_fwd(3)[0].Hs
        assert f" RW={min(rows, (Hs + 3) // 4)}" in hooked[0] and f" RW={min(8, (Hs + 3) // 4)}" in plain[0], (key, hooked[0], plain[0])
        changed += hooked != plain
    assert changed >= 4


ROUTES = {
    # 64x64 3->16 k3 s1 same
    (64, 3, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["convS_fwd_ring<3,3,1,3,1> ntask=72 nseg=4 nrb=6 RW=12 grid=(18,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["convS_fwd_ring<3,3,1,3,1> ntask=12000 nseg=4 nrb=6 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_thin_fwd<3,3,3> ntask=90 nseg=5 nrb=6 RW=12 grid=(23,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_thin_fwd<3,3,3> ntask=15000 nseg=5 nrb=6 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "convS_wgrad_ring<3,3,1,3,{out},0> nwg=64 RW=8 grid=(64,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=64 len=432 stride=432 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "convS_wgrad_ring<3,3,1,3,{out},0> nwg=1024 RW=8 grid=(1024,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=1024 len=432 stride=432 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 64x64 16->16 k3 s2 same
    (64, 16, 16, 3, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,2,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,2,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,1,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,1,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,2,2,{out}> nwg=64 RW=8 grid=(64,1,1) lds=9504e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,2,2,{out}> nwg=1024 RW=8 grid=(1024,1,1) lds=9504e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 16x16 16->16 k3 s1 same
    (16, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=64 RW=4 grid=(64,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=1024 RW=4 grid=(1024,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 8x8 16->16 k3 s1 same up
    (8, 16, 16, 3, 1, "same", True): {
        "fwd": {
            "n=3": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd<16> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<16> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<4> nwg=16 R=8 lpw=432 grid=(16,4,1) lds=1728e class=-1 desc=given",
                "sum_partials ng=16 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<4> nwg=256 R=8 lpw=432 grid=(256,4,1) lds=1728e class=-1 desc=given",
                "sum_partials ng=256 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 32x32 16->16 k3 s1 same up
    (32, 16, 16, 3, 1, "same", True): {
        "fwd": {
            "n=3": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<4,4,2,0,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<4,4,2,0,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<2,2,1,1,{out}> nwg=16 RW=8 grid=(16,4,1) lds=2176e class=-1 desc=grid",
                "sum_partials ng=16 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<2,2,1,1,{out}> nwg=256 RW=8 grid=(256,4,1) lds=2176e class=-1 desc=grid",
                "sum_partials ng=256 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 64x64 16->3 k3 s1 same
    (64, 16, 3, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_thin_fwd<3,3,3> ntask=90 nseg=5 nrb=6 RW=12 grid=(23,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_thin_fwd<3,3,3> ntask=15000 nseg=5 nrb=6 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["convS_fwd_ring<3,3,1,3,1> ntask=72 nseg=4 nrb=6 RW=12 grid=(18,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["convS_fwd_ring<3,3,1,3,1> ntask=12000 nseg=4 nrb=6 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "convS_wgrad_ring<3,3,1,3,0,1> nwg=64 RW=8 grid=(64,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=64 len=432 stride=432 accumulate=0 bias=0",
            ],
            "nwg=1024": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "convS_wgrad_ring<3,3,1,3,0,1> nwg=1024 RW=8 grid=(1024,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=1024 len=432 stride=432 accumulate=0 bias=0",
            ],
        },
    },
    # 64x64 3->16 k2 s2 same
    (64, 3, 16, 2, 2, "same", False): {
        "fwd": {
            "n=3": ["convS_fwd_ring<2,2,2,3,1> ntask=18 nseg=2 nrb=3 RW=12 grid=(5,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["convS_fwd_ring<2,2,2,3,1> ntask=3000 nseg=2 nrb=3 RW=12 grid=(750,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,0> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "convS_wgrad_ring<2,2,2,3,{out},0> nwg=64 RW=8 grid=(64,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=64 len=192 stride=192 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "convS_wgrad_ring<2,2,2,3,{out},0> nwg=1024 RW=8 grid=(1024,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=1024 len=192 stride=192 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 32x32 16->16 k2 s2 same
    (32, 16, 16, 2, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<2,2,2,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<2,2,2,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<2,2,2,2,{out}> nwg=64 RW=4 grid=(64,1,1) lds=6144e class=-1 desc=grid",
                "sum_partials ng=64 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<2,2,2,2,{out}> nwg=1024 RW=4 grid=(1024,1,1) lds=6144e class=-1 desc=grid",
                "sum_partials ng=1024 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 28x28 1->8 k3 s2 valid
    (28, 1, 8, 3, 2, "valid", False): {
        "fwd": {
            "n=3": ["convS_fwd<3> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["convS_fwd<3> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": [
                "convS_fwd<8> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=0 desc=given",
                "convS_fwd<4> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=1 desc=given",
                "convS_fwd<4> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=2 desc=given",
                "convS_fwd<2> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "convS_fwd<8> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=0 desc=given",
                "convS_fwd<4> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=1 desc=given",
                "convS_fwd<4> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=2 desc=given",
                "convS_fwd<2> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "zero_part rows=64",
                "convS_wgrad<1,0> nwg=64 RW=4 grid=(64,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=64 len=72 stride=72 accumulate=0 bias=0",
                "sum_partials ng=64 len=8 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "zero_part rows=1024",
                "convS_wgrad<1,0> nwg=1024 RW=4 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=72 stride=72 accumulate=0 bias=0",
                "sum_partials ng=1024 len=8 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 8x8 8->8 k3 s1 valid up
    (8, 8, 8, 3, 1, "valid", True): {
        "fwd": {
            "n=3": [
                "convS_fwd<8> ntask=3 nseg=1 RW=2 grid=(3,1,1) lds=0 class=0 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=2 grid=(3,1,1) lds=0 class=1 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=2 grid=(3,1,1) lds=0 class=2 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=2 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "convS_fwd<8> ntask=500 nseg=1 RW=2 grid=(500,1,1) lds=0 class=0 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=2 grid=(500,1,1) lds=0 class=1 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=2 grid=(500,1,1) lds=0 class=2 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=2 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "bwd_data": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(1,1,3) lds=8168e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=500 grid=(1,1,500) lds=8168e class=-1 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "zero_part rows=64",
                "convS_wgrad<2,0> nwg=64 RW=2 grid=(64,1,1) lds=0 class=0 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=2 grid=(64,1,1) lds=0 class=1 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=2 grid=(64,1,1) lds=0 class=2 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=2 grid=(64,1,1) lds=0 class=3 desc=given",
                "sum_partials ng=64 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=256 len=8 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "zero_part rows=256",
                "convS_wgrad<2,0> nwg=256 RW=2 grid=(256,1,1) lds=0 class=0 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=2 grid=(256,1,1) lds=0 class=1 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=2 grid=(256,1,1) lds=0 class=2 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=2 grid=(256,1,1) lds=0 class=3 desc=given",
                "sum_partials ng=256 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=1024 len=8 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 14x14 8->1 k3 s1 same up
    (14, 8, 1, 3, 1, "same", True): {
        "fwd": {
            "n=3": [
                "convS_fwd<8> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=0 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=1 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=2 desc=given",
                "convS_fwd<8> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "convS_fwd<8> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=0 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=1 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=2 desc=given",
                "convS_fwd<8> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "bwd_data": {
            "n=3": ["convS_fwd<4> ntask=3 nseg=1 RW=4 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["convS_fwd<4> ntask=500 nseg=1 RW=4 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "zero_part rows=64",
                "convS_wgrad<2,0> nwg=64 RW=4 grid=(64,1,1) lds=0 class=0 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=4 grid=(64,1,1) lds=0 class=1 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=4 grid=(64,1,1) lds=0 class=2 desc=given",
                "convS_wgrad<2,0> nwg=64 RW=4 grid=(64,1,1) lds=0 class=3 desc=given",
                "sum_partials ng=64 len=128 stride=128 accumulate=0 bias=0",
                "sum_partials ng=256 len=1 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "zero_part rows=256",
                "convS_wgrad<2,0> nwg=256 RW=4 grid=(256,1,1) lds=0 class=0 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=4 grid=(256,1,1) lds=0 class=1 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=4 grid=(256,1,1) lds=0 class=2 desc=given",
                "convS_wgrad<2,0> nwg=256 RW=4 grid=(256,1,1) lds=0 class=3 desc=given",
                "sum_partials ng=256 len=128 stride=128 accumulate=0 bias=0",
                "sum_partials ng=1024 len=1 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 20x20 5->7 k3 s1 same
    (20, 5, 7, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(6,1,3) lds=2952e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=342 grid=(6,1,342) lds=2952e class=-1 desc=given"],
        },
        "bwd_data": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(6,1,3) lds=2952e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=342 grid=(6,1,342) lds=2952e class=-1 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "elu_bwd_colsum C=7 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=7 stride=7 accumulate=0 bias=1",
                "zero_part rows=64",
                "conv_taps_wgrad nwg=64 grid=(64,1,1) lds=5128e class=-1 desc=given",
                "sum_partials ng=64 len=315 stride=315 accumulate=0 bias=0",
            ],
            "nwg=1024": [
                "elu_bwd_colsum C=7 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=7 stride=7 accumulate=0 bias=1",
                "zero_part rows=1024",
                "conv_taps_wgrad nwg=1024 grid=(1024,1,1) lds=5128e class=-1 desc=given",
                "sum_partials ng=1024 len=315 stride=315 accumulate=0 bias=0",
            ],
        },
    },
    # 20x20 16->16 k3 s1 same
    (20, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,0> strips=1 RW=5 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,0> strips=1 RW=5 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,0> strips=1 RW=5 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,0> strips=1 RW=5 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_roll<9,1> nwg=64 RW=5 lpw=864 grid=(64,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_roll<9,1> nwg=1024 RW=5 lpw=864 grid=(1024,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 37x37 16->5 k3 s1 valid
    (37, 16, 5, 3, 1, "valid", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,0> strips=2 RW=8 nseg=3 ntask=18 grid=(18,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,0> strips=2 RW=8 nseg=3 ntask=3000 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(15,1,3) lds=2952e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=137 grid=(15,1,137) lds=2952e class=-1 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_roll<9,1> nwg=64 RW=8 lpw=864 grid=(64,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=64 len=720 stride=720 accumulate=0 bias=0",
                "sum_partials ng=64 len=5 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_roll<9,1> nwg=1024 RW=8 lpw=864 grid=(1024,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=1024 len=720 stride=720 accumulate=0 bias=0",
                "sum_partials ng=1024 len=5 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 22x22 16->9 k3 s2 same
    (22, 16, 9, 3, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd<9> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<9> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(2,1,3) lds=3870e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=500 grid=(2,1,500) lds=3870e class=-1 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<9> nwg=64 R=12 lpw=1656 grid=(64,1,1) lds=6624e class=-1 desc=given",
                "sum_partials ng=64 len=1296 stride=1296 accumulate=0 bias=0",
                "sum_partials ng=64 len=9 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<9> nwg=1024 R=12 lpw=1656 grid=(1024,1,1) lds=6624e class=-1 desc=given",
                "sum_partials ng=1024 len=1296 stride=1296 accumulate=0 bias=0",
                "sum_partials ng=1024 len=9 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 10x10 16->16 k3 s1 valid up
    (10, 16, 16, 3, 1, "valid", True): {
        "fwd": {
            "n=3": [
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd<16> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<16> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<4> nwg=16 R=12 lpw=320 grid=(16,4,1) lds=1280e class=-1 desc=given",
                "sum_partials ng=16 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<4> nwg=256 R=12 lpw=320 grid=(256,4,1) lds=1280e class=-1 desc=given",
                "sum_partials ng=256 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 6x6 16->16 k3 s1 same
    (6, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<9> nwg=64 R=8 lpw=512 grid=(64,1,1) lds=2048e class=-1 desc=given",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<9> nwg=1024 R=8 lpw=512 grid=(1024,1,1) lds=2048e class=-1 desc=given",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 5x5 16->7 k3 s1 same up
    (5, 16, 7, 3, 1, "same", True): {
        "fwd": {
            "n=3": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "bwd_data": {
            "n=3": ["conv_taps_fwd<0,0> nchunk=3 grid=(1,1,3) lds=8168e class=-1 desc=given"],
            "n=500": ["conv_taps_fwd<0,0> nchunk=500 grid=(1,1,500) lds=8168e class=-1 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<4> nwg=16 R=8 lpw=384 grid=(16,4,1) lds=1536e class=-1 desc=given",
                "sum_partials ng=16 len=1792 stride=1792 accumulate=0 bias=0",
                "sum_partials ng=64 len=7 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<4> nwg=256 R=8 lpw=384 grid=(256,4,1) lds=1536e class=-1 desc=given",
                "sum_partials ng=256 len=1792 stride=1792 accumulate=0 bias=0",
                "sum_partials ng=1024 len=7 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 18x18 16->11 k2 s2 same
    (18, 16, 11, 2, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd<4> strips=1 R=12 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<4> strips=1 R=12 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": [
                "convS_fwd<3> ntask=3 nseg=1 RW=3 grid=(3,1,1) lds=0 class=0 desc=given",
                "convS_fwd<3> ntask=3 nseg=1 RW=3 grid=(3,1,1) lds=0 class=1 desc=given",
                "convS_fwd<3> ntask=3 nseg=1 RW=3 grid=(3,1,1) lds=0 class=2 desc=given",
                "convS_fwd<3> ntask=3 nseg=1 RW=3 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "convS_fwd<3> ntask=500 nseg=1 RW=3 grid=(500,1,1) lds=0 class=0 desc=given",
                "convS_fwd<3> ntask=500 nseg=1 RW=3 grid=(500,1,1) lds=0 class=1 desc=given",
                "convS_fwd<3> ntask=500 nseg=1 RW=3 grid=(500,1,1) lds=0 class=2 desc=given",
                "convS_fwd<3> ntask=500 nseg=1 RW=3 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<4> nwg=64 R=12 lpw=864 grid=(64,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=64 len=704 stride=704 accumulate=0 bias=0",
                "sum_partials ng=64 len=11 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<4> nwg=1024 R=12 lpw=864 grid=(1024,1,1) lds=3456e class=-1 desc=given",
                "sum_partials ng=1024 len=704 stride=704 accumulate=0 bias=0",
                "sum_partials ng=1024 len=11 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 48x48 16->16 k3 s1 same
    (48, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=3 ntask=18 grid=(18,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=3 ntask=3000 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=3 ntask=18 grid=(18,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=3 ntask=3000 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=64 RW=8 grid=(64,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=1024 RW=8 grid=(1024,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 20x20 16->3 k3 s1 same
    (20, 16, 3, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_thin_fwd<3,3,3> ntask=12 nseg=2 nrb=2 RW=12 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_thin_fwd<3,3,3> ntask=2000 nseg=2 nrb=2 RW=12 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["convS_fwd<7> ntask=6 nseg=2 RW=5 grid=(6,1,1) lds=0 class=0 desc=given"],
            "n=500": ["convS_fwd<7> ntask=1000 nseg=2 RW=5 grid=(1000,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "zero_part rows=64",
                "convS_wgrad<2,1> nwg=64 RW=5 grid=(64,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=64 len=432 stride=432 accumulate=0 bias=0",
            ],
            "nwg=1024": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "zero_part rows=1024",
                "convS_wgrad<2,1> nwg=1024 RW=5 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=432 stride=432 accumulate=0 bias=0",
            ],
        },
    },
    # 37x37 16->3 k3 s1 valid
    (37, 16, 3, 3, 1, "valid", False): {
        "fwd": {
            "n=3": ["conv16_thin_fwd<3,3,3> ntask=27 nseg=3 nrb=3 RW=12 grid=(7,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_thin_fwd<3,3,3> ntask=4500 nseg=3 nrb=3 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["convS_fwd<7> ntask=18 nseg=3 RW=8 grid=(18,1,1) lds=0 class=0 desc=given"],
            "n=500": ["convS_fwd<7> ntask=3000 nseg=3 RW=8 grid=(2048,1,1) lds=0 class=0 desc=given"],
        },
        "wgrad": {
            "nwg=64": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "zero_part rows=64",
                "convS_wgrad<2,1> nwg=64 RW=8 grid=(64,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=64 len=432 stride=432 accumulate=0 bias=0",
            ],
            "nwg=1024": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "zero_part rows=1024",
                "convS_wgrad<2,1> nwg=1024 RW=8 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=432 stride=432 accumulate=0 bias=0",
            ],
        },
    },
    # 32x32 16->3 k3 s1 same
    (32, 16, 3, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_thin_fwd<3,3,3> ntask=27 nseg=3 nrb=3 RW=12 grid=(7,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_thin_fwd<3,3,3> ntask=4500 nseg=3 nrb=3 RW=12 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["convS_fwd_ring<3,3,1,3,1> ntask=18 nseg=2 nrb=3 RW=12 grid=(5,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["convS_fwd_ring<3,3,1,3,1> ntask=3000 nseg=2 nrb=3 RW=12 grid=(750,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "convS_wgrad_ring<3,3,1,3,0,1> nwg=64 RW=8 grid=(64,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=64 len=432 stride=432 accumulate=0 bias=0",
            ],
            "nwg=1024": [
                "elu_bwd_colsum C=3 grid=(1024,1,1) lds=0 class=0 desc=given",
                "sum_partials ng=1024 len=3 stride=3 accumulate=0 bias=1",
                "convS_wgrad_ring<3,3,1,3,0,1> nwg=1024 RW=8 grid=(1024,1,1) lds=0 class=0 desc=grid",
                "sum_partials ng=1024 len=432 stride=432 accumulate=0 bias=0",
            ],
        },
    },
    # 32x32 16->16 k3 s1 same
    (32, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=8 nseg=2 ntask=6 grid=(6,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=1 RW=8 nseg=2 ntask=1000 grid=(1000,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=64 RW=8 grid=(64,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=1024 RW=8 grid=(1024,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 32x32 16->16 k3 s2 same
    (32, 16, 16, 3, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,2,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,2,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<1,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<1,1,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,2,2,{out}> nwg=64 RW=4 grid=(64,1,1) lds=9504e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,2,2,{out}> nwg=1024 RW=4 grid=(1024,1,1) lds=9504e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 16x16 16->16 k3 s2 same
    (16, 16, 16, 3, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<9> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<2> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<2> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<2> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<2> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<9> nwg=64 R=8 lpw=2040 grid=(64,1,1) lds=8160e class=-1 desc=given",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<9> nwg=1024 R=8 lpw=2040 grid=(1024,1,1) lds=8160e class=-1 desc=given",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 16x16 16->16 k3 s1 same up
    (16, 16, 16, 3, 1, "same", True): {
        "fwd": {
            "n=3": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=3 desc=grid",
            ],
            "n=500": [
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=1 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=2 desc=grid",
                "conv16_fwd_roll<2,2,1,1,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=3 desc=grid",
            ],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<4,4,2,0,1> strips=1 RW=4 nseg=1 ntask=3 grid=(3,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<4,4,2,0,1> strips=1 RW=4 nseg=1 ntask=500 grid=(500,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<2,2,1,1,{out}> nwg=16 RW=4 grid=(16,4,1) lds=2176e class=-1 desc=grid",
                "sum_partials ng=16 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<2,2,1,1,{out}> nwg=256 RW=4 grid=(256,4,1) lds=2176e class=-1 desc=grid",
                "sum_partials ng=256 len=4096 stride=4096 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 64x64 16->16 k3 s1 same
    (64, 16, 16, 3, 1, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=4 ntask=24 grid=(24,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=4 ntask=4000 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "bwd_data": {
            "n=3": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=4 ntask=24 grid=(24,1,1) lds=0 class=0 desc=grid"],
            "n=500": ["conv16_fwd_roll<3,3,1,1,1> strips=2 RW=8 nseg=4 ntask=4000 grid=(1024,1,1) lds=0 class=0 desc=grid"],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=64 RW=8 grid=(64,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=64 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad_grid<3,3,1,1,{out}> nwg=1024 RW=8 grid=(1024,1,1) lds=3456e class=-1 desc=grid",
                "sum_partials ng=1024 len=2304 stride=2304 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
    # 16x16 16->16 k2 s2 same
    (16, 16, 16, 2, 2, "same", False): {
        "fwd": {
            "n=3": ["conv16_fwd<4> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given"],
            "n=500": ["conv16_fwd<4> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given"],
        },
        "bwd_data": {
            "n=3": [
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(3,1,1) lds=0 class=3 desc=given",
            ],
            "n=500": [
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=0 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=1 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=2 desc=given",
                "conv16_fwd<1> strips=1 R=8 nseg=1 grid=(500,1,1) lds=0 class=3 desc=given",
            ],
        },
        "wgrad": {
            "nwg=64": [
                "conv16_wgrad<4> nwg=64 R=8 lpw=1536 grid=(64,1,1) lds=6144e class=-1 desc=given",
                "sum_partials ng=64 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=64 len=16 stride=16 accumulate=0 bias=1",
            ],
            "nwg=1024": [
                "conv16_wgrad<4> nwg=1024 R=8 lpw=1536 grid=(1024,1,1) lds=6144e class=-1 desc=given",
                "sum_partials ng=1024 len=1024 stride=1024 accumulate=0 bias=0",
                "sum_partials ng=1024 len=16 stride=16 accumulate=0 bias=1",
            ],
        },
    },
}
