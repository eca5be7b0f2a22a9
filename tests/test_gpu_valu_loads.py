"""Branch-free operand loads in the decoder's VALU convolution forms (tap_operands, vae_dev.hpp: kept in the rolled forward, tried in
the others) and one staging round trip per image in the decoder's weight-gradient riders (decoder_wgrad_rider): only loads move --
every FMA and every reduction keeps its order -- so every result must be bit-equal to what the code computed before.  The fixtures
tests/golden/valu_loads_<b>_<m>_<L>.npz were recorded on an MI355X from the build of the parent commit 7f754c3 ("Moving ball: one step body for the four engines, one parameter setup") by
tools/make_valu_loads_golden.py, which refuses to record from any other tree.

Shapes (b, m, L): (1, 32, 16) and (2, 16, 8) the smallest -- every image touches all four borders of every layer, so the select of
a tap outside the tile is always exercised; L = 8 the latent-width guards; (257, 32, 16) workgroup 0 and rider slot 0 walk a second
image (prefetch, one-image-ahead staging); (5, 72, 16) the m > 64 route: the stand-alone kernels with the unrolled forward and
UpC2's VALU weight gradient outside the merged launches.

A fixture holds one Adam step (theta, state, gradients, scalars) and, per stand-alone entry point, its outputs on the workspace a
step without Adam left behind.  Arrays of more than WHOLE elements are kept as a fingerprint of two rows, which keeps the files
small: the wrap-around int64 sum of their bit patterns over the batch axis, and the same sum with row r weighted by 2 r + 1.  One
changed element changes both; changes d0, d1 in two rows r0, r1 of a column that cancel in the first sum cancel in the second only
if 2 (r1 - r0) d1 = 0 mod 2^64, i.e. d1 a multiple of 2^55 at the 257 rows used here: a sign / exponent flip of equal size in both.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 16), (2, 16, 8), (257, 32, 16), (5, 72, 16)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHOLE = 2048
RIDER_LAYOUTS = [(256, 1), (256, 2), (256, 3), (512, 1), (512, 3)]      # (threads, n_types) of svgp_mnist_decoder_bwd_weights
NAN = float("nan")


def golden_path(b, m, L):
    return os.path.join(GOLDEN, f"valu_loads_{b}_{m}_{L}.npz")


def bound_engine(b, m, L, seed=47):
    # m > 64: 16 auxiliary features and jitter 1e-4, as the other m = 72 tests (tests/test_gpu_parity.py): with 4 features the linear
    # kernel leaves K_mm of rank <= 5 and the 1e-6 jitter does not carry its Cholesky factor at m = 72 -- every scalar is NaN in
    # any build, which compares nothing
    big = m > 64
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=16 if big else 4, n_obj=30 if big else 20, seed=seed)
    eng = H.engine_for(params, b, geco=True, N_train=400.0, jitter=1e-4 if big else 1e-6)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    return eng


def _keep(v):
    """float64 device tensor -> numpy: the array itself, or (more than WHOLE elements) its two bit-pattern sums over axis 0."""
    v = v.contiguous()
    if v.numel() <= WHOLE:
        return v.cpu().numpy().copy()
    bits = v.view(torch.int64).reshape(v.shape[0], -1)
    w = 2 * torch.arange(v.shape[0], dtype=torch.int64, device=v.device)[:, None] + 1
    return torch.stack([bits.sum(0), (bits * w).sum(0)]).cpu().numpy().copy()


def one_step(b, m, L):
    """One Adam step -> dict: theta, state, grad_<name>, sc_<name>."""
    eng = bound_engine(b, m, L)
    eng.run(adam=True)
    eng.synchronize()
    out = dict(theta=eng.theta.cpu().numpy().copy(), state=eng.state.cpu().numpy().copy())
    for k, v in eng.grads().items():
        out["grad_" + k] = v.cpu().numpy().copy()
    for k, v in eng.scalars().items():
        out["sc_" + k] = np.float64(v)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


def entry_points(b, m, L):
    """Every stand-alone entry point that runs a rewritten form, on the workspace one step without Adam left behind; its outputs are
    filled with NaN first.  -> dict '<form>.<array>' -> array or fingerprint."""
    from svgp_vae_amd import _lib
    eng = bound_engine(b, m, L)
    state0 = eng.state.clone()
    eng.run(adam=False)
    eng.synchronize()
    eng.state.copy_(state0)            # the step closes with the GECO update of the multiplier, which the decoder's reverse pass reads
    torch.cuda.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, ep = eng._bound[0].data_ptr(), eng._bound[2].data_ptr()
    s = eng.stream.cuda_stream
    n_part, n_dec = int(eng.wl.n_part), int(eng.pl.n_vae - eng.pl.n_enc)
    dec_fwd = dict(dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784))
    dec_bwd = dict(dec_d2=(b, 1568), dec_d1=(b, 512), dec_dh0=(b, 128), zbar=(b, L))
    both = dict(dec_fwd, **dec_bwd)
    wgrad = dict(part_dec=(n_part, n_dec))
    sq = lambda: eng.ws_view("part_sums", (n_part, 4))[:, 2]
    out = {}

    def form(label, outs, with_sq, *calls):
        for k, sh in outs.items():
            eng.ws_view(k, sh).fill_(NAN)
        if with_sq:
            sq().fill_(NAN)
        torch.cuda.synchronize()
        for sym, args in calls:
            _lib.call(sym, *args)
        eng.synchronize()
        for k, sh in outs.items():
            v = eng.ws_view(k, sh)
            assert torch.isfinite(v).all(), (label, k)
            out[f"{label}.{k}"] = _keep(v)
        if with_sq:
            assert torch.isfinite(sq()).all(), label
            out[f"{label}.sq"] = _keep(sq())

    if m <= 64:
        form("decoder_fwd_pre", dec_fwd, True, ("svgp_mnist_decoder_fwd_pre", (cfg, th, img, ws, s)))
        form("decoder_bwd_data_pre", dec_bwd, False, ("svgp_mnist_decoder_bwd_data_pre", (cfg, th, img, ws, st, s)))
        form("decoder_fwd_bwd_data_pre", both, True, ("svgp_mnist_decoder_fwd_bwd_data_pre", (cfg, th, img, ws, st, s)))
    if m <= 32:
        # the riders of the _aji form finish (A_hat + jI)^-1 and the KL terms, those of the _tail form the whole tail of the forward
        # factor stage: re-open them first (tests/test_gpu_decoder_fused.py, tests/test_gpu_fwd_split.py)
        form("decoder_fwd_bwd_data_pre_aji", both, True,
             ("svgp_gp_factor_fwd_defer_aji", (cfg, ws, s)), ("svgp_gp_posterior_fwd", (cfg, ep, ws, st, s)),
             ("svgp_mnist_decoder_fwd_bwd_data_pre_aji", (cfg, th, img, ws, st, s)))
        form("decoder_fwd_bwd_data_pre_tail", both, True,
             ("svgp_gp_factor_fwd_head", (cfg, ws, s)), ("svgp_gp_posterior_fwd_z", (cfg, ep, ws, st, s)),
             ("svgp_mnist_decoder_fwd_bwd_data_pre_tail", (cfg, th, img, ws, st, s)))
    if m <= 64:
        form("gp_stats_factor_bwd_wgrad", wgrad, False, ("svgp_gp_stats_factor_bwd_wgrad", (cfg, img, ws, st, s)))
        fl = eng.ws_view("flags", (64,)).view(torch.int64)
        assert torch.count_nonzero(fl) == 0, fl.tolist()
    form("decoder_fwd", dec_fwd, True, ("svgp_mnist_decoder_fwd", (cfg, th, img, ws, s)))
    form("decoder_bwd_data", dec_bwd, False, ("svgp_mnist_decoder_bwd_data", (cfg, th, img, ws, st, s)))
    for threads, n_types in RIDER_LAYOUTS:
        form(f"decoder_bwd_weights_{threads}x{n_types}", wgrad, False,
             ("svgp_mnist_decoder_bwd_weights", (cfg, img, ws, st, threads, n_types, s)))
    form("decoder_bwd", dict(wgrad, zbar=(b, L)), False, ("svgp_mnist_decoder_bwd", (cfg, th, img, ws, st, s)))
    eng.scalars()                      # raises if a hand-off timed out
    return out


def record(b, m, L):
    return dict(one_step(b, m, L), **entry_points(b, m, L))


_golden = {}


def _want(b, m, L):
    if (b, m, L) not in _golden:
        with np.load(golden_path(b, m, L)) as z:
            _golden[(b, m, L)] = {k: z[k] for k in z.files}
    return _golden[(b, m, L)]


def _assert_equal(got, want, keys):
    assert keys, "nothing to compare"
    for k in keys:
        if k.startswith("sc_"):
            assert float(got[k]) == float(want[k]), (k, float(got[k]), float(want[k]))
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), k


@pytest.mark.parametrize("b,m,L", SHAPES)
def test_one_step_equals_the_parent_build(b, m, L):
    got, want = one_step(b, m, L), _want(b, m, L)
    step_keys = sorted(k for k in want if "." not in k)
    assert step_keys == sorted(got), sorted(set(step_keys) ^ set(got))
    _assert_equal(got, want, step_keys)


@pytest.mark.parametrize("b,m,L", SHAPES)
def test_entry_points_equal_the_parent_build(b, m, L):
    """The stand-alone decoder launches (plain, `_pre`, fused `_pre`, `_pre_aji`, `_pre_tail`), the reverse factor launch with its
    riders, the one-kernel reverse pass and every rider layout of svgp_mnist_decoder_bwd_weights."""
    got, want = entry_points(b, m, L), _want(b, m, L)
    ep_keys = sorted(k for k in want if "." in k)
    assert ep_keys == sorted(got), sorted(set(ep_keys) ^ set(got))
    forms = {k.split(".")[0] for k in ep_keys}
    assert {"decoder_fwd", "decoder_bwd", "decoder_bwd_weights_256x1", "decoder_bwd_weights_256x2", "decoder_bwd_weights_256x3"} <= forms
    if m <= 32:
        assert {"decoder_fwd_bwd_data_pre", "decoder_fwd_bwd_data_pre_aji", "decoder_fwd_bwd_data_pre_tail",
                "gp_stats_factor_bwd_wgrad"} <= forms
    _assert_equal(got, want, ep_keys)
