"""Batched staging in the encoder / decoder kernels (stage_issue / stage_copy / stage_commit, vae_dev.hpp): the loads of a staging
group are issued together and stored afterwards.  Only loads move, so every result must be bit-equal to what the code computed before
the change.  The fixtures tests/golden/stage_batched_<b>_<m>_<L>.npz were recorded on an MI355X from the build of the parent commit
3aa483ba ("Casale GP-VAE: stage, step and row kernels tested across their shapes") by tools/make_stage_batched_golden.py, which refuses
to run on any other commit; they hold theta, the state vector, every gradient and the scalars after three Adam steps.

Shapes (b, m, L): (1, 12, 1) one workgroup, every run-time count below or just above one pass of 512 threads; (7, 12, 3) small b,
odd L; (300, 24, 5) and (257, 32, 16) workgroups walk two images (prefetch registers, LDS reuse), the run-time-m and the m = 32
instances; (20, 40, 64) the largest L -- the chunk loop runs more than one chunk with a partial last one -- and the form without riders.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(1, 12, 1), (7, 12, 3), (300, 24, 5), (257, 32, 16), (20, 40, 64)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_path(b, m, L):
    return os.path.join(GOLDEN, f"stage_batched_{b}_{m}_{L}.npz")


def bound_engine(b, m, L, seed=31):
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=seed)
    eng = H.engine_for(params, b, geco=True, N_train=400.0)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    return eng


def three_steps(b, m, L, graph=False):
    """Three Adam steps (explicit eps) -> (engine, dict of float64 arrays: theta, state, grad_<name>, and the scalars as sc_<name>)."""
    eng = bound_engine(b, m, L)
    if graph:
        eng.capture("step", adam=True)          # capture does not execute
    for _ in range(3):
        if graph:
            eng.replay("step")
        else:
            eng.run(adam=True)
    eng.synchronize()
    out = dict(theta=eng.theta.cpu().numpy().copy(), state=eng.state.cpu().numpy().copy())
    for k, v in eng.grads().items():
        out["grad_" + k] = v.cpu().numpy().copy()
    for k, v in eng.scalars().items():
        out["sc_" + k] = np.float64(v)
    return eng, out


def _assert_handoffs_clean(eng):
    fl = eng.ws_view("flags", (64,)).view(torch.int64)
    assert torch.count_nonzero(fl) == 0, fl.tolist()
    eng.scalars()                      # raises SvgpError("... hand-off ...") if a consumer gave up waiting


def _assert_golden(got, b, m, L):
    want = np.load(golden_path(b, m, L))
    assert set(want.files) == set(got), sorted(set(want.files) ^ set(got))
    for k in want.files:
        if k.startswith("sc_"):
            assert float(got[k]) == float(want[k]), (k, float(got[k]), float(want[k]))
        else:
            assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), k


@pytest.mark.parametrize("b,m,L", SHAPES)
def test_three_steps_equal_the_parent_build(b, m, L):
    """(a) golden steps, eager; (c) the hand-off counters are re-armed and no hand-off timed out."""
    eng, got = three_steps(b, m, L)
    _assert_golden(got, b, m, L)
    _assert_handoffs_clean(eng)


def test_three_replayed_steps_equal_the_parent_build():
    eng, got = three_steps(257, 32, 16, graph=True)
    _assert_golden(got, 257, 32, 16)
    _assert_handoffs_clean(eng)


@pytest.mark.parametrize("b,m,L", SHAPES)
def test_phase_entry_points_reproduce_the_step(b, m, L):
    """(b) every stand-alone entry point that runs a changed kernel, on the workspace one step (no Adam: theta stays) left behind:
    its outputs, filled with NaN first, must come back finite and equal to the step's."""
    from svgp_vae_amd import _lib
    eng = bound_engine(b, m, L)
    state0 = eng.state.clone()
    eng.run(adam=False)
    eng.synchronize()
    eng.state.copy_(state0)            # the step closes with the GECO update of the multiplier, which the decoder's reverse pass reads
    torch.cuda.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, aux, ep = (t.data_ptr() for t in eng._bound)
    s = eng.stream.cuda_stream
    n_part, n_enc = int(eng.wl.n_part), int(eng.pl.n_enc)
    enc_fwd = dict(enc_a1=(b, 1352), enc_a2=(b, 288), enc_a3=(b, 32), qnet_mu=(b, L), qnet_var_raw=(b, L), qnet_var=(b, L))
    enc_bwd = dict(part_enc=(n_part, n_enc))
    dec_fwd = dict(dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784))
    dec_bwd = dict(dec_d2=(b, 1568), dec_d1=(b, 512), dec_dh0=(b, 128), zbar=(b, L))
    sq = lambda: eng.ws_view("part_sums", (n_part, 4))[:, 2]
    step = {k: eng.ws_view(k, sh).clone() for d in (enc_fwd, enc_bwd, dec_fwd, dec_bwd) for k, sh in d.items()}
    step["sq"] = sq().clone()

    def check(label, outs, with_sq, *calls):
        for k, sh in outs.items():
            eng.ws_view(k, sh).fill_(float("nan"))
        if with_sq:
            sq().fill_(float("nan"))
        for sym, args in calls:
            _lib.call(sym, *args)
        eng.synchronize()
        for k, sh in outs.items():
            v = eng.ws_view(k, sh)
            assert torch.isfinite(v).all(), (label, k)
            assert torch.equal(v, step[k]), (label, k)
        if with_sq:
            assert torch.isfinite(sq()).all(), label
            assert torch.equal(sq(), step["sq"]), label

    check("encoder_fwd", enc_fwd, False, ("svgp_mnist_encoder_fwd", (cfg, th, img, ws, s)))
    check("encoder_bwd", enc_bwd, False, ("svgp_mnist_encoder_bwd", (cfg, th, img, ws, s)))
    check("encoder_bwd_km_sum", enc_bwd, False, ("svgp_mnist_encoder_bwd_km_sum", (cfg, th, img, aux, ws, st, s)))
    _assert_handoffs_clean(eng)
    check("decoder_fwd_pre", dec_fwd, True, ("svgp_mnist_decoder_fwd_pre", (cfg, th, img, ws, s)))
    check("decoder_bwd_data_pre", dec_bwd, False, ("svgp_mnist_decoder_bwd_data_pre", (cfg, th, img, ws, st, s)))
    both = dict(dec_fwd, **dec_bwd)
    check("decoder_fwd_bwd_data_pre", both, True, ("svgp_mnist_decoder_fwd_bwd_data_pre", (cfg, th, img, ws, st, s)))
    if m <= 32:
        # the riders of the _aji form finish (A_hat + jI)^-1 and the KL terms: re-open them first (tests/test_gpu_decoder_fused.py)
        check("decoder_fwd_bwd_data_pre_aji", both, True,
              ("svgp_gp_factor_fwd_defer_aji", (cfg, ws, s)), ("svgp_gp_posterior_fwd", (cfg, ep, ws, st, s)),
              ("svgp_mnist_decoder_fwd_bwd_data_pre_aji", (cfg, th, img, ws, st, s)))
    _assert_handoffs_clean(eng)
