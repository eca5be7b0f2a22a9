"""The two moving-ball engines over the shape range they accept, against the float64 oracle (oracle/ball_oracle.py), at the
shapes where their kernels change form.  Case tables, problems and tolerances: tests/ball_cases.py; that the oracle itself is
well conditioned at every case: tests/test_ball_envelope_oracle_cpu.py.

Sparse step (BallStepEngine; 1 <= m <= 64, 1 <= batch <= 64, any tmax): the shared GP stage kernels with kl_form = 1,
clip_pv = 2, M = 1, n_obj = 0, rows = frames, channels = videos -- a configuration nothing else uses.  kl_form has its own
branches in the forward and reverse factor kernels (gp_kernels.hip: never the five-matrix form, so m = 31 must take the
four-matrix one; m == 32 its own instance; m = 64 the LDS limit), batch = 64 is the largest channel count, tmax >= 128 takes four
statistics partitions, tmax = 257 is one row past SVGP_MAX_PART and runs the 64-thread frame loop of k_ball_assemble five times.

Exact GP (PearceStepEngine; tmax <= 64): k_pearce_fwd / k_pearce_bwd <32> for n <= 32 and <64> (RL = 4, RMAX = 16, its own
Gauss-Jordan sweep, more than 64 KB of dynamic LDS: 101 KB forward and 135 808 bytes reverse at n = 64) above; the NP ELBO runs a
second, context-set GP whose reverse pass accumulates into the first one's gradients.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ball_oracle as BO
from oracle import pearce_vae_oracle as PO
from tests import ball_cases as BC
from tests import helpers as H
from tests.ball_cases import DT, _engine, _pearce_engine, _problem

pytestmark = pytest.mark.gpu

SPARSE_NAMES = ("elbo", "recon", "KL_term", "inside_elbo", "ce_term", "full_p_mu", "full_p_var", "qnet_mu", "qnet_var",
                "pred_vid", "l_x", "l_y", "inside_recon", "inside_kl", "ip_x", "ip_y", "cov_mean_x", "cov_mean_y")
PEARCE_NAMES = ("elbo", "recon", "prior_kl", "full_p_mu", "full_p_var", "qnet_mu", "qnet_var", "pred_vid")


@pytest.mark.parametrize("case", list(BC.SPARSE_CASES))
def test_sparse_step_matches_oracle_across_the_shape_range(case):
    cs = BC.SPARSE_CASES[case]
    batch, T, m = cs["batch"], cs["tmax"], cs["m"]
    p, vid, eps, out, grads = BC.sparse_reference(case)
    eng = _engine(p, batch, T, BC.ENV_PX, BC.ENV_HIDDEN, m, titsias=cs["titsias"], jitter=BC.SPARSE_JITTER, clip_qs=True,
                  beta=BC.SPARSE_BETA)
    assert eng.wl.stat_parts == (4 if T >= 128 else 1)
    eng.step(vid.cuda(), eps.cuda(), adam=False)
    got = eng.outputs()
    bad = []
    for i, n in enumerate(SPARSE_NAMES):
        want = out[i] if torch.is_tensor(out[i]) else torch.tensor(float(out[i]), dtype=DT)
        if n == "inside_kl" and cs["titsias"]:
            want = torch.zeros(batch, dtype=DT)
        e = H.relerr(got[i], want)
        print(f"{case} {n}: {e:.2e}")
        if not e < BC.OUT_TOL:
            bad.append(f"{n}: {e:.2e}")
    sc = eng.scalars()
    mean_elbo = float(out[0].mean())
    print(f"{case} mean elbo: {abs(sc['elbo'] - mean_elbo) / abs(mean_elbo):.2e}")
    if not abs(sc["elbo"] - mean_elbo) <= BC.ELBO_TOL * abs(mean_elbo):
        bad.append(f"mean elbo {sc['elbo']} vs {mean_elbo}")
    eng.stream.synchronize()
    for k in BO.PARAM_ORDER:
        e = H.relerr(eng.grads[k].reshape(-1), grads[k].reshape(-1))
        print(f"{case} grad {k}: {e:.2e}")
        if not e < BC.GRAD_TOL:
            bad.append(f"grad {k}: {e:.2e}")
    assert not bad, "\n".join(bad)


def test_three_adam_steps_at_the_largest_shape_follow_the_oracle_trajectory():
    cs = BC.SPARSE_CASES["m64_B64"]
    batch, T, m, px, hidden = cs["batch"], cs["tmax"], cs["m"], BC.ENV_PX, BC.ENV_HIDDEN
    p, _, _ = _problem(batch, T, px, hidden, m, seed=5, lt=cs["lt"])
    g = torch.Generator().manual_seed(11)
    vids = [PO.make_video_batch(tmax=T, px=px, py=px, lt=cs["lt"], batch=batch, r=2, generator=g, dtype=DT) for _ in range(3)]
    epss = [torch.randn(batch, T, 2, dtype=DT, generator=g) for _ in range(3)]
    want, elbos = BO.train_trajectory(p, vids, epss, beta=1.0, titsias=False, jitter=1e-6, clipping_qs=True, lr=1e-3,
                                      clip_grad=True, train_ip=True, train_gp=False)
    eng = _engine(p, batch, T, px, hidden, m, titsias=False, jitter=1e-6, clip_qs=True, beta=1.0, fixed_gp=True,
                  clip_grad=True, lr=1e-3)
    got_elbo = []
    for v, e in zip(vids, epss):
        eng.step(v.cuda(), e.cuda(), adam=True)
        got_elbo.append(eng.scalars()["elbo"])
    print("elbo trajectory:", got_elbo, elbos)
    assert np.allclose(got_elbo, elbos, rtol=BC.TRAJ_ELBO_RTOL)
    assert eng.scalars()["adam_t"] == 3.0
    for k in BO.PARAM_ORDER:
        e = H.relerr(eng.params[k].reshape(-1), want[k].reshape(-1))
        print(f"param {k}: {e:.2e}")
        assert e < BC.TRAJ_PARAM_TOL, k
    assert float(eng.params["l_x"][0]) == float(p["l_x"]) and float(eng.params["l_y"][0]) == float(p["l_y"])


def test_sparse_engine_limits_are_enforced():
    from svgp_vae_amd import _lib, ball
    mk = lambda n, m: ball.SVGP(False, m, False, 1, 64, 2.0, False, n, 1e-6, 1, 64, 2.0)
    kw = dict(tmax=64, px=8, py=8, hidden=8)
    with pytest.raises(_lib.SvgpError):
        ball.BallStepEngine(mk("x", 65), mk("y", 65), batch=64, **kw)
    with pytest.raises(_lib.SvgpError):
        ball.BallStepEngine(mk("x", 64), mk("y", 64), batch=65, **kw)
    eng = ball.BallStepEngine(mk("x", 64), mk("y", 64), batch=64, **kw)
    assert (eng.m, eng.B, eng.cfg.L, eng.cfg.b) == (64, 64, 64, 64)


# ---------------------------------------------------------------------------------------------------------
# exact per-video GP
# ---------------------------------------------------------------------------------------------------------
def _pearce_step(case):
    cs = BC.PEARCE_ENV_CASES[case]
    p, vid, eps, ran_ind, out, grads = BC.pearce_reference(case)
    eng = _pearce_engine(p, cs["type_elbo"], cs["lt"], cs["joint"], cs["batch"], cs["tmax"], BC.ENV_PX, BC.ENV_HIDDEN,
                         BC.PEARCE_BETA)
    eng.step(vid.cuda(), eps.cuda(), adam=False, ran_ind=None if ran_ind is None else ran_ind.numpy(), con_tf=cs["con_tf"])
    return cs, eng, out, grads


@pytest.mark.parametrize("case", list(BC.PEARCE_ENV_CASES))
def test_pearce_step_matches_oracle_across_the_shape_range(case):
    cs, eng, out, grads = _pearce_step(case)
    got = eng.outputs()
    bad = []
    for i, n in enumerate(PEARCE_NAMES):
        e = H.relerr(got[i], out[i])
        print(f"{case} {n}: {e:.2e}")
        if not e < BC.OUT_TOL:
            bad.append(f"{n}: {e:.2e}")
    mean_elbo = float(out[0].mean())
    print(f"{case} mean elbo: {abs(eng.scalars()['elbo'] - mean_elbo) / abs(mean_elbo):.2e}")
    if not abs(eng.scalars()["elbo"] - mean_elbo) <= BC.ELBO_TOL * abs(mean_elbo):
        bad.append("mean elbo")
    eng.stream.synchronize()
    for k in BO.PEARCE_PARAM_ORDER:
        if k.startswith("l_") and not cs["joint"]:
            assert float(eng.grads[k].abs().max()) == 0.0          # constants when not --GP_joint
            continue
        e = H.relerr(eng.grads[k].reshape(-1), grads[k].reshape(-1))
        print(f"{case} grad {k}: {e:.2e}")
        if not e < BC.GRAD_TOL:
            bad.append(f"grad {k}: {e:.2e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", ["NP64_c33", "NP64_c32", "NP64_c62"])
def test_context_length_scale_gradient_matches_oracle(case):
    """The context likelihoods use the constant model length scale; their reverse pass still leaves d loss / d lt per
    coordinate in eng.c_dl (accumulating launch, so one step on a fresh engine).  Expected: autograd of the oracle."""
    cs, eng, out, grads = _pearce_step(case)
    eng.stream.synchronize()
    want = torch.stack([grads["ctx_l_x"], grads["ctx_l_y"]])
    e = H.relerr(eng.c_dl, want)
    print(f"{case} c_dl: {e:.2e} (want {want.tolist()})")
    assert e < BC.GRAD_TOL


def test_exact_gp_limit_is_enforced_on_the_host():
    from svgp_vae_amd import _lib
    from svgp_vae_amd._lib import PearceBufs
    with pytest.raises(_lib.SvgpError):
        _pearce_engine({}, "GPVAE_Pearce", 2.0, True, 4, 65, 8, 8, 1.0)
    lib = _lib.load_library()
    # n = 65: refused before any pointer is looked at and before anything is launched
    rc = lib.svgp_pearce_gp_fwd(C.byref(PearceBufs(B=2, T=65, n=65)), None, None, None, None)
    assert rc == -2, rc                                               # SVGP_ERR_UNSUPPORTED (include/svgpvae_hip.h)
    assert b"n=65" in lib.svgp_last_error()
    rc = lib.svgp_pearce_gp_bwd(C.byref(PearceBufs(B=2, T=65, n=65)), 1.0, 0, None, None, None, None)
    assert rc == -2, rc
