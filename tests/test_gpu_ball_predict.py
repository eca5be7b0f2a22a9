"""Moving-ball predictor on the GPU: svgp_ball_predict / svgp_ball_predict_large against the float64 restatement of
tests/ball_predict_cases.py over its case table, the entry points' behaviour, the training engines' posterior at the frame times,
BallPredictor.predict against the oracle's MLPs composed with the restatement, and the command line end to end."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ball_predict_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CANARY, PAD = 12345.678, 64


class _Out:
    """A (Q, B) output with PAD canary values on both sides."""

    def __init__(self, Q, B):
        self.buf = torch.full((Q * B + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
        self.view = self.buf[PAD:PAD + Q * B].view(Q, B)

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all() and (self.buf[-PAD:] == CANARY).all())


def run(prob, large, *, eps=True, want_z=True, mask=True, tq=None):
    """One call of an entry point on a problem dict -> dict(p_m, p_v, z (2, Q, B) numpy; z None when not asked for).  Asserts that
    the canaries around every output are intact (and that a z that was not asked for is not written)."""
    from svgp_vae_amd import _lib
    from svgp_vae_amd._lib import BallPredictBufs, BallPredictCfg
    lib = _lib.load_library()
    T, B = prob["y"].shape[1:]
    tq = prob["tq"] if tq is None else tq
    Q, m = tq.size, prob["ip"].shape[1]
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)
    d = {k: dv(prob[k]) for k in ("times", "ip", "ls", "y", "s2")}
    d["tq"] = dv(tq)
    d["mask"] = dv(prob["mask"]) if mask is True else (None if mask is None or mask is False else dv(mask))
    d["eps"] = dv(prob["eps"]) if eps is True else (None if eps is None or eps is False else dv(eps))
    outs = {k: [_Out(Q, B) for _ in range(2)] for k in ("p_m", "p_v", "z")}
    cfg = BallPredictCfg(B=B, T=T, m=m, Q=Q, jitter=prob["jitter"], clip_lo=PC.CLIP[0], clip_hi=PC.CLIP[1])
    q = BallPredictBufs()
    q.times, q.tq, q.mask = d["times"].data_ptr(), d["tq"].data_ptr(), None if d["mask"] is None else d["mask"].data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"ip_{cn}", d["ip"][c].data_ptr()); setattr(q, f"ls_{cn}", d["ls"][c:].data_ptr())
        setattr(q, f"mu_{cn}", d["y"][c].data_ptr()); setattr(q, f"var_{cn}", d["s2"][c].data_ptr())
        setattr(q, f"eps_{cn}", None if d["eps"] is None else d["eps"][c].data_ptr())
        setattr(q, f"p_m_{cn}", outs["p_m"][c].view.data_ptr()); setattr(q, f"p_v_{cn}", outs["p_v"][c].view.data_ptr())
        setattr(q, f"z_{cn}", outs["z"][c].view.data_ptr() if want_z else None)
    s = torch.cuda.current_stream().cuda_stream
    if large:
        n = int(lib.svgp_ball_predict_large_workspace_elems(C.byref(cfg)))
        assert n > 0
        work = _Out(n, 1)
        _lib.call("svgp_ball_predict_large", C.byref(cfg), C.byref(q), work.view.data_ptr(), s)
    else:
        _lib.call("svgp_ball_predict", C.byref(cfg), C.byref(q), s)
    torch.cuda.synchronize()
    assert not large or work.intact()
    for k, pair in outs.items():
        for o in pair:
            assert o.intact(), k
            if k == "z" and not want_z:
                assert bool((o.view == CANARY).all())
    get = lambda k: np.stack([o.view.cpu().numpy() for o in outs[k]])
    return dict(p_m=get("p_m"), p_v=get("p_v"), z=get("z") if want_z else None)


def entries(case):
    return [False, True] if PC.kernel_shape(case)[2] <= PC.FUSED_M_MAX else [True]


# ---------------------------------------------------------------------------------------------- case sweep
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_case_sweep_against_the_restatement(case):
    prob, ref = PC.kernel_problem(case), dict(zip(("p_m", "p_v", "z"), PC.kernel_reference(case)))
    got = {large: run(prob, large) for large in entries(case)}
    bad = []
    for large, g in got.items():
        for k in ("p_m", "p_v", "z"):
            e = PC.relerr(g[k], ref[k])
            print(f"{case} {'large' if large else 'fused'} {k}: {e:.2e}")
            if not e <= PC.TOL:
                bad.append((large, k, e))
    if len(got) == 2:
        for k in ("p_m", "p_v", "z"):
            e = PC.relerr(got[False][k], got[True][k])
            print(f"{case} fused against large {k}: {e:.2e}")
            if not e <= PC.TOL:
                bad.append(("both", k, e))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- entry-point behaviour
BEHAVIOUR = [("3-30-17-33", False), ("2-64-64-40", False), ("3-30-17-33", True), ("2-100-65-40", True), ("70-30-15-9", True)]
BEHAVIOUR_IDS = [f"{c}-{'large' if l else 'fused'}" for c, l in BEHAVIOUR]


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_eps_and_z_may_be_null_and_two_calls_are_bitwise_equal(case, large):
    prob = PC.kernel_problem(case)
    a, b = run(prob, large), run(prob, large)
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(a[k], b[k]), k
    mean = run(prob, large, eps=None)
    assert np.array_equal(mean["p_m"], a["p_m"]) and np.array_equal(mean["p_v"], a["p_v"]) and np.array_equal(mean["z"], a["p_m"])
    noz = run(prob, large, want_z=False)
    assert noz["z"] is None and np.array_equal(noz["p_m"], a["p_m"]) and np.array_equal(noz["p_v"], a["p_v"])
    ref = PC.reference_of(prob, use_eps=False)
    assert PC.relerr(mean["z"], ref[2]) <= PC.TOL


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_null_mask_is_a_mask_of_ones_bitwise(case, large):
    prob = PC.kernel_problem(case)
    a, b = run(prob, large, mask=None), run(prob, large, mask=np.ones_like(prob["mask"]))
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(a[k], b[k]), k
    ref = PC.reference_of(prob, use_mask=False)
    for k, r in zip(("p_m", "p_v", "z"), ref):
        assert PC.relerr(a[k], r) <= PC.TOL, k


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_permuted_query_times_give_the_permuted_outputs_bitwise(case, large):
    prob = PC.kernel_problem(case)
    perm = np.random.RandomState(5).permutation(prob["tq"].size)
    a = run(prob, large)
    b = run(prob, large, tq=prob["tq"][perm], eps=prob["eps"][:, perm])
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(a[k][:, perm], b[k]), k


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_all_dropped_video_gives_the_prior_exactly(case, large):
    g = run(PC.kernel_problem(case), large)
    assert (g["p_m"][:, :, 1] == 0).all()
    assert np.abs(g["p_v"][:, :, 1] - 1).max() <= 1e-10
    if not large:
        assert (g["p_v"][:, :, 1] == 1).all()                            # X = 0 exactly: one LDS routine inverts both matrices


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_nan_in_one_videos_mu_stays_in_that_videos_outputs(case, large):
    prob = PC.kernel_problem(case)
    assert prob["mask"][0, 0] == 1 and prob["s2"][1, 0, 0] > 0          # a kept frame that carries information
    y = prob["y"].copy()
    y[1, 0, 0] = np.nan
    a, b = run(prob, large), run(dict(prob, y=y), large)
    for k in ("p_m", "z"):
        assert np.isnan(b[k][1, :, 0]).all(), k
        assert np.array_equal(b[k][0], a[k][0]) and np.array_equal(b[k][1, :, 1:], a[k][1, :, 1:]), k
    assert np.array_equal(b["p_v"], a["p_v"])                            # the variance does not depend on mu


# ---------------------------------------------------------------------------------------------- against the training path
def _predictor(p, T, m, px, hidden, jitter, clip_qs, tmax=None):
    from svgp_vae_amd.ball_predict import BallPredictor
    return BallPredictor(p, tmax=T if tmax is None else tmax, m=m, hidden=hidden, px=px, py=px, jitter=jitter, clip_qs=clip_qs)


@pytest.mark.parametrize("B,T,m", [(35, 30, 15), (3, 30, 64), (3, 30, 65)])
def test_frame_times_with_nothing_dropped_equal_the_training_engines_posterior(B, T, m):
    from svgp_vae_amd import ball
    from tests.helpers import relerr
    px, hidden, jitter = 8, 16, 1e-6
    p, vid, _, _, _ = PC.predictor_problem(B, T, m, 1, px=px, hidden=hidden, seed=3)
    cls = ball.sparse_engine_class(m, B)
    assert cls is (ball.BallStepEngine if m <= 64 else ball.BallLargeStepEngine)
    mk = lambda n: ball.SVGP(False, m, False, 1, T, 2.0, False, n, jitter, 1, T, 2.0)
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items()}
    eng = cls(mk("x"), mk("y"), batch=B, tmax=T, px=px, py=px, hidden=hidden, clip_qs=True, beta=1.0, params=flat)
    eng.step(vid.to(DEV), torch.zeros(B, T, 2, dtype=torch.float64), adam=False, backward=False)
    out = eng.outputs()
    got = _predictor(p, T, m, px, hidden, jitter, True).predict(vid, np.arange(1, T + 1))
    e_m, e_v = relerr(got["p_m"], out[5]), relerr(got["p_v"], out[6])
    print(f"({B}, {T}, {m}) against {cls.__name__}: p_m {e_m:.2e}, p_v {e_v:.2e}")
    assert e_m <= PC.TOL and e_v <= PC.TOL
    assert relerr(got["z"], got["p_m"]) == 0                             # eps None: the posterior mean is decoded


# ---------------------------------------------------------------------------------------------- BallPredictor.predict
@pytest.mark.parametrize("B,T,m,Q,kw", [
    (1, 12, 5, 7, dict()),                                               # B = 1, T different from the training tmax
    (3, 12, 15, 20, dict(drop_video=1, eps=True)),                       # a wholly dropped video, a draw
    (2, 9, 4, 5, dict(frame_times=True, observed=None)),                 # other frame times, nothing dropped
    (2, 20, 65, 9, dict(drop_video=0, eps=True)),                        # the large entry behind the same interface
], ids=["B1", "dropped-video", "frame-times", "m65"])
def test_predict_against_the_oracle_mlps_composed_with_the_restatement(B, T, m, Q, kw):
    px, hidden, jitter = 8, 16, 1e-9
    p, vid, observed, tq, eps = PC.predictor_problem(B, T, m, Q, px=px, hidden=hidden, seed=7 + m, drop_video=kw.get("drop_video"))
    observed = None if "observed" in kw else observed
    eps = eps if kw.get("eps") else None
    ft = 0.5 + 1.25 * np.arange(T) if kw.get("frame_times") else None
    if ft is not None:                                                   # inducing points over the span of these frame times
        for c in "xy":
            p[f"ip_{c}"] = torch.as_tensor(np.linspace(ft[0], ft[-1], m))
        lt = 0.75 * (ft[-1] - ft[0]) / (m - 1)
        p["l_x"], p["l_y"] = torch.tensor(lt, dtype=torch.float64), torch.tensor(lt / 1.1, dtype=torch.float64)
    ref = PC.predictor_reference(p, vid, observed, tq, eps, jitter=jitter, clip_qs=True, frame_times=ft)
    pred = _predictor(p, T, m, px, hidden, jitter, True, tmax=30)
    state = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    got = pred.predict(vid, tq, observed=observed, frame_times=ft, eps=eps)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state[0]) and torch.equal(torch.get_rng_state(), state[1])
    assert tuple(got["frames"].shape) == (B, Q, px, px) and tuple(got["p_m"].shape) == (B, Q, 2)
    for k in ("frames", "p_m", "p_v", "z"):
        e = PC.relerr(got[k].cpu().numpy(), ref[k])
        print(f"predict {k}: {e:.2e}")
        assert e <= PC.TOL, (k, e)
    fr = got["frames"].cpu().numpy()
    assert np.isfinite(fr).all() and fr.min() >= 0 and fr.max() <= 1
    assert pred.route(B, T, Q) == PC.expected_route(B, T, m, Q, m > PC.FUSED_M_MAX)


# ---------------------------------------------------------------------------------------------- end to end
def test_train_save_then_fill_and_upsample_from_the_command_line(tmp_path):
    """Two fresh child processes, each under its own time limit; the second starts only if the first succeeded."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = str(tmp_path)
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.BALL_experiment", "--elbo", "SVGPVAE_Hensman", "--steps", "12", "--save_model",
                        "--base_dir", base, "--expid", "bp"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    ckpts = glob.glob(os.path.join(base, "bp_*", "model.pt"))
    assert len(ckpts) == 1, ckpts
    ck = torch.load(ckpts[0], map_location="cpu")
    assert ck["meta"] == dict(elbo="SVGPVAE_Hensman", tmax=30, m=15, hidden=500, px=32, py=32, jitter=1e-9, clip_qs=False, vidlt=2.0)
    assert set(ck) == {"theta", "adam_m", "adam_v", "state", "shapes", "meta"}
    out = str(tmp_path / "frames.npy")
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.ball_predict", "--checkpoint", ckpts[0], "--test_batch", "0", "--base_dir", base,
                        "--drop", "0.5", "--upsample", "2", "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    frames = np.load(out)
    assert frames.shape == (35, 59, 32, 32) and np.isfinite(frames).all() and frames.min() >= 0 and frames.max() <= 1
    assert "route (1 GP launch): k_ball_predict" in r.stdout
    assert "MSE of the" in r.stdout
