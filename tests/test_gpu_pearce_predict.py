"""Exact-GP moving-ball predictor on the GPU: svgp_pearce_predict / svgp_pearce_predict_long against the float64 restatement of
tests/pearce_predict_cases.py over its case table, the entry points' behaviour, the training engines' posterior at the frame
times, PearcePredictor.predict against the oracle's MLPs composed with the restatement, and the command line end to end."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pearce_predict_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CANARY, PAD = 12345.678, 64
KEYS = ("p_m", "p_v", "z", "lh")


class _Out:
    """A (rows, B) output with PAD canary values on both sides."""

    def __init__(self, rows, B):
        self.buf = torch.full((rows * B + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
        self.view = self.buf[PAD:PAD + rows * B].view(rows, B)

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all() and (self.buf[-PAD:] == CANARY).all())


def run(prob, long_form, *, eps=True, want_z=True, want_lh=True, mask=True, tq=None, q_slices=0, y=None, s2=None):
    """One call of an entry point on a problem dict -> dict(p_m, p_v, z (2, Q, B), lh (2, B) numpy; z / lh None when not asked for).
    Asserts that the canaries around every output (and the workspace) are intact and that an output not asked for is not written."""
    from svgp_vae_amd import _lib
    lib = _lib.load_library()
    T, B = prob["y"].shape[1:]
    tq = prob["tq"] if tq is None else tq
    Q = tq.size
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)
    d = dict(times=dv(prob["times"]), ls=dv(prob["ls"]), y=dv(prob["y"] if y is None else y),
             s2=dv(prob["s2"] if s2 is None else s2), tq=dv(tq))
    d["mask"] = dv(prob["mask"]) if mask is True else (None if mask is None or mask is False else dv(mask))
    d["eps"] = dv(prob["eps"]) if eps is True else (None if eps is None or eps is False else dv(eps))
    outs = {k: [_Out(Q, B) for _ in range(2)] for k in ("p_m", "p_v", "z")}
    lh = _Out(2, B)
    cfg = _lib.PearcePredictCfg(B=B, T=T, Q=Q, q_slices=q_slices)
    q = _lib.PearcePredictBufs()
    q.times, q.tq, q.mask = d["times"].data_ptr(), d["tq"].data_ptr(), None if d["mask"] is None else d["mask"].data_ptr()
    q.lh = lh.view.data_ptr() if want_lh else None
    for c, cn in enumerate("xy"):
        setattr(q, f"ls_{cn}", d["ls"][c:].data_ptr())
        setattr(q, f"mu_{cn}", d["y"][c].data_ptr()); setattr(q, f"var_{cn}", d["s2"][c].data_ptr())
        setattr(q, f"eps_{cn}", None if d["eps"] is None else d["eps"][c].data_ptr())
        setattr(q, f"p_m_{cn}", outs["p_m"][c].view.data_ptr()); setattr(q, f"p_v_{cn}", outs["p_v"][c].view.data_ptr())
        setattr(q, f"z_{cn}", outs["z"][c].view.data_ptr() if want_z else None)
    s = torch.cuda.current_stream().cuda_stream
    if long_form:
        n = int(lib.svgp_pearce_predict_long_workspace_elems(C.byref(cfg)))
        assert n > 0
        work = _Out(n, 1)
        _lib.call("svgp_pearce_predict_long", C.byref(cfg), C.byref(q), work.view.data_ptr(), s)
    else:
        _lib.call("svgp_pearce_predict", C.byref(cfg), C.byref(q), s)
    torch.cuda.synchronize()
    assert not long_form or work.intact()
    assert lh.intact() and (want_lh or bool((lh.view == CANARY).all()))
    for k, pair in outs.items():
        for o in pair:
            assert o.intact(), k
            if k == "z" and not want_z:
                assert bool((o.view == CANARY).all())
    get = lambda k: np.stack([o.view.cpu().numpy() for o in outs[k]])
    return dict(p_m=get("p_m"), p_v=get("p_v"), z=get("z") if want_z else None, lh=lh.view.cpu().numpy() if want_lh else None)


def same(a, b, keys=KEYS):
    return [k for k in keys if not np.array_equal(a[k], b[k])]


# ---------------------------------------------------------------------------------------------- case sweep
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_case_sweep_against_the_restatement(case):
    """Largest errors seen on an MI355X: DESIGN.md section 9i."""
    prob, ref = PC.kernel_problem(case), PC.kernel_reference(case)
    got = {long_form: run(prob, long_form) for long_form in PC.entries(case)}
    bad = []
    for long_form, g in got.items():
        for k in KEYS:
            e = PC.relerr(g[k], ref[k])
            print(f"{case} {'long' if long_form else 'lds'} {k}: {e:.2e}")
            if not e <= PC.TOL:
                bad.append((long_form, k, e))
    if len(got) == 2:
        for k in KEYS:
            e = PC.relerr(got[False][k], got[True][k])
            print(f"{case} lds against long {k}: {e:.2e}")
            if not e <= PC.TOL:
                bad.append(("both", k, e))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- entry-point behaviour
BEHAVIOUR = [("3-5-4", False), ("2-33-5", False), ("3-64-300", False), ("35-30-59", False), ("3-5-4", True), ("3-64-300", True),
             ("2-130-7", True), (f"{PC.NB + 1}-65-3", True)]
BEHAVIOUR_IDS = [f"{c}-{'long' if l else 'lds'}" for c, l in BEHAVIOUR]


@pytest.mark.parametrize("case,long_form", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_eps_z_and_lh_may_be_null_and_two_calls_are_bitwise_equal(case, long_form):
    prob = PC.kernel_problem(case)
    a, b = run(prob, long_form), run(prob, long_form)
    assert not same(a, b)
    mean = run(prob, long_form, eps=None)
    assert not same(mean, a, ("p_m", "p_v", "lh")) and np.array_equal(mean["z"], a["p_m"])
    bare = run(prob, long_form, want_z=False, want_lh=False)
    assert bare["z"] is None and bare["lh"] is None and not same(bare, a, ("p_m", "p_v"))
    assert PC.relerr(mean["z"], PC.reference_of(prob, use_eps=False)["z"]) <= PC.TOL


@pytest.mark.parametrize("case,long_form", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_null_mask_is_a_mask_of_ones_bitwise(case, long_form):
    prob = PC.kernel_problem(case)
    a, b = run(prob, long_form, mask=None), run(prob, long_form, mask=np.ones_like(prob["mask"]))
    assert not same(a, b)
    ref = PC.reference_of(prob, use_mask=False)
    for k in KEYS:
        assert PC.relerr(a[k], ref[k]) <= PC.TOL, k


@pytest.mark.parametrize("case,long_form", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_permuted_query_times_give_each_query_the_same_bits(case, long_form):
    prob = PC.kernel_problem(case)
    perm = np.random.RandomState(5).permutation(prob["tq"].size)
    a = run(prob, long_form)
    b = run(prob, long_form, tq=prob["tq"][perm], eps=prob["eps"][:, perm])
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(a[k][:, perm], b[k]), k
    assert np.array_equal(a["lh"], b["lh"])


@pytest.mark.parametrize("case", ["3-5-4", "2-64-70", "3-64-300", "35-30-59"])
def test_query_slices_do_not_change_a_bit(case):
    prob = PC.kernel_problem(case)
    one, three, plan = run(prob, False, q_slices=1), run(prob, False, q_slices=3), run(prob, False)
    assert not same(one, three) and not same(one, plan)
    assert not same(one, run(prob, False, q_slices=prob["tq"].size))        # a query time per slice


@pytest.mark.parametrize("case,long_form", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_nan_in_dropped_frames_reaches_no_output(case, long_form):
    prob = PC.kernel_problem(case)
    nan = np.where(prob["mask"][None] == 0, np.nan, 1.0)
    assert np.isnan(nan).any()
    a, b = run(prob, long_form), run(prob, long_form, y=prob["y"] * nan, s2=prob["s2"] * nan)
    assert not same(a, b) and all(np.isfinite(b[k]).all() for k in KEYS)


@pytest.mark.parametrize("case,long_form", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_all_dropped_video_gives_the_prior_exactly(case, long_form):
    prob = PC.kernel_problem(case)
    g = run(prob, long_form)
    assert (g["p_m"][:, :, 1] == 0).all() and (g["p_v"][:, :, 1] == 1).all() and (g["lh"][:, 1] == 0).all()
    assert np.array_equal(g["z"][:, :, 1], prob["eps"][:, :, 1])           # the draw from the prior: 0 + eps sqrt(1)


# ---------------------------------------------------------------------------------------------- against the training path
@pytest.mark.parametrize("B,T", [(35, 30), (3, 70)])
def test_frame_times_with_nothing_dropped_equal_the_training_engines_posterior(B, T):
    """The engines count the frames 0..T-1; the same times go to the entry point, tq = times, no mask."""
    from svgp_vae_amd import ball
    from tests.ball_cases import _problem
    from tests.helpers import relerr
    px, hidden = 8, 16
    p, vid, eps = _problem(B, T, px, hidden, 1, seed=11, lt=2.0)
    flat = {k: (v.reshape(-1) if k.startswith(("encB", "decB", "l_")) else v) for k, v in p.items() if not k.startswith("ip_")}
    cls = ball.pearce_engine_class(T)
    assert cls is (ball.PearceStepEngine if T <= 64 else ball.PearceLongStepEngine)
    eng = cls("GPVAE_Pearce", 2.0, 0.5, True, 2.0, batch=B, tmax=T, px=px, py=px, hidden=hidden, beta=1.0, params=flat)
    eng.step(vid.to(DEV), eps, adam=False, backward=False)
    eng.stream.synchronize()
    times = eng.times.cpu().numpy()
    assert times[0] == 0 and times[-1] == T - 1
    prob = dict(times=times, tq=times, ls=np.array([float(p["l_x"]), float(p["l_y"])]), y=eng.buf["y"].cpu().numpy(),
                s2=eng.buf["s2"].cpu().numpy(), mask=None, eps=None)
    got = run(prob, T > PC.FUSED_T_MAX, mask=None, eps=None)
    for k, want in (("p_m", eng.buf["p_m"]), ("p_v", eng.buf["p_v"]), ("lh", eng.lh)):
        e = relerr(got[k], want.cpu().numpy())
        print(f"({B}, {T}) against {cls.__name__} {k}: {e:.2e}")
        assert e <= 1e-12, (k, e)


# ---------------------------------------------------------------------------------------------- PearcePredictor.predict
@pytest.mark.parametrize("B,T,Q,kw", [
    (1, 12, 7, dict()),                                                  # B = 1, T different from the training tmax
    (3, 12, 20, dict(drop_video=1, eps=True)),                           # a wholly dropped video, a draw
    (2, 9, 5, dict(frame_times=True, observed=None)),                    # other frame times, nothing dropped
    (2, 70, 9, dict(drop_video=0, eps=True)),                            # the long entry behind the same interface
], ids=["B1", "dropped-video", "frame-times", "T70"])
def test_predict_against_the_oracle_mlps_composed_with_the_restatement(B, T, Q, kw):
    from svgp_vae_amd.ball_predict import PearcePredictor
    px, hidden = 8, 16
    p, vid, observed, tq, eps = PC.predictor_problem(B, T, Q, px=px, hidden=hidden, seed=7 + T, drop_video=kw.get("drop_video"))
    observed = None if "observed" in kw else observed
    eps = eps if kw.get("eps") else None
    ft = 0.5 + 1.25 * np.arange(T) if kw.get("frame_times") else None
    ref = PC.predictor_reference(p, vid, observed, tq, eps, frame_times=ft)
    pred = PearcePredictor(p, tmax=30, hidden=hidden, px=px, py=px)
    state = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    got = pred.predict(vid, tq, observed=observed, frame_times=ft, eps=eps)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state[0]) and torch.equal(torch.get_rng_state(), state[1])
    assert tuple(got["frames"].shape) == (B, Q, px, px) and tuple(got["p_m"].shape) == (B, Q, 2) and tuple(got["lh"].shape) == (B, 2)
    for k in ("frames", "p_m", "p_v", "z", "lh"):
        e = PC.relerr(got[k].cpu().numpy(), ref[k])
        print(f"predict {k}: {e:.2e}")
        assert e <= PC.TOL, (k, e)
    fr = got["frames"].cpu().numpy()
    assert np.isfinite(fr).all() and fr.min() >= 0 and fr.max() <= 1
    assert pred.route(B, T, Q) == PC.expected_route(B, T, Q, T > PC.FUSED_T_MAX)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("elbo,kernel", [("GPVAE_Pearce", "k_pearce_predict"), ("SVGPVAE_Hensman", "k_ball_predict")])
def test_train_save_then_fill_and_upsample_from_the_command_line(tmp_path, elbo, kernel):
    """Two fresh child processes, each under its own time limit; the second starts only if the first succeeded."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = str(tmp_path)
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.BALL_experiment", "--elbo", elbo, "--steps", "2", "--tmax", "8", "--hidden", "16",
                        "--save_model", "--base_dir", base, "--expid", "pp"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    ckpts = glob.glob(os.path.join(base, "pp_*", "model.pt"))
    assert len(ckpts) == 1, ckpts
    ck = torch.load(ckpts[0], map_location="cpu")
    assert ck["meta"] == dict(elbo=elbo, tmax=8, m=15, hidden=16, px=32, py=32, jitter=1e-9, clip_qs=False, vidlt=2.0)
    assert ("ip_x" in ck["shapes"]) == elbo.startswith("SVGPVAE")
    out = str(tmp_path / "frames.npy")
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.ball_predict", "--checkpoint", ckpts[0], "--test_batch", "0", "--base_dir", base,
                        "--drop", "0.5", "--upsample", "2", "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    frames = np.load(out)
    assert frames.shape == (35, 15, 32, 32) and np.isfinite(frames).all() and frames.min() >= 0 and frames.max() <= 1
    assert f"route (1 GP launch): {kernel}" in r.stdout
    assert "MSE of the" in r.stdout
