"""Moving-ball joint predictor on the GPU: svgp_ball_predict_joint / svgp_ball_predict_joint_large against the float64 restatement of
tests/ball_joint_cases.py over its case table, identities of the device's own factor at the model's jitter, the entry points'
behaviour, BallPredictor.predict(paths=True, return_cov=True) against the oracle's MLPs composed with the restatement, and the
command line end to end."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ball_joint_cases as JC
from tests import ball_predict_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CANARY, PAD = 12345.678, 64
OUTPUTS = ("p_m", "cov", "chol", "z")


class _Out:
    """An output of the given shape with PAD canary values on both sides."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(*shape)

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all() and (self.buf[-PAD:] == CANARY).all())


def run(prob, large, jp, *, eps=True, mask=True, tq=None, want=("cov", "chol", "z")):
    """One call of an entry point on a problem dict -> dict(p_m, z (2, Q, B); cov, chol (2, B, Q, Q)) numpy, None for an output
    that was not asked for.  Asserts that the canaries around every output are intact and that an output that was not asked for
    is not written."""
    from svgp_vae_amd import _lib
    lib = _lib.load_library()
    T, B = prob["y"].shape[1:]
    tq = prob["tq"] if tq is None else tq
    Q, m = tq.size, prob["ip"].shape[1]
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)
    d = {k: dv(prob[k]) for k in ("times", "ip", "ls", "y", "s2")}
    d["tq"] = dv(tq)
    d["mask"] = dv(prob["mask"]) if mask is True else (None if mask is None or mask is False else dv(mask))
    d["eps"] = dv(prob["eps"]) if eps is True else (None if eps is None or eps is False else dv(eps))
    shape = dict(p_m=(Q, B), z=(Q, B), cov=(B, Q, Q), chol=(B, Q, Q))
    outs = {k: [_Out(*shape[k]) for _ in range(2)] for k in OUTPUTS}
    cfg = _lib.BallPredictJointCfg(B=B, T=T, m=m, Q=Q, jitter=prob["jitter"], path_jitter=jp)
    q = _lib.BallPredictJointBufs()
    q.times, q.tq, q.mask = d["times"].data_ptr(), d["tq"].data_ptr(), None if d["mask"] is None else d["mask"].data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"ip_{cn}", d["ip"][c].data_ptr()); setattr(q, f"ls_{cn}", d["ls"][c:].data_ptr())
        setattr(q, f"mu_{cn}", d["y"][c].data_ptr()); setattr(q, f"var_{cn}", d["s2"][c].data_ptr())
        setattr(q, f"eps_{cn}", None if d["eps"] is None else d["eps"][c].data_ptr())
        for k in OUTPUTS:
            setattr(q, f"{k}_{cn}", outs[k][c].view.data_ptr() if k == "p_m" or k in want else None)
    s = torch.cuda.current_stream().cuda_stream
    if large:
        n = int(lib.svgp_ball_predict_joint_large_workspace_elems(C.byref(cfg)))
        assert n > 0
        work = _Out(n)
        _lib.call("svgp_ball_predict_joint_large", C.byref(cfg), C.byref(q), work.view.data_ptr(), s)
    else:
        _lib.call("svgp_ball_predict_joint", C.byref(cfg), C.byref(q), s)
    torch.cuda.synchronize()
    assert not large or work.intact()
    for k, pair in outs.items():
        for o in pair:
            assert o.intact(), k
            if k != "p_m" and k not in want:
                assert bool((o.view == CANARY).all()), k
    return {k: np.stack([o.view.cpu().numpy() for o in outs[k]]) if k == "p_m" or k in want else None for k in OUTPUTS}


def entries(case):
    return [False, True] if JC.is_fused(case) else [True]


@functools.lru_cache(maxsize=None)
def device_run(case, large, jp):
    """Shared by the tests of the sweep: callers must not write to it."""
    return run(JC.kernel_problem(case), large, jp)


def marginal_p_v(prob, large):
    from tests.test_gpu_ball_predict import run as run_marginal
    return run_marginal(prob, large, eps=None, want_z=False)["p_v"]


# ---------------------------------------------------------------------------------------------- case sweep
@pytest.mark.parametrize("case", JC.KERNEL_IDS)
def test_case_sweep_of_p_m_and_cov_against_the_restatement(case):
    prob, ref = JC.kernel_problem(case), JC.kernel_reference(case)
    got = {large: device_run(case, large, JC.JITTER) for large in entries(case)}
    p_v = marginal_p_v(prob, PC.kernel_shape(case)[2] > PC.FUSED_M_MAX)
    bad = []
    for large, g in got.items():
        name = "large" if large else "fused"
        for k in ("p_m", "cov"):
            e = JC.relerr(g[k], ref[k])
            print(f"{case} {name} {k}: {e:.2e}")
            if not e <= JC.TOL:
                bad.append((name, k, e))
        if not np.array_equal(g["cov"], g["cov"].transpose(0, 1, 3, 2)):
            bad.append((name, "cov is not symmetric bit for bit"))
        e = JC.relerr(np.diagonal(g["cov"], axis1=2, axis2=3).transpose(0, 2, 1), p_v)
        print(f"{case} {name} diag(cov) against svgp_ball_predict's p_v: {e:.2e}")
        if not e <= JC.TOL:
            bad.append((name, "diag", e))
    if len(got) == 2:
        for k in ("p_m", "cov"):
            e = JC.relerr(got[False][k], got[True][k])
            print(f"{case} fused against large {k}: {e:.2e}")
            if not e <= JC.TOL:
                bad.append(("both", k, e))
    assert not bad, bad


@pytest.mark.parametrize("case", JC.KERNEL_IDS)
def test_identities_of_the_devices_own_factor_at_the_models_jitter(case):
    """At path_jitter = 1e-9 the factor is not compared with the restatement (ball_joint_cases): chol is lower triangular with a
    positive diagonal, chol chol^T is cov + jp I within the derived bound, and z is p_m + chol eps, all on the device's outputs.

    Measured on an MI355X, residual / bound: fused at most 0.086 (3-5-1-3), the large route at most 0.17 (3-5-1-3); beyond one
    64-block 0.014 (2-64-33-70) and 0.008 (3-12-5-700).  Those two stood at 2.04 and 3.10 while the large route factored with
    svgp_potrf_batched as it is, whose panel solves multiply by the explicit inverse of the diagonal block's factor; the route now
    runs it with every panel solve refined once (svgp_potrf_batched_refined, cholesky.hip)."""
    prob = JC.kernel_problem(case)
    bad = []
    for large in entries(case):
        g, name = device_run(case, large, JC.JITTER), "large" if large else "fused"
        L, Q = g["chol"], g["chol"].shape[-1]
        assert np.isfinite(L).all() and np.isfinite(g["z"]).all()
        assert (np.triu(L, 1) == 0).all() and (np.diagonal(L, axis1=2, axis2=3) > 0).all()
        A = g["cov"] + JC.JITTER * np.eye(Q)
        worst = 0.0
        for c in range(2):
            for b in range(L.shape[1]):
                r = np.abs(L[c, b] @ L[c, b].T - A[c, b]).max() / JC.chol_residual_bound(A[c, b])
                worst = max(worst, float(r))
        print(f"{case} {name}: residual / bound {worst:.3f}")
        if not worst <= 1.0:
            bad.append((name, "residual / bound", worst))
        z = g["p_m"] + np.einsum("cbqr,crb->cqb", L, prob["eps"])
        e = JC.relerr(g["z"], z)
        print(f"{case} {name} z against p_m + chol eps: {e:.2e}")
        if not e <= JC.TOL:
            bad.append((name, "z", e))
    assert not bad, bad


@pytest.mark.parametrize("case", JC.KERNEL_IDS)
def test_z_and_chol_against_the_restatement_at_the_direct_path_jitter(case):
    ref = JC.kernel_reference(case)
    got = {large: device_run(case, large, JC.PATH_JITTER_DIRECT) for large in entries(case)}
    bad = []
    for large, g in got.items():
        for k in OUTPUTS:
            e = JC.relerr(g[k], ref[k])
            print(f"{case} {'large' if large else 'fused'} {k}: {e:.2e}")
            if not e <= JC.TOL:
                bad.append((large, k, e))
    if len(got) == 2:
        for k in ("z", "chol"):
            e = JC.relerr(got[False][k], got[True][k])
            print(f"{case} fused against large {k}: {e:.2e}")
            if not e <= JC.TOL:
                bad.append(("both", k, e))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- entry-point behaviour
BEHAVIOUR = [("3-30-17-33", False), ("2-64-64-64", False), ("3-30-17-33", True), ("2-64-33-70", True), ("2-100-65-40", True),
             ("70-30-15-9", True)]
BEHAVIOUR_IDS = [f"{c}-{'large' if l else 'fused'}" for c, l in BEHAVIOUR]


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_optional_pointers_may_be_null_in_turn_and_two_calls_are_bitwise_equal(case, large):
    prob, jp = JC.kernel_problem(case), JC.PATH_JITTER_DIRECT
    a, b = device_run(case, large, jp), run(prob, large, jp)
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    mean = run(prob, large, jp, eps=None)
    assert np.array_equal(mean["z"], a["p_m"])
    for k in ("p_m", "cov", "chol"):
        assert np.array_equal(mean[k], a[k]), k
    for drop in ("cov", "chol", "z"):
        g = run(prob, large, jp, want=tuple(k for k in ("cov", "chol", "z") if k != drop))
        assert g[drop] is None
        for k in OUTPUTS:
            assert k == drop or np.array_equal(g[k], a[k]), (drop, k)
    only = run(prob, large, jp, want=())
    assert np.array_equal(only["p_m"], a["p_m"])
    nomask = run(prob, large, jp, mask=None)
    ones = run(prob, large, jp, mask=np.ones_like(prob["mask"]))
    for k in OUTPUTS:
        assert np.array_equal(nomask[k], ones[k]), k


@pytest.mark.parametrize("case", ["3-30-17-33", "35-30-15-61", "2-64-64-64"])
def test_fused_entry_permuted_query_times_permute_cov_bitwise(case):
    prob = JC.kernel_problem(case)
    perm = np.random.RandomState(5).permutation(prob["tq"].size)
    a = device_run(case, False, JC.JITTER)
    b = run(prob, False, JC.JITTER, tq=prob["tq"][perm], eps=prob["eps"][:, perm])
    assert np.array_equal(a["cov"][:, :, perm][:, :, :, perm], b["cov"])
    assert np.array_equal(a["p_m"][:, perm], b["p_m"])


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_all_dropped_video_gives_the_prior(case, large):
    prob, g = JC.kernel_problem(case), device_run(case, large, JC.JITTER)
    assert (g["p_m"][:, :, 1] == 0).all()
    for c in range(2):
        assert JC.relerr(g["cov"][c, 1], JC.se(prob["tq"], prob["tq"], prob["ls"][c])) <= JC.TOL


@pytest.mark.parametrize("case,large", BEHAVIOUR, ids=BEHAVIOUR_IDS)
def test_nan_in_one_videos_mu_stays_in_that_videos_outputs(case, large):
    prob = JC.kernel_problem(case)
    assert prob["mask"][0, 0] == 1 and prob["s2"][1, 0, 0] > 0          # a kept frame that carries information
    y = prob["y"].copy()
    y[1, 0, 0] = np.nan
    a, b = device_run(case, large, JC.PATH_JITTER_DIRECT), run(dict(prob, y=y), large, JC.PATH_JITTER_DIRECT)
    for k in ("p_m", "z"):
        assert np.isnan(b[k][1, :, 0]).all(), k
        assert np.array_equal(b[k][0], a[k][0]) and np.array_equal(b[k][1, :, 1:], a[k][1, :, 1:]), k
    for k in ("cov", "chol"):                                            # neither depends on mu
        assert np.array_equal(b[k], a[k]), k


@pytest.mark.parametrize("large", [False, True], ids=["fused", "large"])
def test_zero_path_jitter_with_two_equal_query_times_gives_nan_where_the_factor_fails_and_nowhere_else(large):
    """A numerical outcome, not a fault.  The first and the last query time are equal.  In the all-dropped video C = SE(tau, tau):
    the first pivot is 1, the last row's first element 1, every later element of it 0 and its pivot 1 - 1 = 0 in exact
    arithmetic of floating-point numbers, so that (video, coordinate)'s factor fails for certain: NaN in the last row of chol
    and in the last z, nowhere before.  In the other videos rounding decides whether the last pivot comes out positive: each
    has either such NaNs from the failing row on or a factor within the residual bound.  p_m and cov never see the factor."""
    case = "3-30-17-33"
    prob = JC.kernel_problem(case)
    tq = prob["tq"].copy()
    tq[-1] = tq[0]
    Q = tq.size
    ok, g = run(prob, large, JC.JITTER, tq=tq), run(prob, large, 0.0, tq=tq)
    assert np.array_equal(g["p_m"], ok["p_m"]) and np.array_equal(g["cov"], ok["cov"]) and np.isfinite(g["cov"]).all()
    assert np.isfinite(ok["chol"]).all() and np.isfinite(ok["z"]).all()
    failed = 0
    for c in range(2):
        for b in range(g["chol"].shape[1]):
            L, z = g["chol"][c, b], g["z"][c, :, b]
            if np.isnan(L).any():
                failed += 1
                assert np.isfinite(L[:Q - 1]).all() and np.isnan(L[Q - 1, Q - 1]) and np.isfinite(z[:Q - 1]).all() and np.isnan(z[Q - 1])
                assert (np.triu(L[:Q - 1], 1) == 0).all()
            else:
                assert (large or b != 1) and np.isfinite(z).all()
                assert np.abs(L @ L.T - g["cov"][c, b]).max() <= JC.chol_residual_bound(g["cov"][c, b])
        if not large:                # the fused kernel's X is 0 exactly there; the large form's inverse promises it at TOL only
            assert np.isnan(g["chol"][c, 1]).any()
    print(f"{'large' if large else 'fused'}: {failed} of {2 * g['chol'].shape[1]} factors failed")


# ---------------------------------------------------------------------------------------------- BallPredictor.predict
def _predictor(p, T, m, px, hidden, jitter, clip_qs, tmax=None):
    from svgp_vae_amd.ball_predict import BallPredictor
    return BallPredictor(p, tmax=T if tmax is None else tmax, m=m, hidden=hidden, px=px, py=px, jitter=jitter, clip_qs=clip_qs)


def _joint_predictor_reference(p, vid, observed, tq, eps, *, jitter, path_jitter):
    """The oracle's MLP forward composed with the joint restatement: dict(frames, p_m, z (B, Q, 2), p_cov (B, 2, Q, Q))."""
    from oracle import pearce_vae_oracle as PO
    B, T, px, py = vid.shape
    mu, var = PO.mlp_inference(p, vid)
    var = torch.clamp(var, 1e-6, 1e3)
    tr = lambda t: np.ascontiguousarray(t.numpy().transpose(2, 1, 0))          # (B, T, 2) -> (2, T, B)
    prob = dict(times=np.arange(1, T + 1, dtype=np.float64), tq=np.asarray(tq, dtype=np.float64),
                ip=np.stack([p["ip_x"].numpy(), p["ip_y"].numpy()]), ls=np.array([float(p["l_x"]), float(p["l_y"])]), y=tr(mu),
                s2=tr(var), mask=np.asarray(observed, dtype=np.float64).T, eps=np.ascontiguousarray(np.asarray(eps).transpose(2, 1, 0)),
                jitter=jitter)
    r = JC.reference_of(prob, path_jitter)
    bq2 = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))                   # (2, Q, B) -> (B, Q, 2)
    frames = torch.sigmoid(PO.mlp_decoder(p, torch.as_tensor(bq2(r["z"])), px, py)).numpy()
    return dict(frames=frames, p_m=bq2(r["p_m"]), z=bq2(r["z"]), p_cov=np.ascontiguousarray(r["cov"].transpose(1, 0, 2, 3)))


@pytest.mark.parametrize("B,T,m,Q", [(3, 30, 15, 40), (2, 30, 65, 20)], ids=["fused", "large"])
def test_predict_paths_and_cov_against_the_oracle_mlps_composed_with_the_restatement(B, T, m, Q):
    px, hidden, jitter, jp = 8, 16, 1e-9, JC.PATH_JITTER_DIRECT
    p, vid, observed, tq, eps = PC.predictor_problem(B, T, m, Q, px=px, hidden=hidden, seed=7 + m, drop_video=1)
    ref = _joint_predictor_reference(p, vid, observed, tq, eps, jitter=jitter, path_jitter=jp)
    marginal = PC.predictor_reference(p, vid, observed, tq, eps, jitter=jitter, clip_qs=True)
    pred = _predictor(p, T, m, px, hidden, jitter, True)
    before = pred.predict(vid, tq, observed=observed, eps=eps)
    state = torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    got = pred.predict(vid, tq, observed=observed, eps=eps, paths=True, return_cov=True, path_jitter=jp)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state[0]) and torch.equal(torch.get_rng_state(), state[1])
    assert set(got) == {"frames", "p_m", "p_v", "z", "p_cov"} and tuple(got["p_cov"].shape) == (B, 2, Q, Q)
    for k in ("frames", "p_m", "z", "p_cov"):
        e = PC.relerr(got[k].cpu().numpy(), ref[k])
        print(f"predict(paths, cov) {k}: {e:.2e}")
        assert e <= PC.TOL, (k, e)
    assert PC.relerr(got["p_v"].cpu().numpy(), marginal["p_v"]) <= PC.TOL
    fr = got["frames"].cpu().numpy()
    assert np.isfinite(fr).all() and fr.min() >= 0 and fr.max() <= 1
    fused = m <= 64 and Q <= 64
    assert pred.route(B, T, Q, joint=True) == JC.expected_route(B, T, m, Q, not fused)
    # the covariance alone leaves today's keys with today's bits; and no state is shared between the calls
    cov_only = pred.predict(vid, tq, observed=observed, eps=eps, return_cov=True, path_jitter=jp)
    after = pred.predict(vid, tq, observed=observed, eps=eps)
    other = _predictor(p, T, m, px, hidden, jitter, True).predict(vid, tq, observed=observed, eps=eps)
    assert set(before) == set(after) == {"frames", "p_m", "p_v", "z"}
    for k in before:
        assert torch.equal(before[k], after[k]) and torch.equal(before[k], other[k]) and torch.equal(before[k], cov_only[k]), k
    assert torch.equal(cov_only["p_cov"], got["p_cov"])
    for k in ("frames", "p_m", "p_v", "z"):
        assert PC.relerr(before[k].cpu().numpy(), marginal[k]) <= PC.TOL, k


def test_predict_raises_on_a_path_that_is_not_finite_and_names_the_videos():
    from svgp_vae_amd._lib import SvgpError
    B, T, m, Q, px, hidden = 3, 30, 15, 8, 8, 16
    p, vid, observed, tq, eps = PC.predictor_problem(B, T, m, Q, px=px, hidden=hidden, seed=3, drop_video=1)
    tq = tq.copy()
    tq[-1] = tq[0]                   # the all-dropped video's factor fails for certain at path_jitter = 0 (see the kernel test)
    pred = _predictor(p, T, m, px, hidden, 1e-9, True)
    with pytest.raises(SvgpError) as e:
        pred.predict(vid, tq, observed=observed, eps=eps, paths=True, path_jitter=0.0)
    assert "video" in str(e.value) and " 1" in str(e.value) and "raise path_jitter" in str(e.value)
    out = pred.predict(vid, tq, observed=observed, eps=eps, paths=True, path_jitter=1e-6)
    assert bool(torch.isfinite(out["z"]).all())


# ---------------------------------------------------------------------------------------------- end to end
def test_sample_paths_and_save_cov_from_the_command_line(tmp_path):
    """One fresh child process under its own time limit, on a checkpoint written here."""
    from svgp_vae_amd import ball_predict as BP
    B, T, m, px, hidden = 3, 12, 5, 8, 16
    p, vid, _, _, _ = PC.predictor_problem(B, T, m, 1, px=px, hidden=hidden, seed=11)
    shapes = BP.param_shapes(m, px, px, hidden)
    theta = torch.cat([torch.as_tensor(p[k], dtype=torch.float64).reshape(-1) for k in shapes])
    ckpt, videos, out, cov = (str(tmp_path / n) for n in ("model.pt", "videos.npy", "frames.npy", "cov.npy"))
    torch.save({"theta": theta, "shapes": {k: tuple(v) for k, v in shapes.items()},
                "meta": dict(elbo="SVGPVAE_Hensman", tmax=T, m=m, hidden=hidden, px=px, py=px, jitter=1e-9, clip_qs=True, vidlt=2.0)}, ckpt)
    np.save(videos, vid.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.ball_predict", "--checkpoint", ckpt, "--videos", videos, "--drop", "0.5",
                        "--upsample", "2", "--sample_paths", "--seed", "4", "--path_jitter", "1e-6", "--save_cov", cov, "--out", out],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    Q = 2 * (T - 1) + 1
    frames, C_ = np.load(out), np.load(cov)
    assert frames.shape == (B, Q, px, px) and np.isfinite(frames).all() and frames.min() >= 0 and frames.max() <= 1
    assert C_.shape == (B, 2, Q, Q) and np.isfinite(C_).all() and np.array_equal(C_, C_.transpose(0, 1, 3, 2))
    assert "route (1 GP launch): k_ball_predict" in r.stdout and "joint route (1 GP launch): k_ball_predict_joint" in r.stdout
    # the same draw through the interface
    observed = np.random.RandomState(0).rand(B, T) >= 0.5
    eps = np.random.RandomState(4).randn(B, Q, 2)
    got = BP.load_predictor(ckpt).predict(vid, BP.query_grid(T, 2)[0], observed=observed, eps=eps, paths=True, return_cov=True,
                                          path_jitter=1e-6)
    assert np.array_equal(got["frames"].cpu().numpy(), frames) and np.array_equal(got["p_cov"].cpu().numpy(), C_)
