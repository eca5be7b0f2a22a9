"""Moving-ball joint predictor: everything that needs no GPU.  The guards that make the bar of tests/ball_joint_cases.py meaningful,
the restatement anchored to the marginal one and to the oracle's full covariance, the C ABI's declarations, exports, refusals,
workspace and launch route, and the predictor's argument checks and command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from oracle import ball_oracle as BO
from svgp_vae_amd import _lib
from tests import ball_joint_cases as JC
from tests import ball_predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_ball_predict_joint", "svgp_ball_predict_joint_large", "svgp_ball_predict_joint_large_workspace_elems",
               "svgp_ball_predict_joint_route")
FAKE = 4096                          # never dereferenced: every call below fails validation first
REQUIRED = ("times", "tq", "ip_x", "ip_y", "ls_x", "ls_y", "mu_x", "mu_y", "var_x", "var_y", "p_m_x", "p_m_y")
OPTIONAL = ("mask", "eps_x", "eps_y", "cov_x", "cov_y", "chol_x", "chol_y", "z_x", "z_y")


# ---------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("case", JC.KERNEL_IDS)
def test_restatement_response_to_one_ulp_and_second_summation_order(case):
    """cov and p_m at any path_jitter; z and chol at PATH_JITTER_DIRECT, where the GPU test compares them directly."""
    prob, ref = JC.kernel_problem(case), JC.kernel_reference(case)
    ulp, flip = JC.reference_of(JC.one_ulp(prob), JC.PATH_JITTER_DIRECT), JC.kernel_reference(case, JC.PATH_JITTER_DIRECT, True)
    for name in ("p_m", "cov", "z", "chol"):
        assert np.isfinite(ref[name]).all()
        e_u, e_f = JC.relerr(ulp[name], ref[name]), JC.relerr(flip[name], ref[name])
        print(f"{case} {name}: one-ulp response {e_u:.2e}, second order {e_f:.2e}")
        assert e_u <= JC.TOL / 100, (case, name, e_u)
        assert e_f <= JC.TOL / 10, (case, name, e_f)


@pytest.mark.parametrize("case", JC.KERNEL_IDS)
def test_cov_is_symmetric_and_its_diagonal_is_the_marginal_restatements_p_v(case):
    prob, ref = JC.kernel_problem(case), JC.kernel_reference(case)
    p_m, p_v, _ = PC.reference_of(prob)
    assert np.array_equal(ref["cov"], ref["cov"].transpose(0, 1, 3, 2))
    e_v = JC.relerr(np.diagonal(ref["cov"], axis1=2, axis2=3).transpose(0, 2, 1), p_v)
    e_m = JC.relerr(ref["p_m"], p_m)
    print(f"{case}: diag(cov) against p_v {e_v:.2e}, p_m {e_m:.2e}")
    assert e_v <= JC.TOL / 10 and e_m == 0
    mean = JC.reference_of(prob, JC.PATH_JITTER_DIRECT, use_eps=False)
    assert np.array_equal(mean["z"], mean["p_m"])


@pytest.mark.parametrize("case", ["35-30-15-61", "3-30-17-33", "2-64-64-64", "3-5-1-3"])
def test_cov_is_the_oracles_full_covariance_at_the_frame_times(case):
    """tau = t, nothing dropped: the full B of SVGP.approximate_posterior_params (SVGPVAE_model.py:141-171)."""
    p = JC.kernel_problem(case)
    B = p["y"].shape[2]
    ref = JC.reference_of(p, JC.JITTER, use_mask=False, use_eps=False, tq=p["times"])
    for c in range(2):
        sv = BO.BallSVGP(False, torch.as_tensor(p["ip"][c]), torch.tensor(p["ls"][c], dtype=BO.DT), p["jitter"])
        mean, Bm, _, _ = sv.approximate_posterior_params(torch.as_tensor(p["times"]).repeat(B, 1), torch.as_tensor(p["y"][c].T.copy()),
                                                         torch.as_tensor(p["s2"][c].T.copy()))
        assert tuple(Bm.shape) == (B, p["times"].size, p["times"].size)
        e_m, e_c = JC.relerr(ref["p_m"][c].T, mean.numpy()), JC.relerr(ref["cov"][c], Bm.numpy())
        print(f"{case} coordinate {c}: mean {e_m:.2e}, B {e_c:.2e}")
        assert e_m <= 1e-10 and e_c <= 1e-10


@pytest.mark.parametrize("case", [c for c in JC.KERNEL_IDS if JC.kernel_shape(c)[0] > 1])
def test_all_dropped_video_has_the_prior_covariance(case):
    p, ref = JC.kernel_problem(case), JC.kernel_reference(case)
    assert (ref["p_m"][:, :, 1] == 0).all()
    for c in range(2):
        assert JC.relerr(ref["cov"][c, 1], JC.se(p["tq"], p["tq"], p["ls"][c])) <= 1e-10


def test_chol_bound_constant_and_case_table_are_as_specified():
    assert JC.CHOL_C == 4.0 and JC.TOL == 1e-8 and JC.JITTER == 1e-9 and JC.PATH_JITTER_DIRECT == 1e-4
    assert JC.KERNEL_IDS == ["1-1-1-1", "3-5-1-3", "2-2-3-4", "3-30-16-16", "3-30-17-33", "35-30-15-61", "2-64-64-64", "2-64-33-70",
                             "2-100-65-40", "70-30-15-9", "3-12-5-700"]
    assert [JC.is_fused(c) for c in JC.KERNEL_IDS] == [True] * 7 + [False, False, True, False]
    A = np.diag([1.0, 2.0, 3.0])
    assert JC.chol_residual_bound(A) == 4.0 * 3 * 2.0 ** -53 * 3.0


# ---------------------------------------------------------------------------------------------- ABI
def _cfg(B=3, T=30, m=15, Q=7, jitter=1e-9, jp=1e-9):
    return _lib.BallPredictJointCfg(B=B, T=T, m=m, Q=Q, jitter=jitter, path_jitter=jp)


def _bufs(**null):
    q = _lib.BallPredictJointBufs()
    for n in REQUIRED:
        setattr(q, n, None if null.get(n) else FAKE)
    return q


def _fused(cfg, bufs):
    return _lib.call("svgp_ball_predict_joint", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), None)


def _large(cfg, bufs, work=FAKE):
    return _lib.call("svgp_ball_predict_joint_large", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), work,
                     None)


def _route(cfg, large, cap=1 << 16):
    buf = C.create_string_buffer(cap)
    _lib.call("svgp_ball_predict_joint_route", None if cfg is None else C.byref(cfg), int(large), buf, cap)
    return buf.value.decode().split()


def test_header_declares_library_exports_and_binding_mirrors_the_structs():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_predict_joint_cfg\s*;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t B, T, m, Q; double jitter, path_jitter;"
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_predict_joint_bufs\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [n for n, _ in _lib.BallPredictJointBufs._fields_]
    assert lib.svgp_struct_sizeof(22) == C.sizeof(_lib.BallPredictJointCfg) == 32
    assert lib.svgp_struct_sizeof(23) == C.sizeof(_lib.BallPredictJointBufs) == 8 * 21
    assert lib.svgp_struct_sizeof(24) == -1
    assert set(REQUIRED) | set(OPTIONAL) == {n for n, _ in _lib.BallPredictJointBufs._fields_}
    # the marginal entry's inputs, in its order, come first
    marginal = [n for n, _ in _lib.BallPredictBufs._fields_]
    assert [n for n, _ in _lib.BallPredictJointBufs._fields_][:13] == marginal[:13]


REFUSALS = [
    (lambda: _fused(None, _bufs()), -1, "cfg is NULL"), (lambda: _fused(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _fused(_cfg(m=0), _bufs()), -1, "m=0"), (lambda: _fused(_cfg(m=65), _bufs()), -2, "m=65"),
    (lambda: _fused(_cfg(T=0), _bufs()), -1, "T=0"), (lambda: _fused(_cfg(T=16385), _bufs()), -2, "T=16385"),
    (lambda: _fused(_cfg(B=0), _bufs()), -1, "B=0"), (lambda: _fused(_cfg(Q=0), _bufs()), -1, "Q=0"),
    (lambda: _fused(_cfg(Q=65), _bufs()), -2, "Q=65"), (lambda: _fused(_cfg(jp=-1e-9), _bufs()), -1, "path_jitter >= 0"),
    (lambda: _fused(_cfg(jp=float("nan")), _bufs()), -1, "path_jitter >= 0"),
    (lambda: _large(None, _bufs()), -1, "cfg is NULL"), (lambda: _large(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _large(_cfg(m=0), _bufs()), -1, "m=0"), (lambda: _large(_cfg(m=2049), _bufs()), -2, "m=2049"),
    (lambda: _large(_cfg(T=2049), _bufs()), -2, "T=2049"), (lambda: _large(_cfg(Q=2049), _bufs()), -2, "Q=2049"),
    (lambda: _large(_cfg(B=0), _bufs()), -1, "B=0"), (lambda: _large(_cfg(Q=0), _bufs()), -1, "Q=0"),
    (lambda: _large(_cfg(jp=-1.0), _bufs()), -1, "path_jitter >= 0"),
    (lambda: _large(_cfg(), _bufs(), work=None), -1, "work is NULL"),
    (lambda: _large(_cfg(m=65, Q=70), _bufs(), work=None), -1, "work is NULL"),
    (lambda: _route(_cfg(m=65), False), -2, "m=65"), (lambda: _route(_cfg(Q=65), False), -2, "Q=65"),
    (lambda: _route(_cfg(m=2049), True), -2, "m=2049"), (lambda: _route(_cfg(Q=2049), True), -2, "Q=2049"),
    (lambda: _route(_cfg(T=2049), True), -2, "T=2049"), (lambda: _route(None, False), -1, "cfg is NULL"),
    (lambda: _lib.call("svgp_ball_predict_joint_route", C.byref(_cfg()), 0, None, 10), -1, "bad argument"),
    (lambda: _route(_cfg(), False, cap=4), -1, "route text"), (lambda: _route(_cfg(), True, cap=40), -1, "route text"),
]
REFUSALS += [(lambda n=n: _fused(_cfg(), _bufs(**{n: True})), -1, "NULL device pointer") for n in REQUIRED]
REFUSALS += [(lambda n=n: _large(_cfg(), _bufs(**{n: True})), -1, "NULL device pointer") for n in REQUIRED]


@pytest.mark.parametrize("call,code,message", REFUSALS)
def test_refusals_carry_their_code_and_a_message_and_launch_nothing(call, code, message):
    """Before any pointer is looked at: the pointers here are fake and there is no device."""
    with pytest.raises(_lib.SvgpError) as e:
        call()
    assert f"status {code}:" in str(e.value) and message in str(e.value), (message, str(e.value))


def test_workspace_is_zero_for_a_refused_cfg_and_grows_with_neither_videos_nor_the_covariance_block_beyond_a_chunk():
    lib = svgp_vae_amd.load_library()
    n = lambda **kw: lib.svgp_ball_predict_joint_large_workspace_elems(C.byref(_cfg(**kw)))
    assert lib.svgp_ball_predict_joint_large_workspace_elems(None) == 0
    for bad in (dict(m=0), dict(m=2049), dict(T=2049), dict(Q=2049), dict(B=0), dict(Q=0), dict(jp=-1.0)):
        assert n(**bad) == 0, bad
    for m, Q in ((15, 9), (65, 40), (15, 70)):
        assert 0 < n(B=3, m=m, Q=Q) < n(B=64, m=m, Q=Q) == n(B=65, m=m, Q=Q) == n(B=70, m=m, Q=Q) == n(B=100000, m=m, Q=Q)
    # the chunk is capped by the covariance block: at Q = 2048 one video, at Q = 1024 four
    assert n(B=1, m=4, T=8, Q=2048) == n(B=9, m=4, T=8, Q=2048) == n(B=100000, m=4, T=8, Q=2048)
    assert n(B=3, m=4, T=8, Q=1024) < n(B=4, m=4, T=8, Q=1024) == n(B=5, m=4, T=8, Q=1024) == n(B=64, m=4, T=8, Q=1024)
    for B, Q in ((9, 2048), (64, 1024), (64, 700), (64, 256), (7, 300)):
        nb = JC.chunk(B, Q)
        assert nb * Q * Q <= max(JC.CAP, Q * Q)
        assert nb * Q * Q <= n(B=B, m=4, T=8, Q=Q) <= (nb * Q * Q + lib.svgp_potrf_workspace_elems(Q, nb) + lib.svgp_spd_inverse_workspace_elems(4, nb + 1)
                                                          + 200 * nb * Q + 4096)


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("case", JC.KERNEL_IDS + ["9-8-4-2048"])
def test_route_of_every_case(case):
    B, T, m, Q = JC.kernel_shape(case)
    fused = m <= JC.FUSED_M_MAX and Q <= JC.FUSED_Q_MAX
    if fused:
        assert _route(_cfg(B, T, m, Q), False) == ["k_ball_predict_joint"]
    names = _route(_cfg(B, T, m, Q), True)
    assert names == JC.expected_route(B, T, m, Q, True)
    chunks = -(-B // JC.chunk(B, Q))
    assert names.count("svgp_potrf_batched") == names.count("k_bpj_cov") == names.count("k_bpj_finish") == 2 * chunks
    assert names.count("svgp_se1d_kernel_matrix_fwd") == 2 + 2 * chunks and names.count("svgp_dgemm_batched") == 2 * 5 * chunks
    from svgp_vae_amd import ball_predict as BP
    assert BP.route((B, T, m, Q), joint=True) == JC.expected_route(B, T, m, Q, not fused)
    assert BP.route((B, T, m, Q)) == PC.expected_route(B, T, m, Q, m > PC.FUSED_M_MAX)           # the marginal route is as it was


def test_chunk_of_the_large_route():
    assert [JC.chunk(*s) for s in [(9, 2048), (9, 1449), (9, 1448), (9, 1024), (70, 9), (3, 700), (64, 256), (64, 257)]] == \
        [1, 1, 2, 4, 64, 3, 64, 63]
    assert _route(_cfg(9, 8, 4, 2048), True).count("svgp_potrf_batched") == 18
    assert _route(_cfg(70, 30, 15, 9), True).count("svgp_potrf_batched") == 4


def test_fused_route_is_one_launch_whatever_the_batch():
    for B, T in [(1, 1), (35, 30), (256, 64), (100000, 16384)]:
        for m, Q in ((1, 1), (32, 64), (33, 1), (64, 64)):
            assert _route(_cfg(B, T, m, Q), False) == ["k_ball_predict_joint"]


# ---------------------------------------------------------------------------------------------- predictor and command line
def _bare(cls, **attrs):
    """An instance without a device: `predict` checks its arguments before it touches one."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_predict_checks_the_joint_arguments_before_anything_else():
    from svgp_vae_amd import ball_predict as BP
    vid, tq = np.zeros((2, 5, 4, 4)), np.arange(3.0)
    sparse = _bare(BP.BallPredictor, jitter=1e-9, px=4, py=4)
    with pytest.raises(ValueError, match="paths=True needs eps"):
        sparse.predict(vid, tq, paths=True)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="path_jitter"):
            sparse.predict(vid, tq, return_cov=True, path_jitter=bad)
    with pytest.raises(ValueError, match="path_jitter applies"):
        sparse.predict(vid, tq, path_jitter=1e-4)
    exact = _bare(BP.PearcePredictor, px=4, py=4)
    for kw in (dict(paths=True, eps=np.zeros((2, 3, 2))), dict(return_cov=True)):
        with pytest.raises(NotImplementedError, match="BallPredictor"):
            exact.predict(vid, tq, **kw)
    assert BP.joint_is_fused(64, 64) and not BP.joint_is_fused(65, 64) and not BP.joint_is_fused(64, 65)


BASE = ["--checkpoint", "run/model.pt", "--out", "frames.npy", "--videos", "v.npy"]


@pytest.mark.parametrize("extra", [["--sample", "--sample_paths"], ["--sample_paths", "--path_jitter", "-1e-4"], ["--path_jitter", "1e-4"],
                                   ["--sample", "--path_jitter", "1e-4"], ["--save_cov"]])
def test_cli_refuses_inconsistent_joint_arguments(extra):
    from svgp_vae_amd import ball_predict as BP
    with pytest.raises(SystemExit) as e:
        BP.parse_args(BASE + extra)
    assert e.value.code == 2


def test_cli_parser_of_the_joint_arguments():
    from svgp_vae_amd import ball_predict as BP
    a = BP.parse_args(BASE)
    assert not a.sample and BP.joint_args(a) == (False, None, None)
    a = BP.parse_args(BASE + ["--sample_paths", "--seed", "4", "--path_jitter", "1e-4", "--save_cov", "cov.npy", "--upsample", "2"])
    assert (a.sample, a.seed, a.upsample) == (False, 4, 2) and BP.joint_args(a) == (True, 1e-4, "cov.npy")
    a = BP.parse_args(BASE + ["--save_cov", "cov.npy", "--path_jitter", "0"])
    assert BP.joint_args(a) == (False, 0.0, "cov.npy")
    a = BP.parse_args(BASE + ["--sample", "--save_cov", "cov.npy"])
    assert a.sample and BP.joint_args(a) == (False, None, "cov.npy")


def test_cli_refuses_an_exact_gp_checkpoint_with_the_joint_arguments(tmp_path, monkeypatch):
    """Told by the checkpoint's family, before any video is read or any device touched."""
    from svgp_vae_amd import ball_predict as BP
    monkeypatch.setattr(BP, "load_predictor", lambda path, **kw: _bare(BP.PearcePredictor))
    for extra in (["--sample_paths"], ["--save_cov", str(tmp_path / "c.npy")], ["--sample_paths", "--path_jitter", "1e-4"]):
        with pytest.raises(SystemExit) as e:
            BP.main(BASE + extra)
        assert "sparse-GP checkpoint" in str(e.value) and "exact-GP" in str(e.value)
