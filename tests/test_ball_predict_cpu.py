"""Moving-ball predictor: everything that needs no GPU.  The guards that make the bar of tests/ball_predict_cases.py meaningful, the
restatement anchored to the existing oracle, the C ABI's declarations, exports, refusals, workspace and launch route, and the
driver's checkpoint handling and command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from oracle import ball_oracle as BO
from svgp_vae_amd import _lib
from svgp_vae_amd._lib import BallPredictBufs, BallPredictCfg
from tests import ball_predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_ball_predict", "svgp_ball_predict_large", "svgp_ball_predict_large_workspace_elems", "svgp_ball_predict_route")
FAKE = 4096                          # never dereferenced: every call below fails validation first
REQUIRED = ("times", "tq", "ip_x", "ip_y", "ls_x", "ls_y", "mu_x", "mu_y", "var_x", "var_y", "p_m_x", "p_m_y", "p_v_x", "p_v_y")
OPTIONAL = ("mask", "eps_x", "eps_y", "z_x", "z_y")


# ---------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_restatement_response_to_one_ulp_and_second_summation_order(case):
    prob, ref = PC.kernel_problem(case), PC.kernel_reference(case)
    ulp, flip = PC.reference_of(PC.one_ulp(prob)), PC.kernel_reference(case, True)
    for name, r, u, f in zip(("p_m", "p_v", "z"), ref, ulp, flip):
        assert np.isfinite(r).all()
        e_u, e_f = PC.relerr(u, r), PC.relerr(f, r)
        print(f"{case} {name}: one-ulp response {e_u:.2e}, second order {e_f:.2e}")
        assert e_u <= PC.TOL / 100, (case, name, e_u)
        assert e_f <= PC.TOL / 10, (case, name, e_f)


@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_case_inputs_are_as_specified(case):
    B, T, m, Q = PC.kernel_shape(case)
    p = PC.kernel_problem(case)
    kept_videos = [b for b in range(B) if b != 1]                         # video 1 is the wholly dropped one
    assert (p["mask"][0, kept_videos] == 1).all() and set(np.unique(p["mask"])) <= {0.0, 1.0}
    assert p["s2"][0, 0, 0] == 0 and (np.delete(p["s2"].reshape(-1), 0) >= 1e-3).all() and (p["s2"] <= 1).all()
    assert p["tq"].shape == (Q,) and (p["tq"] >= -2).all() and (p["tq"] <= T + 5).all()
    assert Q < 2 or (np.diff(p["tq"]) < 0).any()                         # unsorted
    if B > 1:
        assert (p["mask"][:, 1] == 0).all()
    rest = p["mask"][1:, kept_videos]                                    # about 40 % of the other frames are dropped
    if rest.size >= 60:
        assert 0.25 <= 1 - rest.mean() <= 0.55, 1 - rest.mean()


@pytest.mark.parametrize("case", ["35-30-15-61", "3-30-17-33", "2-64-64-40", "3-5-1-3"])
def test_restatement_is_the_oracles_posterior_at_the_frame_times(case):
    """tau = t, nothing dropped: SVGP.approximate_posterior_params, mean and diag(B)."""
    p = PC.kernel_problem(case)
    B = p["y"].shape[2]
    p_m, p_v, _ = PC.reference_of(p, use_mask=False, use_eps=False, tq=p["times"])
    for c in range(2):
        sv = BO.BallSVGP(False, torch.as_tensor(p["ip"][c]), torch.tensor(p["ls"][c], dtype=BO.DT), p["jitter"])
        mean, Bm, _, _ = sv.approximate_posterior_params(torch.as_tensor(p["times"]).repeat(B, 1), torch.as_tensor(p["y"][c].T.copy()),
                                                         torch.as_tensor(p["s2"][c].T.copy()))
        e_m = PC.relerr(p_m[c].T, mean.numpy())
        e_v = PC.relerr(p_v[c].T, torch.diagonal(Bm, dim1=1, dim2=2).numpy())
        print(f"{case} coordinate {c}: mean {e_m:.2e}, diag(B) {e_v:.2e}")
        assert e_m <= 1e-10 and e_v <= 1e-10


@pytest.mark.parametrize("case", ["35-30-15-61", "3-30-16-16", "2-64-33-70"])
def test_masked_restatement_is_the_oracle_on_the_kept_frames_only(case):
    p = PC.kernel_problem(case)
    B = p["y"].shape[2]
    worst = 0.0
    for c in range(2):
        sv = BO.BallSVGP(False, torch.as_tensor(p["ip"][c]), torch.tensor(p["ls"][c], dtype=BO.DT), p["jitter"])
        for b in range(B):
            keep = p["mask"][:, b] == 1
            if not keep.any():
                continue
            t = p["times"][keep]
            got = PC.posterior(p["times"], p["y"][c, :, b], p["s2"][c, :, b], p["mask"][:, b], p["ip"][c], p["ls"][c], p["jitter"], t)
            mean, Bm, _, _ = sv.approximate_posterior_params(torch.as_tensor(t)[None], torch.as_tensor(p["y"][c, keep, b])[None],
                                                             torch.as_tensor(p["s2"][c, keep, b])[None])
            worst = max(worst, PC.relerr(got[0], mean[0].numpy()), PC.relerr(got[1], torch.diagonal(Bm[0]).numpy()))
    print(f"{case}: masked against kept-frames-only {worst:.2e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("case", [c for c in PC.KERNEL_IDS if PC.kernel_shape(c)[0] > 1])
def test_all_dropped_video_gives_the_prior(case):
    p_m, p_v, z = PC.kernel_reference(case)
    assert (p_m[:, :, 1] == 0).all() and np.abs(p_v[:, :, 1] - 1).max() <= 1e-10


# ---------------------------------------------------------------------------------------------- ABI
def _cfg(B=3, T=30, m=15, Q=7, jitter=1e-9, lo=PC.CLIP[0], hi=PC.CLIP[1]):
    return BallPredictCfg(B=B, T=T, m=m, Q=Q, jitter=jitter, clip_lo=lo, clip_hi=hi)


def _bufs(**null):
    q = BallPredictBufs()
    for n in REQUIRED:
        setattr(q, n, None if null.get(n) else FAKE)
    return q


def _fused(cfg, bufs):
    return _lib.call("svgp_ball_predict", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), None)


def _large(cfg, bufs, work=FAKE):
    return _lib.call("svgp_ball_predict_large", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), work, None)


def _route(cfg, large, cap=1 << 16):
    buf = C.create_string_buffer(cap)
    _lib.call("svgp_ball_predict_route", None if cfg is None else C.byref(cfg), int(large), buf, cap)
    return buf.value.decode().split()


def test_header_declares_library_exports_and_binding_mirrors_the_structs():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_predict_cfg\s*;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t B, T, m, Q; double jitter, clip_lo, clip_hi;"
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_predict_bufs\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [n for n, _ in BallPredictBufs._fields_]
    assert lib.svgp_struct_sizeof(13) == C.sizeof(BallPredictCfg) == 40
    assert lib.svgp_struct_sizeof(14) == C.sizeof(BallPredictBufs) == 8 * 19
    assert set(REQUIRED) | set(OPTIONAL) == {n for n, _ in BallPredictBufs._fields_}


REFUSALS = [
    (lambda: _fused(None, _bufs()), -1, "cfg is NULL"), (lambda: _fused(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _fused(_cfg(m=0), _bufs()), -1, "m=0"), (lambda: _fused(_cfg(m=65), _bufs()), -2, "m=65"),
    (lambda: _fused(_cfg(T=0), _bufs()), -1, "T=0"), (lambda: _fused(_cfg(T=16385), _bufs()), -2, "T=16385"),
    (lambda: _fused(_cfg(B=0), _bufs()), -1, "B=0"), (lambda: _fused(_cfg(Q=0), _bufs()), -1, "Q=0"),
    (lambda: _fused(_cfg(lo=2.0, hi=1.0), _bufs()), -1, "clip_lo <= clip_hi"),
    (lambda: _large(None, _bufs()), -1, "cfg is NULL"), (lambda: _large(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _large(_cfg(m=0), _bufs()), -1, "m=0"), (lambda: _large(_cfg(m=2049), _bufs()), -2, "m=2049"),
    (lambda: _large(_cfg(T=2049), _bufs()), -2, "T=2049"), (lambda: _large(_cfg(B=0), _bufs()), -1, "B=0"),
    (lambda: _large(_cfg(Q=0), _bufs()), -1, "Q=0"), (lambda: _large(_cfg(lo=2.0, hi=1.0), _bufs()), -1, "clip_lo <= clip_hi"),
    (lambda: _large(_cfg(), _bufs(), work=None), -1, "work is NULL"),
    (lambda: _large(_cfg(m=65), _bufs(), work=None), -1, "work is NULL"),
    (lambda: _route(_cfg(m=65), False), -2, "m=65"), (lambda: _route(_cfg(m=2049), True), -2, "m=2049"),
    (lambda: _route(_cfg(T=2049), True), -2, "T=2049"), (lambda: _route(None, False), -1, "cfg is NULL"),
    (lambda: _lib.call("svgp_ball_predict_route", C.byref(_cfg()), 0, None, 10), -1, "bad argument"),
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


def test_workspace_is_zero_for_a_refused_cfg_and_grows_with_neither_videos_nor_queries_beyond_a_chunk():
    lib = svgp_vae_amd.load_library()
    n = lambda **kw: lib.svgp_ball_predict_large_workspace_elems(C.byref(_cfg(**kw)))
    assert lib.svgp_ball_predict_large_workspace_elems(None) == 0
    for bad in (dict(m=0), dict(m=2049), dict(T=2049), dict(B=0), dict(Q=0), dict(lo=2.0, hi=1.0)):
        assert n(**bad) == 0, bad
    for m in (15, 65, 300):
        assert 0 < n(B=3, m=m) < n(B=64, m=m) == n(B=65, m=m) == n(B=70, m=m) == n(B=100000, m=m)
        assert n(Q=100, m=m) < n(Q=4096, m=m) == n(Q=4097, m=m) == n(Q=10 ** 6, m=m)
    # what a chunk holds: the scaled rows (nb, T, m), (nb + 1) m x m matrices and the inverse's own workspace dominate
    B, T, m, Q = 70, 100, 130, 50
    floor = 64 * T * m + 65 * m * m + lib.svgp_spd_inverse_workspace_elems(m, 65)
    assert floor <= n(B=B, T=T, m=m, Q=Q) <= floor + 3 * m * m + 2 * T * m + 64 * (T + 2 * m + 2 * Q + 4) + Q * (m + 1) + 16 * 20


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_route_of_every_case(case):
    B, T, m, Q = PC.kernel_shape(case)
    if m <= PC.FUSED_M_MAX:
        assert _route(_cfg(B, T, m, Q), False) == ["k_ball_predict"]
    if T <= 2048:
        assert _route(_cfg(B, T, m, Q), True) == PC.expected_route(B, T, m, Q, True)
    from svgp_vae_amd import ball_predict as BP
    assert BP.route((B, T, m, Q)) == PC.expected_route(B, T, m, Q, m > PC.FUSED_M_MAX)


@pytest.mark.parametrize("B,Q,m,windows,qchunks", [(1, 1, 65, 1, 1), (64, 9, 65, 1, 1), (65, 9, 65, 2, 1), (70, 9, 15, 2, 1),
                                                   (129, 9, 65, 3, 1), (3, 4096, 65, 1, 1), (3, 4097, 65, 1, 2), (70, 8193, 300, 2, 3)])
def test_large_route_follows_the_channel_windows_and_query_chunks(B, Q, m, windows, qchunks):
    names = _route(_cfg(B, 30, m, Q), True)
    assert names == PC.expected_route(B, 30, m, Q, True)
    assert names.count("k_bp_scale_rows") == names.count("svgp_spd_inverse_batched") == 2 * windows
    assert names.count("k_sprites_posterior_rows") == names.count("k_bp_finish") == 2 * windows * qchunks
    assert names.count("svgp_se1d_kernel_matrix_fwd") == 2 + 2 * windows * qchunks


def test_fused_route_is_one_launch_whatever_the_batch_and_the_query_count():
    for B, T, Q in [(1, 1, 1), (35, 30, 59), (256, 64, 512), (100000, 16384, 10 ** 6)]:
        for m in (1, 32, 33, 64):
            assert _route(_cfg(B, T, m, Q), False) == ["k_ball_predict"]


# ---------------------------------------------------------------------------------------------- driver
def _checkpoint(tmp_path, name, m=5, hidden=6, px=4, meta=True, pearce=False):
    from svgp_vae_amd import ball_predict as BP
    shapes = dict(BP.param_shapes(m, px, px, hidden))
    if pearce:
        shapes = {k: v for k, v in shapes.items() if not k.startswith("ip_")}
    n = sum(int(np.prod(s)) for s in shapes.values())
    ck = {"theta": torch.arange(n, dtype=torch.float64), "adam_m": torch.zeros(n), "adam_v": torch.zeros(n), "state": torch.zeros(16),
          "shapes": shapes}
    if meta:
        ck["meta"] = dict(elbo="GPVAE_Pearce" if pearce else "SVGPVAE_Hensman", tmax=30, m=m, hidden=hidden, px=px, py=px, jitter=1e-9,
                          clip_qs=True, vidlt=2.0)
    path = str(tmp_path / name)
    torch.save(ck, path)
    return path


def test_load_on_a_checkpoint_without_meta_names_the_missing_keys(tmp_path):
    from svgp_vae_amd import ball_predict as BP
    path = _checkpoint(tmp_path, "old.pt", meta=False)
    with pytest.raises(ValueError) as e:
        BP.BallPredictor.load(path)
    for k in BP.META_KEYS:
        assert k in str(e.value), (k, str(e.value))
    with pytest.raises(ValueError) as e:
        BP.BallPredictor.load(path, tmax=30, m=5, hidden=6, px=4, py=4)
    assert "jitter" in str(e.value) and "clip_qs" in str(e.value) and "hidden" not in str(e.value).split("pass")[1]
    with pytest.raises(ValueError) as e:                                     # every key given, but another model's shape
        BP.BallPredictor.load(path, tmax=30, m=7, hidden=6, px=4, py=4, jitter=1e-9, clip_qs=True)
    assert "ip_x" in str(e.value)


def test_checkpoints_of_the_exact_gp_baselines_and_other_files_are_refused(tmp_path):
    from svgp_vae_amd import ball_predict as BP
    for path in (_checkpoint(tmp_path, "pearce.pt", pearce=True), _checkpoint(tmp_path, "pearce_old.pt", pearce=True, meta=False)):
        with pytest.raises(ValueError) as e:
            BP.BallPredictor.load(path)
        assert "exact-GP baseline" in str(e.value) and "SVGPVAE" in str(e.value)
    other = str(tmp_path / "other.pt")
    torch.save({"w": torch.zeros(3)}, other)
    with pytest.raises(ValueError) as e:
        BP.BallPredictor.load(other)
    assert "other.pt" in str(e.value)


def test_predictor_is_re_exported_from_the_ball_module_and_checks_its_parameters():
    from svgp_vae_amd import ball
    from svgp_vae_amd import ball_predict as BP
    assert ball.BallPredictor is BP.BallPredictor
    with pytest.raises(ValueError) as e:
        BP.BallPredictor({}, tmax=30, m=5, hidden=6, px=4, py=4, jitter=1e-9, clip_qs=False)
    assert "ip_x" in str(e.value)


def test_the_driver_writes_the_meta_dict_the_predictor_reads():
    """BALL_experiment --save_model: the keys load() looks for are exactly those the driver writes."""
    from svgp_vae_amd import ball_predict as BP
    src = open(os.path.join(ROOT, "svgp-vae_amd", "BALL_experiment.py")).read()
    meta = re.search(r'"meta":\s*dict\((.*?)\)\}', src, flags=re.S).group(1)
    keys = re.findall(r"(\w+)=", meta)
    assert set(keys) == set(BP.META_KEYS) | {"elbo", "vidlt"}


BASE = ["--checkpoint", "run/model.pt", "--out", "frames.npy"]


@pytest.mark.parametrize("extra", [[], ["--videos", "v.npy", "--test_batch", "0", "--base_dir", "d"], ["--test_batch", "0"],
                                   ["--test_batch", "10", "--base_dir", "d"], ["--videos", "v.npy", "--drop", "0.5", "--observed", "m.npy"],
                                   ["--videos", "v.npy", "--upsample", "2", "--query_times", "1.5"], ["--videos", "v.npy", "--drop", "1.0"],
                                   ["--videos", "v.npy", "--upsample", "0"]])
def test_cli_refuses_inconsistent_arguments(extra):
    from svgp_vae_amd import ball_predict as BP
    with pytest.raises(SystemExit) as e:
        BP.parse_args(BASE + extra)
    assert e.value.code == 2


def test_cli_parser_and_query_grid():
    from svgp_vae_amd import ball_predict as BP
    a = BP.parse_args(BASE + ["--test_batch", "0", "--base_dir", "d", "--drop", "0.5", "--drop_seed", "3", "--upsample", "2"])
    assert (a.test_batch, a.base_dir, a.drop, a.drop_seed, a.upsample, a.sample, a.videos) == (0, "d", 0.5, 3, 2, False, None)
    a = BP.parse_args(BASE + ["--videos", "v.npy", "--observed", "m.npy", "--query_times", "0.5", "31", "2.25", "--sample", "--seed", "4"])
    assert a.query_times == [0.5, 31.0, 2.25] and a.sample and a.seed == 4 and a.observed == "m.npy" and a.drop is None
    tq, at = BP.query_grid(30, upsample=2)
    assert tq.shape == (59,) and tq[0] == 1 and tq[-1] == 30 and np.array_equal(tq[at], np.arange(1, 31))
    tq, at = BP.query_grid(30)
    assert np.array_equal(tq, np.arange(1, 31)) and np.array_equal(at, np.arange(30))
    tq, at = BP.query_grid(30, query_times=[31.0, 0.5])
    assert np.array_equal(tq, [31.0, 0.5]) and at is None
