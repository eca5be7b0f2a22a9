"""Exact-GP moving-ball predictor: everything that needs no GPU.  The guards that make the bar of tests/pearce_predict_cases.py
meaningful, the C ABI's declarations, exports, refusals, workspace and launch route, and the checkpoint handling and command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import svgp_vae_amd
from svgp_vae_amd import _lib
from tests import pearce_predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_pearce_predict", "svgp_pearce_predict_long", "svgp_pearce_predict_long_workspace_elems", "svgp_pearce_predict_route")
FAKE = 4096                          # never dereferenced: every call below fails validation first
REQUIRED = ("times", "tq", "ls_x", "ls_y", "mu_x", "mu_y", "var_x", "var_y", "p_m_x", "p_m_y", "p_v_x", "p_v_y")
OPTIONAL = ("mask", "eps_x", "eps_y", "z_x", "z_y", "lh")


# ---------------------------------------------------------------------------------------------- the references themselves
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_two_float64_formulations_and_the_one_ulp_response_stay_within_a_hundredth_of_the_bar(case):
    prob, ref = PC.kernel_problem(case), PC.kernel_reference(case)
    second, ulp = PC.reference_of(prob, form=PC.masked_inverse), PC.reference_of(PC.one_ulp_var(prob))
    print(f"{case}: cond(A) <= {PC.condition_number(prob):.3g}")
    for name in ("p_m", "p_v", "z", "lh"):
        assert np.isfinite(ref[name]).all()
        e_s, e_u = PC.relerr(second[name], ref[name]), PC.relerr(ulp[name], ref[name])
        print(f"{case} {name}: second formulation {e_s:.2e}, one-ulp response {e_u:.2e}")
        assert e_s <= PC.TOL / 100, (case, name, e_s)
        assert e_u <= PC.TOL / 100, (case, name, e_u)


@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_case_inputs_are_as_specified(case):
    B, T, Q = PC.kernel_shape(case)
    p = PC.kernel_problem(case)
    assert p["y"].shape == p["s2"].shape == (2, T, B) and p["mask"].shape == (T, B) and p["eps"].shape == (2, Q, B)
    assert (p["s2"] >= 0.01).all() and (p["s2"] <= 1).all() and set(np.unique(p["mask"])) <= {0.0, 1.0}
    assert np.array_equal(p["times"], np.arange(1, T + 1)) and (p["ls"] == (8.0 if case == PC.LS8_CASE else 2.0)).all()
    assert p["tq"].shape == (Q,) and (p["tq"] >= -2).all() and (p["tq"] <= T + 3).all() and np.isin(p["tq"], p["times"]).any()
    assert p["mask"][:, 0].sum() >= 1
    if B > 1:
        assert (p["mask"][:, 1] == 0).all()
    if B > 2:
        assert p["mask"][:, 2].sum() == 1
    rest = p["mask"][:, [b for b in range(B) if b not in (1, 2)]]
    if rest.size >= 60:
        assert 0.4 <= rest.mean() <= 0.8, rest.mean()
    assert PC.condition_number(p) <= (5e3 if case == PC.LS8_CASE else 3.3e2)


def test_case_table_is_the_specified_one():
    assert PC.FUSED_CASES == [(1, 1, 1), (2, 2, 3), (3, 5, 4), (2, 32, 5), (2, 33, 5), (2, 64, 70), (3, 64, 300), (35, 30, 59)]
    assert PC.LONG_ONLY_CASES == [(2, 65, 5), (2, 130, 7), (1, 300, 4), (PC.NB + 1, 65, 3)]
    assert [PC.entries(c) for c in PC.KERNEL_IDS] == [[False, True]] * 8 + [[True]] * 4


@pytest.mark.parametrize("case", [c for c in PC.KERNEL_IDS if PC.kernel_shape(c)[0] > 1])
def test_all_dropped_video_gives_the_prior_and_dropped_frames_are_never_read(case):
    prob, ref = PC.kernel_problem(case), PC.kernel_reference(case)
    assert (ref["p_m"][:, :, 1] == 0).all() and (ref["p_v"][:, :, 1] == 1).all() and (ref["lh"][:, 1] == 0).all()
    nan = np.where(prob["mask"][None] == 0, np.nan, 1.0)
    for form in (PC.posterior, PC.masked_inverse):
        a, b = PC.reference_of(prob, form=form), PC.reference_of(dict(prob, y=prob["y"] * nan, s2=prob["s2"] * nan), form=form)
        for k in a:
            assert np.array_equal(a[k], b[k]), (form.__name__, k)


# ---------------------------------------------------------------------------------------------- ABI
def _cfg(B=3, T=30, Q=7, q_slices=0):
    return _lib.PearcePredictCfg(B=B, T=T, Q=Q, q_slices=q_slices)


def _bufs(**null):
    q = _lib.PearcePredictBufs()
    for n in REQUIRED:
        setattr(q, n, None if null.get(n) else FAKE)
    return q


def _fused(cfg, bufs):
    return _lib.call("svgp_pearce_predict", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), None)


def _long(cfg, bufs, work=FAKE):
    return _lib.call("svgp_pearce_predict_long", None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), work, None)


def _route(cfg, long_form, cap=1 << 16):
    buf = C.create_string_buffer(cap)
    _lib.call("svgp_pearce_predict_route", None if cfg is None else C.byref(cfg), int(long_form), buf, cap)
    return buf.value.decode().split()


def test_header_declares_library_exports_and_binding_mirrors_the_structs():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_pearce_predict_cfg\s*;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t B, T, Q, q_slices;"
    assert [n for n, _ in _lib.PearcePredictCfg._fields_] == ["B", "T", "Q", "q_slices"]
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_pearce_predict_bufs\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [n for n, _ in _lib.PearcePredictBufs._fields_]
    assert lib.svgp_struct_sizeof(15) == C.sizeof(_lib.PearcePredictCfg) == 16
    assert lib.svgp_struct_sizeof(16) == C.sizeof(_lib.PearcePredictBufs) == 8 * 18
    assert lib.svgp_struct_sizeof(12) == -1 and lib.svgp_struct_sizeof(17) == -1
    assert set(REQUIRED) | set(OPTIONAL) == {n for n, _ in _lib.PearcePredictBufs._fields_}


REFUSALS = [
    (lambda: _fused(None, _bufs()), -1, "cfg is NULL"), (lambda: _fused(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _fused(_cfg(T=0), _bufs()), -1, "T=0"), (lambda: _fused(_cfg(T=65), _bufs()), -2, "T=65: svgp_pearce_predict takes T <= 64"),
    (lambda: _fused(_cfg(B=0), _bufs()), -1, "B=0"), (lambda: _fused(_cfg(Q=0), _bufs()), -1, "Q=0"),
    (lambda: _fused(_cfg(q_slices=-1), _bufs()), -1, "q_slices=-1"), (lambda: _fused(_cfg(Q=7, q_slices=8), _bufs()), -1, "q_slices=8"),
    (lambda: _long(None, _bufs()), -1, "cfg is NULL"), (lambda: _long(_cfg(), None), -1, "bufs is NULL"),
    (lambda: _long(_cfg(T=0), _bufs()), -1, "T=0"), (lambda: _long(_cfg(T=2049), _bufs()), -2, "T=2049: svgp_pearce_predict_long takes T <= 2048"),
    (lambda: _long(_cfg(B=0), _bufs()), -1, "B=0"), (lambda: _long(_cfg(Q=0), _bufs()), -1, "Q=0"),
    (lambda: _long(_cfg(q_slices=-1), _bufs()), -1, "q_slices=-1"), (lambda: _long(_cfg(Q=7, q_slices=8), _bufs()), -1, "q_slices=8"),
    (lambda: _long(_cfg(), _bufs(), work=None), -1, "work is NULL"), (lambda: _long(_cfg(T=65), _bufs(), work=None), -1, "work is NULL"),
    (lambda: _route(_cfg(T=65), False), -2, "T=65"), (lambda: _route(_cfg(T=2049), True), -2, "T=2049"),
    (lambda: _route(_cfg(Q=0), True), -1, "Q=0"), (lambda: _route(None, False), -1, "cfg is NULL"),
    (lambda: _route(_cfg(q_slices=9), False), -1, "q_slices=9"),
    (lambda: _lib.call("svgp_pearce_predict_route", C.byref(_cfg()), 0, None, 10), -1, "bad argument"),
    (lambda: _lib.call("svgp_pearce_predict_route", C.byref(_cfg()), 0, C.create_string_buffer(8), 0), -1, "bad argument"),
    (lambda: _route(_cfg(), False, cap=4), -1, "route text"), (lambda: _route(_cfg(), True, cap=40), -1, "route text"),
]
REFUSALS += [(lambda n=n: _fused(_cfg(), _bufs(**{n: True})), -1, "NULL device pointer") for n in REQUIRED]
REFUSALS += [(lambda n=n: _long(_cfg(), _bufs(**{n: True})), -1, "NULL device pointer") for n in REQUIRED]


@pytest.mark.parametrize("call,code,message", REFUSALS)
def test_refusals_carry_their_code_and_a_message_and_launch_nothing(call, code, message):
    """Before any pointer is looked at: the pointers here are fake and there is no device."""
    with pytest.raises(_lib.SvgpError) as e:
        call()
    assert f"status {code}:" in str(e.value) and message in str(e.value), (message, str(e.value))


def test_workspace_is_zero_for_a_refused_cfg_and_grows_with_neither_videos_nor_queries_beyond_a_chunk():
    lib = svgp_vae_amd.load_library()
    n = lambda **kw: lib.svgp_pearce_predict_long_workspace_elems(C.byref(_cfg(**kw)))
    assert lib.svgp_pearce_predict_long_workspace_elems(None) == 0
    for bad in (dict(T=0), dict(T=2049), dict(B=0), dict(Q=0), dict(q_slices=-1), dict(Q=3, q_slices=4)):
        assert n(**bad) == 0, bad
    for T in (5, 65, 300):
        assert 0 < n(B=3, T=T) < n(B=PC.NB, T=T) == n(B=PC.NB + 1, T=T) == n(B=70, T=T) == n(B=100000, T=T)
        assert n(Q=100, T=T) < n(Q=PC.QC, T=T) == n(Q=PC.QC + 1, T=T) == n(Q=10 ** 6, T=T)
    # what a chunk holds: 2 NB matrices, the inverse's own workspace, and two (2 NB, nq, T) blocks of query rows
    B, T, Q = 70, 130, 50
    floor = 2 * PC.NB * T * T + lib.svgp_spd_inverse_workspace_elems(T, 2 * PC.NB) + 2 * 2 * PC.NB * Q * T
    assert floor <= n(B=B, T=T, Q=Q) <= floor + 2 * PC.NB * (2 * T + 1) + 16 * 8


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("case", PC.KERNEL_IDS)
def test_route_of_every_case(case):
    from svgp_vae_amd import ball_predict as BP
    B, T, Q = PC.kernel_shape(case)
    for long_form in PC.entries(case):
        assert _route(_cfg(B, T, Q), long_form) == PC.expected_route(B, T, Q, long_form)
    assert BP.pearce_route((B, T, Q)) == PC.expected_route(B, T, Q, T > PC.FUSED_T_MAX)


@pytest.mark.parametrize("B,Q,chunks,qchunks", [(1, 1, 1, 1), (8, 9, 1, 1), (9, 9, 2, 1), (17, 512, 3, 1), (3, 513, 1, 2), (20, 1025, 3, 3)])
def test_long_route_follows_the_video_chunks_and_query_chunks(B, Q, chunks, qchunks):
    names = _route(_cfg(B, 70, Q), True)
    assert names == PC.expected_route(B, 70, Q, True)
    assert names.count("k_pp_build") == names.count("svgp_spd_inverse_batched") == names.count("k_pp_alpha") == chunks
    assert names.count("svgp_dgemm_batched") == names.count("k_pp_finish") == chunks * qchunks


def test_fused_route_is_one_launch_whatever_the_batch_the_query_count_and_the_slices():
    for B, T, Q in [(1, 1, 1), (35, 30, 59), (256, 64, 512), (100000, 64, 10 ** 6)]:
        for s in (0, 1, min(Q, 3)):
            assert _route(_cfg(B, T, Q, s), False) == ["k_pearce_predict"]


# ---------------------------------------------------------------------------------------------- checkpoints
def _checkpoint(tmp_path, name, elbo="GPVAE_Pearce", m=5, hidden=6, px=4, meta=True):
    from svgp_vae_amd import ball_predict as BP
    sparse = elbo.startswith("SVGPVAE")
    shapes = dict(BP.param_shapes(m, px, px, hidden)) if sparse else dict(BP.pearce_param_shapes(px, px, hidden))
    n = sum(int(np.prod(s)) for s in shapes.values())
    ck = {"theta": torch.arange(n, dtype=torch.float64), "adam_m": torch.zeros(n), "adam_v": torch.zeros(n), "state": torch.zeros(16),
          "shapes": shapes}
    if meta:                          # the dict BALL_experiment --save_model writes
        ck["meta"] = dict(elbo=elbo, tmax=30, m=m, hidden=hidden, px=px, py=px, jitter=1e-9, clip_qs=False, vidlt=2.0)
    path = str(tmp_path / name)
    torch.save(ck, path)
    return path


def _accepted(make, cls_name):
    """The checkpoint passed every check: with a device the predictor exists, without one its constructor says so."""
    try:
        pred = make()
    except _lib.SvgpError as e:
        assert f"{cls_name} needs a HIP device" in str(e), str(e)
        return None
    assert type(pred).__name__ == cls_name
    return pred


@pytest.mark.parametrize("elbo", ["GPVAE_Pearce", "NP", "VAE"])
def test_exact_gp_checkpoints_are_accepted_from_the_meta_the_driver_writes(tmp_path, elbo):
    from svgp_vae_amd import ball_predict as BP
    path = _checkpoint(tmp_path, "p.pt", elbo=elbo)
    pred = _accepted(lambda: BP.PearcePredictor.load(path), "PearcePredictor")
    _accepted(lambda: BP.load_predictor(path), "PearcePredictor")
    if pred is not None:
        assert (pred.tmax, pred.H, pred.px, pred.py) == (30, 6, 4, 4) and list(pred.shapes) == list(BP.pearce_param_shapes(4, 4, 6))
        n = sum(int(np.prod(s)) for s in pred.shapes.values())
        assert float(pred.params["l_x"][0]) == n - 2 and float(pred.params["l_y"][0]) == n - 1       # theta = 0, 1, 2, ...
    with pytest.raises(ValueError) as e:                                     # BallPredictor refuses it as before, and says where to go
        BP.BallPredictor.load(path)
    assert "exact-GP baseline" in str(e.value) and "PearcePredictor" in str(e.value)


def test_sparse_checkpoints_are_refused_by_the_exact_gp_predictor_and_dispatched_by_load_predictor(tmp_path):
    from svgp_vae_amd import ball_predict as BP
    for name, kw in (("s.pt", dict()), ("s_old.pt", dict(meta=False))):
        path = _checkpoint(tmp_path, name, elbo="SVGPVAE_Hensman", **kw)
        with pytest.raises(ValueError) as e:
            BP.PearcePredictor.load(path)
        assert "sparse-GP" in str(e.value) and "BallPredictor" in str(e.value)
    _accepted(lambda: BP.load_predictor(_checkpoint(tmp_path, "s2.pt", elbo="SVGPVAE_Titsias")), "BallPredictor")


def test_load_on_a_checkpoint_without_meta_names_the_missing_keys(tmp_path):
    from svgp_vae_amd import ball_predict as BP
    path = _checkpoint(tmp_path, "old.pt", meta=False)
    for load in (BP.PearcePredictor.load, BP.load_predictor):
        with pytest.raises(ValueError) as e:
            load(path)
        said = str(e.value).split("meta entry for")[1]
        assert all(k in said for k in BP.PEARCE_META_KEYS) and not any(k in said for k in ("jitter", "clip_qs")), said
    with pytest.raises(ValueError) as e:
        BP.PearcePredictor.load(path, tmax=30, px=4)
    assert "hidden=..., py=..." in str(e.value) and "tmax" not in str(e.value).split("pass")[1]
    with pytest.raises(ValueError) as e:                                     # every key given, but another model's shape
        BP.PearcePredictor.load(path, tmax=30, hidden=7, px=4, py=4)
    assert "encW1" in str(e.value)
    _accepted(lambda: BP.PearcePredictor.load(path, tmax=30, hidden=6, px=4, py=4), "PearcePredictor")


def test_foreign_files_are_refused(tmp_path):
    from svgp_vae_amd import ball_predict as BP
    other = str(tmp_path / "other.pt")
    torch.save({"w": torch.zeros(3)}, other)
    for load in (BP.PearcePredictor.load, BP.load_predictor):
        with pytest.raises(ValueError) as e:
            load(other)
        assert "other.pt" in str(e.value) and "not a checkpoint" in str(e.value)


def test_predictor_is_re_exported_from_the_ball_module_and_checks_its_parameters():
    from svgp_vae_amd import ball
    from svgp_vae_amd import ball_predict as BP
    assert ball.PearcePredictor is BP.PearcePredictor and ball.BallPredictor is BP.BallPredictor
    with pytest.raises(ValueError) as e:
        BP.PearcePredictor({}, tmax=30, hidden=6, px=4, py=4)
    assert "l_x" in str(e.value) and "ip_x" not in str(e.value)


def test_the_driver_still_writes_the_meta_keys_both_predictors_read():
    from svgp_vae_amd import ball_predict as BP
    src = open(os.path.join(ROOT, "svgp-vae_amd", "BALL_experiment.py")).read()
    meta = re.search(r'"meta":\s*dict\((.*?)\)\}', src, flags=re.S).group(1)
    keys = set(re.findall(r"(\w+)=", meta))
    assert keys == set(BP.META_KEYS) | {"elbo", "vidlt"} and set(BP.PEARCE_META_KEYS) < keys


# ---------------------------------------------------------------------------------------------- command line
def test_cli_parses_as_before():
    from svgp_vae_amd import ball_predict as BP
    base = ["--checkpoint", "run/model.pt", "--out", "frames.npy"]
    a = BP.parse_args(base + ["--test_batch", "0", "--base_dir", "d", "--drop", "0.5", "--upsample", "2"])
    assert (a.checkpoint, a.test_batch, a.base_dir, a.drop, a.drop_seed, a.upsample, a.sample, a.videos, a.device) == \
        ("run/model.pt", 0, "d", 0.5, 0, 2, False, None, "cuda:0")
    assert sorted(vars(a)) == ["base_dir", "checkpoint", "device", "drop", "drop_seed", "observed", "out", "query_times", "sample", "seed",
                               "test_batch", "upsample", "videos"]
    for extra in ([], ["--test_batch", "0"], ["--videos", "v.npy", "--drop", "1.0"]):
        with pytest.raises(SystemExit) as e:
            BP.parse_args(base + extra)
        assert e.value.code == 2
    tq, at = BP.query_grid(8, upsample=2)
    assert tq.shape == (15,) and np.array_equal(tq[at], np.arange(1, 9))
