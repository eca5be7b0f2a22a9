"""Streamed moving-ball posterior state: everything that needs no GPU.  The C ABI's declarations, exports, struct mirrors, refusals,
workspace sizes and launch routes; the additivity and the order response of the restatement of the statistics (the margin behind
the GPU test's bar on stats; these pin the test oracle only, not the feature); the argument checks of BallPosteriorState on an
instance without a device; the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svgp_vae_amd
from svgp_vae_amd import _lib
from tests import ball_state_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svgp_ball_state_update", "svgp_ball_state_finalize", "svgp_ball_state_query", "svgp_ball_state_query_joint",
               "svgp_ball_state_workspace_elems", "svgp_ball_state_route")
FAKE = 4096                          # never dereferenced: every call below fails validation first
ALWAYS = ("ip_x", "ip_y", "ls_x", "ls_y")
REQUIRED = dict(update=ALWAYS + ("times", "mu_x", "mu_y", "var_x", "var_y", "stats"), finalize=ALWAYS + ("stats", "post"),
                query=ALWAYS + ("tq", "post", "p_m_x", "p_m_y", "p_v_x", "p_v_y"), query_joint=ALWAYS + ("tq", "post", "p_m_x", "p_m_y"))
FIELDS = ("times", "tq", "ip_x", "ip_y", "ls_x", "ls_y", "mu_x", "mu_y", "var_x", "var_y", "mask", "eps_x", "eps_y", "stats", "post",
          "p_m_x", "p_m_y", "p_v_x", "p_v_y", "cov_x", "cov_y", "chol_x", "chol_y", "z_x", "z_y")


def _cfg(B=3, T=30, m=15, Q=7, large=0, q_slices=0, jitter=1e-9, lo=1e-4, hi=1e3, jp=1e-9):
    return _lib.BallStateCfg(B=B, T=T, m=m, Q=Q, large=large, q_slices=q_slices, jitter=jitter, clip_lo=lo, clip_hi=hi, path_jitter=jp)


def _bufs(op, **null):
    q = _lib.BallStateBufs()
    for n in REQUIRED[op]:
        setattr(q, n, None if null.get(n) else FAKE)
    return q


def _run(op, cfg, bufs="default", work=FAKE, **null):
    bufs = _bufs(op, **null) if bufs == "default" else bufs
    return _lib.call("svgp_ball_state_" + op, None if cfg is None else C.byref(cfg), None if bufs is None else C.byref(bufs), work, None)


def _route(op, cfg, cap=1 << 16):
    buf = C.create_string_buffer(cap)
    _lib.call("svgp_ball_state_route", None if cfg is None else C.byref(cfg), SC.OPS[op] if isinstance(op, str) else op, buf, cap)
    return buf.value.decode().split()


# ---------------------------------------------------------------------------------------------- ABI
def test_header_declares_library_exports_and_binding_mirrors_the_structs():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svgpvae_hip.h")).read(), flags=re.S)
    lib = svgp_vae_amd.load_library()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} not declared in include/svgpvae_hip.h"
        assert hasattr(lib, n), f"{n} not exported"
        assert n in _lib.SIGNATURES or n in _lib.NON_STATUS
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_state_cfg\s*;", src, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == ("int32_t B, T, m, Q; int32_t large; int32_t q_slices; "
                                                 "double jitter, clip_lo, clip_hi, path_jitter;")
    assert [n for n, _ in _lib.BallStateCfg._fields_] == ["B", "T", "m", "Q", "large", "q_slices", "jitter", "clip_lo", "clip_hi",
                                                          "path_jitter"]
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*svgp_ball_state_bufs\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == [n for n, _ in _lib.BallStateBufs._fields_] == list(FIELDS)
    assert lib.svgp_struct_sizeof(25) == C.sizeof(_lib.BallStateCfg) == 56
    assert lib.svgp_struct_sizeof(26) == C.sizeof(_lib.BallStateBufs) == 8 * 25
    for unassigned in (12, 17, 21, 24, 27):
        assert lib.svgp_struct_sizeof(unassigned) == -1
    for op, code in SC.OPS.items():
        assert re.search(rf"#define\s+SVGP_BALL_STATE_{op.upper()}\s+{code}\b", src) and _lib.BALL_STATE_OPS[op] == code
    # the marginal entry's inputs, in its order, come first
    assert list(FIELDS[:13]) == [n for n, _ in _lib.BallPredictBufs._fields_][:13]


REFUSALS = []
for _op in SC.OPS:
    REFUSALS += [(lambda o=_op: _run(o, None), -1, "cfg is NULL"), (lambda o=_op: _run(o, _cfg(), None), -1, "bufs is NULL"),
                 (lambda o=_op: _run(o, _cfg(B=0)), -1, "B=0"), (lambda o=_op: _run(o, _cfg(m=0)), -1, "m=0"),
                 (lambda o=_op: _run(o, _cfg(m=2049, large=1)), -2, "m=2049"),
                 (lambda o=_op: _route(o, _cfg(m=2049, large=1)), -2, "m=2049"), (lambda o=_op: _route(o, None), -1, "cfg is NULL"),
                 (lambda o=_op: _route(o, _cfg(), cap=4), -1, "route text")]
    REFUSALS += [(lambda o=_op, n=n: _run(o, _cfg(), **{n: True}), -1, "NULL device pointer") for n in REQUIRED[_op]]
    REFUSALS += [(lambda o=_op, n=n: _run(o, _cfg(m=65, Q=40, large=1), **{n: True}), -1, "NULL device pointer") for n in REQUIRED[_op]]
    REFUSALS += [(lambda o=_op: _run(o, _cfg(m=65, large=1), work=None), -1, "work is NULL")]
    if _op != "query_joint":
        REFUSALS += [(lambda o=_op: _run(o, _cfg(m=65)), -2, "m=65"), (lambda o=_op: _route(o, _cfg(m=65)), -2, "m=65")]
REFUSALS += [
    (lambda: _run("update", _cfg(T=0)), -1, "T=0"), (lambda: _run("update", _cfg(T=16385)), -2, "T=16385"),
    (lambda: _run("update", _cfg(T=2049, large=1)), -2, "T=2049"), (lambda: _route("update", _cfg(T=2049, large=1)), -2, "T=2049"),
    (lambda: _run("query", _cfg(Q=0)), -1, "Q=0"), (lambda: _run("query_joint", _cfg(Q=0)), -1, "Q=0"),
    (lambda: _run("query", _cfg(lo=2.0, hi=1.0)), -1, "clip_lo <= clip_hi"),
    (lambda: _run("query", _cfg(lo=2.0, hi=1.0, large=1)), -1, "clip_lo <= clip_hi"),
    (lambda: _run("query", _cfg(q_slices=-1)), -1, "q_slices=-1"), (lambda: _run("query", _cfg(Q=33, q_slices=4)), -1, "q_slices=4"),
    (lambda: _run("query", _cfg(Q=16, q_slices=2)), -1, "q_slices=2"),
    (lambda: _run("query", _cfg(Q=16 * 70000, q_slices=65536)), -1, "q_slices=65536"),
    (lambda: _run("query_joint", _cfg(jp=-1e-9)), -1, "path_jitter >= 0"),
    (lambda: _run("query_joint", _cfg(jp=float("nan"))), -1, "path_jitter >= 0"),
    (lambda: _run("query_joint", _cfg(Q=2049)), -2, "Q=2049"), (lambda: _route("query_joint", _cfg(Q=2049)), -2, "Q=2049"),
    (lambda: _run("query_joint", _cfg(), work=None), -1, "work is NULL"),
    (lambda: _route(4, _cfg()), -1, "op=4"), (lambda: _route(-1, _cfg()), -1, "op=-1"),
    (lambda: _lib.call("svgp_ball_state_route", C.byref(_cfg()), 0, None, 10), -1, "bad argument"),
    (lambda: _route("finalize", _cfg(B=70, large=1), cap=40), -1, "route text"),
]


@pytest.mark.parametrize("call,code,message", REFUSALS)
def test_refusals_carry_their_code_and_a_message_and_launch_nothing(call, code, message):
    """Before any pointer is looked at: the pointers here are fake and there is no device."""
    with pytest.raises(_lib.SvgpError) as e:
        call()
    assert f"status {code}:" in str(e.value) and message in str(e.value), (message, str(e.value))


def test_each_entry_looks_only_at_the_sizes_it_needs():
    """finalize and the queries take a cfg whose T is 0, update and finalize one whose Q is 0: they get past the size checks and
    stop at the NULL pointer put there for that purpose."""
    for op, cfg in (("finalize", _cfg(T=0, Q=0)), ("query", _cfg(T=0)), ("query_joint", _cfg(T=0)), ("update", _cfg(Q=0)),
                    ("update", _cfg(Q=0, lo=2.0, hi=1.0, jp=-1.0, q_slices=-3)), ("finalize", _cfg(T=99999, Q=99999, large=1))):
        with pytest.raises(_lib.SvgpError, match="NULL device pointer"):
            _run(op, cfg, ip_x=True)
        assert _route(op, cfg)


def test_workspace_is_zero_for_the_fused_routes_and_a_refused_cfg_and_grows_with_neither_videos_nor_queries_beyond_a_chunk():
    lib = svgp_vae_amd.load_library()
    n = lambda op, **kw: lib.svgp_ball_state_workspace_elems(C.byref(_cfg(**kw)), SC.OPS[op])
    for op in ("update", "finalize", "query"):
        assert lib.svgp_ball_state_workspace_elems(None, SC.OPS[op]) == 0
        for B, T, m, Q in [(1, 1, 1, 1), (35, 30, 15, 61), (100000, 16384, 64, 100000)]:
            assert n(op, B=B, T=T, m=m, Q=Q) == 0
        for bad in (dict(m=65), dict(m=0, large=1), dict(m=2049, large=1), dict(B=0, large=1)):
            assert n(op, **bad) == 0, (op, bad)
        for m in (15, 65):
            assert 0 < n(op, B=3, m=m, large=1) < n(op, B=64, m=m, large=1) == n(op, B=65, m=m, large=1) == n(op, B=100000, m=m, large=1)
    assert lib.svgp_ball_state_workspace_elems(C.byref(_cfg()), 4) == 0
    assert n("update", T=2049, large=1) == 0 and n("update", T=0, large=1) == 0 and n("query", Q=0, large=1) == 0
    assert n("query", lo=2.0, hi=1.0, large=1) == 0 and n("query_joint", jp=-1.0) == 0 and n("query_joint", Q=2049) == 0
    assert n("update", T=30, large=1) < n("update", T=60, large=1)
    assert n("finalize", T=30, large=1) == n("finalize", T=2048, Q=5000, large=1)                       # neither T nor Q enters
    assert n("query", Q=100, large=1) < n("query", Q=4096, large=1) == n("query", Q=4097, large=1) == n("query", Q=10 ** 6, large=1)
    # the joint query: large whatever cfg.large says; its chunk is capped by the covariance block
    for large in (0, 1):
        assert 0 < n("query_joint", B=3, Q=9, large=large) < n("query_joint", B=64, Q=9, large=large) == n("query_joint", B=70, Q=9, large=large)
    assert n("query_joint", B=1, m=4, Q=2048) == n("query_joint", B=9, m=4, Q=2048) == n("query_joint", B=100000, m=4, Q=2048)
    assert n("query_joint", B=3, m=4, Q=1024) < n("query_joint", B=4, m=4, Q=1024) == n("query_joint", B=64, m=4, Q=1024)
    for B, Q in ((9, 2048), (64, 1024), (64, 700), (7, 300)):
        nb = SC.joint_chunk(B, Q)
        assert nb * Q * Q <= n("query_joint", B=B, m=4, Q=Q) <= nb * Q * Q + lib.svgp_potrf_workspace_elems(Q, nb) + 200 * nb * Q + 4096


# ---------------------------------------------------------------------------------------------- route
@pytest.mark.parametrize("case", SC.CASE_IDS + ["9-8-4-2048", "130-2048-300-5000"])
def test_route_of_every_operation_on_both_routes(case):
    from svgp_vae_amd import ball_predict as BP
    B, T, m, Q = SC.shape_of(case)
    for op in SC.OPS:
        if op == "query_joint" and Q > 2048:
            continue
        if m <= SC.FUSED_M_MAX and op != "query_joint":
            assert _route(op, _cfg(B, T, m, Q)) == ["k_ball_state_" + op]
        names = _route(op, _cfg(B, T, m, Q, large=1))
        assert names == SC.expected_route(op, B, T, m, Q, True), op
        assert BP.state_route(op, (B, T, m, Q)) == SC.expected_route(op, B, T, m, Q, m > SC.FUSED_M_MAX)
        chunks = -(-B // (SC.joint_chunk(B, Q) if op == "query_joint" else SC.NB))
        count = dict(update=("k_bp_scale_rows", 1), finalize=("svgp_spd_inverse_batched", 1), query=("k_bp_finish", -(-Q // SC.QC)),
                     query_joint=("svgp_potrf_batched", 1))[op]
        assert names.count(count[0]) == 2 * chunks * count[1]
    assert _route("query_joint", _cfg(B, T, m, min(Q, 2048), large=0)) == _route("query_joint", _cfg(B, T, m, min(Q, 2048), large=1))


def test_fused_routes_are_one_launch_whatever_the_batch_the_frames_the_queries_and_the_slices():
    for B, T, Q in [(1, 1, 1), (35, 30, 61), (256, 64, 4096), (100000, 16384, 10 ** 6)]:
        for m in (1, 32, 33, 64):
            for op in ("update", "finalize", "query"):
                assert _route(op, _cfg(B, T, m, Q)) == ["k_ball_state_" + op]
    assert _route("query", _cfg(2, 30, 64, 4096, q_slices=256)) == _route("query", _cfg(2, 30, 64, 4096, q_slices=1)) == ["k_ball_state_query"]


def test_slice_choice_as_specified():
    assert [SC.slices_of(B, Q) for B, Q in [(1, 1), (35, 61), (2, 4096), (2, 100), (1, 10 ** 6), (1000, 4096)]] == [1, 4, 128, 7, 256, 1]
    assert SC.slices_max(16) == 1 and SC.slices_max(17) == 2 and SC.slices_max(16 * 65535 + 1) == 65535
    assert _route("query", _cfg(Q=17, q_slices=2)) == ["k_ball_state_query"]            # the largest forced count is accepted
    # Q close to 2^31: the rounds are counted in 64 bits, so the largest slice count is accepted and one more is refused
    big = 2 ** 31 - 1
    assert SC.slices_max(big) == 65535 and _route("query", _cfg(Q=big, q_slices=65535)) == ["k_ball_state_query"]
    assert _route("query", _cfg(B=1, Q=big)) == ["k_ball_state_query"]
    with pytest.raises(_lib.SvgpError, match="q_slices=65536"):
        _route("query", _cfg(Q=big, q_slices=65536))


# ---------------------------------------------------------------------------------------------- the restatement of the statistics
# (The four tests of this block use only the numpy helpers of tests/ball_state_cases.py: they pin the TEST ORACLE -- its additivity,
# its response to the frame order, which is the margin behind the GPU test's 1e-12 bar, its agreement with kernel_reference, and the
# case table -- not the feature, and so pass with or without the library's new entries.)
@pytest.mark.parametrize("case", SC.CASE_IDS)
def test_restatement_stats_of_the_pieces_add_up_and_frame_order_moves_them_by_1e_14_at_most(case):
    prob, whole = SC.kernel_problem(case), SC.case_stats(case)
    T = prob["times"].size
    assert np.isfinite(whole).all() and whole.shape == (prob["y"].shape[2], 2, prob["ip"].shape[1] * (prob["ip"].shape[1] + 1))
    scale = np.abs(whole).max() + 1e-300
    for cut in SC.cuts_of(case) + [T // 2]:
        pieces = SC.problem_stats(prob, slice(0, cut)) + SC.problem_stats(prob, slice(cut, T))
        e = float(np.abs(pieces - whole).max() / scale)
        print(f"{case} cut {cut}: pieces against whole {e:.2e}")
        assert e <= SC.ORDER_TOL, (cut, e)
    back = SC.problem_stats(prob, np.arange(T)[::-1])
    e = float(np.abs(back - whole).max() / scale)
    print(f"{case}: reversed frame order {e:.2e}")
    assert e <= SC.ORDER_TOL, e
    assert SC.STATS_TOL >= 100 * SC.ORDER_TOL


@pytest.mark.parametrize("case", ["3-5-1-3", "3-30-17-33", "2-64-64-40", "2-100-65-40"])
def test_restatement_stats_give_the_reference_posterior(case):
    """post_of(stats) is the X and w of ball_predict_cases.posterior: p_m = k w and p_v = 1 + k X k^T meet kernel_reference."""
    prob, (p_m, p_v, _) = SC.kernel_problem(case), SC.kernel_reference(case)
    post, m = SC.post_of(prob, SC.case_stats(case)), prob["ip"].shape[1]
    for c in range(2):
        k = SC.se(prob["tq"], prob["ip"][c], prob["ls"][c])
        for b in range(post.shape[0]):
            X, w = post[b, c, :m * m].reshape(m, m), post[b, c, m * m:]
            assert SC.relerr(k @ w, p_m[c, :, b]) <= SC.TOL / 10 or np.abs(p_m[c, :, b]).max() == 0
            assert SC.relerr(1.0 + np.einsum("qi,ij,qj->q", k, X, k), p_v[c, :, b]) <= SC.TOL / 10
    if post.shape[0] > 1:            # video 1 has every frame dropped
        assert (SC.case_stats(case)[1] == 0).all() and np.abs(post[1]).max() == 0


def test_case_table_is_as_specified():
    assert SC.CASE_IDS == ["1-1-1-1", "3-5-1-3", "2-2-3-4", "3-30-16-16", "3-30-17-33", "2-64-32-17", "2-64-33-70", "2-64-64-40",
                           "35-30-15-61", "2-100-65-40", "70-30-15-9"]
    assert [SC.cuts_of(c) for c in SC.CASE_IDS] == [[], [2], [1], [1, 15, 16, 17], [16], [], [31, 32, 33], [16, 48], [10, 20], [50], []]
    assert SC.LARGE_ONLY == [(2, 100, 65, 40), (70, 30, 15, 9)]
    assert (SC.STATS_TOL, SC.ORDER_TOL, SC.PATH_TOL, SC.TOL, SC.PATH_JITTER_DIRECT) == (1e-12, 1e-14, 1e-10, 1e-8, 1e-4)
    for case in SC.CASE_IDS:
        T = SC.shape_of(case)[1]
        assert all(0 < c < T for c in SC.cuts_of(case))


# ---------------------------------------------------------------------------------------------- the Python object and the command line
def _bare(cls, **attrs):
    """An instance without a device: the argument checks come before it is touched."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _bare_state(B=2, m=5, n_seen=0):
    from svgp_vae_amd import ball_predict as BP
    pred = _bare(BP.BallPredictor, jitter=1e-9, px=4, py=4, m=m)
    return _bare(BP.BallPosteriorState, pred=pred, B=B, large=m > 64, n_seen=n_seen, _dirty=True)


def test_state_checks_its_arguments_before_any_device_work():
    from svgp_vae_amd import ball, ball_predict as BP
    assert ball.BallPosteriorState is BP.BallPosteriorState
    st, vid, tq = _bare_state(), np.zeros((2, 5, 4, 4)), np.arange(3.0)
    for bad in (np.zeros((2, 5, 4)), np.zeros((2, 5, 4, 5))):
        with pytest.raises(ValueError, match=r"videos must be \(B, T, 4, 4\)"):
            st.observe(bad)
    with pytest.raises(ValueError, match="the state's B = 2"):
        st.observe(np.zeros((3, 5, 4, 4)))
    with pytest.raises(ValueError, match="at least one video, frame"):
        st.observe(np.zeros((2, 0, 4, 4)))
    with pytest.raises(ValueError, match=r"observed must be \(B, T\) = \(2, 5\)"):
        st.observe(vid, observed=np.ones((2, 4), bool))
    with pytest.raises(ValueError, match="frame_times must have T = 5 entries"):
        st.observe(vid, frame_times=np.arange(4.0))
    with pytest.raises(ValueError, match="frame_times must be finite"):
        st.observe(vid, frame_times=np.array([1.0, 2.0, np.nan, 4.0, 5.0]))
    with pytest.raises(ValueError, match="paths=True needs eps"):
        st.predict(tq, paths=True)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="path_jitter"):
            st.predict(tq, return_cov=True, path_jitter=bad)
    with pytest.raises(ValueError, match="path_jitter applies"):
        st.predict(tq, path_jitter=1e-4)
    with pytest.raises(ValueError, match="at least one video, frame and query time"):
        st.predict(np.zeros(0))
    with pytest.raises(ValueError, match="query_times must be finite"):
        st.predict(np.array([1.0, np.inf]))
    with pytest.raises(ValueError, match=r"eps must be \(B, Q, 2\) = \(2, 3, 2\)"):
        st.predict(tq, eps=np.zeros((2, 4, 2)))
    assert st.n_seen == 0
    with pytest.raises(TypeError, match="BallPredictor"):
        BP.BallPosteriorState(_bare(BP.PearcePredictor, px=4, py=4), 2)
    with pytest.raises(ValueError, match="at least one video"):
        BP.BallPosteriorState(_bare(BP.BallPredictor, m=5), 0)


def test_state_route_needs_no_device_and_follows_the_dirty_flag():
    st = _bare_state(B=3, m=15)
    assert st.route("update", T=30) == ["k_ball_state_update"] and st.route("finalize") == ["k_ball_state_finalize"]
    assert st.route("query", Q=40) == ["k_ball_state_query"]
    assert st.route("query_joint", Q=40) == SC.expected_route("query_joint", 3, 1, 15, 40, True)
    assert st.route("predict", Q=40) == ["k_ball_state_finalize", "k_ball_state_query"]
    st._dirty = False
    assert st.route("predict", Q=40) == ["k_ball_state_query"]
    assert st.route("predict", Q=40, joint=True) == ["k_ball_state_query"] + SC.expected_route("query_joint", 3, 1, 15, 40, True)
    big = _bare_state(B=2, m=65)
    for op in ("update", "finalize", "query"):
        assert big.route(op, T=30, Q=20) == SC.expected_route(op, 2, 30, 65, 20, True)
    with pytest.raises(ValueError, match="op must be one of"):
        st.route("observe")


BASE = ["--checkpoint", "run/model.pt", "--out", "frames.npy", "--videos", "v.npy"]


def test_cli_parser_of_stream_chunk():
    from svgp_vae_amd import ball_predict as BP
    a = BP.parse_args(BASE)
    assert not hasattr(a, "stream_chunk")                 # without the flag the namespace is what it was
    a = BP.parse_args(BASE + ["--stream_chunk", "7", "--sample", "--upsample", "2"])
    assert a.stream_chunk == 7 and a.sample and a.upsample == 2
    a = BP.parse_args(BASE + ["--stream_chunk", "1", "--sample_paths", "--save_cov", "c.npy"])
    assert a.stream_chunk == 1 and BP.joint_args(a) == (True, None, "c.npy")
    for bad in (["--stream_chunk", "0"], ["--stream_chunk", "-3"], ["--stream_chunk"], ["--stream_chunk", "x"]):
        with pytest.raises(SystemExit) as e:
            BP.parse_args(BASE + bad)
        assert e.value.code == 2


def test_cli_refuses_an_exact_gp_checkpoint_with_stream_chunk(monkeypatch):
    """Told by the checkpoint's family, before any video is read or any device touched."""
    from svgp_vae_amd import ball_predict as BP
    monkeypatch.setattr(BP, "load_predictor", lambda path, **kw: _bare(BP.PearcePredictor))
    with pytest.raises(SystemExit) as e:
        BP.main(BASE + ["--stream_chunk", "7"])
    assert "--stream_chunk" in str(e.value) and "SVGPVAE_Hensman" in str(e.value) and "SVGPVAE_Titsias" in str(e.value)
