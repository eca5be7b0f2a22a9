"""Streamed moving-ball posterior state on the GPU: svgp_ball_state_update / finalize / query / query_joint over the case table of
tests/ball_state_cases.py against the float64 restatement and against the existing one-shot entries, the bit-level properties of the
fused routes, the large routes, guarding, BallPosteriorState against BallPredictor.predict, and the command line end to end."""
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
from tests import ball_state_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CANARY, PAD = 12345.678, 64
JOINT_OUTPUTS = ("p_m", "cov", "chol", "z")


class _Buf:
    """A device array of the given shape with PAD canary values on both sides; `fill` None leaves canaries inside too."""

    def __init__(self, *shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(*shape)
        if fill is not None:
            self.view.copy_(torch.as_tensor(np.broadcast_to(np.asarray(fill, dtype=np.float64), shape).copy()))

    def intact(self):
        return bool((self.buf[:PAD] == CANARY).all() and (self.buf[-PAD:] == CANARY).all())

    def numpy(self):
        return self.view.cpu().numpy()


same_bits = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))       # (a NaN equals itself)
dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV)


def _call(op, prob, large, bufs, keep, *, T=0, Q=0, jp=0.0, q_slices=0):
    """One svgp_ball_state_<op> call; the workspace has canaries of its own.  `keep` holds the device tensors alive."""
    from svgp_vae_amd import _lib
    lib = _lib.load_library()
    B, m = prob["y"].shape[2], prob["ip"].shape[1]
    cfg = _lib.BallStateCfg(B=B, T=T, m=m, Q=Q, large=int(large), q_slices=q_slices, jitter=prob["jitter"], clip_lo=PC.CLIP[0],
                            clip_hi=PC.CLIP[1], path_jitter=jp)
    ip, ls = dv(prob["ip"]), dv(prob["ls"])
    keep += [ip, ls]
    for c, cn in enumerate("xy"):
        setattr(bufs, f"ip_{cn}", ip[c].data_ptr()); setattr(bufs, f"ls_{cn}", ls[c:].data_ptr())
    n = int(lib.svgp_ball_state_workspace_elems(C.byref(cfg), SC.OPS[op]))
    assert (n > 0) == (bool(large) or op == "query_joint"), (op, n)
    work = _Buf(n) if n else None
    _lib.call("svgp_ball_state_" + op, C.byref(cfg), C.byref(bufs), work.view.data_ptr() if n else None,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert work is None or work.intact(), op


def new_stats(prob, fill=0.0):
    B, m = prob["y"].shape[2], prob["ip"].shape[1]
    return _Buf(B, 2, m * m + m, fill=fill)


def update(prob, stats, large, frames=None, *, mask=True, y=None):
    """stats += the frames `frames` (slice or index array; default all) of the problem.  Returns stats."""
    from svgp_vae_amd import _lib
    sel = slice(None) if frames is None else frames
    y = prob["y"] if y is None else y
    keep = [dv(prob["times"][sel]), dv(y[:, sel]), dv(prob["s2"][:, sel])]
    mk = None if mask is None or mask is False else dv((prob["mask"] if mask is True else mask)[sel])
    q = _lib.BallStateBufs()
    q.times, q.mask, q.stats = keep[0].data_ptr(), None if mk is None else mk.data_ptr(), stats.view.data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"mu_{cn}", keep[1][c].data_ptr()); setattr(q, f"var_{cn}", keep[2][c].data_ptr())
    _call("update", prob, large, q, keep + [mk], T=int(keep[0].numel()))
    assert stats.intact()
    return stats


def finalize(prob, stats, large, post=None):
    from svgp_vae_amd import _lib
    post = new_stats(prob, fill=None) if post is None else post
    before = stats.view.clone()
    q = _lib.BallStateBufs()
    q.stats, q.post = stats.view.data_ptr(), post.view.data_ptr()
    _call("finalize", prob, large, q, [])
    assert stats.intact() and post.intact() and same_bits(stats.view, before)
    return post


def query(prob, post, large, *, eps=True, want_z=True, tq=None, q_slices=0):
    """dict(p_m, p_v, z (2, Q, B) numpy; z None when not asked for)."""
    from svgp_vae_amd import _lib
    B, tq = prob["y"].shape[2], prob["tq"] if tq is None else tq
    Q = tq.size
    keep = [dv(tq), dv(prob["eps"]) if eps is True else (None if eps is None or eps is False else dv(eps))]
    outs = {k: [_Buf(Q, B) for _ in range(2)] for k in ("p_m", "p_v", "z")}
    before = post.view.clone()
    q = _lib.BallStateBufs()
    q.tq, q.post = keep[0].data_ptr(), post.view.data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"eps_{cn}", None if keep[1] is None else keep[1][c].data_ptr())
        setattr(q, f"p_m_{cn}", outs["p_m"][c].view.data_ptr()); setattr(q, f"p_v_{cn}", outs["p_v"][c].view.data_ptr())
        setattr(q, f"z_{cn}", outs["z"][c].view.data_ptr() if want_z else None)
    _call("query", prob, large, q, keep, Q=Q, q_slices=q_slices)
    assert post.intact() and same_bits(post.view, before)
    for k, pair in outs.items():
        for o in pair:
            assert o.intact(), k
            if k == "z" and not want_z:
                assert bool((o.view == CANARY).all())
    get = lambda k: np.stack([o.numpy() for o in outs[k]])
    return dict(p_m=get("p_m"), p_v=get("p_v"), z=get("z") if want_z else None)


def query_joint(prob, post, jp, *, eps=True, want=("cov", "chol", "z"), tq=None, large=0):
    """dict(p_m, z (2, Q, B); cov, chol (2, B, Q, Q)) numpy, None for an output that was not asked for."""
    from svgp_vae_amd import _lib
    B, tq = prob["y"].shape[2], prob["tq"] if tq is None else tq
    Q = tq.size
    keep = [dv(tq), dv(prob["eps"]) if eps is True else (None if eps is None or eps is False else dv(eps))]
    shape = dict(p_m=(Q, B), z=(Q, B), cov=(B, Q, Q), chol=(B, Q, Q))
    outs = {k: [_Buf(*shape[k]) for _ in range(2)] for k in JOINT_OUTPUTS}
    before = post.view.clone()
    q = _lib.BallStateBufs()
    q.tq, q.post = keep[0].data_ptr(), post.view.data_ptr()
    for c, cn in enumerate("xy"):
        setattr(q, f"eps_{cn}", None if keep[1] is None else keep[1][c].data_ptr())
        for k in JOINT_OUTPUTS:
            setattr(q, f"{k}_{cn}", outs[k][c].view.data_ptr() if k == "p_m" or k in want else None)
    _call("query_joint", prob, large, q, keep, Q=Q, jp=jp)
    assert post.intact() and same_bits(post.view, before)
    for k, pair in outs.items():
        for o in pair:
            assert o.intact(), k
            if k != "p_m" and k not in want:
                assert bool((o.view == CANARY).all()), k
    return {k: np.stack([o.numpy() for o in outs[k]]) if k == "p_m" or k in want else None for k in JOINT_OUTPUTS}


@functools.lru_cache(maxsize=None)
def device_state(case, large):
    """(stats, post) buffers of a case fed in one call (T > the route's limit never occurs in the table).  Shared: read only."""
    prob = SC.kernel_problem(case)
    stats = update(prob, new_stats(prob), large)
    return stats, finalize(prob, stats, large)


@functools.lru_cache(maxsize=None)
def device_query(case, large):
    return query(SC.kernel_problem(case), device_state(case, large)[1], large)


@functools.lru_cache(maxsize=None)
def existing_marginal(case, large):
    from tests.test_gpu_ball_predict import run
    return run(SC.kernel_problem(case), large)


@functools.lru_cache(maxsize=None)
def existing_joint(case, jp):
    from tests.test_gpu_joint_predict import run
    return run(SC.kernel_problem(case), True, jp)


# ---------------------------------------------------------------------------------------------- against the restatement and the entries
@pytest.mark.parametrize("case,large", SC.ROUTES, ids=SC.ROUTE_IDS)
def test_stats_against_the_restatement(case, large):
    stats, ref = device_state(case, large)[0].numpy(), SC.case_stats(case)
    e = SC.relerr(stats, ref)
    print(f"{case} {'large' if large else 'fused'} stats: {e:.2e}")
    assert e <= SC.STATS_TOL, e
    if stats.shape[0] > 1:           # video 1 has every frame dropped
        assert (stats[1] == 0).all()


@pytest.mark.parametrize("case,large", SC.ROUTES, ids=SC.ROUTE_IDS)
def test_post_and_marginal_query_against_the_restatement_and_the_one_shot_entry(case, large):
    """Against svgp_ball_predict the fused route is held to the bits: update, finalize and query run the device pieces k_ball_predict
    is made of (bp_accumulate, bp_invert, bp_store_x, bp_query_chunks) on the same operands.  The large route keeps PATH_TOL."""
    prob, ref = SC.kernel_problem(case), dict(zip(("p_m", "p_v", "z"), SC.kernel_reference(case)))
    got, one = device_query(case, large), existing_marginal(case, large)
    bad = []
    for k in ("p_m", "p_v", "z"):
        e_r, e_o = SC.relerr(got[k], ref[k]), SC.relerr(got[k], one[k])
        print(f"{case} {'large' if large else 'fused'} {k}: restatement {e_r:.2e}, one-shot entry {e_o:.2e}")
        if not e_r <= SC.TOL:
            bad.append((k, "restatement", e_r))
        if not (e_o <= SC.PATH_TOL if large else np.array_equal(got[k], one[k])):
            bad.append((k, "one-shot", e_o))
    m = prob["ip"].shape[1]
    post = device_state(case, large)[1].numpy()
    if post.shape[0] > 1 and not large:                   # the fused route promises the prior exactly
        assert (post[1] == 0).all() and (got["p_m"][:, :, 1] == 0).all() and (got["p_v"][:, :, 1] == 1).all()
    assert np.isfinite(post).all() and post.shape[2] == m * m + m
    assert not bad, bad


@pytest.mark.parametrize("case,large", SC.ROUTES, ids=SC.ROUTE_IDS)
def test_joint_query_against_the_restatement_and_the_one_shot_entry(case, large):
    """The bars of tests/test_gpu_joint_predict.py: p_m and cov at TOL at the model's jitter, chol and z at TOL at PATH_JITTER_DIRECT,
    the identities of the device's own factor at the model's jitter.  Against svgp_ball_predict_joint_large at PATH_TOL: p_m and cov
    at both jitters, chol and z at PATH_JITTER_DIRECT (at 1e-9 the factor answers one ulp of its input with up to 2e-8,
    tests/ball_joint_cases.py, so no two evaluation paths of X can be held to 1e-10 there)."""
    prob, post = SC.kernel_problem(case), device_state(case, large)[1]
    Q = prob["tq"].size
    bad = []
    for jp in (JC.JITTER, JC.PATH_JITTER_DIRECT):
        g, ref, one = query_joint(prob, post, jp), JC.reference_of(prob, jp), existing_joint(case, jp)
        assert np.array_equal(g["cov"], g["cov"].transpose(0, 1, 3, 2))
        for k in JOINT_OUTPUTS if jp == JC.PATH_JITTER_DIRECT else ("p_m", "cov"):
            e_r, e_o = JC.relerr(g[k], ref[k]), JC.relerr(g[k], one[k])
            print(f"{case} {'large' if large else 'fused'} state, jp {jp:g} {k}: restatement {e_r:.2e}, one-shot entry {e_o:.2e}")
            if not e_r <= JC.TOL:
                bad.append((jp, k, "restatement", e_r))
            if not e_o <= SC.PATH_TOL:
                bad.append((jp, k, "one-shot", e_o))
        if jp == JC.JITTER:
            L = g["chol"]
            assert np.isfinite(L).all() and np.isfinite(g["z"]).all()
            assert (np.triu(L, 1) == 0).all() and (np.diagonal(L, axis1=2, axis2=3) > 0).all()
            A = g["cov"] + jp * np.eye(Q)
            worst = max(float(np.abs(L[c, b] @ L[c, b].T - A[c, b]).max() / JC.chol_residual_bound(A[c, b]))
                        for c in range(2) for b in range(L.shape[1]))
            e = JC.relerr(g["z"], g["p_m"] + np.einsum("cbqr,crb->cqb", L, prob["eps"]))
            print(f"{case}: residual / bound {worst:.3f}, z against p_m + chol eps {e:.2e}")
            if not worst <= 1.0:
                bad.append(("residual / bound", worst))
            if not e <= JC.TOL:
                bad.append(("z identity", e))
            e = JC.relerr(np.diagonal(g["cov"], axis1=2, axis2=3).transpose(0, 2, 1), device_query(case, large)["p_v"])
            if not e <= JC.TOL:
                bad.append(("diag(cov) against the marginal query's p_v", e))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- bit for bit on the fused routes
@pytest.mark.parametrize("case", [c for c in SC.FUSED_IDS if SC.cuts_of(c)])
def test_fused_update_in_pieces_gives_the_bits_of_one_call(case):
    prob, whole = SC.kernel_problem(case), device_state(case, False)[0].numpy()
    T = prob["times"].size
    for cut in SC.cuts_of(case):
        st = update(prob, new_stats(prob), False, slice(0, cut))
        assert np.array_equal(update(prob, st, False, slice(cut, T)).numpy(), whole), cut
    st = new_stats(prob)             # every listed cut at once
    for t0, t1 in zip([0] + SC.cuts_of(case), SC.cuts_of(case) + [T]):
        update(prob, st, False, slice(t0, t1))
    assert np.array_equal(st.numpy(), whole)


@pytest.mark.parametrize("case", ["3-30-17-33", "2-64-64-40", "35-30-15-61"])
def test_fused_update_ignores_a_dropped_frame_and_an_all_dropped_call_bit_for_bit(case):
    prob, whole = SC.kernel_problem(case), device_state(case, False)[0].numpy()
    T, B = prob["mask"].shape
    t = 1 + int(np.argmax(prob["mask"][1:, 0] == 0))       # a dropped frame of video 0 that is not the first
    assert prob["mask"][t, 0] == 0
    y = prob["y"].copy()
    y[:, t, 0] = np.nan
    assert np.array_equal(update(prob, new_stats(prob), False, y=y).numpy(), whole)
    # the call without the frames that every video dropped... there is none in general: drop frame t for all, then compare without it
    mask = prob["mask"].copy()
    mask[t, :] = 0
    y[:, t, :] = np.nan
    without = np.delete(np.arange(T), t)
    a = update(prob, new_stats(prob), False, y=y, mask=mask).numpy()
    b = update(prob, new_stats(prob), False, without).numpy()
    assert np.array_equal(a, b)
    st = new_stats(prob, fill=whole)
    assert np.array_equal(update(prob, st, False, mask=np.zeros((T, B)), y=y).numpy(), whole)


@pytest.mark.parametrize("case", ["1-1-1-1", "3-30-16-16", "2-64-33-70", "2-64-64-40"])
def test_zero_stats_finalise_to_zero_and_query_to_the_prior_exactly(case):
    prob = SC.kernel_problem(case)
    post = finalize(prob, new_stats(prob), False)
    assert (post.numpy() == 0).all()
    g = query(prob, post, False)
    assert (g["p_m"] == 0).all() and (g["p_v"] == 1).all()
    assert np.array_equal(g["z"], prob["eps"] * np.sqrt(1.0))


@pytest.mark.parametrize("case", ["3-30-16-16", "3-30-17-33", "2-64-33-70", "2-64-64-40", "35-30-15-61"])
def test_fused_query_bits_depend_neither_on_the_slices_nor_on_the_position_in_tq(case):
    prob, post, a = SC.kernel_problem(case), device_state(case, False)[1], device_query(case, False)
    B, _, _, Q = SC.shape_of(case)
    for S in (1, SC.slices_max(Q), max(1, SC.slices_max(Q) // 2)):
        g = query(prob, post, False, q_slices=S)
        for k in ("p_m", "p_v", "z"):
            assert np.array_equal(g[k], a[k]), (S, k)
    perm = np.random.RandomState(5).permutation(Q)
    g = query(prob, post, False, tq=prob["tq"][perm], eps=prob["eps"][:, perm])
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(g[k], a[k][:, perm]), k
    # one more query time than a whole number of rounds and slices: the last slice's last round is partial
    tq = np.concatenate([prob["tq"], prob["tq"][:1]])
    g = query(prob, post, False, tq=tq, eps=None, q_slices=SC.slices_max(Q + 1))
    assert np.array_equal(g["p_m"][:, :Q], a["p_m"]) and np.array_equal(g["p_m"][:, Q], a["p_m"][:, 0])


@pytest.mark.parametrize("case,large", [("3-30-17-33", False), ("2-64-64-40", False), ("3-30-17-33", True), ("2-100-65-40", True)],
                         ids=["17-fused", "64-fused", "17-large", "65-large"])
def test_every_entry_repeats_bitwise(case, large):
    prob = SC.kernel_problem(case)
    stats, post = device_state(case, large)
    again = update(prob, new_stats(prob), large)
    assert np.array_equal(again.numpy(), stats.numpy())
    assert np.array_equal(finalize(prob, again, large).numpy(), post.numpy())
    a, b = device_query(case, large), query(prob, post, large)
    for k in ("p_m", "p_v", "z"):
        assert np.array_equal(a[k], b[k]), k
    a, b = query_joint(prob, post, JC.PATH_JITTER_DIRECT), query_joint(prob, post, JC.PATH_JITTER_DIRECT)
    for k in JOINT_OUTPUTS:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- the large route; frame order
@pytest.mark.parametrize("case", ["3-30-17-33", "2-100-65-40", "70-30-15-9"])
def test_large_update_in_pieces_against_the_whole(case):
    prob, whole = SC.kernel_problem(case), device_state(case, True)[0].numpy()
    T = prob["times"].size
    for cut in SC.cuts_of(case) or [T // 2]:
        st = update(prob, update(prob, new_stats(prob), True, slice(0, cut)), True, slice(cut, T)).numpy()
        e = SC.relerr(st, whole)
        print(f"{case} cut {cut}: pieces against whole {e:.2e}")
        assert e <= SC.STATS_TOL, (cut, e)


@pytest.mark.parametrize("case,large", [("3-30-17-33", False), ("2-64-64-40", False), ("3-30-17-33", True), ("2-100-65-40", True)],
                         ids=["17-fused", "64-fused", "17-large", "65-large"])
def test_frames_in_reversed_order_agree_with_the_restatement(case, large):
    prob, ref = SC.kernel_problem(case), dict(zip(("p_m", "p_v", "z"), SC.kernel_reference(case)))
    T = prob["times"].size
    stats = update(prob, new_stats(prob), large, np.arange(T)[::-1])
    e = SC.relerr(stats.numpy(), SC.case_stats(case))
    print(f"{case} reversed stats: {e:.2e}")
    assert e <= SC.STATS_TOL
    g = query(prob, finalize(prob, stats, large), large)
    for k in ("p_m", "p_v", "z"):
        e = SC.relerr(g[k], ref[k])
        print(f"{case} reversed {k}: {e:.2e}")
        assert e <= SC.TOL, (k, e)


# ---------------------------------------------------------------------------------------------- guarding
@pytest.mark.parametrize("case,large", [("3-30-17-33", False), ("2-64-64-40", False), ("2-100-65-40", True), ("70-30-15-9", True)],
                         ids=["17-fused", "64-fused", "65-large", "70-videos-large"])
def test_optional_pointers_may_be_null_in_turn(case, large):
    """(Canaries around stats, post, the workspace and every output are checked by every helper of this file.)"""
    prob, (_, post) = SC.kernel_problem(case), device_state(case, large)
    nomask = update(prob, new_stats(prob), large, mask=None).numpy()
    ones = update(prob, new_stats(prob), large, mask=np.ones_like(prob["mask"])).numpy()
    assert np.array_equal(nomask, ones) and not np.array_equal(nomask, device_state(case, large)[0].numpy())
    a = device_query(case, large)
    mean, noz = query(prob, post, large, eps=None), query(prob, post, large, want_z=False)
    assert np.array_equal(mean["z"], a["p_m"]) and noz["z"] is None
    for k in ("p_m", "p_v"):
        assert np.array_equal(mean[k], a[k]) and np.array_equal(noz[k], a[k]), k
    jp = JC.PATH_JITTER_DIRECT
    j = query_joint(prob, post, jp)
    jmean = query_joint(prob, post, jp, eps=None)
    assert np.array_equal(jmean["z"], j["p_m"])
    for drop in ("cov", "chol", "z"):
        g = query_joint(prob, post, jp, want=tuple(k for k in ("cov", "chol", "z") if k != drop))
        assert g[drop] is None
        for k in JOINT_OUTPUTS:
            assert k == drop or np.array_equal(g[k], j[k]), (drop, k)
    assert np.array_equal(query_joint(prob, post, jp, want=())["p_m"], j["p_m"])


@pytest.mark.parametrize("case,large", [("3-30-17-33", False), ("2-64-64-40", False), ("2-100-65-40", True), ("70-30-15-9", True)],
                         ids=["17-fused", "64-fused", "65-large", "70-videos-large"])
def test_nan_in_one_videos_kept_frame_stays_in_that_video(case, large):
    prob = SC.kernel_problem(case)
    assert prob["mask"][0, 0] == 1 and prob["s2"][1, 0, 0] > 0          # a kept frame that carries information
    y = prob["y"].copy()
    y[1, 0, 0] = np.nan
    ok_stats, ok_post = device_state(case, large)
    stats = update(prob, new_stats(prob), large, y=y)
    s, o = stats.numpy(), ok_stats.numpy()
    m = prob["ip"].shape[1]
    assert np.isnan(s[0, 1, m * m:]).any() and np.array_equal(s[0, 1, :m * m], o[0, 1, :m * m])     # r of (video 0, y) only
    assert np.array_equal(s[0, 0], o[0, 0]) and np.array_equal(s[1:], o[1:])
    post = finalize(prob, stats, large)
    p, po = post.numpy(), ok_post.numpy()
    assert np.array_equal(p[0, 0], po[0, 0]) and np.array_equal(p[1:], po[1:])
    g, a = query(prob, post, large), device_query(case, large)
    for k in ("p_m", "z"):
        assert np.isnan(g[k][1, :, 0]).all(), k
        assert np.array_equal(g[k][0], a[k][0]) and np.array_equal(g[k][1, :, 1:], a[k][1, :, 1:]), k
    assert np.array_equal(g["p_v"], a["p_v"])


# ---------------------------------------------------------------------------------------------- BallPosteriorState
def _predictor(p, T, m, px, hidden, jitter=1e-9, clip_qs=True):
    from svgp_vae_amd.ball_predict import BallPredictor
    return BallPredictor(p, tmax=T, m=m, hidden=hidden, px=px, py=px, jitter=jitter, clip_qs=clip_qs)


def _close(got, want, keys=None):
    assert set(got) == set(want)
    for k in keys or want:
        e = PC.relerr(got[k].cpu().numpy(), want[k].cpu().numpy())
        print(f"{k}: {e:.2e}")
        assert e <= SC.PATH_TOL, (k, e)


@pytest.mark.parametrize("B,T,m,Q", [(3, 30, 15, 40), (2, 30, 65, 20)], ids=["fused", "large"])
def test_state_observe_predict_equals_the_predictors_predict(B, T, m, Q):
    from svgp_vae_amd.ball_predict import BallPosteriorState
    px, hidden, jp = 8, 16, JC.PATH_JITTER_DIRECT
    p, vid, observed, tq, eps = PC.predictor_problem(B, T, m, Q, px=px, hidden=hidden, seed=7 + m, drop_video=1)
    ft = np.arange(1, T + 1) * 1.0 + 0.25
    pred = _predictor(p, T, m, px, hidden)
    want = pred.predict(vid, tq, observed=observed, frame_times=ft, eps=eps)
    want_j = pred.predict(vid, tq, observed=observed, frame_times=ft, eps=eps, paths=True, return_cov=True, path_jitter=jp)
    state = pred.state(B)
    assert isinstance(state, BallPosteriorState) and state.n_seen == 0
    assert state.observe(vid, ft, observed) is state and state.n_seen == T
    assert state.route("predict", Q=Q)[:len(state.route("finalize"))] == state.route("finalize")
    _close(state.predict(tq, eps), want)
    _close(state.predict(tq, eps, paths=True, return_cov=True, path_jitter=jp), want_j)
    assert set(want_j) == {"frames", "p_m", "p_v", "z", "p_cov"}
    # three observe calls without frame_times reproduce predict's 1..T
    want = pred.predict(vid, tq, observed=observed, eps=eps)
    pieces = pred.state(B)
    for t0, t1 in ((0, 7), (7, 8), (8, T)):
        pieces.observe(vid[:, t0:t1], observed=observed[:, t0:t1])
    assert pieces.n_seen == T
    got = pieces.predict(tq, eps)
    _close(got, want)
    # a second predict at other query times: no encoder, no update, no finalize -- the route says so and post is untouched
    post, stats = pieces.post.clone(), pieces.stats.clone()
    assert pieces.route("predict", Q=5) == pieces.route("query", Q=5)
    tq2 = np.linspace(-1.0, T + 2.0, 5)
    again = pieces.predict(tq2)
    assert torch.equal(pieces.post, post) and torch.equal(pieces.stats, stats)
    _close(again, pred.predict(vid, tq2, observed=observed))
    # clone() is independent; reset() gives the prior
    twin = pieces.clone()
    twin.observe(vid[:, :3], frame_times=[T + 1.0, T + 2.0, T + 3.0])
    assert twin.n_seen == T + 3 and pieces.n_seen == T and torch.equal(pieces.stats, stats) and not torch.equal(twin.stats, stats)
    assert twin.route("predict", Q=5) != pieces.route("predict", Q=5)
    same = pieces.predict(tq, eps)
    for k in got:
        assert torch.equal(same[k], got[k]), k
    assert not torch.equal(twin.predict(tq, eps)["p_m"], got["p_m"]) and torch.equal(pieces.post, post)
    prior = twin.reset().predict(tq)
    assert twin.n_seen == 0 and float(prior["p_m"].abs().max()) <= SC.TOL and float((prior["p_v"] - 1).abs().max()) <= SC.TOL


# ---------------------------------------------------------------------------------------------- end to end
def test_stream_chunk_from_the_command_line(tmp_path):
    """The command line with --stream_chunk 7 against the same command line without it, one fresh child process each under its own
    time limit, on a checkpoint written here: the mask of --drop and the draw of --seed are the command's own in both."""
    from svgp_vae_amd import ball_predict as BP
    B, T, m, px, hidden = 3, 30, 5, 8, 16
    p, vid, _, _, _ = PC.predictor_problem(B, T, m, 1, px=px, hidden=hidden, seed=11)
    shapes = BP.param_shapes(m, px, px, hidden)
    theta = torch.cat([torch.as_tensor(p[k], dtype=torch.float64).reshape(-1) for k in shapes])
    ckpt, videos = str(tmp_path / "model.pt"), str(tmp_path / "videos.npy")
    torch.save({"theta": theta, "shapes": {k: tuple(v) for k, v in shapes.items()},
                "meta": dict(elbo="SVGPVAE_Hensman", tmax=T, m=m, hidden=hidden, px=px, py=px, jitter=1e-9, clip_qs=True, vidlt=2.0)}, ckpt)
    np.save(videos, vid.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    Q, got = 2 * (T - 1) + 1, {}
    for name, extra in (("plain", []), ("streamed", ["--stream_chunk", "7"])):
        out, cov = str(tmp_path / f"frames_{name}.npy"), str(tmp_path / f"cov_{name}.npy")
        r = subprocess.run([sys.executable, "-m", "svgp_vae_amd.ball_predict", "--checkpoint", ckpt, "--videos", videos, "--drop", "0.5",
                            "--upsample", "2", "--sample_paths", "--seed", "4", "--path_jitter", "1e-6", "--save_cov", cov, "--out", out]
                           + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
        assert r.returncode == 0, r.stdout + r.stderr
        print(r.stdout)
        got[name] = (np.load(out), np.load(cov), r.stdout)
        assert got[name][0].shape == (B, Q, px, px) and got[name][1].shape == (B, 2, Q, Q)
        assert "route (1 GP launch): k_ball_predict" in r.stdout and "joint route (1 GP launch): k_ball_predict_joint" in r.stdout
    assert "state routes" not in got["plain"][2]
    assert "state routes (these ran; the one-shot routes above were not launched), 5 pieces of at most 7 frames: update (1): " \
           "k_ball_state_update; finalize (1): k_ball_state_finalize; query (1): k_ball_state_query; query_joint (" in got["streamed"][2]
    e_f, e_c = PC.relerr(got["streamed"][0], got["plain"][0]), PC.relerr(got["streamed"][1], got["plain"][1])
    print(f"--stream_chunk 7 against the run without it: frames {e_f:.2e}, p_cov {e_c:.2e}")
    assert e_f <= SC.PATH_TOL and e_c <= SC.PATH_TOL
