"""The float32 streaming statistics (csrc/gp_stream_f32.hip) across their shape edges, resolved per element: bit equality with the
float64 reference on inputs where float32 is exact (a lost, doubled or misplaced row or element cannot hide behind the diagonal of
S), and on random data a bound per element from rounding analysis.  Case tables, inputs, references and the derivation of the
bounds: tests/stream_cases.py; tests/test_stream_cases_cpu.py guards them without a GPU.  Default stream, through
svgp_vae_amd.stream_stats."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stream_cases as SC

pytestmark = pytest.mark.gpu

GUARD = 256           # float32 elements of NaN on either side of an output, and behind the workspace


def _cuda(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda:0").contiguous()


def _guarded(shape):
    """A NaN-filled buffer and the view of `shape` in its middle, GUARD elements from either end."""
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda:0")
    return buf, buf[GUARD:GUARD + size].view(*shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _ratio(a, ref, bound):
    """max over the elements of |a - ref| / bound (0 / 0 counts as 0: an element whose bound is 0 must be exact)."""
    err = np.abs(np.asarray(a, np.float64) - ref)
    r = np.divide(err, bound, out=np.where(err == 0, 0.0, np.inf), where=bound > 0)
    return float(r.max())


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def _run_stats(n, m, L, K, means, vars_):
    """svgp_stream_stats_f32 into guarded outputs on a workspace of exactly the required size, poisoned with NaN and followed by a
    guard in the same allocation.  Returns (S, v, second-call S, second-call v, workspace) as numpy arrays after checking the
    guards."""
    from svgp_vae_amd import _lib, stream_stats as SS
    elems = _lib.load_library().svgp_stream_stats_workspace_elems(n, m, L)
    wsbuf = torch.full((elems + GUARD,), float("nan"), dtype=torch.float32, device="cuda:0")
    ws = wsbuf[:elems]
    Sbuf, S = _guarded((L, m, m))
    vbuf, v = _guarded((L, m))
    dK, dm, dv = _cuda(K), _cuda(means), _cuda(vars_)
    SS.stats(dK, dm, dv, ws=ws, S=S, v=v)
    S1, v1 = S.cpu().numpy(), v.cpu().numpy()
    assert bool(torch.isnan(wsbuf[elems:]).all()), "the call wrote behind its workspace"
    assert _guards_intact(Sbuf) and _guards_intact(vbuf), "the call wrote outside S or v"
    SS.stats(dK, dm, dv, ws=ws, S=S, v=v)                     # same workspace, not poisoned again
    S2, v2 = S.cpu().numpy(), v.cpu().numpy()
    assert bool(torch.isnan(wsbuf[elems:]).all()) and _guards_intact(Sbuf) and _guards_intact(vbuf)
    return S1, v1, S2, v2, ws.cpu().numpy()


@pytest.mark.parametrize("case", SC.STATS_EXACT, ids=lambda c: "n{} m{} L{}".format(*c[:3]))
def test_stats_exact(case):
    """Bit equality with the float64 reference; an element the reductions read without it having been written is NaN."""
    n, m, L, nsplit, nsplit_v, _ = case
    K, means, vars_, Sr, vr = SC.stats_exact_inputs(n, m, L)
    S1, v1, S2, v2, ws = _run_stats(n, m, L, K, means, vars_)
    assert np.array_equal(S1, Sr), "S: %d elements differ" % (S1 != Sr).sum()
    assert np.array_equal(v1, vr), "v: %d elements differ" % (v1 != vr).sum()
    assert np.array_equal(S1, S1.transpose(0, 2, 1))
    assert np.array_equal(S2, S1) and np.array_equal(v2, v1)
    # every row slice of the tile kernel is a whole number of 32-row chunks (only the last slice has a ragged chunk, so the
    # branch-free fetch holds everywhere else): the partial tiles, where the reduction reads them, are the sums over those rows
    lay = SC.stats_workspace_layout(n, m, L, nsplit, nsplit_v)
    part = ws[lay["part"]:lay["partv"]].reshape(nsplit, L, m, m)
    blk = np.arange(m) >> 5
    upper = blk[:, None] <= blk[None, :]
    for s in range(nsplit if nsplit > 1 else 0):
        rows = slice(s * lay["rows_per_split"], min(n, (s + 1) * lay["rows_per_split"]))
        Ss, _ = SC.stats64(K[rows], means[rows], vars_[rows])
        assert np.array_equal(part[s][:, upper], Ss[:, upper]), "row slice %d" % s


@pytest.mark.parametrize("m,L", SC.STATS_ONE_ROW)
def test_stats_one_row_resolves_computed_and_mirrored(m, L):
    """One row of random data: every element is one correctly rounded float32 product (operands cut to fewer bits on the matrix
    cores would show), k_i (p k_j) where the tile kernel computes it and the mirrored k_j (p k_i) where the reduction copies."""
    K, means, vars_, Sr, vr = SC.stats_one_row_inputs(m, L)
    S1, v1, S2, v2, _ = _run_stats(1, m, L, K, means, vars_)
    assert np.array_equal(S1, Sr), "S: %d elements differ" % (S1 != Sr).sum()
    assert np.array_equal(v1, vr)
    assert np.array_equal(S2, S1) and np.array_equal(v2, v1)


def test_stats_refuses_a_short_workspace():
    from svgp_vae_amd import SvgpError, _lib, stream_stats as SS
    n, m, L = 100, 36, 2
    K, means, vars_, _, _ = SC.stats_exact_inputs(300, 36, 16)
    Sr, vr = SC.stats64(K[:n], means[:n, :L], vars_[:n, :L])
    K, means, vars_ = _cuda(K[:n]), _cuda(means[:n, :L]), _cuda(vars_[:n, :L])
    elems = _lib.load_library().svgp_stream_stats_workspace_elems(n, m, L)
    ws = torch.zeros(elems, dtype=torch.float32, device="cuda:0")
    S = torch.full((L, m, m), -7.0, dtype=torch.float32, device="cuda:0")
    v = torch.full((L, m), -7.0, dtype=torch.float32, device="cuda:0")
    with pytest.raises(SvgpError, match="workspace"):
        SS.stats(K, means, vars_, ws=ws[:elems - 1], S=S, v=v)
    torch.cuda.synchronize()
    assert bool((S == -7.0).all()) and bool((v == -7.0).all()) and bool((ws == 0).all())
    SS.stats(K, means, vars_, ws=ws, S=S, v=v)                # the exact size is accepted
    assert np.array_equal(S.cpu().numpy(), Sr) and np.array_equal(v.cpu().numpy(), vr)


@pytest.mark.parametrize("case", SC.STATS_RANDOM, ids=lambda c: "n{} m{} L{}".format(*c[:3]))
def test_stats_random_within_the_rounding_bound(case):
    """|S - S64| <= (n + 4) 2^-24 sum_r |k_ri| p_rl |k_rj| for every element, and the same for v: the worst case of an n-term
    float32 inner product in any order.  A change of accumulation precision shows here."""
    n, m, L = case[:3]
    K, means, vars_, Sr, vr, bS, bv = SC.stats_random_inputs(n, m, L)
    S1, v1, S2, v2, _ = _run_stats(n, m, L, K, means, vars_)
    rS, rv = _ratio(S1, Sr, bS), _ratio(v1, vr, bv)
    print("max |err| / bound: S %.4f, v %.4f" % (rS, rv))
    assert rS <= 1.0 and rv <= 1.0
    # outside the 32 x 32 blocks on the diagonal the lower part is a copy of the upper one; inside them (i, j) and (j, i) are
    # two sums, sum k_i (p k_j) and sum k_j (p k_i), each within the bound of the same reference
    St = S1.transpose(0, 2, 1)
    blk = np.arange(m) >> 5
    copied = blk[:, None] != blk[None, :]
    assert np.array_equal(S1[:, copied], St[:, copied])
    assert (np.abs(S1.astype(np.float64) - St) <= 2 * bS).all()
    assert np.array_equal(S2, S1) and np.array_equal(v2, v1)


# ---- K_nm -------------------------------------------------------------------------------------------------------------------------
def _kdesc(kind, d1, d2, normalize, n_table):
    from svgp_vae_amd import stream_stats as SS
    return SS.kernel_desc(kind, d1, d2, normalize=normalize, n_table=n_table, params=SC.knm_params(kind, d1, d2))


def _widen(a, extra):
    """`a` as the leading columns of a matrix `extra` columns wider, the rest NaN."""
    wide = np.full((a.shape[0], a.shape[1] + extra), np.nan, np.float32)
    wide[:, :a.shape[1]] = a
    return wide


def _knm(kd, x, z, tab, extra=0):
    """K_nm and K_mm of batch rows x and inducing rows z, each written into a guarded buffer."""
    from svgp_vae_amd import stream_stats as SS
    n, m = x.shape[0], z.shape[0]
    fr = SS.features(kd, _cuda(_widen(x, extra)), inducing=False, table=None if tab is None else _cuda(tab))
    fi = SS.features(kd, _cuda(_widen(z, extra)), inducing=True)
    out = []
    for f, rows in ((fr, n), (fi, m)):
        buf, K = _guarded((rows, m))
        SS.knm(kd, f, rows, fi, m, out=K)
        out.append(K.cpu().numpy())
        assert _guards_intact(buf), "the call wrote outside K"
    return out


@pytest.mark.parametrize("case", SC.KNM_EXACT + [c + (3,) for c in SC.KNM_EXACT_WIDE], ids=str)
def test_knm_exact(case):
    """Linear x linear on integers: both dot products and their product are exact."""
    kind, d1, d2, n, m = case[:5]
    x, z, tab, knm_ref, kmm_ref = SC.knm_exact_inputs(kind, d1, d2, n, m)
    knm, kmm = _knm(_kdesc(kind, d1, d2, False, SC.N_ACT), x, z, tab, extra=case[5] if len(case) > 5 else 0)
    assert np.array_equal(knm, knm_ref), "K_nm: %d elements differ" % (knm != knm_ref).sum()
    assert np.array_equal(kmm, kmm_ref) and np.array_equal(kmm, kmm.T)


@pytest.mark.parametrize("case", SC.KNM_BOUNDED, ids=str)
def test_knm_within_the_rounding_bound(case):
    kind, d1, d2, normalize, table, n, m = case
    x, z, tab, knm_ref, b_nm, kmm_ref, b_mm = SC.knm_bounded_inputs(*case)
    n_table = 0 if tab is None else tab.shape[0]
    knm, kmm = _knm(_kdesc(kind, d1, d2, normalize, n_table), x, z, tab)
    r_nm, r_mm = _ratio(knm, knm_ref, b_nm), _ratio(kmm, kmm_ref, b_mm)
    print("max |err| / bound: K_nm %.4f, K_mm %.4f" % (r_nm, r_mm))
    assert r_nm <= 1.0 and r_mm <= 1.0
    # K_mm against its own transpose: both elements are within the bound of the same (symmetric) reference
    assert (np.abs(kmm.astype(np.float64) - kmm.T) <= b_mm + b_mm.T).all()


def _features_raw(kd, n, x, ldx, inducing, table, feat):
    from svgp_vae_amd import _lib
    _lib.call("svgp_stream_features_f32", C.byref(kd), n, x.data_ptr(), ldx, int(inducing),
              None if table is None else table.data_ptr(), feat.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _knm_raw(kd, n, m, fr, fi, K):
    from svgp_vae_amd import _lib
    _lib.call("svgp_stream_knm_f32", C.byref(kd), n, m, fr.data_ptr(), fi.data_ptr(), K.data_ptr(),
              torch.cuda.current_stream().cuda_stream)


def test_refusals_leave_the_output_alone():
    from svgp_vae_amd import SvgpError
    n, m = 5, 4
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device="cuda:0")
    untouched = lambda t: bool((t == -7.0).all())
    x = torch.ones((n, 40), dtype=torch.float32, device="cuda:0")
    tab = torch.ones((SC.N_ACT, 8), dtype=torch.float32, device="cuda:0")
    feat, K = sent(n * 41), sent(n, m)
    # a feature split without an instantiation: the features exist for any split, the K_nm build refuses
    kd = _kdesc(0, 2, 5, False, 0)
    _features_raw(kd, n, x, 7, True, None, feat)
    with pytest.raises(SvgpError, match="no instantiation"):
        _knm_raw(kd, n, m, feat, feat, K)
    feat.fill_(-7.0)
    # periodic x linear is (cos, sin) x M
    kd = _kdesc(0, 3, 4, False, 0)
    with pytest.raises(SvgpError, match="d1 = 2"):
        _features_raw(kd, n, x, 7, True, None, feat)
    with pytest.raises(SvgpError, match="d1 = 2"):
        _knm_raw(kd, n, m, x, x, K)
    # the row stride one short of the columns read: periodic rows, SPRITES inducing rows, SPRITES batch rows
    for kd, inducing, need in ((_kdesc(0, 2, 8, False, 0), False, 10), (_kdesc(1, 8, 16, False, SC.N_ACT), True, 24),
                               (_kdesc(2, 4, 6, False, SC.N_ACT), False, 7)):
        with pytest.raises(SvgpError, match="row stride"):
            _features_raw(kd, n, x, need - 1, inducing, tab, feat)
    # SPRITES batch rows gather the action vector: no table, or a table of no rows
    with pytest.raises(SvgpError, match="table"):
        _features_raw(_kdesc(1, 8, 16, False, SC.N_ACT), n, x, 17, False, None, feat)
    with pytest.raises(SvgpError, match="table"):
        _features_raw(_kdesc(1, 8, 16, False, 0), n, x, 17, False, tab, feat)
    torch.cuda.synchronize()
    assert untouched(feat) and untouched(K)
    # n = 0 is accepted and writes nothing
    kd = _kdesc(1, 8, 16, False, SC.N_ACT)
    _features_raw(kd, 0, x, 17, False, tab, feat)
    _knm_raw(kd, 0, m, x, x, K)
    torch.cuda.synchronize()
    assert untouched(feat) and untouched(K)
