"""Guards the case tables of tests/stream_cases.py without a GPU: the exactness condition of the exact statistics cases, the row
slices each statistics case was written for (svgp_stream_stats_workspace_elems is a host-only call), the per-element bounds against
a plain numpy float32 evaluation, and that the K_nm tables reach every instantiation and both sides of every edge they name."""
import os

import numpy as np
import pytest

import svgp_vae_amd
from svgp_vae_amd import _lib
from tests import stream_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(svgp_vae_amd.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


@pytest.mark.parametrize("case", SC.STATS_EXACT, ids=lambda c: "n{} m{} L{}".format(*c[:3]))
def test_exact_statistics_are_exact_in_float32(case):
    n, m, L = case[:3]
    assert 96 * n <= 2 ** 24
    K, means, vars_, S, v = SC.stats_exact_inputs(n, m, L)
    assert set(np.unique(K)) <= {-2, -1, 0, 1, 2} and set(np.unique(means)) <= set(range(-3, 4))
    assert set(np.unique(vars_)) <= {0, 0.25, 0.5, 1, 2, 4}
    for a, cap in ((S, 16 * n), (v, 24 * n)):
        assert np.array_equal(4 * a, np.rint(4 * a)) and np.abs(a).max(initial=0) <= cap
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert np.array_equal(S, S.transpose(0, 2, 1))
    if n >= 31:                                           # every value of the three sets is drawn, zeros of var among them
        assert len(np.unique(K)) == 5 and len(np.unique(vars_)) == 6 and len(np.unique(means)) == 7
    # numpy's float32 products are exact on these inputs too
    S32, v32 = SC.stats_f32_numpy(K, means, vars_)
    assert np.array_equal(S32, S) and np.array_equal(v32, v)


@pytest.mark.parametrize("case", SC.STATS_EXACT + [c + ("random",) for c in SC.STATS_RANDOM], ids=lambda c: "n{} m{} L{}".format(*c[:3]))
def test_statistics_cases_reach_their_row_slices(case):
    n, m, L, nsplit, nsplit_v = case[:5]
    lay = SC.stats_workspace_layout(n, m, L, nsplit, nsplit_v)
    assert lay["total"] == SC.round_up(2 * L * n, 4) + nsplit * L * m * m + nsplit_v * L * m
    assert _lib.load_library().svgp_stream_stats_workspace_elems(n, m, L) == lay["total"]
    assert (nsplit - 1) * lay["rows_per_split"] < n <= nsplit * lay["rows_per_split"]      # no empty tile slice


def test_statistics_table_holds_the_edges_it_names():
    shapes = {c[:3] for c in SC.STATS_EXACT}
    assert len(shapes) == len(SC.STATS_EXACT)
    ms = {m for _, m, _ in shapes}
    assert {31, 32, 33, 255, 256, 257, 260, 512, 516, 1028, 2048} <= ms
    assert {-(-m // 256) for m in ms} >= {1, 2, 3, 5, 8}                    # tiles per side
    assert {n for n, _, _ in shapes} >= {1, 31, 32, 33}
    assert {-(-L // 16) for _, _, L in shapes} >= {1, 2, 3}                 # channel passes of k_stats_v_f32
    assert {c[3] for c in SC.STATS_EXACT} >= {1, 2, 64} and max(c[4] for c in SC.STATS_EXACT) == 512
    n, m, L, nsplit, nsplit_v = SC.STATS_EXACT[-2][:5]
    lay = SC.stats_workspace_layout(n, m, L, nsplit, nsplit_v)
    assert (lay["rows_per_split"], n - lay["rows_per_split"], -(-n // nsplit_v)) == (2080, 2017, 257)
    n, m, L, nsplit, nsplit_v = SC.STATS_EXACT[-1][:5]
    assert n - (nsplit - 1) * SC.stats_workspace_layout(n, m, L, nsplit, nsplit_v)["rows_per_split"] == 33
    assert [c[:3] for c in SC.STATS_RANDOM[:4]] == [(1000, 64, 3), (5000, 300, 5), (4100, 516, 2), (40, 30, 17)]


@pytest.mark.parametrize("case", SC.STATS_RANDOM, ids=lambda c: "n{} m{} L{}".format(*c[:3]))
def test_random_statistics_bound_holds_for_numpy_float32(case):
    K, means, vars_, S, v, bS, bv = SC.stats_random_inputs(*case[:3])
    assert (vars_ == 0).any() and K.dtype == means.dtype == vars_.dtype == np.float32
    S32, v32 = SC.stats_f32_numpy(K, means, vars_)
    assert (np.abs(S32 - S) <= bS).all() and (np.abs(v32 - v) <= bv).all()


@pytest.mark.parametrize("m,L", SC.STATS_ONE_ROW)
def test_one_row_statistics_tell_computed_from_mirrored(m, L):
    """Inside the diagonal blocks the two products of an element pair differ in some last bits, so bit equality with the table's
    S holds only if exactly the blocks bi <= bj are computed; and S is within the bound of section 2 of the float64 reference."""
    K, means, vars_, S, v = SC.stats_one_row_inputs(m, L)
    blk = np.arange(m) >> 5
    inside = blk[:, None] == blk[None, :]
    St = S.transpose(0, 2, 1)
    assert (S != St)[:, inside].sum() >= m and np.array_equal(S[:, ~inside], St[:, ~inside])
    assert m > 64 and (m > 256) == (m == 300)             # more than one block; (300: more than one tile)
    S64, v64 = SC.stats64(K, means, vars_)
    bS, bv = SC.stats64(np.abs(K), np.abs(means), vars_)
    assert (np.abs(S - S64) <= 5 * SC.U * bS).all() and (np.abs(v - v64) <= 5 * SC.U * bv).all()


def test_knm_tables_cover_every_instantiation_and_edge():
    assert {c[:3] for c in SC.KNM_BOUNDED} == set(SC.KNM_INSTANCES) and len(SC.KNM_INSTANCES) == 8
    for kind, d1, d2 in SC.KNM_INSTANCES:
        sub = [c for c in SC.KNM_BOUNDED if c[:3] == (kind, d1, d2)]
        assert {c[3] for c in sub} == ({False} if kind == 2 else {False, True})
        assert {c[4] for c in sub} == ({True, False} if kind == 0 else {True})
    assert (0, 2, 32, True, True, 300, 1100) in SC.KNM_BOUNDED
    for (kind, d1, d2), rb in SC.KNM_ROW_BLOCK.items():
        assert rb == (32 if d1 + d2 <= 12 else 128)
        ns = {c[3] for c in SC.KNM_EXACT if c[:3] == (kind, d1, d2)}
        assert {rb - 1, rb, rb + 1} <= ns
        for n in ns:
            assert {c[4] for c in SC.KNM_EXACT if c[:4] == (kind, d1, d2, n)} == {1, 3, 4, 1023, 1024, 1025, 1028}
    assert {c[:3] for c in SC.KNM_EXACT_WIDE} == set(SC.KNM_ROW_BLOCK)


@pytest.mark.parametrize("case", SC.KNM_EXACT[::7] + SC.KNM_EXACT[6::7], ids=str)
def test_exact_knm_is_exact_in_float32(case):
    kind, d1, d2, n, m = case
    x, z, tab, knm, kmm = SC.knm_exact_inputs(*case)
    for a in (x[:, 1:], z, tab):
        assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 3
    assert np.abs(knm).max() <= 81 * d1 * d2 < 2 ** 24 and np.array_equal(knm, np.rint(knm))
    assert np.array_equal(SC.knm_f32_numpy(kind, d1, d2, False, x, z, tab, False), knm)
    assert np.array_equal(kmm, kmm.T)


@pytest.mark.parametrize("case", SC.KNM_BOUNDED, ids=str)
def test_knm_bound_holds_for_numpy_float32_with_margin(case):
    kind, d1, d2, normalize, table, n, m = case
    x, z, tab, knm, b_nm, kmm, b_mm = SC.knm_bounded_inputs(*case)
    assert (tab is not None) == (table or kind != 0)
    assert (b_nm > 0).all() and (b_mm > 0).all()
    r_nm = np.abs(SC.knm_f32_numpy(kind, d1, d2, normalize, x, z, tab, False) - knm) / b_nm
    r_mm = np.abs(SC.knm_f32_numpy(kind, d1, d2, normalize, z, z, None, True) - kmm) / b_mm
    print("max |err| / bound: K_nm %.3f, K_mm %.3f" % (r_nm.max(), r_mm.max()))
    assert r_nm.max() < 0.5 and r_mm.max() < 0.5


def test_references_agree_with_the_first_stream_suite():
    """stream_cases restates the float64 functions of tests/test_gpu_stream_f32.py; they must stay the same functions."""
    from tests import test_gpu_stream_f32 as T
    rng = np.random.default_rng(5)
    n, m, M = 9, 7, 4
    tab = rng.normal(0, 1.5, (SC.N_OBJ, M))
    x = np.concatenate([rng.integers(0, SC.N_OBJ, (n, 1)).astype(float), rng.uniform(0, 6, (n, 1)), rng.normal(0, 1, (n, M))], 1)
    z = np.concatenate([np.zeros((m, 1)), rng.uniform(0, 6, (m, 1)), rng.normal(0, 1, (m, M))], 1)
    for table, nz, ind in ((tab, False, False), (None, True, False), (None, True, True)):
        assert np.array_equal(SC.mnist_kernel64(x, z, 1.3, 0.9, table, nz, ind), T._mnist_kernel64(x, z, 1.3, 0.9, table, nz, ind))
    tab = rng.normal(0, 1, (SC.N_ACT, 4))
    x = np.concatenate([rng.integers(0, SC.N_ACT, (n, 1)).astype(float), rng.normal(0, 1, (n, 6))], 1)
    z = rng.normal(0, 1, (m, 10))
    for nz, se in ((False, None), (True, None), (False, (2.0, 1.0, 2.5, 1.0))):
        assert np.array_equal(SC.sprites_kernel64(x, z, tab, nz, se, False, 4), T._sprites_kernel64(x, z, tab, nz, se, False, 4))
    K, means, vars_ = rng.normal(0, 1, (n, m)), rng.normal(0, 1, (n, 3)), rng.uniform(0.1, 2, (n, 3))
    vars_[2, 1] = 0.0
    for a, b in zip(SC.stats64(K, means, vars_), T._stats64(K, means, vars_)):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)        # one matrix product per channel against one einsum
