"""The Titsias form of the MNIST step (cfg.titsias, csrc/gp_titsias.hip) over the shape range svgp_check_cfg accepts, at the shapes
where the code changes form, against the oracle's LITERAL b x b branch (tests/titsias_cases.py holds the table, the bars and the
references; tests/test_titsias_envelope_oracle_cpu.py shows that the references are far more exact than the bars).

What changes with the shape: a capacity of at least 128 rows at m <= 64 gives four row partials of the Hensman statistic S, which
the reverse stage sums (L x 4 blocks, empty ones for small batches; the layout comes from the capacity, the kernels use the current
rows); the single-workgroup scalar kernel loops over L; ws.scr_mm holds (L + 3) m^2 of the stage's matrices; m = 32 has its own
kernel instance, m > 64 the global-memory path, m >= 512 the potrf + potri inverse; and for (L - 1) m < 2 L (L = 1, m <= 2, and
m = 3 with L = 2) the reverse stage's W | cA | cB need more than the L b m elements ws.Knbar_part otherwise has.
Every step must leave the hand-off counters in ws.flags re-armed (all zero) and raise no timed-out hand-off."""
import pytest
import torch

from tests import helpers as H
from tests import titsias_cases as TC

pytestmark = pytest.mark.gpu


def _assert_handoffs_clean(eng):
    fl = eng.ws_view("flags", (64,)).view(torch.int64)
    assert torch.count_nonzero(fl) == 0, fl.tolist()
    eng.scalars()                      # raises SvgpError("... hand-off ...") if a consumer gave up waiting


@pytest.mark.parametrize("case", TC.ENVELOPE_CASES)
def test_titsias_step_matches_literal_oracle_across_the_shape_range(case):
    eng = TC.engine(case)
    bad, _ = TC.compare(case, eng)
    assert not bad, "\n".join(bad)
    assert eng.wl.stat_parts == TC.expected_stat_parts(TC.CASES[case])
    _assert_handoffs_clean(eng)


def test_titsias_batches_below_capacity_on_one_engine():
    """One engine with 256 rows of capacity (four partials of S, some of them empty for small batches) given 1, 3, 127, 255 and
    256 rows, then 3 rows again (partials that held a full batch must read as empty): each against the oracle for that batch."""
    case = TC.CAPACITY_CASE
    eng = TC.engine(case, b_max=256)
    for rows in TC.CAPACITY_BATCHES:
        bad, _ = TC.compare(case, eng, None if rows == TC.CASES[case]["b"] else rows, label=f"{case} rows {rows} of 256")
        assert not bad, "\n".join(bad)
        assert eng.wl.stat_parts == 4
        _assert_handoffs_clean(eng)


@pytest.mark.parametrize("case,parts", [("b127", 1), ("b128", 4)])
def test_titsias_full_batch_at_the_statistics_partition_threshold(case, parts):
    eng = TC.engine(case)
    bad, _ = TC.compare(case, eng)
    assert not bad, "\n".join(bad)
    assert eng.wl.stat_parts == parts == TC.expected_stat_parts(TC.CASES[case])
    _assert_handoffs_clean(eng)


@pytest.mark.parametrize("case", TC.GRAPH_CASES)
def test_titsias_graph_replay_equals_eager(case):
    """The Titsias step captured once and replayed three times against three eager steps of a twin engine: bit-equal."""
    _, images, aux, eps = TC.rows_of(case)
    twins = []
    for _ in range(2):
        eng = TC.engine(case)
        dev = eng.device
        eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
        twins.append(eng)
    a, g = twins
    for _ in range(3):
        a.run(adam=True)
    a.synchronize()
    g.capture("step", adam=True)           # capture does not execute
    for _ in range(3):
        g.replay("step")
    g.synchronize()
    _assert_handoffs_clean(a)
    _assert_handoffs_clean(g)
    assert a.scalars()["adam_t"] == 3.0
    assert torch.equal(a.theta, g.theta)
    assert torch.equal(a.state, g.state)
    assert a.scalars()["elbo"] == g.scalars()["elbo"]


@pytest.mark.parametrize("b,m,L,M", [(96, 72, 4, 16), (256, 32, 16, 8)])
def test_titsias_two_virtual_ranks_equal_single_engine(b, m, L, M):
    """Row sharding at m > 64 -- where L divisible by the rank count would select the channel-sharded schedule, which excludes
    Titsias: the plan must stay the row-sharded one -- and at the config-2 shape (four row partials per rank): two Adam steps of
    two virtual ranks against a single engine, at the bars of tests/test_gpu_titsias.py."""
    from svgp_vae_amd.engine import shard_rows
    from tests.test_gpu_dp_virtual import _lockstep
    G = 2
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=M, n_obj=60, seed=390 + m)
    kw = dict(geco=True, clip_qs=True, N_train=500.0, jitter=1e-4, titsias=True)
    single = H.engine_for(params, b, **kw)
    dev = single.device
    di, da, de = images.to(dev), aux.to(dev), eps.to(dev)
    single.bind(di, da, de)
    ranks = []
    for r in range(G):
        lo, hi = shard_rows(b, G, r)
        e = H.engine_for(params, hi - lo, rank=r, world_size=G, **kw)
        e.set_batch_size(hi - lo, b)
        e.bind(di[lo:hi].contiguous(), da[lo:hi].contiguous(), de[lo:hi].contiguous())
        assert L % G == 0 and not e.channel_sharded()
        ranks.append(e)
    for step in range(2):
        single.run(adam=True)
        single.synchronize()
        _lockstep(ranks, adam=True)
        ref = single.scalars()
        for e in ranks:
            sc = e.scalars()
            for k in ("elbo", "kl_term", "inside_elbo", "ce_term", "c_ma", "lagrange"):
                print(f"m{m} step {step} rank {e.rank} {k}: {abs(sc[k] - ref[k]) / max(1.0, abs(ref[k])):.2e}")
                assert abs(sc[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (step, k, sc[k], ref[k])
            # Adam's first steps are sign steps, lr g / (|g| + eps): a gradient wrong by a factor passes the two checks above and
            # below (m = 72 did, with the replicated part of Kbar counted once per rank).  So the reduced gradients themselves
            # are compared, at the bar gradients are held to everywhere (tests/titsias_cases.py).
            g, gs = e.grads(), single.grads()
            for k in gs:
                print(f"m{m} step {step} rank {e.rank} grad {k}: {H.relerr(g[k], gs[k]):.2e}")
                assert H.relerr(g[k], gs[k]) < TC.GRAD_TOL, (step, k)
            print(f"m{m} step {step} rank {e.rank} theta: {H.relerr(e.theta, single.theta):.2e}")
            assert H.relerr(e.theta, single.theta) < 1e-7
            _assert_handoffs_clean(e)
