"""The MNIST SVGP step over the shape range svgp_check_cfg accepts (1 <= L <= 64, 1 <= m <= 2048, M <= 128, any b up to the
engine's capacity), at the shapes where the single-GPU step changes form, against the float64 oracle.

What changes with the shape (svgp-vae_amd/csrc): L <= 56 lets the reverse statistics ride in the reverse factor launch, whose channel
workgroup l waits on ws.flags[8 + l] (api.hip stat_rides); the decoder's zbar runs 8 lanes per channel over 512 threads; the LDS of
the encoder / decoder reverse launches grows with L (one workgroup per CU near L = 64); m == 32 has its own kernel instance, m <= 32
the five-LDS-matrix form and the deferred inverse in the decoder launch (aji_in_dec); m > 64 the global-memory path; the statistics
row partials are sized from the capacity b_max, not from b; 256 rows is the limit of the weight-gradient partial slots.  Where the
m <= 64 step's decoder split does not apply (m > 64), the one-launch decoder reverse pass fits the LDS up to L = 21 only and the
data and weight halves take over from L = 22 (svgp_mnist_decoder_bwd).
Every step must also leave the hand-off counters in ws.flags re-armed (all zero) and raise no timed-out hand-off.
"""
import pytest
import torch

from tests import helpers as H
from tests.helpers import _compare_step

pytestmark = pytest.mark.gpu


def _assert_handoffs_clean(eng):
    fl = eng.ws_view("flags", (64,)).view(torch.int64)
    assert torch.count_nonzero(fl) == 0, fl.tolist()
    eng.scalars()                      # raises SvgpError("... hand-off ...") if a consumer gave up waiting


# name: (b, m, L, M), toy_problem / _compare_step keywords
CASES = {
    "L17": ((256, 32, 17, 8), dict(geco=False)),                        # first channel past every other test's L
    "L33": ((256, 32, 33, 8), dict(geco=True)),                         # zbar lanes of the second 256 threads
    "L56": ((256, 32, 56, 8), dict(geco=False)),                        # last L with stat_rides: flags[63]
    "L57": ((256, 32, 57, 8), dict(geco=True, with_table=False)),       # first L without: svgp_gp_stats_bwd of its own
    "L64": ((256, 32, 64, 8), dict(geco=False, K_obj_normalize=True)),  # largest LDS of the encoder / decoder reverse launches
    "L1": ((256, 64, 1, 16), dict(geco=True, jitter=1e-4)),             # one channel, m at the LDS limit
    "m64L64": ((200, 64, 64, 16), dict(geco=False, jitter=1e-4)),       # four-matrix form at the largest L
    "m72L64": ((100, 72, 64, 16), dict(geco=True, jitter=1e-4)),        # first global-memory (large-m) shape at the largest L
    "m31": ((150, 31, 40, 8), dict(geco=False)),                        # generic instance below kern<32>: five matrices, aji_in_dec
    "m33": ((150, 33, 40, 8), dict(geco=True)),                         # ... above it: four matrices, the inverse in the row stage
    "m1": ((60, 1, 4, 3), dict(geco=True)),                             # 256 rows per workgroup
    "m2": ((60, 2, 3, 3), dict(geco=False)),                            # 128
    "m7": ((60, 7, 5, 3), dict(geco=True)),                             # 36
    "b257": ((257, 16, 16, 4), dict(geco=False)),                       # one row past SVGP_MAX_PART
    "m72L22": ((100, 72, 22, 16), dict(geco=False, jitter=1e-4)),       # first L whose decoder reverse pass at m > 64 is two launches
}


@pytest.mark.parametrize("case", list(CASES))
def test_step_matches_oracle_across_the_shape_range(case):
    (b, m, L, M), kw = CASES[case]
    kw = dict(kw)
    with_table = kw.pop("with_table", True)
    p = H.toy_problem(b=b, m=m, L=L, M=M, n_obj=60, seed=100 + list(CASES).index(case), with_table=with_table)
    bad, eng = _compare_step(*p, N_train=4050.0, label=case, **kw)
    assert not bad, "\n".join(bad)
    _assert_handoffs_clean(eng)


@pytest.mark.parametrize("L", [16, 64])
def test_batches_below_capacity_on_one_engine(L):
    """One engine with 256 rows of capacity (4 statistics partitions, some of them empty for small b) given 1, 3, 127 and 255
    rows, then a full batch: each compared against the oracle for that batch."""
    params, images, aux, eps = H.toy_problem(b=256, m=32, L=L, M=8, n_obj=60, seed=130 + L)
    eng = None
    for b in (1, 3, 127, 255, 256):
        # 1 or 3 rows against 32 inducing points: the oracle's own response to a one-ulp input perturbation is 1e-9 .. 1e-7
        # (field e), so those two batches are held to 20x of it; the rest are well conditioned and take the fixed tolerances
        bad, eng = _compare_step(params, images[:b].contiguous(), aux[:b].contiguous(), eps[:b].contiguous(), geco=L == 64,
                                 N_train=256.0, b_max=256, eng=eng, self_consistency=b <= 3, label=f"L{L} b{b} of 256")
        assert not bad, "\n".join(bad)
        assert eng.wl.stat_parts == 4
        _assert_handoffs_clean(eng)


@pytest.mark.parametrize("b_max,parts", [(127, 1), (128, 4)])
def test_full_batch_at_the_statistics_partition_threshold(b_max, parts):
    params, images, aux, eps = H.toy_problem(b=b_max, m=32, L=16, M=8, n_obj=60, seed=140 + b_max)
    bad, eng = _compare_step(params, images, aux, eps, geco=False, N_train=4050.0, b_max=b_max, label=f"b_max {b_max}")
    assert not bad, "\n".join(bad)
    assert eng.wl.stat_parts == parts
    _assert_handoffs_clean(eng)


def _bound_engine(L, seed):
    params, images, aux, eps = H.toy_problem(b=256, m=32, L=L, M=8, n_obj=60, seed=seed)
    eng = H.engine_for(params, 256, geco=True)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    return eng


@pytest.mark.parametrize("L", [16, 56, 64])
def test_merged_launch_fallbacks_are_bit_equal(L, monkeypatch):
    """SVGP_ENC_KM_MERGE=0 (kernel-matrix VJP and encoder reverse pass in two launches) and SVGP_SUM_MERGE=0 (the closing sums in
    a launch of their own): the documented fallbacks must give the merged step's numbers bit for bit."""
    out = {}
    for name, flag in (("merged", None), ("enc_km", "SVGP_ENC_KM_MERGE"), ("sum", "SVGP_SUM_MERGE")):
        for f in ("SVGP_ENC_KM_MERGE", "SVGP_SUM_MERGE"):
            if f == flag:
                monkeypatch.setenv(f, "0")
            else:
                monkeypatch.delenv(f, raising=False)
        eng = _bound_engine(L, seed=150 + L)
        for _ in range(3):
            eng.run(adam=True)
        eng.synchronize()
        _assert_handoffs_clean(eng)
        out[name] = (eng.theta.clone(), eng.state.clone(), eng.scalars()["elbo"])
    for name in ("enc_km", "sum"):
        assert torch.equal(out[name][0], out["merged"][0]), name
        assert torch.equal(out[name][1], out["merged"][1]), name
        assert out[name][2] == out["merged"][2], name


def test_graph_replay_equals_eager_at_the_largest_L():
    """Captured once, replayed three times at one workgroup per CU in the large-LDS launches: the counters in ws.flags must
    re-arm between replays."""
    a, b_ = _bound_engine(64, seed=160), _bound_engine(64, seed=160)
    for _ in range(3):
        a.run(adam=True)
    a.synchronize()
    b_.capture("step", adam=True)          # capture does not execute
    for _ in range(3):
        b_.replay("step")
    b_.synchronize()
    _assert_handoffs_clean(a)
    _assert_handoffs_clean(b_)
    assert torch.equal(a.theta, b_.theta)
    assert a.scalars() == b_.scalars()
