"""Guard for tests/test_gpu_dp_envelope.py: at every case of its tables (tests/dp_cases.py) the references must be far more exact
than the bars the data-parallel step is held to, and the one thing row sharding changes in exact arithmetic's stead -- the order in
which the statistics are added -- must not itself consume the bar.

(a) The oracle evaluated twice, the second time with its real inputs perturbed by one ulp, changes by at most bar / 100 per
    quantity, in the measure of that quantity's bar.
(b) The rank-sum restatement (dp_cases._restate: S_l, v_l formed per shard with the oracle's own formulas and added in rank order,
    every later stage from the sum) differs from the oracle on the whole batch by at most bar / 10.
(c) For the cases under the ill rule, which cannot pass (a) or (b), the restatement -- a correct float64 evaluation -- lies inside
    the bound the GPU is given: max(bar, 20 x the one-ulp response).
A case that fails (a) or (b) gets another seed, N_train or jitter, never a wider bar.  (Measured when the table was written:
NOTEBOOK.md, "Data-parallel envelope".)"""
import pytest

from tests import dp_cases as DC


def test_the_tables_invariants():
    ill = [c for c, cs in DC.ALL.items() if cs["ill"]]
    assert set(ill) <= set(DC.ILL_ALLOWED) and {"big520", "ch520"} <= set(ill), ill
    for flag, value in (("geco", True), ("geco", False), ("normalize", True), ("with_table", False), ("clip_qs", False)):
        assert sum(cs[flag] == value for cs in DC.CASES.values()) >= 2, flag
    for c, cs in DC.CASES.items():
        assert cs["G"] > 1 and max(hi - lo for lo, hi in DC.shards(c)) <= cs["b_max"], c
        if cs["route"] == DC.CHANNELS:
            assert cs["m"] > 64 and cs["L"] % cs["G"] == 0 and not cs["split_grad_exchange"], c
        if cs["route"] == DC.ROWS_LARGE:
            assert cs["m"] > 64 and cs["L"] % cs["G"] != 0, c
        if cs["route"] == DC.ROWS:
            assert cs["m"] <= 64, c
    assert sorted(hi - lo for lo, hi in DC.shards("rows5")) == [1, 2, 2]
    assert [hi - lo for lo, hi in DC.shards("ragged8")] == [27, 27] + [26] * 6
    assert (DC.expected_stat_parts("cap127"), DC.expected_stat_parts("cap128"), DC.expected_stat_parts("cap129")) == (1, 4, 4)
    assert DC.expected_stat_parts("one_block") == 1
    # the DP-entry table: every m <= 64 shape with the split gradient exchange off / on, two of them also with one statistics block;
    # every m > 64 shape on the wire-buffer workspace with the blocks as they are / packed
    for name, (shape, _) in DC.ENTRY_SHAPES.items():
        mine = {c: cs for c, cs in DC.ENTRY_CASES.items() if c.startswith(name + "-")}
        if shape[1] > 64:
            assert sorted(cs["pack"] for cs in mine.values()) == ["0", "1"] and all(cs["single_stat_block"] for cs in mine.values())
        else:
            assert {(cs["split_grad_exchange"], bool(cs["single_stat_block"])) for cs in mine.values()} == \
                {(s, o) for s in (False, True) for o in ((False, True) if name in DC.ENTRY_ONE_BLOCK else (False,))}


@pytest.mark.parametrize("case", list(DC.ALL))
def test_every_case_takes_the_route_its_comment_claims(case):
    """From the library's plan of STEP_FORM_DP (svgp_mnist_step_route; no device): the channel-sharded cases reduce-scatter, the
    others do not; the split cases exchange gradC in its two halves; the symmetric blocks travel packed exactly where the case
    says; rank 0 and rank G - 1 print the same text."""
    cs = DC.ALL[case]
    text = DC.route_text(case, 0)
    assert text == DC.route_text(case, cs["G"] - 1)
    lines = text.splitlines()
    assert ("main reduce_scatter v" in lines) == (cs["route"] == DC.CHANNELS)
    split = cs["split_grad_exchange"] and cs["route"] != DC.CHANNELS
    assert ("side1 allreduce gradC_hi" in lines and "main allreduce gradC_lo" in lines) == split
    assert ("main allreduce gradC" in lines) == (not split)
    if cs["route"] == DC.CHANNELS:
        packed = cs["pack"] == "1" or (cs["pack"] is None and cs["m"] >= 512)
        assert ("main reduce_scatter S packed" in lines) == packed and ("main reduce_scatter S" in lines) == (not packed)
        assert any(ln.endswith("svgp_big_factor_bwd FINAL") or ln.endswith("svgp_big_factor_bwd LATE") for ln in lines)
    else:
        assert "main allreduce statA" in lines and "main allreduce statB" in lines
        assert ("main svgp_gp_titsias_bwd" in lines) == cs["titsias"]
    if cs["route"] == DC.ROWS_LARGE:
        assert "main svgp_gp_factor_bwd_late_a" in lines
    if cs["m"] > 64 and not cs["titsias"]:   # m > 64 beyond L = 21: the decoder's reverse pass is the plain entry (two launches inside)
        assert "main svgp_mnist_decoder_bwd" in lines
    assert "main svgp_gp_stats_factor_bwd_wgrad" not in lines      # no statistics rider where something is exchanged in between


# (the DP-entry variants of one shape share one problem and one reference: one of them stands for the shape)
@pytest.mark.parametrize("case", list(DC.CASES) + sorted({DC._canonical(c) for c in DC.ENTRY_CASES}))
def test_case_references_are_far_more_exact_than_the_bars(case):
    resp, gap, tol = DC.oracle_response(case), DC.restatement_gap(case), DC.tolerances(case)
    wr, wg = DC.worst(resp), DC.worst(gap)
    print(f"{case}: one-ulp response scalars {wr['scalar']:.1e} fields {wr['field']:.1e} gradients {wr['grad']:.1e}; "
          f"rank-sum gap scalars {wg['scalar']:.1e} fields {wg['field']:.1e} gradients {wg['grad']:.1e}")
    fixed = not DC.ALL[case]["ill"]
    assert all(tol[k] == DC.bar(case, k) for k in tol) or not fixed
    bad = [f"(a) {k}: {v:.2e}" for k, v in resp.items() if fixed and not v <= DC.bar(case, k) / 100]
    bad += [f"(b) {k}: {v:.2e}" for k, v in gap.items() if fixed and not v <= DC.bar(case, k) / 10]
    bad += [f"(c) restatement outside the GPU bound, {k}: {v:.2e} > {tol[k]:.1e}" for k, v in gap.items() if not v <= tol[k]]
    assert not bad, case + "\n" + "\n".join(bad)
