"""Guard for tests/test_gpu_titsias_envelope.py: at every case of its table, and at every batch of its below-capacity test, the
references themselves must be far more exact than the bars the GPU step is held to (tests/titsias_cases.py).

(a) The literal oracle (b x b covariance per channel) evaluated twice, the second time with its real inputs perturbed by one ulp,
    must change by at most bar / 100 per quantity, in the measure of that quantity's bar.
(b) The m x m restatement of oracle/staged_gp.py -- the formulation the HIP path implements -- must differ from the literal
    oracle by at most bar / 10: two correct float64 evaluations of the two formulations.
Exactly one case, m520, is marked ill-conditioned (toy inducing points at m >= 512: gradient response 5e-7) and is held to
max(bar, 20 x its own one-ulp response) per quantity on the GPU; the 1- and 3-row batches of the capacity test (32 inducing points
against 1 or 3 rows: gradient response 1e-6) take that rule too, as in the Hensman suite.  Neither (a) nor (b) can hold for those
three; what the guard shows for them instead is that the restatement, a correct float64 evaluation, sits inside the bound the GPU
step is given.  Every other case and batch passes (a) and (b).  A case that fails gets another seed, M or objective, never a wider
bar.  (Measured when the table was written: NOTEBOOK.md, "Titsias envelope".)"""
import pytest

from tests import titsias_cases as TC

SUB_BATCHES = [rows for rows in sorted(set(TC.CAPACITY_BATCHES)) if rows != TC.CASES[TC.CAPACITY_CASE]["b"]]


def _check(case, rows=None):
    label = case if rows is None else f"{case} rows {rows}"
    resp, gap, tol = TC.oracle_response(case, rows), TC.restatement_gap(case, rows), TC.tolerances(case, rows)
    wr, wg = TC.worst(resp), TC.worst(gap)
    print(f"{label}: one-ulp response scalars {wr['scalar']:.1e} fields {wr['field']:.1e} gradients {wr['grad']:.1e}; "
          f"restatement gap scalars {wg['scalar']:.1e} fields {wg['field']:.1e} gradients {wg['grad']:.1e}")
    fixed = not TC.CASES[case]["ill"] and rows not in TC.SELF_CONSISTENCY_ROWS
    assert all(tol[k] == TC.bar(k) for k in tol) or not fixed
    bad = [f"(a) {k}: {v:.2e}" for k, v in resp.items() if fixed and not v <= TC.bar(k) / 100]
    bad += [f"(b) {k}: {v:.2e}" for k, v in gap.items() if fixed and not v <= TC.bar(k) / 10]
    bad += [f"restatement outside the GPU bound, {k}: {v:.2e} > {tol[k]:.1e}" for k, v in gap.items() if not v <= tol[k]]
    assert not bad, label + "\n" + "\n".join(bad)


def test_exactly_one_case_is_marked_ill_conditioned():
    assert [c for c, cs in TC.CASES.items() if cs["ill"]] == ["m520"]
    assert set(TC.STAGE_CASES) | set(TC.GRAPH_CASES) <= set(TC.ENVELOPE_CASES)
    for flag, value in (("geco", True), ("geco", False), ("normalize", True), ("with_table", False), ("clip_qs", False)):
        assert sum(TC.CASES[c][flag] == value for c in TC.ENVELOPE_CASES) >= 2, flag


@pytest.mark.parametrize("case", list(TC.CASES))
def test_case_references_are_far_more_exact_than_the_bars(case):
    _check(case)


@pytest.mark.parametrize("rows", SUB_BATCHES)
def test_sub_batch_references_are_far_more_exact_than_the_bars(rows):
    _check(TC.CAPACITY_CASE, rows)
