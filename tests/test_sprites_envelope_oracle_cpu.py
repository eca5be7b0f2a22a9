"""Guard for tests/test_gpu_sprites_envelope.py: at every case of its tables the oracle itself must be well conditioned.

The GPU tests hold the SPRITES step to fixed float64 tolerances (tests/sprites_cases.py: FWD_TOL on the 16-tuple, GRAD_TOL on
the gradients).  Those mean something only where two backward-stable evaluations of the same formulas agree far more closely than
that, so each case's oracle is evaluated twice, the second time with every real input (parameters, images, eps) multiplied by
1 + 2^-52, and its own response -- relative to the tensor's max-abs, as the GPU tests measure -- must stay within 1/100 of the
tolerance applied.  The batches of the below-capacity test are cases of their own here.  A case that fails gets another seed or
another shape of the same form, never a wider tolerance.  (Measured when the table was written: NOTEBOOK.md, "SPRITES envelope".)
"""
import pytest

from tests import sprites_cases as SC

SUB_BATCHES = [(case, rows) for case, batches in SC.CAPACITY_BATCHES.items() for rows in sorted(set(batches))
               if rows != SC.CASES[case]["b"]]


def _check(label, resp):
    e_fwd, e_grad = resp
    print(f"{label}: oracle response 16-tuple {e_fwd:.2e}, gradients {e_grad:.2e}")
    assert e_fwd <= SC.FWD_TOL / 100, (label, e_fwd)
    assert e_grad <= SC.GRAD_TOL / 100, (label, e_grad)


@pytest.mark.parametrize("case", list(SC.CASES))
def test_case_oracle_response_is_far_below_the_tolerances(case):
    _check(case, SC.oracle_response(case))


@pytest.mark.parametrize("case,rows", SUB_BATCHES)
def test_sub_batch_oracle_response_is_far_below_the_tolerances(case, rows):
    _check(f"{case} rows {rows}", SC.oracle_response(case, rows))
