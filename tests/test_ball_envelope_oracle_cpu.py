"""Guard for tests/test_gpu_ball_envelope.py: at every case of its tables the oracle itself must be well conditioned.

The GPU tests hold the HIP engines to fixed float64 tolerances (tests/ball_cases.py).  Those mean something only where two
backward-stable evaluations of the same formulas agree far more closely than that, so each case's oracle is evaluated twice, the
second time with every parameter multiplied by 1 + 2^-52, and its own response -- relative to the tensor's max-abs, as the GPU
tests measure -- must stay within 1/100 of the tolerance applied.  A case that fails here gets another length scale or tmax,
never a wider tolerance.  (Measured when the tables were written: outputs up to 4.5e-14, gradients up to 4.5e-11, the latter
on the Titsias cases.)
"""
import pytest
import torch

from tests import ball_cases as BC
from tests import helpers as H

ONE_ULP = 1.0 + 2.0 ** -52


def _response(out, grads, out2, grads2):
    outs = [(o, o2) for o, o2 in zip(out, out2) if torch.is_tensor(o)]
    e_out = max(H.relerr(o2, o) for o, o2 in outs)
    e_elbo = abs(float(out2[0].mean()) - float(out[0].mean())) / abs(float(out[0].mean()))
    e_grad = max(H.relerr(grads2[k], grads[k]) for k in grads)
    return e_out, e_elbo, e_grad


def _check(case, resp):
    e_out, e_elbo, e_grad = resp
    print(f"{case}: oracle response outputs {e_out:.2e}, mean elbo {e_elbo:.2e}, gradients {e_grad:.2e}")
    assert e_out <= BC.OUT_TOL / 100, (case, e_out)
    assert e_elbo <= BC.ELBO_TOL / 100, (case, e_elbo)
    assert e_grad <= BC.GRAD_TOL / 100, (case, e_grad)


@pytest.mark.parametrize("case", list(BC.SPARSE_CASES))
def test_sparse_case_oracle_response_is_far_below_the_tolerances(case):
    p, vid, eps, out, grads = BC.sparse_reference(case)
    out2, _, grads2 = BC.sparse_oracle(BC.SPARSE_CASES[case], {k: v * ONE_ULP for k, v in p.items()}, vid, eps)
    _check(case, _response(out, grads, out2, grads2))


@pytest.mark.parametrize("case", list(BC.PEARCE_ENV_CASES))
def test_pearce_case_oracle_response_is_far_below_the_tolerances(case):
    p, vid, eps, ran_ind, out, grads = BC.pearce_reference(case)
    out2, _, grads2 = BC.pearce_oracle(BC.PEARCE_ENV_CASES[case], {k: v * ONE_ULP for k, v in p.items()}, vid, eps, ran_ind)
    _check(case, _response(out, grads, out2, grads2))
