"""The two kernels of the bias analysis (bias.hip) through the C ABI, with the conventions and the bounds of
tests/test_gpu_glue_kernels.py: every output is NaN before the call and carries guard elements behind it; a copy or a single IEEE
operation is bit-equal; a sum of n terms is within 2^-52 (n + 8) sum |term| of the longdouble sum.  Nothing here is measured.

Shapes (L, m): one element, odd sizes, one short of / exactly / one past a 256-thread workgroup, more than one workgroup, the
shapes of the step tests, and the largest m the library takes."""
import numpy as np
import pytest
import torch

from tests.test_gpu_glue_kernels import EPS, F64, LD, Buf, _call, assert_within, dev, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (16, 32), (1, 255), (1, 256), (2, 257), (24, 64), (5, 100), (1, 2048)]
INVALID, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("L,m", SHAPES)
def test_accumulate_is_the_left_to_right_sum(L, m):
    """After k = 1, 2 and 7 calls acc[:L m] equals x_1 + x_2 + ... + x_k added in that order in float64, to the bit, and
    acc[L m] equals k."""
    g = torch.Generator().manual_seed(L * 10000 + m)
    n = L * m
    acc = Buf(data=torch.zeros(n + 1, dtype=F64))
    want = np.zeros(n)
    for k in range(1, 8):
        x = rnd(g, L, m) * (10.0 ** ((k % 3) - 1))                 # magnitudes differ from step to step: the order matters
        _call("svgp_mean_vectors_accumulate", L, m, dev(x).data_ptr(), acc.ptr)
        want = want + x.numpy().reshape(-1)
        if k in (1, 2, 7):
            got = acc.get().numpy()
            assert np.array_equal(got[:n], want), (L, m, k)
            assert got[n] == float(k), (L, m, k)


def _bias_inputs(L, m, B, seed):
    g = torch.Generator().manual_seed(seed)
    mean = rnd(g, L, m) * 2
    acc = torch.cat([((mean + 0.3 * rnd(g, L, m)) * B).reshape(-1), torch.tensor([float(B)], dtype=F64)])
    full = mean + 0.01 * rnd(g, L, m)
    return acc, full


@pytest.mark.parametrize("L,m", SHAPES)
def test_bias_sums(L, m):
    """out[1 + l] = sum_j |acc[l, j] / B - full[l, j]|: the terms are one division, one subtraction and one sign flip each, so the
    device forms the float64 terms numpy forms, and their sum over j is a sum of m terms.  out[0] = (sum_l out[1 + l]) / L: a sum of
    L terms, the channel sums as the device stored them, then one division.  Two calls give the same bits."""
    for B in (1, 7, 3):
        acc, full = _bias_inputs(L, m, B, L * 10000 + m + B)
        outs = []
        for _ in range(2):
            out = Buf(1 + L)
            _call("svgp_mean_vectors_bias", L, m, dev(acc).data_ptr(), dev(full).data_ptr(), out.ptr)
            outs.append(out.get().numpy())
        got = outs[0]
        assert np.array_equal(outs[0], outs[1]), "not deterministic"
        terms = np.abs(acc[:-1].numpy().reshape(L, m) / float(B) - full.numpy()).astype(LD)
        assert_within(got[1:], terms.sum(1), EPS[F64] * (m + 8) * terms.sum(1), f"bias channels L {L} m {m} B {B}")
        ch = got[1:].astype(LD)
        assert_within(got[:1], ch.sum(keepdims=True) / L, EPS[F64] * (L + 8) * np.abs(ch).sum() / L, f"bias mean L {L} m {m} B {B}")


def test_bias_with_no_step_is_nan_not_an_error():
    """B = 0 on a zeroed accumulator (the state right after mean_vectors_begin): 0 / 0 - full is NaN in every term."""
    for L, m in ((1, 1), (3, 5), (2, 257)):
        _, full = _bias_inputs(L, m, 1, 5)
        out = Buf(1 + L)
        _call("svgp_mean_vectors_bias", L, m, dev(torch.zeros(L * m + 1, dtype=F64)).data_ptr(), dev(full).data_ptr(), out.ptr)
        assert torch.isnan(out.get()).all(), (L, m)


def test_refusals_come_before_any_launch():
    """L = 0, m = 0, a NULL pointer: SVGP_ERR_INVALID; m = 2049: SVGP_ERR_UNSUPPORTED.  The outputs stay NaN (a launch with one of
    the NULL pointers would fault)."""
    from svgp_vae_amd._lib import load_library
    lib = load_library()
    s = torch.cuda.current_stream().cuda_stream
    L, m = 3, 5
    x = torch.ones(L * 2049, dtype=F64).cuda()
    acc, out = Buf(L * 2049 + 1), Buf(1 + L)
    for (l_, m_), code in (((0, m), INVALID), ((L, 0), INVALID), ((-1, m), INVALID), ((L, -4), INVALID), ((L, 2049), UNSUPPORTED)):
        assert lib.svgp_mean_vectors_accumulate(l_, m_, x.data_ptr(), acc.ptr, s) == code, (l_, m_)
        assert lib.svgp_mean_vectors_bias(l_, m_, x.data_ptr(), x.data_ptr(), out.ptr, s) == code, (l_, m_)
    assert lib.svgp_mean_vectors_accumulate(L, m, None, acc.ptr, s) == INVALID
    assert lib.svgp_mean_vectors_accumulate(L, m, x.data_ptr(), None, s) == INVALID
    for args in ((None, x.data_ptr(), out.ptr), (x.data_ptr(), None, out.ptr), (x.data_ptr(), x.data_ptr(), None)):
        assert lib.svgp_mean_vectors_bias(L, m, *args, s) == INVALID
    assert b"NULL" in lib.svgp_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(acc.get()).all() and torch.isnan(out.get()).all()
