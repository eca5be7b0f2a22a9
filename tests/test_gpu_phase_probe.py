"""The phase-timeline instances of the fused decoder launch and of the reverse factor launch with its riders
(svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe, svgp_gp_stats_factor_bwd_wgrad_probe; tools/decoder_phase_probe.py prints them):
a probe launch leaves exactly what the product launch leaves, and every workgroup's row of stamps is complete and non-decreasing.
Shape (70, 32, 3): the m = 32 instances the probes exist for, 70 image workgroups and 3 x 70 riders, three channels."""
import ctypes as C

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEC_SLOTS, FB_SLOTS = 16, 8
NAN = float("nan")


def test_probe_launches_equal_the_product_launches_and_stamps_are_monotone():
    from svgp_vae_amd import _lib
    b, m, L = 70, 32, 3
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=5)
    eng = H.engine_for(params, b, geco=True, N_train=400.0)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    state0 = eng.state.clone()
    eng.run(adam=False)
    eng.synchronize()
    eng.state.copy_(state0)
    torch.cuda.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, ep, s = eng._bound[0].data_ptr(), eng._bound[2].data_ptr(), eng.stream.cuda_stream
    n_part, n_dec = int(eng.wl.n_part), int(eng.pl.n_vae - eng.pl.n_enc)
    P = eng.wl.statB_len // (L * (m * m + 2 * m))
    mats, rows = (L, m, m), (b, L)
    dec_out = dict(G=mats, A=mats, M2=mats, Aji=mats, KL=(L,), dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784),
                   dec_d2=(b, 1568), dec_d1=(b, 512), dec_dh0=(b, 128), zbar=rows)
    fb_out = dict(fb_part=(2, L, m, m), vbar=(L, m), Ssym=mats, Qm=mats, part_dec=(n_part, n_dec))
    sq = lambda: eng.ws_view("part_sums", (n_part, 4))[:, 2]

    def run(outs, with_sq, *calls):
        for k, sh in outs.items():
            eng.ws_view(k, sh).fill_(NAN)
        if with_sq:
            sq().fill_(NAN)
        torch.cuda.synchronize()
        for sym, args in calls:
            _lib.call(sym, *args)
        eng.synchronize()
        got = {k: eng.ws_view(k, sh).clone() for k, sh in outs.items()}
        if with_sq:
            got["sq"] = sq().clone()
        for k, v in got.items():
            assert torch.isfinite(v).all(), k
        return got

    def stamps_of(n):
        return torch.zeros(n, dtype=torch.int64, device=dev)

    # the riders of the decoder launch run the tail of the forward factor stage: re-open it first (tests/test_gpu_fwd_split.py)
    reopen = (("svgp_gp_factor_fwd_head", (cfg, ws, s)), ("svgp_gp_posterior_fwd_z", (cfg, ep, ws, st, s)))
    want = run(dec_out, True, *reopen, ("svgp_mnist_decoder_fwd_bwd_data_pre_tail", (cfg, th, img, ws, st, s)))
    n_wg = L + b
    buf = stamps_of(n_wg * DEC_SLOTS + 5)
    got = run(dec_out, True, *reopen,
              ("svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe", (cfg, th, img, ws, st, buf.data_ptr(), buf.numel(), s)))
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert torch.count_nonzero(buf[n_wg * DEC_SLOTS:]) == 0
    r = buf[:n_wg * DEC_SLOTS].view(n_wg, DEC_SLOTS).cpu()
    role = (r[:, 15] >> 60) & 15
    assert (role[:L] == 2).all() and (role[L:] == 1).all(), role.tolist()
    t = r[L:, :15]
    assert (t > 0).all() and (t[:, 1:] >= t[:, :-1]).all(), t.tolist()
    assert (r[:L, 0] > 0).all() and (r[:L, 14] >= r[:L, 0]).all()
    assert int(t[:, 14].max() - r[:, 0].min()) < 100 * 1000        # one time axis: the whole launch within a millisecond (100 MHz)

    want = run(fb_out, False, ("svgp_gp_stats_factor_bwd_wgrad", (cfg, img, ws, st, s)))
    n_wg = P * L + L + 3 * b
    buf = stamps_of(n_wg * FB_SLOTS)
    got = run(fb_out, False, ("svgp_gp_stats_factor_bwd_wgrad_probe", (cfg, img, ws, st, buf.data_ptr(), buf.numel(), s)))
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    fl = eng.ws_view("flags", (64,)).view(torch.int64)
    assert torch.count_nonzero(fl) == 0, fl.tolist()
    r = buf.view(n_wg, FB_SLOTS).cpu()
    role, mask = (r[:, 7] >> 60) & 15, (r[:, 7] >> 56) & 15
    assert (role[:P * L] == 1).all() and (role[P * L:P * L + L] == 2).all() and (role[P * L + L:] == 3).all(), role.tolist()
    assert sorted(mask[P * L + L:].tolist()) == sorted([1] * b + [2] * b + [4] * b)
    assert (r[:, 0] > 0).all() and (r[:, 6] >= r[:, 0]).all()
    t = r[P * L + L:, :7]
    assert (t > 0).all() and (t[:, 1:] >= t[:, :-1]).all(), t.tolist()
    eng.scalars()                      # raises if a hand-off timed out

    # a buffer one element short is refused before anything is launched
    with pytest.raises(_lib.SvgpError):
        _lib.call("svgp_gp_stats_factor_bwd_wgrad_probe", cfg, img, ws, st, buf.data_ptr(), buf.numel() - 1, s)
    with pytest.raises(_lib.SvgpError):
        _lib.call("svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe", cfg, th, img, ws, st, buf.data_ptr(), (L + b) * DEC_SLOTS - 1, s)
