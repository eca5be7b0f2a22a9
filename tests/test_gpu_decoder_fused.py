"""The decoder's forward launch and its data-reverse launch as ONE launch (svgp_mnist_decoder_fwd_bwd_data_pre[_aji], the
SVGP_DEC_FUSE schedule switch): one image loop keeps a1, a2, the reconstruction and the weights in LDS and the image pixels in
registers between the two halves.  The arithmetic and its order are those of svgp_mnist_decoder_fwd_pre followed by
svgp_mnist_decoder_bwd_data_pre[_aji] (the forward's tap loops are rolled, not reordered), so every comparison here is exact."""
import ctypes as C

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

# (300, 24, 5): b above the 256 partial slots -- workgroups walk two images (prefetch registers, LDS reuse);
# (20, 40, 3): 32 < m <= 64 -- the form without riders
SHAPES = [(7, 12, 3), (48, 16, 4), (300, 24, 5), (20, 40, 3), (256, 32, 16)]


def _engine(b, m, L, seed=21):
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=seed)
    eng = H.engine_for(params, b, geco=True, N_train=400.0)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    return eng


@pytest.mark.parametrize("b,m,L", SHAPES)
def test_fused_launch_equals_the_two_launches(b, m, L):
    from svgp_vae_amd import _lib
    eng = _engine(b, m, L)
    eng.run(adam=False)
    eng.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, ep, s = eng._bound[0].data_ptr(), eng._bound[2].data_ptr(), eng.stream.cuda_stream
    riders = m <= 32
    n_part = int(eng.wl.n_part)
    shapes = dict(dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784), dec_d2=(b, 1568), dec_d1=(b, 512),
                  dec_dh0=(b, 128), zbar=(b, L), Aji=(L, m, m), KL=(2 * L,), z=(b, L))
    sq = lambda: eng.ws_view("part_sums", (n_part, 4))[:, 2]
    out = {}
    for form in ("two", "one"):
        for k, sh in shapes.items():
            if k not in ("KL", "z"):
                eng.ws_view(k, sh).fill_(float("nan"))
        sq().fill_(float("nan"))
        _lib.call("svgp_gp_factor_fwd_defer_aji", cfg, ws, s)                 # re-opens A_hat / the KL terms for the riders
        _lib.call("svgp_gp_posterior_fwd" if riders else "svgp_gp_posterior_fwd_with_aji", cfg, ep, ws, st, s)
        sfx = "_aji" if riders else ""
        if form == "two":
            _lib.call("svgp_mnist_decoder_fwd_pre", cfg, th, img, ws, s)
            _lib.call("svgp_mnist_decoder_bwd_data_pre" + sfx, cfg, th, img, ws, st, s)
        else:
            _lib.call("svgp_mnist_decoder_fwd_bwd_data_pre" + sfx, cfg, th, img, ws, st, s)
        eng.synchronize()
        out[form] = {k: eng.ws_view(k, sh).clone() for k, sh in shapes.items()}
        out[form]["sqerr_partials"] = sq().clone()
    for k in out["two"]:
        assert torch.isfinite(out["one"][k]).all(), k
        assert torch.equal(out["one"][k], out["two"][k]), k


def _three_steps(b, m, L, flag, monkeypatch, graph=False):
    monkeypatch.setenv("SVGP_DEC_FUSE", flag)
    eng = _engine(b, m, L, seed=22)
    if graph:
        eng.capture("step", adam=True)          # capture does not execute
    for _ in range(3):
        if graph:
            eng.replay("step")
        else:
            eng.run(adam=True)
    eng.synchronize()
    return eng.theta.clone(), eng.state.clone(), {k: v.clone() for k, v in eng.grads().items()}, eng.scalars()


def _assert_same_step(x, y):
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    for k, v in x[2].items():
        assert torch.equal(v, y[2][k]), k
    assert x[3] == y[3]


@pytest.mark.parametrize("b,m,L", [(256, 32, 16), (300, 24, 5)])
def test_step_with_and_without_the_fused_decoder_launch_is_bit_equal(b, m, L, monkeypatch):
    off = _three_steps(b, m, L, "0", monkeypatch)
    _assert_same_step(off, _three_steps(b, m, L, "1", monkeypatch))
    if (b, m, L) == (256, 32, 16):
        _assert_same_step(off, _three_steps(b, m, L, "1", monkeypatch, graph=True))


def test_fused_kernel_keeps_two_workgroups_per_cu():
    """No occupancy hint on k_decoder_fwd_bwd_data: both instantiations must stay at <= 168 registers per lane without scratch, and
    an image workgroup at L = 16 within 80 KB of LDS, or a rider and an image workgroup no longer share a CU."""
    from svgp_vae_amd import _lib
    n = (C.c_int * 6)()
    _lib.call("svgp_mnist_decoder_fused_regs", 16, n)
    for regs, scratch, lds in (tuple(n[0:3]), tuple(n[3:6])):
        assert 0 < regs <= 168, list(n)
        assert scratch == 0, list(n)
        assert 0 < lds <= 81920, list(n)
