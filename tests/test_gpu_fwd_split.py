"""The m <= 32 forward block with only Si, t, u ahead of the decoder (schedule switch SVGP_FWD_SPLIT): the head form of the forward
factor stage, the z form of the forward row stage, the decoder launch whose riders finish the factor stage, and pass 1 of the
reverse row stage in its d form.  What moved is the code of the full forms (csrc/gp_kernels.hip: factor_fwd_tail, row_quad_term,
row_d, row_l3), run with the same thread layout and summation order, so every comparison here is exact."""
import ctypes as C

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

# (7, 12, 3): one padded 16-tile, one row block; (48, 16, 4): exact tile; (300, 24, 5): two padded tiles, workgroups walk two images;
# (10, 17, 57): mp = 32 with 15 pad columns, L above the 56-channel limit of the merged statistics; (256, 32, 16): config 2
SHAPES = [(7, 12, 3), (48, 16, 4), (300, 24, 5), (10, 17, 57), (256, 32, 16)]
NAN = float("nan")


def _engine(b, m, L, seed=31, kl_form=0, eps=True):
    params, images, aux, ep = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=seed)
    eng = H.engine_for(params, b, geco=True, N_train=400.0)
    if kl_form:
        eng.base["kl_form"] = 1
        eng.set_batch_size(b)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), ep.to(dev) if eps else None)
    return eng


@pytest.mark.parametrize("b,m,L,kl_form", [s + (0,) for s in SHAPES] + [(48, 16, 4, 1)])
def test_the_four_forms_equal_the_full_forms_stage_by_stage(b, m, L, kl_form):
    from svgp_vae_amd import _lib
    eng = _engine(b, m, L, kl_form=kl_form)
    eng.run(adam=False)
    eng.synchronize()
    cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
    img, ep, s = eng._bound[0].data_ptr(), eng._bound[2].data_ptr(), eng.stream.cuda_stream
    n_part, nb = int(eng.wl.n_part), (b + (256 // m) - 1) // (256 // m)
    mats, vecs, rows = (L, m, m), (L, m), (b, L)
    shapes = dict(Si=mats, t=vecs, mu_hat=vecs, u=vecs, G=mats, A=mats, M2=mats, Aji=mats, KL=(2 * L,), q=(b,),
                  p_m=rows, p_v=rows, e=rows, d=rows, eps=rows, z=rows, zbar=rows,
                  dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784), dec_d2=(b, 1568), dec_d1=(b, 512),
                  dec_dh0=(b, 128), ybar=rows, s2bar=rows, Knbar_part=(L, b, m))
    view = lambda k: eng.ws_view(k, shapes[k])
    part = lambda: eng.ws_view("part_sums", (n_part * 4 + L * nb * 2,))
    row_part = lambda: part()[n_part * 4:].view(L * nb, 2)
    sq = lambda: part()[:n_part * 4].view(n_part, 4)[:, 2]

    # (the library's launches run on the engine's stream, torch's fills and copies on torch's own: each side waits for the other)
    def snapshot():
        eng.synchronize()
        out = {k: view(k).clone() for k in shapes}
        if not kl_form:
            out["KL"] = out["KL"][:L]
        out["row_partials"], out["sqerr_partials"] = row_part().clone(), sq().clone()
        torch.cuda.synchronize(eng.device)
        return out

    def blank():
        for k in shapes:
            view(k).fill_(NAN)
        row_part().fill_(NAN)
        sq().fill_(NAN)
        torch.cuda.synchronize(eng.device)

    def reverse_in_between():           # what the step runs between the decoder launch and pass 1 of the reverse row stage
        _lib.call("svgp_gp_stats_bwd", cfg, ws, st, s)
        _lib.call("svgp_gp_factor_bwd_nofinal_wgrad", cfg, img, ws, st, s)

    blank()
    _lib.call("svgp_gp_factor_fwd_defer_aji", cfg, ws, s)
    _lib.call("svgp_gp_posterior_fwd", cfg, ep, ws, st, s)
    _lib.call("svgp_mnist_decoder_fwd_bwd_data_pre_aji", cfg, th, img, ws, st, s)
    reverse_in_between()
    _lib.call("svgp_gp_posterior_bwd_rows", cfg, ws, st, s)
    old = snapshot()
    for k, v in old.items():
        assert torch.isfinite(v).all(), k

    blank()
    _lib.call("svgp_gp_factor_fwd_head", cfg, ws, s)
    _lib.call("svgp_gp_posterior_fwd_z", cfg, ep, ws, st, s)
    mid = snapshot()
    # nothing on the chain up to the decoder launch reads (or has written) what moved ...
    for k in ("G", "A", "M2", "Aji", "d"):
        assert torch.isnan(mid[k]).all(), k
    assert torch.isnan(mid["KL"]).all() and torch.isnan(mid["row_partials"][:, 0]).all()
    # ... and what the decoder and the reverse statistics read is there already
    for k in ("Si", "t", "mu_hat", "u", "q", "z", "e", "p_m", "p_v", "eps"):
        assert torch.equal(mid[k], old[k]), k
    assert torch.equal(mid["row_partials"][:, 1], old["row_partials"][:, 1])
    _lib.call("svgp_mnist_decoder_fwd_bwd_data_pre_tail", cfg, th, img, ws, st, s)
    reverse_in_between()
    _lib.call("svgp_gp_posterior_bwd_rows_d", cfg, ws, st, s)
    new = snapshot()
    for k, v in old.items():
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(new[k], v), k


def _three_steps(b, m, L, flag, monkeypatch, graph=False, eps=True, dp=False):
    monkeypatch.setenv("SVGP_FWD_SPLIT", flag)
    eng = _engine(b, m, L, seed=32, eps=eps)
    if dp:
        from svgp_vae_amd.engine import RcclComm
        eng.attach_comm(RcclComm(0, 1, RcclComm.unique_id()))
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
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, y[2][k]), k
    assert x[3] == y[3]


@pytest.mark.parametrize("b,m,L", [(256, 32, 16), (300, 24, 5)])
def test_step_with_and_without_the_split_forward_block_is_bit_equal(b, m, L, monkeypatch):
    off = _three_steps(b, m, L, "0", monkeypatch)
    _assert_same_step(off, _three_steps(b, m, L, "1", monkeypatch))
    if (b, m, L) == (256, 32, 16):
        _assert_same_step(off, _three_steps(b, m, L, "1", monkeypatch, graph=True))


def test_step_with_device_drawn_eps_is_bit_equal(monkeypatch):
    off = _three_steps(300, 24, 5, "0", monkeypatch, eps=False)
    _assert_same_step(off, _three_steps(300, 24, 5, "1", monkeypatch, eps=False))


def test_data_parallel_step_on_one_rank_is_bit_equal(monkeypatch):
    off = _three_steps(256, 32, 16, "0", monkeypatch, dp=True)
    _assert_same_step(off, _three_steps(256, 32, 16, "1", monkeypatch, dp=True))


def test_the_new_kernels_keep_their_resources():
    """The rider instantiation of k_decoder_fwd_bwd_data is held to the bounds of the other two (tests/test_gpu_decoder_fused.py): <= 168
    registers per lane, no scratch, <= 80 KB of LDS at L = 16, or a rider and an image workgroup no longer share a CU.  The head, z
    and d kernels must not spill."""
    from svgp_vae_amd import _lib
    n = (C.c_int * 3)()
    _lib.call("svgp_mnist_decoder_fused_tail_regs", 16, n)
    regs, scratch, lds = tuple(n)
    assert 0 < regs <= 168, list(n)
    assert scratch == 0, list(n)
    assert 0 < lds <= 81920, list(n)
    k = (C.c_int * 12)()
    _lib.call("svgp_fwd_split_regs", k)
    for i in range(6):
        assert k[2 * i] > 0 and k[2 * i + 1] == 0, list(k)
