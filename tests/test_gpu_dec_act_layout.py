"""The fused decoder launches keep d2, d1 and a2 at a padded pixel stride in LDS, d1 inside the d3 block and dh0 on h0
(svgp_mnist_decoder_fused_lds_array; tests/test_dec_act_layout_cpu.py has the map itself); the unfused pair
svgp_mnist_decoder_fwd_pre + svgp_mnist_decoder_bwd_data_pre keeps every array packed and in a block of its own.  Same expressions in
the same order on either map, and the global copies stay packed, so the two are compared through everything they write, exactly.

(513, 32, 16): the grid has 256 image workgroups, so the first walks three images and reuses the aliased blocks twice;
(257, 48, 4): m > 32 -- only the form without riders runs -- with a small latent size, so another place of every array in the block;
(3, 16, 8): fewer images than a wave has lanes."""
import ctypes as C

import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

SHAPES = [(513, 32, 16), (257, 48, 4), (3, 16, 8)]
FORMS = {"svgp_mnist_decoder_fwd_bwd_data_pre": None, "svgp_mnist_decoder_fwd_bwd_data_pre_aji": "svgp_gp_factor_fwd_defer_aji",
         "svgp_mnist_decoder_fwd_bwd_data_pre_tail": "svgp_gp_factor_fwd_head"}       # launch -> what makes its riders' inputs


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "b%d_m%d_L%d" % s)
def case(request):
    """the engine after one pass (z and ws.dec_weff valid) and the outputs of the unfused pair, computed once per shape"""
    b, m, L = request.param
    params, images, aux, eps = H.toy_problem(b=b, m=m, L=L, M=4, n_obj=20, seed=47)
    eng = H.engine_for(params, b, geco=True, N_train=400.0)
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), eps.to(dev))
    eng.run(adam=False)
    eng.synchronize()
    n_part = int(eng.wl.n_part)
    shapes = dict(dec_h0=(b, 128), dec_a1=(b, 512), dec_a2=(b, 1568), recon=(b, 784), dec_d2=(b, 1568), dec_d1=(b, 512),
                  dec_dh0=(b, 128), zbar=(b, L))
    views = {k: eng.ws_view(k, sh) for k, sh in shapes.items()}
    views["sqerr_partials"] = eng.ws_view("part_sums", (n_part, 4))[:, 2]

    def run(*launches):
        from svgp_vae_amd import _lib
        cfg, th, ws, st = C.byref(eng.cfg), eng.theta.data_ptr(), eng.ws.data_ptr(), eng.state.data_ptr()
        img, s = eng._bound[0].data_ptr(), eng.stream.cuda_stream
        for v in views.values():
            v.fill_(float("nan"))
        for name in launches:
            if name.startswith("svgp_gp_factor_fwd"):
                _lib.call(name, cfg, ws, s)
            elif name == "svgp_mnist_decoder_fwd_pre":
                _lib.call(name, cfg, th, img, ws, s)
            else:
                _lib.call(name, cfg, th, img, ws, st, s)
        eng.synchronize()
        return {k: v.clone() for k, v in views.items()}

    want = run("svgp_mnist_decoder_fwd_pre", "svgp_mnist_decoder_bwd_data_pre")
    for k, v in want.items():
        assert torch.isfinite(v).all(), k
    return m, run, want


@pytest.mark.parametrize("form", sorted(FORMS))
def test_padded_activations_give_the_bits_of_the_packed_ones(case, form):
    m, run, want = case
    if m > 32 and FORMS[form]:
        # the rider forms refuse m > 32 before anything is launched (SVGP_ERR_UNSUPPORTED): there is no such launch to compare
        from svgp_vae_amd import _lib
        with pytest.raises(_lib.SvgpError, match="48"):            # the message names the offending m
            run(form)
        return
    got = run(*([FORMS[form]] if FORMS[form] else []), form)
    for k, v in want.items():
        assert torch.equal(got[k], v), k
