"""The generation kernels decode exactly as the training decoder does: k_generate, k_casale_generate and k_decoder_fwd run the one
decoder forward piece of csrc/vae_dev.hpp (the generation kernels with the rolled up-convolutions, the same FMA order), so the
images of a generate call are, bit for bit, svgp_mnist_decoder_fwd of the latent rows the call returns.  With eps = NULL the
returned first moment (p_m, Casale: mean) IS the latent row.  Cases and caches: tests/test_gpu_generate.py,
tests/test_gpu_casale_generate.py."""
import ctypes as C

import pytest
import torch

from tests import casale_generate_cases as CG
from tests import generate_cases as GC
from tests import test_gpu_casale_generate as TC
from tests import test_gpu_generate as TG

pytestmark = pytest.mark.gpu
DT = torch.float64
ROWS = 300          # more rows than workgroups in the grid (256): a workgroup walks two images
_ENGINES = {}


def training_decoder(params, L, z):
    """svgp_mnist_decoder_fwd at the decoder parameters of `params` on the latent rows z (b, L): recon (b, 28, 28, 1)."""
    from svgp_vae_amd import _lib
    from svgp_vae_amd.engine import MnistStepEngine
    if L not in _ENGINES:
        _ENGINES[L] = MnistStepEngine(4, L, 1, 0, b_max=ROWS)
    eng, b = _ENGINES[L], z.shape[0]
    eng.load_params({k: v for k, v in params.items() if k.startswith("dec_")})
    eng.set_batch_size(b, b)
    eng.ws_view("z", (b, L)).copy_(z)
    images = torch.zeros(b, 28, 28, 1, dtype=DT, device=eng.device)
    torch.cuda.synchronize()
    _lib.call("svgp_mnist_decoder_fwd", C.byref(eng.cfg), eng.theta.data_ptr(), images.data_ptr(), eng.ws.data_ptr(),
              eng.stream.cuda_stream)
    eng.synchronize()
    return eng.ws_view("recon", (b, 28, 28, 1)).cpu()


def query_rows(qaux, n):
    """n query rows: the case's own, or copies of them with an angle of their own each."""
    if n == qaux.shape[0]:
        return qaux
    aux = qaux[torch.arange(n) % qaux.shape[0]].clone()
    aux[:, 1] += torch.arange(n, dtype=DT) * 0.01
    return aux


@pytest.mark.parametrize("rows", ["q", ROWS])
@pytest.mark.parametrize("case", ["A", "C", "D", "E", "F", "G"])
def test_mnist_generate_decodes_as_the_training_decoder(case, rows):
    cs = GC.CASES[case]
    params, _, _, qaux, _ = GC.problem(case)
    aux = query_rows(qaux, cs["q"] if rows == "q" else rows)
    images, p_m, _ = TG.raw_generate(TG.cache_of(case), aux, None, cs["table"])
    assert bool(torch.isfinite(images).all()) and float(images.abs().max()) > 0
    recon = training_decoder(params, cs["L"], p_m)
    assert torch.equal(images, recon), (case, int((images != recon).sum()), float((images - recon).abs().max()))


@pytest.mark.parametrize("rows", ["q", ROWS])
@pytest.mark.parametrize("variant", ["L1", "L64", "C-norm", "H258-raw"])
def test_casale_generate_decodes_as_the_training_decoder(variant, rows):
    pr = CG.problem(variant)
    aux = query_rows(pr["qaux"], CG.N_QUERY if rows == "q" else rows)
    images, mean, _ = TC.raw_generate(TC.cache_of(variant), aux, None, 1)
    assert bool(torch.isfinite(images).all()) and float(images.abs().max()) > 0
    recon = training_decoder(pr["p"], pr["L"], mean)
    assert torch.equal(images, recon), (variant, int((images != recon).sum()), float((images - recon).abs().max()))
