"""CPU checks of the VAE / CVAE feature: the restatement of tests/cvae_cases.py against the project's older VAE restatement and
against the reference-executed fixture, its sensitivity to summation order, and everything of csrc/cvae.hip and the driver
that needs no device: ABI sizes, layouts, refusals, routes, the LDS figure, the parser and the messages."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import casale_cases as KC
from tests import cvae_cases as CC
from tests import helpers as H

DT = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "ref_cvae_small.npz")))


@pytest.fixture(scope="module")
def lib():
    import svgp_vae_amd
    return svgp_vae_amd.load_library()


def _cfg(**kw):
    from svgp_vae_amd._lib import CvaeCfg
    d = dict(b=4, b_cap=8, L=16, cvae=1, clip_qs=0, store=0, sigma=0.01)
    d.update(kw)
    return CvaeCfg(**d)


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["b2_L16", "angles"])
def test_vae_restatement_equals_casale_elbo_vae(name):
    c = CC.make_case(name, False)
    out, g = CC.case_reference(c)
    p = {k: v.clone().requires_grad_(True) for k, v in c["params"].items()}
    obj, kout = KC.elbo_vae(p, c["images"], c["eps"], L=c["L"])
    kg = torch.autograd.grad(obj, [p[k] for k in p])
    for k in ("elbo", "recon_loss", "KL_term", "qnet_mu", "qnet_var", "recon"):
        assert H.relerr(out[k], kout[k].detach()) < 1e-12, k
    for k, v in zip(p, kg):
        assert H.relerr(g[k], v) < 1e-12, k


@pytest.mark.parametrize("tag,cvae,clip", [("cvae", True, False), ("cvae_clip", True, True), ("vae", False, False)])
def test_restatement_equals_reference_fixture(fx, tag, cvae, clip):
    names = [n for n, _ in CC.param_shapes(4, cvae)]
    params = {k: CC.t64(fx[f"{tag}.param.{k}"]) for k in names}
    out, g = CC.step_reference(params, CC.t64(fx["images"]), CC.t64(fx["aux"]), CC.t64(fx["eps"]), L=4, cvae=cvae, clip=clip)
    for k in ("recon_loss", "KL_term", "elbo"):
        want = float(fx[f"{tag}.fwd.{k}"])
        assert abs(float(out[k]) - want) <= CC.SCALAR_TOL * max(1.0, abs(want)), k
    for k in ("recon", "qnet_mu", "qnet_var", "z"):
        assert H.relerr(out[k], fx[f"{tag}.fwd.{k}"]) < CC.FWD_TOL, k
    for k in names:
        assert H.relerr(g[k], fx[f"{tag}.grad.{k}"]) < CC.GRAD_TOL, k
    if clip:
        v = fx["cvae.fwd.qnet_var"]                          # (the unclipped variances of the same problem)
        assert (v < 1e-3).any() and (v > 10).any()          # the fixture exercises both clip bounds


def test_predict_restatement_equals_reference_fixture(fx):
    params = {k: CC.t64(fx[f"cvae.param.{k}"]) for k, _ in CC.param_shapes(4, True)}
    rec, loss = CC.predict_reference(params, CC.t64(fx["images"]), CC.t64(fx["images_test"]), CC.t64(fx["aux"]), CC.t64(fx["aux_test"]),
                                     CC.t64(fx["eps_predict"]), L=4)
    want = fx["cvae.predict.recon"]
    assert np.isnan(want[2]).all() and torch.isnan(rec[2]).all()          # the empty-group row
    keep = [0, 1, 3]
    assert H.relerr(rec[keep], want[keep]) < CC.FWD_TOL
    assert torch.isnan(loss) and np.isnan(fx["cvae.predict.loss"])


@pytest.mark.parametrize("cvae", [False, True])
def test_restatement_in_reversed_row_order(cvae):
    """The batch rows in reverse order: the same sums in another order.  The scalars and gradients move by less than 1e-12, so the
    bars of the GPU tests are not spent on the order in which the reference happens to sum."""
    c = CC.make_case("b40_cap64", cvae)
    out, g = CC.case_reference(c)
    rev = lambda t: torch.flip(t, dims=[0])
    out2, g2 = CC.step_reference(c["params"], rev(c["images"]), rev(c["aux"]), rev(c["eps"]), L=c["L"], cvae=cvae)
    for k in ("elbo", "recon_loss", "KL_term"):
        assert abs(float(out[k]) - float(out2[k])) <= 1e-12 * abs(float(out[k])), k
    assert H.relerr(rev(out2["recon"]), out["recon"]) < 1e-12
    for k in g:
        assert H.relerr(g2[k], g[k]) < 1e-12, k


# ------------------------------------------------------------------------------------------------------------ the library, host side
def test_abi_sizes(lib):
    from svgp_vae_amd import _lib
    assert lib.svgp_struct_sizeof(19) == C.sizeof(_lib.CvaeCfg) == 32
    assert lib.svgp_struct_sizeof(20) == C.sizeof(_lib.CvaeWsLayout) == 12 * 8
    assert lib.svgp_struct_sizeof(12) == -1 and lib.svgp_struct_sizeof(17) == -1 and lib.svgp_struct_sizeof(21) == -1


@pytest.mark.parametrize("L", [1, 16, 64])
def test_layouts(lib, L):
    from svgp_vae_amd import _lib
    pv, pc, pm = _lib.ParamLayout(), _lib.ParamLayout(), _lib.ParamLayout()
    assert lib.svgp_cvae_param_layout_get(C.byref(_cfg(L=L, cvae=0)), C.byref(pv)) == 0
    assert lib.svgp_cvae_param_layout_get(C.byref(_cfg(L=L, cvae=1)), C.byref(pc)) == 0
    mc = _lib.MnistCfg(b=4, b_global=4, m=3, L=L, M=2, n_obj=0, N_train=10.0, jitter=1e-6, rep_weight=1.0)
    assert lib.svgp_mnist_param_layout_get(C.byref(mc), C.byref(pm)) == 0
    vae_fields = [f for f in _lib.PARAM_FIELDS if f.startswith(("enc_", "dec_"))] + ["n_enc", "n_vae"]
    for f in vae_fields:
        assert getattr(pv, f) == getattr(pm, f), f
    assert pv.n_total == pv.n_vae == pm.n_vae
    # mnistCVAE: the reference's creation order with its four wider variables
    off = 0
    for name, shp in CC.param_shapes(L, True):
        assert getattr(pc, name) == off, name
        off += int(np.prod(shp))
    assert pc.n_total == off and pc.n_enc == pc.dec_d_w
    if L == 16:
        assert pc.n_total == 6329 and pv.n_total == 5721
    # workspace: fields in order, 16-element boundaries, sized by b_cap and not by b
    w1, w2 = _lib.CvaeWsLayout(), _lib.CvaeWsLayout()
    assert lib.svgp_cvae_ws_layout_get(C.byref(_cfg(L=L, b=1, b_cap=40)), C.byref(w1)) == 0
    assert lib.svgp_cvae_ws_layout_get(C.byref(_cfg(L=L, b=40, b_cap=40)), C.byref(w2)) == 0
    offs = [getattr(w1, f) for f in _lib.CVAE_WS_FIELDS if f not in ("part_stride", "total")]
    assert offs == sorted(offs) and all(o % 16 == 0 for o in offs) and offs[0] == 0
    assert [getattr(w2, f) for f in _lib.CVAE_WS_FIELDS] == [getattr(w1, f) for f in _lib.CVAE_WS_FIELDS]
    assert w1.total >= w1.z + 40 * L and w1.recon + 40 * 784 <= w1.qnet_mu
    assert w1.part_stride == 2 * (576 + 8) + 27 * 8 + 8 + (90 * 8 + 8 + 576 + 8 + 72 + 1)


def test_refusals(lib):
    from svgp_vae_amd import _lib
    INVALID, UNSUPPORTED = -1, -2
    wl, pl = _lib.CvaeWsLayout(), _lib.ParamLayout()
    bad = [(dict(b=-1), INVALID), (dict(b=9, b_cap=8), INVALID), (dict(cvae=2), INVALID), (dict(cvae=-1), INVALID),
           (dict(store=2), INVALID), (dict(store=-1), INVALID), (dict(sigma=0.0), INVALID), (dict(sigma=-0.01), INVALID),
           (dict(sigma=float("nan")), INVALID), (dict(L=0), UNSUPPORTED), (dict(L=65), UNSUPPORTED)]
    buf = C.create_string_buffer(256)
    for kw, code in bad:
        cfg = _cfg(**kw)
        assert lib.svgp_cvae_ws_layout_get(C.byref(cfg), C.byref(wl)) == code, kw
        assert lib.svgp_cvae_param_layout_get(C.byref(cfg), C.byref(pl)) == code, kw
        assert lib.svgp_cvae_step_route(C.byref(cfg), buf, 256) == code, kw
        # the entry points refuse before they look at a pointer (these are not device pointers)
        assert lib.svgp_cvae_train_step(C.byref(cfg), 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, None) == code, kw
        assert lib.svgp_cvae_forward(C.byref(cfg), 8, 8, 8, 8, 8, 8, None) == code, kw
        assert lib.svgp_cvae_encode(C.byref(cfg), 8, 8, 8, 8, 8, None) == code, kw
        assert lib.svgp_cvae_decode(C.byref(cfg), 8, 8, 8, 8, None) == code, kw
        assert lib.svgp_cvae_predict(C.byref(cfg), 3, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, None) == code, kw
        assert lib.svgp_last_error()
    cfg = _cfg()
    assert lib.svgp_cvae_ws_layout_get(None, C.byref(wl)) == INVALID
    assert lib.svgp_cvae_ws_layout_get(C.byref(cfg), None) == INVALID and lib.svgp_cvae_param_layout_get(C.byref(cfg), None) == INVALID
    assert lib.svgp_cvae_train_step(C.byref(cfg), None, 8, 8, 8, 8, 8, 8, 8, 8, 1, None) == INVALID          # NULL theta
    assert lib.svgp_cvae_train_step(C.byref(cfg), 8, 8, None, 8, 8, 8, 8, 8, 8, 1, None) == INVALID          # cvae = 1 without aux
    assert lib.svgp_cvae_train_step(C.byref(cfg), 8, 8, 8, 8, 8, 8, None, 8, 8, 1, None) == INVALID          # Adam without moments
    assert lib.svgp_cvae_forward(C.byref(cfg), 8, 8, 8, 8, None, 8, None) == INVALID
    assert lib.svgp_cvae_encode(C.byref(cfg), 8, 8, 8, None, 8, None) == INVALID
    assert lib.svgp_cvae_decode(C.byref(cfg), 8, None, 8, 8, None) == INVALID
    assert lib.svgp_cvae_predict(C.byref(_cfg(cvae=0)), 3, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, None) == INVALID    # plain VAE
    assert lib.svgp_cvae_predict(C.byref(cfg), -1, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, None) == INVALID
    assert lib.svgp_cvae_predict(C.byref(cfg), 3, 8, 8, 8, 8, 8, 8, None, 8, 8, 8, None) == INVALID          # NULL work
    assert lib.svgp_cvae_step_route(C.byref(cfg), None, 256) == INVALID and lib.svgp_cvae_step_route(C.byref(cfg), buf, 8) == INVALID
    # b = 0: OK without a launch (no device here: a launch would fail)
    z = _cfg(b=0)
    assert lib.svgp_cvae_train_step(C.byref(z), 8, 8, 8, 8, 8, 8, 8, 8, 8, 1, None) == 0
    assert lib.svgp_cvae_forward(C.byref(z), 8, 8, 8, 8, 8, 8, None) == 0
    assert lib.svgp_cvae_encode(C.byref(z), 8, 8, 8, 8, 8, None) == 0 and lib.svgp_cvae_decode(C.byref(z), 8, 8, 8, 8, None) == 0
    assert lib.svgp_cvae_predict(C.byref(z), 3, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, None) == 0


def test_routes_and_lds(lib):
    buf = C.create_string_buffer(256)
    for L in (1, 16, CC.FUSED_LIMIT):           # one fused form up to the ceiling: the route does not depend on L
        for cvae, nm in ((0, "VAE"), (1, "CVAE")):
            assert lib.svgp_cvae_step_route(C.byref(_cfg(L=L, cvae=cvae)), buf, 256) == 0
            assert buf.value.decode().split() == [f"k_cvae_step_images<{nm}>", "k_cvae_reduce_adam"]
    assert lib.svgp_cvae_step_route(C.byref(_cfg(b=0)), buf, 256) == 0 and buf.value == b""
    assert lib.svgp_cvae_predict_route(C.byref(_cfg()), buf, 256) == 0
    assert buf.value.decode().split() == ["k_cvae_fwd<CVAE>:encode", "k_cvae_fwd<CVAE>:predict"]
    assert lib.svgp_cvae_predict_route(C.byref(_cfg(cvae=0)), buf, 256) == -1
    for cvae in (0, 1):
        sizes = {lib.svgp_cvae_lds_bytes(cvae, L) for L in range(1, 65)}
        assert len(sizes) == 1 and 0 < sizes.pop() <= 160 * 1024
        for L in (0, -3, 65, 1000):
            assert lib.svgp_cvae_lds_bytes(cvae, L) == -1
    assert lib.svgp_cvae_lds_bytes(2, 16) == -1 and lib.svgp_cvae_lds_bytes(-1, 16) == -1
    assert lib.svgp_cvae_lds_bytes(1, 16) > lib.svgp_cvae_lds_bytes(0, 16)


# ------------------------------------------------------------------------------------------------------------ the drivers
def test_driver_parser_and_refusals():
    from svgp_vae_amd import MNIST_experiment as M
    from svgp_vae_amd import VAE_experiment as V
    a = V.parser().parse_args(["--elbo", "CVAE"])
    assert vars(a) == vars(M.build_parser().parse_args(["--elbo", "CVAE"]))         # the MNIST driver's command line, unchanged
    assert "--clip_qs has no effect" in V.parser().format_help().replace("\n", " ").replace("  ", " ")
    V.check_args(a)
    V.check_args(V.parser().parse_args(["--elbo", "VAE", "--clip_qs", "--opt_regime", "joint-3"]))
    for extra, word in ((["--GECO"], "GECO"), (["--save_latents"], "save_latents"), (["--bias_analysis"], "bias_analysis"),
                        (["--restore", "x/model_3.pt"], "restore"), (["--first_epoch", "2"], "first_epoch")):
        for elbo in ("VAE", "CVAE"):
            with pytest.raises(NotImplementedError, match=word):
                V.main(["--elbo", elbo] + extra)
    for elbo in ("SVGPVAE_Hensman", "SVGPVAE_Titsias", "GPVAE_Casale", "GPVAE_Casale_batch", "SVIGP_Hensman"):
        with pytest.raises(NotImplementedError, match="MNIST_experiment"):
            V.main(["--elbo", elbo])


@pytest.mark.parametrize("elbo", ["VAE", "CVAE"])
def test_mnist_driver_names_the_new_command(elbo):
    from svgp_vae_amd.MNIST_experiment import main
    with pytest.raises(NotImplementedError) as e:
        main(["--elbo", elbo])
    msg = str(e.value)
    assert f"--elbo {elbo}" in msg and f"python -m svgp_vae_amd.VAE_experiment --elbo {elbo}" in msg


def test_mnist_driver_still_refuses_casale_batch():
    from svgp_vae_amd.MNIST_experiment import main
    with pytest.raises(NotImplementedError, match="GPVAE_Casale_batch"):
        main(["--elbo", "GPVAE_Casale_batch"])


def test_python_surface_without_a_device():
    from svgp_vae_amd import CVAE_model as M
    p = M.glorot_uniform_params(16, 0, cvae=True)
    assert sum(int(np.prod(v.shape)) for v in p.values()) == 6329
    assert p["enc_c1_w"].shape == (3, 3, 3, 8) and p["dec_c1_w"].shape == (3, 3, 10, 8) and not p["enc_d_b"].any()
    from svgp_vae_amd.VAE_utils import glorot_uniform_params
    pv, pv0 = M.glorot_uniform_params(16, 3, cvae=False), glorot_uniform_params(16, 3)
    assert all(np.array_equal(pv[k], pv0[k]) for k in pv0)
    vae = M.mnistCVAE(L=5, seed=1)
    assert vae.params["dec_d_w"].shape == (7, 128)
    with pytest.raises(NotImplementedError):
        M.mnistCVAE(im_width=32)


def test_step_kernels_compile_without_scratch():
    """csrc/cvae.hip keeps its kernels spill-free with two compiler-only measures (every threadIdx.x behind an empty asm, an opaque
    LDS base).  Neither shows in a result: an include reshuffle or another compiler could bring the scratch back
    silently, so the compiler's own resource remarks are checked here: ScratchSize 0 for every kernel of the file, and the step
    kernels within the 256 VGPRs that two waves per SIMD leave them."""
    import re
    import shutil
    import subprocess
    import tempfile
    csrc = os.path.join(os.path.dirname(HERE), "svgp-vae_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "cvae.hip"), "-o", os.path.join(d, "cvae.o")],
                           capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                kernels[name][key] = int(m.group(1))
    step = [k for k in kernels if "k_cvae_step_images" in k]
    assert len(step) == 2 and len([k for k in kernels if "k_cvae_fwd" in k]) == 2 and any("k_cvae_reduce_adam" in k for k in kernels)
    for k, v in kernels.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgprs"] <= 256, (k, v)
