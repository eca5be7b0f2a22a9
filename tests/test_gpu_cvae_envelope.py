"""svgp_cvae_train_step (csrc/cvae.hip) against the float64 restatement of tests/cvae_cases.py across the case table, both
variants: scalars, stored fields, every gradient, a 3-step Adam trajectory, bit reproducibility, no stale reads, guard bands,
adam = 0, the on-device draw, and -- mnistVAE only -- CasaleStepEngine.step("VAE") as an independent path through older kernels."""
import numpy as np
import pytest
import torch

from tests import cvae_cases as CC
from tests import helpers as H

pytestmark = pytest.mark.gpu

DT = torch.float64
VARIANTS = [(name, cvae) for name in CC.CASES for cvae in (False, True)]
_REF = {}


def _case(name, cvae):
    key = (name, cvae)
    if key not in _REF:
        c = CC.make_case(name, cvae)
        _REF[key] = (c, *CC.case_reference(c))
    return _REF[key]


def _vae(c, seed=0):
    from svgp_vae_amd.CVAE_model import mnistCVAE
    from svgp_vae_amd.VAE_utils import mnistVAE
    vae = (mnistCVAE if c["cvae"] else mnistVAE)(L=c["L"], seed=seed)
    vae.params = {k: v.clone() for k, v in c["params"].items()}
    return vae


def _engine(c, lr=1e-3, store=True):
    from svgp_vae_amd.CVAE_model import VaeStepEngine
    return VaeStepEngine(_vae(c), b_max=c["b_cap"], lr=lr, clip_qs=c["clip"], sigma=c["sigma"], store=store)


@pytest.mark.parametrize("name,cvae", VARIANTS)
def test_step_matches_restatement(name, cvae):
    c, out, grads = _case(name, cvae)
    if c["clip"]:
        mu, var_raw = CC.encode(c["params"], c["images"], c["aux"][:, 1], c["L"], cvae)
        CC.assert_clip_margin(var_raw)
        assert (var_raw < 1e-3).any() and (var_raw > 10).any() and ((var_raw > 1e-3) & (var_raw < 10)).any()
    eng = _engine(c)
    theta0, m0 = eng.theta.clone(), eng.adam_m.clone()
    eng.step(c["images"], c["aux"], c["eps"], adam=False)
    sc = eng.scalars()
    errs = {}
    for k in ("elbo", "recon_loss", "KL_term"):
        want = float(out[k])
        errs[k] = abs(sc[k] - want) / max(1.0, abs(want))
    for k in ("recon", "qnet_mu", "qnet_var", "z"):
        errs[k] = H.relerr(eng.ws_view(k), out[k])
    g = eng.grads()
    gerr = {k: H.relerr(g[k], grads[k]) for k in grads}
    print(f"{name} cvae={cvae}: scalars {max(errs[k] for k in ('elbo', 'recon_loss', 'KL_term')):.2e} "
          f"fields {max(errs[k] for k in ('recon', 'qnet_mu', 'qnet_var', 'z')):.2e} grads {max(gerr.values()):.2e}")
    for k in ("elbo", "recon_loss", "KL_term"):
        assert errs[k] <= CC.SCALAR_TOL, (k, errs[k])
    for k in ("recon", "qnet_mu", "qnet_var", "z"):
        assert errs[k] < CC.FWD_TOL, (k, errs[k])
    for k, e in gerr.items():
        assert e < CC.GRAD_TOL, (k, e)
    # adam = 0: theta and the moments bit-equal, the step count stays
    assert torch.equal(eng.theta, theta0) and torch.equal(eng.adam_m, m0) and not eng.adam_v.any()
    assert sc["adam_t"] == 0.0 and sc["rng_ctr"] == 0.0


@pytest.mark.parametrize("name,cvae", VARIANTS)
def test_three_step_trajectory(name, cvae):
    c, _, _ = _case(name, cvae)
    rng = np.random.RandomState(7)
    batches = [(c["images"], c["aux"], CC.t64(rng.randn(c["b"], c["L"]))) for _ in range(3)]
    want_p, want_elbo, _, _ = CC.train_trajectory(c["params"], batches, L=c["L"], cvae=cvae, lr=2e-3, clip=c["clip"])
    eng = _engine(c, lr=2e-3, store=False)
    for t, (img, aux, eps) in enumerate(batches):
        eng.step(img, aux, eps, adam=True)
        got = eng.scalars()["elbo"]
        assert abs(got - want_elbo[t]) <= CC.TRAJ_TOL * abs(want_elbo[t]), (t, got, want_elbo[t])
    assert eng.scalars()["adam_t"] == 3.0
    for k, v in want_p.items():
        assert H.relerr(eng.params[k], v) < CC.TRAJ_TOL, k


def _raw_step(c, *, store, fill, guard=64):
    """One adam = 0 step through the C entry point on buffers this test owns: ws pre-filled with `fill`, guard bands of `guard`
    doubles behind grad and ws.  Returns (grad, state, ws, guards intact)."""
    import ctypes as Ct
    from svgp_vae_amd import _lib
    from svgp_vae_amd.CVAE_model import _flat
    dev = torch.device("cuda:0")
    vae = _vae(c)
    cfg = _lib.CvaeCfg(b=c["b"], b_cap=c["b_cap"], L=c["L"], cvae=int(c["cvae"]), clip_qs=int(c["clip"]), store=store, sigma=c["sigma"])
    wl, pl = _lib.CvaeWsLayout(), _lib.ParamLayout()
    _lib.call("svgp_cvae_ws_layout_get", Ct.byref(cfg), Ct.byref(wl))
    _lib.call("svgp_cvae_param_layout_get", Ct.byref(cfg), Ct.byref(pl))
    n, tot = int(pl.n_total), int(wl.total)
    SENT = -12345.678
    ws = torch.full((tot + guard,), fill, dtype=DT, device=dev)
    ws[tot:] = SENT
    grad = torch.full((n + guard,), SENT, dtype=DT, device=dev)
    state = torch.zeros(_lib.STATE_LEN, dtype=DT, device=dev)
    theta = _flat(vae, dev)
    img, aux, eps = (c[k].to(dev).contiguous() for k in ("images", "aux", "eps"))
    _lib.call("svgp_cvae_train_step", Ct.byref(cfg), theta.data_ptr(), img.data_ptr(), aux[:, :2].contiguous().data_ptr(), eps.data_ptr(),
              ws.data_ptr(), grad.data_ptr(), None, None, state.data_ptr(), 0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    intact = bool((ws[tot:] == SENT).all()) and bool((grad[n:] == SENT).all())
    return grad[:n].cpu(), state.cpu(), ws[:tot].cpu(), intact, wl


@pytest.mark.parametrize("name,cvae", VARIANTS)
def test_bits_stale_reads_guards_and_store(name, cvae):
    c, _, _ = _case(name, cvae)
    g0, s0, w0, ok0, wl = _raw_step(c, store=1, fill=0.0)
    g1, s1, w1, ok1, _ = _raw_step(c, store=1, fill=0.0)
    gn, sn, wn, okn, _ = _raw_step(c, store=1, fill=float("nan"))
    gs, ss, ws_, oks, _ = _raw_step(c, store=0, fill=-7.0)
    assert ok0 and ok1 and okn and oks, "guard band behind grad or ws[total:] was written"
    assert torch.equal(g0, g1) and torch.equal(s0, s1), "the same step twice gave other bits"
    assert torch.equal(g0, gn) and torch.equal(s0, sn), "a NaN-filled workspace changed the result: something stale is read"
    assert torch.equal(g0, gs) and torch.equal(s0, ss), "store = 0 and store = 1 differ"
    b, L = c["b"], c["L"]
    for name_, n in (("recon", b * 784), ("qnet_mu", b * L), ("qnet_var", b * L), ("z", b * L)):
        off = int(getattr(wl, name_))
        assert torch.equal(w0[off:off + n], wn[off:off + n]), name_
        # the rows behind b (capacity b_cap) and the whole field with store = 0 keep their fill
        nxt = off + (n + 15) // 16 * 16 if c["b_cap"] == b else off + c["b_cap"] * (784 if name_ == "recon" else L)
        assert bool((w0[off + n:nxt] == 0.0).all()), f"{name_}: rows behind b written"
        assert bool((ws_[off:off + n] == -7.0).all()), f"{name_}: written with store = 0"
    assert torch.isfinite(g0).all()


@pytest.mark.parametrize("name,cvae", VARIANTS)
def test_device_draw(name, cvae):
    """eps = NULL: (z - mu) / sqrt(var) is finite and not constant, the counter in `state` advances, two calls draw different
    numbers.  (b1_L1 draws ONE number per call: "not constant" has nothing to compare there, the two calls still differ.)"""
    c, _, _ = _case(name, cvae)
    eng = _engine(c)
    eng.set_rng_counter(5.0)
    draws = []
    for _ in range(2):
        eng.step(c["images"], c["aux"], None, adam=False)
        e = (eng.ws_view("z") - eng.ws_view("qnet_mu")) / torch.sqrt(eng.ws_view("qnet_var"))
        assert torch.isfinite(e).all() and float(e.abs().max()) < 8.0
        if e.numel() > 1:
            assert float(e.max()) > float(e.min())
        if e.numel() >= 100:
            assert abs(float(e.mean())) < 0.5 and 0.5 < float(e.std()) < 1.5
        draws.append(e.clone())
    assert eng.scalars()["rng_ctr"] == 7.0
    assert not torch.equal(draws[0], draws[1])
    if c["b"] > 256:        # the second image of a workgroup draws at its own Philox index n L + l
        assert not torch.equal(draws[0][0], draws[0][256])
        assert len(torch.unique(draws[0])) == draws[0].numel()
    eng.forward(c["images"], c["aux"], None)
    assert eng.scalars()["rng_ctr"] == 8.0


@pytest.mark.parametrize("name", list(CC.CASES))
def test_vae_variant_matches_casale_vae_regime(name):
    """The VAE regime of CasaleStepEngine (ten entry points of older kernels) on the same rows: an independent path.
    That regime is the plain VAE WITHOUT clipping whatever the engine's clipping_qs says (k_vae_sample / k_vae_seeds of
    csrc/casale.hip take no clip argument; MNIST_experiment.py:870-876), so the `clip` case runs here with clip_qs = 0 on both sides:
    its shifted encoder biases still put exp(.) near 1e-4 and 90, the ends of the range the reverse pass sees; the clip mask itself
    is covered against the restatement above."""
    from tests import casale_cases as KC
    from svgp_vae_amd.CVAE_model import VaeStepEngine
    c, _, _ = _case(name, False)
    b, L = c["b"], c["L"]
    aux = np.stack([np.arange(b, dtype=np.float64), np.arange(b) % 3, (np.arange(b) % 5) * 0.7], 1)
    aux = aux[np.lexsort((aux[:, 2], aux[:, 1]))]
    aux[:, 0] = np.arange(b)
    params = dict(c["params"])
    params.update(l_GP=CC.t64(1.0), amplitude=CC.t64(0.9), alpha=CC.t64(0.15), object_vectors=CC.t64(np.ones((3, 2))))
    prob = dict(L=L, normalize=False, params=params, images=c["images"], aux=aux, object_vectors=np.ones((3, 2)), l_GP=1.0,
                amplitude=0.9, alpha=0.15)
    ceng = KC.step_engine(prob, batch_size=b, beta=1.0, clip=c["clip"], ov_joint=True)
    ceng.step("VAE", 0, b, eps_batch=c["eps"].to(ceng.dev), adam=False)
    csc, cg = ceng.scalars(), ceng.grads()
    eng = VaeStepEngine(_vae(c), b_max=c["b_cap"], lr=1e-3, clip_qs=False, sigma=c["sigma"])
    eng.step(c["images"], c["aux"], c["eps"], adam=False)
    sc, g = eng.scalars(), eng.grads()
    assert abs(sc["elbo"] - csc["elbo"]) <= CC.GRAD_TOL * abs(csc["elbo"])
    assert abs(sc["KL_term"] - csc["KL_term"]) <= CC.GRAD_TOL * max(1.0, abs(csc["KL_term"]))
    assert abs(sc["recon_loss"] - csc["recon_loss"]) <= CC.GRAD_TOL * max(1.0, abs(csc["recon_loss"]))
    gerr = {k: H.relerr(g[k], cg[k]) for k in CC.VAE_NAMES}
    print(f"{name}: against the Casale VAE regime, grads {max(gerr.values()):.2e}")
    for k, e in gerr.items():
        assert e < CC.GRAD_TOL, (k, e)
