"""Shared test helpers: toy problems and the oracle's stage-by-stage intermediates."""
import math

import numpy as np
import torch

from oracle import staged_gp as SG
from oracle import svgpvae_oracle as O

DT = torch.float64


def toy_problem(b=40, m=12, L=3, M=4, n_obj=20, seed=0, with_table=True):
    """Random rotated-MNIST-shaped problem.  Returns (params dict of float64 CPU tensors, images, aux, eps)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=DT, generator=g)
    u = lambda *s: torch.rand(*s, dtype=DT, generator=g)
    params = {k: torch.tensor(v, dtype=DT) for k, v in O.glorot_uniform_init(L, seed).items()}
    for k in list(params):
        if k.endswith("_b"):
            params[k] = 0.1 * r(*params[k].shape)
    params["inducing_index_points"] = torch.cat([torch.arange(m, dtype=DT)[:, None], u(m, 1) * 6.28,
                                                 r(m, M) * 1.5], 1)
    params["l_GP"] = torch.tensor(1.2, dtype=DT)
    params["amplitude"] = torch.tensor(0.9, dtype=DT)
    if with_table:
        params["object_vectors"] = r(n_obj, M) * 1.5
    ids = torch.randint(0, max(n_obj, 1), (b, 1), generator=g).to(DT)
    aux = torch.cat([ids, u(b, 1) * 6.28, r(b, M) * 1.5], 1).contiguous()
    images = torch.clamp(0.142 + 0.316 * r(b, 28, 28, 1), -0.2, 1.2).contiguous()
    eps = r(b, L).contiguous()
    return params, images, aux, eps


def golden_problem(golden, rows=slice(0, 256)):
    gin, _ = golden
    params = {k[4:]: torch.tensor(v, dtype=DT) for k, v in gin.items() if k.startswith("vae_")}
    for k in ("inducing_index_points", "l_GP", "amplitude", "object_vectors"):
        params[k] = torch.tensor(gin[k], dtype=DT)
    images, aux, eps = (torch.tensor(gin[k][rows], dtype=DT).contiguous() for k in ("images", "aux", "epsilon"))
    return params, images, aux, eps


def oracle_stages(params, images, aux, eps, *, N_train, jitter, clip_qs, geco, beta, lagrange_mult=1.0,
                  K_obj_normalize=False, b_global=None):
    """Every intermediate the HIP workspace exposes, from the oracle (single rank)."""
    L = eps.shape[1]
    b = images.shape[0]
    bg = float(b if b_global is None else b_global)
    c = N_train / bg
    vae = O.MnistVAE(params, L)
    mu, var_raw = vae.encode(images)
    var = O.clip_by_value(var_raw, 1e-3, 10.0) if clip_qs else var_raw
    ov = params.get("object_vectors")
    K, Kn, knn = SG.kernel_matrix_fwd(aux, params["inducing_index_points"], ov, params["l_GP"],
                                      params["amplitude"], K_obj_normalize)
    p = O.reciprocal_no_nan(var)
    S, v, _ = SG.gp_stats(Kn, p, p * mu)
    f = SG.gp_factor_fwd(K, S, v, jitter, c)
    ps = SG.gp_posterior_fwd(Kn, knn, mu, var, eps, f, c)
    recon = vae.decode(ps["z"])
    out = dict(qnet_mu=mu, qnet_var_raw=var_raw, qnet_var=var, K=K, Kn=Kn, knn=knn, S=S, v=v, Ki=f["Ki"],
               ldK=f["ldK"].reshape(1), Si=f["Si"], t=f["t"], G=f["G"], A=f["A"], Aji=f["Aji"], mu_hat=f["mu"],
               u=f["u"], KL=f["KL"], q=ps["q"], p_m=ps["p_m"], p_v=ps["p_v"], e=ps["e"], d=ps["d"], z=ps["z"],
               recon=recon.reshape(b, 784),
               M2=f["Ki"][None] @ f["A"] @ f["Ki"][None])
    return out


def engine_for(params, b, *, geco, clip_qs=True, N_train=4050.0, jitter=1e-6, beta=0.001, lr=1e-3,
               K_obj_normalize=False, alpha=0.99, kappa_squared=0.020, **kw):
    from svgp_vae_amd.engine import MnistStepEngine
    m, Mp2 = params["inducing_index_points"].shape
    L = params["dec_d_w"].shape[0]
    n_obj = params["object_vectors"].shape[0] if "object_vectors" in params else 0
    eng = MnistStepEngine(m, L, Mp2 - 2, n_obj, N_train=N_train, jitter=jitter, clip_qs=clip_qs, geco=geco,
                          K_obj_normalize=K_obj_normalize, beta=beta, lr=lr, alpha=alpha,
                          kappa_squared=kappa_squared, b_max=b, **kw)
    eng.load_params(params)
    return eng


def relerr(a, b):
    a = torch.as_tensor(a, dtype=DT).cpu().reshape(-1)
    b = torch.as_tensor(b, dtype=DT).cpu().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ---------------------------------------------------------------- one training step of the HIP engine against the oracle
# Tolerances (float64 end to end): forward intermediates 1e-9 relative to the tensor's max-abs, scalars 1e-9 relative,
# gradients 1e-7 relative to the tensor's max-abs (tests/test_gpu_parity.py).
FWD_TOL, GRAD_TOL, SCALAR_TOL = 1e-9, 1e-7, 1e-9

FIELD_SHAPES = lambda b, m, L: dict(
    qnet_mu=(b, L), qnet_var_raw=(b, L), qnet_var=(b, L), K=(m, m), Kn=(b, m), knn=(b,), S=(L, m, m), v=(L, m),
    Ki=(m, m), ldK=(1,), Si=(L, m, m), t=(L, m), G=(L, m, m), A=(L, m, m), Aji=(L, m, m), mu_hat=(L, m),
    u=(L, m), M2=(L, m, m), KL=(L,), q=(b,), p_m=(b, L), p_v=(b, L), e=(b, L), d=(b, L), z=(b, L),
    recon=(b, 784))


def _run_once(eng, images, aux, eps, adam=False):
    dev = eng.device
    eng.bind(images.to(dev), aux.to(dev), None if eps is None else eps.to(dev))
    eng.run(adam=adam)
    eng.synchronize()


def _compare_step(params, images, aux, eps, *, geco, clip_qs=True, N_train=4050.0, jitter=1e-6, beta=0.001,
                  K_obj_normalize=False, C_ma=0.0, lagrange=1.0, alpha=0.0, kappa2=0.020, label="",
                  FWD_TOL=FWD_TOL, GRAD_TOL=GRAD_TOL, self_consistency=False, b_max=None, eng=None):
    """One step (no Adam) of a fresh engine -- built for b_max >= b rows of capacity when b_max is given -- or of `eng`, an
    engine of the same shape and settings built earlier (params are loaded into it), against the float64 oracle.
    Returns (list of failures, engine)."""
    b, L = eps.shape
    m = params["inducing_index_points"].shape[0]
    if eng is None:
        eng = engine_for(params, b if b_max is None else b_max, geco=geco, clip_qs=clip_qs, N_train=N_train, jitter=jitter,
                         beta=beta, K_obj_normalize=K_obj_normalize, kappa_squared=kappa2)
    else:
        eng.load_params(params)
    if eng.cfg.b != b:
        eng.set_batch_size(b)
    eng.set_scalars(c_ma=C_ma, lagrange=lagrange, alpha=alpha)
    _run_once(eng, images, aux, eps)
    bad = []
    ref = oracle_stages(params, images, aux, eps, N_train=N_train, jitter=jitter, clip_qs=clip_qs, geco=geco,
                        beta=beta, K_obj_normalize=K_obj_normalize)
    fwd_tol = {name: FWD_TOL for name in FIELD_SHAPES(b, m, L)}
    p2 = img2 = None
    if self_consistency:
        # ill-conditioned cases: the yardstick is the oracle's own response to a one-ulp perturbation of its real inputs
        # (what any two backward-stable float64 evaluations of these formulas may differ by; tests/test_gpu_fullsize.py);
        # the HIP result must sit within 20x of it, forward fields, scalars and gradients alike
        gen = torch.Generator().manual_seed(17)
        ulp = lambda t: t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=gen).to(DT) * 2 - 1))
        p2 = {k: ulp(v) for k, v in params.items()}
        p2["inducing_index_points"][:, 0] = params["inducing_index_points"][:, 0]
        img2 = ulp(images)
        ref2 = oracle_stages(p2, img2, aux, eps, N_train=N_train, jitter=jitter, clip_qs=clip_qs, geco=geco,
                             beta=beta, K_obj_normalize=K_obj_normalize)
        fwd_tol = {name: max(FWD_TOL, 20 * relerr(ref2[name], ref[name])) for name in fwd_tol}
    for name, shp in FIELD_SHAPES(b, m, L).items():
        if name == "M2" and m > 64:
            # the large-m path evaluates k^T M2 k as w^T Si w and does not form M2 = Ki A Ki (gp_large.hip, "W form"): its
            # channel-independent rows W = Kn Ki K sit behind the b rows of K_nm and are compared instead
            W = eng.ws[eng.wl.Kn + b * m:eng.wl.Kn + 2 * b * m].view(b, m)
            want = ref["Kn"] @ ref["Ki"] @ ref["K"]
            err = relerr(W, want)
            if not err < fwd_tol["M2"]:
                bad.append(f"{label} fwd W: rel {err:.3e} (tol {fwd_tol['M2']:.1e})")
            continue
        err = relerr(eng.ws_view(name, shp), ref[name])
        if not err < fwd_tol[name]:
            bad.append(f"{label} fwd {name}: rel {err:.3e} (tol {fwd_tol[name]:.1e})")
    out, grads = O.loss_and_grads(params, images, aux, eps, beta=beta, C_ma=torch.tensor(C_ma, dtype=DT),
                                  lagrange_mult=torch.tensor(lagrange, dtype=DT), alpha=alpha,
                                  kappa=math.sqrt(kappa2), clipping_qs=clip_qs, GECO=geco, jitter=jitter,
                                  N_train=N_train, L=L, formulation="efficient", K_obj_normalize=K_obj_normalize)
    sc = eng.scalars()
    out_ulp = g_ulp = None
    if self_consistency:
        out_ulp, g_ulp = O.loss_and_grads(p2, img2, aux, eps, beta=beta, C_ma=torch.tensor(C_ma, dtype=DT),
                                          lagrange_mult=torch.tensor(lagrange, dtype=DT), alpha=alpha,
                                          kappa=math.sqrt(kappa2), clipping_qs=clip_qs, GECO=geco, jitter=jitter,
                                          N_train=N_train, L=L, formulation="efficient",
                                          K_obj_normalize=K_obj_normalize)
    for key, idx in (("elbo", 0), ("recon_loss", 1), ("kl_term", 2), ("inside_elbo", 3), ("ce_term", 4),
                     ("inside_recon", 10), ("inside_kl", 11)):
        want = float(out[idx])
        stol = SCALAR_TOL * max(1.0, abs(want))
        if out_ulp is not None:
            stol = max(stol, 20 * abs(float(out_ulp[idx]) - want))
        if not abs(sc[key] - want) <= stol:
            bad.append(f"{label} scalar {key}: got {sc[key]!r} want {want!r} (tol {stol:.1e})")
    if geco:
        for key, idx in (("c_ma", 13), ("lagrange", 14)):
            want = float(out[idx])
            if not abs(sc[key] - want) <= SCALAR_TOL * max(1.0, abs(want)):
                bad.append(f"{label} scalar {key}: got {sc[key]!r} want {want!r}")
    tol = {k: GRAD_TOL for k in grads}
    if self_consistency:
        # ill-conditioned cases: the oracle's literal and efficient formulations (same mathematics, float64)
        # disagree by far more than GRAD_TOL; the HIP result must sit within 5x of that self-disagreement
        _, g_lit = O.loss_and_grads(params, images, aux, eps, beta=beta, C_ma=torch.tensor(C_ma, dtype=DT),
                                    lagrange_mult=torch.tensor(lagrange, dtype=DT), alpha=alpha,
                                    kappa=math.sqrt(kappa2), clipping_qs=clip_qs, GECO=geco, jitter=jitter,
                                    N_train=N_train, L=L, formulation="literal", K_obj_normalize=K_obj_normalize)
        # ... or within 20x of the oracle's response to the one-ulp input perturbation above
        tol = {k: max(GRAD_TOL, 5 * relerr(g_lit[k], grads[k]), 20 * relerr(g_ulp[k], grads[k])) for k in grads}
    g = eng.grads()
    for k, want in grads.items():
        err = relerr(g[k], want)
        if not err < tol[k]:
            bad.append(f"{label} grad {k}: rel {err:.3e} (max|want| {float(want.abs().max()):.3e})")
    return bad, eng
