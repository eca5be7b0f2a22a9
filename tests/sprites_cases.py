"""SPRITES step test problems, engine builder, comparison and the shape-envelope case tables, shared by
tests/test_gpu_sprites_envelope.py (GPU) and tests/test_sprites_envelope_oracle_cpu.py (the oracle's own response at every case).
The problem builder is the one of tests/test_gpu_sprites.py, restated."""
import functools
import math

import torch

from oracle import sprites_oracle as SO

DT = torch.float64

# Tolerances of tests/test_gpu_sprites.py (float64 end to end), relative to the tensor's max-abs with a 1e-9 floor (rel): each
# member of the 16-tuple, each gradient.  The four SE hyper-parameter gradients are compared for the `se` kernel only.
FWD_TOL, GRAD_TOL = 1e-8, 1e-6
# float32 networks against the float64 oracle: the bars of tests/test_gpu_f32.py::test_sprites_step_float32
F32_ENC_TOL, F32_ELBO_TOL, F32_POST_TOL, F32_WGRAD_TOL = 1e-4, 1e-3, 1e-2, 2e-2
F32_WGRADS = ("enc_c1_w", "dec_c7_w", "dec_c1_w", "repr_c1_w", "enc_d_w", "dec_d_w")

JITTER, N_TRAIN, BETA = 0.01, 100.0, 0.001
C_MA, LAGRANGE, ALPHA, KAPPA_SQUARED = 0.02, 1.4, 0.9, 0.0075
SE_SCALES = (5.0, 1.4, 7.0, 1.2)          # l_action, sigma_action, l_character, sigma_character
SE_NAMES = ("l_action", "sigma_action", "l_character", "sigma_character")
TUPLE_NAMES = ("elbo", "recon_loss", "KL_term", "inside_elbo", "ce_term", "p_m", "p_v", "qnet_mu", "qnet_var", "recon_images",
               "inside_elbo_recon", "inside_elbo_kl", "latent_samples", "C_ma", "lagrange_mult", "aux_data")


def _case(b, seg, L, La, Lc, m, n_act, kernel, geco, titsias, **kw):
    assert kernel in ("lin", "cos", "se") and b % seg == 0
    return dict(b=b, seg=seg, L=L, La=La, Lc=Lc, m=m, n_act=n_act, kernel=kernel, geco=geco, titsias=titsias,
                clip_qs=kw.pop("clip_qs", True), clip_grad=kw.pop("clip_grad", None), b_max=kw.pop("b_max", b), **kw)


# name: (b, seg_len, L, L_action, L_character, m, n_act, kernel, GECO, titsias).  The problem's seed is 200 + the row's index.
CASES = {
    "L1": _case(12, 3, 1, 8, 16, 10, 9, "lin", True, False),              # one channel
    "L17": _case(8, 4, 17, 8, 16, 12, 9, "cos", False, False),            # first L past the other tests
    "L33se": _case(8, 4, 33, 8, 16, 10, 9, "se", True, False, clip_grad=0.05),
    "L64m64": _case(16, 4, 64, 8, 16, 64, 9, "cos", True, False),         # LDS path at both limits
    "m1": _case(8, 4, 6, 8, 16, 1, 9, "cos", True, False),                # one inducing point
    "m2se": _case(8, 4, 6, 8, 16, 2, 9, "se", False, False),
    "m31": _case(8, 4, 6, 8, 16, 31, 9, "cos", True, False),              # generic instance below kern<32>
    "m32": _case(8, 4, 6, 8, 16, 32, 9, "cos", False, False),             # the instance of its own
    "m33": _case(8, 4, 6, 8, 16, 33, 9, "se", True, False),               # four-matrix form
    "m65": _case(8, 4, 6, 8, 16, 65, 9, "cos", True, False),              # first global-memory shape
    "m130L64t": _case(36, 3, 64, 8, 16, 130, 5, "cos", True, True),       # Titsias, m not a multiple of 64, largest L
    "m130L22": _case(36, 3, 22, 8, 16, 130, 5, "se", False, False),
    "seg1b5": _case(5, 1, 6, 8, 16, 12, 9, "cos", True, False),           # every frame its own character, odd b
    "seg7f5_11": _case(21, 7, 6, 5, 11, 12, 3, "se", True, False),        # generic repr-net kernels (Lc = 11), bucket (8,16) not filled
    "f16_16": _case(8, 4, 6, 16, 16, 12, 4, "cos", True, False),          # bucket (16,32) at its La bound
    "f9_16se": _case(8, 4, 6, 9, 16, 12, 4, "se", True, False),           # first La in the second bucket
    "f20_9": _case(8, 4, 6, 20, 9, 12, 4, "se", False, False),            # outside both buckets: per-target reference kernels
    "f32_16": _case(8, 4, 6, 32, 16, 12, 4, "cos", True, False),          # SP_MAXD x conv channel limit
    "f1_1": _case(8, 4, 6, 1, 1, 3, 4, "se", True, False),                # one-dimensional feature groups, one-channel repr net
    "Lc3": _case(8, 2, 6, 8, 3, 12, 9, "lin", True, False),
    "nact1": _case(8, 4, 6, 8, 16, 12, 1, "cos", True, False),            # every row hits GPLVM row 0
    "b1": _case(1, 1, 6, 8, 16, 4, 9, "cos", True, False),
    "noclip": _case(8, 4, 6, 8, 16, 12, 9, "cos", False, False, clip_qs=False),      # every other step test clips q's variance
    "b127": _case(127, 1, 6, 8, 16, 24, 9, "se", True, False),            # b_max = 127: one statistics partition
    "b128": _case(128, 8, 6, 8, 16, 24, 9, "cos", True, False),           # b_max = 128: four
    "b260": _case(260, 5, 6, 8, 16, 40, 9, "cos", False, False),          # past 256 rows
    # problems of the below-capacity tests: built once at the capacity, stepped with their first rows (CAPACITY_BATCHES)
    "cap24m12": _case(24, 4, 6, 8, 16, 12, 9, "se", True, False),
    "cap24m72": _case(24, 4, 6, 8, 16, 72, 9, "cos", False, False),
}
ENVELOPE_CASES = [c for c in CASES if not c.startswith("cap")]
# case -> the row counts one engine of the case's capacity is stepped with, in this order: a small batch follows the full one
CAPACITY_BATCHES = {"cap24m12": (4, 12, 20, 24, 4), "cap24m72": (4, 12, 20, 24, 4), "b260": (5, 255, 260, 5)}
SIDE_STREAM_CASES = ("m130L22", "m65")
F32_CASES = ("seg7f5_11", "L33se")


def problem(b, frames, L, La, Lc, m, n_act, seed):
    """(network parameters, GP parameters, images, action ids, eps, segment ids, repeats): tests/test_gpu_sprites.py::_problem."""
    g = torch.Generator().manual_seed(seed)
    params = {k: torch.tensor(v, dtype=DT) for k, v in SO.glorot_init(L, Lc, seed).items()}
    for k in params:
        if k.endswith("_b"):
            params[k] = 0.05 * torch.randn(*params[k].shape, dtype=DT, generator=g)
    gp = dict(inducing_index_points=torch.randn(m, La + Lc, dtype=DT, generator=g) * 1.5,
              GPLVM_action=torch.randn(n_act, La, dtype=DT, generator=g) * 1.5,
              # SE scales chosen so that kernel values are O(0.1..1) for N(0,1.5^2) features (distances ~6-8)
              **{k: torch.tensor(v, dtype=DT) for k, v in zip(SE_NAMES, SE_SCALES)})
    images = torch.rand(b, 64, 64, 3, dtype=DT, generator=g)
    ids = torch.randint(0, n_act, (b,), generator=g)
    eps = torch.randn(b, L, dtype=DT, generator=g)
    seg, rep = SO.aux_data_sprites_utils(b, frames, frames)
    return params, gp, images, ids, eps, seg, rep


def rel(a, c):
    a, c = torch.as_tensor(a, dtype=DT).cpu().reshape(-1), torch.as_tensor(c, dtype=DT).cpu().reshape(-1)
    return float((a - c).abs().max() / max(float(c.abs().max()), 1e-9))     # gradients below 1e-9 are noise


def case_problem(case):
    cs = CASES[case]
    return problem(cs["b"], cs["seg"], cs["L"], cs["La"], cs["Lc"], cs["m"], cs["n_act"], seed=200 + list(CASES).index(case))


def oracle(cs, params, gp, images, ids, eps, rows=None):
    """The oracle's (16-tuple, gradients) for the first `rows` rows (default: all) of a case's problem."""
    b = cs["b"] if rows is None else rows
    assert b % cs["seg"] == 0
    seg, rep = SO.aux_data_sprites_utils(b, cs["seg"], cs["seg"])
    return SO.loss_and_grads(params, gp, (images[:b], ids[:b]), eps[:b], formulation="efficient", beta=BETA,
                             C_ma=torch.tensor(C_MA, dtype=DT), lagrange_mult=torch.tensor(LAGRANGE, dtype=DT), alpha=ALPHA,
                             kappa=math.sqrt(KAPPA_SQUARED), L=cs["L"], L_action=cs["La"], jitter=JITTER, N_train=N_TRAIN,
                             segment_ids=seg, repeats=rep, clipping_qs=cs["clip_qs"], GECO=cs["geco"],
                             K_obj_normalize=cs["kernel"] == "cos", K_SE=cs["kernel"] == "se", clip_grad=cs["clip_grad"],
                             titsias=cs["titsias"])


def reference(case, rows=None):
    """(params, gp, images, ids, eps, oracle 16-tuple, oracle gradients) of a CASES entry, the last five for its first `rows` rows
    (default: all); computed once per process and shared: callers must not write to it."""
    return _reference(case, CASES[case]["b"] if rows is None else rows)


@functools.lru_cache(maxsize=None)
def _reference(case, b):
    params, gp, images, ids, eps, _, _ = case_problem(case)
    want, wgrads = oracle(CASES[case], params, gp, images, ids, eps, b)
    return params, gp, images[:b].contiguous(), ids[:b].contiguous(), eps[:b].contiguous(), want, wgrads


def oracle_response(case, rows=None):
    """The oracle evaluated again with every real input (parameters, images, eps) multiplied by 1 + 2^-52: the largest
    relative change (rel) over the 16-tuple and over the gradients that the GPU test compares."""
    cs = CASES[case]
    params, gp, images, ids, eps, want, wgrads = reference(case, rows)
    ulp = 1.0 + 2.0 ** -52
    want2, wgrads2 = oracle(cs, {k: v * ulp for k, v in params.items()}, {k: v * ulp for k, v in gp.items()}, images * ulp, ids,
                            eps * ulp, rows)
    e_fwd = max(rel(want2[i], want[i]) for i in range(16))
    e_grad = max(rel(wgrads2[k], w) for k, w in wgrads.items() if k not in SE_NAMES)
    if cs["kernel"] == "se":
        e_grad = max(e_grad, rel(torch.stack([wgrads2[k] for k in SE_NAMES]), torch.stack([wgrads[k] for k in SE_NAMES])))
    return e_fwd, e_grad


def engine(case, params, gp, *, b_max=None, **kw):
    """A SpritesStepEngine for a CASES entry, initialised with the problem's parameters and the common scalars."""
    from svgp_vae_amd import sprites as S
    cs = CASES[case]
    svgp = S.spritesSVGP(cs["titsias"], False, gp["inducing_index_points"].numpy(), 'main', JITTER, N_TRAIN, cs["La"],
                         gp["GPLVM_action"].numpy(), cs["Lc"], cs["L"], fixed_GP_params=False, fixed_GPLVM=False,
                         K_obj_normalize=cs["kernel"] == "cos", K_SE=cs["kernel"] == "se")
    init = dict(params)
    init["se"] = torch.stack([gp[k] for k in SE_NAMES])
    eng = S.SpritesStepEngine(S.spritesVAE(cs["L"]), S.sprites_representation_network(cs["Lc"]), svgp,
                              b_max=cs["b_max"] if b_max is None else b_max, seg_len=cs["seg"], clip_qs=cs["clip_qs"],
                              geco=cs["geco"], kappa_squared=KAPPA_SQUARED, beta=BETA, clip_grad=cs["clip_grad"], params=init, **kw)
    eng.set_scalars(c_ma=C_MA, lagrange=LAGRANGE, alpha=ALPHA)
    return eng


def step(eng, images, ids, eps):
    """One step without the optimiser from the common scalars (GECO steps move C_ma and the multiplier: set again)."""
    eng.set_scalars(c_ma=C_MA, lagrange=LAGRANGE, alpha=ALPHA)
    dev = eng.dev
    eng.step(images.to(dev), ids.to(dev, DT), eps.to(dev), adam=False)
    eng.scalars()                      # synchronises; raises SvgpError if a stage of the step reported one
    return eng.outputs()


def compare(eng, got, want, wgrads, se, label):
    """Every member of the 16-tuple and every gradient against the oracle; finiteness of all of them.
    Returns (failures, worst forward error, worst gradient error) and prints each figure."""
    bad, e_fwd, e_grad = [], 0.0, 0.0
    for i, n in enumerate(TUPLE_NAMES):
        if not bool(torch.isfinite(torch.as_tensor(got[i])).all()):
            bad.append(f"{n} is not finite")
        e = rel(got[i], want[i])
        e_fwd = max(e_fwd, e)
        print(f"{label} {n}: {e:.2e}")
        if not e < FWD_TOL:
            bad.append(f"{n} rel {e:.3e}")
    g = eng.grads
    todo = [(k, g[k], w) for k, w in wgrads.items() if k not in SE_NAMES]
    if se:
        todo.append(("se", g["se"], torch.stack([wgrads[k] for k in SE_NAMES])))
    for k, have, w in todo:
        if not bool(torch.isfinite(have).all()):
            bad.append(f"grad {k} is not finite")
        e = rel(have, w)
        e_grad = max(e_grad, e)
        print(f"{label} grad {k}: {e:.2e} (max {float(w.abs().max()):.2e})")
        if not e < GRAD_TOL:
            bad.append(f"grad {k} rel {e:.3e} (max {float(w.abs().max()):.2e})")
    print(f"{label} WORST forward {e_fwd:.2e} gradient {e_grad:.2e}")
    return bad, e_fwd, e_grad
