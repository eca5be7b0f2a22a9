"""Cases, builders and float64 references of the SPRITES posterior cache / animate tests (tests/test_animate_cpu.py,
tests/test_gpu_animate.py).

Kernel cases: svgp_sprites_posterior_rows on synthetic inputs -- X ~ N(0, 1), NOT symmetric -- against a float64 numpy einsum.
Stage cases: svgp_sprites_kernel_matrix_fwd then svgp_sprites_posterior_rows against the oracle's
approximate_posterior_params_precomputed with the oracle's own mean_terms, Sigma^-1 and jitter-free K_mm^-1.
Pipeline: the problem of tests/test_gpu_sprites_cgen.py::test_sprites_test_character_pipeline.

Bars (the project's own, tests/generate_cases.py; relative to the tensor's max-abs, helpers.relerr): against the oracle TOL = 1e-8,
which holds only where the oracle's own response to a one-ulp change of its inputs stays within 1/100 of it; between two
evaluations of the same algebra PATH_TOL = 1e-10, where the reference in a second summation order moves by at most 1e-12.
test_animate_cpu.py asserts both guards for every case below."""
import functools

import numpy as np
import torch

from oracle import sprites_oracle as SO
from oracle import svgpvae_oracle as O

DT = torch.float64
TOL, PATH_TOL = 1e-8, 1e-10
CLIP = (1e-4, 100.0)                 # SVGPVAE_model.py:1180
LA, LC, N_ACT = 8, 16, 9
SE = (5.0, 1.4, 7.0, 1.2)            # l_action, sigma_action, l_character, sigma_character (tests/test_gpu_sprites_cgen.py)

# (b, m, L): the edges of a 16-wide MFMA tile in rows and columns, one row, one channel, the 64 / 65 boundary the library uses
# elsewhere, more rows than one workgroup's block (64), several column tiles (130); beyond m = 256 the entry deals the column tiles
# of a row block to several workgroups and adds their partial sums in a second launch: the last shape of the one-launch form (256),
# the first of the split form (257) and one with more rows than a block; and a last case whose p_v are clamped
KERNEL_CASES = [(1, 1, 1), (17, 15, 3), (16, 16, 2), (33, 17, 3), (40, 64, 2), (40, 65, 4), (70, 130, 2), (5, 33, 6), (300, 72, 8),
                (9, 256, 2), (17, 257, 3), (70, 300, 2)]
CLAMP_CASE = "clamp"                 # (40, 33, 3) with k^T X k of the size of the clip range
KERNEL_IDS = [f"{b}-{m}-{L}" for b, m, L in KERNEL_CASES] + [CLAMP_CASE]


def kernel_shape(case):
    return (40, 33, 3) if case == CLAMP_CASE else tuple(int(v) for v in case.split("-"))


@functools.lru_cache(maxsize=None)
def kernel_problem(case):
    """dict(Kb (b,m), kbb (b), w (L,m), X (L,m,m), eps (b,L)) float64 numpy, never modified.  Kb ~ N(0, 10 / m): k^T X k has
    standard deviation ~10 around kbb ~ 50, inside the clip range; the clamp case: ~80 around 50, on both sides of it."""
    b, m, L = kernel_shape(case)
    rs = np.random.RandomState(1000 + 7 * b + 3 * m + L + (500 if case == CLAMP_CASE else 0))
    s2 = (80.0 if case == CLAMP_CASE else 10.0) / m
    return dict(Kb=np.sqrt(s2) * rs.randn(b, m), kbb=50.0 + rs.rand(b), w=rs.randn(L, m), X=rs.randn(L, m, m),
                eps=rs.randn(b, L))


def kernel_reference(case, flip=False, clip=CLIP):
    """(p_m, p_v clamped, z, p_v unclamped) by einsum; flip: the same sums with the inducing index reversed (a second order)."""
    p = kernel_problem(case)
    Kb, X, w = p["Kb"], p["X"], p["w"]
    if flip:
        Kb, X, w = Kb[:, ::-1].copy(), X[:, ::-1, ::-1].copy(), w[:, ::-1].copy()
    p_m = np.einsum("bm,lm->bl", Kb, w)
    raw = p["kbb"][:, None] + np.einsum("bi,lij,bj->bl", Kb, X, Kb)
    p_v = np.clip(raw, *clip)
    return p_m, p_v, p_m + p["eps"] * np.sqrt(p_v), raw


# ---------------------------------------------------------------------------------------------- stage cases
# name -> (m, L, train rows, query rows, K_SE)
STAGE_CASES = {
    "se-1-1": (1, 1, 20, 1, True), "se-15-3": (15, 3, 48, 17, True), "se-16-2": (16, 2, 48, 16, True),
    "se-17-3": (17, 3, 48, 33, True), "se-64-2": (64, 2, 150, 40, True), "se-65-4": (65, 4, 150, 40, True),
    "se-130-2": (130, 2, 300, 70, True), "se-33-6": (33, 6, 100, 5, True),
    "lin-12-3": (12, 3, 48, 17, False),          # normalised linear x linear: m below the rank bound LA * LC of that kernel
}


@functools.lru_cache(maxsize=None)
def stage_problem(case):
    """dict(ip, table, aux (train rows [action id, character vector]), mu, var, qaux (query rows), eps); CPU float64, never modified."""
    m, L, n, q, _ = STAGE_CASES[case]
    g = torch.Generator().manual_seed(100 + sorted(STAGE_CASES).index(case))
    rn = lambda *s: torch.randn(*s, dtype=DT, generator=g)
    rows = lambda k: torch.cat([torch.randint(0, N_ACT, (k, 1), generator=g).to(DT), 1.5 * rn(k, LC)], 1)
    return dict(ip=1.5 * rn(m, LA + LC), table=1.5 * rn(N_ACT, LA), aux=rows(n), mu=rn(n, L),
                var=0.5 + torch.rand(n, L, dtype=DT, generator=g), qaux=rows(q), eps=rn(q, L))


def stage_svgp(case, p):
    K_SE = STAGE_CASES[case][4]
    se = dict(zip(("l_action", "sigma_action", "l_character", "sigma_character"), (torch.tensor(v, dtype=DT) for v in SE)))
    return SO.SpritesSVGP(p["ip"], p["table"], 0.01, float(p["aux"].shape[0]), LA, K_obj_normalize=not K_SE, K_SE=K_SE, se_params=se)


def stage_outputs(case, p=None):
    """dict(w (L,m), Si (L,m,m), Ki (m,m), p_m, p_v (clamped), z) of the oracle, optionally at other inputs (the one-ulp response)."""
    p = stage_problem(case) if p is None else p
    L = STAGE_CASES[case][1]
    svgp = stage_svgp(case, p)
    w, Si = SO.precompute_GP_params_SVGPVAE(p["mu"], p["var"], p["aux"], svgp)
    Ki = torch.linalg.inv(svgp.kernel_matrix(p["ip"], p["ip"]))
    pm, pv = zip(*(SO.approximate_posterior_params_precomputed(svgp, p["qaux"], w[l], Si[l], Ki) for l in range(L)))
    p_m, p_v = torch.stack(pm, 1), torch.clamp(torch.stack(pv, 1), *CLIP)
    return dict(w=w, Si=Si, Ki=Ki, p_m=p_m, p_v=p_v, z=p_m + p["eps"] * torch.sqrt(p_v))


@functools.lru_cache(maxsize=None)
def stage_reference(case):
    return stage_outputs(case)


def stage_one_ulp(case):
    """The case's inputs with every real value moved by one ulp up or down (action ids stay integers)."""
    p = stage_problem(case)
    g = torch.Generator().manual_seed(17)
    ulp = lambda t: t * (1.0 + 2.0 ** -52 * (torch.randint(0, 2, t.shape, generator=g).to(DT) * 2 - 1))
    p2 = {k: ulp(v) for k, v in p.items() if k != "eps"}
    p2["eps"] = p["eps"]
    for k in ("aux", "qaux"):
        p2[k][:, 0] = p[k][:, 0]
    return p2


# ---------------------------------------------------------------------------------------------- the test-character pipeline
@functools.lru_cache(maxsize=None)
def pipeline(K_SE):
    """The problem of test_sprites_test_character_pipeline (6 characters x 8 train frames, L = 6, a test batch of 2 characters x 8
    actions with 3 context frames each) and the oracle's answers, as a namespace-like dict; CPU float64, never modified."""
    g = torch.Generator().manual_seed(5 + int(K_SE))
    L, La, Lc, n_act = 6, LA, LC, N_ACT
    m = 20 if K_SE else 12
    n_char, fpc = 6, 8
    n_train = n_char * fpc
    params = {k: torch.tensor(v, dtype=DT) for k, v in SO.glorot_init(L, Lc, 3).items()}
    for k in params:
        if k.endswith("_b"):
            params[k] = 0.05 * torch.randn(*params[k].shape, dtype=DT, generator=g)
    gp = dict(inducing_index_points=torch.randn(m, La + Lc, dtype=DT, generator=g) * 1.5,
              GPLVM_action=torch.randn(n_act, La, dtype=DT, generator=g) * 1.5,
              l_action=torch.tensor(5.0, dtype=DT), sigma_action=torch.tensor(1.4, dtype=DT),
              l_character=torch.tensor(7.0, dtype=DT), sigma_character=torch.tensor(1.2, dtype=DT))
    frames = torch.rand(n_train, 64, 64, 3, dtype=DT, generator=g)
    ids = torch.randint(0, n_act, (n_train,), generator=g)
    seg, rep = SO.aux_data_sprites_utils(n_train, fpc, fpc)
    osvgp = SO.SpritesSVGP(gp["inducing_index_points"], gp["GPLVM_action"], 0.01, float(n_train), La,
                           K_obj_normalize=not K_SE, K_SE=K_SE,
                           se_params={k: gp[k] for k in ("l_action", "sigma_action", "l_character", "sigma_character")})
    mu_o, var_o = SO.SpritesVAE(params, L).encode(frames)
    var_o = O.clip_by_value(var_o, 1e-3, 10.0)
    aux_o = SO.aux_data_SVGPVAE_sprites((frames, ids), params, seg, rep)
    mt_o, inv_o = SO.precompute_GP_params_SVGPVAE(mu_o, var_o, aux_o, osvgp)
    Kmm_inv = torch.linalg.inv(osvgp.kernel_matrix(gp["inducing_index_points"], gp["inducing_index_points"]))
    bt, N_actions, N_context = 16, 8, 3
    test_frames = torch.rand(bt, 64, 64, 3, dtype=DT, generator=g)
    test_ids = torch.randint(0, n_act, (bt,), generator=g)
    cseg, crep = SO.aux_data_sprites_utils(int(bt * N_context / N_actions), N_context, N_actions - N_context)
    n_target = bt - int(bt * N_context / N_actions)
    eps = torch.randn(n_target, L, dtype=DT, generator=g)
    rec_o, tgt_o, loss_o, pm_o, pv_o, auxt_o = SO.predict_SVGPVAE_sprites_test_character(
        (test_frames, test_ids), params, osvgp, mt_o, inv_o, N_context, N_actions, bt, cseg, crep, Kmm_inv, eps, L)
    return dict(K_SE=K_SE, L=L, La=La, Lc=Lc, n_act=n_act, m=m, fpc=fpc, n_train=n_train, params=params, gp=gp, frames=frames,
                ids=ids, osvgp=osvgp, mt_o=mt_o, inv_o=inv_o, Kmm_inv=Kmm_inv, bt=bt, N_actions=N_actions, N_context=N_context,
                test_frames=test_frames, test_ids=test_ids, cseg=cseg, crep=crep, eps=eps, rec_o=rec_o, pm_o=pm_o, pv_o=pv_o,
                rec_mean_o=SO.SpritesVAE(params, L).decode(pm_o))


def pipeline_single(K_SE, T=4):
    """One character, ONE context frame, T target actions (not the train segment length): the oracle's (frames, p_m, p_v) with
    the posterior mean decoded, and the inputs (context frames (1, 1, ...), actions (1, T))."""
    P = pipeline(K_SE)
    ctx = P["test_frames"][8:9]
    acts = P["test_ids"][9:9 + T]
    aux_t = SO.aux_data_SVGPVAE_sprites((ctx, acts), P["params"], [0], [T])
    pm, pv = zip(*(SO.approximate_posterior_params_precomputed(P["osvgp"], aux_t, P["mt_o"][l], P["inv_o"][l], P["Kmm_inv"])
                   for l in range(P["L"])))
    p_m, p_v = torch.stack(pm, 1), torch.clamp(torch.stack(pv, 1), *CLIP)
    return ctx[None], acts[None], SO.SpritesVAE(P["params"], P["L"]).decode(p_m), p_m, p_v
