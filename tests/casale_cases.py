"""Casale GP-VAE: float64 CPU restatement of the reference (GPVAE_Casale_model.py, MNIST_experiment.py:786-1110), the case
table and the problem / engine builders of the Casale tests.  Test infrastructure only.

Two formulations of the GP prior term:
  literal   : the reference's N x N K_inv, a (L,N), B (L,N,H), c (L) as written (taylor_coeff :311-351, forward_pass_Casale
              :134-142), V as kron(object vectors, chol(K_W)) with the boolean mask (:278-309);
  efficient : the H x H form of include/svgpvae_hip.h, V row-wise.
Gradients come from autograd.

Bars (tests/helpers.relerr: relative to the tensor's max-abs), as in tests/ball_cases.py and tests/test_gpu_ref_model.py:
scalars 1e-9, row and matrix quantities 1e-8, gradients 1e-7, trajectory ELBO rtol and parameters 1e-8.
"""
import math

import numpy as np
import torch

from oracle import svgpvae_oracle as O

DT = torch.float64
SCALAR_TOL, FWD_TOL, GRAD_TOL, TRAJ_TOL = 1e-9, 1e-8, 1e-7, 1e-8
REAL_ANGLES = np.array([k * 2 * math.pi / 16 for k in range(16) if k != 7])
GP_NAMES = ("l_GP", "amplitude", "alpha", "object_vectors")
LR = dict(joint=0.001, GP=0.01, VAE=0.001)

#            P   angles                M  L   normalize  batches (lo, hi; hi None = N)      l_GP
CASES = dict(
    A=dict(P=6, Q=5, M=3, L=3, normalize=False, batches=((4, 12), (16, None)), l_GP=0.8, seed=11),
    B=dict(P=12, Q=15, M=5, L=16, normalize=True, batches=((40, 72),), l_GP=1.0, seed=12),
    C=dict(P=40, Q=15, M=8, L=16, normalize=False, batches=((100, 164),), l_GP=1.0, seed=13),
)


# The shapes at which casale.hip and the library routines under it change form (check_cfg: 1 <= Q <= 32, 1 <= M <= 128,
# H = M Q <= 2048, 1 <= L <= 64, any N).  keep: kept share of the (object, angle) pairs (1.0: all pairs, no single-row object);
# edges: whether table rows 0 and n_obj - 1 occur in the data; norm: also run with the normalised object kernel.
ENVELOPE_CASES = dict(
    # H = Q = M = 1: every GEMM degenerate, a 1 x 1 Cholesky.  Raw only: ov / |ov| is +-1, its gradient identically 0
    H1=dict(P=7, Q=1, M=1, L=2, l_GP=0.8, seed=31, edges=False),
    # Q = 1: the trailing updates of k_kw_chol and both triangular solves of k_chol_bwd are empty
    Q1=dict(P=9, Q=1, M=4, L=3, l_GP=0.8, seed=32, edges=True),
    # Q = 32: the [32][33] LDS tiles are full, solves on 32 threads; H = 64 is one GEMM tile
    Q32=dict(P=4, Q=32, M=2, L=2, l_GP=0.3, seed=33, edges=False, norm=True),
    # M = 128: every thread of k_ov_bwd, both waves of its normalised reduction; N < H = 384
    M128=dict(P=5, Q=3, M=128, L=2, l_GP=0.8, seed=34, edges=True, norm=True),
    # H = 511 / 512 / 513: last size of the inverse's 32-block sweep, first two of potrf + potri; N < 256: no split-K
    H511=dict(P=30, Q=7, M=73, L=3, l_GP=0.8, seed=35, edges=False),
    H512=dict(P=30, Q=8, M=64, L=3, l_GP=0.8, seed=36, edges=True),
    H513=dict(P=12, Q=19, M=27, L=3, l_GP=0.5, seed=37, edges=False, norm=True),
    # N >= 256 with 64 output tiles: V^T V and V^T Z both take the split-K path with scratch
    H512_N=dict(P=120, Q=8, M=64, L=3, l_GP=0.8, seed=38, edges=True),
    # H = 1024, N >= 256: 256 tiles, V^T V no longer splits, V^T Z (H x L) still does; the scratch is the larger of the two
    H1024=dict(P=12, Q=32, M=32, L=3, l_GP=0.3, seed=39, edges=False, keep=0.85),
    # both limits at once: H = 2048, L = 64, N < H
    H2048_L64=dict(P=3, Q=32, M=64, L=64, l_GP=0.3, seed=40, edges=True, keep=0.9),
    # L = 64 / L = 1: every lane / one lane of the row kernels' waves, the whole / one entry of a cms row
    L64=dict(P=6, Q=5, M=3, L=64, l_GP=0.8, seed=41, edges=False),
    L1=dict(P=6, Q=5, M=3, L=1, l_GP=0.8, seed=42, edges=True),
    # N = 64 / 65: one full chunk of k_lw_part / one row in a second chunk; N % 4 = 0 / 1 (three dead waves that still pass
    # the __syncthreads() of k_rows_bwd); L = 17 is no divisor of 64
    N64=dict(P=16, Q=4, M=3, L=17, l_GP=0.8, seed=43, edges=False, keep=1.0),
    N65=dict(P=13, Q=5, M=3, L=17, l_GP=0.8, seed=44, edges=True, keep=1.0, norm=True),
)


def t64(x):
    return torch.as_tensor(np.asarray(x), dtype=DT)


def envelope_variants():
    """(name, normalize) of every run of the envelope table: raw everywhere, normalised where the entry asks for it."""
    return [(n, nz) for n, c in ENVELOPE_CASES.items() for nz in ((False, True) if c.get("norm") else (False,))]


def make_envelope_case(name, normalize=False):
    """Seeded GP-stage problem of ENVELOPE_CASES, same fields as make_case.
    Angles: k 2 pi / Q moved by at most +-20 % of the spacing (uniformly random angles at Q = 32 give cond(K_W) ~ 4e9).
    Mask: ~keep of the pairs, at least one row per object and per angle (Q and P do not shrink); unless keep is 1, one object
    (first, last or a middle one) has a single row.  Object table of P + 3 rows, three of them unused: with edges False rows 0
    and n_obj - 1 are among the unused ones, with edges True both occur.  Object vectors randn 1.5 / sqrt(M): cond(alpha I + G)
    stays ~1e2 at M >= 64.  Batches on one workspace (b_cap = N), in this order: the whole set, the last row alone, a ragged
    middle range."""
    c = dict(ENVELOPE_CASES[name])
    rng = np.random.RandomState(c["seed"])
    P, Q, M, L, keep = c["P"], c["Q"], c["M"], c["L"], c.get("keep", 0.75)
    angles = (np.arange(Q) + rng.uniform(-0.2, 0.2, Q)) * (2 * math.pi / Q)
    assert np.all(np.diff(angles) > 0)
    mask = rng.rand(P, Q) < keep
    single = None
    if keep < 1.0:
        single = (0, P - 1, P // 2)[c["seed"] % 3]
        mask[single] = False
        mask[single, rng.randint(Q)] = True
    for p in range(P):
        if not mask[p].any():
            mask[p, rng.randint(Q)] = True
    for q in range(Q):
        if not mask[:, q].any():
            mask[rng.choice([p for p in range(P) if p != single] or [0]), q] = True
    n_obj = P + 3
    if c["edges"]:
        ids = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n_obj - 1), P - 2, replace=False)), [n_obj - 1]])
    else:
        ids = np.sort(rng.choice(np.arange(1, n_obj - 1), P, replace=False))
    jj, rr = np.nonzero(mask)
    N = len(jj)
    aux = np.stack([np.arange(N, dtype=np.float64), ids[jj].astype(np.float64), angles[rr]], 1)
    lo = max(1, N // 3)
    mid = (lo, min(N - 1, lo + max(1, (2 * N) // 5) + 1))
    c.update(name=name, N=N, H=M * Q, n_obj=n_obj, angles=angles, mask=mask.reshape(-1), aux=aux, normalize=bool(normalize),
             ids=ids, unused=np.setdiff1d(np.arange(n_obj), ids), single=None if single is None else int(ids[single]),
             object_vectors=rng.randn(n_obj, M) * 1.5 / math.sqrt(M), amplitude=0.9, alpha=0.15, Z=rng.randn(N, L),
             batches=((0, N), (N - 1, N), mid))
    c["zb"] = {b: rng.randn(b[1] - b[0], L) for b in c["batches"]}
    return c


def make_case(name, normalize=None):
    """Seeded problem of the GP stage: a mask that keeps ~75 % of the (object, angle) pairs with at least one angle per
    object, sorted aux rows [global id, object id, angle], an object table with two unused rows, Z and the batch samples."""
    c = dict(CASES[name])
    rng = np.random.RandomState(c["seed"])
    P, Q, M, L = c["P"], c["Q"], c["M"], c["L"]
    angles = REAL_ANGLES.copy() if Q == 15 else np.sort(rng.uniform(0.0, 2 * math.pi, Q))
    mask = rng.rand(P, Q) < 0.75
    for p in range(P):
        if not mask[p].any():
            mask[p, rng.randint(Q)] = True
    n_obj = P + 2
    ids = np.sort(rng.choice(n_obj, P, replace=False))             # object ids: not all table rows occur
    jj, rr = np.nonzero(mask)
    N = len(jj)
    aux = np.stack([np.arange(N, dtype=np.float64), ids[jj].astype(np.float64), angles[rr]], 1)
    c.update(name=name, N=N, H=M * Q, n_obj=n_obj, angles=angles, mask=mask.reshape(-1), aux=aux,
             normalize=c["normalize"] if normalize is None else normalize,
             object_vectors=rng.randn(n_obj, M) * 1.5, amplitude=0.9, alpha=0.15,
             Z=rng.randn(N, L), batches=tuple((lo, N if hi is None else hi) for lo, hi in c["batches"]))
    c["zb"] = {b: rng.randn(b[1] - b[0], L) for b in c["batches"]}
    return c


# ------------------------------------------------------------------------------------------------------------ V
def K_W_of(angles, l_GP, amplitude):
    a = t64(angles)
    return O.exp_sin_squared(a, a, amplitude, l_GP)


def _normalised(ov, normalize):
    return ov / torch.linalg.norm(ov, dim=1, keepdim=True) if normalize else ov


def V_literal(ov_table, aux, mask, l_GP, amplitude, normalize):
    """casaleGP.V_matrix (:278-309): kron(object vectors of the sorted unique ids, chol(K_W)), rows selected by the mask."""
    rows = np.asarray(aux)[:, 1:]
    ids = np.sort(np.unique(rows[:, 0])).astype(np.int64)
    angles = np.sort(np.unique(rows[:, 1]))
    ov = _normalised(ov_table[torch.as_tensor(ids)], normalize)
    L_W = torch.linalg.cholesky(K_W_of(angles, l_GP, amplitude))
    kron = (ov.reshape(ov.shape[0], 1, ov.shape[1], 1) * L_W.reshape(1, L_W.shape[0], 1, L_W.shape[1])).reshape(
        ov.shape[0] * L_W.shape[0], ov.shape[1] * L_W.shape[1])
    return kron[torch.as_tensor(np.asarray(mask, dtype=bool))]


def V_rowwise(ov_table, aux, l_GP, amplitude, normalize):
    """V[i, k Q + r] = ov[p_i, k] L_W[q_i, r]."""
    rows = np.asarray(aux)[:, 1:]
    angles = np.sort(np.unique(rows[:, 1]))
    p = torch.as_tensor(rows[:, 0].astype(np.int64))
    q = torch.as_tensor(np.searchsorted(angles, rows[:, 1]))
    L_W = torch.linalg.cholesky(K_W_of(angles, l_GP, amplitude))
    ov = _normalised(ov_table, normalize)[p]
    return (ov[:, :, None] * L_W[q][:, None, :]).reshape(len(p), -1)


# ------------------------------------------------------------------------------------------------------------ GP prior term
def taylor_coeff_literal(Z, V, alpha):
    """casaleGP.taylor_coeff (:311-351) as written: N x N K_inv, a (L,N), B (L,N,H), c (L)."""
    N, H = V.shape
    inside_inv = torch.linalg.inv(alpha * torch.eye(H, dtype=DT) + V.T @ V)
    K_inv = (1 / alpha) * torch.eye(N, dtype=DT) - (1 / alpha) * (V @ (inside_inv @ V.T))
    a = Z.T @ K_inv
    K_inv_V = K_inv @ V
    B, c = [], []
    for l in range(Z.shape[1]):
        z = Z[:, l:l + 1]
        B.append(-K_inv @ (z @ (z.T @ K_inv_V)) + K_inv_V)
        c.append(0.5 * (-(z.T @ (K_inv @ (K_inv @ z))).reshape(()) + torch.trace(K_inv)))
    return a, torch.stack(B, 0), torch.stack(c)


def gp_prior_literal(Z, zb, V, alpha, lo, hi):
    """forward_pass_Casale :134-142 on the literal coefficients."""
    a, B, c = taylor_coeff_literal(Z, V, alpha)
    idx = torch.arange(lo, hi)
    a_b, B_b, V_b = a.T[idx], B.permute(1, 2, 0)[idx], V[idx]
    B_terms = sum(torch.sum(B_b[:, :, l] * V_b) for l in range(Z.shape[1]))
    return torch.sum(zb * a_b) + B_terms + torch.sum(c) * alpha


def gp_prior_efficient(Z, zb, V, alpha, lo, hi, want=False):
    N, H = V.shape
    L = Z.shape[1]
    G = V.T @ V
    P = torch.linalg.inv(alpha * torch.eye(H, dtype=DT) + G)
    W = V.T @ Z
    U = P @ W
    A = (Z - V @ U) / alpha
    trKinv = (N - H) / alpha + torch.trace(P)
    Vb, Ab = V[lo:hi], A[lo:hi]
    t1, t2, t3 = torch.sum(zb * Ab), -torch.sum(Ab * (Vb @ U)), L * torch.sum((Vb @ P) * Vb)
    term = t1 + t2 + t3 + (alpha / 2) * (-torch.sum(A * A) + L * trKinv)
    if want:
        return term, dict(G=G, P=P, W=W, U=U, A=A, terms=torch.stack([t1, t2, t3]))
    return term


def gp_stage_reference(case, batch, train_gp=True, train_ov=True, formulation="efficient", seed=1.0):
    """Every quantity GPU test 1 compares, with autograd gradients of seed * GP_prior_term."""
    lo, hi = batch
    leaf = lambda v: t64(v).clone().requires_grad_(True)
    l_GP, amp, alpha, ov = leaf(case["l_GP"]), leaf(case["amplitude"]), leaf(case["alpha"]), leaf(case["object_vectors"])
    Z, zb = leaf(case["Z"]), leaf(case["zb"][batch])
    if formulation == "literal":
        V = V_literal(ov, case["aux"], case["mask"], l_GP, amp, case["normalize"])
        term, inter = gp_prior_literal(Z, zb, V, alpha, lo, hi), {}
    else:
        V = V_rowwise(ov, case["aux"], l_GP, amp, case["normalize"])
        term, inter = gp_prior_efficient(Z, zb, V, alpha, lo, hi, want=True)
    gZ, gzb, gl, ga, gal, gov = torch.autograd.grad(seed * term, [Z, zb, l_GP, amp, alpha, ov])
    zero = torch.zeros((), dtype=DT)
    out = dict(V=V.detach(), GP_prior_term=term.detach(), Zbar=gZ, zbbar=gzb,
               l_GP=gl if train_gp else zero, amplitude=ga if train_gp else zero, alpha=gal if train_gp else zero,
               object_vectors=gov if train_ov else torch.zeros_like(gov))
    K_W = K_W_of(case["angles"], l_GP, amp).detach()
    out.update(K_W=K_W, L_W=torch.linalg.cholesky(K_W), **{k: v.detach() for k, v in inter.items()})
    return out


# ------------------------------------------------------------------------------------------------------------ the step
def elbo_casale(p, images, aux, lo, hi, eps_f, eps_b, *, beta, clip, normalize, L, formulation="efficient", mask=None):
    """forward_pass_Casale (:96-155) on top of encode (:69-93) over the whole train set; p: dict of tensors."""
    vae = O.MnistVAE(p, L)
    mu_all, var_all = vae.encode(images)
    Z = mu_all + eps_f * torch.sqrt(O.clip_by_value(var_all, 1e-3, 10.0) if clip else var_all)
    if formulation == "literal":
        V = V_literal(p["object_vectors"], aux, mask, p["l_GP"], p["amplitude"], normalize)
    else:
        V = V_rowwise(p["object_vectors"], aux, p["l_GP"], p["amplitude"], normalize)
    mu, var = vae.encode(images[lo:hi])
    if clip:
        var = O.clip_by_value(var, 1e-3, 100.0)
    log_var = torch.sum(torch.log(var))
    zb = mu + eps_b * torch.sqrt(var)
    gp = (gp_prior_literal if formulation == "literal" else gp_prior_efficient)(Z, zb, V, p["alpha"], lo, hi)
    recon = vae.decode(zb)
    sq = torch.sum((images[lo:hi] - recon) ** 2)
    elbo = sq / 784.0 - (beta / L) * (gp + 0.5 * log_var)
    return elbo, dict(elbo=elbo, recon_loss=sq / 784.0, GP_prior_term=gp, log_var=log_var, qnet_mu=mu, qnet_var=var,
                      recon=recon, var_all=var_all)


def elbo_vae(p, images_b, eps_b, *, L):
    """forward_pass_standard_VAE_rotated_mnist (SVGPVAE_model.py:718-782), sigma 0.01, no clipping; returns -elbo_VAE."""
    vae = O.MnistVAE(p, L)
    mu, var = vae.encode(images_b)
    recon = vae.decode(mu + eps_b * torch.sqrt(var))
    sq = torch.sum((images_b - recon) ** 2)
    KL = O.KL_term_standard_normal_prior(mu, var)
    elbo = -(0.5 / 0.01 ** 2) * sq - KL
    return -elbo, dict(elbo=elbo, recon_loss=sq / 784.0, KL_term=KL, qnet_mu=mu, qnet_var=var, recon=recon)


def regime_variables(regime, ov_joint, fixed_gp=False):
    vae = [n for n, _ in O.mnist_vae_param_shapes(1)]
    gp = ([] if fixed_gp else ["l_GP", "amplitude", "alpha"]) + (["object_vectors"] if ov_joint else [])
    return dict(VAE=vae, GP=gp, joint=vae + gp)[regime]


def step_reference(regime, params, images, aux, lo, hi, eps_f, eps_b, *, beta, clip, normalize, L, ov_joint, **kw):
    """(scalars / tensors dict, gradients of the regime's objective; zero for variables outside its list)."""
    p = {k: t64(v).clone().requires_grad_(True) for k, v in params.items()}
    if regime == "VAE":
        obj, out = elbo_vae(p, images[lo:hi], eps_b, L=L)
    else:
        obj, out = elbo_casale(p, images, aux, lo, hi, eps_f, eps_b, beta=beta, clip=clip, normalize=normalize, L=L, **kw)
    names = regime_variables(regime, ov_joint)
    g = torch.autograd.grad(obj, [p[k] for k in names], allow_unused=True)
    grads = {k: torch.zeros_like(v) for k, v in p.items()}
    grads.update({k: (torch.zeros_like(p[k]) if gi is None else gi) for k, gi in zip(names, g)})
    return {k: v.detach() for k, v in out.items()}, grads


def train_trajectory(params, images, aux, schedule, *, beta, clip, normalize, L, ov_joint):
    """schedule: list of (regime, lo, hi, eps_f, eps_b).  One TF1 Adam state and one step count for all regimes; variables
    outside a regime's list keep their moments (MNIST_experiment.py:891-906, 987-1011)."""
    p = {k: t64(v).clone() for k, v in params.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(x) for k, x in p.items()}
    elbos = []
    for t, (regime, lo, hi, eps_f, eps_b) in enumerate(schedule, start=1):
        out, g = step_reference(regime, p, images, aux, lo, hi, eps_f, eps_b, beta=beta, clip=clip, normalize=normalize,
                                L=L, ov_joint=ov_joint)
        elbos.append(float(out["elbo"]))
        names = regime_variables(regime, ov_joint)
        O.adam_tf1_step({k: p[k] for k in names}, g, m, v, t, LR[regime])
    return p, elbos, m, v


# ------------------------------------------------------------------------------------------------------------ prediction
def kernel_matrix_ref(x, y, ov_table, l_GP, amplitude, normalize, ov_joint):
    """casaleGP.kernel_matrix (:249-276); rows [id, angle, o..]."""
    xo = ov_table[x[:, 0].long()] if ov_joint else x[:, 2:]
    yo = ov_table[y[:, 0].long()] if ov_joint else y[:, 2:]
    return O.exp_sin_squared(x[:, 1], y[:, 1], amplitude, l_GP) * O.linear_kernel(xo, yo, normalize)


def predict_reference(test_images, test_aux, train_aux, p, V, Z, *, L, normalize, ov_joint, take_mean, epsilon=None):
    """predict_test_set_Casale (:158-203), literal N x N form, including its tile / reshape of the T variances to (T, L)
    (:194): row i, channel l gets var[(i L + l) mod T], not var[i]."""
    N, H = V.shape
    alpha = p["alpha"]
    Ktn = kernel_matrix_ref(test_aux, train_aux[:, 1:], p["object_vectors"], p["l_GP"], p["amplitude"], normalize, ov_joint)
    Ktt = kernel_matrix_ref(test_aux, test_aux, p["object_vectors"], p["l_GP"], p["amplitude"], normalize, ov_joint)
    inside_inv = torch.linalg.inv(alpha * torch.eye(H, dtype=DT) + V.T @ V)
    K_inv = (1 / alpha) * torch.eye(N, dtype=DT) - (1 / alpha) * (V @ (inside_inv @ V.T))
    mean = Ktn @ (K_inv @ Z)
    z = mean
    var = None
    if not take_mean:
        var = torch.diagonal(Ktt - Ktn @ (K_inv @ Ktn.T))
        z = mean + epsilon * torch.sqrt(torch.reshape(var.repeat(L), (-1, L)))
    recon = O.MnistVAE(p, L).decode(z)
    return recon, torch.mean((test_images - recon) ** 2), mean, var


# ------------------------------------------------------------------------------------------------------------ real-image problem
def real_problem(golden_inputs, n_objects=6, n_angles=5, M=3, L=3, seed=5, keep=0.75, normalize=False):
    """A-sized step problem on real rotated-MNIST images: rows of the golden inputs of n_objects objects at n_angles
    angles, a seeded ~75 % subset of the (object, angle) pairs (all distinct), sorted by (object, angle), object ids
    remapped to table rows 0..n_objects-1 (+ one unused row)."""
    rng = np.random.RandomState(seed)
    aux, images = golden_inputs["aux"], golden_inputs["images"]
    ids = np.sort(np.unique(aux[:, 0]))[:n_objects]
    angles = np.sort(np.unique(aux[:, 1]))[1:2 * n_angles:2]
    rows = [i for i in range(len(aux)) if aux[i, 0] in ids and aux[i, 1] in angles and rng.rand() < keep]
    rows.sort(key=lambda i: (aux[i, 0], aux[i, 1]))
    N = len(rows)
    obj = np.searchsorted(ids, aux[rows, 0]).astype(np.float64)
    train_aux = np.stack([np.arange(N, dtype=np.float64), obj, aux[rows, 1]], 1)
    params = {k: v for k, v in O.glorot_uniform_init(L, seed).items()}
    for k in params:
        if k.endswith("_b"):
            params[k] = 0.1 * rng.randn(*params[k].shape)
    # encoder variances on both sides of every clip bound: below 1e-3, inside, between 10 and 100, above 100
    params["enc_d_b"][L:] += np.array([-7.5, 3.3, 5.5, 0.0])[np.arange(L) % 4]
    params.update(l_GP=np.array(0.8), amplitude=np.array(0.9), alpha=np.array(0.15),
                  object_vectors=rng.randn(n_objects + 1, M) * 1.5)
    return dict(N=N, L=L, M=M, normalize=normalize, params={k: t64(v) for k, v in params.items()},
                images=t64(images[rows]), aux=train_aux, eps_f=t64(rng.randn(N, L)), rng=rng)


def assert_clip_margin(var_all, lo, hi, rel=1e-6):
    """Every clipped variance stays at least `rel` (relative) away from a clip bound, so the clip masks of two
    implementations cannot differ."""
    v = var_all.detach()
    for bound, rows in ((1e-3, v), (10.0, v), (100.0, v[lo:hi])):
        assert float(((rows - bound).abs() / bound).min()) > rel, bound


# ------------------------------------------------------------------------------------------------------------ engine builders
def gp_object(case_or_prob, ov_joint=True, fixed_gp=False, normalize=None, values=None):
    from svgp_vae_amd.GPVAE_Casale_model import casaleGP
    v = values or case_or_prob
    GP = casaleGP(fixed_gp, np.asarray(v["object_vectors"]), case_or_prob["normalize"] if normalize is None else normalize,
                  ov_joint)
    GP.set_values(l_GP=float(v["l_GP"]), amplitude=float(v["amplitude"]), alpha=float(v["alpha"]))
    return GP


def step_engine(prob, *, batch_size, beta, clip, ov_joint, device="cuda:0"):
    from svgp_vae_amd.GPVAE_Casale_model import CasaleStepEngine
    from svgp_vae_amd.VAE_utils import mnistVAE
    vae = mnistVAE(L=prob["L"])
    GP = gp_object(prob, ov_joint=ov_joint, values=prob["params"])
    return CasaleStepEngine(vae, GP, prob["images"], prob["aux"], batch_size=batch_size, beta=beta, clipping_qs=clip,
                            device=device, params=prob["params"])


# ------------------------------------------------------------------------------------------------------------ reference-executed fixture
def fixture_problem(golden_inputs, normalize):
    """The problem tests/golden/make_ref_casale_fixtures.py runs the reference's own code on: case A's index structure with
    the first N golden images, a seeded VAE (L 3), one batch, seeded N(0,1) draws and 5 test rows at other angles."""
    case = make_case("A", normalize=normalize)
    N, L, M = case["N"], case["L"], case["M"]
    rng = np.random.RandomState(77)
    params = {k: v for k, v in O.glorot_uniform_init(L, 3).items()}
    for k in params:
        if k.endswith("_b"):
            params[k] = 0.1 * rng.randn(*params[k].shape)
    params["enc_d_b"][L:] += np.array([-7.5, 3.3, 5.5])
    params.update(l_GP=np.array(case["l_GP"]), amplitude=np.array(case["amplitude"]), alpha=np.array(case["alpha"]),
                  object_vectors=case["object_vectors"])
    ov = case["object_vectors"]
    aux_full = np.concatenate([case["aux"], ov[case["aux"][:, 1].astype(int)]], 1)          # [gid, id, angle, o..]
    T = 5
    ids = case["aux"][rng.randint(0, N, T), 1]
    test_aux = np.concatenate([np.stack([ids, rng.uniform(0, 6.28, T)], 1), ov[ids.astype(int)]], 1)
    return dict(case=case, N=N, L=L, M=M, params={k: t64(v) for k, v in params.items()}, images=t64(golden_inputs["images"][:N]),
                aux=aux_full, lo=4, hi=12, beta=0.7, eps_f=t64(rng.randn(N, L)), eps_b=t64(rng.randn(8, L)),
                test_aux=t64(test_aux), test_images=t64(golden_inputs["images"][100:100 + T]), eps_t=t64(rng.randn(T, L)))
