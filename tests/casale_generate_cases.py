"""Cases, query rows and float64 references of the Casale posterior cache / generation tests
(tests/test_casale_generate_cpu.py, tests/test_gpu_casale_generate.py).  Test infrastructure only.

Reference: casale_cases.predict_reference, the literal N x N form of predict_test_set_Casale (GPVAE_Casale_model.py:158-203): its
mean (T, L) and var (T) are the moments; the images are O.MnistVAE.decode(mean + eps sqrt(var[:, None])) -- row i's own variance
for all its channels (the generation deviates from the reference's tiling var[(i L + l) mod T], :194 sic, on purpose).

The cache form is restated here in numpy for the CPU guard and for the cache fields:
    L_W = chol(K_W)   V[i, k Q + r] = on[p_i, k] L_W[q_i, r]   P = (alpha I + V^T V)^-1   U = P V^T Z
    kappa_r = k_W(angle*, angle_r)   lambda = L_W^-1 kappa   v* = on* (x) lambda
    mean* = v*^T U   var* = k** - |v*|^2 + alpha v*^T P v*   k** = amplitude^2 |on*|^2

Bars: the project's casale_cases.FWD_TOL = 1e-8 with helpers.relerr for everything on the GPU; GUARD_TOL = 1e-10 for the numpy
restatement against the literal form on the CPU, 100 x under the GPU bar, so that bar measures the kernel and not the literal
form's own cancellation.  Raw C (1.3e-8: the N x N literal loses there) and raw B (1.7e-10) miss the guard and are no cases."""
import functools
import math

import numpy as np
import torch

from oracle import svgpvae_oracle as O
from tests import casale_cases as CC

DT = torch.float64
GUARD_TOL = 1e-10
COND_MAX = 1e7
N_QUERY = 9

# Two boundary shapes of the generation route, built by the recipe of casale_cases.make_envelope_case (same fields as its
# table): H256 is the last shape of the one-launch kernel with every LDS field full (Q = 32, H = 256), H258 the first split shape.
BOUNDARY_CASES = dict(
    H256=dict(P=6, Q=32, M=8, L=3, l_GP=0.3, seed=51, edges=False),
    H258=dict(P=8, Q=6, M=43, L=3, l_GP=0.8, seed=52, edges=True),
)

#         name              source      key     normalize
VARIANTS = {
    "A-raw": ("case", "A", False), "A-norm": ("case", "A", True),
    "B-norm": ("case", "B", True),                   # H = 75, L = 16
    "C-norm": ("case", "C", True),                   # P 40, Q 15 real angles, M 8, L 16, H 120, N 447: the reference's shape
    "H1": ("env", "H1", False), "Q1": ("env", "Q1", False),
    "Q32-raw": ("env", "Q32", False), "Q32-norm": ("env", "Q32", True),      # H = 64
    "L64": ("env", "L64", False), "L1": ("env", "L1", False),
    "M128": ("env", "M128", False),                  # H = 384, N = 10 < H: a shape on the split route
    "H513-norm": ("env", "H513", True),              # Q = 19
    "H256-raw": ("bnd", "H256", False), "H256-norm": ("bnd", "H256", True),
    "H258-raw": ("bnd", "H258", False), "H258-norm": ("bnd", "H258", True),
}


def _boundary_case(name, normalize):
    """casale_cases.make_envelope_case's recipe on an entry of BOUNDARY_CASES: jittered-grid angles, ~75 % of the pairs with one
    row per object and angle at least, one single-row object, a table of P + 3 rows of which three are unused."""
    c = dict(BOUNDARY_CASES[name])
    rng = np.random.RandomState(c["seed"])
    P, Q, M, L, keep = c["P"], c["Q"], c["M"], c["L"], c.get("keep", 0.75)
    angles = (np.arange(Q) + rng.uniform(-0.2, 0.2, Q)) * (2 * math.pi / Q)
    assert np.all(np.diff(angles) > 0)
    mask = rng.rand(P, Q) < keep
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
    c.update(name=name, N=N, H=M * Q, n_obj=n_obj, angles=angles, mask=mask.reshape(-1), aux=aux, normalize=bool(normalize),
             ids=ids, unused=np.setdiff1d(np.arange(n_obj), ids), object_vectors=rng.randn(n_obj, M) * 1.5 / math.sqrt(M),
             amplitude=0.9, alpha=0.15, Z=rng.randn(N, L))
    return c


@functools.lru_cache(maxsize=None)
def problem(variant):
    """dict of a variant: the GP-stage case (casale_cases' fields, not modified), decoder / encoder parameters with non-zero
    biases, the parameter dict `p` of predict_reference and the 9 query rows qaux (9, 2+M) = [id, angle, o_1..o_M] (the
    table's vector in the row, so the same rows serve gather = 1 and gather = 0) with their draws eps (9, L)."""
    src, key, normalize = VARIANTS[variant]
    case = (CC.make_case(key, normalize=normalize) if src == "case" else
            CC.make_envelope_case(key, normalize=normalize) if src == "env" else _boundary_case(key, normalize))
    L, M, n_obj = case["L"], case["M"], case["n_obj"]
    rng = np.random.RandomState(1000 + case["seed"])
    params = {k: v for k, v in O.glorot_uniform_init(L, case["seed"]).items()}
    for k in params:
        if k.endswith("_b"):
            params[k] = 0.1 * rng.randn(*params[k].shape)
    p = {k: CC.t64(v) for k, v in params.items()}
    p.update(l_GP=CC.t64(case["l_GP"]), amplitude=CC.t64(case["amplitude"]), alpha=CC.t64(case["alpha"]),
             object_vectors=CC.t64(case["object_vectors"]))
    train_ids = np.unique(case["aux"][:, 1]).astype(int)
    unused = np.setdiff1d(np.arange(n_obj), train_ids)
    assert len(unused) >= 1
    ids = rng.choice(train_ids, N_QUERY)
    ids[4] = unused[0]                                  # a table row that has no train row
    ang = rng.uniform(0.0, 2 * math.pi, N_QUERY)
    ang[0], ang[1], ang[2], ang[3] = case["angles"][0], case["angles"][-1], -0.3, 7.0      # two train angles; periodicity
    qaux = np.concatenate([np.stack([ids.astype(np.float64), ang], 1), case["object_vectors"][ids]], 1)
    return dict(variant=variant, case=case, normalize=bool(normalize), L=L, M=M, Q=case["Q"], H=case["H"], N=case["N"],
                n_obj=n_obj, p=p, qaux=CC.t64(qaux), eps=CC.t64(rng.randn(N_QUERY, L)), unused_id=int(unused[0]))


@functools.lru_cache(maxsize=None)
def reference(variant):
    """The literal oracle of a variant: mean (9, L), var (9), images with eps and images of the mean.  Computed once."""
    pr = problem(variant)
    case, p, L = pr["case"], pr["p"], pr["L"]
    V = CC.V_rowwise(p["object_vectors"], case["aux"], p["l_GP"], p["amplitude"], pr["normalize"])
    Z = CC.t64(case["Z"])
    zeros = torch.zeros(N_QUERY, 28, 28, 1, dtype=DT)
    _, _, mean, var = CC.predict_reference(zeros, pr["qaux"], CC.t64(case["aux"]), p, V, Z, L=L, normalize=pr["normalize"],
                                           ov_joint=True, take_mean=False, epsilon=pr["eps"])
    vae = O.MnistVAE(p, L)
    return dict(mean=mean, var=var, images=vae.decode(mean + pr["eps"] * torch.sqrt(var[:, None])), images_mean=vae.decode(mean))


@functools.lru_cache(maxsize=None)
def cache_form(variant):
    """The cache form in float64 numpy: dict(K_W, L_W, P, U, mean, var) (module docstring)."""
    pr = problem(variant)
    case = pr["case"]
    Q, M = pr["Q"], pr["M"]
    l_GP, amp, alpha = float(case["l_GP"]), float(case["amplitude"]), float(case["alpha"])
    ang = np.asarray(case["angles"], dtype=np.float64)
    kW = lambda x, y: amp ** 2 * np.exp(-2.0 * np.sin(0.5 * (x[:, None] - y[None, :])) ** 2 / l_GP ** 2)
    K_W = kW(ang, ang)
    L_W = np.linalg.cholesky(K_W)
    ov = np.asarray(case["object_vectors"], dtype=np.float64)
    on = ov / np.linalg.norm(ov, axis=1, keepdims=True) if pr["normalize"] else ov
    rows = case["aux"][:, 1:]
    pi, qi = rows[:, 0].astype(int), np.searchsorted(ang, rows[:, 1])
    V = (on[pi][:, :, None] * L_W[qi][:, None, :]).reshape(len(pi), M * Q)
    P = np.linalg.inv(alpha * np.eye(M * Q) + V.T @ V)
    U = P @ (V.T @ np.asarray(case["Z"], dtype=np.float64))
    q = pr["qaux"].numpy()
    oq = q[:, 2:]
    oq = oq / np.linalg.norm(oq, axis=1, keepdims=True) if pr["normalize"] else oq
    kappa = kW(q[:, 1], ang)                                              # (9, Q)
    lam = np.stack([_forward_subst(L_W, k) for k in kappa])
    v = (oq[:, :, None] * lam[:, None, :]).reshape(len(q), M * Q)
    kss = amp ** 2 * np.sum(oq * oq, 1)
    return dict(K_W=K_W, L_W=L_W, P=P, U=U, mean=v @ U, var=kss - np.sum(v * v, 1) + alpha * np.sum((v @ P) * v, 1))


def _forward_subst(Lm, b):
    x = np.zeros_like(b)
    for r in range(len(b)):
        x[r] = (b[r] - Lm[r, :r] @ x[:r]) / Lm[r, r]
    return x
