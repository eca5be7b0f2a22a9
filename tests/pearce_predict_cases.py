"""Cases, problems and the float64 restatement of the exact-GP moving-ball predictor tests (tests/test_pearce_predict_cpu.py,
tests/test_gpu_pearce_predict.py).

The restatement is the oracle's build_1d_gp (oracle/pearce_vae_oracle.py; the reference's Cholesky formulation,
GPVAE_Pearce_model.py:8-86) applied per video and latent coordinate to the frames the mask keeps, with X_test = the query times; a
video without a kept frame gives the prior (0, 1, 0); z = p_m + eps sqrt(max(p_v, 0)).  `masked_inverse` is a second float64
formulation of the same algebra, the one the long entry implements: the explicit inverse of the full-size matrix whose rows and
columns of dropped frames are those of the identity.

Bar: TOL = 1e-10 relative to the tensor's max-abs (ball_predict_cases.relerr).  With these inputs cond(A) is a few hundred; the two
float64 formulations differ by a few 1e-15 and a one-ulp change of var moves p_m by about as much, so the bar leaves four decades
for the Gauss-Jordan sweep and another summation order.  test_pearce_predict_cpu.py asserts <= TOL / 100 for both, for every case."""
import functools

import numpy as np

from tests.ball_predict_cases import relerr  # noqa: F401  (re-exported: the tests take it from here)

TOL = 1e-10
FUSED_T_MAX = 64
NB, QC = 8, 512                      # videos / query rows of a chunk of the long entry

# (B, T, Q).  One of everything; two frames; an odd small size; 32 / 33: the edge between the LDS kernel's two instances; 64, the
# last LDS shape, with more query times than one round of waves and with more than one slice's worth; the reference batch at twice
# its frame rate.  Long entry only: 65, 130 (more than one 64-wide tile), 300, and NB + 1 videos: a second chunk.
FUSED_CASES = [(1, 1, 1), (2, 2, 3), (3, 5, 4), (2, 32, 5), (2, 33, 5), (2, 64, 70), (3, 64, 300), (35, 30, 59)]
LONG_ONLY_CASES = [(2, 65, 5), (2, 130, 7), (1, 300, 4), (NB + 1, 65, 3)]
KERNEL_CASES = FUSED_CASES + LONG_ONLY_CASES
KERNEL_IDS = ["-".join(str(v) for v in c) for c in KERNEL_CASES]
FUSED_IDS = KERNEL_IDS[:len(FUSED_CASES)]
LS8_CASE = "2-33-5"                  # the one case with length scale 8


def kernel_shape(case):
    return tuple(int(v) for v in case.split("-"))


def entries(case):
    """long_form flags of the entries that take the case."""
    return [False, True] if kernel_shape(case)[1] <= FUSED_T_MAX else [True]


@functools.lru_cache(maxsize=None)
def kernel_problem(case):
    """dict of float64 numpy arrays in the kernels' layout, never modified: times (T), tq (Q), ls (2), y, s2 (2, T, B), mask (T, B),
    eps (2, Q, B).  Where B allows, video 1 has every frame dropped and video 2 keeps a single frame."""
    B, T, Q = kernel_shape(case)
    rs = np.random.RandomState(4000 + 13 * B + 7 * T + Q)
    times = np.arange(1, T + 1, dtype=np.float64)
    y = rs.randn(2, T, B)
    s2 = rs.uniform(0.01, 1.0, (2, T, B))
    keep = rs.uniform(0.5, 0.7, B)                         # per video, drawn independently
    mask = (rs.rand(T, B) < keep[None, :]).astype(np.float64)
    mask[rs.randint(T), 0] = 1.0                           # video 0 keeps at least one frame
    if B > 1:
        mask[:, 1] = 0.0
    if B > 2:
        mask[:, 2] = 0.0
        mask[rs.randint(T), 2] = 1.0
    tq = rs.uniform(-2.0, T + 3.0, Q)
    tq[Q // 2] = times[T // 2]                             # one exact frame time
    l = 8.0 if case == LS8_CASE else 2.0
    return dict(times=times, tq=tq, ls=np.array([l, l]), y=y, s2=s2, mask=mask, eps=rs.randn(2, Q, B))


def posterior(times, y, s2, mask, ls, tau, eps=None):
    """One video, one coordinate: (p_m, p_v, z, lh) at the query times tau by the oracle's build_1d_gp on the kept frames."""
    import torch

    from oracle import pearce_vae_oracle as PO
    keep = np.ones(times.size, bool) if mask is None else mask != 0
    if not keep.any():
        p_m, p_v, lh = np.zeros(tau.size), np.ones(tau.size), 0.0
    else:
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)[None]
        pm, pv, l = PO.build_1d_gp(t(times[keep]), t(y[keep]), t(s2[keep]), t(tau), float(ls))
        p_m, p_v, lh = pm[0].numpy(), pv[0].numpy(), float(l[0])
    return p_m, p_v, (p_m if eps is None else p_m + eps * np.sqrt(np.maximum(p_v, 0.0))), lh


def masked_inverse(times, y, s2, mask, ls, tau, eps=None):
    """The same four quantities from the explicit inverse of the masked full-size matrix; y and s2 of dropped frames are not read."""
    keep = np.ones(times.size, bool) if mask is None else mask != 0
    se = lambda a, b: np.exp(-(a[:, None] - b[None, :]) ** 2 / (2.0 * ls * ls))
    A = np.where(keep[:, None] & keep[None, :], se(times, times), 0.0)
    ym, sm = np.where(keep, y, 0.0), np.where(keep, s2, 0.0)
    A[np.diag_indices_from(A)] = 1.0 + sm
    Ai = np.linalg.inv(A)
    alpha = Ai @ ym
    k = np.where(keep[None, :], se(tau, times), 0.0)
    p_m, p_v = k @ alpha, 1.0 - np.einsum("qi,ij,qj->q", k, Ai, k)
    n = int(keep.sum())
    lh = -0.5 * (n * np.log(2 * np.pi) + ym @ alpha + np.linalg.slogdet(A)[1]) if n else 0.0
    return p_m, p_v, (p_m if eps is None else p_m + eps * np.sqrt(np.maximum(p_v, 0.0))), lh


def reference_of(prob, use_mask=True, use_eps=True, tq=None, form=posterior):
    """dict(p_m, p_v, z (2, Q, B), lh (2, B)) of a problem dict."""
    tq = prob["tq"] if tq is None else tq
    B = prob["y"].shape[2]
    out = dict(p_m=np.zeros((2, tq.size, B)), p_v=np.zeros((2, tq.size, B)), z=np.zeros((2, tq.size, B)), lh=np.zeros((2, B)))
    for c in range(2):
        for b in range(B):
            r = form(prob["times"], prob["y"][c, :, b], prob["s2"][c, :, b], prob["mask"][:, b] if use_mask else None,
                     prob["ls"][c], tq, prob["eps"][c, :, b] if use_eps else None)
            out["p_m"][c, :, b], out["p_v"][c, :, b], out["z"][c, :, b], out["lh"][c, b] = r
    return out


@functools.lru_cache(maxsize=None)
def kernel_reference(case):
    """Computed once per process and shared: callers must not write to it."""
    return reference_of(kernel_problem(case))


def one_ulp_var(prob, seed=23):
    """The problem with every var moved by one ulp up or down."""
    rs = np.random.RandomState(seed)
    return dict(prob, s2=prob["s2"] * (1.0 + 2.0 ** -52 * (rs.randint(0, 2, prob["s2"].shape) * 2 - 1)))


def condition_number(prob):
    """The largest cond(A) over the videos and coordinates of a problem."""
    worst = 1.0
    for c in range(2):
        for b in range(prob["y"].shape[2]):
            keep = prob["mask"][:, b] != 0
            if keep.any():
                t = prob["times"][keep]
                A = np.exp(-(t[:, None] - t[None, :]) ** 2 / (2.0 * prob["ls"][c] ** 2)) + np.diag(prob["s2"][c, keep, b])
                worst = max(worst, float(np.linalg.cond(A)))
    return worst


# ---------------------------------------------------------------------------------------------- the long entry's plan, as specified
def expected_route(B, T, Q, long_form):
    if not long_form:
        return ["k_pearce_predict"]
    names = []
    for _ in range(0, B, NB):
        names += ["k_pp_build", "svgp_spd_inverse_batched", "k_pp_alpha", "k_pp_lh"]
        for _ in range(0, Q, QC):
            names += ["k_pp_kq", "svgp_dgemm_batched", "k_pp_finish"]
    return names


# ---------------------------------------------------------------------------------------------- the predictor's problems
def predictor_problem(B, T, Q, px=8, hidden=16, seed=0, drop_video=None):
    """(params of float64 torch tensors with l_x = 2, l_y = 2.3, videos (B, T, px, px), observed (B, T) bool, query times (Q),
    eps (B, Q, 2))."""
    from tests import ball_cases as BC
    p, vid, _ = BC._problem(B, T, px, hidden, 1, seed=seed, lt=2.0)
    p = {k: v for k, v in p.items() if not k.startswith("ip_")}
    rs = np.random.RandomState(500 + seed)
    observed = rs.rand(B, T) < rs.uniform(0.5, 0.7, (B, 1))
    observed[:, 0] = True
    if drop_video is not None:
        observed[drop_video, :] = False
    return p, vid, observed, rs.uniform(-2.0, T + 3.0, Q), rs.randn(B, Q, 2)


def predictor_reference(p, vid, observed, tq, eps, frame_times=None):
    """The oracle's MLP forward (no clamp of the encoder's variances, as the exact-GP engines) composed with the restatement:
    dict(frames (B, Q, px, py), p_m, p_v, z (B, Q, 2), lh (B, 2)) as numpy."""
    import torch

    from oracle import pearce_vae_oracle as PO
    B, T, px, py = vid.shape
    mu, var = PO.mlp_inference(p, vid)
    times = np.arange(1, T + 1, dtype=np.float64) if frame_times is None else np.asarray(frame_times, dtype=np.float64)
    tr = lambda t: np.ascontiguousarray(t.numpy().transpose(2, 1, 0))          # (B, T, 2) -> (2, T, B)
    prob = dict(times=times, tq=np.asarray(tq, dtype=np.float64), ls=np.array([float(p["l_x"]), float(p["l_y"])]), y=tr(mu), s2=tr(var),
                mask=np.ones((T, B)) if observed is None else np.asarray(observed, dtype=np.float64).T,
                eps=None if eps is None else np.ascontiguousarray(np.asarray(eps).transpose(2, 1, 0)))
    r = reference_of(prob, use_eps=eps is not None)
    bq2 = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))                   # (2, Q, B) -> (B, Q, 2)
    frames = torch.sigmoid(PO.mlp_decoder(p, torch.as_tensor(bq2(r["z"])), px, py)).numpy()
    return dict(frames=frames, p_m=bq2(r["p_m"]), p_v=bq2(r["p_v"]), z=bq2(r["z"]), lh=np.ascontiguousarray(r["lh"].T))
