"""Cases and the float64 numpy restatement of the moving-ball joint predictor tests (tests/test_ball_joint_cpu.py,
tests/test_gpu_joint_predict.py).  Problems, the bar and its guard are those of tests/ball_predict_cases.py.

The restatement, per video and latent coordinate (include/svgpvae_hip.h, "moving ball: joint posterior over the query times"),
with X, w and k exactly those of ball_predict_cases.posterior:
    C = SE(tau, tau) + k X k^T      Lc = chol(C + jp I) lower      p_m = k w      z = p_m + Lc eps
`flip=True` evaluates the same sums with the inducing index reversed: a second summation order of the same algebra.

Bar: TOL = 1e-8 relative to the tensor's max-abs, meaningful only where the restatement's own response to a one-ulp change of its
inputs stays within TOL / 100 (test_ball_joint_cpu.py asserts it for cov and p_m, and for z and chol at jp = PATH_JITTER_DIRECT).
At the model's jitter 1e-9 the factor of C + jp I answers a one-ulp change with up to 2e-8, so z and chol are not compared with
the restatement there; the GPU test checks identities of the device's own outputs instead, with the bound below.

CHOL_C, the constant of the residual bound  |Lc Lc^T - (C + jp I)|_ij <= CHOL_C * Q * 2^-53 * max diag(C + jp I):
  * a Cholesky factorisation in floating point satisfies |A - L L^T| <= gamma_(Q+1) |L| |L|^T with gamma_k = k u / (1 - k u), u =
    2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 10.3), and (|L| |L|^T)_ij <= |l_i| |l_j| =
    sqrt(a_ii a_jj) (1 + O(Q u)) <= max diag; (Q + 1) <= 2 Q gives 2 Q u max diag;
  * the device multiplies a column by the reciprocal of the pivot instead of dividing (one more rounding per element of L, and
    two elements meet in every product): at most 2 u |l_i| |l_j| more per term of the sum, which the sum's own Q terms bound by
    Q u max diag;
  * the test forms Lc Lc^T in float64 numpy: another gamma_Q |L| |L|^T <= Q u max diag.
Together 4 Q u max diag.  It is derived, not measured, and stays as it is."""
import functools

import numpy as np

from tests.ball_predict_cases import JITTER, TOL, kernel_problem, one_ulp, relerr, se  # noqa: F401  (re-exported)

PATH_JITTER_DIRECT = 1e-4            # where z and chol are compared with the restatement directly
CHOL_C = 4.0
FUSED_M_MAX, FUSED_Q_MAX = 64, 64
NB, CAP = 64, 1 << 22                # videos of a chunk at most; doubles of one chunk's covariance block at most

# (B, T, m, Q): one of everything; one inducing point; more inducing points than frames; the 16 / 17 edges of the marginal kernel's
# lane groups; 33 (the first size of the 64-column instance); the reference shape at twice the frame rate plus one (Q = 61: an odd
# size, a Cholesky that stops inside the last row group); 64 / 64, the last shape fused in both; Q = 70: large because of Q, and two
# Cholesky block steps; m = 65: large because of m; 70 videos: more than one chunk; Q = 700: eleven Cholesky block steps
KERNEL_CASES = [(1, 1, 1, 1), (3, 5, 1, 3), (2, 2, 3, 4), (3, 30, 16, 16), (3, 30, 17, 33), (35, 30, 15, 61), (2, 64, 64, 64),
                (2, 64, 33, 70), (2, 100, 65, 40), (70, 30, 15, 9), (3, 12, 5, 700)]
KERNEL_IDS = ["-".join(str(v) for v in c) for c in KERNEL_CASES]


def kernel_shape(case):
    return tuple(int(v) for v in case.split("-"))


def is_fused(case):
    _, _, m, Q = kernel_shape(case)
    return m <= FUSED_M_MAX and Q <= FUSED_Q_MAX


def joint_posterior(times, y, s2, mask, z, ls, jitter, tau, path_jitter, eps=None, flip=False):
    """One video, one coordinate: (p_m (Q), C (Q, Q), Lc (Q, Q), z_s (Q)) at the query times tau.  mask None: every frame kept; eps
    None: z_s = p_m.  Lc is NaN where C + path_jitter I has no Cholesky factor."""
    if flip:
        z = z[::-1].copy()
    with np.errstate(divide="ignore"):
        p = np.where(s2 == 0.0, 0.0, 1.0 / s2)
    if mask is not None:
        p = mask * p
    py = np.where(p == 0.0, 0.0, p * y)
    m, Q = z.size, tau.size
    K, Kn, k = se(z, z, ls), se(times, z, ls), se(tau, z, ls)
    Sig = K + Kn.T @ (p[:, None] * Kn)
    Si, Ki = np.linalg.inv(Sig + jitter * np.eye(m)), np.linalg.inv(K + jitter * np.eye(m))
    w, X = Si @ (Kn.T @ py), Si - Ki
    p_m = k @ w
    C = se(tau, tau, ls) + k @ X @ k.T
    C = np.tril(C) + np.tril(C, -1).T                    # one triangle, mirrored
    try:
        Lc = np.linalg.cholesky(C + path_jitter * np.eye(Q))
    except np.linalg.LinAlgError:
        Lc = np.full((Q, Q), np.nan)
    return p_m, C, Lc, p_m if eps is None else p_m + Lc @ eps


def reference_of(prob, path_jitter, flip=False, use_mask=True, use_eps=True, tq=None):
    """dict(p_m, z (2, Q, B); cov, chol (2, B, Q, Q)) of a problem dict."""
    tq = prob["tq"] if tq is None else tq
    B, Q = prob["y"].shape[2], tq.size
    out = dict(p_m=np.zeros((2, Q, B)), z=np.zeros((2, Q, B)), cov=np.zeros((2, B, Q, Q)), chol=np.zeros((2, B, Q, Q)))
    for c in range(2):
        for b in range(B):
            r = joint_posterior(prob["times"], prob["y"][c, :, b], prob["s2"][c, :, b], prob["mask"][:, b] if use_mask else None,
                                prob["ip"][c], prob["ls"][c], prob["jitter"], tq, path_jitter,
                                prob["eps"][c, :, b] if use_eps else None, flip)
            out["p_m"][c, :, b], out["cov"][c, b], out["chol"][c, b], out["z"][c, :, b] = r
    return out


@functools.lru_cache(maxsize=None)
def kernel_reference(case, path_jitter=PATH_JITTER_DIRECT, flip=False):
    """Computed once per process and shared: callers must not write to it."""
    return reference_of(kernel_problem(case), path_jitter, flip)


def chol_residual_bound(A):
    """The bound above for A = C + jp I (Q, Q)."""
    return CHOL_C * A.shape[-1] * 2.0 ** -53 * float(np.max(np.diagonal(A, axis1=-2, axis2=-1)))


# ---------------------------------------------------------------------------------------------- the plans, as specified
FACTOR_STEPS = ["k_bp_scale_rows", "svgp_dgemm_batched", "k_bp_add_prior", "svgp_dgemm_batched", "svgp_spd_inverse_batched",
                "svgp_dgemm_batched", "k_bp_subtract"]
JOINT_STEPS = ["svgp_se1d_kernel_matrix_fwd", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_bpj_cov", "svgp_potrf_batched",
               "k_bpj_finish"]


def chunk(B, Q):
    return min(NB, B, max(1, CAP // (Q * Q)))


def expected_route(B, T, m, Q, large):
    if not large:
        return ["k_ball_predict_joint"]
    names, nb = [], chunk(B, Q)
    for _ in range(2):
        names.append("svgp_se1d_kernel_matrix_fwd")
        for _b0 in range(0, B, nb):
            names += FACTOR_STEPS + JOINT_STEPS
    return names
