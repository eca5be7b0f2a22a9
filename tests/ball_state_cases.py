"""Cases, helpers and the float64 numpy restatement of the streamed moving-ball posterior state (tests/test_ball_state_cpu.py,
tests/test_gpu_ball_state.py).  Problems, references and bars are those of tests/ball_predict_cases.py and tests/ball_joint_cases.py,
imported as they are.

The restatement of the state (include/svgpvae_hip.h, "moving ball: streamed posterior state"), per video and latent coordinate,
with se, p and py exactly as in ball_predict_cases.posterior:
    Kn = se(t, z)      S = Kn^T diag(p) Kn  (m x m)      r = Kn^T (p y)  (m)        stats = [S row-major, r]
Both are sums over the frames, so the stats of the pieces of a video add up to those of the whole.

Bars: stats at STATS_TOL = 1e-12 relative to the tensor's max-abs, the project's bar between two float64 evaluations of a
well-conditioned sum (every term of an element of S is a non-negative product; test_ball_state_cpu.py measures the restatement's
own response to the summation order at 1e-14, the margin behind it).  Everything behind the inverse at TOL = 1e-8 against the
restatement and at PATH_TOL = 1e-10 between two HIP paths (DESIGN.md sections 9f / 9g)."""
import functools

import numpy as np

from tests.ball_joint_cases import PATH_JITTER_DIRECT, joint_posterior  # noqa: F401  (re-exported)
from tests.ball_predict_cases import TOL, kernel_problem, kernel_reference, reference_of, relerr, se  # noqa: F401  (re-exported)

STATS_TOL = 1e-12
ORDER_TOL = 1e-14                    # forward against reversed frame order in the restatement itself
PATH_TOL = 1e-10
FUSED_M_MAX = 64
NB, QC, CAP = 64, 4096, 1 << 22      # videos of a chunk; query rows of a chunk; doubles of a joint chunk's covariance block
OPS = dict(update=0, finalize=1, query=2, query_joint=3)

# (B, T, m, Q) -> cut points of the frames (each one a two-piece feeding; a case without cuts is fed whole only)
CASES = {(1, 1, 1, 1): [], (3, 5, 1, 3): [2], (2, 2, 3, 4): [1], (3, 30, 16, 16): [1, 15, 16, 17], (3, 30, 17, 33): [16],
         (2, 64, 32, 17): [], (2, 64, 33, 70): [31, 32, 33], (2, 64, 64, 40): [16, 48], (35, 30, 15, 61): [10, 20],
         (2, 100, 65, 40): [50], (70, 30, 15, 9): []}
LARGE_ONLY = [(2, 100, 65, 40), (70, 30, 15, 9)]       # m > 64; forced large: more videos than one chunk
cid = lambda shape: "-".join(str(v) for v in shape)
shape_of = lambda case: tuple(int(v) for v in case.split("-"))
CASE_IDS = [cid(s) for s in CASES]
FUSED_IDS = [cid(s) for s in CASES if s not in LARGE_ONLY]
# (case, large) of every route a case runs on: the large route also on a few shapes the fused one serves
LARGE_TOO = [(3, 5, 1, 3), (3, 30, 17, 33), (2, 64, 33, 70)]
ROUTES = [(cid(s), False) for s in CASES if s not in LARGE_ONLY] + [(cid(s), True) for s in LARGE_TOO + LARGE_ONLY]
ROUTE_IDS = [f"{c}-{'large' if l else 'fused'}" for c, l in ROUTES]


def cuts_of(case):
    return CASES[shape_of(case)]


def stats_of(times, y, s2, mask, z, ls):
    """One video, one coordinate: [S row-major, r] (m m + m) of the frames at `times`.  mask None: every frame kept."""
    with np.errstate(divide="ignore"):
        p = np.where(s2 == 0.0, 0.0, 1.0 / s2)
    if mask is not None:
        p = mask * p
    py = np.where(p == 0.0, 0.0, p * y)
    Kn = se(times, z, ls)
    return np.concatenate([(Kn.T @ (p[:, None] * Kn)).reshape(-1), Kn.T @ py])


def problem_stats(prob, frames=None):
    """stats (B, 2, m m + m) of a problem dict over the frames `frames` (a slice or an index array; default all, in order)."""
    sel = slice(None) if frames is None else frames
    B, m = prob["y"].shape[2], prob["ip"].shape[1]
    out = np.zeros((B, 2, m * m + m))
    for c in range(2):
        for b in range(B):
            out[b, c] = stats_of(prob["times"][sel], prob["y"][c, sel, b], prob["s2"][c, sel, b], prob["mask"][sel, b], prob["ip"][c],
                                 prob["ls"][c])
    return out


@functools.lru_cache(maxsize=None)
def case_stats(case):
    """Computed once per process and shared: callers must not write to it."""
    return problem_stats(kernel_problem(case))


def post_of(prob, stats):
    """post (B, 2, m m + m) = [X row-major, w] from stats, as ball_predict_cases.posterior forms them."""
    B, m = stats.shape[0], prob["ip"].shape[1]
    out = np.zeros_like(stats)
    for c in range(2):
        K = se(prob["ip"][c], prob["ip"][c], prob["ls"][c])
        Ki = np.linalg.inv(K + prob["jitter"] * np.eye(m))
        for b in range(B):
            S, r = stats[b, c, :m * m].reshape(m, m), stats[b, c, m * m:]
            Si = np.linalg.inv(K + S + prob["jitter"] * np.eye(m))
            out[b, c] = np.concatenate([(Si - Ki).reshape(-1), Si @ r])
    return out


# ---------------------------------------------------------------------------------------------- the plans, as specified
def slices_of(B, Q, q_slices=0):
    """S of the fused query: q_slices forces it; else about 512 workgroups, at least one round of 16 query times a slice."""
    if q_slices > 0:
        return q_slices
    return max(1, min(-(-512 // (2 * B)), slices_max(Q)))


def slices_max(Q):
    return min(-(-Q // 16), 65535)


def joint_chunk(B, Q):
    return min(NB, B, max(1, CAP // (Q * Q)))


def expected_route(op, B, T, m, Q, large):
    from tests.ball_predict_cases import rows_names
    if op != "query_joint" and not large:
        return ["k_ball_state_" + op]
    names, nb_max = [], joint_chunk(B, Q) if op == "query_joint" else NB
    for _ in range(2):
        if op in ("update", "finalize"):
            names.append("svgp_se1d_kernel_matrix_fwd")
        for b0 in range(0, B, nb_max):
            nb = min(nb_max, B - b0)
            if op == "update":
                names += ["k_bp_scale_rows", "svgp_dgemm_batched", "svgp_dgemm_batched"]
            elif op == "finalize":
                names += ["k_bs_gather", "k_bp_add_prior", "svgp_spd_inverse_batched", "svgp_dgemm_batched", "k_bp_subtract", "k_bs_scatter"]
            elif op == "query":
                names.append("k_bs_gather")
                for q0 in range(0, Q, QC):
                    names += ["svgp_se1d_kernel_matrix_fwd"] + rows_names(min(QC, Q - q0), m, nb) + ["k_bp_finish"]
            else:
                names += ["k_bs_gather", "svgp_se1d_kernel_matrix_fwd", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_bpj_cov",
                          "svgp_potrf_batched", "k_bpj_finish"]
    return names
