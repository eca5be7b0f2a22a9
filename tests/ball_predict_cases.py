"""Cases, problems and the float64 numpy restatement of the moving-ball predictor tests (tests/test_ball_predict_cpu.py,
tests/test_gpu_ball_predict.py).

The restatement, per video and latent coordinate (include/svgpvae_hip.h, "moving ball: fill dropped frames"):
    p = mask * reciprocal_no_nan(s2)        K = SE(z, z)    Kn = SE(t, z)    Sig = K + Kn^T diag(p) Kn
    Si = (Sig + j I)^-1    Ki = (K + j I)^-1    w = Si Kn^T (p y)    X = Si - Ki
    k = SE(tau, z)    p_m = k w    p_v = 1 + diag(k X k^T)    z_s = p_m + eps sqrt(clamp(p_v, 1e-4, 1000))
`flip=True` evaluates the same sums with the inducing index reversed: a second summation order of the same algebra.

Bar (the project's own, tests/generate_cases.py and tests/animate_cases.py): TOL = 1e-8 relative to the tensor's max-abs
(helpers.relerr).  It is meaningful only where the restatement's own response to a one-ulp change of y, s2 and z stays within
TOL / 100; test_ball_predict_cpu.py asserts that for every case.  That is why the length scale is tied to the inducing spacing:
with ls = 2 and a spacing below about 1, K + j I has a condition number around 1e8 and the float64 restatement itself moves by
1e-5 under a one-ulp change of its inputs."""
import functools

import numpy as np

TOL = 1e-8
CLIP = (1e-4, 1000.0)                # SVGPVAE_model.py:701
JITTER = 1e-9

# (B, T, m, Q): one of everything; one inducing point; more inducing points than frames; the reference shape at twice the frame
# rate plus one; the 16 / 17 edges of the fused kernel's lane groups; 33 (the first size of its 64-column instance); 64, the last
# fused shape; 65 and 130: the large form only; 70 videos: more than the 64 channels of one rows call, so the large form windows
KERNEL_CASES = [(1, 1, 1, 1), (3, 5, 1, 3), (2, 2, 3, 4), (35, 30, 15, 61), (3, 30, 16, 16), (3, 30, 17, 33), (2, 64, 33, 70),
                (2, 64, 64, 40), (2, 100, 65, 40), (2, 130, 130, 70), (70, 30, 15, 9)]
KERNEL_IDS = ["-".join(str(v) for v in c) for c in KERNEL_CASES]
FUSED_M_MAX = 64


def kernel_shape(case):
    return tuple(int(v) for v in case.split("-"))


def length_scale(T, m):
    """min(2, 0.75 x inducing spacing); 2 where there is no spacing (m = 1)."""
    return 2.0 if m == 1 else min(2.0, 0.75 * (T - 1) / (m - 1))


@functools.lru_cache(maxsize=None)
def kernel_problem(case):
    """dict of float64 numpy arrays in the kernels' layout, never modified: times (T), tq (Q), ip (2, m), ls (2), y, s2, mask
    (2 | 1, T, B), eps (2, Q, B).  Video 1 (where there is one) has every frame dropped; one s2 entry of a kept frame is 0."""
    B, T, m, Q = kernel_shape(case)
    rs = np.random.RandomState(2000 + 11 * B + 7 * T + 3 * m + Q)
    times = np.arange(1, T + 1, dtype=np.float64)
    z = np.linspace(1.0, float(T), m) if m > 1 else np.array([0.5 * (1 + T)])
    ls = length_scale(T, m)
    ph, fr = rs.rand(2, 1, B) * 6.28, 0.5 + rs.rand(2, 1, B)
    y = np.sin(fr * times[None, :, None] / max(T, 2) * 6.28 + ph) + 0.1 * rs.randn(2, T, B)
    s2 = np.exp(rs.uniform(np.log(1e-3), np.log(1.0), (2, T, B)))
    mask = (rs.rand(T, B) >= 0.4).astype(np.float64)
    mask[0, :] = 1.0
    if B > 1:
        mask[:, 1] = 0.0
    tq = rs.uniform(-2.0, T + 5.0, Q)
    if Q > 1 and (np.diff(tq) > 0).all():                 # (a few draws can come out sorted)
        tq = tq[::-1].copy()
    s2[0, 0, 0] = 0.0                                     # reciprocal_no_nan: this kept frame carries no information either
    return dict(times=times, tq=tq, ip=np.stack([z, z.copy()]), ls=np.array([ls, ls / 1.1]), y=y, s2=s2,
                mask=mask, eps=rs.randn(2, Q, B), jitter=JITTER)


def se(a, b, ls):
    d = a[:, None] - b[None, :]
    return np.exp(-d * d / (2.0 * ls * ls))


def posterior(times, y, s2, mask, z, ls, jitter, tau, eps=None, flip=False, clip=CLIP):
    """One video, one coordinate: (p_m, p_v, z_s) at the query times tau.  mask None: every frame kept; eps None: z_s = p_m."""
    if flip:
        z = z[::-1].copy()
    with np.errstate(divide="ignore"):
        p = np.where(s2 == 0.0, 0.0, 1.0 / s2)
    if mask is not None:
        p = mask * p
    py = np.where(p == 0.0, 0.0, p * y)
    m = z.size
    K, Kn, k = se(z, z, ls), se(times, z, ls), se(tau, z, ls)
    Sig = K + Kn.T @ (p[:, None] * Kn)
    Si, Ki = np.linalg.inv(Sig + jitter * np.eye(m)), np.linalg.inv(K + jitter * np.eye(m))
    w, X = Si @ (Kn.T @ py), Si - Ki
    p_m, p_v = k @ w, 1.0 + np.einsum("qi,ij,qj->q", k, X, k)
    return p_m, p_v, p_m if eps is None else p_m + eps * np.sqrt(np.clip(p_v, *clip))


def reference_of(prob, flip=False, use_mask=True, use_eps=True, tq=None):
    """(p_m, p_v, z) of a problem dict, each (2, Q, B)."""
    tq = prob["tq"] if tq is None else tq
    B = prob["y"].shape[2]
    out = np.zeros((3, 2, tq.size, B))
    for c in range(2):
        for b in range(B):
            r = posterior(prob["times"], prob["y"][c, :, b], prob["s2"][c, :, b], prob["mask"][:, b] if use_mask else None,
                          prob["ip"][c], prob["ls"][c], prob["jitter"], tq, prob["eps"][c, :, b] if use_eps else None, flip)
            for i in range(3):
                out[i, c, :, b] = r[i]
    return out[0], out[1], out[2]


@functools.lru_cache(maxsize=None)
def kernel_reference(case, flip=False):
    """Computed once per process and shared: callers must not write to it."""
    return reference_of(kernel_problem(case), flip)


def one_ulp(prob, seed=17):
    """The problem with every y, s2 and inducing point moved by one ulp up or down."""
    rs = np.random.RandomState(seed)
    ulp = lambda t: t * (1.0 + 2.0 ** -52 * (rs.randint(0, 2, t.shape) * 2 - 1))
    return dict(prob, y=ulp(prob["y"]), s2=ulp(prob["s2"]), ip=ulp(prob["ip"]))


def relerr(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-300))


# ---------------------------------------------------------------------------------------------- the large form's plan, as specified
NB, QC = 64, 4096                    # videos of a chunk = channels of one rows call; query rows of a chunk


def rows_names(rows, m, L):
    """svgp_sprites_posterior_rows_route (tests/test_animate_cpu.py): one launch up to m = 256, a bounded column split beyond."""
    one = ["k_sprites_posterior_rows"]
    if m <= 256:
        return one
    base = ((rows + 63) // 64) * L
    S = min(min((1024 + base - 1) // base, 16), (m + 63) // 64)
    return one if S == 1 else one + ["k_sprites_posterior_finish"]


def expected_route(B, T, m, Q, large):
    if not large:
        return ["k_ball_predict"]
    names = []
    for _ in range(2):
        names.append("svgp_se1d_kernel_matrix_fwd")
        for b0 in range(0, B, NB):
            nb = min(NB, B - b0)
            names += ["k_bp_scale_rows", "svgp_dgemm_batched", "k_bp_add_prior", "svgp_dgemm_batched", "svgp_spd_inverse_batched",
                      "svgp_dgemm_batched", "k_bp_subtract"]
            for q0 in range(0, Q, QC):
                names += ["svgp_se1d_kernel_matrix_fwd"] + rows_names(min(QC, Q - q0), m, nb) + ["k_bp_finish"]
    return names


# ---------------------------------------------------------------------------------------------- the predictor's problems
def predictor_problem(B, T, m, Q, px=8, hidden=16, seed=0, drop_video=None):
    """(params of float64 torch tensors, videos (B, T, px, px), observed (B, T) bool, query times (Q), eps (B, Q, 2)) with the
    length scales tied to the inducing spacing as above."""
    import torch

    from tests import ball_cases as BC
    lt = length_scale(T, m)
    p, vid, _ = BC._problem(B, T, px, hidden, m, seed=seed, lt=lt)
    p["l_y"] = torch.tensor(lt / 1.1, dtype=torch.float64)
    rs = np.random.RandomState(300 + seed)
    observed = rs.rand(B, T) >= 0.4
    observed[:, 0] = True
    if drop_video is not None:
        observed[drop_video, :] = False
    return p, vid, observed, rs.uniform(-2.0, T + 5.0, Q), rs.randn(B, Q, 2)


def predictor_reference(p, vid, observed, tq, eps, *, jitter, clip_qs, frame_times=None):
    """The oracle's MLP forward composed with the restatement: dict(frames (B, Q, px, py), p_m, p_v, z (B, Q, 2)) as numpy."""
    import torch

    from oracle import pearce_vae_oracle as PO
    B, T, px, py = vid.shape
    mu, var = PO.mlp_inference(p, vid)
    if clip_qs:
        var = torch.clamp(var, 1e-6, 1e3)
    times = np.arange(1, T + 1, dtype=np.float64) if frame_times is None else np.asarray(frame_times, dtype=np.float64)
    tr = lambda t: np.ascontiguousarray(t.numpy().transpose(2, 1, 0))          # (B, T, 2) -> (2, T, B)
    prob = dict(times=times, tq=np.asarray(tq, dtype=np.float64), ip=np.stack([p["ip_x"].numpy(), p["ip_y"].numpy()]),
                ls=np.array([float(p["l_x"]), float(p["l_y"])]), y=tr(mu), s2=tr(var),
                mask=np.ones((T, B)) if observed is None else np.asarray(observed, dtype=np.float64).T,
                eps=None if eps is None else np.ascontiguousarray(np.asarray(eps).transpose(2, 1, 0)), jitter=jitter)
    p_m, p_v, z = reference_of(prob, use_eps=eps is not None)
    bq2 = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))                   # (2, Q, B) -> (B, Q, 2)
    frames = torch.sigmoid(PO.mlp_decoder(p, torch.as_tensor(bq2(z)), px, py)).numpy()
    return dict(frames=frames, p_m=bq2(p_m), p_v=bq2(p_v), z=bq2(z))
