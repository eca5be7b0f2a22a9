// Moving-ball SVGP-VAE after training: the sparse-GP posterior of a video at ARBITRARY query times, from the
// frames that were observed.  Per video b and latent coordinate c, with SE(a, b) = exp(-(a - b)^2 / (2 ls^2)):
//   p   = mask * reciprocal_no_nan(s2)                         (a dropped frame is a frame of precision 0)
//   K   = SE(z, z)       Kn = SE(t, z)
//   Sig = K + Kn^T diag(p) Kn       Si = (Sig + j I)^-1        Ki = (K + j I)^-1
//   w   = Si Kn^T (p y)             X  = Si - Ki
//   k   = SE(tau, z)     p_m = k w     p_v = 1 + diag(k X k^T)     z = p_m + eps sqrt(clamp(p_v, clip_lo, clip_hi))
// which for tau = t and mask = 1 is SVGP.approximate_posterior_params (SVGPVAE_model.py:142-171; mean and diag(B)) and the draw of
// :701.  p_v is reported unclamped.  Where p = 0 the product p y is taken as 0 whatever y holds.
//
// svgp_ball_predict (m <= 64): ONE launch, a workgroup of 256 threads per (video, coordinate).  K in LDS; the frames are streamed
// in chunks of BP_TC: the chunk's kernel rows k_t are formed from times[t] into LDS, every thread adds p_t k_t[i] k_t[j] to the
// elements (i, j) it owns (registers) in frame order, so Sig and Kn^T (p y) have a fixed summation order and no (T, m) matrix
// exists.  Both matrices are inverted by lds_spd_inverse; a video without a kept frame has Sig + j I == K + j I bit for bit, hence
// X = 0 and w = 0 exactly.  The query times are walked in chunks of 16: 16 lanes share a query, each takes the rows i = lane,
// lane + 16, ... of k^T X k and of k . w, and an xor-shuffle adds the 16 partials; a query's bits do not depend on where it stands.
// LDS at m = 64: two 64 x 65 matrices, the 16 x 65 chunk and 4 x 64 + 32 values = 77 184 bytes (two workgroups per CU).
// k_ball_predict is two device pieces of ball_predict_shared.hpp: bp_factors (bp_prior, bp_accumulate from zeros, bp_invert,
// bp_store_x in place), which the joint predictor (ball_predict_joint.hip) inlines too, and bp_query_chunks over all Q query times; the streamed
// state (ball_state.hip) composes the same pieces around its stats and post.
//
// svgp_ball_predict_large (m <= 2048, T <= 2048): the same quantities from the library's global-memory pieces, walked in chunks of
// BPL_NB videos and BPL_QC query rows so that the workspace grows with neither B nor Q (bp_walk below is the one plan both the
// launch code and svgp_ball_predict_route follow).  This file holds the factor steps (bp_factor_launch) and the marginal tail
// (bp_tail_work, bp_tail_launch) for every caller, and bp_route_line, the route line of a step.  svgp_sprites_posterior_rows
// runs with the videos of a chunk as its channels (kbb = 1), an unbounded clip range and no draw: the clamp applies to the sample
// only and is taken in k_bp_finish.
#include "common.hpp"
#include "lds_spd_inverse.hpp"
#include "ball_predict_shared.hpp"

#include <cmath>

namespace {

template <int CW>
__global__ __launch_bounds__(256) void k_ball_predict(BpArgs a) {
    extern __shared__ __align__(16) real smem[];
    const int b = blockIdx.x, c = blockIdx.y, m = a.m;
    const BpLds s = bp_lds_map<CW>(smem, m * (m + 1), m * (m + 1));
    const real il2 = bp_factors<CW>(a, b, c, s);          // X in Sg, w in wv
    bp_query_chunks<CW>(a, b, c, s.Sg, m + 1, s.wv, s.zv, s.kt, il2, 0, a.Q);
}

inline size_t bp_lds_bytes(int m, int CW) { return ((size_t)2 * m * (m + 1) + bp_lds_tail_elems(CW)) * sizeof(real); }
static_assert(((size_t)2 * 64 * 65 + BP_TC * 65 + 4 * 64 + 2 * BP_TC) * sizeof(real) <= SVGP_LDS_MAX_BYTES / 2, "two workgroups per CU at m = 64");

// ---------------------------------------------------------------------------------------------------------
// the large form's own kernels
// ---------------------------------------------------------------------------------------------------------
// KnP (nb, T, m) = diag(p_l) Kn per video l = b0 + .. of the chunk, PY (T, nb) = p y
__global__ __launch_bounds__(SVGP_BLOCK) void k_bp_scale_rows(BpIn a, int c, int b0, int nb, const real* __restrict__ Kn,
                                                              real* __restrict__ KnP, real* __restrict__ PY) {
    const long long tot = (long long)nb * a.T * a.m, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= tot) return;
    const int i = (int)(e % a.m), t = (int)((e / a.m) % a.T), l = (int)(e / ((long long)a.m * a.T));
    real p, py;
    bp_precision(a, c, (size_t)t * a.B + b0 + l, p, py);
    KnP[e] = p * Kn[(size_t)t * a.m + i];
    if (i == 0) PY[(size_t)t * nb + l] = py;
}
// Mats (nb + 1, m, m): the first nb hold Kn^T diag(p_l) Kn and become Sig_l + j I, the last becomes K + j I
__global__ __launch_bounds__(SVGP_BLOCK) void k_bp_add_prior(int m, int nb, real jitter, const real* __restrict__ K, real* __restrict__ Mats) {
    const long long mm = (long long)m * m, tot = (nb + 1) * mm, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= tot) return;
    const long long o = e % mm;
    const real k = K[o], jit = (o / m == o % m) ? jitter : real(0);
    Mats[e] = e < nb * mm ? (k + Mats[e]) + jit : k + jit;
}
// X_l = Si_l - Ki in place
__global__ __launch_bounds__(SVGP_BLOCK) void k_bp_subtract(int m, int nb, real* __restrict__ Mats) {
    const long long mm = (long long)m * m, tot = nb * mm, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e < tot) Mats[e] -= Mats[tot + e % mm];
}
// (nq, nb) rows of a chunk -> the (Q, B) outputs; the draw with the clamped variance
__global__ __launch_bounds__(SVGP_BLOCK) void k_bp_finish(BpArgs a, int c, int b0, int nb, int q0, int nq, const real* __restrict__ tpm,
                                                          const real* __restrict__ tpv) {
    const long long tot = (long long)nq * nb, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= tot) return;
    const size_t o = (size_t)(q0 + e / nb) * a.B + b0 + e % nb;
    const real pm = tpm[e], pv = tpv[e];
    a.p_m[c][o] = pm; a.p_v[c][o] = pv;
    if (a.z[c]) a.z[c][o] = a.eps[c] ? pm + a.eps[c][o] * sqrt(clip_keep_nan(pv, a.lo, a.hi)) : pm;
}

// ---------------------------------------------------------------------------------------------------------
// one plan for the launch code and the route text
// ---------------------------------------------------------------------------------------------------------
// calls f(step) for every launch group of one call, in order; stops at the first non-zero return
template <class F>
int bp_walk(const svgp_ball_predict_cfg* g, bool large, F f) {
    int rc;
    if (!large) return f(BpStep{BP_FUSED, 0, 0, g->B, 0, g->Q});
    for (int c = 0; c < 2; ++c) {
        if ((rc = f(BpStep{BP_KMAT, c, 0, 0, 0, 0}))) return rc;
        for (int b0 = 0; b0 < g->B; b0 += BPL_NB) {
            const int nb = g->B - b0 < BPL_NB ? g->B - b0 : BPL_NB;
            if ((rc = bp_walk_factors(c, b0, nb, f))) return rc;
            if ((rc = bp_walk_tail(c, b0, nb, g->Q, f))) return rc;
        }
    }
    return SVGP_OK;
}

int bp_check(const svgp_ball_predict_cfg* g, bool large) {
    SVGP_REQUIRE(g != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(g->B >= 1 && g->T >= 1 && g->m >= 1 && g->Q >= 1, SVGP_ERR_INVALID, "need B, T, m, Q >= 1 (B=%d T=%d m=%d Q=%d)", g->B,
                 g->T, g->m, g->Q);
    const int m_max = large ? SVGP_M_LIMIT : BP_M_MAX, t_max = large ? BPL_T_MAX : BP_T_MAX;
    SVGP_REQUIRE(g->m <= m_max, SVGP_ERR_UNSUPPORTED, "m=%d: %s takes m <= %d", g->m, large ? "svgp_ball_predict_large" : "svgp_ball_predict", m_max);
    SVGP_REQUIRE(g->T <= t_max, SVGP_ERR_UNSUPPORTED, "T=%d: %s takes T <= %d", g->T, large ? "svgp_ball_predict_large" : "svgp_ball_predict", t_max);
    SVGP_REQUIRE(g->clip_lo <= g->clip_hi, SVGP_ERR_INVALID, "need clip_lo <= clip_hi (%g, %g)", g->clip_lo, g->clip_hi);
    return SVGP_OK;
}

int bp_args(const svgp_ball_predict_cfg* g, const svgp_ball_predict_bufs* q, BpArgs* a) {
    int rc = bp_marshal(g, q, true, true, a);
    if (rc) return rc;
    SVGP_REQUIRE(q->p_v_x && q->p_v_y, SVGP_ERR_INVALID, "NULL device pointer");
    a->lo = g->clip_lo; a->hi = g->clip_hi; a->p_v[0] = q->p_v_x; a->p_v[1] = q->p_v_y;
    return SVGP_OK;
}

struct BpWork { BpFactorWork f; BpTailWork t; int64_t total; };
BpWork bp_work(const svgp_ball_predict_cfg* g) {
    const int64_t nb = g->B < BPL_NB ? g->B : BPL_NB;
    SvgpTake16 c16;
    BpWork o;
    o.f = bp_factor_work(c16, g->m, g->T, nb);
    o.t = bp_tail_work(c16, g->m, g->Q, nb);
    o.total = c16.p;
    return o;
}

// the route text's name of each BpOp
const char* const BP_NAME[] = {"k_ball_predict", "svgp_se1d_kernel_matrix_fwd", "k_bp_scale_rows", "svgp_dgemm_batched", "k_bp_add_prior",
                               "svgp_dgemm_batched", "svgp_spd_inverse_batched", "svgp_dgemm_batched", "k_bp_subtract",
                               "svgp_se1d_kernel_matrix_fwd", "svgp_sprites_posterior_rows", "k_bp_finish",
                               "k_ball_predict_joint", "svgp_se1d_kernel_matrix_fwd", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_bpj_cov",
                               "svgp_potrf_batched", "k_bpj_finish"};
// the rows entry runs with the videos of a chunk as its channels, an unbounded clip range and no draw
inline svgp_posterior_rows_cfg bp_rows_cfg(const BpStep& s, int m) { return {s.nq, m, s.nb, -INFINITY, INFINITY}; }

}  // namespace

int bp_route_line(const BpStep& s, int m, char* buf, int cap, int* pos) {
    if (s.op != BP_ROWS) return svgp_route_append(buf, cap, pos, "%s\n", BP_NAME[s.op]);
    const svgp_posterior_rows_cfg rc_ = bp_rows_cfg(s, m);
    char sub[128];
    int r = svgp_sprites_posterior_rows_route(&rc_, sub, (int)sizeof(sub));
    if (r) return r;
    return svgp_route_append(buf, cap, pos, "%s", sub);
}

BpFactorWork bp_factor_work(SvgpTake16& c16, int64_t m, int64_t T, int64_t nb) {
    BpFactorWork o;
    o.K = c16.take(m * m); o.Kn = c16.take(T * m); o.knn = c16.take(T);
    o.KnP = c16.take(nb * T * m); o.PY = c16.take(T * nb); o.Mats = c16.take((nb + 1) * m * m); o.V = c16.take(m * nb); o.W = c16.take(nb * m);
    o.logdet = c16.take(nb + 1); o.inv = c16.take((int64_t)svgp_spd_inverse_workspace_elems((int)m, (int)nb + 1));
    return o;
}

BpTailWork bp_tail_work(SvgpTake16& c16, int64_t m, int64_t Q, int64_t nb) {
    const int64_t nq = Q < BPL_QC ? Q : BPL_QC;
    BpTailWork o;
    o.K2 = c16.take(m * m); o.Kq = c16.take(nq * m); o.kbb = c16.take(nq);
    o.tpm = c16.take(nq * nb); o.tpv = c16.take(nq * nb);
    o.rows = c16.take(m > 256 ? 16 * nq * nb : 0);      // svgp_sprites_posterior_rows_workspace_elems: at most 16 b L, 0 up to m = 256
    return o;
}

int bp_tail_launch(const BpArgs& a, const BpStep& s, const BpTailWork& w, const real* X, const real* W, double* work, void* stream) {
    switch (s.op) {
    case BP_KQ:
        return svgp_se1d_kernel_matrix_fwd(s.nq, a.m, a.tq + s.q0, a.ip[s.c], a.ls[s.c], work + w.K2, work + w.Kq, work + w.kbb, stream);
    case BP_ROWS: {     // the clamp applies to the sample only and is taken in k_bp_finish
        const svgp_posterior_rows_cfg rc_ = bp_rows_cfg(s, a.m);
        return svgp_sprites_posterior_rows(&rc_, work + w.Kq, work + w.kbb, W, X, nullptr, work + w.tpm, work + w.tpv, nullptr, work + w.rows,
                                           stream);
    }
    case BP_FINISH:
        hipLaunchKernelGGL(k_bp_finish, dim3(svgp_blocks((long long)s.nq * s.nb)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, a, s.c, s.b0, s.nb,
                           s.q0, s.nq, work + w.tpm, work + w.tpv);
        SVGP_LAUNCH_CHECK();
        break;
    default:
        SVGP_REQUIRE(false, SVGP_ERR_INVALID, "bp_tail_launch: op %d is not a step of the marginal tail", (int)s.op);
    }
    return SVGP_OK;
}

int bp_factor_launch(const BpIn& a, const BpStep& s, const BpFactorWork& w, double* work, void* stream) {
    const int c = s.c, nb = s.nb, m = a.m, T = a.T;
    const long long mm = (long long)m * m;
    hipStream_t st = (hipStream_t)stream;
    switch (s.op) {
    case BP_KMAT:
        return svgp_se1d_kernel_matrix_fwd(T, m, a.times, a.ip[c], a.ls[c], work + w.K, work + w.Kn, work + w.knn, stream);
    case BP_SCALE:
        hipLaunchKernelGGL(k_bp_scale_rows, dim3(svgp_blocks((long long)nb * T * m)), dim3(SVGP_BLOCK), 0, st, a, c, s.b0, nb, work + w.Kn,
                           work + w.KnP, work + w.PY);
        SVGP_LAUNCH_CHECK();
        break;
    case BP_SIGMA:      // Kn^T diag(p_l) Kn: the shared Kn has stride 0
        return svgp_dgemm_batched(1, 0, m, m, T, 1.0, work + w.Kn, m, 0, work + w.KnP, m, (long long)T * m, 0.0, work + w.Mats, m, mm, nb,
                                  stream);
    case BP_PRIOR:
        hipLaunchKernelGGL(k_bp_add_prior, dim3(svgp_blocks((nb + 1) * mm)), dim3(SVGP_BLOCK), 0, st, m, nb, a.jitter, work + w.K,
                           work + w.Mats);
        SVGP_LAUNCH_CHECK();
        break;
    case BP_V:          // V (m, nb) = Kn^T PY
        return svgp_dgemm_batched(1, 0, m, nb, T, 1.0, work + w.Kn, m, 0, work + w.PY, nb, 0, 0.0, work + w.V, nb, 0, 1, stream);
    case BP_INVERSE:
        return svgp_spd_inverse_batched(m, nb + 1, work + w.Mats, work + w.logdet, work + w.inv, stream);
    case BP_W:          // w_l = Si_l V[:, l]
        return svgp_dgemm_batched(0, 0, m, 1, m, 1.0, work + w.Mats, m, mm, work + w.V, nb, 1, 0.0, work + w.W, 1, m, nb, stream);
    case BP_SUB:
        hipLaunchKernelGGL(k_bp_subtract, dim3(svgp_blocks(nb * mm)), dim3(SVGP_BLOCK), 0, st, m, nb, work + w.Mats);
        SVGP_LAUNCH_CHECK();
        break;
    default:
        SVGP_REQUIRE(false, SVGP_ERR_INVALID, "bp_factor_launch: op %d is not a factor step", (int)s.op);
    }
    return SVGP_OK;
}

extern "C" int svgp_ball_predict_route(const svgp_ball_predict_cfg* g, int large, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = bp_check(g, large != 0);
    if (rc) return rc;
    int pos = 0;
    buf[0] = 0;
    return bp_walk(g, large != 0, [&](const BpStep& s) -> int { return bp_route_line(s, g->m, buf, cap, &pos); });
}

extern "C" int svgp_ball_predict(const svgp_ball_predict_cfg* g, const svgp_ball_predict_bufs* q, void* stream) {
    int rc = bp_check(g, false);
    if (rc) return rc;
    BpArgs a;
    rc = bp_args(g, q, &a);
    if (rc) return rc;
    return bp_walk(g, false, [&](const BpStep&) -> int {
        const dim3 grid((unsigned)a.B, 2);
        if (a.m <= 32) {
            const size_t lds = bp_lds_bytes(a.m, 32);
            rc = set_dyn_lds(k_ball_predict<32>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL(k_ball_predict<32>, grid, dim3(256), lds, (hipStream_t)stream, a);
        } else {
            const size_t lds = bp_lds_bytes(a.m, 64);
            rc = set_dyn_lds(k_ball_predict<64>, lds);
            if (rc) return rc;
            hipLaunchKernelGGL(k_ball_predict<64>, grid, dim3(256), lds, (hipStream_t)stream, a);
        }
        SVGP_LAUNCH_CHECK();
        return (int)SVGP_OK;
    });
}

extern "C" long long svgp_ball_predict_large_workspace_elems(const svgp_ball_predict_cfg* g) {
    if (bp_check(g, true)) return 0;
    return bp_work(g).total;
}

extern "C" int svgp_ball_predict_large(const svgp_ball_predict_cfg* g, const svgp_ball_predict_bufs* q, double* work, void* stream) {
    int rc = bp_check(g, true);
    if (rc) return rc;
    BpArgs a;
    rc = bp_args(g, q, &a);
    if (rc) return rc;
    const BpWork w = bp_work(g);
    SVGP_REQUIRE(work != nullptr, SVGP_ERR_INVALID, "work is NULL (B = %d, T = %d, m = %d, Q = %d needs %lld doubles)", g->B, g->T, g->m,
                 g->Q, (long long)w.total);
    return bp_walk(g, true, [&](const BpStep& s) -> int {
        switch (s.op) {
        case BP_KQ: case BP_ROWS: case BP_FINISH:
            return bp_tail_launch(a, s, w.t, work + w.f.Mats, work + w.f.W, work, stream);
        default:            // BP_KMAT and the seven factor steps; anything else is refused there
            return bp_factor_launch(a, s, w.f, work, stream);
        }
    });
}
