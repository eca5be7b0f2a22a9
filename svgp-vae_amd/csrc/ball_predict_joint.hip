// Moving-ball SVGP-VAE after training, joint over the query times: the full posterior covariance of a
// video's latent path at the query times and coherent sample paths.  With X, w and k = SE(tau, z) of ball_predict.hip (9h), per
// video b and latent coordinate c:
//   C   = SE(tau, tau) + k X k^T                 (Q x Q; diag C = p_v of 9h; no clamp anywhere)
//   Lc  = chol(C + jp I)  lower                  jp = path_jitter
//   p_m = k w             z = p_m + Lc eps       (eps NULL: z = p_m)
// which for tau = t and mask = 1 is the full B of SVGP.approximate_posterior_params (SVGPVAE_model.py:141-171).  A video with every
// frame dropped has X = 0 and w = 0 exactly, hence C = SE(tau, tau) and p_m = 0: paths from the prior.  A non-positive pivot gives
// NaN in that (video, coordinate)'s chol and z only (the convention of svgp_potrf_batched: no error code, no synchronisation).
//
// svgp_ball_predict_joint (m <= 64, Q <= 64): ONE launch, a workgroup of 256 threads per (video, coordinate).  bp_factors (the
// pieces bp_prior, bp_accumulate, bp_invert, bp_store_x of ball_predict_shared.hpp) leaves X and w in LDS exactly as in
// k_ball_predict.  Then the kernel rows of all Q query times (kq), G = kq X in the slot K + j I
// occupied, and the lower triangle of C in the slot of X (which G no longer needs): element (q, r) is G[a] . kq[b] + SE(tau_q,
// tau_r) where a is the one of q, r with the larger query time -- the pair's value, not its position, decides which row goes
// through X, so permuting tau permutes the rows and columns of C bit for bit (equal times have equal rows).  The triangle is
// mirrored, stored, jp goes on the diagonal, and a right-looking Cholesky runs in place (two barriers a column; column j = tid &
// 63, rows tid / 64 + 4 r).  Thread q forms p_m[q] = kq[q] . w and z[q] = p_m[q] + sum_{r <= q} Lc[q][r] eps[r] in index order.
// LDS at m = Q = 64: three 64 x 65 matrices (G, C, kq), the 16 x 65 chunk, 4 x 64 + 32 and 3 x 64 values = 112 000 bytes of the
// CU's 160 KiB: one workgroup per CU.
//
// svgp_ball_predict_joint_large (m, T, Q <= 2048): the library's pieces.  Per coordinate svgp_se1d_kernel_matrix_fwd (K, Kn), then
// per chunk of nb = min(64, B, max(1, BPJL_CAP / Q^2)) videos the seven steps of the marginal large form up to X_l and w_l
// (bp_walk_factors), svgp_se1d_kernel_matrix_fwd for k, svgp_dgemm_batched twice (k X_l, then (k X_l) k^T, k at stride 0),
// k_bpj_cov (adds SE(tau, tau), mirrors the lower triangle, writes cov, adds jp), svgp_potrf_batched with its panel solves refined
// once (svgp_potrf_batched_refined: beyond Q = 64 the plain routine's residual of Lc Lc^T carries the condition number of the
// diagonal blocks, and C + jp I at jp = 1e-9 is ill conditioned), and k_bpj_finish (p_m = k w_l, z = p_m + Lc eps, the copy of chol).
// Those six steps are the joint tail (bpj_walk_tail), whose workspace and launches (bpj_tail_work, bpj_tail_launch) this file holds
// for the streamed state's joint query too.  bpj_walk is the one plan the launch code and svgp_ball_predict_joint_route follow.
#include "common.hpp"
#include "lds_spd_inverse.hpp"
#include "ball_predict_shared.hpp"

#include <cmath>

namespace {

constexpr int BPJ_Q_MAX = 64;                        // query times of the fused kernel

// LDS beyond bp_lds_map's: kq (Q x ld), eps of the video, p_m, the query times (BPJ_Q_MAX each)
__host__ __device__ constexpr int bpj_ldq(int Q) { return Q | 1; }          // odd row stride of C: a column walk spreads over the banks
inline int bpj_slot1(int m, int Q) { return (m > Q ? m : Q) * (m + 1); }
inline int bpj_slot2(int m, int Q) { const int a = m * (m + 1), b = Q * bpj_ldq(Q); return a > b ? a : b; }
inline size_t bpj_lds_bytes(int m, int Q, int CW) {
    return ((size_t)bpj_slot1(m, Q) + bpj_slot2(m, Q) + bp_lds_tail_elems(CW) + (size_t)Q * (m + 1) + 3 * BPJ_Q_MAX) * sizeof(real);
}
static_assert(((size_t)3 * 64 * 65 + bp_lds_tail_elems(64) + 3 * 64) * sizeof(real) == 112000, "the LDS map of DESIGN 9l at m = Q = 64");
static_assert(112000 <= SVGP_LDS_MAX_BYTES, "one workgroup per CU at m = Q = 64");

template <int CW>
__global__ __launch_bounds__(256) void k_ball_predict_joint(BpjArgs a, int n1, int n2) {
    extern __shared__ __align__(16) real smem[];
    const int tid = threadIdx.x, j = tid & 63, i0 = tid >> 6;
    const int b = blockIdx.x, c = blockIdx.y, m = a.m, ld = m + 1, B = a.B, Q = a.Q, lq = bpj_ldq(Q);
    const BpLds s = bp_lds_map<CW>(smem, n1, n2);
    real* G = s.Km;                  // Q x ld : kq X, in the slot of (K + j I)^-1
    real* Cm = s.Sg;                 // Q x lq : C, C + jp I, Lc, in the slot of X
    real* kq = s.pyc + BP_TC;        // Q x ld : kernel rows of the query times
    real* ev = kq + Q * ld;          // BPJ_Q_MAX : eps of this video
    real* pmv = ev + BPJ_Q_MAX;      // BPJ_Q_MAX : p_m
    real* tv = pmv + BPJ_Q_MAX;      // BPJ_Q_MAX : the query times
    const real* __restrict__ eps = a.eps[c];
    real* __restrict__ o_cov = a.cov[c];
    real* __restrict__ o_chol = a.chol[c];
    real* __restrict__ o_z = a.z[c];
    const real il2 = bp_factors<CW>(a, b, c, s);          // X in s.Sg, w in s.wv
    // ---- kernel rows of all query times
    for (int e = tid; e < Q * m; e += 256) {
        const int q = e / m, i = e - q * m;
        const real d = a.tq[q] - s.zv[i];
        kq[q * ld + i] = exp(d * d * il2);
    }
    if (tid < Q) { ev[tid] = eps ? eps[(size_t)tid * B + b] : real(0); tv[tid] = a.tq[tid]; }
    __syncthreads();                 // X and kq are complete, K + j I's slot is free
    // ---- G = kq X (consecutive lanes walk a row of X), p_m = kq w
    for (int e = tid; e < Q * m; e += 256) {
        const int q = e / m, i = e - q * m;
        const real* kr = kq + q * ld;
        real g = 0;
#pragma unroll 4
        for (int k = 0; k < m; ++k) g += kr[k] * s.Sg[k * ld + i];
        G[q * ld + i] = g;
    }
    if (tid < Q) {
        const real* kr = kq + tid * ld;
        real pm = 0;
#pragma unroll 4
        for (int k = 0; k < m; ++k) pm += kr[k] * s.wv[k];
        pmv[tid] = pm;
        a.p_m[c][(size_t)tid * B + b] = pm;
    }
    __syncthreads();                 // G is complete, X is no longer needed
    // ---- the lower triangle of C and its mirror image
#pragma unroll 1
    for (int r = 0; r < BPJ_Q_MAX / 4; ++r) {
        const int q = i0 + 4 * r;
        if (q < Q && j <= q) {
            const bool qfirst = tv[q] >= tv[j];
            const real* gr = G + (qfirst ? q : j) * ld;
            const real* kr = kq + (qfirst ? j : q) * ld;
            real sum = 0;
#pragma unroll 4
            for (int k = 0; k < m; ++k) sum += gr[k] * kr[k];
            const real d = tv[q] - tv[j], v = sum + exp(d * d * il2);
            Cm[q * lq + j] = v;
            Cm[j * lq + q] = v;
        }
    }
    __syncthreads();
    // ---- cov out; jp on the diagonal (by the thread that read it)
#pragma unroll 1
    for (int r = 0; r < BPJ_Q_MAX / 4; ++r) {
        const int q = i0 + 4 * r;
        if (q < Q && j < Q) {
            const real v = Cm[q * lq + j];
            if (o_cov) o_cov[((size_t)b * Q + q) * Q + j] = v;
            if (q == j) Cm[q * lq + q] = v + a.jp;
        }
    }
    if (!o_chol && !(o_z && eps)) {                       // no factor asked for: z is the mean
        if (o_z && tid < Q) o_z[(size_t)tid * B + b] = pmv[tid];
        return;
    }
    // ---- Lc = chol(C + jp I) in place on the lower triangle: a thread owns (i0 + 4 r, j)
    for (int k = 0; k < Q; ++k) {
        __syncthreads();
        const real akk = Cm[k * lq + k], piv = akk > real(0) ? sqrt(akk) : real(NAN), ip = real(1) / piv;
        const real ljk = (j > k && j < Q) ? Cm[j * lq + k] * ip : real(0);
        real f[BPJ_Q_MAX / 4];
#pragma unroll
        for (int r = 0; r < BPJ_Q_MAX / 4; ++r) { const int i = i0 + 4 * r; f[r] = (i > k && i < Q) ? Cm[i * lq + k] * ip : real(0); }
        __syncthreads();
        if (j == k) {
#pragma unroll
            for (int r = 0; r < BPJ_Q_MAX / 4; ++r) {
                const int i = i0 + 4 * r;
                if (i == k) Cm[k * lq + k] = piv;
                else if (i > k && i < Q) Cm[i * lq + k] = f[r];
            }
        } else if (j > k && j < Q) {
#pragma unroll
            for (int r = 0; r < BPJ_Q_MAX / 4; ++r) {
                const int i = i0 + 4 * r;
                if (i >= j && i < Q) Cm[i * lq + j] -= f[r] * ljk;
            }
        }
    }
    __syncthreads();
    if (o_chol) {
#pragma unroll 1
        for (int r = 0; r < BPJ_Q_MAX / 4; ++r) {
            const int q = i0 + 4 * r;
            if (q < Q && j < Q) o_chol[((size_t)b * Q + q) * Q + j] = j <= q ? Cm[q * lq + j] : real(0);
        }
    }
    if (o_z && tid < Q) {
        real sum = 0;
        if (eps)
            for (int r = 0; r <= tid; ++r) sum += Cm[tid * lq + r] * ev[r];
        o_z[(size_t)tid * B + b] = eps ? pmv[tid] + sum : pmv[tid];
    }
}

// ---------------------------------------------------------------------------------------------------------
// the large form's own kernels
// ---------------------------------------------------------------------------------------------------------
// Cb (nb, Q, Q) holds (k X_l) k^T: the thread of (l, q, r <= q) adds SE(tau_q, tau_r), writes the value to both triangles of Cb and
// of cov[b0 + l] (when given), and adds jp to Cb's diagonal
__global__ __launch_bounds__(SVGP_BLOCK) void k_bpj_cov(BpjArgs a, int c, int b0, int nb, real* __restrict__ Cb) {
    const long long QQ = (long long)a.Q * a.Q, tot = nb * QQ, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= tot) return;
    const int r = (int)(e % a.Q), q = (int)((e / a.Q) % a.Q);
    const long long l = e / QQ;
    if (r > q) return;
    const real ls = *a.ls[c], il2 = real(-0.5) / (ls * ls), d = a.tq[q] - a.tq[r];
    const real v = Cb[e] + exp(d * d * il2);
    const long long et = l * QQ + (long long)r * a.Q + q;
    Cb[et] = v;
    Cb[e] = q == r ? v + a.jp : v;
    if (a.cov[c]) {
        real* o = a.cov[c] + (size_t)(b0 + l) * QQ;
        o[(size_t)q * a.Q + r] = v;
        o[(size_t)r * a.Q + q] = v;
    }
}
// a wave per (l, q): p_m = k[q] . w_l, z = p_m + Lc_l[q] . eps (fixed-order wave sums), row q of chol
__global__ __launch_bounds__(SVGP_BLOCK) void k_bpj_finish(BpjArgs a, int c, int b0, int nb, const real* __restrict__ Kq,
                                                           const real* __restrict__ W, const real* __restrict__ Lb) {
    const int lane = threadIdx.x & 63, Q = a.Q, m = a.m;
    const long long row = (long long)blockIdx.x * (SVGP_BLOCK / 64) + (threadIdx.x >> 6);
    if (row >= (long long)nb * Q) return;
    const int q = (int)(row % Q), l = (int)(row / Q);
    const real* kr = Kq + (size_t)q * m;
    const real* wl = W + (size_t)l * m;
    const real* lr = Lb + ((size_t)l * Q + q) * Q;
    const real* eps = a.eps[c];
    real pm = 0, sum = 0;
    for (int k = lane; k < m; k += 64) pm += kr[k] * wl[k];
    pm = wave_sum(pm);
    if (eps && a.z[c])
        for (int r = lane; r <= q; r += 64) sum += lr[r] * eps[(size_t)r * a.B + b0 + l];
    sum = wave_sum(sum);
    if (lane == 0) {
        const size_t o = (size_t)q * a.B + b0 + l;
        a.p_m[c][o] = pm;
        if (a.z[c]) a.z[c][o] = eps ? pm + sum : pm;
    }
    if (a.chol[c]) {
        real* o = a.chol[c] + ((size_t)(b0 + l) * Q + q) * Q;
        for (int r = lane; r < Q; r += 64) o[r] = lr[r];       // svgp_potrf_batched zeroed the strict upper triangle
    }
}

// ---------------------------------------------------------------------------------------------------------
// one plan for the launch code and the route text
// ---------------------------------------------------------------------------------------------------------
// calls f(step) for every launch group of one call, in order; stops at the first non-zero return
template <class F>
int bpj_walk(const svgp_ball_predict_joint_cfg* g, bool large, F f) {
    int rc;
    if (!large) return f(BpStep{BPJ_FUSED, 0, 0, g->B, 0, g->Q});
    const int chunk = bpj_chunk(g->B, g->Q);
    for (int c = 0; c < 2; ++c) {
        if ((rc = f(BpStep{BP_KMAT, c, 0, 0, 0, 0}))) return rc;
        for (int b0 = 0; b0 < g->B; b0 += chunk) {
            const int nb = g->B - b0 < chunk ? g->B - b0 : chunk;
            if ((rc = bp_walk_factors(c, b0, nb, f))) return rc;
            if ((rc = bpj_walk_tail(c, b0, nb, g->Q, f))) return rc;
        }
    }
    return SVGP_OK;
}

int bpj_check(const svgp_ball_predict_joint_cfg* g, bool large) {
    const char* name = large ? "svgp_ball_predict_joint_large" : "svgp_ball_predict_joint";
    SVGP_REQUIRE(g != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(g->B >= 1 && g->T >= 1 && g->m >= 1 && g->Q >= 1, SVGP_ERR_INVALID, "need B, T, m, Q >= 1 (B=%d T=%d m=%d Q=%d)", g->B,
                 g->T, g->m, g->Q);
    SVGP_REQUIRE(g->path_jitter >= 0, SVGP_ERR_INVALID, "need path_jitter >= 0 (%g)", g->path_jitter);
    const int m_max = large ? SVGP_M_LIMIT : BP_M_MAX, t_max = large ? BPL_T_MAX : BP_T_MAX, q_max = large ? BPJL_Q_MAX : BPJ_Q_MAX;
    SVGP_REQUIRE(g->m <= m_max, SVGP_ERR_UNSUPPORTED, "m=%d: %s takes m <= %d", g->m, name, m_max);
    SVGP_REQUIRE(g->T <= t_max, SVGP_ERR_UNSUPPORTED, "T=%d: %s takes T <= %d", g->T, name, t_max);
    SVGP_REQUIRE(g->Q <= q_max, SVGP_ERR_UNSUPPORTED, "Q=%d: %s takes Q <= %d", g->Q, name, q_max);
    return SVGP_OK;
}

int bpj_args(const svgp_ball_predict_joint_cfg* g, const svgp_ball_predict_joint_bufs* q, BpjArgs* a) {
    int rc = bp_marshal(g, q, true, true, a);
    if (rc) return rc;
    a->jp = g->path_jitter; a->cov[0] = q->cov_x; a->cov[1] = q->cov_y; a->chol[0] = q->chol_x; a->chol[1] = q->chol_y;
    return SVGP_OK;
}

struct BpjWork { BpFactorWork f; BpjTailWork t; int64_t total; };
BpjWork bpj_work(const svgp_ball_predict_joint_cfg* g) {
    const int64_t nb = bpj_chunk(g->B, g->Q);
    SvgpTake16 c16;
    BpjWork o;
    o.f = bp_factor_work(c16, g->m, g->T, nb);
    o.t = bpj_tail_work(c16, g->m, g->Q, nb);
    o.total = c16.p;
    return o;
}

template <int CW>
int bpj_launch_fused(const BpjArgs& a, void* stream) {
    const size_t lds = bpj_lds_bytes(a.m, a.Q, CW);
    SVGP_REQUIRE(lds <= SVGP_LDS_MAX_BYTES, SVGP_ERR_UNSUPPORTED, "m=%d Q=%d needs %zu bytes of LDS", a.m, a.Q, lds);
    int rc = set_dyn_lds(k_ball_predict_joint<CW>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ball_predict_joint<CW>, dim3((unsigned)a.B, 2), dim3(256), lds, (hipStream_t)stream, a, bpj_slot1(a.m, a.Q),
                       bpj_slot2(a.m, a.Q));
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

}  // namespace

BpjTailWork bpj_tail_work(SvgpTake16& c16, int64_t m, int64_t Q, int64_t nb) {
    BpjTailWork o;
    o.K2 = c16.take(m * m); o.Kq = c16.take(Q * m); o.kbb = c16.take(Q);
    o.G = c16.take(nb * Q * m); o.Cb = c16.take(nb * Q * Q); o.logdet = c16.take(nb);
    o.potrf = c16.take((int64_t)svgp_potrf_workspace_elems((int)Q, (int)nb));
    return o;
}

int bpj_tail_launch(const BpjArgs& a, const BpStep& s, const BpjTailWork& w, const real* X, long long xstride, const real* W, double* work,
                    void* stream) {
    const int c = s.c, nb = s.nb, m = a.m, Q = a.Q;
    const long long QQ = (long long)Q * Q, Qm = (long long)Q * m;
    hipStream_t st = (hipStream_t)stream;
    switch (s.op) {
    case BPJ_KQ:
        return svgp_se1d_kernel_matrix_fwd(Q, m, a.tq, a.ip[c], a.ls[c], work + w.K2, work + w.Kq, work + w.kbb, stream);
    case BPJ_G:         // G_l (Q, m) = k X_l: the shared k has stride 0
        return svgp_dgemm_batched(0, 0, Q, m, m, 1.0, work + w.Kq, m, 0, X, m, xstride, 0.0, work + w.G, m, Qm, nb, stream);
    case BPJ_GK:        // (Q, Q) = G_l k^T
        return svgp_dgemm_batched(0, 1, Q, Q, m, 1.0, work + w.G, m, Qm, work + w.Kq, m, 0, 0.0, work + w.Cb, Q, QQ, nb, stream);
    case BPJ_COV:
        hipLaunchKernelGGL(k_bpj_cov, dim3(svgp_blocks(nb * QQ)), dim3(SVGP_BLOCK), 0, st, a, c, s.b0, nb, work + w.Cb);
        SVGP_LAUNCH_CHECK();
        break;
    case BPJ_POTRF:
        // with its panel solves refined: the residual of Lc Lc^T then stays at the level of an unblocked factorisation beyond Q = 64 too
        return svgp_potrf_batched_refined(Q, nb, work + w.Cb, Q, QQ, work + w.logdet, work + w.potrf, stream);
    case BPJ_FINISH:
        hipLaunchKernelGGL(k_bpj_finish, dim3((unsigned)(((long long)nb * Q + SVGP_BLOCK / 64 - 1) / (SVGP_BLOCK / 64))), dim3(SVGP_BLOCK), 0, st,
                           a, c, s.b0, nb, work + w.Kq, W, work + w.Cb);
        SVGP_LAUNCH_CHECK();
        break;
    default:
        SVGP_REQUIRE(false, SVGP_ERR_INVALID, "bpj_tail_launch: op %d is not a step of the joint tail", (int)s.op);
    }
    return SVGP_OK;
}

extern "C" int svgp_ball_predict_joint_route(const svgp_ball_predict_joint_cfg* g, int large, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = bpj_check(g, large != 0);
    if (rc) return rc;
    int pos = 0;
    buf[0] = 0;
    return bpj_walk(g, large != 0, [&](const BpStep& s) -> int { return bp_route_line(s, g->m, buf, cap, &pos); });
}

extern "C" int svgp_ball_predict_joint(const svgp_ball_predict_joint_cfg* g, const svgp_ball_predict_joint_bufs* q, void* stream) {
    int rc = bpj_check(g, false);
    if (rc) return rc;
    BpjArgs a;
    rc = bpj_args(g, q, &a);
    if (rc) return rc;
    return bpj_walk(g, false, [&](const BpStep&) -> int { return a.m <= 32 ? bpj_launch_fused<32>(a, stream) : bpj_launch_fused<64>(a, stream); });
}

extern "C" long long svgp_ball_predict_joint_large_workspace_elems(const svgp_ball_predict_joint_cfg* g) {
    if (bpj_check(g, true)) return 0;
    return bpj_work(g).total;
}

extern "C" int svgp_ball_predict_joint_large(const svgp_ball_predict_joint_cfg* g, const svgp_ball_predict_joint_bufs* q, double* work,
                                             void* stream) {
    int rc = bpj_check(g, true);
    if (rc) return rc;
    BpjArgs a;
    rc = bpj_args(g, q, &a);
    if (rc) return rc;
    const BpjWork w = bpj_work(g);
    SVGP_REQUIRE(work != nullptr, SVGP_ERR_INVALID, "work is NULL (B = %d, T = %d, m = %d, Q = %d needs %lld doubles)", g->B, g->T, g->m,
                 g->Q, (long long)w.total);
    return bpj_walk(g, true, [&](const BpStep& s) -> int {
        switch (s.op) {
        case BPJ_KQ: case BPJ_G: case BPJ_GK: case BPJ_COV: case BPJ_POTRF: case BPJ_FINISH:
            return bpj_tail_launch(a, s, w.t, work + w.f.Mats, (long long)a.m * a.m, work + w.f.W, work, stream);
        default:            // BP_KMAT and the seven factor steps; anything else is refused there
            return bp_factor_launch(a, s, w.f, work, stream);
        }
    });
}
