// Exact per-video GP regression of the Pearce baselines (build_1d_gp, GPVAE_Pearce_model.py:8-86, X_test = X) for videos
// longer than the LDS kernels of ball.hip hold (k_pearce_fwd / k_pearce_bwd: n <= 64): every n x n matrix stays in global
// memory, the only n^3 work of the forward pass is svgp_spd_inverse_batched and the only n^3 work of the reverse pass is one
// svgp_dgemm_batched, needed for the length-scale gradient alone.  1 <= n <= T <= 2048.
//
// With A = K + S, S = diag(s), K_ii = 1, Ai = A^-1 (so K = A - S):
//   alpha = Ai y        p_m = K alpha = y - s o alpha        p_v = 1 - diag(K Ai K) = s - s^2 o diag(Ai)
//   lhood = -1/2 (n log 2pi + y.alpha + log det A)
// Reverse, g_m / g_v the seeds on p_m / p_v (cross-entropy term + sample z = p_m + eps sqrt(p_v)), gl = gT seed_lh_scale:
//   alphabar = -s o g_m      w = Ai alphabar      D = diag(s^2 g_v)
//   Abar = 1/2 gl (alpha alpha^T - Ai) - w alpha^T + Ai D Ai
//   ybar  = g_m + (CE term) + w - gl alpha
//   s2bar = diag(Abar) - g_m o alpha + g_v (1 - 2 s o diag(Ai)) + (CE term),     diag(Ai D Ai)_i = sum_k D_k Ai_ik^2
//   d_ls  = sum_ij Abar_ij K_ij (t_i - t_j)^2 / l^3
// K enters through A only, so without the length-scale gradient nothing needs Ai D Ai in full: the reverse pass is then ONE read
// of Ai per matrix.  A context set (idx != NULL) produces lhood only: Abar = 1/2 gl (alpha alpha^T - Ai), no product.
//
// One wave per matrix row everywhere (lane k, k + 64, ... of the row: 512-byte coalesced reads), the wave sum is the fixed
// shuffle tree of wave_sum, sums over rows run in a second launch in fixed order: no float atomics, bitwise reproducible.
// Ai is read by rows only and never mirrored (see k_symmetrize in linalg.hip).
#include "common.hpp"

namespace {

struct LongArgs {
    int B, T, n, use_rng, full, want_dls, accumulate;
    const real* times; const int* idx; const real* tmask;
    const real* ls[2];
    const real* y[2]; const real* s2[2];
    const real* eps_in[2]; const real* state;
    real* Ai;                                    // (2, B, n, n): A, inverted in place
    real* alpha;                                 // (2, B, n)
    real* p_m[2]; real* p_v[2]; real* eps[2]; real* z[2];
    real* lh; real* ce; real* row_ce;
    const real* zbar[2];
    real* ybar[2]; real* s2bar[2];
    real* dl_part;                               // (2, B)
    real seed_lh_scale;
    // workspace: (2B) log det; (2B, n) gathered y / times, alphabar, diag(D), w, row partials of d_ls; the inverse's scratch;
    // (2B, n, n) D Ai and Ai D Ai
    real* logdet; real* yv; real* tv; real* ab; real* dv; real* wv; real* dlrow; real* inv; real* DA; real* P;
};

__device__ __forceinline__ int long_frame(const LongArgs& a, int b, int i) {
    return a.idx ? a.idx[(size_t)b * a.n + i] : i;
}

// (a) A = K_SE(l) + diag(s2) for all 2B matrices, straight into the buffer the inverse works on; the diagonal thread also
// gathers y into the contiguous (2B, n) vector the row pass reads
__global__ __launch_bounds__(256) void k_long_build(LongArgs a) {
    const int n = a.n, mt = blockIdx.y, c = mt / a.B, b = mt - c * a.B;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n * n) return;
    const int i = o / n, j = o - i * n;
    const int fi = long_frame(a, b, i), fj = long_frame(a, b, j);
    const real l = *a.ls[c], il2 = real(-0.5) / (l * l);
    const real d = a.times[fi] - a.times[fj];
    real v = exp(d * d * il2);
    if (i == j) {
        const size_t e = (size_t)fi * a.B + b;
        v += a.s2[c][e];
        a.yv[(size_t)mt * n + i] = a.y[c][e];
    }
    a.Ai[(size_t)mt * n * n + o] = v;
}

// (b) forward row pass: alpha_i = Ai_i. y; full set: p_m, p_v, eps, z and the frame's cross-entropy term
__global__ __launch_bounds__(256) void k_long_fwd_rows(LongArgs a) {
    const int n = a.n, mt = blockIdx.y, c = mt / a.B, b = mt - c * a.B;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const real* row = a.Ai + (size_t)mt * n * n + (size_t)i * n;
    const real* yv = a.yv + (size_t)mt * n;
    real s = 0;
#pragma unroll 4
    for (int k = lane; k < n; k += 64) s += row[k] * yv[k];
    s = wave_sum(s);
    if (lane != 0) return;
    a.alpha[(size_t)mt * n + i] = s;
    if (!a.full) return;
    const size_t e = (size_t)i * a.B + b;
    const real s2 = a.s2[c][e], yi = yv[i];
    const real pm = yi - s2 * s, pv = s2 - s2 * s2 * row[i];
    const real ep = a.use_rng ? svgp_philox_normal((unsigned long long)a.state[SVGP_ST_RNG_CTR],
                                                   (unsigned long long)(e * 2 + c))
                              : a.eps_in[c][e];
    a.p_m[c][e] = pm; a.p_v[c][e] = pv; a.eps[c][e] = ep; a.z[c][e] = pm + ep * sqrt(pv);
    const real p = recip_no_nan(s2), dm = pm - yi;
    a.row_ce[((size_t)c * a.T + i) * a.B + b] = real(0.5) * (real(SVGP_LOG_2PI) + log(s2) + (pv + dm * dm) * p);
}

// one workgroup per matrix: lhood and the sum of the cross-entropy terms
__global__ __launch_bounds__(256) void k_long_fwd_reduce(LongArgs a) {
    __shared__ real red[16];
    const int n = a.n, mt = blockIdx.x, c = mt / a.B, b = mt - c * a.B;
    real quad = 0, ce = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        quad += a.yv[(size_t)mt * n + i] * a.alpha[(size_t)mt * n + i];
        if (a.full) ce += a.row_ce[((size_t)c * a.T + i) * a.B + b];
    }
    quad = block_sum(quad, red);
    ce = block_sum(ce, red);
    if (threadIdx.x != 0) return;
    a.lh[mt] = real(-0.5) * ((real)n * real(SVGP_LOG_2PI) + quad + a.logdet[mt]);
    if (a.full) a.ce[mt] = ce;
}

// seeds on p_m / p_v of frame i of the full set, as k_pearce_bwd forms them; gC = seed of the frame's cross-entropy term
struct LongSeed { real g_m, g_v, gC, s2, p, dm, pv; };
__device__ __forceinline__ LongSeed long_seed(const LongArgs& a, int c, int b, int i, real gT) {
    LongSeed q;
    const size_t e = (size_t)i * a.B + b;
    q.s2 = a.s2[c][e]; q.p = recip_no_nan(q.s2); q.pv = a.p_v[c][e]; q.dm = a.p_m[c][e] - a.y[c][e];
    const real zb = a.zbar[c][e];
    q.gC = gT * (a.tmask ? a.tmask[(size_t)b * a.T + i] : real(1));
    q.g_v = real(0.5) * q.gC * q.p + zb * a.eps[c][e] / (real(2) * sqrt(q.pv));
    q.g_m = q.gC * q.p * q.dm + zb;
    return q;
}

// reverse, O(n) per matrix: the gathered times; full set: alphabar = -s o g_m and diag(D) = s^2 g_v
__global__ __launch_bounds__(256) void k_long_bwd_prep(LongArgs a) {
    const int n = a.n, mt = blockIdx.y, c = mt / a.B, b = mt - c * a.B;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    a.tv[(size_t)mt * n + i] = a.times[long_frame(a, b, i)];
    if (!a.full) return;
    const LongSeed q = long_seed(a, c, b, i, svgp_seed_T(0, a.B, a.state));
    a.ab[(size_t)mt * n + i] = -q.s2 * q.g_m;
    a.dv[(size_t)mt * n + i] = q.s2 * q.s2 * q.g_v;
}

// (c) reverse row pass, one read of Ai.  Full set: w_i = Ai_i. alphabar and sum_k D_k Ai_ik^2 together (+ the row D_i Ai_i.
// of the product's operand when the length-scale gradient is wanted) -> ybar, s2bar.  Context set: Abar = 1/2 gl (alpha alpha^T
// - Ai) needs no product, so its row of the d_ls sum is formed here too; ybar / s2bar scatter through idx.
__global__ __launch_bounds__(256) void k_long_bwd_rows(LongArgs a) {
    const int n = a.n, mt = blockIdx.y, c = mt / a.B, b = mt - c * a.B;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t ov = (size_t)mt * n;
    const real* row = a.Ai + ov * n + (size_t)i * n;
    const real gT = svgp_seed_T(0, a.B, a.state), gl = gT * a.seed_lh_scale;
    const real al_i = a.alpha[ov + i];
    real w = 0, q2 = 0, dl = 0;
    if (a.full) {
        const real* ab = a.ab + ov;
        const real* dv = a.dv + ov;
        if (a.want_dls) {
            real* da = a.DA + ov * n + (size_t)i * n;
            const real di = dv[i];
#pragma unroll 4
            for (int k = lane; k < n; k += 64) {
                const real r = row[k];
                w += r * ab[k]; q2 += dv[k] * r * r; da[k] = di * r;
            }
        } else {
#pragma unroll 4
            for (int k = lane; k < n; k += 64) {
                const real r = row[k];
                w += r * ab[k]; q2 += dv[k] * r * r;
            }
        }
        w = wave_sum(w); q2 = wave_sum(q2);
    } else {
        const real l = *a.ls[c], il2 = real(-0.5) / (l * l), il3 = real(1) / (l * l * l);
        const real* al = a.alpha + ov;
        const real* tv = a.tv + ov;
        const real ti = tv[i];
        for (int k = lane; k < n; k += 64) {
            const real d = ti - tv[k], d2 = d * d;
            dl += real(0.5) * gl * (al_i * al[k] - row[k]) * exp(d2 * il2) * d2 * il3;
        }
        dl = wave_sum(dl);
    }
    if (lane != 0) return;
    const real aii = row[i];
    real sb = real(0.5) * gl * (al_i * al_i - aii), yb = -gl * al_i;
    if (a.full) {
        const LongSeed q = long_seed(a, c, b, i, gT);
        sb += q2 - w * al_i - q.g_m * al_i + q.g_v * (real(1) - real(2) * q.s2 * aii) +
              real(0.5) * q.gC * (q.p - (q.pv + q.dm * q.dm) * q.p * q.p);
        yb += q.g_m - q.gC * q.p * q.dm + w;
        a.wv[ov + i] = w;
    } else {
        a.dlrow[ov + i] = dl;
    }
    const size_t e = (size_t)long_frame(a, b, i) * a.B + b;
    if (a.accumulate) { a.s2bar[c][e] += sb; a.ybar[c][e] += yb; }
    else { a.s2bar[c][e] = sb; a.ybar[c][e] = yb; }
}

// (d) full set with the length-scale gradient: row i of sum_ij Abar_ij K_ij (t_i - t_j)^2 / l^3; Ai and P = Ai D Ai read once
__global__ __launch_bounds__(256) void k_long_dls_rows(LongArgs a) {
    const int n = a.n, mt = blockIdx.y, c = mt / a.B;
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t ov = (size_t)mt * n;
    const real* row = a.Ai + ov * n + (size_t)i * n;
    const real* prow = a.P + ov * n + (size_t)i * n;
    const real* al = a.alpha + ov;
    const real* tv = a.tv + ov;
    const real gl = svgp_seed_T(0, a.B, a.state) * a.seed_lh_scale;
    const real l = *a.ls[c], il2 = real(-0.5) / (l * l), il3 = real(1) / (l * l * l);
    const real al_i = al[i], w_i = a.wv[ov + i], ti = tv[i];
    real dl = 0;
    for (int k = lane; k < n; k += 64) {
        const real d = ti - tv[k], d2 = d * d;
        const real abar = real(0.5) * gl * (al_i * al[k] - row[k]) - w_i * al[k] + prow[k];
        dl += abar * exp(d2 * il2) * d2 * il3;
    }
    dl = wave_sum(dl);
    if (lane == 0) a.dlrow[ov + i] = dl;
}

// one workgroup per coordinate: rows, then videos, in fixed order -> dl_part (2, B) and d_ls[c] (+)= sum_b dl_part[c][b]
__global__ __launch_bounds__(256) void k_long_dl_final(int B, int n, int accumulate, const real* __restrict__ dlrow,
                                                       real* __restrict__ part, real* dl_x, real* dl_y) {
    __shared__ real red[16];
    const int c = blockIdx.x;
    real tot = 0;
    for (int b = 0; b < B; ++b) {
        const real* r = dlrow + ((size_t)c * B + b) * n;
        real s = 0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) s += r[i];
        s = block_sum(s, red);
        if (threadIdx.x == 0) { part[c * B + b] = s; tot += s; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    real* o = c ? dl_y : dl_x;
    *o = accumulate ? *o + tot : tot;
}

}  // namespace

#define REQ_PTRS(...)                                                                             \
    do {                                                                                          \
        const void* ps_[] = {__VA_ARGS__};                                                        \
        for (const void* q_ : ps_) SVGP_REQUIRE(q_ != nullptr, SVGP_ERR_INVALID, "NULL device pointer"); \
    } while (0)

#define LONG_T_MAX SVGP_M_LIMIT

// work: [log det (2B) | six (2B, n) vectors | the inverse's scratch | want_dls: D Ai and Ai D Ai, (2B, n, n) each]
extern "C" size_t svgp_pearce_long_workspace_elems(int B, int T, int n, int want_dls) {
    if (B < 1 || B > 32767 || T < 1 || T > LONG_T_MAX || n < 1 || n > T) return 0;
    return (size_t)2 * B + (size_t)6 * 2 * B * n + svgp_spd_inverse_workspace_elems(n, 2 * B) +
           (want_dls ? (size_t)2 * 2 * B * n * n : 0);
}

static int long_args(const svgp_pearce_bufs* q, double* work, LongArgs* a) {
    SVGP_REQUIRE(q != nullptr, SVGP_ERR_INVALID, "bufs is NULL");
    SVGP_REQUIRE(q->B >= 1 && q->B <= 32767 && q->T >= 1 && q->n >= 1 && q->n <= q->T, SVGP_ERR_INVALID,
                 "bad shape B=%d T=%d n=%d (need 1 <= n <= T, 1 <= B <= 32767)", q->B, q->T, q->n);
    SVGP_REQUIRE(q->T <= LONG_T_MAX, SVGP_ERR_UNSUPPORTED, "T=%d: the global-memory exact GP accepts T <= %d", q->T, LONG_T_MAX);
    SVGP_REQUIRE(q->idx != nullptr || q->n == q->T, SVGP_ERR_INVALID, "n != T needs an index set");
    REQ_PTRS(q->times, q->ls_x, q->ls_y, q->y_x, q->y_y, q->s2_x, q->s2_y, q->Ai, q->alpha, q->lh, work);
    memset(a, 0, sizeof(*a));
    a->B = q->B; a->T = q->T; a->n = q->n; a->times = q->times; a->idx = q->idx; a->tmask = q->tmask;
    a->full = q->idx == nullptr;
    a->ls[0] = q->ls_x; a->ls[1] = q->ls_y; a->y[0] = q->y_x; a->y[1] = q->y_y; a->s2[0] = q->s2_x; a->s2[1] = q->s2_y;
    a->p_m[0] = q->p_m_x; a->p_m[1] = q->p_m_y; a->p_v[0] = q->p_v_x; a->p_v[1] = q->p_v_y;
    a->eps[0] = q->eps_x; a->eps[1] = q->eps_y; a->z[0] = q->z_x; a->z[1] = q->z_y;
    a->zbar[0] = q->zbar_x; a->zbar[1] = q->zbar_y; a->ybar[0] = q->ybar_x; a->ybar[1] = q->ybar_y;
    a->s2bar[0] = q->s2bar_x; a->s2bar[1] = q->s2bar_y;
    a->Ai = q->Ai; a->alpha = q->alpha; a->lh = q->lh; a->ce = q->ce; a->row_ce = q->row_ce; a->dl_part = q->dl_part;
    const size_t vec = (size_t)2 * a->B * a->n;
    real* w = work;
    a->logdet = w; w += 2 * a->B;
    a->yv = w; w += vec; a->tv = w; w += vec; a->ab = w; w += vec; a->dv = w; w += vec; a->wv = w; w += vec;
    a->dlrow = w; w += vec;
    a->inv = w; w += svgp_spd_inverse_workspace_elems(a->n, 2 * a->B);
    a->DA = w; a->P = w + vec * a->n;           // there only when the workspace was sized with want_dls
    return SVGP_OK;
}

static inline dim3 long_row_grid(const LongArgs& a) { return dim3((a.n + 3) / 4, 2 * a.B); }

extern "C" int svgp_pearce_long_fwd(const svgp_pearce_bufs* q, const double* eps_x, const double* eps_y, const double* state,
                                    double* work, void* stream) {
    LongArgs a;
    int rc = long_args(q, work, &a);
    if (rc) return rc;
    if (a.full) {
        REQ_PTRS(q->p_m_x, q->p_m_y, q->p_v_x, q->p_v_y, q->eps_x, q->eps_y, q->z_x, q->z_y, q->ce, q->row_ce, state);
        SVGP_REQUIRE((eps_x == nullptr) == (eps_y == nullptr), SVGP_ERR_INVALID, "give both eps or neither");
    }
    a.eps_in[0] = eps_x; a.eps_in[1] = eps_y; a.use_rng = eps_x == nullptr; a.state = state;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_long_build, dim3((a.n * a.n + 255) / 256, 2 * a.B), dim3(256), 0, s, a);
    SVGP_LAUNCH_CHECK();
    rc = svgp_spd_inverse_batched(a.n, 2 * a.B, a.Ai, a.logdet, a.inv, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_long_fwd_rows, long_row_grid(a), dim3(256), 0, s, a);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_long_fwd_reduce, dim3(2 * a.B), dim3(256), 0, s, a);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_pearce_long_bwd(const svgp_pearce_bufs* q, double seed_lh_scale, int accumulate, int want_dls,
                                    const double* state, double* d_ls_x, double* d_ls_y, double* work, void* stream) {
    LongArgs a;
    int rc = long_args(q, work, &a);
    if (rc) return rc;
    REQ_PTRS(q->ybar_x, q->ybar_y, q->s2bar_x, q->s2bar_y, state);
    if (a.full) REQ_PTRS(q->p_m_x, q->p_m_y, q->p_v_x, q->p_v_y, q->eps_x, q->eps_y, q->zbar_x, q->zbar_y);
    a.want_dls = a.full ? (want_dls != 0) : 1;          // a context set's d_ls costs no product: always formed
    if (a.want_dls) REQ_PTRS(q->dl_part, d_ls_x, d_ls_y);
    a.state = state; a.seed_lh_scale = seed_lh_scale; a.accumulate = accumulate;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_long_bwd_prep, dim3((a.n + 255) / 256, 2 * a.B), dim3(256), 0, s, a);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_long_bwd_rows, long_row_grid(a), dim3(256), 0, s, a);
    SVGP_LAUNCH_CHECK();
    if (!a.want_dls) return SVGP_OK;
    if (a.full) {
        const long long nn = (long long)a.n * a.n;
        rc = svgp_dgemm_batched(0, 0, a.n, a.n, a.n, 1.0, a.Ai, a.n, nn, a.DA, a.n, nn, 0.0, a.P, a.n, nn, 2 * a.B, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_long_dls_rows, long_row_grid(a), dim3(256), 0, s, a);
        SVGP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_long_dl_final, dim3(2), dim3(256), 0, s, a.B, a.n, accumulate, a.dlrow, a.dl_part, d_ls_x, d_ls_y);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}
