// Moving-ball exact-GP baselines after training: the exact per-video GP posterior of build_1d_gp
// (GPVAE_Pearce_model.py:8-86) at ARBITRARY query times X_test, from the frames that were observed.  Per video b and latent
// coordinate c, with SE(s, t) = exp(-(s - t)^2 / (2 l_c^2)) and O the kept frames of the video (mask != 0; n of them):
//   A     = SE(t_O, t_O) + diag(var_O)                 (n x n; no jitter, as in the reference)
//   alpha = A^-1 mu_O          lh = -1/2 (n log 2pi + mu_O . alpha + log det A)
//   k_q   = SE(tq_q, t_O)      p_m = k_q . alpha       p_v = 1 - k_q^T A^-1 k_q        z = p_m + eps sqrt(max(p_v, 0))
// A dropped frame is absent: its mu / var are never read.  n = 0 gives the prior, p_m = 0, p_v = 1, lh = 0.  p_v is reported as
// computed; the reference takes sqrt(p_v) unguarded, the max(., 0) applies to the sample only.
//
// svgp_pearce_predict (T <= 64): ONE launch, grid (B, 2, S), 256 threads.  Wave 0 compacts the kept frames (ballot + popcount),
// the workgroup builds A in LDS (n x (n + 1)), inverts it in place with lds_spd_inverse (log det comes with it) and forms alpha;
// then a wave per query time of the workgroup's slice: lane i holds k_i and column i of A^-1 (= row i up to rounding; lanes read
// consecutive LDS addresses), k is broadcast through the wave's LDS line, both reductions are wave_sum.  A query's bits depend on
// neither its position in tq nor S; every slice repeats the inverse (at most 64^3 operations), slice 0 writes lh.
//
// svgp_pearce_predict_long (T <= 2048): the same quantities from the library's global-memory pieces, both coordinates of
// PPL_NB videos per chunk and PPL_QC query rows per chunk, so the workspace grows with neither B nor Q (pp_walk is the one plan
// of the launch code and of svgp_pearce_predict_route).  The chunk's matrices are the masked full-size A: the rows / columns of
// dropped frames are those of the identity, which leaves log det and the inverse of the kept block as they are.
#include "common.hpp"
#include "lds_spd_inverse.hpp"

namespace {

constexpr int PP_T_MAX = 64, PPL_T_MAX = SVGP_M_LIMIT;
constexpr int PP_WG_TARGET = 512;    // workgroups the slice plan aims for: two per CU
constexpr int PP_S_MAX = 65535;      // gridDim.z
constexpr int PPL_NB = 8;            // videos of a chunk of the long form (2 PPL_NB matrices)
constexpr int PPL_QC = 512;          // query rows of a chunk of the long form

struct PpArgs {
    int B, T, Q;
    const real* times; const real* tq; const real* mask;
    const real* ls[2]; const real* mu[2]; const real* var[2]; const real* eps[2];
    real* p_m[2]; real* p_v[2]; real* z[2]; real* lh;
};

__device__ __forceinline__ bool pp_kept(const PpArgs& a, int t, int b) {
    return a.mask ? a.mask[(size_t)t * a.B + b] != real(0) : true;
}
__device__ __forceinline__ void pp_write(const PpArgs& a, int c, size_t e, real pm, real qs) {
    const real pv = real(1) - qs;
    a.p_m[c][e] = pm; a.p_v[c][e] = pv;
    if (a.z[c]) a.z[c][e] = a.eps[c] ? pm + a.eps[c][e] * sqrt(pv > real(0) ? pv : real(0)) : pm;
}

// Thread layout of the build as in lds_spd_inverse: column j = tid & (CW - 1), row lane i0 = tid / CW; a thread owns (i0 + RL r, j).
template <int CW>
__global__ __launch_bounds__(256) void k_pearce_predict(PpArgs a) {
    extern __shared__ __align__(16) real smem[];
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x, c = blockIdx.y, B = a.B, T = a.T;
    real* tO = smem;                 // 64 : times of the kept frames
    real* yO = tO + 64;              // 64 : their mu
    real* vO = yO + 64;              // 64 : their var
    real* al = vO + 64;              // 64 : alpha
    real* piv = al + 64;             // 64 : pivots of the sweep
    real* kl = piv + 64;             // 4 x 64 : one line of k per wave
    real* cnt = kl + 256;            // 8 : n
    real* A = cnt + 8;               // n x (n + 1)
    const real* __restrict__ tq = a.tq;
    const real l = *a.ls[c], il2 = real(-0.5) / (l * l);
    if (tid < 64) {                  // T <= 64: one wave sees every frame
        const bool keep = lane < T && pp_kept(a, lane, b);
        const unsigned long long kept = __ballot(keep);
        if (keep) {
            const int pos = __popcll(kept & ((1ull << lane) - 1ull));
            const size_t e = (size_t)lane * B + b;
            tO[pos] = a.times[lane]; yO[pos] = a.mu[c][e]; vO[pos] = a.var[c][e];
        }
        if (lane == 0) cnt[0] = (real)__popcll(kept);
    }
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane((int)cnt[0]), ld = n + 1;      // the same in every lane: scalar loop bounds
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < n && j < n) {
            const real d = tO[i] - tO[j];
            real v = exp(d * d * il2);
            if (i == j) v += vO[i];
            A[i * ld + j] = v;
        }
    }
    const real logdet = lds_spd_inverse<CW>(A, ld, n, piv);
    if (tid < 64) {
        real s = 0;
        if (tid < n) {
#pragma unroll 4
            for (int k = 0; k < n; ++k) s += A[k * ld + tid] * yO[k];
        }
        al[tid] = s;
        const real quad = wave_sum(tid < n ? yO[tid] * s : real(0));
        if (tid == 0 && blockIdx.z == 0 && a.lh)
            a.lh[(size_t)c * B + b] = n ? real(-0.5) * ((real)n * real(SVGP_LOG_2PI) + quad + logdet) : real(0);
    }
    __syncthreads();
    // ---- the slice's query times: a wave each, four per round
    const int S = gridDim.z, sl = blockIdx.z;
    const int q_lo = (int)((long long)sl * a.Q / S), q_hi = (int)((long long)(sl + 1) * a.Q / S);
    real* kw = kl + wv * 64;
    const real ali = lane < n ? al[lane] : real(0);
    for (int q0 = q_lo; q0 < q_hi; q0 += 4) {
        const int q = q0 + wv;
        const bool live = q < q_hi;
        real ki = 0;
        if (live && lane < n) { const real d = tq[q] - tO[lane]; ki = exp(d * d * il2); }
        __syncthreads();             // the previous round's lines are consumed
        kw[lane] = ki;
        __syncthreads();
        real row = 0;
        if (lane < n) {
#pragma unroll 4
            for (int k = 0; k < n; ++k) row += A[k * ld + lane] * kw[k];
        }
        const real pm = wave_sum(ki * ali), qs = wave_sum(ki * row);
        if (live && lane == 0) pp_write(a, c, (size_t)q * B + b, pm, qs);
    }
}

inline size_t pp_lds_bytes(int T) { return ((size_t)T * (T + 1) + 5 * 64 + 256 + 8) * sizeof(real); }
static_assert(((size_t)64 * 65 + 5 * 64 + 256 + 8) * sizeof(real) <= 64 * 1024, "no opt-in for the dynamic LDS at T = 64");

// ---------------------------------------------------------------------------------------------------------
// the long form's own kernels; matrix mt = c nb + l of a chunk is coordinate c of video b0 + l
// ---------------------------------------------------------------------------------------------------------
struct PlChunk { int b0, nb, q0, nq; real* Am; real* yv; real* alpha; real* logdet; real* Kq; real* R; };

// the masked full-size A (2 nb, T, T) and, by the diagonal threads, mu with the dropped frames zeroed (2 nb, T)
__global__ __launch_bounds__(SVGP_BLOCK) void k_pp_build(PpArgs a, PlChunk h) {
    const int T = a.T, mt = blockIdx.y, c = mt / h.nb, b = h.b0 + mt - c * h.nb;
    const int o = blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (o >= T * T) return;
    const int i = o / T, j = o - i * T;
    const bool ki = pp_kept(a, i, b), kj = i == j ? ki : pp_kept(a, j, b);
    real v = 0;
    if (ki && kj) {
        const real l = *a.ls[c], d = a.times[i] - a.times[j];
        v = exp(d * d * (real(-0.5) / (l * l)));
    }
    if (i == j) {
        const size_t e = (size_t)i * a.B + b;
        v = ki ? v + a.var[c][e] : real(1);
        h.yv[(size_t)mt * T + i] = ki ? a.mu[c][e] : real(0);
    }
    h.Am[(size_t)mt * T * T + o] = v;
}

// alpha_i = Ai_i. y, one wave per row (a dropped frame's row is that of the identity: alpha_i = 0)
__global__ __launch_bounds__(256) void k_pp_alpha(PpArgs a, PlChunk h) {
    const int T = a.T, mt = blockIdx.y, lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= T) return;
    const real* row = h.Am + (size_t)mt * T * T + (size_t)i * T;
    const real* yv = h.yv + (size_t)mt * T;
    real s = 0;
#pragma unroll 4
    for (int k = lane; k < T; k += 64) s += row[k] * yv[k];
    s = wave_sum(s);
    if (lane == 0) h.alpha[(size_t)mt * T + i] = s;
}

// one workgroup per matrix: lh from y . alpha, log det A and the number of kept frames
__global__ __launch_bounds__(256) void k_pp_lh(PpArgs a, PlChunk h) {
    __shared__ real red[16];
    const int T = a.T, mt = blockIdx.x, c = mt / h.nb, b = h.b0 + mt - c * h.nb;
    real quad = 0, n = 0;
    for (int i = threadIdx.x; i < T; i += blockDim.x) {
        quad += h.yv[(size_t)mt * T + i] * h.alpha[(size_t)mt * T + i];
        n += pp_kept(a, i, b) ? real(1) : real(0);
    }
    quad = block_sum(quad, red);
    n = block_sum(n, red);
    if (threadIdx.x == 0)
        a.lh[(size_t)c * a.B + b] = n > real(0) ? real(-0.5) * (n * real(SVGP_LOG_2PI) + quad + h.logdet[mt]) : real(0);
}

// Kq (2 nb, nq, T): SE(tq, t) with the columns of dropped frames zeroed
__global__ __launch_bounds__(SVGP_BLOCK) void k_pp_kq(PpArgs a, PlChunk h) {
    const int T = a.T, mt = blockIdx.y, c = mt / h.nb, b = h.b0 + mt - c * h.nb;
    const long long o = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (o >= (long long)h.nq * T) return;
    const int q = (int)(o / T), t = (int)(o - (long long)q * T);
    real v = 0;
    if (pp_kept(a, t, b)) {
        const real l = *a.ls[c], d = a.tq[h.q0 + q] - a.times[t];
        v = exp(d * d * (real(-0.5) / (l * l)));
    }
    h.Kq[(size_t)mt * h.nq * T + o] = v;
}

// one wave per (matrix, query row): p_m = k . alpha, k^T Ai k = (k^T Ai) . k with R = Kq Ai; the draw
__global__ __launch_bounds__(256) void k_pp_finish(PpArgs a, PlChunk h) {
    const int T = a.T, mt = blockIdx.y, c = mt / h.nb, b = h.b0 + mt - c * h.nb;
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= h.nq) return;
    const real* kr = h.Kq + ((size_t)mt * h.nq + q) * T;
    const real* rr = h.R + ((size_t)mt * h.nq + q) * T;
    const real* al = h.alpha + (size_t)mt * T;
    real pm = 0, qs = 0;
#pragma unroll 4
    for (int t = lane; t < T; t += 64) { const real k = kr[t]; pm += k * al[t]; qs += k * rr[t]; }
    pm = wave_sum(pm); qs = wave_sum(qs);
    if (lane == 0) pp_write(a, c, (size_t)(h.q0 + q) * a.B + b, pm, qs);
}

// ---------------------------------------------------------------------------------------------------------
// one plan for the launch code and the route text
// ---------------------------------------------------------------------------------------------------------
enum PpOp { PP_FUSED, PP_BUILD, PP_INVERSE, PP_ALPHA, PP_LH, PP_KQ, PP_GEMM, PP_FINISH };
const char* const PP_NAME[] = {"k_pearce_predict", "k_pp_build", "svgp_spd_inverse_batched", "k_pp_alpha", "k_pp_lh", "k_pp_kq",
                               "svgp_dgemm_batched", "k_pp_finish"};
struct PpStep { PpOp op; int b0, nb, q0, nq, S; };

// query slices of the one-launch form: as many as bring the grid to PP_WG_TARGET workgroups, each with a round of four queries
int pp_slices(const svgp_pearce_predict_cfg* g) {
    if (g->q_slices > 0) return g->q_slices;
    const long long want = (PP_WG_TARGET + 2LL * g->B - 1) / (2LL * g->B), cap = (g->Q + 3) / 4;
    const long long s = want < cap ? want : cap;
    return (int)(s < 1 ? 1 : s);
}

// calls f(step) for every launch group of one call, in order; stops at the first non-zero return
template <class F>
int pp_walk(const svgp_pearce_predict_cfg* g, bool long_form, F f) {
    int rc;
    if (!long_form) return f(PpStep{PP_FUSED, 0, g->B, 0, g->Q, pp_slices(g)});
    for (int b0 = 0; b0 < g->B; b0 += PPL_NB) {
        const int nb = g->B - b0 < PPL_NB ? g->B - b0 : PPL_NB;
        for (PpOp op : {PP_BUILD, PP_INVERSE, PP_ALPHA, PP_LH})
            if ((rc = f(PpStep{op, b0, nb, 0, 0, 0}))) return rc;
        for (int q0 = 0; q0 < g->Q; q0 += PPL_QC) {
            const int nq = g->Q - q0 < PPL_QC ? g->Q - q0 : PPL_QC;
            for (PpOp op : {PP_KQ, PP_GEMM, PP_FINISH})
                if ((rc = f(PpStep{op, b0, nb, q0, nq, 0}))) return rc;
        }
    }
    return SVGP_OK;
}

int pp_check(const svgp_pearce_predict_cfg* g, bool long_form) {
    SVGP_REQUIRE(g != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(g->B >= 1 && g->T >= 1 && g->Q >= 1, SVGP_ERR_INVALID, "need B, T, Q >= 1 (B=%d T=%d Q=%d)", g->B, g->T, g->Q);
    const int t_max = long_form ? PPL_T_MAX : PP_T_MAX;
    SVGP_REQUIRE(g->T <= t_max, SVGP_ERR_UNSUPPORTED, "T=%d: %s takes T <= %d", g->T,
                 long_form ? "svgp_pearce_predict_long" : "svgp_pearce_predict", t_max);
    SVGP_REQUIRE(g->q_slices >= 0 && g->q_slices <= g->Q && g->q_slices <= PP_S_MAX, SVGP_ERR_INVALID,
                 "q_slices=%d: need 0 (the plan chooses) or 1 <= q_slices <= min(Q, %d) (Q=%d)", g->q_slices, PP_S_MAX, g->Q);
    return SVGP_OK;
}

int pp_args(const svgp_pearce_predict_cfg* g, const svgp_pearce_predict_bufs* q, PpArgs* a) {
    SVGP_REQUIRE(q != nullptr, SVGP_ERR_INVALID, "bufs is NULL");
    const void* need[] = {q->times, q->tq, q->ls_x, q->ls_y, q->mu_x, q->mu_y, q->var_x, q->var_y, q->p_m_x, q->p_m_y, q->p_v_x, q->p_v_y};
    for (const void* p : need) SVGP_REQUIRE(p != nullptr, SVGP_ERR_INVALID, "NULL device pointer");
    a->B = g->B; a->T = g->T; a->Q = g->Q;
    a->times = q->times; a->tq = q->tq; a->mask = q->mask;
    a->ls[0] = q->ls_x; a->ls[1] = q->ls_y; a->mu[0] = q->mu_x; a->mu[1] = q->mu_y; a->var[0] = q->var_x; a->var[1] = q->var_y;
    a->eps[0] = q->eps_x; a->eps[1] = q->eps_y; a->p_m[0] = q->p_m_x; a->p_m[1] = q->p_m_y; a->p_v[0] = q->p_v_x; a->p_v[1] = q->p_v_y;
    a->z[0] = q->z_x; a->z[1] = q->z_y; a->lh = q->lh;
    return SVGP_OK;
}

struct PlWork { int64_t Am, yv, alpha, logdet, inv, Kq, R, total; };
PlWork pp_work(const svgp_pearce_predict_cfg* g) {
    const int64_t T = g->T, nm = 2 * (g->B < PPL_NB ? g->B : PPL_NB), nq = g->Q < PPL_QC ? g->Q : PPL_QC;
    SvgpTake16 c16;
    PlWork o;
    o.Am = c16.take(nm * T * T); o.yv = c16.take(nm * T); o.alpha = c16.take(nm * T); o.logdet = c16.take(nm);
    o.inv = c16.take((int64_t)svgp_spd_inverse_workspace_elems((int)T, (int)nm));
    o.Kq = c16.take(nm * nq * T); o.R = c16.take(nm * nq * T);
    o.total = c16.p;
    return o;
}

}  // namespace

extern "C" int svgp_pearce_predict_route(const svgp_pearce_predict_cfg* g, int long_form, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = pp_check(g, long_form != 0);
    if (rc) return rc;
    int pos = 0;
    buf[0] = 0;
    return pp_walk(g, long_form != 0, [&](const PpStep& s) -> int {
        return svgp_route_append(buf, cap, &pos, "%s\n", PP_NAME[s.op]);
    });
}

extern "C" int svgp_pearce_predict(const svgp_pearce_predict_cfg* g, const svgp_pearce_predict_bufs* q, void* stream) {
    int rc = pp_check(g, false);
    if (rc) return rc;
    PpArgs a;
    rc = pp_args(g, q, &a);
    if (rc) return rc;
    return pp_walk(g, false, [&](const PpStep& s) -> int {
        const dim3 grid((unsigned)a.B, 2, (unsigned)s.S);
        const size_t lds = pp_lds_bytes(a.T);
        if (a.T <= 32) hipLaunchKernelGGL(k_pearce_predict<32>, grid, dim3(256), lds, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(k_pearce_predict<64>, grid, dim3(256), lds, (hipStream_t)stream, a);
        SVGP_LAUNCH_CHECK();
        return (int)SVGP_OK;
    });
}

extern "C" long long svgp_pearce_predict_long_workspace_elems(const svgp_pearce_predict_cfg* g) {
    if (pp_check(g, true)) return 0;
    return pp_work(g).total;
}

extern "C" int svgp_pearce_predict_long(const svgp_pearce_predict_cfg* g, const svgp_pearce_predict_bufs* q, double* work, void* stream) {
    int rc = pp_check(g, true);
    if (rc) return rc;
    PpArgs a;
    rc = pp_args(g, q, &a);
    if (rc) return rc;
    const PlWork w = pp_work(g);
    SVGP_REQUIRE(work != nullptr, SVGP_ERR_INVALID, "work is NULL (B = %d, T = %d, Q = %d needs %lld doubles)", g->B, g->T, g->Q,
                 (long long)w.total);
    const int T = a.T;
    const long long tt = (long long)T * T;
    hipStream_t st = (hipStream_t)stream;
    return pp_walk(g, true, [&](const PpStep& s) -> int {
        const PlChunk h = {s.b0, s.nb, s.q0, s.nq, work + w.Am, work + w.yv, work + w.alpha, work + w.logdet, work + w.Kq, work + w.R};
        const int nm = 2 * s.nb;
        switch (s.op) {
        case PP_FUSED: break;
        case PP_BUILD:
            hipLaunchKernelGGL(k_pp_build, dim3(svgp_blocks(tt), nm), dim3(SVGP_BLOCK), 0, st, a, h);
            SVGP_LAUNCH_CHECK();
            break;
        case PP_INVERSE:
            return svgp_spd_inverse_batched(T, nm, h.Am, h.logdet, work + w.inv, stream);
        case PP_ALPHA:
            hipLaunchKernelGGL(k_pp_alpha, dim3((T + 3) / 4, nm), dim3(256), 0, st, a, h);
            SVGP_LAUNCH_CHECK();
            break;
        case PP_LH:
            if (!a.lh) break;        // nothing else reads what this launch forms
            hipLaunchKernelGGL(k_pp_lh, dim3(nm), dim3(256), 0, st, a, h);
            SVGP_LAUNCH_CHECK();
            break;
        case PP_KQ:
            hipLaunchKernelGGL(k_pp_kq, dim3(svgp_blocks((long long)s.nq * T), nm), dim3(SVGP_BLOCK), 0, st, a, h);
            SVGP_LAUNCH_CHECK();
            break;
        case PP_GEMM:       // R_l (nq, T) = Kq_l (nq, T) Ai_l (T, T)
            return svgp_dgemm_batched(0, 0, s.nq, T, T, 1.0, h.Kq, T, (long long)s.nq * T, h.Am, T, tt, 0.0, h.R, T, (long long)s.nq * T, nm,
                                      stream);
        case PP_FINISH:
            hipLaunchKernelGGL(k_pp_finish, dim3((s.nq + 3) / 4, nm), dim3(256), 0, st, a, h);
            SVGP_LAUNCH_CHECK();
            break;
        }
        return (int)SVGP_OK;
    });
}
