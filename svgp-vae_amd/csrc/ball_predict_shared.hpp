// What the marginal moving-ball predictor (ball_predict.hip), the joint one (ball_predict_joint.hip,
// section 9l) and the streamed posterior state (ball_state.hip, section 9m) share, each stated once: the inputs of a call and their
// marshalling, the device pieces of the fused kernels (bp_prior: K; bp_accumulate: the frames; bp_invert: the two inverses and w;
// bp_store_x: X; bp_query_chunks: the query times), the steps of the large forms (the factors up to X and w, the marginal tail, the joint tail)
// with their workspace and launches, and the route line of a step.  Include after common.hpp and lds_spd_inverse.hpp.
#pragma once

constexpr int BP_TC = 16;            // frames (and query times) of a chunk of the fused kernels
constexpr int BP_M_MAX = 64, BP_T_MAX = 16384;
constexpr int BPL_T_MAX = 2048;
constexpr int BPL_NB = 64;           // at most this many videos in a chunk of a large form
constexpr int BPL_QC = 4096;         // query rows of a chunk of the marginal large form
constexpr int BPJL_Q_MAX = 2048;     // query times of the joint large form
constexpr long long BPJL_CAP = 1LL << 22;            // doubles of one chunk's covariance block in the joint large form (32 MiB)

// videos of a chunk of the joint large form: min(BPL_NB, B, max(1, BPJL_CAP / Q^2))
inline int bpj_chunk(int B, int Q) {
    const long long qq = (long long)Q * Q, cap = BPJL_CAP / qq > 1 ? BPJL_CAP / qq : 1;
    const long long nb = B < BPL_NB ? B : BPL_NB;
    return (int)(nb < cap ? nb : cap);
}

// the inputs of both predictors
struct BpIn {
    int B, T, m, Q;
    real jitter;
    const real* times; const real* tq; const real* mask;
    const real* ip[2]; const real* ls[2]; const real* mu[2]; const real* var[2];
};

// the arguments of the marginal and of the joint kernels
struct BpArgs : BpIn {
    real lo, hi;
    const real* eps[2];
    real* p_m[2]; real* p_v[2]; real* z[2];
};
struct BpjArgs : BpIn {
    real jp;
    const real* eps[2];
    real* p_m[2]; real* cov[2]; real* chol[2]; real* z[2];
};

// What BpArgs and BpjArgs share, from any of the three cfg / bufs pairs of the header (their field names agree).  Checks ip and ls,
// the pointers of the frames (times, mu, var) where `frames`, and those of the query times (tq, p_m) where `query`.
template <class Cfg, class Bufs, class Args>
int bp_marshal(const Cfg* g, const Bufs* q, bool frames, bool query, Args* a) {
    SVGP_REQUIRE(q != nullptr, SVGP_ERR_INVALID, "bufs is NULL");
    const void* always[] = {q->ip_x, q->ip_y, q->ls_x, q->ls_y};
    const void* of_frames[] = {q->times, q->mu_x, q->mu_y, q->var_x, q->var_y};
    const void* of_query[] = {q->tq, q->p_m_x, q->p_m_y};
    for (const void* p : always) SVGP_REQUIRE(p != nullptr, SVGP_ERR_INVALID, "NULL device pointer");
    for (const void* p : of_frames) SVGP_REQUIRE(!frames || p != nullptr, SVGP_ERR_INVALID, "NULL device pointer");
    for (const void* p : of_query) SVGP_REQUIRE(!query || p != nullptr, SVGP_ERR_INVALID, "NULL device pointer");
    a->B = g->B; a->T = g->T; a->m = g->m; a->Q = g->Q; a->jitter = g->jitter;
    a->times = q->times; a->tq = q->tq; a->mask = q->mask;
    a->ip[0] = q->ip_x; a->ip[1] = q->ip_y; a->ls[0] = q->ls_x; a->ls[1] = q->ls_y; a->mu[0] = q->mu_x; a->mu[1] = q->mu_y;
    a->var[0] = q->var_x; a->var[1] = q->var_y; a->eps[0] = q->eps_x; a->eps[1] = q->eps_y;
    a->p_m[0] = q->p_m_x; a->p_m[1] = q->p_m_y; a->z[0] = q->z_x; a->z[1] = q->z_y;
    return SVGP_OK;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------------------------------------
// the device pieces of the fused kernels.  256 threads, thread layout as in lds_spd_inverse: column j = tid & (CW - 1), row lane
// i0 = tid / CW of RL = 256 / CW; a thread owns the RMAX = CW / RL elements (i0 + RL r, j) of an m x m matrix.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bp_precision(const BpIn& a, int c, size_t e, real& p, real& py) {
    p = recip_no_nan(a.var[c][e]);
    if (a.mask) p *= a.mask[e];
    py = p == real(0) ? real(0) : p * a.mu[c][e];
}
// -1 / (2 ls^2) of the SE kernel exp(d * d * il2)
__device__ __forceinline__ real bp_il2(const BpIn& a, int c) { const real l = *a.ls[c]; return real(-0.5) / (l * l); }
// the inducing points into zv (no barrier)
template <int CW>
__device__ __forceinline__ void bp_load_z(const BpIn& a, int c, real* zv) {
    const int tid = threadIdx.x;
    if (tid < CW) zv[tid] = tid < a.m ? a.ip[c][tid] : real(0);
}

// The scalars of a call the pieces use.  The caller reads them once, ahead of its first barrier, and hands them down: read inside
// each piece they are loaded behind barriers and m exists as several values, which costs k_ball_predict_joint 1 - 3 %
struct BpDims { int m, B, T; const real* times; };
__device__ __forceinline__ BpDims bp_dims(const BpIn& a) { return {a.m, a.B, a.T, a.times}; }

// LDS of the factor stage: two slots of n1 and n2 >= m (m + 1) values for the matrices, the chunk of kernel rows and the vectors
struct BpLds {
    real* Km;                        // m x ld : K, K + j I, its inverse; free once X exists
    real* Sg;                        // m x ld : Sig + j I, its inverse, X
    real* kt;                        // BP_TC x KS : kernel rows of a chunk of frames / of query times, columns >= m zero
    real* zv;                        // CW : inducing points
    real* vv;                        // CW : Kn^T (p y)
    real* wv;                        // CW : w
    real* piv;                       // CW : pivots of the sweep
    real* pc;                        // BP_TC : p of the chunk
    real* pyc;                       // BP_TC : p y of the chunk
};
constexpr int bp_lds_tail_elems(int CW) { return BP_TC * (CW + 1) + 4 * CW + 2 * BP_TC; }
template <int CW>
__device__ __forceinline__ BpLds bp_lds_map(real* smem, int n1, int n2) {
    BpLds s;
    s.Km = smem; s.Sg = s.Km + n1; s.kt = s.Sg + n2; s.zv = s.kt + BP_TC * (CW + 1);
    s.vv = s.zv + CW; s.wv = s.vv + CW; s.piv = s.wv + CW; s.pc = s.piv + CW; s.pyc = s.pc + BP_TC;
    return s;
}

// The frames: adds p_t k_t[i] k_t[j] of the T frames of video b, coordinate c to the caller's acc (its elements of S = Kn^T diag(p)
// Kn) and p_t y_t k_t[j] to vacc (r = Kn^T (p y), row lane 0), in frame order and every addition an explicit fma: accumulators that
// start from the sums of earlier frames end with the bits of one call over all of them, and a frame of precision 0 adds +0 to a
// non-negative sum.  Uses s.kt, s.pc, s.pyc and s.zv only; the caller has written s.zv, and the loop's first
// barrier completes it.
template <int CW>
__device__ __forceinline__ void bp_accumulate(const BpIn& a, const BpDims& d, int b, int c, const BpLds& s, real il2,
                                              real (&acc)[CW * CW / 256], real& vacc) {
    constexpr int RL = 256 / CW, RMAX = CW / RL, KS = CW + 1;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW;
    const int m = d.m, B = d.B, T = d.T;
    real* kt = s.kt; real* pc = s.pc; real* pyc = s.pyc;
    const real* zv = s.zv;
    const real* __restrict__ times = d.times;
    for (int t0 = 0; t0 < T; t0 += BP_TC) {
        const int cnt = T - t0 < BP_TC ? T - t0 : BP_TC;
        __syncthreads();             // zv is complete / the previous chunk is consumed
        if (tid < BP_TC) {
            real p = 0, py = 0;
            if (tid < cnt) bp_precision(a, c, (size_t)(t0 + tid) * B + b, p, py);
            pc[tid] = p; pyc[tid] = py;
        }
#pragma unroll
        for (int r = 0; r < BP_TC / RL; ++r) {
            const int tc = i0 + RL * r;
            real k = 0;
            if (tc < cnt && j < m) { const real d = times[t0 + tc] - zv[j]; k = exp(d * d * il2); }
            kt[tc * KS + j] = k;
        }
        __syncthreads();
#pragma unroll 2
        for (int tc = 0; tc < cnt; ++tc) {
            const real* kr = kt + tc * KS;
            const real kj = kr[j], pk = pc[tc] * kj;
#pragma unroll
            for (int r = 0; r < RMAX; ++r) acc[r] = fma(pk, kr[i0 + RL * r], acc[r]);
            if (i0 == 0) vacc = fma(pyc[tc], kj, vacc);
        }
    }
}

// K = SE(z, z) into s.Km (s.zv complete): a thread writes the elements it owns, the ones it reads back in bp_invert (no barrier)
template <int CW>
__device__ __forceinline__ void bp_prior(const BpLds& s, int m, real il2) {
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int j = threadIdx.x & (CW - 1), i0 = threadIdx.x / CW, ld = m + 1;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) { const real d = s.zv[i] - s.zv[j]; s.Km[i * ld + j] = exp(d * d * il2); }
    }
}

// The factor finish, from K in s.Km (bp_prior), the caller's m and the thread's elements acc of S and vacc of r: on return, behind a barrier, s.Sg
// holds Si = ((K + S) + j I)^-1, s.Km holds Ki = (K + j I)^-1 and s.wv holds w = Si r.
template <int CW>
__device__ __forceinline__ void bp_invert(const BpIn& a, int m, const BpLds& s, const real (&acc)[CW * CW / 256], real vacc) {
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW;
    const int ld = m + 1;
    real* Km = s.Km; real* Sg = s.Sg; real* vv = s.vv;
    // (K + S) + j I beside K + j I: equal bit for bit where S is 0 (zero stats, or every frame dropped), and then so are the two
    // inverses: X = 0 and w = 0 exactly
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) {
            const real k = Km[i * ld + j], jit = i == j ? a.jitter : real(0);
            Sg[i * ld + j] = (k + acc[r]) + jit;
            Km[i * ld + j] = k + jit;
        }
    }
    if (i0 == 0) vv[j] = vacc;
#pragma unroll 1
    for (int which = 0; which < 2; ++which) lds_spd_inverse<CW>(which ? Sg : Km, ld, m, s.piv);    // one copy of the sweep's code
    if (tid < CW) {
        real sum = 0;
        if (tid < m) {
#pragma unroll 4
            for (int k = 0; k < m; ++k) sum += Sg[tid * ld + k] * vv[k];
        }
        s.wv[tid] = sum;
    }
    __syncthreads();
}

// X = Si - Ki from s.Sg and s.Km to dst (row stride ldd), which may be s.Sg itself
template <int CW>
__device__ __forceinline__ void bp_store_x(const BpLds& s, int m, real* dst, int ldd) {
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int j = threadIdx.x & (CW - 1), i0 = threadIdx.x / CW, ld = m + 1;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) dst[i * ldd + j] = s.Sg[i * ld + j] - s.Km[i * ld + j];
    }
}

// Video b, coordinate c: bp_prior, bp_accumulate from zeros, bp_invert, X in place.  On return (no closing barrier: the caller's next
// __syncthreads() completes it) s.Sg holds X = Si - Ki, s.wv holds w, s.zv the inducing points and s.Km is free.  Returns il2.
template <int CW>
__device__ __forceinline__ real bp_factors(const BpIn& a, int b, int c, const BpLds& s) {
    const BpDims d = bp_dims(a);
    const real il2 = bp_il2(a, c);
    real acc[CW * CW / 256] = {}, vacc = 0;
    bp_load_z<CW>(a, c, s.zv);
    __syncthreads();
    bp_prior<CW>(s, d.m, il2);
    bp_accumulate<CW>(a, d, b, c, s, il2, acc, vacc);
    bp_invert<CW>(a, d.m, s, acc, vacc);
    bp_store_x<CW>(s, d.m, s.Sg, d.m + 1);
    return il2;
}

// The query times [q_lo, q_hi) of video b, coordinate c from X (row stride ld), wv and zv in LDS, which the first barrier completes:
// 16 per chunk (kernel rows into kt), 16 lanes per query, each takes the rows i = lane, lane + 16, ... of k^T X k and of k . w, and an
// xor-shuffle adds the 16 partials: a query's bits depend neither on where it stands in tq nor on the slice that serves it.
template <int CW>
__device__ __forceinline__ void bp_query_chunks(const BpArgs& a, int b, int c, const real* X, int ld, const real* wv, const real* zv,
                                                real* kt, real il2, long long q_lo, long long q_hi) {
    constexpr int RL = 256 / CW, KS = CW + 1;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW, qc = tid >> 4, l16 = tid & 15;
    const int m = a.m, B = a.B, Q = a.Q;
    const real* __restrict__ tq = a.tq;
    const real* __restrict__ eps = a.eps[c];
    real* __restrict__ o_pm = a.p_m[c];
    real* __restrict__ o_pv = a.p_v[c];
    real* __restrict__ o_z = a.z[c];
    for (long long q0 = q_lo; q0 < q_hi; q0 += BP_TC) {          // (64 bits: Q may be close to 2^31)
        __syncthreads();             // X, w, zv are complete / the previous chunk is consumed
#pragma unroll
        for (int r = 0; r < BP_TC / RL; ++r) {
            const int qq = i0 + RL * r;
            real k = 0;
            if (q0 + qq < Q && j < m) { const real d = tq[q0 + qq] - zv[j]; k = exp(d * d * il2); }
            kt[qq * KS + j] = k;
        }
        __syncthreads();
        const real* kr = kt + qc * KS;
        real pm = 0, qs = 0;
        for (int i = l16; i < m; i += 16) {
            const real* xr = X + i * ld;
            real row = 0;
#pragma unroll 4
            for (int k = 0; k < m; ++k) row += xr[k] * kr[k];
            qs += kr[i] * row;
            pm += kr[i] * wv[i];
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { pm += __shfl_xor(pm, o, 64); qs += __shfl_xor(qs, o, 64); }
        if (l16 == 0 && q0 + qc < Q) {
            const size_t e = (size_t)(q0 + qc) * B + b;
            const real pv = real(1) + qs;
            o_pm[e] = pm; o_pv[e] = pv;
            if (o_z) o_z[e] = eps ? pm + eps[e] * sqrt(clip_keep_nan(pv, a.lo, a.hi)) : pm;
        }
    }
}
#endif

// ---------------------------------------------------------------------------------------------------------
// the steps of the large forms.  Per coordinate one BP_KMAT, then per chunk of nb videos the seven steps of bp_walk_factors up to
// X_l and w_l, then the marginal tail (bp_walk_tail) or the joint one (bpj_walk_tail)
// ---------------------------------------------------------------------------------------------------------
enum BpOp { BP_FUSED, BP_KMAT, BP_SCALE, BP_SIGMA, BP_PRIOR, BP_V, BP_INVERSE, BP_W, BP_SUB, BP_KQ, BP_ROWS, BP_FINISH,
            BPJ_FUSED, BPJ_KQ, BPJ_G, BPJ_GK, BPJ_COV, BPJ_POTRF, BPJ_FINISH };             // the joint predictor's own steps
struct BpStep { BpOp op; int c, b0, nb, q0, nq; };
// appends the route line(s) of a step: the name of its kernel or entry point; BP_ROWS prints the rows entry's own one or two kernels
// (ball_predict.hip)
int bp_route_line(const BpStep& s, int m, char* buf, int cap, int* pos);

template <class F>
int bp_walk_factors(int c, int b0, int nb, F f) {
    for (BpOp op : {BP_SCALE, BP_SIGMA, BP_PRIOR, BP_V, BP_INVERSE, BP_W, BP_SUB})
        if (int rc = f(BpStep{op, c, b0, nb, 0, 0})) return rc;
    return 0;
}
// the marginal tail of a chunk of videos: its three steps per chunk of BPL_QC query rows
template <class F>
int bp_walk_tail(int c, int b0, int nb, int Q, F f) {
    for (long long q0 = 0; q0 < Q; q0 += BPL_QC) {
        const int nq = Q - q0 < BPL_QC ? (int)(Q - q0) : BPL_QC;
        for (BpOp op : {BP_KQ, BP_ROWS, BP_FINISH})
            if (int rc = f(BpStep{op, c, b0, nb, (int)q0, nq})) return rc;
    }
    return 0;
}
// the joint tail of a chunk of videos: its six steps over all Q query times
template <class F>
int bpj_walk_tail(int c, int b0, int nb, int Q, F f) {
    for (BpOp op : {BPJ_KQ, BPJ_G, BPJ_GK, BPJ_COV, BPJ_POTRF, BPJ_FINISH})
        if (int rc = f(BpStep{op, c, b0, nb, 0, Q})) return rc;
    return 0;
}

// workspace of the factor steps for chunks of at most nb videos; on return of a chunk Mats (nb, m, m) holds X_l and W (nb, m) holds w_l
struct BpFactorWork { int64_t K, Kn, knn, KnP, PY, Mats, V, W, logdet, inv; };
BpFactorWork bp_factor_work(SvgpTake16& c16, int64_t m, int64_t T, int64_t nb);
// launches BP_KMAT or one of the seven steps (ball_predict.hip)
int bp_factor_launch(const BpIn& a, const BpStep& s, const BpFactorWork& w, double* work, void* stream);

// the marginal tail (ball_predict.hip): workspace for chunks of at most nb videos and min(Q, BPL_QC) query rows, and the launch of one
// of its steps from X (nb, m, m) and W (nb, m), both contiguous as svgp_sprites_posterior_rows takes them
struct BpTailWork { int64_t K2, Kq, kbb, tpm, tpv, rows; };
BpTailWork bp_tail_work(SvgpTake16& c16, int64_t m, int64_t Q, int64_t nb);
int bp_tail_launch(const BpArgs& a, const BpStep& s, const BpTailWork& w, const real* X, const real* W, double* work, void* stream);

// the joint tail (ball_predict_joint.hip): workspace for chunks of at most nb videos, and the launch of one of its steps from the X_l
// at X + l xstride and W (nb, m)
struct BpjTailWork { int64_t K2, Kq, kbb, G, Cb, logdet, potrf; };
BpjTailWork bpj_tail_work(SvgpTake16& c16, int64_t m, int64_t Q, int64_t nb);
int bpj_tail_launch(const BpjArgs& a, const BpStep& s, const BpjTailWork& w, const real* X, long long xstride, const real* W, double* work,
                    void* stream);
