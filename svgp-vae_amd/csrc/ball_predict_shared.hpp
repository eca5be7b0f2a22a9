// What the marginal moving-ball predictor (ball_predict.hip), the joint one (ball_predict_joint.hip,
// section 9l) and the streamed posterior state (ball_state.hip, section 9m) share: the inputs of a call, the fused kernels' way to
// K, Sig, their inverses, w and X in LDS, the plan and launches of the large form up to X and w, and the launches of the large
// forms' closing kernels.  Include after common.hpp and lds_spd_inverse.hpp.
#pragma once

constexpr int BP_TC = 16;            // frames (and query times) of a chunk of the fused kernels
constexpr int BP_M_MAX = 64, BP_T_MAX = 16384;
constexpr int BPL_T_MAX = 2048;
constexpr int BPL_NB = 64;           // at most this many videos in a chunk of a large form
constexpr int BPL_QC = 4096;         // query rows of a chunk of the marginal large form
constexpr int BPJL_Q_MAX = 2048;     // query times of the joint large form
constexpr long long BPJL_CAP = 1LL << 22;            // doubles of one chunk's covariance block in the joint large form (32 MiB)

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

#ifdef __HIPCC__
__device__ __forceinline__ void bp_precision(const BpIn& a, int c, size_t e, real& p, real& py) {
    p = recip_no_nan(a.var[c][e]);
    if (a.mask) p *= a.mask[e];
    py = p == real(0) ? real(0) : p * a.mu[c][e];
}

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

// Video b, coordinate c, 256 threads.  On return (no closing barrier: the caller's next __syncthreads() completes it) s.Sg holds
// X = Si - Ki, s.wv holds w, s.zv the inducing points and s.Km is free.  Thread layout as in lds_spd_inverse: column j = tid &
// (CW - 1), row lane i0 = tid / CW; a thread owns (i0 + RL r, j).  Returns -1 / (2 ls^2).
template <int CW>
__device__ __forceinline__ real bp_factors(const BpIn& a, int b, int c, const BpLds& s) {
    constexpr int RL = 256 / CW, RMAX = CW / RL, KS = CW + 1;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW;
    const int m = a.m, ld = m + 1, B = a.B, T = a.T;
    real* Km = s.Km; real* Sg = s.Sg; real* kt = s.kt; real* zv = s.zv; real* vv = s.vv; real* wv = s.wv; real* pc = s.pc; real* pyc = s.pyc;
    const real* __restrict__ times = a.times;
    const real l = *a.ls[c], il2 = real(-0.5) / (l * l);
    if (tid < CW) zv[tid] = tid < m ? a.ip[c][tid] : real(0);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) { const real d = zv[i] - zv[j]; Km[i * ld + j] = exp(d * d * il2); }
    }
    // ---- the frames, in order
    real acc[RMAX], vacc = 0;
#pragma unroll
    for (int r = 0; r < RMAX; ++r) acc[r] = 0;
    for (int t0 = 0; t0 < T; t0 += BP_TC) {
        const int cnt = T - t0 < BP_TC ? T - t0 : BP_TC;
        __syncthreads();             // the previous chunk is consumed
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
            for (int r = 0; r < RMAX; ++r) acc[r] += pk * kr[i0 + RL * r];
            if (i0 == 0) vacc += pyc[tc] * kj;
        }
    }
    // Sig + j I beside K + j I: equal bit for bit where every p was 0
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
        wv[tid] = sum;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) Sg[i * ld + j] -= Km[i * ld + j];
    }
    return il2;
}
#endif

// ---------------------------------------------------------------------------------------------------------
// the large forms up to X and w: per coordinate one BP_KMAT, then per chunk of nb videos the seven steps of bp_walk_factors
// ---------------------------------------------------------------------------------------------------------
enum BpOp { BP_FUSED, BP_KMAT, BP_SCALE, BP_SIGMA, BP_PRIOR, BP_V, BP_INVERSE, BP_W, BP_SUB, BP_KQ, BP_ROWS, BP_FINISH,
            BPJ_FUSED, BPJ_KQ, BPJ_G, BPJ_GK, BPJ_COV, BPJ_POTRF, BPJ_FINISH };             // the joint predictor's own steps
extern const char* const BP_NAME[];  // the route text's name of each op (ball_predict.hip)
struct BpStep { BpOp op; int c, b0, nb, q0, nq; };

template <class F>
int bp_walk_factors(int c, int b0, int nb, F f) {
    for (BpOp op : {BP_SCALE, BP_SIGMA, BP_PRIOR, BP_V, BP_INVERSE, BP_W, BP_SUB})
        if (int rc = f(BpStep{op, c, b0, nb, 0, 0})) return rc;
    return 0;
}

// workspace of those steps for chunks of at most nb videos; on return of a chunk Mats (nb, m, m) holds X_l and W (nb, m) holds w_l
struct BpFactorWork { int64_t K, Kn, knn, KnP, PY, Mats, V, W, logdet, inv; };
BpFactorWork bp_factor_work(SvgpTake16& c16, int64_t m, int64_t T, int64_t nb);
// launches BP_KMAT or one of the seven steps (ball_predict.hip)
int bp_factor_launch(const BpIn& a, const BpStep& s, const BpFactorWork& w, double* work, void* stream);
// the closing kernels of the large forms, for callers outside their files: k_bp_finish (ball_predict.hip), k_bpj_cov and k_bpj_finish
// (ball_predict_joint.hip) with exactly the arguments documented there
int bp_finish_launch(const BpArgs& a, int c, int b0, int nb, int q0, int nq, const real* tpm, const real* tpv, void* stream);
int bpj_cov_launch(const BpjArgs& a, int c, int b0, int nb, real* Cb, void* stream);
int bpj_finish_launch(const BpjArgs& a, int c, int b0, int nb, const real* Kq, const real* W, const real* Lb, void* stream);
