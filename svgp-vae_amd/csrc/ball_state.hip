// Moving-ball SVGP-VAE after training, streamed: the posterior of section 9h with its state kept in device
// memory between calls, so that frames can arrive over time and a finished state serves any number of query grids.  The sparse
// posterior depends on the frames only through two additive statistics per video b and latent coordinate c,
//   S = Kn^T diag(p) Kn  (m x m)        r = Kn^T (p y)  (m)
// with p, Kn, K, k exactly those of ball_predict.hip.  The four entries cut 9h at the two places where its state is complete:
//   update    stats += (S, r) of T more frames                          stats (B, 2, m m + m): S row-major, then r; zeros = the prior
//   finalize  Si = ((K + S) + j I)^-1, Ki = (K + j I)^-1, post = (X = Si - Ki, w = Si r)        post (B, 2, m m + m): X, then w
//   query     k = SE(tau, z):  p_m = k w,  p_v = 1 + diag(k X k^T),  z = p_m + eps sqrt(clamp(p_v))           (9h's tail)
//   joint     C = SE(tau, tau) + k X k^T,  Lc = chol(C + jp I),  p_m = k w,  z = p_m + Lc eps                  (9l's tail)
//
// Fused routes (cfg.large = 0, m <= 64), one launch each, 256 threads, thread layout of lds_spd_inverse, each a composition of the
// device pieces of ball_predict_shared.hpp that k_ball_predict is made of:
//   k_ball_state_update<CW>    grid (B, 2).  The accumulators from stats, bp_accumulate, and back.  Feeding the frames in pieces gives
//       the bits of one call because bp_accumulate adds every frame with an explicit fma in frame order onto whatever sums it is
//       handed, here and in the one-shot entries alike; a frame of precision 0 adds +0 to a non-negative sum.
//       LDS: the 16 x (CW + 1) chunk, zv, pc, pyc (9 088 bytes at CW = 64).
//   k_ball_state_finalize<CW>  grid (B, 2).  S and r from stats, bp_prior (K), bp_invert ((K + S) + j I beside K + j I in LDS, the one inlined
//       two-trip sweep, w = Si r), then bp_store_x writes X = Si - Ki straight from LDS to post, and w follows.  Zero stats: the two
//       matrices are equal bit for bit, X = 0 and w = 0 exactly.
//   k_ball_state_query<CW>     grid (B, 2, S).  X (row stride m + 1) and w into LDS, then bp_query_chunks on the workgroup's slice of
//       the query times: a query's bits depend neither on S nor on its position in tq.
// Large routes (cfg.large != 0, m <= 2048; update T <= 2048 a call): the steps of bp_factor_launch on chunks of BPL_NB videos, the
// two GEMMs of the update accumulating into stats (beta = 1), with k_bs_gather / k_bs_scatter between the state layout and the
// contiguous blocks those steps and the marginal tail (bp_tail_launch) work on; the joint tail (bpj_tail_launch) reads X in place
// from post.  The joint query has the large form only.
// bs_walk is the one plan the launch code and svgp_ball_state_route follow.
#include "common.hpp"
#include "lds_spd_inverse.hpp"
#include "ball_predict_shared.hpp"

#include <cmath>

namespace {

constexpr int BS_WG_TARGET = 512;    // workgroups the query's slice choice aims at: about two per CU
constexpr int BS_SLICES_MAX = 65535;
enum BsOp { BS_UPDATE = SVGP_BALL_STATE_UPDATE, BS_FINALIZE = SVGP_BALL_STATE_FINALIZE, BS_QUERY = SVGP_BALL_STATE_QUERY,
            BS_JOINT = SVGP_BALL_STATE_QUERY_JOINT };
const char* const BS_ENTRY[] = {"svgp_ball_state_update", "svgp_ball_state_finalize", "svgp_ball_state_query", "svgp_ball_state_query_joint"};

// what the kernels of this file take beyond BpArgs (whose p_m .. z the query writes)
struct BsArgs : BpArgs {
    real* stats; real* post;
    int rps;                         // rounds of BP_TC query times per slice
};

__host__ __device__ inline long long bs_elems(int m) { return (long long)m * m + m; }
__device__ __forceinline__ real* bs_block(real* base, int m, int b, int c) { return base + ((size_t)b * 2 + c) * bs_elems(m); }

// ---------------------------------------------------------------------------------------------------------
// the fused routes
// ---------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(256) void k_ball_state_update(BsArgs a) {
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    __shared__ real kt[BP_TC * (CW + 1)], zv[CW], pc[BP_TC], pyc[BP_TC];
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW;
    const int b = blockIdx.x, c = blockIdx.y, m = a.m;
    BpLds s = {};                    // what bp_accumulate uses
    s.kt = kt; s.zv = zv; s.pc = pc; s.pyc = pyc;
    real* __restrict__ S = bs_block(a.stats, m, b, c);
    real* __restrict__ rv = S + (size_t)m * m;
    bp_load_z<CW>(a, c, zv);
    real acc[RMAX], vacc = (i0 == 0 && j < m) ? rv[j] : real(0);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        acc[r] = (i < m && j < m) ? S[(size_t)i * m + j] : real(0);
    }
    bp_accumulate<CW>(a, bp_dims(a), b, c, s, bp_il2(a, c), acc, vacc);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        if (i < m && j < m) S[(size_t)i * m + j] = acc[r];
    }
    if (i0 == 0 && j < m) rv[j] = vacc;
}

template <int CW>
__global__ __launch_bounds__(256) void k_ball_state_finalize(BsArgs a) {
    extern __shared__ __align__(16) real smem[];
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int tid = threadIdx.x, j = tid & (CW - 1), i0 = tid / CW;
    const int b = blockIdx.x, c = blockIdx.y, m = a.m;
    const BpLds s = bp_lds_map<CW>(smem, m * (m + 1), m * (m + 1));
    const real* __restrict__ S = bs_block(a.stats, m, b, c);
    real* __restrict__ X = bs_block(a.post, m, b, c);
    bp_load_z<CW>(a, c, s.zv);
    real acc[RMAX];
    const real vacc = (i0 == 0 && j < m) ? S[(size_t)m * m + j] : real(0);
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        const int i = i0 + RL * r;
        acc[r] = (i < m && j < m) ? S[(size_t)i * m + j] : real(0);
    }
    __syncthreads();                 // zv is complete
    bp_prior<CW>(s, m, bp_il2(a, c));
    bp_invert<CW>(a, m, s, acc, vacc);
    bp_store_x<CW>(s, m, X, m);
    if (tid < m) X[(size_t)m * m + tid] = s.wv[tid];
}

constexpr int bsq_lds_elems(int m, int CW) { return m * (m + 1) + 2 * CW + BP_TC * (CW + 1); }
static_assert((size_t)bsq_lds_elems(64, 64) * sizeof(real) == 42624, "the query's LDS map of DESIGN 9m at m = 64");
static_assert(3 * 42624 <= SVGP_LDS_MAX_BYTES, "three query workgroups per CU at m = 64");
static_assert(((size_t)BP_TC * 65 + 64 + 2 * BP_TC) * sizeof(real) == 9088, "the update's LDS of DESIGN 9m at CW = 64");
static_assert(((size_t)2 * 64 * 65 + bp_lds_tail_elems(64)) * sizeof(real) == 77184, "the finalize's LDS is k_ball_predict's");

template <int CW>
__global__ __launch_bounds__(256) void k_ball_state_query(BsArgs a) {
    extern __shared__ __align__(16) real smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x, c = blockIdx.y, m = a.m, ld = m + 1, Q = a.Q;
    const long long span = (long long)a.rps * BP_TC, q_lo = (long long)blockIdx.z * span;     // (64 bits: Q may be close to 2^31)
    if (q_lo >= Q) return;           // (a forced slice count may leave slices without a round)
    const long long q_hi = Q - q_lo < span ? (long long)Q : q_lo + span;
    real* Xs = smem;                 // m x ld
    real* wv = Xs + m * ld;          // CW
    real* zv = wv + CW;              // CW
    real* kt = zv + CW;              // BP_TC x (CW + 1)
    const real* __restrict__ X = bs_block(a.post, m, b, c);
    for (int e = tid; e < m * m; e += 256) { const int i = e / m; Xs[i * ld + e - i * m] = X[e]; }
    bp_load_z<CW>(a, c, zv);
    if (tid < CW) wv[tid] = tid < m ? X[(size_t)m * m + tid] : real(0);
    bp_query_chunks<CW>(a, b, c, Xs, ld, wv, zv, kt, bp_il2(a, c), q_lo, q_hi);
}

// ---------------------------------------------------------------------------------------------------------
// the large routes' own kernels: between the state layout and the contiguous blocks of a chunk
// ---------------------------------------------------------------------------------------------------------
// Mats (nb, m, m) and vec of the chunk's videos from src (stats or post); vec is V (m, nb) when as_V, else W (nb, m).  Mats NULL: the
// vectors only, and the launch covers nb m elements (bs_gather_elems)
__host__ __device__ inline long long bs_gather_elems(int m, int nb, bool mats) { return nb * (mats ? bs_elems(m) : (long long)m); }
__global__ __launch_bounds__(SVGP_BLOCK) void k_bs_gather(int m, int c, int b0, int nb, int as_V, const real* __restrict__ src,
                                                          real* __restrict__ Mats, real* __restrict__ vec) {
    const long long E = bs_elems(m), mm = (long long)m * m, per = Mats ? E : m, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= nb * per) return;
    const long long l = e / per, o = e % per + (Mats ? 0 : mm);
    const real v = src[((b0 + l) * 2 + c) * E + o];
    if (o < mm) Mats[l * mm + o] = v;
    else vec[as_V ? (o - mm) * nb + l : l * m + (o - mm)] = v;
}
// post of the chunk's videos from Mats (nb, m, m) = X_l and W (nb, m) = w_l
__global__ __launch_bounds__(SVGP_BLOCK) void k_bs_scatter(int m, int c, int b0, int nb, const real* __restrict__ Mats,
                                                           const real* __restrict__ W, real* __restrict__ post) {
    const long long E = bs_elems(m), tot = nb * E, e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= tot) return;
    const long long l = e / E, o = e % E, mm = (long long)m * m;
    post[((b0 + l) * 2 + c) * E + o] = o < mm ? Mats[l * mm + o] : W[l * m + (o - mm)];
}

// ---------------------------------------------------------------------------------------------------------
// one plan for the launch code and the route text
// ---------------------------------------------------------------------------------------------------------
enum BsStepOp { BSS_UPDATE, BSS_FINALIZE, BSS_QUERY, BSS_GATHER, BSS_SCATTER, BSS_BP };     // BSS_BP: the BpOp of the step
const char* const BSS_NAME[] = {"k_ball_state_update", "k_ball_state_finalize", "k_ball_state_query", "k_bs_gather", "k_bs_scatter"};
struct BsStep { BsStepOp own; BpStep s; };

inline int bs_rounds(const svgp_ball_state_cfg* g) { return (int)(((long long)g->Q + BP_TC - 1) / BP_TC); }
inline int bs_slices_max(const svgp_ball_state_cfg* g) { return bs_rounds(g) < BS_SLICES_MAX ? bs_rounds(g) : BS_SLICES_MAX; }
// slices of the fused query: about BS_WG_TARGET workgroups, at least one round of BP_TC query times per slice
int bs_slices(const svgp_ball_state_cfg* g) {
    if (g->q_slices > 0) return g->q_slices;
    const long long want = (BS_WG_TARGET + 2LL * g->B - 1) / (2LL * g->B), cap = bs_slices_max(g);
    const long long s = want < cap ? want : cap;
    return (int)(s < 1 ? 1 : s);
}

// calls f(step) for every launch group of one call, in order; stops at the first non-zero return
template <class F>
int bs_walk(const svgp_ball_state_cfg* g, int op, F f) {
    int rc;
    auto own = [&](BsStepOp o, int c, int b0, int nb) { return f(BsStep{o, BpStep{BP_FUSED, c, b0, nb, 0, 0}}); };
    auto step = [&](const BpStep& s) { return f(BsStep{BSS_BP, s}); };
    auto bp = [&](BpOp o, int c, int b0, int nb) { return step(BpStep{o, c, b0, nb, 0, 0}); };
    if (!g->large && op != BS_JOINT) return own(op == BS_UPDATE ? BSS_UPDATE : op == BS_FINALIZE ? BSS_FINALIZE : BSS_QUERY, 0, 0, g->B);
    const int chunk = op == BS_JOINT ? bpj_chunk(g->B, g->Q) : BPL_NB;
    for (int c = 0; c < 2; ++c) {
        if (op == BS_UPDATE || op == BS_FINALIZE)
            if ((rc = bp(BP_KMAT, c, 0, 0))) return rc;
        for (int b0 = 0; b0 < g->B; b0 += chunk) {
            const int nb = g->B - b0 < chunk ? g->B - b0 : chunk;
            switch (op) {
            case BS_UPDATE:
                for (BpOp o : {BP_SCALE, BP_SIGMA, BP_V})
                    if ((rc = bp(o, c, b0, nb))) return rc;
                break;
            case BS_FINALIZE:
                if ((rc = own(BSS_GATHER, c, b0, nb))) return rc;
                for (BpOp o : {BP_PRIOR, BP_INVERSE, BP_W, BP_SUB})
                    if ((rc = bp(o, c, b0, nb))) return rc;
                if ((rc = own(BSS_SCATTER, c, b0, nb))) return rc;
                break;
            case BS_QUERY:
                if ((rc = own(BSS_GATHER, c, b0, nb))) return rc;
                if ((rc = bp_walk_tail(c, b0, nb, g->Q, step))) return rc;
                break;
            default:
                if ((rc = own(BSS_GATHER, c, b0, nb))) return rc;
                if ((rc = bpj_walk_tail(c, b0, nb, g->Q, step))) return rc;
            }
        }
    }
    return SVGP_OK;
}

int bs_check(const svgp_ball_state_cfg* g, int op) {
    SVGP_REQUIRE(op >= BS_UPDATE && op <= BS_JOINT, SVGP_ERR_INVALID, "op=%d: not an operation of svgp_ball_state", op);
    const char* name = BS_ENTRY[op];
    SVGP_REQUIRE(g != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    const bool query = op == BS_QUERY || op == BS_JOINT, large = g->large != 0 || op == BS_JOINT;
    SVGP_REQUIRE(g->B >= 1 && g->m >= 1, SVGP_ERR_INVALID, "need B, m >= 1 (B=%d m=%d)", g->B, g->m);
    SVGP_REQUIRE(op != BS_UPDATE || g->T >= 1, SVGP_ERR_INVALID, "need T >= 1 (T=%d)", g->T);
    SVGP_REQUIRE(!query || g->Q >= 1, SVGP_ERR_INVALID, "need Q >= 1 (Q=%d)", g->Q);
    const int m_max = large ? SVGP_M_LIMIT : BP_M_MAX, t_max = large ? BPL_T_MAX : BP_T_MAX;
    SVGP_REQUIRE(g->m <= m_max, SVGP_ERR_UNSUPPORTED, "m=%d: %s takes m <= %d%s", g->m, name, m_max, large ? "" : " on the fused route");
    if (op == BS_UPDATE)
        SVGP_REQUIRE(g->T <= t_max, SVGP_ERR_UNSUPPORTED, "T=%d: %s takes T <= %d a call%s", g->T, name, t_max, large ? " on the large route" : "");
    if (op == BS_QUERY) {
        SVGP_REQUIRE(g->clip_lo <= g->clip_hi, SVGP_ERR_INVALID, "need clip_lo <= clip_hi (%g, %g)", g->clip_lo, g->clip_hi);
        SVGP_REQUIRE(g->q_slices >= 0 && g->q_slices <= bs_slices_max(g), SVGP_ERR_INVALID, "q_slices=%d: need 0 (the library chooses) .. %d",
                     g->q_slices, bs_slices_max(g));
    }
    if (op == BS_JOINT) {
        SVGP_REQUIRE(g->path_jitter >= 0, SVGP_ERR_INVALID, "need path_jitter >= 0 (%g)", g->path_jitter);
        SVGP_REQUIRE(g->Q <= BPJL_Q_MAX, SVGP_ERR_UNSUPPORTED, "Q=%d: %s takes Q <= %d", g->Q, name, BPJL_Q_MAX);
    }
    return SVGP_OK;
}

// the pointers an operation needs, and the kernels' arguments
int bs_args(const svgp_ball_state_cfg* g, int op, const svgp_ball_state_bufs* q, BsArgs* a, BpjArgs* ja) {
    const bool frames = op == BS_UPDATE, query = op == BS_QUERY || op == BS_JOINT;
    int rc = bp_marshal(g, q, frames, query, a);
    if (!rc) rc = bp_marshal(g, q, frames, query, ja);
    if (rc) return rc;
    SVGP_REQUIRE(query || q->stats, SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(frames || q->post, SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(op != BS_QUERY || (q->p_v_x && q->p_v_y), SVGP_ERR_INVALID, "NULL device pointer");
    a->lo = g->clip_lo; a->hi = g->clip_hi; a->p_v[0] = q->p_v_x; a->p_v[1] = q->p_v_y;
    a->stats = q->stats; a->post = q->post; a->rps = 1;
    ja->jp = g->path_jitter; ja->cov[0] = q->cov_x; ja->cov[1] = q->cov_y; ja->chol[0] = q->chol_x; ja->chol[1] = q->chol_y;
    return SVGP_OK;
}

// workspace of the large routes: the fields of BpFactorWork an operation's steps touch, then its own
struct BsWork { BpFactorWork f; BpTailWork t; BpjTailWork j; int64_t total; };
BsWork bs_work(const svgp_ball_state_cfg* g, int op) {
    const int64_t m = g->m, T = g->T, nb = op == BS_JOINT ? bpj_chunk(g->B, g->Q) : (g->B < BPL_NB ? g->B : BPL_NB);
    SvgpTake16 c16;
    BsWork o = {};
    if (!g->large && op != BS_JOINT) return o;
    switch (op) {
    case BS_UPDATE:
        o.f.K = c16.take(m * m); o.f.Kn = c16.take(T * m); o.f.knn = c16.take(T); o.f.KnP = c16.take(nb * T * m); o.f.PY = c16.take(T * nb);
        break;
    case BS_FINALIZE:       // K from svgp_se1d_kernel_matrix_fwd on one row: Kn (1, m), knn (1)
        o.f.K = c16.take(m * m); o.f.Kn = c16.take(m); o.f.knn = c16.take(1); o.f.Mats = c16.take((nb + 1) * m * m);
        o.f.V = c16.take(m * nb); o.f.W = c16.take(nb * m); o.f.logdet = c16.take(nb + 1);
        o.f.inv = c16.take((int64_t)svgp_spd_inverse_workspace_elems((int)m, (int)nb + 1));
        break;
    case BS_QUERY:
        o.f.Mats = c16.take(nb * m * m); o.f.W = c16.take(nb * m);
        o.t = bp_tail_work(c16, m, g->Q, nb);
        break;
    default:                // X_l is read in place from post; only w_l is gathered
        o.f.W = c16.take(nb * m);
        o.j = bpj_tail_work(c16, m, g->Q, nb);
    }
    o.total = c16.p;
    return o;
}

template <int CW>
int bs_launch_fused(BsStepOp op, const svgp_ball_state_cfg* g, BsArgs a, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a.B, 2);
    int rc;
    switch (op) {
    case BSS_UPDATE:
        hipLaunchKernelGGL(k_ball_state_update<CW>, grid, dim3(256), 0, st, a);
        break;
    case BSS_FINALIZE: {
        const size_t lds = ((size_t)2 * a.m * (a.m + 1) + bp_lds_tail_elems(CW)) * sizeof(real);
        if ((rc = set_dyn_lds(k_ball_state_finalize<CW>, lds))) return rc;
        hipLaunchKernelGGL(k_ball_state_finalize<CW>, grid, dim3(256), lds, st, a);
        break;
    }
    default: {
        const int S = bs_slices(g);
        a.rps = (bs_rounds(g) + S - 1) / S;
        const size_t lds = (size_t)bsq_lds_elems(a.m, CW) * sizeof(real);
        if ((rc = set_dyn_lds(k_ball_state_query<CW>, lds))) return rc;
        hipLaunchKernelGGL(k_ball_state_query<CW>, dim3((unsigned)a.B, 2, (unsigned)S), dim3(256), lds, st, a);
    }
    }
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

int bs_run(const svgp_ball_state_cfg* g, int op, const svgp_ball_state_bufs* q, double* work, void* stream) {
    int rc = bs_check(g, op);
    if (rc) return rc;
    BsArgs a;
    BpjArgs ja;
    if ((rc = bs_args(g, op, q, &a, &ja))) return rc;
    const BsWork w = bs_work(g, op);
    SVGP_REQUIRE(w.total == 0 || work != nullptr, SVGP_ERR_INVALID, "work is NULL (%s: B = %d, T = %d, m = %d, Q = %d needs %lld doubles)",
                 BS_ENTRY[op], g->B, g->T, g->m, g->Q, (long long)w.total);
    const int m = a.m;
    const long long mm = (long long)m * m, E = bs_elems(m);
    hipStream_t st = (hipStream_t)stream;
    BpIn one = a;                    // finalize: K from the kernel-matrix entry, its one "frame" at the first inducing point
    one.T = 1; one.times = a.ip[0];
    return bs_walk(g, op, [&](const BsStep& step) -> int {
        const BpStep& s = step.s;
        const int c = s.c, nb = s.nb;
        real* stats_c = a.stats + ((long long)s.b0 * 2 + c) * E;
        real* post_c = a.post + ((long long)s.b0 * 2 + c) * E;
        switch (step.own) {
        case BSS_UPDATE: case BSS_FINALIZE: case BSS_QUERY:
            return m <= 32 ? bs_launch_fused<32>(step.own, g, a, stream) : bs_launch_fused<64>(step.own, g, a, stream);
        case BSS_GATHER:
            hipLaunchKernelGGL(k_bs_gather, dim3(svgp_blocks(bs_gather_elems(m, nb, op != BS_JOINT))), dim3(SVGP_BLOCK), 0, st, m, c, s.b0, nb,
                               op == BS_FINALIZE ? 1 : 0,
                               op == BS_FINALIZE ? a.stats : a.post, op == BS_JOINT ? nullptr : work + w.f.Mats,
                               work + (op == BS_FINALIZE ? w.f.V : w.f.W));
            SVGP_LAUNCH_CHECK();
            return (int)SVGP_OK;
        case BSS_SCATTER:
            hipLaunchKernelGGL(k_bs_scatter, dim3(svgp_blocks(nb * E)), dim3(SVGP_BLOCK), 0, st, m, c, s.b0, nb, work + w.f.Mats, work + w.f.W,
                               a.post);
            SVGP_LAUNCH_CHECK();
            return (int)SVGP_OK;
        default: break;
        }
        switch (s.op) {
        case BP_KMAT:
            if (op == BS_FINALIZE) { one.times = a.ip[c]; return bp_factor_launch(one, s, w.f, work, stream); }
            return bp_factor_launch(a, s, w.f, work, stream);
        case BP_SIGMA:      // S_l += Kn^T diag(p_l) Kn, in the state's layout
            return svgp_dgemm_batched(1, 0, m, m, a.T, 1.0, work + w.f.Kn, m, 0, work + w.f.KnP, m, (long long)a.T * m, 1.0, stats_c, m, 2 * E,
                                      nb, stream);
        case BP_V:          // r_l += (Kn^T PY)[:, l]: (nb, m) = PY^T Kn with the state's row stride
            return svgp_dgemm_batched(1, 0, nb, m, a.T, 1.0, work + w.f.PY, nb, 0, work + w.f.Kn, m, 0, 1.0, stats_c + mm, (int)(2 * E), 0, 1,
                                      stream);
        case BP_KQ: case BP_ROWS: case BP_FINISH:
            return bp_tail_launch(a, s, w.t, work + w.f.Mats, work + w.f.W, work, stream);
        case BPJ_KQ: case BPJ_G: case BPJ_GK: case BPJ_COV: case BPJ_POTRF: case BPJ_FINISH:      // X_l in place in post
            return bpj_tail_launch(ja, s, w.j, post_c, 2 * E, work + w.f.W, work, stream);
        default:            // BP_SCALE, BP_PRIOR, BP_INVERSE, BP_W, BP_SUB as they are
            return bp_factor_launch(a, s, w.f, work, stream);
        }
    });
}

}  // namespace

extern "C" long long svgp_ball_state_workspace_elems(const svgp_ball_state_cfg* g, int op) {
    if (bs_check(g, op)) return 0;
    return bs_work(g, op).total;
}

extern "C" int svgp_ball_state_route(const svgp_ball_state_cfg* g, int op, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = bs_check(g, op);
    if (rc) return rc;
    int pos = 0;
    buf[0] = 0;
    return bs_walk(g, op, [&](const BsStep& step) -> int {
        if (step.own != BSS_BP) return svgp_route_append(buf, cap, &pos, "%s\n", BSS_NAME[step.own]);
        return bp_route_line(step.s, g->m, buf, cap, &pos);
    });
}

extern "C" int svgp_ball_state_update(const svgp_ball_state_cfg* g, const svgp_ball_state_bufs* q, double* work, void* stream) {
    return bs_run(g, BS_UPDATE, q, work, stream);
}
extern "C" int svgp_ball_state_finalize(const svgp_ball_state_cfg* g, const svgp_ball_state_bufs* q, double* work, void* stream) {
    return bs_run(g, BS_FINALIZE, q, work, stream);
}
extern "C" int svgp_ball_state_query(const svgp_ball_state_cfg* g, const svgp_ball_state_bufs* q, double* work, void* stream) {
    return bs_run(g, BS_QUERY, q, work, stream);
}
extern "C" int svgp_ball_state_query_joint(const svgp_ball_state_cfg* g, const svgp_ball_state_bufs* q, double* work, void* stream) {
    return bs_run(g, BS_JOINT, q, work, stream);
}
