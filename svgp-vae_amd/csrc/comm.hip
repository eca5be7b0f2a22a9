// Data-parallel exchange of the SVGPVAE step over RCCL, enqueued on the SAME stream as the kernels.
//
// The step has three sum-exchanges (SVGPVAE_model.py:328-334,339-340 are the statistics that
// couple batch rows): ws[statA] after phase 0, ws[statB] after phase 1, ws[gradC] after phase 2.  Issuing
// ncclAllReduce from here, on the compute stream, keeps the whole step one in-order queue: no host
// round trip and no cross-stream event wait per collective (each costs ~10 us on this part, the same
// order as the collectives themselves at 135 KB).
//
// RCCL is resolved at run time: the process normally has librccl.so.1 mapped already (PyTorch's), and a
// box without RCCL can still load this library for everything that is not multi-GPU.
#include "common.hpp"
#include <dlfcn.h>
#include <mutex>
#include <rccl/rccl.h>

namespace {

struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*ReduceScatter)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
std::mutex g_rccl_mu;
Rccl g_rccl;

int rccl_get(Rccl** out) {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (!g_rccl.ok) {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);   // the copy the process already uses
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
        if (!h) h = dlopen("librccl.so", RTLD_NOW);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW);
        SVGP_REQUIRE(h != nullptr, SVGP_ERR_UNSUPPORTED, "RCCL not found (librccl.so.1): %s", dlerror());
        g_rccl.handle = h;
#define SYM(field, name)                                                                           \
        *(void**)(&g_rccl.field) = dlsym(h, name);                                                 \
        SVGP_REQUIRE(g_rccl.field != nullptr, SVGP_ERR_UNSUPPORTED, "RCCL symbol %s missing", name)
        SYM(GetUniqueId, "ncclGetUniqueId");
        SYM(CommInitRank, "ncclCommInitRank");
        SYM(CommDestroy, "ncclCommDestroy");
        SYM(AllReduce, "ncclAllReduce");
        SYM(ReduceScatter, "ncclReduceScatter");
        SYM(AllGather, "ncclAllGather");
        SYM(GroupStart, "ncclGroupStart");
        SYM(GroupEnd, "ncclGroupEnd");
        SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
        g_rccl.ok = true;
    }
    *out = &g_rccl;
    return SVGP_OK;
}

#define SVGP_CHECK_RCCL(r, expr)                                                                   \
    do {                                                                                           \
        ncclResult_t _e = (expr);                                                                  \
        if (_e != ncclSuccess) {                                                                   \
            svgp_set_error("%s failed: %s (%s:%d)", #expr, (r)->GetErrorString(_e), __FILE__, __LINE__); \
            return SVGP_ERR_COMM;                                                                  \
        }                                                                                          \
    } while (0)

#define SVGP_COMM_MAX_POINTS 8
struct Comm {
    ncclComm_t comm;
    int rank, nranks;
    // optional per-exchange-point timing of svgp_mnist_train_step_dp (svgp_comm_timing)
    bool timing = false;
    int npoints = 0;
    hipEvent_t ev[2 * SVGP_COMM_MAX_POINTS] = {};
};

// ---- tile-packed symmetric matrices (include/svgpvae_hip.h svgp_sym_pack)
#define SP_T 32
__device__ __forceinline__ void sym_tile_of(int t, int& ti, int& tj) {
    ti = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
}
__global__ __launch_bounds__(256) void k_sym_pack(int m, int avg, long long pe, const double* __restrict__ src,
                                                  double* __restrict__ dst) {
    __shared__ double tr[SP_T][SP_T + 1];
    int ti, tj;
    sym_tile_of((int)blockIdx.x, ti, tj);
    const double* X = src + (size_t)blockIdx.y * m * m;
    double* P = dst + (size_t)blockIdx.y * pe + (size_t)blockIdx.x * SP_T * SP_T;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    if (avg && ti != tj) {                       // the mirrored tile (tj, ti), transposed through LDS
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + 8 * k, gi = tj * SP_T + r, gj = ti * SP_T + c;
            tr[r][c] = (gi < m && gj < m) ? X[(size_t)gi * m + gj] : 0.0;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 8 * k, gi = ti * SP_T + r, gj = tj * SP_T + c;
        double v = (gi < m && gj < m) ? X[(size_t)gi * m + gj] : 0.0;
        if (avg) {
            const double w = ti != tj ? tr[c][r] : ((gi < m && gj < m) ? X[(size_t)gj * m + gi] : 0.0);
            v = 0.5 * (v + w);
        }
        P[r * SP_T + c] = v;
    }
}
__global__ __launch_bounds__(256) void k_sym_unpack(int m, long long pe, const double* __restrict__ src,
                                                    double* __restrict__ dst) {
    __shared__ double tr[SP_T][SP_T + 1];
    int ti, tj;
    sym_tile_of((int)blockIdx.x, ti, tj);
    const double* P = src + (size_t)blockIdx.y * pe + (size_t)blockIdx.x * SP_T * SP_T;
    double* X = dst + (size_t)blockIdx.y * m * m;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 8 * k, gi = ti * SP_T + r, gj = tj * SP_T + c;
        const double v = P[r * SP_T + c];
        tr[r][c] = v;
        // diagonal tiles: the lower part is written here, the upper part below from the transposed read
        if (gi < m && gj < m && (ti != tj || c <= r)) X[(size_t)gi * m + gj] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + 8 * k, gi = tj * SP_T + r, gj = ti * SP_T + c;      // element (r, c) of the mirrored tile
        if (gi < m && gj < m && (ti != tj || c > r)) X[(size_t)gi * m + gj] = tr[c][r];
    }
}

}  // namespace

extern "C" int svgp_comm_unique_id_bytes(void) { return (int)sizeof(ncclUniqueId); }

extern "C" int svgp_comm_unique_id(void* out, int nbytes) {
    SVGP_REQUIRE(out && nbytes == (int)sizeof(ncclUniqueId), SVGP_ERR_INVALID, "unique id buffer must be %d bytes",
                 (int)sizeof(ncclUniqueId));
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    SVGP_CHECK_RCCL(r, r->GetUniqueId((ncclUniqueId*)out));
    return SVGP_OK;
}

extern "C" int svgp_comm_init(const void* unique_id, int nbytes, int rank, int nranks, void** comm_out) {
    SVGP_REQUIRE(unique_id && comm_out && nbytes == (int)sizeof(ncclUniqueId), SVGP_ERR_INVALID,
                 "unique id buffer must be %d bytes", (int)sizeof(ncclUniqueId));
    SVGP_REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, SVGP_ERR_INVALID, "rank %d of %d", rank, nranks);
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    Comm* c = new Comm{nullptr, rank, nranks};
    ncclResult_t e = r->CommInitRank(&c->comm, nranks, id, rank);   // binds to the calling thread's current device
    if (e != ncclSuccess) {
        delete c;
        svgp_set_error("ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, r->GetErrorString(e));
        return SVGP_ERR_COMM;
    }
    *comm_out = c;
    return SVGP_OK;
}

extern "C" int svgp_comm_destroy(void* comm) {
    if (!comm) return SVGP_OK;
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    Comm* c = (Comm*)comm;
    ncclResult_t e = r->CommDestroy(c->comm);
    for (int k = 0; k < 2 * SVGP_COMM_MAX_POINTS; ++k)          // the timing events of svgp_comm_timing
        if (c->ev[k]) (void)hipEventDestroy(c->ev[k]);
    delete c;
    SVGP_REQUIRE(e == ncclSuccess, SVGP_ERR_COMM, "ncclCommDestroy failed: %s", r->GetErrorString(e));
    return SVGP_OK;
}

extern "C" int svgp_allreduce_sum_f64(void* comm, double* buf, int64_t count, void* stream) {
    SVGP_REQUIRE(comm && buf && count >= 0, SVGP_ERR_INVALID, "NULL communicator / buffer");
    if (count == 0) return SVGP_OK;
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    Comm* c = (Comm*)comm;
    SVGP_CHECK_RCCL(r, r->AllReduce(buf, buf, (size_t)count, ncclFloat64, ncclSum, c->comm, (hipStream_t)stream));
    return SVGP_OK;
}

extern "C" int svgp_allreduce_sum_f32(void* comm, float* buf, int64_t count, void* stream) {
    SVGP_REQUIRE(comm && buf && count >= 0, SVGP_ERR_INVALID, "NULL communicator / buffer");
    if (count == 0) return SVGP_OK;
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    Comm* c = (Comm*)comm;
    SVGP_CHECK_RCCL(r, r->AllReduce(buf, buf, (size_t)count, ncclFloat32, ncclSum, c->comm, (hipStream_t)stream));
    return SVGP_OK;
}

// In-place reduce-scatter / all-gather of a buffer of nranks equal chunks: rank r's chunk is buf[r * count, (r + 1) * count).
// Channel-sharded exchange of the large statistics blocks: reduce-scatter S (L,m,m) over the channels,
// every rank factors its L / nranks channels, all-gather of what the row stage needs.
extern "C" int svgp_reduce_scatter_sum_f64(void* comm, double* buf, int64_t count_per_rank, void* stream) {
    SVGP_REQUIRE(comm && buf && count_per_rank >= 0, SVGP_ERR_INVALID, "NULL communicator / buffer");
    if (count_per_rank == 0) return SVGP_OK;
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    Comm* c = (Comm*)comm;
    SVGP_CHECK_RCCL(r, r->ReduceScatter(buf, buf + (size_t)c->rank * count_per_rank, (size_t)count_per_rank, ncclFloat64, ncclSum,
                                        c->comm, (hipStream_t)stream));
    return SVGP_OK;
}
extern "C" int svgp_allgather_f64(void* comm, double* buf, int64_t count_per_rank, void* stream) {
    SVGP_REQUIRE(comm && buf && count_per_rank >= 0, SVGP_ERR_INVALID, "NULL communicator / buffer");
    if (count_per_rank == 0) return SVGP_OK;
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    Comm* c = (Comm*)comm;
    SVGP_CHECK_RCCL(r, r->AllGather(buf + (size_t)c->rank * count_per_rank, buf, (size_t)count_per_rank, ncclFloat64, c->comm,
                                    (hipStream_t)stream));
    return SVGP_OK;
}

extern "C" int64_t svgp_sym_packed_elems(int m) {
    if (m < 1) return 0;
    const int64_t nt = (m + SP_T - 1) / SP_T;
    return nt * (nt + 1) / 2 * SP_T * SP_T;
}
extern "C" int svgp_sym_pack(int m, int L, int avg, const double* src, double* dst, void* stream) {
    SVGP_REQUIRE(m >= 1 && L >= 0 && src && dst, SVGP_ERR_INVALID, "bad argument");
    if (L == 0) return SVGP_OK;
    const int nt = (m + SP_T - 1) / SP_T;
    hipLaunchKernelGGL(k_sym_pack, dim3(nt * (nt + 1) / 2, L), dim3(256), 0, (hipStream_t)stream, m, avg,
                       (long long)svgp_sym_packed_elems(m), src, dst);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}
extern "C" int svgp_sym_unpack(int m, int L, const double* src, double* dst, void* stream) {
    SVGP_REQUIRE(m >= 1 && L >= 0 && src && dst, SVGP_ERR_INVALID, "bad argument");
    if (L == 0) return SVGP_OK;
    const int nt = (m + SP_T - 1) / SP_T;
    hipLaunchKernelGGL(k_sym_unpack, dim3(nt * (nt + 1) / 2, L), dim3(256), 0, (hipStream_t)stream, m,
                       (long long)svgp_sym_packed_elems(m), src, dst);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_comm_group_begin(void* comm) {
    SVGP_REQUIRE(comm, SVGP_ERR_INVALID, "NULL communicator");
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    SVGP_CHECK_RCCL(r, r->GroupStart());
    return SVGP_OK;
}
extern "C" int svgp_comm_group_end(void* comm) {
    SVGP_REQUIRE(comm, SVGP_ERR_INVALID, "NULL communicator");
    Rccl* r;
    int rc = rccl_get(&r);
    if (rc) return rc;
    SVGP_CHECK_RCCL(r, r->GroupEnd());
    return SVGP_OK;
}

extern "C" int svgp_comm_timing(void* comm, int enable) {
    SVGP_REQUIRE(comm, SVGP_ERR_INVALID, "NULL communicator");
    Comm* c = (Comm*)comm;
    if (enable && !c->ev[0])
        for (int k = 0; k < 2 * SVGP_COMM_MAX_POINTS; ++k) SVGP_CHECK_HIP(hipEventCreate(&c->ev[k]));
    c->timing = enable != 0;
    c->npoints = 0;
    return SVGP_OK;
}
extern "C" int svgp_comm_timing_read(void* comm, float* us, int cap, int* n) {
    SVGP_REQUIRE(comm && us && n && cap >= 0, SVGP_ERR_INVALID, "bad argument");
    Comm* c = (Comm*)comm;
    *n = 0;
    for (int k = 0; k < c->npoints && k < cap; ++k) {
        float ms = 0;
        SVGP_CHECK_HIP(hipEventSynchronize(c->ev[2 * k + 1]));
        SVGP_CHECK_HIP(hipEventElapsedTime(&ms, c->ev[2 * k], c->ev[2 * k + 1]));
        us[k] = ms * 1000.0f;
        *n = k + 1;
    }
    return SVGP_OK;
}

// One data-parallel step, everything enqueued on `stream`:
//   phase 0 | all-reduce statA | phase 1 | all-reduce statB | phase 2 | all-reduce gradC | phase 3
// c->b is this rank's row count, c->b_global the global batch, c->rep_weight 1 on exactly one rank.
//
// Large-m path (m > 64) with L divisible by the rank count (Hensman branch): the channel-sharded schedule instead
//  -- the (L,m,m) statistics are reduce-SCATTERED over the channels, every rank factors its L / G channels
// (svgp_gp_factor_*_channels) and what the row stages need is all-gathered:
//   encoder + kernel matrices + statistics | reduce-scatter S, v | window factor stage | all-gather Sigma^-1, t, u |
//   row stage, decoder fwd + bwd, backward statistics | reduce-scatter A2, ud, td | window reverse factor stage |
//   all-gather Ssym, vbar, KL (round 4: M2 = Ki A Ki is neither formed nor exchanged, gp_large.hip "W form") |
//   row gradients, kernel-matrix VJP (every rank's Kbar share counts), encoder reverse pass,
//   gradient reduction | all-reduce gradC | phase 3
// At config 3 on 8 ranks: 2 channels of 256 x 256 per rank instead of 16, 8.4 MB blocks moved as 7/8 of their size.
namespace {
int rs(void* comm, double* p, int64_t total, int nranks, void* stream) {
    return svgp_reduce_scatter_sum_f64(comm, p, total / nranks, stream);
}
int ag(void* comm, double* p, int64_t total, int nranks, void* stream) { return svgp_allgather_f64(comm, p, total / nranks, stream); }
// exchange-point bracket: optional events + one RCCL group
struct Point {
    Comm* cm; hipStream_t st; int idx;
    int begin() {
        idx = -1;
        if (cm->timing && cm->npoints < SVGP_COMM_MAX_POINTS) {
            idx = cm->npoints++;
            SVGP_CHECK_HIP(hipEventRecord(cm->ev[2 * idx], st));
        }
        return SVGP_OK;
    }
    int end() {
        if (idx >= 0) SVGP_CHECK_HIP(hipEventRecord(cm->ev[2 * idx + 1], st));
        return SVGP_OK;
    }
};
}  // namespace
extern "C" int svgp_dp_pack_default(int m) { return svgp_dp_pack_rule(m) ? 1 : 0; }

// One exchange op of a step plan (step_plan.hpp) on the communicator a.comm, enqueued on `stream`.  An all-reduce is an exchange
// point of its own; points 1..4 of the channel-sharded form are bracketed by STEP_POINT_BEGIN / _END ops.
int svgp_step_exchange(const StepOp& op, const StepArgs& a, void* stream, int* point) {
    Comm* cm = (Comm*)a.comm;
    SVGP_REQUIRE(cm && a.wl, SVGP_ERR_INVALID, "step plan: an exchange op without a communicator");
    const svgp_mnist_ws_layout& wl = *a.wl;
    Point pt{cm, (hipStream_t)stream, *point};
    const int G = cm->nranks, L = a.c->L, m = a.c->m;
    const int64_t mm = (int64_t)m * m, Lm = (int64_t)L * m;
    int rc = SVGP_OK;
    if (op.kind == STEP_POINT_BEGIN || op.kind == STEP_POINT_END) {
        rc = op.kind == STEP_POINT_BEGIN ? pt.begin() : pt.end();
        *point = op.kind == STEP_POINT_BEGIN ? pt.idx : -1;
        return rc;
    }
    // the blocks in the order of SVGP_STEP_BLOCKS: offset, elements (the members of points 1..4: over all channels)
    static_assert(STEP_BLK_gradC_lo == 4 && STEP_BLK_S == 5 && STEP_BLK_KL == 15 && STEP_BLK_COUNT == 16, "the two tables below");
    const int64_t off[STEP_BLK_COUNT] = {wl.statA, wl.statB, wl.gradC, wl.gradC + a.n_enc, wl.gradC, wl.S, wl.v, wl.Si, wl.t, wl.u,
                                         wl.A2, wl.ud, wl.td, wl.Ssym, wl.vbar, wl.KL};
    const int64_t len[STEP_BLK_COUNT] = {wl.statA_len, wl.statB_len, wl.gradC_len, wl.gradC_len - a.n_enc, a.n_enc, L * mm, Lm, L * mm,
                                         Lm, Lm, L * mm, Lm, Lm, L * mm, Lm, L};
    SVGP_REQUIRE(op.arg < STEP_BLK_COUNT && (op.arg <= STEP_BLK_gradC_lo) == (op.kind == STEP_ALLREDUCE), SVGP_ERR_INVALID,
                 "step plan: op kind %d on block %u", (int)op.kind, op.arg);
    double* blk = a.ws + off[op.arg];
    if (op.kind == STEP_ALLREDUCE) {
        if ((rc = pt.begin())) return rc;
        if ((rc = svgp_allreduce_sum_f64(cm, blk, len[op.arg], stream))) return rc;
        return pt.end();
    }
    // a symmetric (L,m,m) block on the wire: the tile-packed buffer (all channels / the rank's window) or the block itself
    const int64_t pe = svgp_sym_packed_elems(m);
    double* xp0 = a.ws + wl.xpack;
    const int l0 = a.l0, nl = a.nl, hi0 = l0 + nl;
    switch (op.kind) {
    case STEP_REDUCE_SCATTER:
        return op.part == STEP_PART_PACKED ? rs(cm, xp0, L * pe, G, stream) : rs(cm, blk, len[op.arg], G, stream);
    case STEP_ALLGATHER:
        return op.part == STEP_PART_PACKED ? ag(cm, xp0, L * pe, G, stream) : ag(cm, blk, len[op.arg], G, stream);
    case STEP_PACK:
        return op.part == STEP_PART_WINDOW ? svgp_sym_pack(m, nl, 0, blk + (size_t)l0 * mm, xp0 + (size_t)l0 * pe, stream)
                                           : svgp_sym_pack(m, L, 0, blk, xp0, stream);
    case STEP_UNPACK:
        if (op.part == STEP_PART_WINDOW) return svgp_sym_unpack(m, nl, xp0 + (size_t)l0 * pe, blk + (size_t)l0 * mm, stream);
        if (op.part == STEP_PART_ALL) return svgp_sym_unpack(m, L, xp0, blk, stream);
        // the other ranks' windows (the side branch reads the rank's own window only)
        if ((rc = svgp_sym_unpack(m, l0, xp0, blk, stream))) return rc;
        return svgp_sym_unpack(m, L - hi0, xp0 + (size_t)hi0 * pe, blk + (size_t)hi0 * mm, stream);
    }
    svgp_set_error("step plan: op kind %d is no exchange", (int)op.kind);
    return SVGP_ERR_INVALID;
}

// The schedule of every form is step_plan's (step_plan.hpp); the stages of the channel-sharded form run on a copy of the
// configuration with rep_weight 1 (Kbar = this rank's channel-window share: every share counts).
extern "C" int svgp_mnist_train_step_dp(const svgp_mnist_cfg* c, void* comm, double* theta, const double* images,
                                        const double* aux, const double* eps, double* ws, double* state,
                                        double* adam_m, double* adam_v, void* stream) {
    SVGP_REQUIRE(c && comm, SVGP_ERR_INVALID, "NULL cfg / communicator");
    svgp_mnist_ws_layout wl;
    int rc = svgp_mnist_ws_layout_get(c, &wl);
    if (rc) return rc;
    Comm* cm = (Comm*)comm;
    const SvgpSched sc = sched_read();
    StepPlan P;
    rc = svgp_step_plan_checked(c, STEP_FORM_DP, 0, cm->nranks, cm->rank, adam_m != nullptr, false, sc, P);
    if (rc) return rc;
    svgp_mnist_cfg cc = *c;
    if (P.sharded) cc.rep_weight = 1.0;
    StepArgs a{&cc, theta, images, aux, eps, ws, state, adam_m, adam_v, comm, &wl};
    if (c->split_grad_exchange) {
        svgp_mnist_param_layout pl;
        rc = svgp_mnist_param_layout_get(c, &pl);
        if (rc) return rc;
        a.n_enc = pl.n_enc;
    }
    if (P.sharded) { a.nl = c->L / cm->nranks; a.l0 = cm->rank * a.nl; }
    SVGP_REQUIRE(!P.pack || wl.xpack_len >= (int64_t)c->L * svgp_sym_packed_elems(c->m), SVGP_ERR_INVALID,
                 "the packed exchange needs the workspace's wire buffer: lay the workspace out with cfg.single_stat_block = 1");
    if (cm->timing) cm->npoints = 0;
    return svgp_step_run(P, a, stream, sc);
}
