// C-ABI glue: error strings, layouts, phase orchestration, HIP graph / event helpers.
#include <cstdarg>

#include "common.hpp"
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <cstdlib>
#include <algorithm>

static thread_local char g_err[512] = "";

void svgp_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* svgp_last_error(void) { return g_err; }
extern "C" int svgp_version(void) { return SVGP_VERSION_MAJOR * 100 + SVGP_VERSION_MINOR; }
extern "C" int svgp_struct_sizeof(int which) {
    switch (which) {
    case 0: return (int)sizeof(svgp_mnist_cfg);
    case 1: return (int)sizeof(svgp_mnist_param_layout);
    case 2: return (int)sizeof(svgp_mnist_ws_layout);
    case 3: return (int)sizeof(svgp_stream_kdesc);
    case 4: return (int)sizeof(svgp_conv_desc);
    case 5: return (int)sizeof(svgp_sprites_kcfg);
    case 6: return (int)sizeof(svgp_pearce_bufs);
    case 7: return (int)sizeof(svgp_sum_job);
    case 8: return (int)sizeof(svgp_casale_cfg);
    case 9: return (int)sizeof(svgp_casale_layout);
    case 10: return (int)sizeof(svgp_ball_large_cfg);
    case 11: return (int)sizeof(svgp_mnist_cache_layout);
    case 13: return (int)sizeof(svgp_ball_predict_cfg);       // (12 stays unassigned: tests/test_generate_cpu.py pins it to -1)
    case 14: return (int)sizeof(svgp_ball_predict_bufs);
    case 15: return (int)sizeof(svgp_pearce_predict_cfg);
    case 16: return (int)sizeof(svgp_pearce_predict_bufs);
    case 18: return (int)sizeof(svgp_casale_cache_layout);    // (17 stays unassigned: tests/test_pearce_predict_cpu.py pins it to -1)
    case 19: return (int)sizeof(svgp_cvae_cfg);
    case 20: return (int)sizeof(svgp_cvae_ws_layout);
    case 22: return (int)sizeof(svgp_ball_predict_joint_cfg); // (21 stays unassigned: pinned to -1 by the tests)
    case 23: return (int)sizeof(svgp_ball_predict_joint_bufs);
    case 25: return (int)sizeof(svgp_ball_state_cfg);         // (24 stays unassigned: pinned to -1 by the tests)
    case 26: return (int)sizeof(svgp_ball_state_bufs);
    default: return -1;
    }
}

int svgp_check_cfg(const svgp_mnist_cfg* c) {
    SVGP_REQUIRE(c != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(c->b >= 1 && c->b_global >= c->b, SVGP_ERR_INVALID, "need 1 <= b <= b_global (b=%d b_global=%d)",
                 c->b, c->b_global);
    SVGP_REQUIRE(c->m >= 1 && c->L >= 1 && c->M >= 1 && c->n_obj >= 0, SVGP_ERR_INVALID,
                 "bad shape m=%d L=%d M=%d n_obj=%d", c->m, c->L, c->M, c->n_obj);
    SVGP_REQUIRE(c->m <= SVGP_M_LIMIT, SVGP_ERR_UNSUPPORTED,
                 "m=%d inducing points: this build supports m <= %d", c->m, SVGP_M_LIMIT);
    SVGP_REQUIRE(c->M <= 128, SVGP_ERR_UNSUPPORTED, "M=%d: object-vector dimension > 128 not supported", c->M);
    SVGP_REQUIRE(c->L <= 64, SVGP_ERR_UNSUPPORTED, "L=%d: more than 64 latent channels not supported", c->L);
    SVGP_REQUIRE(c->N_train > 0 && c->jitter >= 0, SVGP_ERR_INVALID, "bad N_train / jitter");
    SVGP_REQUIRE(c->kl_form == 0 || c->kl_form == 1, SVGP_ERR_INVALID, "kl_form=%d (0 or 1)", c->kl_form);
    SVGP_REQUIRE(c->clip_pv >= 0 && c->clip_pv <= 2, SVGP_ERR_INVALID, "clip_pv=%d (0, 1 or 2)", c->clip_pv);
    SVGP_REQUIRE(c->gemm_f32 >= 0 && c->gemm_f32 <= 2, SVGP_ERR_INVALID, "gemm_f32=%d (0, 1 or 2)", c->gemm_f32);
    // every rank must take the same exchange schedule: a stray non-zero value would switch only some ranks to two messages
    SVGP_REQUIRE(c->split_grad_exchange == 0 || c->split_grad_exchange == 1, SVGP_ERR_INVALID,
                 "split_grad_exchange=%d (0 or 1)", c->split_grad_exchange);
    SVGP_REQUIRE(!(c->kl_form && c->m > SVGP_M_MAX), SVGP_ERR_UNSUPPORTED,
                 "kl_form=1 (moving-ball SVGP) is implemented for m <= %d inducing points (m=%d)", SVGP_M_MAX, c->m);
    SVGP_REQUIRE(!(c->kl_form && c->b != c->b_global), SVGP_ERR_UNSUPPORTED,
                 "kl_form=1 couples all channels of the batch; it is not sharded over ranks");
    return SVGP_OK;
}

// The two layouts as functions of a configuration that has ALREADY been validated by its entry point: svgp_check_cfg for the
// svgp_mnist_* queries below, the checks of csrc/ball_large.hip for the moving-ball large engine (which lifts the 64-channel and
// the kl_form = 1 / m <= 64 refusals of svgp_check_cfg for its own entry points only).
static void param_layout_fill(const svgp_mnist_cfg* c, svgp_mnist_param_layout* o) {
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
    o->enc_c1_w = take(3 * 3 * 1 * 8);  o->enc_c1_b = take(8);
    o->enc_c2_w = take(3 * 3 * 8 * 8);  o->enc_c2_b = take(8);
    o->enc_c3_w = take(3 * 3 * 8 * 8);  o->enc_c3_b = take(8);
    o->enc_d_w = take(32 * 2 * c->L);   o->enc_d_b = take(2 * c->L);
    o->n_enc = p;
    o->dec_d_w = take((int64_t)c->L * 128); o->dec_d_b = take(128);
    o->dec_c1_w = take(3 * 3 * 8 * 8);  o->dec_c1_b = take(8);
    o->dec_c2_w = take(3 * 3 * 8 * 8);  o->dec_c2_b = take(8);
    o->dec_c3_w = take(3 * 3 * 8 * 1);  o->dec_c3_b = take(1);
    o->n_vae = p;
    o->ip = take((int64_t)c->m * (2 + c->M));
    o->l_GP = take(1);
    o->amplitude = take(1);
    o->ov = take((int64_t)c->n_obj * c->M);
    o->n_total = p;
}

extern "C" int svgp_mnist_param_layout_get(const svgp_mnist_cfg* c, svgp_mnist_param_layout* o) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(o != nullptr, SVGP_ERR_INVALID, "out is NULL");
    param_layout_fill(c, o);
    return SVGP_OK;
}

extern "C" int svgp_mnist_ws_layout_get(const svgp_mnist_cfg* c, svgp_mnist_ws_layout* o) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(o != nullptr, SVGP_ERR_INVALID, "out is NULL");
    SVGP_REQUIRE(c->b_cap == 0 || c->b_cap >= c->b, SVGP_ERR_INVALID, "b_cap=%d < b=%d", c->b_cap, c->b);
    return svgp_ws_layout_fill(c, o, false);
}

// ball_large: the workspace of one latent coordinate of the moving-ball large engine (csrc/ball_large.hip) -- the fields of the
// large-m GP stages at EVERY m (also m <= SVGP_M_MAX, which that engine runs on the large-m kernels), none of the MNIST
// networks' fields, and scratch floors for small m where the large-m stages otherwise rely on m > SVGP_M_MAX.
int svgp_ws_layout_fill(const svgp_mnist_cfg* c, svgp_mnist_ws_layout* o, bool ball_large) {
    svgp_mnist_param_layout pl;
    param_layout_fill(c, &pl);
    const bool big = ball_large || c->m > SVGP_M_MAX;
    svgp_mnist_cfg cc = *c;              // layout is a function of the capacity, not of the current rows
    cc.b = c->b_cap > 0 ? c->b_cap : c->b;
    const int64_t b = cc.b, m = c->m, L = c->L, M = c->M;
    int64_t p = 0;
    // every field starts on a 16-element (128-byte) boundary
    auto take = [&](int64_t n) { int64_t r = p; p += (n + 15) / 16 * 16; return r; };
    auto vae = [&](int64_t n) { return take(ball_large ? 0 : n); };      // fields of the MNIST networks
    o->enc_a1 = vae(b * 13 * 13 * 8); o->enc_a2 = vae(b * 6 * 6 * 8); o->enc_a3 = vae(b * 32);
    o->qnet_mu = take(b * L); o->qnet_var_raw = take(b * L); o->qnet_var = take(b * L);
    // m > 64: the rows W = Kn Ki K (gp_large.hip, "W form") sit right behind the CURRENT b rows of K_nm, so that [Kn; W] is
    // one (2 b, m) operand of the row-stage product and of the reverse statistic
    o->K = take(m * m); o->Kn = take(big ? 2 * b * m : b * m); o->knn = take(b);
    const int64_t P = svgp_stat_parts(c);      // capacity from b_cap
    o->stat_parts = P;
    o->statA = p; o->S = p; p += P * L * m * m; o->v = p; p += P * L * m;
    o->tit_S2 = p; if (c->titsias) p += L * m * m;
    o->tit_v2 = p; if (c->titsias) p += L * m;
    o->statA_len = p - o->statA; take(0);
    // Si (L,m,m) and Ki (m,m) form ONE contiguous (L+1, m, m) block whenever that keeps Ki on a 16-element boundary
    // (m a multiple of 4): the large-m path then inverts them as one batch
    o->ldK = take(1);
    o->Si = take(L * m * m + ((L * m * m) % 16 == 0 ? m * m : 0));
    o->Ki = (L * m * m) % 16 == 0 ? o->Si + L * m * m : take(m * m);
    o->t = take(L * m); o->G = take(L * m * m); o->A = take(L * m * m);
    // (M2 = Ki A Ki and Qm exist on the LDS-resident path only: the large-m path evaluates k^T M2 k as w^T Si w)
    o->Aji = take(L * m * m); o->mu_hat = take(L * m); o->u = take(L * m); o->M2 = take(big ? 0 : L * m * m);
    o->KL = take(2 * L); o->q = take(b);   // [KL | kl_form 1: tr(Ki A_l A_l)]
    o->p_m = take(b * L); o->p_v = take(b * L); o->e = take(b * L); o->d = take(b * L);
    o->eps = take(b * L); o->z = take(b * L);
    o->dec_h0 = vae(b * 128); o->dec_a1 = vae(b * 512); o->dec_a2 = vae(b * 1568); o->recon = vae(b * 784);
    o->dec_d2 = vae(b * 1568); o->dec_d1 = vae(b * 512); o->dec_dh0 = vae(b * 128); o->dec_weff = vae(2176);
    o->flags = take(64);
    o->zbar = take(b * L); o->g_pv = take(b * L); o->g_pm = take(b * L); o->mvbar = take(b * L);
    o->statB = p; o->A2 = p; p += P * L * m * m; o->ud = p; p += P * L * m; o->td = p; p += P * L * m;
    o->statB_len = p - o->statB; take(0);
    o->Kbar = take(m * m); o->fb_part = take(ball_large ? svgp_ball_large_fb_part_elems(m, L) : 2 * L * m * m); o->Qm = take(big ? 0 : L * m * m); o->vbar = take(L * m);
    // (the Titsias reverse stage keeps W | cA | cB, b m + 2 b L elements, here: more than L b m only when (L - 1) m < 2 L)
    o->Ssym = take(L * m * m); o->Knbar_part = take(ball_large || c->titsias ? std::max(L * b * m, b * m + 2 * b * L) : L * b * m);
    // scratch of the large-m path (gp_large.hip)
    // m > 64: (L,b,m) scratch + the forward products [Kn; W] Si_l (L,2b,m), Kn Ki (b,m) kept for the reverse pass + X (b,2m)
    o->scr_bm = take(big ? 3 * L * b * m + 3 * b * m : L * b * m); o->scr_mm = take(4 * L * m * m);
    o->scr_vec = take(3 * L * m + 3 * L + 16 + b);
    o->scr_inv = take((int64_t)svgp_spd_inverse_workspace_elems((int)m, (int)L + 1)); o->scr_bl = take(2 * b * L);
    // m > 64: ten channel-independent m x m matrices + the split-K scratch of the (2 m, m, b) row contraction of the W form (K Ki, Kn^T Wbar, Kn^T diag(qbar) Kn, channel sums, temporaries)
    o->scr_sm = take(big ? 10 * m * m + svgp_dgemm_splitk_scratch_elems((int)(2 * m), (int)m, (int)b) : 0);
    o->Knbar = take(b * m); o->knnbar = take(b); o->ybar = take(b * L); o->s2bar = take(b * L);
    o->d_on = take(b * M);
    o->n_part = svgp_n_part(&cc);
    o->part_dec = vae(o->n_part * (pl.n_vae - pl.n_enc));
    o->part_enc = vae(o->n_part * pl.n_enc);
    o->part_gp = take((m + svgp_n_postblk(&cc)) * 2);
    o->n_post = (int64_t)L * svgp_n_postblk(&cc);
    o->part_sums = take(o->n_part * 4 + o->n_post * 2);
    o->gradC = p; o->grad = p; p += ball_large ? 0 : pl.n_total; o->sums = p; p += 8; o->gradC_len = p - o->gradC; take(0);
    o->tit_Si = take(c->titsias ? L * m * m : 0); o->tit_t = take(c->titsias ? L * m : 0);
    o->tit_scal = take(c->titsias ? 2 * L + 1 : 0);
    // the wire buffer of the channel-sharded exchange: one tile-packed (L, m, m) block; only when the batch is sharded over
    // ranks (cfg.single_stat_block, set by the engines for world sizes > 1): a single-GPU workspace does not carry it
    o->xpack_len = (big && !ball_large && c->single_stat_block) ? L * svgp_sym_packed_elems((int)m) : 0;
    o->xpack = take(o->xpack_len);
    o->total = p;
    return SVGP_OK;
}

// ---------------------------------------------------------------------------------------------
// phases
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Side streams.  Most stages of the step are short dependent launches that fill only a part of the chip
// (the GP factor kernels run L workgroups on 256 CUs), so work that is OFF the critical path -- the
// kernel-matrix reverse pass and the VAE weight gradients -- is forked onto a library-owned side stream
// and joined where its result is consumed.  hipEventRecord / hipStreamWaitEvent are capturable, so under
// stream capture the fork becomes a parallel branch of the hipGraph.
// ---------------------------------------------------------------------------------------------
namespace {
// One Side per (device, caller stream): two engines that enqueue on different streams (or from different threads) never
// share a fork event, a join decision or a side stream.  `open[k]` (branch k forked and not yet joined) and `early_ws`
// (workspaces whose early reverse factor half was issued by a stand-alone phase 1 and not yet consumed by a stand-alone phase 2;
// the whole-step forms do not touch it) are only touched under the Side's own mutex, which fork / join hold for the whole
// record + wait pair.
struct Side {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr, done[2] = {nullptr, nullptr};
    bool open[2] = {false, false};
    std::set<const void*> early_ws;
    std::mutex mu;
};
std::mutex g_side_mu;
std::map<std::pair<int, hipStream_t>, Side*> g_side;

// ---- do two streams run concurrently?  HIP maps streams onto a small pool of hardware queues (GPU_MAX_HW_QUEUES, 4 by default)
// in creation order; two streams that share a queue execute one after the other whatever events say.  Which streams collide
// depends on every stream the process has created so far -- torch's, RCCL's, ours: measured round 4, config 3 with a 1-rank RCCL
// communicator: the library's side branch shared the caller's queue and hid NOTHING (1.454 ms against 1.313 ms with 8 queues), while
// the SPRITES step lost 5 ms with 8 queues for the same reason in the other direction.  So the side streams are chosen by a
// probe instead of by luck: a ~40 us single-workgroup spin on stream a, an empty kernel on stream b issued right behind it; b
// runs beside a iff its kernel finishes well before the spin does.
__global__ void k_spin(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
__global__ void k_noop() {}
int streams_overlap(hipStream_t a, hipStream_t b, bool* out) {
    hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
    SVGP_CHECK_HIP(hipEventCreate(&e0)); SVGP_CHECK_HIP(hipEventCreate(&ea)); SVGP_CHECK_HIP(hipEventCreate(&eb));
    int votes = 0;
    for (int rep = 0; rep < 3; ++rep) {
        SVGP_CHECK_HIP(hipStreamSynchronize(a)); SVGP_CHECK_HIP(hipStreamSynchronize(b));
        SVGP_CHECK_HIP(hipEventRecord(e0, a));
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, 4000LL);        // 100 MHz wall clock: 40 us
        SVGP_CHECK_HIP(hipEventRecord(ea, a));
        hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, b);
        SVGP_CHECK_HIP(hipEventRecord(eb, b));
        SVGP_CHECK_HIP(hipEventSynchronize(ea)); SVGP_CHECK_HIP(hipEventSynchronize(eb));
        float ta = 0, tb = 0;
        SVGP_CHECK_HIP(hipEventElapsedTime(&ta, e0, ea));
        SVGP_CHECK_HIP(hipEventElapsedTime(&tb, e0, eb));
        if (tb < 0.6f * ta) ++votes;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    *out = votes >= 2;
    return SVGP_OK;
}

int side_get(hipStream_t main, const SvgpSched& sc, Side** out) {
    int dev = 0;
    SVGP_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto key = std::make_pair(dev, main);
    auto it = g_side.find(key);
    if (it == g_side.end()) {
        Side* sd = new Side();
        // Two side streams that run concurrently with the caller's stream AND with each other, picked from up to 12 candidates by
        // the probe above.  Not under stream capture (the probe synchronises) and not with SVGP_STREAM_PROBE=0: then the first two.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(main, &cap);
        const bool probe = cap == hipStreamCaptureStatusNone && sc.stream_probe;
        hipStream_t cand[12];
        int n_cand = 0, picked = 0;
        while (picked < 2 && n_cand < (probe ? 12 : 2)) {
            hipStream_t c = nullptr;
            SVGP_CHECK_HIP(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
            cand[n_cand++] = c;
            bool ok = true;
            if (probe) {
                int rc = streams_overlap(main, c, &ok);
                if (rc) return rc;
                if (ok && picked == 1) { rc = streams_overlap(sd->s[0], c, &ok); if (rc) return rc; }
            }
            if (ok) sd->s[picked++] = c;
        }
        for (int i = 0; i < n_cand; ++i) {           // candidates that collide with the caller's stream (or with each other) go back
            if (cand[i] == sd->s[0] || cand[i] == sd->s[1]) continue;
            if (picked < 2) sd->s[picked++] = cand[i];                      // fewer than two concurrent queues exist: take what there is
            else (void)hipStreamDestroy(cand[i]);
        }
        for (int k = 0; k < 2; ++k) SVGP_CHECK_HIP(hipEventCreateWithFlags(&sd->done[k], hipEventDisableTiming));
        SVGP_CHECK_HIP(hipEventCreateWithFlags(&sd->fork, hipEventDisableTiming));
        it = g_side.emplace(key, sd).first;
    }
    *out = it->second;
    return SVGP_OK;
}
// side stream k continues after everything issued on `main` so far
int side_fork(Side* sd, int k, hipStream_t main) {
    std::lock_guard<std::mutex> lk(sd->mu);
    SVGP_CHECK_HIP(hipEventRecord(sd->fork, main));
    SVGP_CHECK_HIP(hipStreamWaitEvent(sd->s[k], sd->fork, 0));
    sd->open[k] = true;
    return SVGP_OK;
}
// `main` continues after everything issued on side stream k (no-op when this Side's branch k is not open)
int side_join(Side* sd, int k, hipStream_t main) {
    std::lock_guard<std::mutex> lk(sd->mu);
    if (!sd->open[k]) return SVGP_OK;
    SVGP_CHECK_HIP(hipEventRecord(sd->done[k], sd->s[k]));
    SVGP_CHECK_HIP(hipStreamWaitEvent(main, sd->done[k], 0));
    sd->open[k] = false;
    return SVGP_OK;
}
void side_mark_early(Side* sd, const void* ws) { std::lock_guard<std::mutex> lk(sd->mu); sd->early_ws.insert(ws); }
bool side_take_early(Side* sd, const void* ws) { std::lock_guard<std::mutex> lk(sd->mu); return sd->early_ws.erase(ws) > 0; }

}  // namespace

// cholesky.hip (look-ahead of the blocked factorisation, branch 0): side branch k of the caller's stream.
// _fork: the branch continues after everything issued on the caller's stream so far (re-forking an open branch just adds
// that dependency); _join: the caller's stream continues after everything issued on the branch.
int svgp_side_branch_fork(const SvgpSched& sc, void* main_stream, void** side_stream_out, int k) {
    Side* sd = nullptr;
    int rc = side_get((hipStream_t)main_stream, sc, &sd);
    if (rc) return rc;
    rc = side_fork(sd, k, (hipStream_t)main_stream);
    if (rc) return rc;
    *side_stream_out = (void*)sd->s[k];
    return SVGP_OK;
}
int svgp_side_branch_join(void* main_stream, int k) {
    int dev = 0;
    SVGP_CHECK_HIP(hipGetDevice(&dev));
    Side* sd = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(std::make_pair(dev, (hipStream_t)main_stream));
        if (it == g_side.end()) return SVGP_OK;                 // never forked: nothing to join
        sd = it->second;
    }
    return side_join(sd, k, (hipStream_t)main_stream);
}

// ---- the step: step_plan (step_plan.hpp) decides, svgp_step_run executes, svgp_mnist_step_route prints.  The schedule switches
// (sched.hpp) are read once per exported call and arrive in `sc`; a caller must not change SVGP_DEC_SPLIT between phase 1 and
// phase 2 of a step.
int svgp_step_plan_checked(const svgp_mnist_cfg* c, int form, int phase, int nranks, int rank, bool adam, bool early_issued,
                           const SvgpSched& sc, StepPlan& P) {
    SVGP_REQUIRE(form != STEP_FORM_PHASE || (phase >= 0 && phase <= 5), SVGP_ERR_INVALID, "phase %d out of range 0..5", phase);
    SVGP_REQUIRE(step_plan(c, form, phase, nranks, rank, adam, early_issued, sc, P) == SVGP_OK, SVGP_ERR_INVALID,
                 "no step plan for form %d (0 phase, 1 step, 2 data parallel), rank %d of %d", form, rank, nranks);
    return SVGP_OK;
}

namespace {
// split: StepPlan::fwd_split -- the four slots below that have a second form run it
int step_stage(const StepOp& op, const StepArgs& a, void* st, const SvgpSched& sc, bool split) {
    const svgp_mnist_cfg* c = a.c;
    if (split) {
        switch (op.stage) {
        case STEP_ST_FACTOR_FWD_DEFER_AJI: return svgp_gp_factor_fwd_head(c, a.ws, st);
        case STEP_ST_POST_FWD: return svgp_gp_posterior_fwd_z(c, a.eps, a.ws, a.state, st);
        case STEP_ST_DEC_FUSED_AJI: return svgp_mnist_decoder_fwd_bwd_data_pre_tail(c, a.theta, a.images, a.ws, a.state, st);
        case STEP_ST_POST_BWD_ROWS: return svgp_gp_posterior_bwd_rows_d(c, a.ws, a.state, st);
        case STEP_ST_POST_BWD_FINAL: return svgp_gp_posterior_bwd_with_final_d(c, a.ws, a.state, st);
        default: break;
        }
    }
    switch (op.stage) {
    case STEP_ST_ENC_KM_FWD: return svgp_mnist_encoder_kernel_matrix_fwd(c, a.theta, a.images, a.aux, a.ws, st);
    case STEP_ST_STATS_FWD: return svgp_gp_stats_fwd(c, a.ws, st);
    case STEP_ST_TIT_STATS: return svgp_gp_titsias_stats(c, a.ws, st);
    case STEP_ST_FACTOR_FWD_PIECES: return svgp_gp_factor_fwd_pieces(c, a.ws, st, op.arg);
    case STEP_ST_FACTOR_FWD_DEFER_AJI: return svgp_gp_factor_fwd_defer_aji(c, a.ws, st);
    case STEP_ST_FACTOR_FWD_AJI_TAIL: return svgp_gp_factor_fwd_aji_tail(c, a.ws, st);
    case STEP_ST_BIG_FACTOR_FWD: return svgp_big_factor_fwd(c, *a.wl, a.ws, st, a.l0, a.nl, op.arg);
    case STEP_ST_POST_FWD: return svgp_gp_posterior_fwd(c, a.eps, a.ws, a.state, st);
    case STEP_ST_POST_FWD_AJI: return svgp_gp_posterior_fwd_with_aji(c, a.eps, a.ws, a.state, st);
    case STEP_ST_TIT_FWD: return svgp_gp_titsias_fwd(c, a.ws, a.state, st);
    case STEP_ST_DEC_FUSED_AJI: return svgp_mnist_decoder_fwd_bwd_data_pre_aji(c, a.theta, a.images, a.ws, a.state, st);
    case STEP_ST_DEC_FUSED: return svgp_mnist_decoder_fwd_bwd_data_pre(c, a.theta, a.images, a.ws, a.state, st);
    case STEP_ST_DEC_FWD_PRE: return svgp_mnist_decoder_fwd_pre(c, a.theta, a.images, a.ws, st);
    case STEP_ST_DEC_BWD_DATA_PRE_AJI: return svgp_mnist_decoder_bwd_data_pre_aji(c, a.theta, a.images, a.ws, a.state, st);
    case STEP_ST_DEC_BWD_DATA_PRE: return svgp_mnist_decoder_bwd_data_pre(c, a.theta, a.images, a.ws, a.state, st);
    case STEP_ST_DEC_FWD: return svgp_mnist_decoder_fwd(c, a.theta, a.images, a.ws, st);
    case STEP_ST_DEC_BWD: return svgp_mnist_decoder_bwd(c, a.theta, a.images, a.ws, a.state, st);
    case STEP_ST_STATS_BWD: return svgp_gp_stats_bwd(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_EARLY: return svgp_gp_factor_bwd_early(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_LATE_A: return svgp_gp_factor_bwd_late_a(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_LATE_B: return svgp_gp_factor_bwd_late_b(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_LATE_B_KBAR: return svgp_gp_factor_bwd_late_b_kbar(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_LATE_B_CHANNELS: return svgp_gp_factor_bwd_late_b_channels(c, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_LATE_B_FINAL: return svgp_gp_factor_bwd_late_b_final(c, a.ws, a.state, st);
    case STEP_ST_BIG_FACTOR_BWD: return svgp_big_factor_bwd(c, *a.wl, a.ws, a.state, st, a.l0, a.nl, op.arg);
    case STEP_ST_STATS_FACTOR_BWD_WGRAD: return svgp_gp_stats_factor_bwd_wgrad_sched(c, a.images, a.ws, a.state, st, sc);
    case STEP_ST_FACTOR_BWD_NOFINAL_WGRAD: return svgp_gp_factor_bwd_nofinal_wgrad(c, a.images, a.ws, a.state, st);
    case STEP_ST_FACTOR_BWD_NOFINAL: return svgp_gp_factor_bwd_nofinal(c, a.ws, a.state, st);
    case STEP_ST_POST_BWD_ROWS: return svgp_gp_posterior_bwd_rows(c, a.ws, a.state, st);
    case STEP_ST_POST_BWD_FINAL: return svgp_gp_posterior_bwd_with_final(c, a.ws, a.state, st);
    case STEP_ST_POST_BWD: return svgp_gp_posterior_bwd(c, a.ws, a.state, st);
    case STEP_ST_TIT_BWD: return svgp_gp_titsias_bwd(c, a.ws, a.state, st);
    case STEP_ST_KM_BWD_PARTIALS: return svgp_kernel_matrix_bwd_partials(c, a.theta, a.aux, a.ws, st);
    case STEP_ST_ENC_BWD: return svgp_mnist_encoder_bwd(c, a.theta, a.images, a.ws, st);
    case STEP_ST_ENC_BWD_KM: return svgp_mnist_encoder_bwd_km(c, a.theta, a.images, a.aux, a.ws, st);
    case STEP_ST_ENC_BWD_KM_SUM: return svgp_mnist_encoder_bwd_km_sum(c, a.theta, a.images, a.aux, a.ws, a.state, st);
    case STEP_ST_GRAD_REDUCE_ALL: return svgp_mnist_grad_reduce_all(c, a.aux, a.ws, st);
    case STEP_ST_GRAD_REDUCE_PART: return svgp_mnist_grad_reduce_part(c, a.aux, a.ws, (int)op.arg, st);
    case STEP_ST_ADAM_FINALIZE: {
        svgp_mnist_param_layout pl;
        svgp_mnist_ws_layout wl;
        int rc = svgp_mnist_param_layout_get(c, &pl);
        if (rc) return rc;
        rc = svgp_mnist_ws_layout_get(c, &wl);
        if (rc) return rc;
        SVGP_REQUIRE(a.adam_v != nullptr, SVGP_ERR_INVALID, "adam_v is NULL");
        return svgp_adam_tf1_finalize(c, pl.n_total, a.theta, a.ws + wl.grad, a.adam_m, a.adam_v, a.ws, a.state, 0.9, 0.999, 1e-8, st);
    }
    case STEP_ST_FINALIZE_NOADAM: return svgp_elbo_finalize_noadam(c, a.ws, a.state, st);
    }
    svgp_set_error("step plan: unknown stage %d", (int)op.stage);
    return SVGP_ERR_INVALID;
}

// sd: the Side of `stream` if the caller has looked it up already
int step_run(const StepPlan& P, const StepArgs& a, void* stream, const SvgpSched& sc, Side* sd) {
    SVGP_REQUIRE(a.theta && a.images && a.aux && a.ws && a.state, SVGP_ERR_INVALID, "NULL device pointer");
    hipStream_t lane[3] = {(hipStream_t)stream, (hipStream_t)stream, (hipStream_t)stream};
    if (P.side) {
        if (!sd) {
            int rc = side_get(lane[STEP_MAIN], sc, &sd);
            if (rc) return rc;
        }
        lane[STEP_SIDE0] = sd->s[0]; lane[STEP_SIDE1] = sd->s[1];
    }
    bool group = false, forked[2] = {false, false};
    int rc = SVGP_OK, point = -1;
    for (int i = 0; i < P.n && rc == SVGP_OK; ++i) {
        const StepOp& op = P.op[i];
        const int k = op.lane == STEP_SIDE1 ? 1 : 0;
        switch (op.kind) {
        case STEP_STAGE: rc = step_stage(op, a, (void*)lane[op.lane], sc, P.fwd_split); break;
        case STEP_FORK: rc = side_fork(sd, k, lane[STEP_MAIN]); forked[k] = forked[k] || rc == SVGP_OK; break;
        case STEP_JOIN: rc = side_join(sd, k, lane[STEP_MAIN]); forked[k] = false; break;
        case STEP_GROUP_BEGIN: rc = svgp_comm_group_begin(a.comm); group = rc == SVGP_OK; break;
        case STEP_GROUP_END: group = false; rc = svgp_comm_group_end(a.comm); break;
        default: rc = svgp_step_exchange(op, a, (void*)lane[op.lane], &point); break;
        }
    }
    if (rc != SVGP_OK) {            // (an open group defers every later RCCL call of the thread; an unjoined branch under capture is an unjoined capture)
        if (group) (void)svgp_comm_group_end(a.comm);
        for (int k = 0; k < 2; ++k)
            if (forked[k]) (void)side_join(sd, k, lane[STEP_MAIN]);
    }
    return rc;
}
}  // namespace

int svgp_step_run(const StepPlan& P, const StepArgs& a, void* stream, const SvgpSched& sc) { return step_run(P, a, stream, sc, nullptr); }

extern "C" int svgp_mnist_step_phase(const svgp_mnist_cfg* c, int phase, double* theta, const double* images,
                                     const double* aux, const double* eps, double* ws, double* state,
                                     double* adam_m, double* adam_v, void* stream) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && images && aux && ws && state, SVGP_ERR_INVALID, "NULL device pointer");
    const SvgpSched sc = sched_read();
    // The late reverse half alone is valid only if phase 1 of this library issued the early half on this workspace (recorded per
    // workspace, not inferred from the environment).
    Side* sd = nullptr;
    bool early_issued = false;
    if (c->m > SVGP_M_MAX && (phase == 1 || phase == 2 || phase == 4)) {
        rc = side_get((hipStream_t)stream, sc, &sd);
        if (rc) return rc;
        if (phase != 1) early_issued = side_take_early(sd, ws);
    }
    StepPlan P;
    rc = svgp_step_plan_checked(c, STEP_FORM_PHASE, phase, 1, 0, adam_m != nullptr, early_issued, sc, P);
    if (rc) return rc;
    rc = step_run(P, StepArgs{c, theta, images, aux, eps, ws, state, adam_m, adam_v}, stream, sc, sd);
    if (rc == SVGP_OK && phase == 1 && P.early) side_mark_early(sd, ws);       // phase 2 of THIS workspace may run the late half only
    return rc;
}

extern "C" int svgp_mnist_train_step(const svgp_mnist_cfg* c, double* theta, const double* images,
                                     const double* aux, const double* eps, double* ws, double* state,
                                     double* adam_m, double* adam_v, void* stream) {
    SVGP_REQUIRE(c && c->b == c->b_global, SVGP_ERR_INVALID,
                 "svgp_mnist_train_step is the single-GPU form (b == b_global); use svgp_mnist_step_phase "
                 "with all-reduces between phases for data parallelism");
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    const SvgpSched sc = sched_read();
    StepPlan P;
    rc = svgp_step_plan_checked(c, STEP_FORM_STEP, 0, 1, 0, adam_m != nullptr, false, sc, P);
    if (rc) return rc;
    return svgp_step_run(P, StepArgs{c, theta, images, aux, eps, ws, state, adam_m, adam_v}, stream, sc);
}

// The plan of a call as text, one op per line (the format: include/svgpvae_hip.h): no GPU call, needs no device.
static const char* const STEP_STAGE_NAME[STEP_ST_COUNT] = {
#define X(id, fn) #fn,
    SVGP_STEP_STAGES(X)
#undef X
};
static const char* const STEP_BLOCK_NAME[STEP_BLK_COUNT] = {
#define X(id) #id,
    SVGP_STEP_BLOCKS(X)
#undef X
};
static const char* step_piece_name(bool fwd, unsigned p) {
    static const struct { bool fwd; unsigned pieces; const char* name; } T[] = {
        {true, SVGP_FWD_K, "K"}, {true, SVGP_FWD_SIG, "SIG"}, {true, SVGP_FWD_KL, "KL"}, {true, SVGP_FWD_TAIL, "TAIL"},
        {true, SVGP_FWD_HEAD, "HEAD"}, {true, SVGP_FWD_ALL, "ALL"},
        {false, SVGP_BWD_EARLY, "EARLY"}, {false, SVGP_BWD_LATE_A, "LATE_A"}, {false, SVGP_BWD_CHANNELS, "CHANNELS"},
        {false, SVGP_BWD_KBAR, "KBAR"}, {false, SVGP_BWD_FINAL, "FINAL"}, {false, SVGP_BWD_LATE, "LATE"}, {false, SVGP_BWD_ALL, "ALL"}};
    for (const auto& t : T)
        if (t.fwd == fwd && t.pieces == p) return t.name;
    return "?";
}
// The entry a slot runs when the plan has fwd_split (step_stage), or nullptr: the one table both the executor's switch and the forms
// printer are checked against (tests/test_fwd_split_route_cpu.py compares the printed names with the stage-by-stage GPU test's calls).
static const char* step_split_form(unsigned char stage) {
    switch (stage) {
    case STEP_ST_FACTOR_FWD_DEFER_AJI: return "svgp_gp_factor_fwd_head";
    case STEP_ST_POST_FWD: return "svgp_gp_posterior_fwd_z";
    case STEP_ST_DEC_FUSED_AJI: return "svgp_mnist_decoder_fwd_bwd_data_pre_tail";
    case STEP_ST_POST_BWD_ROWS: return "svgp_gp_posterior_bwd_rows_d";
    case STEP_ST_POST_BWD_FINAL: return "svgp_gp_posterior_bwd_with_final_d";
    default: return nullptr;
    }
}
static int step_route_text(const svgp_mnist_cfg* c, int form, int phase, int nranks, int rank, int adam, int early_issued,
                           char* buf, int cap, bool forms) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    StepPlan P;
    rc = svgp_step_plan_checked(c, form, phase, nranks, rank, adam != 0, early_issued != 0, sched_read(), P);
    if (rc) return rc;
    static const char* const LANE[] = {"main", "side0", "side1"};
    static const char* const PART[] = {"all", "window", "others", "packed"};
    static const char* const KIND[] = {"", "fork", "join", "allreduce", "point_begin", "point_end", "pack", "unpack", "group_begin",
                                       "group_end", "reduce_scatter", "allgather"};
    int pos = 0;
    buf[0] = 0;
    for (int i = 0; i < P.n; ++i) {
        const StepOp& op = P.op[i];
        const char* ln = LANE[op.lane];
        const char* kd = KIND[op.kind];
        const char* blk = op.arg < STEP_BLK_COUNT ? STEP_BLOCK_NAME[op.arg] : "?";
        switch (op.kind) {
        case STEP_STAGE: {
            const bool fwd = op.stage == STEP_ST_FACTOR_FWD_PIECES || op.stage == STEP_ST_BIG_FACTOR_FWD;
            pos += snprintf(buf + pos, cap - pos, "%s %s", ln, STEP_STAGE_NAME[op.stage]);
            if (pos < cap && (fwd || op.stage == STEP_ST_BIG_FACTOR_BWD)) pos += snprintf(buf + pos, cap - pos, " %s", step_piece_name(fwd, op.arg));
            else if (pos < cap && op.stage == STEP_ST_GRAD_REDUCE_PART) pos += snprintf(buf + pos, cap - pos, " %u", op.arg);
            if (pos < cap && forms && P.fwd_split && step_split_form(op.stage)) pos += snprintf(buf + pos, cap - pos, " -> %s", step_split_form(op.stage));
            break;
        }
        case STEP_FORK: case STEP_JOIN: pos += snprintf(buf + pos, cap - pos, "%s %s", kd, ln); break;
        case STEP_GROUP_BEGIN: case STEP_GROUP_END: pos += snprintf(buf + pos, cap - pos, "%s %s", ln, kd); break;
        case STEP_POINT_BEGIN: case STEP_POINT_END: pos += snprintf(buf + pos, cap - pos, "%s %s %u", ln, kd, op.arg); break;
        case STEP_PACK: case STEP_UNPACK: pos += snprintf(buf + pos, cap - pos, "%s %s %s %s", ln, kd, blk, PART[op.part]); break;
        default:        // the collectives
            pos += snprintf(buf + pos, cap - pos, op.part == STEP_PART_PACKED ? "%s %s %s packed" : "%s %s %s", ln, kd, blk);
        }
        if (pos < cap) pos += snprintf(buf + pos, cap - pos, "\n");
        SVGP_REQUIRE(pos < cap, SVGP_ERR_INVALID, "route text needs more than %d bytes", cap);
    }
    return SVGP_OK;
}

extern "C" int svgp_mnist_step_route(const svgp_mnist_cfg* c, int form, int phase, int nranks, int rank, int adam, int early_issued,
                                     char* buf, int cap) {
    return step_route_text(c, form, phase, nranks, rank, adam, early_issued, buf, cap, false);
}
extern "C" int svgp_mnist_step_route_forms(const svgp_mnist_cfg* c, int form, int phase, int nranks, int rank, int adam, int early_issued,
                                           char* buf, int cap) {
    return step_route_text(c, form, phase, nranks, rank, adam, early_issued, buf, cap, true);
}

// ---------------------------------------------------------------------------------------------
// runtime helpers
// ---------------------------------------------------------------------------------------------
// Creates the library's side branches of `stream` now (outside any stream capture), with the concurrency probe; and the probe
// itself for callers that own their side streams (sprites.py).
extern "C" int svgp_side_streams_prepare(void* stream) {
    Side* sd = nullptr;
    return side_get((hipStream_t)stream, sched_read(), &sd);
}
extern "C" int svgp_streams_overlap(void* a, void* b, int* out) {
    SVGP_REQUIRE(out, SVGP_ERR_INVALID, "out is NULL");
    bool ok = false;
    int rc = streams_overlap((hipStream_t)a, (hipStream_t)b, &ok);
    *out = ok ? 1 : 0;
    return rc;
}
extern "C" int svgp_stream_create(void** out) {
    SVGP_REQUIRE(out, SVGP_ERR_INVALID, "out is NULL");
    hipStream_t s;
    SVGP_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = (void*)s;
    return SVGP_OK;
}
extern "C" int svgp_stream_destroy(void* s) { SVGP_CHECK_HIP(hipStreamDestroy((hipStream_t)s)); return SVGP_OK; }
extern "C" int svgp_stream_sync(void* s) { SVGP_CHECK_HIP(hipStreamSynchronize((hipStream_t)s)); return SVGP_OK; }

extern "C" int svgp_graph_begin(void* s) {
    SVGP_CHECK_HIP(hipStreamBeginCapture((hipStream_t)s, hipStreamCaptureModeThreadLocal));
    return SVGP_OK;
}
extern "C" int svgp_graph_end(void* s, void** exec_out) {
    SVGP_REQUIRE(exec_out, SVGP_ERR_INVALID, "exec_out is NULL");
    hipGraph_t g = nullptr;
    SVGP_CHECK_HIP(hipStreamEndCapture((hipStream_t)s, &g));
    hipGraphExec_t e = nullptr;
    hipError_t err = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    SVGP_CHECK_HIP(err);
    *exec_out = (void*)e;
    return SVGP_OK;
}
extern "C" int svgp_graph_launch(void* e, void* s) {
    SVGP_CHECK_HIP(hipGraphLaunch((hipGraphExec_t)e, (hipStream_t)s));
    return SVGP_OK;
}
extern "C" int svgp_graph_destroy(void* e) { SVGP_CHECK_HIP(hipGraphExecDestroy((hipGraphExec_t)e)); return SVGP_OK; }

extern "C" int svgp_event_create(void** out) {
    SVGP_REQUIRE(out, SVGP_ERR_INVALID, "out is NULL");
    hipEvent_t ev;
    SVGP_CHECK_HIP(hipEventCreate(&ev));
    *out = (void*)ev;
    return SVGP_OK;
}
extern "C" int svgp_event_record(void* ev, void* s) {
    SVGP_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)s));
    return SVGP_OK;
}
extern "C" int svgp_event_elapsed_ms(void* a, void* b, float* ms) {
    SVGP_REQUIRE(ms, SVGP_ERR_INVALID, "ms is NULL");
    SVGP_CHECK_HIP(hipEventSynchronize((hipEvent_t)b));
    SVGP_CHECK_HIP(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
    return SVGP_OK;
}
extern "C" int svgp_event_destroy(void* ev) { SVGP_CHECK_HIP(hipEventDestroy((hipEvent_t)ev)); return SVGP_OK; }
