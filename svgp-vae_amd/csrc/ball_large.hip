// Moving-ball SVGP-VAE beyond the LDS-resident stages: more than 64 inducing points or more than 64 videos in the batch
// (BALL_experiment.py --elbo SVGPVAE_Hensman | SVGPVAE_Titsias; SVGPVAE_model.py:17-171, 638-715).
//
// Same mapping as the m <= 64 path (ball.hip header): the tmax frames of a video are the rows, the videos of the batch the
// channels, N_train = b = tmax (c = 1), kl_form = 1, clip_pv = 2, one workspace per latent coordinate.  Here the GP block runs on
// the large-m stages of gp_large.hip at EVERY m (also m <= 64: the hand-over point is the engine's, ball.sparse_engine_class),
// with the moving-ball KL form those stages carry for this engine, and the channel count is not capped at 64: all videos of the
// batch are channels of ONE workspace, so the batch-wide scalar of the reference's KL, the 1/B of the loss seed and the Philox
// counters are those of the whole batch by construction.  The Titsias ELBO runs on the global-memory stages of gp_titsias.hip.
//
// svgp_check_cfg (api.hip) keeps refusing kl_form = 1 above m = 64 and more than 64 channels for every other entry point; the
// checks of this family are ball_check below.  One forward call per coordinate:
//   kernel matrices -> statistics -> (Titsias statistics) -> factor stage -> row stage -> (Titsias terms)
// and one reverse call, the mirror image down to d_ip, d_ls and ws.ybar / ws.s2bar.  Explicit stream, no allocation, no host
// synchronisation; refusals come before any launch.
#include "common.hpp"

extern "C" int svgp_se1d_kernel_matrix_fwd(int T, int m, const double* x, const double* z, const double* ls, double* K,
                                           double* Kn, double* knn, void* stream);
extern "C" int svgp_se1d_kernel_matrix_bwd(int T, int m, const double* x, const double* z, const double* ls,
                                           const double* Kbar, const double* Knbar, double* d_z, double* d_ls, void* stream);

namespace {

#define BALL_LARGE_MAX_T 16384      // int indices of the (tmax, videos) and (tmax, m) element kernels

int ball_check(const svgp_ball_large_cfg* q, svgp_mnist_cfg* c) {
    SVGP_REQUIRE(q != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(q->m >= 1 && q->B >= 1 && q->T >= 1, SVGP_ERR_INVALID, "bad shape T=%d B=%d m=%d", q->T, q->B, q->m);
    SVGP_REQUIRE(q->m <= SVGP_M_LIMIT, SVGP_ERR_UNSUPPORTED, "m=%d inducing points: the moving-ball large engine takes 1 <= m <= %d",
                 q->m, SVGP_M_LIMIT);
    SVGP_REQUIRE(q->B <= SVGP_BALL_LARGE_MAX_VIDEOS, SVGP_ERR_UNSUPPORTED,
                 "B=%d videos: the moving-ball large engine takes 1 <= B <= %d videos per batch", q->B, SVGP_BALL_LARGE_MAX_VIDEOS);
    SVGP_REQUIRE(q->T <= BALL_LARGE_MAX_T, SVGP_ERR_UNSUPPORTED, "T=%d frames: the moving-ball large engine takes 1 <= T <= %d", q->T,
                 BALL_LARGE_MAX_T);
    SVGP_REQUIRE(q->kl_form == 1, SVGP_ERR_INVALID, "kl_form=%d: the moving-ball engine computes the KL of SVGPVAE_model.py:128-137 (kl_form=1)",
                 q->kl_form);
    SVGP_REQUIRE(q->clip_pv == 2, SVGP_ERR_INVALID, "clip_pv=%d: the moving-ball sample clips inside the square root only (clip_pv=2)",
                 q->clip_pv);
    SVGP_REQUIRE(q->titsias == 0 || q->titsias == 1, SVGP_ERR_INVALID, "titsias=%d (0 or 1)", q->titsias);
    SVGP_REQUIRE(q->jitter >= 0, SVGP_ERR_INVALID, "bad jitter");
    // the stage configuration: every row of the batch local (b == b_global: the ball KL couples all videos and is never sharded)
    memset(c, 0, sizeof(*c));
    c->b = c->b_global = c->b_cap = q->T; c->m = q->m; c->L = q->B; c->M = 1;
    c->train_ip = c->train_gp = 1; c->clip_pv = 2; c->titsias = q->titsias; c->kl_form = 1;
    c->single_stat_block = 1;             // one statistics block per channel whatever m is (the large-m stages write one)
    c->N_train = (double)q->T; c->jitter = q->jitter; c->rep_weight = 1.0;
    return SVGP_OK;
}

}  // namespace

#define RUNC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)
#define REQ_PTRS(...)                                                                            \
    do {                                                                                         \
        const void* ps_[] = {__VA_ARGS__};                                                        \
        for (const void* q_ : ps_) SVGP_REQUIRE(q_ != nullptr, SVGP_ERR_INVALID, "NULL device pointer"); \
    } while (0)

extern "C" int svgp_ball_large_ws_layout_get(const svgp_ball_large_cfg* q, svgp_mnist_ws_layout* out) {
    svgp_mnist_cfg c;
    RUNC(ball_check(q, &c));
    SVGP_REQUIRE(out != nullptr, SVGP_ERR_INVALID, "out is NULL");
    return svgp_ws_layout_fill(&c, out, true);
}

extern "C" long long svgp_ball_large_workspace_elems(const svgp_ball_large_cfg* q) {
    svgp_mnist_ws_layout wl;
    return svgp_ball_large_ws_layout_get(q, &wl) == SVGP_OK ? (long long)wl.total : 0;
}

extern "C" int svgp_ball_large_gp_fwd(const svgp_ball_large_cfg* q, const double* times, const double* ip, const double* ls,
                                      const double* eps, double* ws, double* state, void* stream) {
    svgp_mnist_cfg c;
    RUNC(ball_check(q, &c));
    REQ_PTRS(times, ip, ls, ws, state);
    svgp_mnist_ws_layout wl;
    RUNC(svgp_ws_layout_fill(&c, &wl, true));
    RUNC(svgp_se1d_kernel_matrix_fwd(c.b, c.m, times, ip, ls, ws + wl.K, ws + wl.Kn, ws + wl.knn, stream));
    RUNC(svgp_big_stats(&c, wl, ws, nullptr, 0, stream));
    if (c.titsias) RUNC(svgp_titsias_stats_wl(&c, wl, ws, stream));
    RUNC(svgp_big_factor_fwd(&c, wl, ws, stream, 0, c.L, SVGP_FWD_ALL));
    RUNC(svgp_big_posterior_fwd(&c, wl, eps, ws, state, stream));
    if (c.titsias) RUNC(svgp_titsias_fwd_wl(&c, wl, ws, state, stream));
    return SVGP_OK;
}

extern "C" int svgp_ball_large_gp_bwd(const svgp_ball_large_cfg* q, const double* times, const double* ip, const double* ls,
                                      double* ws, const double* state, double* d_ip, double* d_ls, void* stream) {
    svgp_mnist_cfg c;
    RUNC(ball_check(q, &c));
    REQ_PTRS(times, ip, ls, ws, state, d_ip, d_ls);
    svgp_mnist_ws_layout wl;
    RUNC(svgp_ws_layout_fill(&c, &wl, true));
    RUNC(svgp_big_stats(&c, wl, ws, state, 1, stream));
    RUNC(svgp_big_factor_bwd(&c, wl, ws, state, stream, 0, c.L, SVGP_BWD_ALL));
    RUNC(svgp_big_posterior_bwd(&c, wl, ws, state, stream));
    if (c.titsias) RUNC(svgp_titsias_bwd_wl(&c, wl, ws, state, stream));
    return svgp_se1d_kernel_matrix_bwd(c.b, c.m, times, ip, ls, ws + wl.Kbar, ws + wl.Knbar, d_ip, d_ls, stream);
}

extern "C" int svgp_ball_large_elbo_assemble(const svgp_ball_large_cfg* q, const double* ws_x, const double* ws_y,
                                             const double* row_recon, const double* state, double* out, void* stream) {
    svgp_mnist_cfg c;
    RUNC(ball_check(q, &c));
    svgp_mnist_ws_layout wl;
    RUNC(svgp_ws_layout_fill(&c, &wl, true));
    return svgp_ball_assemble_wl(&c, wl, ws_x, ws_y, row_recon, state, out, stream);
}
