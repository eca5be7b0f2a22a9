/*
 * svgpvae_hip.h - C ABI of libsvgpvae_hip.so, the MI355X (gfx950) implementation of the
 * SVGPVAE_Hensman / SVGPVAE_Titsias training step of ratschlab/SVGP-VAE (rotated-MNIST path), of the
 * building blocks of its SPRITES path, and of the N-sized float32 statistics pass of its test pipeline.
 *
 * The reference has no native/FFI layer (it is TensorFlow-1.15 graph code), so each entry point
 * below cites the reference Python it replaces (file:line into the reference checkout) instead of
 * a reference FFI declaration.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = svgp_status; svgp_last_error() gives a
 *     thread-local message.  No C++ exception crosses the boundary.
 *   - all tensor pointers are CALLER-OWNED DEVICE pointers (row-major, contiguous; float64 everywhere
 *     except the svgp_stream_*_f32 entry points); nothing is retained after return.  Scratch lives in the caller-provided workspace whose
 *     layout svgp_mnist_ws_layout() describes (offsets in float64 elements).
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it,
 *     no hidden synchronisation, no allocation -> every call is hipGraph-capturable.
 *   - per-step scalars (GECO state, Adam step, lr, beta, alpha) live in a small DEVICE state
 *     vector (svgp_state_slot) so that a captured graph can be replayed unchanged.
 *   - re-entrant, usable from several threads on different streams.  Process-wide state is limited to
 *     what is created once and then only read -- the dlopen'd RCCL entry points (svgp_comm_*) -- and one pair of
 *     library-owned side streams + events per (device, caller stream), created at the first m > 64 step (or with
 *     SVGP_SIDE_STREAMS=1) on that stream and used only by calls that pass that stream.
 *   - the SVGP_* environment variables named below are schedule switches: same bits, another launch order.  They are read
 *     once per call of an exported entry point; DESIGN.md section 6.4 lists all of them with values and defaults.
 */
#ifndef SVGPVAE_HIP_H
#define SVGPVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVGP_VERSION_MAJOR 0
#define SVGP_VERSION_MINOR 1

typedef enum {
    SVGP_OK = 0,
    SVGP_ERR_INVALID = -1,     /* bad argument / null pointer / inconsistent shapes            */
    SVGP_ERR_UNSUPPORTED = -2, /* shape outside what this build implements (e.g. m > 2048)     */
    SVGP_ERR_HIP = -3,         /* a HIP runtime call failed (message has hipGetErrorString)    */
    SVGP_ERR_COMM = -4         /* an RCCL call failed (message has ncclGetErrorString)         */
} svgp_status;

/* Shapes + constants of one rank's share of a rotated-MNIST SVGPVAE step.
 * Mirrors the constructor arguments of mnistSVGP (SVGPVAE_model.py:383-384), mnistVAE
 * (VAE_utils.py:103) and the flags consumed by forward_pass_SVGPVAE (SVGPVAE_model.py:823-825). */
typedef struct {
    int32_t b;             /* rows of THIS rank's batch                                         */
    int32_t b_global;      /* rows of the global batch (= b on one GPU); N_train/b_global is c  */
    int32_t m;             /* number of inducing points (rows of inducing_index_points)         */
    int32_t L;             /* latent channels (mnistVAE L)                                      */
    int32_t M;             /* GPLVM / object-vector dimension (--M)                             */
    int32_t n_obj;         /* rows of the object_vectors table; 0 = no table (aux cols 2: used) */
    int32_t normalize_obj; /* K_obj_normalize (SVGPVAE_model.py:465-474)                        */
    int32_t clip_qs;       /* clipping_qs: clip qnet_var to [1e-3, 10] (SVGPVAE_model.py:858)   */
    int32_t geco;          /* GECO objective (SVGPVAE_model.py:908-915) else beta-ELBO (:917)   */
    int32_t train_ip;      /* 1: inducing points trainable (--ip_joint)                         */
    int32_t train_gp;      /* 1: l_GP, amplitude trainable (--GP_joint)                         */
    int32_t train_ov;      /* 1: object_vectors trainable (--ov_joint)                          */
    int32_t b_cap;         /* row capacity the workspace LAYOUT is computed for (0 = b); keeps    */
                           /* offsets fixed across ragged batches / train-vs-test row counts      */
    int32_t clip_pv;       /* 1: clip the posterior variance p_v to [1e-4, 100] (SPRITES,          */
                           /* SVGPVAE_model.py:891-892); the clip mask enters the reverse pass.    */
                           /* 2: moving ball (:693): only the sampling step uses clip(p_v, 1e-4,   */
                           /* 1000); p_v itself and the cross-entropy keep the raw value           */
    int32_t n_pix;         /* pixels per image in the reconstruction loss (0 = 784 = MNIST)        */
    int32_t titsias;       /* 1: mainSVGP(titsias=True): inside-ELBO = sum_l L_2 (SVGPVAE_model.py:246-259,  */
                           /* 882-883) instead of the Hensman L_3 / KL pair                          */
    int32_t kl_form;       /* 0: Hensman KL of mainSVGP (:270-279).  1: KL of the moving-ball SVGP (:128-137), which  */
                           /* has A_hat where mu_hat is meant and reduces over the whole batch of videos (= the L      */
                           /* channels here): KL_l = 1/2 [.. + L tr(K_mm^-1 A_l A_l)], same sum over l as the          */
                           /* reference; the KL field is then [KL (L) | tr(K_mm^-1 A_l A_l) (L)]                       */
    int32_t single_stat_block; /* m <= 64: 1 = the statistics launches write ONE block per channel instead of 4 row      */
                           /* partials (optional under data parallelism: by default the partial blocks are exchanged  */
                           /* as one message).  m > 64: 1 = the batch is sharded over ranks: the workspace carries    */
                           /* the wire buffer of the packed exchange (xpack)                                          */
    int32_t gemm_f32;      /* large-m path (m > 64) only.  1: every product of the GP block runs on the float32 MFMA  */
                           /* (svgp_dgemm_f32c_batched: float64 storage, float32 products and sums) -- the arithmetic */
                           /* of the reference's float32 SPRITES graph (SVGPVAE_model.py:516); 2: only the statistics */
                           /* S_l = K_mn diag(w) K_nm (sums of non-negative terms for the forward weights) do.  The   */
                           /* m x m factorisations / inverses stay float64 in every mode               */
    int32_t split_grad_exchange; /* data parallelism, row-sharded schedule: 1 = the closing gradient all-reduce in TWO parts   */
                           /* -- decoder + GP parameters + scalar sums as soon as the kernel-matrix reverse pass is done (they   */
                           /* do not depend on the encoder's reverse pass; svgp_mnist_train_step_dp issues it on a side        */
                           /* stream), the encoder's part behind its reverse pass -- so that one of the three small-message    */
                           /* latencies hides under the encoder's reverse pass.  0 (default): one all-reduce.  Any other value */
                           /* is refused (svgp_check_cfg): an uninitialised field must not switch only some ranks to the two  */
                           /* messages (mismatched collectives hang).  (The field sits in the padding in front of N_train:     */
                           /* the struct's size and every other offset are unchanged.)                                         */
    double  N_train;       /* mainSVGP.N_train                                                  */
    double  jitter;        /* mainSVGP.jitter                                                   */
    double  kappa_squared; /* GECO kappa^2                                                      */
    double  alpha;         /* GECO moving-average alpha used from the 2nd step on               */
    double  rep_weight;    /* weight of rank-replicated gradient terms: 1 on rank 0, else 0     */
} svgp_mnist_cfg;

/* Flat parameter vector theta (float64).  Offsets in elements.  Order = the reference's
 * trainable-variable creation order: VAE encoder, decoder (VAE_utils.py:114-141), inducing points
 * (SVGPVAE_model.py:203), l_GP, amplitude (:412-413), object_vectors (:421).  TF layouts:
 * conv kernels (kh,kw,cin,cout), dense (in,out), NHWC flatten.                                  */
typedef struct {
    int64_t enc_c1_w, enc_c1_b, enc_c2_w, enc_c2_b, enc_c3_w, enc_c3_b, enc_d_w, enc_d_b;
    int64_t dec_d_w, dec_d_b, dec_c1_w, dec_c1_b, dec_c2_w, dec_c2_b, dec_c3_w, dec_c3_b;
    int64_t ip, l_GP, amplitude, ov;
    int64_t n_enc;   /* number of encoder parameters (prefix of theta)       */
    int64_t n_vae;   /* encoder + decoder                                     */
    int64_t n_total; /* everything                                            */
} svgp_mnist_param_layout;

/* Workspace (float64) offsets of every intermediate of the step.  All are inspectable for tests. */
typedef struct {
    /* encoder (VAE_utils.py:114-126,143-152) */
    int64_t enc_a1, enc_a2, enc_a3;       /* post-ELU activations (b,13,13,8) (b,6,6,8) (b,32)    */
    int64_t qnet_mu, qnet_var_raw, qnet_var; /* (b,L) each; var = clip(exp(.))                    */
    /* kernel matrices (SVGPVAE_model.py:427-476) */
    int64_t K, Kn, knn;                   /* (m,m) (b,m) (b); m > 64: W = Kn Ki K (b,m) behind the b rows of Kn */
    /* forward statistics: ONE contiguous all-reduce block [S | v] (titsias: [S | v | tit_S2 | tit_v2]).
     * S (P,L,m,m), v (P,L,m) with P = stat_parts ROW PARTIALS (the LDS-resident path splits the rows of every channel
     * over P workgroups; the statistics are the sums over p, taken by the consumers on load; 1 for m > 64 and
     * with cfg.single_stat_block, which the engines set when the blocks travel through an all-reduce).  The
     * backward block [A2 | ud | td] has the same partial structure.  Sums over ranks commute with the sum over p. */
    int64_t statA, statA_len, S, v, stat_parts;
    /* m x m factor stage (SVGPVAE_model.py:239,270-279,319-341) */
    int64_t Ki, ldK, Si, t, G, A, Aji, mu_hat, u, M2, KL, q; /* M2 = Ki A Ki (L,m,m; m <= 64 only); q (b) */
    /* per-sample stage (:264-299,332-337, 888-902; utils.py:498-504) */
    int64_t p_m, p_v, e, d, eps, z;       /* (b,L) each                                           */
    /* decoder (VAE_utils.py:128-141,154-162) */
    int64_t dec_h0, dec_a1, dec_a2, recon; /* (b,128) (b,8,8,8) (b,14,14,8) (b,28,28,1)           */
    /* pre-activation gradients of the decoder layers, written by svgp_mnist_decoder_bwd_data for the weight half */
    int64_t dec_d2, dec_d1, dec_dh0;      /* (b,14,14,8) (b,8,8,8) (b,128)                        */
    int64_t flags;                        /* (64) u64 counters of the intra-launch hand-offs: [0..2] svgp_mnist_encoder_bwd_km_sum (produced,
                                           * consumed, sticky error), [8, 8+L) svgp_gp_stats_factor_bwd_wgrad (one per channel); the
                                           * workspace must be ZERO here before its first use (every call leaves them zero) */
    int64_t dec_weff;                     /* (2176) effective parity-class weights of the decoder's three up-convolutions for the
                                           * current theta: written by svgp_mnist_encoder_kernel_matrix_fwd, read by the `_pre` forms */
    /* backward */
    int64_t zbar, g_pv, g_pm, mvbar;      /* (b,L) each                                           */
    int64_t statB, statB_len, A2, ud, td; /* ONE contiguous all-reduce block [A2 | ud | td]       */
    int64_t Kbar, fb_part, Qm, vbar, Ssym; /* (m,m) (2,L,m,m) scratch (L,m,m) (L,m) (L,m,m)        */
    int64_t Knbar_part;                   /* (L,b,m) per-channel row gradients before the sum     */
    int64_t scr_bm, scr_mm, scr_vec, scr_inv, scr_bl; /* scratch of the large-m (m > 64) path; scr_bm also holds the
                                           * forward products [Kn; W] Si_l, Kn Ki that the reverse pass re-reads */
    int64_t scr_sm;                       /* m > 64: 10 channel-independent (m,m) matrices (K Ki, Kn^T Wbar, ..) */
    int64_t Knbar, knnbar, ybar, s2bar;   /* (b,m) (b) (b,L) (b,L)                                */
    int64_t d_on;                         /* (b,M) gradient of gathered object rows               */
    /* partial sums */
    int64_t part_dec, part_enc, n_part;   /* (n_part, n_dec) / (n_part, n_enc) weight-grad partials */
    int64_t part_gp;                      /* (m + n_postblk, 2) amplitude / length-scale partials */
    int64_t part_sums, n_post;            /* (n_part,4) [.,.,recon sq,.] then (n_post,2) [L3 data, CE] */
    /* final all-reduce block: [grad (n_total) | sums (8)] */
    int64_t gradC, gradC_len, grad, sums;
    /* Titsias branch (cfg.titsias; zero-sized otherwise): statistics with weights 1/(var + jitter) inside statA,
     * (K + jI + S2)^-1, its product with v2, scalars [logdet (L) | v2.t2 (L) | row sum (1)] */
    int64_t tit_S2, tit_v2, tit_Si, tit_t, tit_scal;
    /* m > 64 with cfg.single_stat_block (batch sharded over ranks): one tile-packed buffer of L symmetric matrices
     * (svgp_sym_pack): what the channel-sharded exchange moves instead of a full (L,m,m) block.
     * xpack_len = L * svgp_sym_packed_elems(m) (0 otherwise).                                                          */
    int64_t xpack, xpack_len;
    int64_t total;                        /* workspace size in float64 elements                   */
} svgp_mnist_ws_layout;

/* Device state vector (float64[SVGP_STATE_LEN]); the host initialises slots 0..5, kernels keep
 * them up to date (MNIST_experiment.py:313-355 host state machine moved on device).            */
typedef enum {
    SVGP_ST_C_MA = 0,        /* GECO moving average C_ma  (init 0.0, MNIST_experiment.py:314)    */
    SVGP_ST_LAGRANGE = 1,    /* GECO lagrange multiplier  (init 1.0, :315)                       */
    SVGP_ST_ALPHA = 2,       /* alpha used by the NEXT step (init 0.0 = first_step, :330-333)    */
    SVGP_ST_ADAM_T = 3,      /* number of Adam updates done so far (global_step)                 */
    SVGP_ST_LR = 4,          /* learning rate                                                    */
    SVGP_ST_BETA = 5,        /* beta of the beta-ELBO                                            */
    SVGP_ST_ELBO = 6,        /* outputs of the last step (the scalar members of the 16-tuple)    */
    SVGP_ST_RECON_LOSS = 7,
    SVGP_ST_KL_TERM = 8,
    SVGP_ST_INSIDE_ELBO = 9,
    SVGP_ST_CE_TERM = 10,
    SVGP_ST_INSIDE_RECON = 11,
    SVGP_ST_INSIDE_KL = 12,
    SVGP_ST_RNG_CTR = 13,    /* counter of the on-device N(0,1) generator (bit pattern of u64)   */
    SVGP_ST_TICKET = 15,     /* u64 workgroup ticket of svgp_adam_tf1_finalize; 0 between launches */
    SVGP_STATE_LEN = 16
} svgp_state_slot;

int         svgp_version(void);
const char* svgp_last_error(void);
/* sizeof() of the ABI structs as compiled into the library, so a binding can verify its own mirror of a struct at load
 * time (a stale mirror shifts every later field silently): which = 0 svgp_mnist_cfg, 1 svgp_mnist_param_layout,
 * 2 svgp_mnist_ws_layout, 3 svgp_stream_kdesc, 4 svgp_conv_desc, 5 svgp_sprites_kcfg, 6 svgp_pearce_bufs,
 * 7 svgp_sum_job, 8 svgp_casale_cfg, 9 svgp_casale_layout, 10 svgp_ball_large_cfg, 11 svgp_mnist_cache_layout,
 * 13 svgp_ball_predict_cfg, 14 svgp_ball_predict_bufs, 15 svgp_pearce_predict_cfg, 16 svgp_pearce_predict_bufs,
 * 18 svgp_casale_cache_layout, 19 svgp_cvae_cfg, 20 svgp_cvae_ws_layout, 22 svgp_ball_predict_joint_cfg,
 * 23 svgp_ball_predict_joint_bufs, 25 svgp_ball_state_cfg, 26 svgp_ball_state_bufs; -1 otherwise (12, 17, 21 and 24 are not
 * assigned). */
int         svgp_struct_sizeof(int which);

int svgp_mnist_param_layout_get(const svgp_mnist_cfg* cfg, svgp_mnist_param_layout* out);
int svgp_mnist_ws_layout_get(const svgp_mnist_cfg* cfg, svgp_mnist_ws_layout* out);

/* ---- stage entry points (each enqueues 1-2 kernels on `stream`) ----------------------------
 * theta: flat parameters; ws: workspace; images (b,28,28,1); aux (b,2+M); state: device state.   */

/* mnistVAE.encode + clip  (VAE_utils.py:143-152, SVGPVAE_model.py:854-859) */
int svgp_mnist_encoder_fwd(const svgp_mnist_cfg*, const double* theta, const double* images,
                           double* ws, void* stream);
/* mnistSVGP.kernel_matrix x3: K_mm, K_nm, diag K_nn (SVGPVAE_model.py:427-476) */
int svgp_kernel_matrix_fwd(const svgp_mnist_cfg*, const double* theta, const double* aux,
                           double* ws, void* stream);
/* mnistSVGP.kernel_matrix(x, y, x_inducing, y_inducing, diag_only) for ARBITRARY row sets (SVGPVAE_model.py:427-476):
 * x (nx, 2+M), y (ny, 2+M), rows [id, angle, o_1..o_M].  x_gather / y_gather != 0: that side's object vector is
 * table[(int)row[0]] (the reference's `not *_inducing` with a GPLVM table, :451,455), else the row's columns 2:.
 * diag_only: out (nx) = k(x_i, y_i), nx == ny (kernel.apply, :458-467); else out (nx, ny) row-major.                 */
int svgp_kernel_matrix_xy(int M, int normalize, int nx, const double* x, int x_gather, int ny, const double* y,
                          int y_gather, const double* table, const double* l_GP, const double* amplitude,
                          int diag_only, double* out, void* stream);
/* S_l = K_mn diag(1/var_l) K_nm, v_l = K_mn (y_l/var_l)  (SVGPVAE_model.py:328-334) and, for m <= 64 in the
 * same launch, K_mm_inv / logdet (:239,270,273) (m > 64: svgp_gp_factor_fwd forms them next to the channel
 * inverses).  Output block statA is what DP all-reduces.                                           */
int svgp_gp_stats_fwd(const svgp_mnist_cfg*, double* ws, void* stream);
/* Sigma_l^-1, mu_hat, A_hat, KL_l (SVGPVAE_model.py:331-341, 270-279) */
int svgp_gp_factor_fwd(const svgp_mnist_cfg*, double* ws, void* stream);
/* posterior mean/var at the batch points, L3 / cross-entropy integrands, z = p_m + eps sqrt(p_v)
 * (SVGPVAE_model.py:264-265,284-299,332-337,895-902).  eps (b,L) may be NULL: then N(0,1) numbers
 * are drawn on device (Philox) as tf.random.normal does at :901.                                  */
int svgp_gp_posterior_fwd(const svgp_mnist_cfg*, const double* eps, double* ws, double* state,
                          void* stream);
/* mnistVAE.decode + squared reconstruction error (VAE_utils.py:154-162, SVGPVAE_model.py:905-918) */
int svgp_mnist_decoder_fwd(const svgp_mnist_cfg*, const double* theta, const double* images,
                           double* ws, void* stream);
/* reverse of the decoder; writes zbar and decoder weight-gradient partials.  One launch up to L = 21; from L = 22 its LDS would
 * exceed a workgroup's 160 KB and it issues svgp_mnist_decoder_bwd_data + _weights (threads 256, n_types 3) instead */
int svgp_mnist_decoder_bwd(const svgp_mnist_cfg*, const double* theta, const double* images,
                           double* ws, const double* state, void* stream);
/* The reverse pass of the decoder in two halves (tf.gradients of VAE_utils.py:128-141,154-162; MNIST_experiment.py:202-205).
 * _data: the chain d recon -> zbar that the GP reverse stages wait for; also stores the pre-activation gradients ws.dec_d2 /
 * dec_d1 / dec_dh0.  _weights: the decoder weight-gradient partials (ws.part_dec) from those and the stored activations; feeds
 * only svgp_mnist_grad_reduce, so it may run anywhere between _data and the reduction -- svgp_gp_factor_bwd_nofinal_wgrad runs
 * it as extra workgroups of the reverse factor launch (m <= 64), which leaves 240 of 256 CUs idle.  threads: 256 or 512 per
 * workgroup (the rider form is 256); n_types: 1, 2 or 3 workgroups per image, each taking a group of layers (the rider form
 * is 3: UpC3 | UpC2 | UpC1 + dense).  _data + _weights == svgp_mnist_decoder_bwd up to summation order. */
int svgp_mnist_decoder_bwd_data(const svgp_mnist_cfg*, const double* theta, const double* images,
                                double* ws, const double* state, void* stream);
int svgp_mnist_decoder_bwd_weights(const svgp_mnist_cfg*, const double* images, double* ws, const double* state,
                                   int threads, int n_types, void* stream);
/* svgp_mnist_decoder_fwd / _bwd_data that LOAD the effective up-convolution weights (UpSampling2D + 3x3 as four parity-specific
 * 2x2 convolutions) from ws.dec_weff instead of rebuilding them in each of their workgroups.  Valid only behind
 * svgp_mnist_encoder_kernel_matrix_fwd with the SAME theta on the same workspace (svgp_mnist_step_phase issues them so). */
int svgp_mnist_decoder_fwd_pre(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws, void* stream);
int svgp_mnist_decoder_bwd_data_pre(const svgp_mnist_cfg*, const double* theta, const double* images,
                                    double* ws, const double* state, void* stream);
/* Titsias branch (cfg.titsias = 1), SVGPVAE_model.py:246-259: L_2 = -1/2 [b log 2pi + log det C + y^T C^-1 y +
 * sum_n (k_nn - q_n)/var_n], C = diag(var) + K_nm (K_mm + jI)^-1 K_mn + jI (b x b).  Computed in m x m space through
 * the Woodbury identity with the statistics S2_l = sum_n k_n k_n^T/(var_nl + j), v2_l = sum_n y_nl k_n/(var_nl + j):
 *   log det C = sum_n log(var_n + j) + log det(K + jI + S2) - log det(K + jI)
 *   y^T C^-1 y = sum_n y_n^2/(var_n + j) - v2^T (K + jI + S2)^-1 v2
 * so the b x b inverse and Cholesky of the reference never exist and the branch shards over rows like the Hensman
 * one (S2, v2 ride in the statA all-reduce).  p_m, p_v, the cross-entropy term and everything downstream are the
 * shared stages; with cfg.titsias the L_3 / KL seeds of their reverse passes are zero and
 * svgp_gp_titsias_bwd adds the L_2 gradients to ybar, s2bar, Knbar, knnbar, Kbar.
 *   svgp_gp_titsias_stats : after svgp_gp_stats_fwd (phase 0)        -> ws[tit_S2], ws[tit_v2]
 *   svgp_gp_titsias_fwd   : after svgp_gp_posterior_fwd (phase 1)    -> ws[tit_Si], ws[tit_t], ws[tit_scal]
 *   svgp_gp_titsias_bwd   : after svgp_gp_posterior_bwd (phase 2), before svgp_kernel_matrix_bwd
 * Scratch: stats ws[scr_bl], ws[scr_bm]; fwd ws[scr_inv]; bwd ws[scr_mm], ws[scr_bm], ws[scr_bl] and ws[Knbar_part], which every
 * layout with cfg.titsias sizes as max(L b m, b m + 2 b L).  The Kbar increment is the same on every rank of a row-sharded step:
 * at m > 64, where the kernel-matrix reverse pass takes Kbar as it is, it is scaled by cfg.rep_weight here.       */
int svgp_gp_titsias_stats(const svgp_mnist_cfg*, double* ws, void* stream);
int svgp_gp_titsias_fwd(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_titsias_bwd(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* upstream gradients of p_m, p_v + backward statistics block statB (DP all-reduces it) */
int svgp_gp_stats_bwd(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* all m x m reverse algebra -> Kbar and the per-channel matrices of the row stage */
int svgp_gp_factor_bwd(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* row-local gradients: Knbar, knnbar, ybar, s2bar */
int svgp_gp_posterior_bwd(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* VJP of kernel_matrix: gradients of inducing points, l_GP, amplitude, object_vectors into grad */
int svgp_kernel_matrix_bwd(const svgp_mnist_cfg*, const double* theta, const double* aux,
                           double* ws, void* stream);
/* reverse of the encoder (through exp and the clip mask); encoder weight-gradient partials */
int svgp_mnist_encoder_bwd(const svgp_mnist_cfg*, const double* theta, const double* images,
                           double* ws, void* stream);
/* fixed-order reduction of all partials into the final block [grad | sums] (DP all-reduces it) */
int svgp_mnist_grad_reduce(const svgp_mnist_cfg*, double* ws, void* stream);
/* What the training phases use instead of the pair (svgp_kernel_matrix_bwd, svgp_mnist_grad_reduce): the
 * kernel-matrix VJP without its last launch (the deterministic scatter of the gathered-row gradients into the object
 * table and the two hyper-parameter sums), and the reduction launch with those workgroups appended -- one dependent
 * launch less on the critical path.  Results are identical. */
int svgp_kernel_matrix_bwd_partials(const svgp_mnist_cfg*, const double* theta, const double* aux, double* ws,
                                    void* stream);
int svgp_mnist_grad_reduce_all(const svgp_mnist_cfg*, const double* aux, double* ws, void* stream);
/* part 1: everything of svgp_mnist_grad_reduce_all except the encoder's weights (decoder weights, scalar sums, object-table
 * scatter and GP hyper-parameter sums) -> gradC[n_enc:]; part 2: the encoder's weights -> gradC[:n_enc].  1 + 2 == _all.
 * svgp_mnist_step_phase phases 4 / 5 = phase 2 cut at that point (4: ... kernel-matrix reverse pass, part 1; 5: encoder reverse
 * pass, part 2) for cfg.split_grad_exchange. */
int svgp_mnist_grad_reduce_part(const svgp_mnist_cfg*, const double* aux, double* ws, int part, void* stream);
/* Two more phase-form pairs with identical results (m <= 64; for larger m they are the plain stages).  A piece of work
 * that is off the critical path moves into extra workgroups of a later launch that leaves most CUs idle:
 *   (A_hat + jI)^-1 and the log det term of KL:  svgp_gp_factor_fwd_defer_aji ... svgp_gp_stats_bwd_with_aji
 *   the channel sum Kbar:                        svgp_gp_factor_bwd_nofinal   ... svgp_gp_posterior_bwd_with_final */
int svgp_gp_factor_fwd_defer_aji(const svgp_mnist_cfg*, double* ws, void* stream);
/* svgp_mnist_encoder_fwd + svgp_kernel_matrix_fwd (independent of each other) in one launch: the kernel-matrix
 * elements are computed by extra workgroups of the encoder launch */
int svgp_mnist_encoder_kernel_matrix_fwd(const svgp_mnist_cfg*, const double* theta, const double* images,
                                         const double* aux, double* ws, void* stream);
int svgp_gp_stats_bwd_with_aji(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* what the training phases use since round 2 for the same deferred work: svgp_gp_factor_fwd_defer_aji ...
 * svgp_gp_posterior_fwd_with_aji (L more workgroups of the row-stage launch, which has several workgroups per CU in
 * flight) ... svgp_gp_stats_bwd.  Results identical. */
int svgp_gp_posterior_fwd_with_aji(const svgp_mnist_cfg*, const double* eps, double* ws, double* state, void* stream);
/* m > 64: svgp_gp_factor_fwd_defer_aji leaves out the whole tail of the stage -- (A_hat_l + jI)^-1, its log det and the KL_l
 * scalars -- and this call performs it.  It may be issued on a DIFFERENT stream (ordered after svgp_gp_factor_fwd_defer_aji,
 * joined before svgp_gp_factor_bwd / the final scalars): it shares no buffer with svgp_gp_posterior_fwd, the decoder and
 * svgp_gp_stats_bwd, so the second batched inverse of the step runs beside them (svgp_mnist_step_phase does this on a
 * library-owned side stream unless SVGP_SIDE_STREAMS=0). */
int svgp_gp_factor_fwd_aji_tail(const svgp_mnist_cfg*, double* ws, void* stream);
/* m > 64: the pieces of the two factor stages.  A piece is what a caller may issue on its own, on another stream, before or
 * after a join; an entry point runs its pieces in the order of the table, and the entry points of one stage that together hold
 * every piece once == the stage itself, operation for operation.
 *
 *   forward   computes                                               entry points that contain it
 *   K         (K + jI)^-1, its log det, Kn Ki, q, W, P^T            svgp_gp_factor_fwd, _defer_aji
 *   SIG       Sigma^-1, t, G, A_hat (+ A_hat + jI), mu              svgp_gp_factor_fwd, _defer_aji
 *   KL        u = Ki mu, the trace terms of KL_l                    svgp_gp_factor_fwd, _defer_aji
 *   TAIL      (A_hat + jI)^-1, its log det, KL_l                    svgp_gp_factor_fwd, _aji_tail
 *
 *   reverse   computes                                               entry points that contain it (svgp_gp_factor_bwd and ...)
 *   SW        SW = P^T S P, unless svgp_gp_stats_bwd formed it      _early, _early_a
 *   EARLY_B   H = G (Ki - (A_hat + jI)^-1), H G^T, channel sums     _early, _early_b
 *   LATE_A    the vector chain ubar, mubar, tbar (+ X block *)      _late, _late_a
 *   CHANNELS  (X block otherwise,) Ssym, the channel sum of Sg      _late, _late_b, _late_b_channels
 *   KBAR      K Pbar^T, Kib, Ki Kib Ki, Pbar^T Ki (five launches)   _late, _late_b, _late_b_kbar
 *   FINAL     the assembly of Kbar                                  _late, _late_b, _late_b_final
 *   (*) X block = X, vbar, Si X, -(Si X) Si: in LATE_A when the statistic SW is formed by svgp_gp_stats_bwd (all rows local,
 *       b < 3 m) or with cfg.titsias -- the row form -- and in CHANNELS otherwise.
 *
 * What a piece needs: SW forward quantities only, not even (A_hat + jI)^-1 -- it may run beside _aji_tail on a third stream;
 * EARLY_B also the loss seeds of `state` and (A_hat + jI)^-1, no reverse statistic -- it may run on the stream of _aji_tail,
 * behind it; the late pieces A2 / ud / td (svgp_gp_stats_bwd and their exchange).  LATE_A reads nothing the early half writes:
 * a caller that runs the early half on another stream issues it BEFORE joining that stream.  KBAR reads nothing of CHANNELS
 * and may run beside it on another stream; FINAL follows both.
 * WRITE SET of _late_a: the scratch vectors ubar / mubar / tbar always; in the row form also ws.vbar, the Ssym slot
 * (it parks Si X there) and scratch matrix 1 (X, then -(Si X) Si) -- none of which the early half touches IN THAT FORM (it then
 * skips its own T = S P in scratch matrix 1).  The form is a function of cfg.b / cfg.b_global / cfg.titsias alone and is
 * evaluated by svgp_gp_stats_bwd, _early and _late_a independently: a caller must not change those fields between the three
 * calls of one step (svgp_mnist_step_phase / _train_step never do; row-form X0 itself is left in scratch matrix 2 by
 * svgp_gp_stats_bwd, so the stage may be repeated on a workspace). */
int svgp_gp_factor_bwd_early(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_early_a(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_early_b(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late_a(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late_b(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late_b_channels(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late_b_kbar(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_late_b_final(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_gp_factor_bwd_nofinal(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* m <= 64: svgp_kernel_matrix_bwd_partials + svgp_mnist_encoder_bwd in ONE launch (the two are independent: both consume the
 * reverse row stage; tf.gradients of SVGPVAE_model.py:427-476 and VAE_utils.py:112-126,143-152).  Results identical. */
int svgp_mnist_encoder_bwd_km(const svgp_mnist_cfg*, const double* theta, const double* images, const double* aux,
                              double* ws, void* stream);
/* m <= 64, the training step's form: svgp_gp_posterior_bwd = _rows (pass 1: ybar, s2bar, the per-channel partials of Knbar) + pass 2
 * (the sums over channels: Knbar, knnbar, Kbar -- consumed by the kernel-matrix VJP only); _km_sum = pass 2 + the VJP + the encoder's
 * reverse pass in ONE launch: the VJP workgroups wait for the pass-2 workgroups on a counter in ws.flags (release / acquire at
 * agent scope), the image workgroups wait for nobody.  Results identical to the separate launches. */
int svgp_gp_posterior_bwd_rows(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_mnist_encoder_bwd_km_sum(const svgp_mnist_cfg*, const double* theta, const double* images, const double* aux,
                                  double* ws, const double* state, void* stream);
/* Diagnostic: registers per lane of the (m 32, M 8) instance of that launch.  A kernel-matrix VJP workgroup and an image workgroup
 * share a CU only while it is <= 168; the kernel carries no occupancy hint (it cost the image code 1.7 us), tests check the number. */
int svgp_mnist_encoder_bwd_km_regs(int* out);
/* m <= 32, training step (round 6): svgp_mnist_decoder_bwd_data_pre + the deferred tail of the forward factor stage -- Aji = (A_hat +
 * jitter I)^-1 and the log det term of KL (SVGPVAE_model.py:271-279), left open by svgp_gp_factor_fwd_defer_aji -- as L rider
 * workgroups at the head of the same launch.  The forward row stage then runs as svgp_gp_posterior_fwd (7.8 us instead of the 10.1 us
 * of svgp_gp_posterior_fwd_with_aji, whose riders bounded it).  Same bits.  _regs: registers per lane of that kernel (<= 168 keeps a
 * rider and an image workgroup on one CU). */
int svgp_mnist_decoder_bwd_data_pre_aji(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws,
                                        const double* state, void* stream);
int svgp_mnist_decoder_bwd_data_aji_regs(int* out);
/* m <= 64, training step (SVGP_DEC_FUSE): svgp_mnist_decoder_fwd_pre followed by svgp_mnist_decoder_bwd_data_pre (_aji: by
 * svgp_mnist_decoder_bwd_data_pre_aji, m <= 32) as ONE launch: workgroup n of the second launch consumed only what workgroup n of
 * the first produced, so one image loop runs z -> h0, a1, a2, recon, squared error -> d2, d1, dh0 -> zbar with the activations and
 * weights resident in LDS.  Same arithmetic in the same order: same bits in every output of the launches it replaces.
 * _fused_regs: out[0..2] for the rider form, out[3..5] for the form without riders: registers per lane, scratch bytes per lane
 * (hipFuncGetAttributes) and the dynamic LDS bytes of an image workgroup at latent size L.  A rider and an image workgroup share a CU
 * only while registers <= 168, scratch == 0 and LDS <= 80 KB; the kernel carries no occupancy hint, tests check the numbers. */
int svgp_mnist_decoder_fwd_bwd_data_pre(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws,
                                        const double* state, void* stream);
int svgp_mnist_decoder_fwd_bwd_data_pre_aji(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws,
                                            const double* state, void* stream);
int svgp_mnist_decoder_fused_regs(int L, int* out);
/* The fused launches keep ws.dec_weff in LDS with the four parity classes of each up-convolution a padded stride apart (disjoint
 * bank windows for the lanes of one 16-byte read; ws.dec_weff itself stays packed).  _weff_lds_offset: host arithmetic, no GPU --
 * the offset in doubles, from the start of that image, of element `element` (packed index ((class * 4 + tap) * CIN + ci) * COUT + co)
 * of layer 0..2 (UpC1, UpC2, UpC3: 1024, 1024, 128 elements); element == the layer's count returns the end of the layer's block;
 * -1 outside.  _fused_lds_bytes: the dynamic LDS bytes of an image workgroup at latent size L (1..64; -1 outside), no GPU. */
int svgp_mnist_decoder_weff_lds_offset(int layer, int element);
int svgp_mnist_decoder_fused_lds_bytes(int L);
/* The same launches keep three 8-channel activation arrays at a padded PIXEL stride in LDS (d2 and d1 for the stride-2 gathers of the
 * two MFMA data reverses, a2 for the 16-byte gathers of the UpC3 forward; a2g, d2g, d1g stay packed) and pay for it, inside the
 * unchanged footprint, by two aliases of arrays that are never live together (d1 in the d3 block, dh0 on h0).  Host arithmetic, no GPU:
 * _fused_lds_array: array `which` (0 dense weights and biases, 1 effective-weight image, 2 z, 3 h0, 4 a1, 5 a2, 6 d3, 7 d2, 8 d1,
 *   9 dh0, 10 reduction scratch) at latent size L (1..64): returns its extent in doubles and writes (where the pointer is not NULL) its
 *   offset in doubles in the block, its pixel stride in doubles (0: no pixel structure) and the first and last phase-probe stamp
 *   (1..14, svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe) of its live interval.  -1 outside.
 * _fused_lds_index: where packed element `packed_element` (pixel * channels + channel; for array 1 the index in ws.dec_weff) of array
 *   1..10 lies in its block, in doubles; -1 outside. */
int svgp_mnist_decoder_fused_lds_array(int L, int which, int* offset, int* pixel_stride, int* first_stamp, int* last_stamp);
int svgp_mnist_decoder_fused_lds_index(int which, int packed_element);
/* m <= 32, no cfg.titsias: the forward block of the training step with ONLY what the decoder needs in front of it (schedule switch
 * SVGP_FWD_SPLIT; svgp_mnist_train_step and the unsharded svgp_mnist_train_step_dp run these four in the slots of
 * svgp_gp_factor_fwd_defer_aji, svgp_gp_posterior_fwd, svgp_mnist_decoder_fwd_bwd_data_pre_aji and svgp_gp_posterior_bwd_rows /
 * _with_final).  Same arithmetic in the same order: every output has the bits of the full forms.
 *   _factor_fwd_head: Si, t = Si v, mu_hat = c K t, u = Ki mu_hat and q; no G, A, M2, Aji, KL.
 *   _posterior_fwd_z: p_m, p_v, e, eps, z and the CE partials from Si, t, u; no d, no L3 partial; M2 is not read.
 *   _decoder_fwd_bwd_data_pre_tail: the fused decoder launch whose L riders run the rest of the factor stage from K, Ki, Si, mu_hat,
 *     u: G, A, M2, the traces, (A_hat + jI)^-1, KL (both entries with cfg.kl_form).  _fused_tail_regs: out[0..2] registers per lane,
 *     scratch bytes per lane, dynamic LDS bytes at latent size L (bounds as for svgp_mnist_decoder_fused_regs).
 *   _posterior_bwd_rows_d: svgp_gp_posterior_bwd_rows that also forms d = (knn - q) + k^T M2 k + e^2 and the L3 partials.
 * svgp_fwd_split_regs: out[0..11] registers and scratch bytes per lane of the head, z and d kernels (m = 32 instance, run-time-m
 * instance).  SVGP_ERR_UNSUPPORTED for m > 32 or cfg.titsias, before anything is launched. */
int svgp_gp_factor_fwd_head(const svgp_mnist_cfg*, double* ws, void* stream);
int svgp_gp_posterior_fwd_z(const svgp_mnist_cfg*, const double* eps, double* ws, double* state, void* stream);
int svgp_mnist_decoder_fwd_bwd_data_pre_tail(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws,
                                             const double* state, void* stream);
int svgp_gp_posterior_bwd_rows_d(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
int svgp_mnist_decoder_fused_tail_regs(int L, int* out);
int svgp_fwd_split_regs(int* out);
/* m <= 64: svgp_gp_factor_bwd_nofinal + svgp_mnist_decoder_bwd_weights(threads = 256) in ONE launch: the L channel workgroups
 * first, then min(b, 256) rider workgroups with the decoder's weight-gradient partials (needs svgp_mnist_decoder_bwd_data before). */
int svgp_gp_factor_bwd_nofinal_wgrad(const svgp_mnist_cfg*, const double* images, double* ws, const double* state,
                                     void* stream);
/* ... and svgp_gp_stats_bwd as P L leading workgroups of the same launch (single-GPU step only: nothing may be exchanged between the
 * reverse statistics and the reverse factor stage).  Channel workgroup l waits for its own P producers on ws.flags[8 + l] (write-through
 * payload, drained, relaxed agent-scope counter; the consumer re-arms it).  Same bits as svgp_gp_stats_bwd followed by
 * svgp_gp_factor_bwd_nofinal_wgrad.  L <= 56. */
int svgp_gp_stats_factor_bwd_wgrad(const svgp_mnist_cfg*, const double* images, double* ws, const double* state,
                                   void* stream);
int svgp_gp_posterior_bwd_with_final(const svgp_mnist_cfg*, double* ws, const double* state, void* stream);
/* In-kernel phase timeline of the two longest launches of the config-2 step (tools/decoder_phase_probe.py): probe instances of
 * svgp_mnist_decoder_fwd_bwd_data_pre_tail and of svgp_gp_stats_factor_bwd_wgrad (m = 32, five LDS matrices).  Same results as the
 * product launches; thread 0 of workgroup w also writes wall_clock64() stamps (100 MHz, one time axis for all workgroups) to row w of
 * `stamps`, a device buffer of n_stamps elements that nothing else reads.  Zero it first: a slot a workgroup does not reach stays 0.
 * Not for a captured stream (the buffer's address is handed over by a blocking copy into one device variable that every workgroup
 * reads at its entry): synchronise the stream between a probe launch and the next probe call -- a call with another buffer while
 * workgroups of the previous launch still wait for a slot would redirect their rows.
 *   _decoder_..._probe: 16 slots per workgroup -- 0 entry, 1 weights staged, 2 z, 3 dense, 4 / 5 / 6 UpC1 / UpC2 / UpC3 forward,
 *     7 copy-outs + squared error, 8 UpC3 data-reverse, 9 d2 scaled and stored, 10 UpC2 data-reverse, 11 d1 scaled and stored,
 *     12 UpC1 data-reverse, 13 z-bar, 14 exit (slots 2..13: the workgroup's last image); a rider workgroup writes 0, 14 and 15 only.
 *   _gp_stats_..._probe: 8 slots -- 0 entry, then for a rider 1 staged, 2 UpC3, 3 UpC2, 4 UpC1 + dense (its last image), 5 partial
 *     stored; 6 exit (every workgroup).
 *   Last slot of a row: bits 0..31 HW_ID (bits 8..15: compute unit, shader array, shader engine), 32..35 XCC_ID, 56..59 a rider's
 *     layer-group mask (1 UpC3, 2 UpC2, 4 UpC1 + dense), 60..63 role (decoder launch: 1 image, 2 rider; factor launch: 1 statistics,
 *     2 channel, 3 rider).
 * SVGP_ERR_INVALID when the buffer is NULL or holds fewer than (workgroups x slots) elements, SVGP_ERR_UNSUPPORTED for another form. */
int svgp_mnist_decoder_fwd_bwd_data_pre_tail_probe(const svgp_mnist_cfg*, const double* theta, const double* images, double* ws,
                                                   const double* state, unsigned long long* stamps, long long n_stamps,
                                                   void* stream);
int svgp_gp_stats_factor_bwd_wgrad_probe(const svgp_mnist_cfg*, const double* images, double* ws, const double* state,
                                         unsigned long long* stamps, long long n_stamps, void* stream);
/* tf.train.AdamOptimizer.apply_gradients, TF1 formula (MNIST_experiment.py:200,207-208) */
int svgp_adam_tf1_step(int64_t n, double* theta, const double* grad, double* adam_m, double* adam_v,
                       const double* state, double beta1, double beta2, double epsilon, void* stream);
/* scalar members of the 16-tuple + GECO state update + global_step (SVGPVAE_model.py:880-925,
 * MNIST_experiment.py:334-355) */
int svgp_elbo_finalize(const svgp_mnist_cfg*, double* ws, double* state, void* stream);
/* svgp_adam_tf1_step + svgp_elbo_finalize in one launch (what phase 3 uses) */
int svgp_adam_tf1_finalize(const svgp_mnist_cfg*, int64_t n, double* theta, const double* grad, double* adam_m,
                           double* adam_v, double* ws, double* state, double beta1, double beta2, double epsilon,
                           void* stream);
/* same, but global_step is not advanced (forward/backward only, no optimiser update) */
int svgp_elbo_finalize_noadam(const svgp_mnist_cfg*, double* ws, double* state, void* stream);

/* ---- phases: the stages above grouped between the data-parallel exchange points -------------
 * phase 0: encoder_kernel_matrix_fwd, gp_stats_fwd                 -> all-reduce ws[statA]
 * phase 1: gp_factor_fwd_defer_aji, gp_posterior_fwd, decoder_fwd, decoder_bwd, gp_stats_bwd_with_aji
 *                                                                   -> all-reduce ws[statB]
 * phase 2: gp_factor_bwd_nofinal, gp_posterior_bwd_with_final, kernel_matrix_bwd_partials, encoder_bwd,
 *          grad_reduce_all
 *                                                                   -> all-reduce ws[gradC]
 * phase 3: adam_tf1_step (skipped when adam_m == NULL), elbo_finalize
 * svgp_mnist_train_step runs phases 0..3 back to back (single GPU).
 * m > 64 without cfg.titsias (unless SVGP_SIDE_STREAMS=0): phase 1 issues svgp_gp_factor_fwd_aji_tail and
 * svgp_gp_factor_bwd_early on a side stream and records that for `ws`; phase 2 joins the branch and runs
 * svgp_gp_factor_bwd_late only when that record exists for the same (stream, ws) -- otherwise (phase-1 stages issued
 * through the individual entry points, switch changed in between, cfg.titsias) it runs the whole reverse factor
 * stage.  With cfg.titsias nothing is forked: svgp_gp_titsias_fwd uses the inverse scratch the tail would use.
 * The lines above are the un-merged outline; what is issued for a configuration, in order, is printed by svgp_mnist_step_route. */
int svgp_mnist_step_phase(const svgp_mnist_cfg*, int phase, double* theta, const double* images,
                          const double* aux, const double* eps, double* ws, double* state,
                          double* adam_m, double* adam_v, void* stream);
int svgp_mnist_train_step(const svgp_mnist_cfg*, double* theta, const double* images,
                          const double* aux, const double* eps, double* ws, double* state,
                          double* adam_m, double* adam_v, void* stream);
/* The launch schedule of a step as text, one op per line, in issue order: what svgp_mnist_step_phase (form 0, `phase` 0..5;
 * early_issued: phase 1 recorded the early reverse half for the workspace), svgp_mnist_train_step (form 1) and
 * svgp_mnist_train_step_dp on rank `rank` of `nranks` (form 2) enqueue for this configuration under the schedule switches of the
 * environment (adam: adam_m != NULL).  It is the plan those entry points execute; no GPU call, needs no device.  Lines:
 *   <lane> <entry point> [arg]      a stage on lane main (the caller's stream), side0 or side1 (the library's side branches); arg: the
 *                                   piece set of svgp_gp_factor_fwd_pieces / svgp_big_factor_fwd / _bwd (K SIG KL TAIL HEAD ALL; EARLY
 *                                   LATE_A CHANNELS KBAR FINAL LATE ALL) or the part of svgp_mnist_grad_reduce_part
 *   fork <lane> / join <lane>       the side branch continues behind the caller's stream / the caller's stream behind the branch
 *   <lane> allreduce <block>        statA statB gradC; gradC_hi = gradC[n_enc:], gradC_lo = gradC[:n_enc] (cfg.split_grad_exchange)
 * and in points 1..4 of the channel-sharded form:
 *   main point_begin <k> / main point_end <k>      (the timing bracket of svgp_comm_timing)
 *   main pack <block> all|window  /  main unpack <block> all|window|others     tile-packing; window: the rank's channels
 *   main group_begin / main group_end              one RCCL launch
 *   main reduce_scatter <block> [packed]  /  main allgather <block> [packed]   block: S v Si t u A2 ud td Ssym vbar KL
 * SVGP_ERR_INVALID when the text needs more than cap bytes. */
int svgp_mnist_step_route(const svgp_mnist_cfg*, int form, int phase, int nranks, int rank, int adam, int early_issued,
                          char* buf, int cap);
/* The same text; where the plan runs the SVGP_FWD_SPLIT forms, the line of each of the four slots ends in " -> <entry that runs>"
 * (svgp_gp_factor_fwd_head, svgp_gp_posterior_fwd_z, svgp_mnist_decoder_fwd_bwd_data_pre_tail, svgp_gp_posterior_bwd_rows_d or, where
 * pass 2 stays in the stage, svgp_gp_posterior_bwd_with_final_d: _with_final with pass 1 in the d form). */
int svgp_mnist_step_route_forms(const svgp_mnist_cfg*, int form, int phase, int nranks, int rank, int adam, int early_issued,
                                char* buf, int cap);

/* ---- data-parallel exchange over RCCL on the compute stream -------------------------
 * The reference is single-process; these are the three sum-exchanges the row-sharded step needs
 * (statistics S_l, v_l of SVGPVAE_model.py:328-334,339-340; their reverse-mode counterparts; the
 * parameter gradients of MNIST_experiment.py:197-208).  One communicator per process (= per GPU).
 * Bootstrap: rank 0 calls svgp_comm_unique_id, the bytes reach the other ranks by any side channel
 * (torch.distributed broadcast_object_list in engine.py), every rank calls svgp_comm_init with its
 * device current.  RCCL itself is resolved with dlopen at the first call (SVGP_ERR_UNSUPPORTED when
 * absent).  svgp_mnist_train_step_dp = phase 0 | all-reduce statA | phase 1 | all-reduce statB |
 * phase 2 | all-reduce gradC | phase 3, all enqueued on `stream` with no host synchronisation;
 * cfg->b is the rank's row count, cfg->b_global the global batch, cfg->rep_weight 1 on one rank.   */
int svgp_comm_unique_id_bytes(void);
int svgp_comm_unique_id(void* out, int nbytes);
int svgp_comm_init(const void* unique_id, int nbytes, int rank, int nranks, void** comm_out);
int svgp_comm_destroy(void* comm);
int svgp_allreduce_sum_f64(void* comm, double* buf, int64_t count, void* stream);
int svgp_allreduce_sum_f32(void* comm, float* buf, int64_t count, void* stream);   /* float32 streaming statistics */
/* Channel-sharded exchange for large (L,m,m) blocks (SURVEY 8e "reduce-scatter over L -> factorize L/G channels per rank
 * -> all-gather"): in-place on a buffer of nranks equal chunks, rank r owning buf[r * count, (r+1) * count).  The
 * schedule (sprites.py / engine.ChannelShardedExchange): reduce-scatter S, v over channels | svgp_gp_factor_fwd_channels
 * on the rank's window | all-gather Sigma_l^-1, M2, t, u, KL | ... | reduce-scatter A2, ud, td |
 * svgp_gp_factor_bwd_channels | all-gather Ssym, vbar.  Kbar needs no exchange: each rank's window share flows
 * through svgp_kernel_matrix_bwd (linear in Kbar) into the gradient all-reduce (cfg.rep_weight = 1 on every rank).    */
int svgp_reduce_scatter_sum_f64(void* comm, double* buf, int64_t count_per_rank, void* stream);
int svgp_allgather_f64(void* comm, double* buf, int64_t count_per_rank, void* stream);
/* the factor stages restricted to the channel window [l0, l0 + nl) (m > 64): (K_mm + jI)^-1 and q_n are formed by every
 * call; with l0 = 0, nl = L they are svgp_gp_factor_fwd / svgp_gp_factor_bwd                                            */
int svgp_gp_factor_fwd_channels(const svgp_mnist_cfg*, int l0, int nl, double* ws, void* stream);
int svgp_gp_factor_bwd_channels(const svgp_mnist_cfg*, int l0, int nl, double* ws, const double* state, void* stream);
/* ... and their pieces (the table at svgp_gp_factor_bwd_early) on a channel window, the split of the two-stream step.
 * Forward `part`: 0 = K SIG KL TAIL, 1 = K SIG KL, 2 = TAIL.  Reverse `part`: 0 = all six, 1 = SW EARLY_B, 2 = LATE_A
 * CHANNELS KBAR FINAL, 3 = SW, 4 = EARLY_B.  Any other value: SVGP_ERR_INVALID.                                          */
int svgp_gp_factor_fwd_channels_part(const svgp_mnist_cfg*, int l0, int nl, int part, double* ws, void* stream);
int svgp_gp_factor_bwd_channels_part(const svgp_mnist_cfg*, int l0, int nl, int part, double* ws, const double* state,
                                     void* stream);
/* svgp_mnist_train_step_dp, channel-sharded form (m > 64, L divisible by the rank count): five exchange POINTS, each ONE
 * grouped RCCL launch (ncclGroupStart / End): [S | v] reduce-scatter, [Sigma^-1 | M2 | t | u] all-gather, [A2 | ud | td]
 * reduce-scatter, [Ssym | vbar | KL] all-gather, gradient all-reduce.  The (L,m,m) members are symmetric and travel
 * TILE-PACKED (svgp_sym_pack: lower triangle in 32 x 32 tiles, 52 % of the square at m = 800; SURVEY 8e "halve via
 * symmetry") with SVGP_DP_PACK=1, off with 0; default: svgp_dp_pack_default(m).  The tail of the forward factor stage and the early
 * half of the reverse one run on the library's side stream beside the all-gather, the row stage, the networks and the reverse
 * statistics (as in the single-GPU step; SVGP_SIDE_STREAMS=0 puts them in line).                                      */
int svgp_mnist_train_step_dp(const svgp_mnist_cfg*, void* comm, double* theta, const double* images,
                             const double* aux, const double* eps, double* ws, double* state,
                             double* adam_m, double* adam_v, void* stream);
/* Several collectives as one RCCL launch: everything issued on `comm` between _begin and _end (ncclGroupStart / End). */
int svgp_comm_group_begin(void* comm);
int svgp_comm_group_end(void* comm);
/* HIP events around every exchange point of svgp_mnist_train_step_dp (pack + collective(s) + unpack): enable != 0 switches
 * the recording on; svgp_comm_timing_read waits for the last recorded step and returns the microseconds of its points
 * (n <= cap of them, in step order).  bench.py --gpus N reports them as `collectives_us`.                              */
int svgp_comm_timing(void* comm, int enable);
int svgp_comm_timing_read(void* comm, float* us, int cap, int* n);
/* Tile-packed lower triangle of L symmetric m x m matrices: per matrix the nt (nt + 1) / 2 tiles (ti >= tj) of 32 x 32,
 * nt = ceil(m / 32), tile t = ti (ti + 1) / 2 + tj stored row-major (rows / columns >= m are zero).  avg != 0: the tile
 * holds (x_ij + x_ji) / 2 (for products that are symmetric only up to rounding, M2 = Ki A Ki); else x_ij of the lower
 * tiles.  svgp_sym_unpack writes both triangles of the square matrices.  src / dst strides: m * m and packed_elems.   */
int64_t svgp_sym_packed_elems(int m);
/* 1 where the packed exchange is the default for this m (the single definition of the rule; SVGP_DP_PACK overrides it). */
int svgp_dp_pack_default(int m);
int svgp_sym_pack(int m, int L, int avg, const double* src, double* dst, void* stream);
int svgp_sym_unpack(int m, int L, const double* src, double* dst, void* stream);

/* ---- full-data statistics in float32, streamed over N (8f rank 1) -----------------
 * replace precompute_GP_params_SVGPVAE's K_nm build and its per-channel
 *   K_mn (K_nm * 1/var_l)  and  K_mn (mean_l / var_l)        (SVGPVAE_model.py:1004-1017)
 * for N-sized inputs: N = 2^20 rows / m = 2048 per the stress config, or the SPRITES training set
 * (SPRITES_experiment.py:176-182).  float32 is the reference's dtype for SPRITES (tf.float32).
 * kind 0: periodic(angle) x linear(object vector)   mnistSVGP.kernel_matrix   :427-476, p = [l_GP, amplitude]
 * kind 1: linear(action) x linear(character)         spritesSVGP.kernel_matrix :550-600
 * kind 2: SE(action) x SE(character), --K_SE         :530-544,                 p = [l1, sigma1, l2, sigma2]
 * normalize = cosine normalisation of the linear factors (:465-474, :576-598).
 * Batch rows x: kind 0 (n, 2+d2) [id, angle, o..] with o gathered from `table` (n_table, d2) when
 * n_table > 0; kinds 1,2 (n, 1+d2) [action_id, chr..] with the action vector gathered from `table`
 * (n_table, d1).  Inducing rows: kind 0 (m, 2+d2); kinds 1,2 (m, d1+d2).
 * svgp_stream_features_f32 writes feature_elems(n) floats; svgp_stream_knm_f32 writes K_nm (n, m) row-major;
 * svgp_stream_stats_f32 writes S (L, m, m) = K_nm^T diag(1/var_l) K_nm and v (L, m) = K_nm^T (mean_l/var_l),
 * means / vars (n, L) row-major, 1/var via reciprocal_no_nan.  Nothing is added or inverted here.       */
typedef struct {
    int32_t kind, d1, d2, normalize, n_table;
    float   p[4];
} svgp_stream_kdesc;
int64_t svgp_stream_feature_elems(const svgp_stream_kdesc*, int64_t n);
int svgp_stream_features_f32(const svgp_stream_kdesc*, int64_t n, const float* x, int ldx, int inducing,
                             const float* table, float* feat, void* stream);
int svgp_stream_knm_f32(const svgp_stream_kdesc*, int64_t n, int m, const float* feat_rows,
                        const float* feat_inducing, float* K_nm, void* stream);
int64_t svgp_stream_stats_workspace_elems(int64_t n, int m, int L);
int svgp_stream_stats_f32(int64_t n, int m, int L, const float* K_nm, const float* means, const float* vars,
                          float* S, float* v, float* ws, int64_t ws_elems, void* stream);

/* ---- batched float64 linear algebra on device matrices (large-m path; also usable on their own) ---
 * replace tf.matmul / tf.linalg.inv / tf.linalg.cholesky+log(diag) (SVGPVAE_model.py:239,270-274,319,328-341)
 * svgp_dgemm_batched: C[l] = alpha op(A[l]) op(B[l]) + beta C[l]; C is M x N, contraction K; ta/tb = 1 means
 *   the operand is stored transposed (A as K x M, B as N x K); strides in elements, 0 = shared operand.
 * svgp_spd_inverse_batched: A (batch, m, m) contiguous SPD -> A^-1 in place (blocked Gauss-Jordan, no
 *   pivoting) and logdet[l] = log det A[l]; work holds svgp_spd_inverse_workspace_elems(m, batch) doubles. */
int svgp_dgemm_batched(int ta, int tb, int M, int N, int K, double alpha, const double* A, int lda,
                       long long strideA, const double* B, int ldb, long long strideB, double beta, double* C,
                       int ldc, long long strideC, int batch, void* stream);
/* the same GEMM on float64 matrices with the products and sums on the float32 MFMA (operands rounded to float32 while
 * staged into LDS, float32 accumulation; twice the matrix rate): the arithmetic of the reference's float32 SPRITES graph
 * (VAE_utils.py:277, SVGPVAE_model.py:516) on float64 storage; and the float32 GEMM of the float32 networks            */
int svgp_dgemm_f32c_batched(int ta, int tb, int M, int N, int K, double alpha, const double* A, int lda,
                            long long strideA, const double* B, int ldb, long long strideB, double beta, double* C,
                            int ldc, long long strideC, int batch, void* stream);
int svgp_sgemm_batched(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, long long strideA,
                       const float* B, int ldb, long long strideB, float beta, float* C, int ldc, long long strideC,
                       int batch, void* stream);
/* one GEMM with few output tiles and a long contraction (dense layers / their weight gradients): K is cut into slices
 * that run as a batch into partial products in `scratch` (svgp_dgemm_splitk_scratch_elems doubles, 0 = no split) and
 * are added in fixed order; same operand conventions as svgp_dgemm_batched with batch 1 */
long long svgp_dgemm_splitk_scratch_elems(int M, int N, int K);
int svgp_dgemm_splitk(int ta, int tb, int M, int N, int K, double alpha, const double* A, int lda, const double* B,
                      int ldb, double beta, double* C, int ldc, double* scratch, long long scratch_elems, void* stream);
size_t svgp_spd_inverse_workspace_elems(int m, int batch);
int svgp_spd_inverse_batched(int m, int batch, double* A, double* logdet, double* work, void* stream);
/* Cholesky family (cholesky.hip) -- north_star's "Cholesky of K_mm and the triangular solves"; they replace
 * tf.linalg.cholesky + log(diag_part) (SVGPVAE_model.py:270-274) and the solves / inverses behind :239,319,331.
 * Blocked right-looking with 64 x 64 diagonal blocks factored in LDS; panel solve, trailing update and every product of
 * the triangular inverse are the batched f64 MFMA GEMM with tiles / k-panels skipped where an operand is structurally 0.
 * svgp_potrf_batched: A (batch; m x m, row stride lda, batch stride strideA) SPD -> lower factor L in place (strict upper
 *   triangle zeroed), logdet[l] = log det A[l] = 2 sum log diag L.  A non-positive pivot gives NaNs (no error code: no
 *   host synchronisation).  On return the head of `work` holds the inverses of the 64 x 64 diagonal blocks of L,
 *   (batch, ceil(m/64), 64, 64), which svgp_potri_batched accepts as `linv_blocks`.
 * svgp_trsm_batched: side 0: op(L) X = B with B (batch; m x n);  side 1: X op(L) = B with B (batch; n x m);  trans 1:
 *   op(L) = L^T.  L lower triangular (its strict upper part is ignored), strideL = 0: one L for the whole batch.  B <- X.
 * svgp_potri_batched: A (batch, m, m) contiguous holding L -> A^-1 = L^-T L^-1 (full symmetric matrix); linv_blocks
 *   may be NULL (recomputed).  svgp_spd_inverse_batched is potrf + potri for m >= 512.                               */
size_t svgp_potrf_workspace_elems(int m, int batch);
size_t svgp_trsm_workspace_elems(int m, int n, int batch);
size_t svgp_potri_workspace_elems(int m, int batch);
int svgp_potrf_batched(int m, int batch, double* A, int lda, long long strideA, double* logdet, double* work, void* stream);
int svgp_trsm_batched(int side, int trans, int m, int n, const double* L, int ldl, long long strideL, double* B, int ldb,
                      long long strideB, int batch, double* work, void* stream);
int svgp_potri_batched(int m, int batch, double* A, const double* linv_blocks, double* work, void* stream);
/* Inverse of ONE general (m x m, m <= 2048) matrix by LU with partial pivoting (lu.hip): the reference's tf.linalg.inv(K_mm)
 * WITHOUT jitter in the SPRITES conditional-generation path (SPRITES_experiment.py:178; consumed at SVGPVAE_model.py:610-635).
 * With the linear x linear kernels K_mm has rank <= 128 < m = 800, where an elimination without pivoting has no answer.
 * A (row-major, contiguous) is not modified; Ainv must not alias it; work: svgp_lu_inverse_workspace_elems(m) doubles. */
size_t svgp_lu_inverse_workspace_elems(int m);
int svgp_lu_inverse(int m, const double* A, double* Ainv, double* work, void* stream);

/* ---- generic NHWC float64 convolution as a tap-table gather-GEMM on the f64 MFMA (conv_taps.hip) ---------
 * out[n][y*osy+ooy][x*osx+oox][co] = act(bias[co] + sum_t sum_ci in[n][y*sy+oy_t][x*sx+ox_t][ci] W_t[ci][co]),
 * (y,x) in Hs x Ws, reads outside the input are zero; W_t = w + woff[t] is a (Ci x Co) row-major matrix.
 * One descriptor = one class; classes of a launch share n, Hs, Ws.  With suitable tables: Keras Conv2D
 * 3x3/2x2, stride 1/2, same/valid; UpSampling2D(2)+Conv2D as four parity classes on effective weights; all
 * data gradients.  Replaces the Keras layers of spritesVAE / sprites_representation_network
 * (VAE_utils.py:294-338,375-391).  act: 0 none, 1 bias + ELU, 2 bias only.                             */
typedef struct {
    int32_t n, Hi, Wi, Ci;      /* input tensor (n,Hi,Wi,Ci)                                  */
    int32_t Ho, Wo, Co;         /* output tensor (n,Ho,Wo,Co)                                 */
    int32_t Hs, Ws;             /* iteration space of this class                              */
    int32_t sy, sx;             /* input stride per iteration step                            */
    int32_t osy, osx, ooy, oox; /* output placement                                           */
    int32_t nt, act;            /* taps (1..16), activation                                   */
    int32_t oy[16], ox[16], woff[16];
} svgp_conv_desc;
int svgp_conv_taps_fwd(const svgp_conv_desc* d, int ncls, const double* in, const double* w, const double* bias,
                       double* out, void* stream);
/* dW_t[ci][co] = sum_{n,y,x} in[...] * dout[...] for the same tap tables; part: (nwg, part_stride) scratch (the classes' tap ranges must be disjoint);
 * dw (part_stride values, laid out by woff) = fixed-order sum (accumulate != 0 adds to dw).               */
int svgp_conv_taps_wgrad(const svgp_conv_desc* d, int ncls, const double* in, const double* dout, double* part,
                         int nwg, int part_stride, double* dw, int accumulate, void* stream);
/* dpre = dout * elu'(out) in place on dout (out == NULL: no activation) and db[c] = sum over pixels of dpre;
 * part: (1024, C) scratch.                                                                                  */
/* UpSampling2D(2) + Conv2D 3x3 as four parity classes: effective weights we (2,2,2,2,Ci,Co) from w (3,3,Ci,Co), and the
 * gradient of w from the gradient of we (VAE_utils.py:317-338 decoder layers) */
int svgp_upconv_weights(int Ci, int Co, const double* w, double* we, void* stream);
/* Deferred partial sums.  Every svgp_conv_taps_wgrad_fused call ends in two small reductions (weight and bias partials ->
 * dw, db): 32 launches of ~10 us in the launch chains of a SPRITES step, whose results only the optimiser reads.  The *_jobs
 * forms run the convolution kernels as usual but RETURN the reductions as descriptors (at most `cap`, *n_jobs written);
 * svgp_sum_partials_multi[_f32] runs any number of them as one launch (per 64 jobs), adding in the same order as the
 * immediate form.  The caller keeps part / part_b intact until then (one scratch region per layer) and orders `stream`
 * behind every stream that produced partials.                                                                         */
typedef struct {
    const void* part;   /* (ng, stride) partials                     */
    void* out;          /* (len) sums                                */
    int32_t ng, len, stride, accumulate;
} svgp_sum_job;
int svgp_conv_taps_wgrad_fused_jobs(const svgp_conv_desc* d, int ncls, const double* in, const double* out, double* dout,
                                    double* part, double* part_b, int nwg, int part_stride, double* dw, double* db,
                                    svgp_sum_job* jobs, int cap, int* n_jobs, void* stream);
int svgp_conv_taps_wgrad_fused_jobs_f32(const svgp_conv_desc* d, int ncls, const float* in, const float* out, float* dout,
                                        float* part, float* part_b, int nwg, int part_stride, float* dw, float* db,
                                        svgp_sum_job* jobs, int cap, int* n_jobs, void* stream);
int svgp_sum_partials_multi(const svgp_sum_job* jobs, int n, void* stream);
int svgp_sum_partials_multi_f32(const svgp_sum_job* jobs, int n, void* stream);
/* w (nt, A, B) -> wt (nt, B, A): the transposed tap weights a data gradient convolves with; element-type casts of the
 * float32-network engine (master parameters / gradients are float64)                                                 */
int svgp_transpose_taps(int nt, int A, int B, const double* w, double* wt, void* stream);
int svgp_transpose_taps_f32(int nt, int A, int B, const float* w, float* wt, void* stream);
int svgp_cast_f64_f32(long long n, const double* x, float* y, void* stream);
int svgp_cast_f32_f64(long long n, const float* x, double* y, void* stream);
int svgp_upconv_fold_wgrad(int Ci, int Co, const double* ge, double* g, void* stream);
int svgp_elu_bwd_bias(long long npix, int C, const double* out, double* dout, double* part, double* db,
                      void* stream);
/* float32 instantiations of the five convolution entry points above: the reference's dtype for the SPRITES networks
 * (VAE_utils.py:277 `dtype = tf.float32`).  Same descriptors and tap tables; the gather-GEMM runs on
 * v_mfma_f32_16x16x4_f32.                                                                                             */
int svgp_conv_taps_fwd_f32(const svgp_conv_desc* d, int ncls, const float* in, const float* w, const float* bias,
                           float* out, void* stream);
int svgp_conv_taps_wgrad_f32(const svgp_conv_desc* d, int ncls, const float* in, const float* dout, float* part, int nwg,
                             int part_stride, float* dw, int accumulate, void* stream);
int svgp_upconv_weights_f32(int Ci, int Co, const float* w, float* we, void* stream);
/* Reverse pass of a layer's activation, bias and weights in ONE pass over dout (tf.gradients of Conv2D + bias + elu,
 * VAE_utils.py:294-338): dpre = dout * elu'(out) in place on dout (out == NULL: dpre = dout), db[co] = sum of dpre over
 * pixels, dW_t[ci][co] = sum in * dpre (layout by woff).  The classes' output pixel sets must be disjoint and together
 * cover dout.  16 input channels with 4 or 9 taps in every class: one fused kernel (every wave stages its own halo, no
 * workgroup barrier in the pixel loop); any other shape: svgp_elu_bwd_bias + svgp_conv_taps_wgrad in sequence.
 * part_b: (1024, 16) scratch; part: (nwg, part_stride) scratch. */
int svgp_conv_taps_wgrad_fused(const svgp_conv_desc* d, int ncls, const double* in, const double* out, double* dout,
                               double* part, double* part_b, int nwg, int part_stride, double* dw, double* db,
                               void* stream);
int svgp_conv_taps_wgrad_fused_f32(const svgp_conv_desc* d, int ncls, const float* in, const float* out, float* dout,
                                   float* part, float* part_b, int nwg, int part_stride, float* dw, float* db,
                                   void* stream);
int svgp_upconv_fold_wgrad_f32(int Ci, int Co, const float* ge, float* g, void* stream);
/* Which kernels a convolution call runs, as text: one line per launch, zero fill or partial-sum job, in order, with the
 * kernel instance (template values), grid, LDS bytes and by-value scalars.  pass 0: svgp_conv_taps_fwd; pass 1:
 * svgp_conv_taps_wgrad_fused (has_out: out != NULL).  elem_size: 4 or 8.  The same plan the launchers execute; makes no GPU
 * call and needs no device.  SVGP_ERR_INVALID when `cap` bytes do not hold the text. */
int svgp_conv_route(const svgp_conv_desc* d, int ncls, int pass, int has_out, int nwg, int part_stride, int elem_size,
                    char* buf, int cap);
int svgp_elu_bwd_bias_f32(long long npix, int C, const float* out, float* dout, float* part, float* db, void* stream);

/* ---- SPRITES pieces (gp_sprites.hip) ----------------------------------------------------------------------
 * spritesSVGP.kernel_matrix (SVGPVAE_model.py:550-600): K = k_action * k_character, each Linear (optionally
 * cosine-normalised) or ExponentiatedQuadratic (k_se; se = [l_action, sigma_action, l_character, sigma_character]).
 * aux (b, 1+Lc) = [action id, character vector]; ip (m, La+Lc); table = GPLVM action vectors (n_act, La).        */
typedef struct {
    int32_t b, m, La, Lc, n_act, normalize, k_se;
    double rep_weight;          /* weight of Kbar: m <= 64: 1 on rank 0 (Kbar is replicated); m > 64: 1 on every rank (the
                                 * reverse factor stage has weighted the replicated part with cfg.rep_weight itself) */
} svgp_sprites_kcfg;
int svgp_sprites_kernel_matrix_fwd(const svgp_sprites_kcfg*, const double* aux, const double* ip, const double* table,
                                   const double* se, double* K, double* Kn, double* knn, void* stream);
/* VJP: d_ip (m,La+Lc), d_table (n_act,La), d_char (b,Lc) (gradient of the batch character vectors), d_se (4).
 * scratch: scratch_elems doubles (row partials of the tiled pass).  svgp_sprites_kernel_bwd_scratch_elems(cfg) reads cfg.b as
 * the row CAPACITY and returns a size that covers every call with 1 <= b <= cfg.b (the need is not monotone in b); the call
 * itself fails with SVGP_ERR_INVALID when scratch_elems is below what its own b needs.                             */
long long svgp_sprites_kernel_bwd_scratch_elems(const svgp_sprites_kcfg*);
int svgp_sprites_kernel_matrix_bwd(const svgp_sprites_kcfg*, const double* aux, const double* ip, const double* table,
                                   const double* se, const double* Kbar, const double* Knbar, const double* knnbar,
                                   double* d_ip, double* d_table, double* d_char, double* d_se, double* scratch,
                                   long long scratch_elems, void* stream);
/* aux_data_SVGPVAE_sprites (SVGPVAE_model.py:1086-1115): segment_mean over seg_len consecutive frames, repeat,
 * prepend the action id; and its reverse.                                                                        */
int svgp_sprites_aux_fwd(int b, int seg_len, int Lc, const double* repr, const double* action_ids, double* aux,
                         void* stream);
int svgp_sprites_aux_bwd(int b, int seg_len, int Lc, const double* d_char, double* d_repr, void* stream);
/* AveragePooling2D over the whole (HW) map of an (n,HW,C) tensor (VAE_utils.py:388) and its reverse */
int svgp_avgpool_fwd(int n, int HW, int C, const double* x, double* y, void* stream);
int svgp_avgpool_bwd(int n, int HW, int C, const double* dy, double* dx, void* stream);
/* encoder head: enc (b,2L) += bias; mu = enc[:, :L], var_raw = exp(enc[:, L:]), var = clip (VAE_utils.py:347-348,
 * SVGPVAE_model.py:858-859); reverse through exp and the clip mask                                             */
int svgp_enc_head_fwd(int b, int L, int clip, const double* bias, double* enc, double* mu, double* var_raw,
                      double* var, void* stream);
int svgp_enc_head_bwd(int b, int L, int clip, const double* var_raw, const double* ybar, const double* s2bar,
                      double* d_enc, void* stream);
int svgp_bias_add(long long rows, int C, const double* bias, double* x, void* stream);
/* utils.py:483-504 gauss_cross_entropy, element-wise over n values: out = -1/2 (log 2 pi + log var2 +
 * (var1 + mu1^2 - 2 mu1 mu2 + mu2^2) / var2).  Inside the training step the same term is evaluated in the
 * per-sample kernels; this is the stand-alone form behind utils.gauss_cross_entropy                          */
int svgp_gauss_cross_entropy(long long n, const double* mu1, const double* var1, const double* mu2, const double* var2,
                             double* out, void* stream);
/* classification loss of the representation-network pre-training (SPRITES_utils.py:335-368): mean sparse softmax
 * cross-entropy over n rows of C logits, labels = class ids as float64; writes per-row losses, their mean and
 * d mean / d logits */
int svgp_softmax_xent(int n, int C, const double* logits, const double* labels, double* row_loss, double* loss,
                      double* dlogits, void* stream);
/* sum (x - xhat)^2 partials into the workspace's partial-sum area (block g writes part_sums[4g+2]) and
 * d loss / d xhat (beta-ELBO: 2(xhat-x)/n_pix; GECO: lagrange_mult/(b_global n_pix) times that)              */
int svgp_sqerr_fwd(long long tot, int n_part, const double* x, const double* xhat, double* part_sums, void* stream);
int svgp_sqerr_bwd(long long tot, int geco, int b_global, int n_pix, const double* state, const double* x,
                   const double* xhat, double* dxhat, void* stream);
/* float32 forms of the per-frame glue of the float32 networks; the squared-error partial sums and the device state stay
 * float64 (they feed the float64 scalar epilogue)                                                                     */
int svgp_avgpool_fwd_f32(int n, int HW, int C, const float* x, float* y, void* stream);
int svgp_avgpool_bwd_f32(int n, int HW, int C, const float* dy, float* dx, void* stream);
int svgp_bias_add_f32(long long rows, int C, const float* bias, float* x, void* stream);
int svgp_sqerr_fwd_f32(long long tot, int n_part, const float* x, const float* xhat, double* part_sums, void* stream);
int svgp_sqerr_bwd_f32(long long tot, int geco, int b_global, int n_pix, const double* state, const float* x,
                       const float* xhat, float* dxhat, void* stream);
/* tf.clip_by_value(grad, -thr, thr) (SPRITES_experiment.py:234-235) */
int svgp_clip_by_value(long long tot, double thr, double* g, void* stream);

/* ---- moving-ball experiment (ball.hip): BALL_experiment.py --elbo SVGPVAE_Hensman | SVGPVAE_Titsias ----------
 * build_SVGPVAE_elbo_graph (SVGPVAE_model.py:638-715) runs its two SVGP objects (:17-171) on the shared GP stage
 * entry points above with rows = the tmax frames, channels = the videos of the batch (all videos share the time
 * stamps 1..tmax, :663-664), N_train = b = tmax, kl_form = 1, clip_pv = 2: one workspace per latent coordinate.
 * svgp_se1d_kernel_matrix_fwd/bwd: tfk.ExponentiatedQuadratic(amplitude=None, length_scale) on scalar inputs (:60,
 *   :80-86): K (m,m), Kn (T,m), knn (T) = 1 from times x (T), inducing points z (m), *ls; VJP -> d_z (m), d_ls (1).
 * svgp_bias_act_fwd / svgp_act_bwd_bias: x = act(x + bias) in place (act 0 none, 1 tanh); dpre = dout act'(out) in
 *   place and db = column sums (one launch, fixed summation order; `part` is unused and may be NULL) - the layers of
 *   build_MLP_inference_graph / build_MLP_decoder_graph (VAE_utils.py:9-96); the matmuls are svgp_dgemm_batched.
 * svgp_ball_head_fwd/bwd: h (B*T,4) + bias -> qnet_mu, exp, clip [1e-6,1e3] (VAE_utils.py:50-55, SVGPVAE_model.py:
 *   670-671) written in the (T,B) channel layout of the x / y workspaces; reverse through exp and the clip mask.
 * svgp_ball_pack_z / unpack_zbar: latent samples (T,B) x 2 <-> (B*T,2).
 * svgp_sigmoid_xent: per frame -sum_pix sigmoid_cross_entropy_with_logits (:697-700), pred = sigmoid, and
 *   dlogits = scale (sigmoid - label); pred / dlogits may be NULL.
 * svgp_ball_elbo_assemble: per-video [elbo, recon, KL_term, inside_elbo, ce_term, inside_recon, inside_kl] (7,B)
 *   (:677-705), incl. the reference's batch-wide KL scalar; svgp_ball_finalize: their means over videos into the
 *   state's output slots (BALL_experiment.py:116-123), Adam step counter and RNG counter advance.               */
int svgp_se1d_kernel_matrix_fwd(int T, int m, const double* x, const double* z, const double* ls, double* K,
                                double* Kn, double* knn, void* stream);
int svgp_se1d_kernel_matrix_bwd(int T, int m, const double* x, const double* z, const double* ls, const double* Kbar,
                                const double* Knbar, double* d_z, double* d_ls, void* stream);
int svgp_bias_act_fwd(long long rows, int C, int act, const double* bias, double* x, void* stream);
int svgp_act_bwd_bias_scratch_elems(int C);
int svgp_act_bwd_bias(int rows, int C, int act, const double* out, double* dout, double* part, double* db,
                      void* stream);
int svgp_ball_head_fwd(int B, int T, int clip, const double* bias, const double* h, double* mu_x, double* var_raw_x,
                       double* var_x, double* mu_y, double* var_raw_y, double* var_y, void* stream);
int svgp_ball_head_bwd(int B, int T, int clip, const double* var_raw_x, const double* ybar_x, const double* s2bar_x,
                       const double* var_raw_y, const double* ybar_y, const double* s2bar_y, double* dh, void* stream);
int svgp_ball_pack_z(int B, int T, const double* zx, const double* zy, double* z, void* stream);
int svgp_ball_unpack_zbar(int B, int T, const double* dz, double* zbar_x, double* zbar_y, void* stream);
int svgp_sigmoid_xent(int rows, int P, double scale, const double* logits, const double* labels, double* pred,
                      double* row_recon, double* dlogits, void* stream);
int svgp_ball_elbo_assemble(const svgp_mnist_cfg* cfg_x, const double* ws_x, const double* ws_y,
                            const double* row_recon, const double* state, double* out, void* stream);
int svgp_ball_finalize(int B, int did_adam, long long rng_advance, const double* out, double* state, void* stream);
int svgp_state_add(double* state, int slot, double v, void* stream);
/* build_video_batch_graph's rasterisation (utils.py:172-187): vid[f][i][j] = (i - paths[f][0])^2 + (j - paths[f][1])^2 < r^2 */
int svgp_ball_rasterize(long long frames, int px, int py, double r, const double* paths, double* vid, void* stream);

/* ---- Pearce baseline of the moving-ball experiment: BALL_experiment.py --elbo GPVAE_Pearce | VAE | NP ----------
 * build_1d_gp (GPVAE_Pearce_model.py:8-86) with X_test = X (a general X_test, after training: svgp_pearce_predict
 * further down): exact GP regression per (video, latent coordinate),
 * one workgroup each, n <= 64 points:  A = K_SE(l) + diag(var), alpha = A^-1 y,
 *   lhood = -1/2 (n log 2pi + y.alpha + log det A),  p_m = K alpha,  p_v = 1 - diag(K A^-1 K),
 *   z = p_m + eps sqrt(p_v), per-frame -gauss_cross_entropy (utils.py:483-504) and their sums.
 * All per-frame buffers are (T, B) (frame-major, the layout svgp_ball_head_fwd writes); times (T).
 * idx (B, n) int32 != NULL: the points are times[idx[b][.]] (neural-process context sets, :121-155): forward gives
 * lhood only, reverse seeds it with seed_lh_scale (-1: the context likelihood is subtracted, :186) and accumulates.
 * tmask (B, T): weights of the cross-entropy terms (NP: 1 on target frames, :178-182).
 * svgp_pearce_elbo_assemble: per-video [elbo, recon, prior_kl, lhood, ce, context lhood, 0] (7,B) (:157-236). */
typedef struct {
    int32_t B, T, n;
    const double* times; const int32_t* idx; const double* tmask;
    const double* ls_x; const double* ls_y;
    double* y_x; double* y_y; double* s2_x; double* s2_y;
    double* p_m_x; double* p_m_y; double* p_v_x; double* p_v_y; double* eps_x; double* eps_y; double* z_x; double* z_y;
    double* zbar_x; double* zbar_y; double* ybar_x; double* ybar_y; double* s2bar_x; double* s2bar_y;
    double* Ai; double* alpha; double* lh; double* ce; double* row_ce; double* dl_part;
} svgp_pearce_bufs;
int svgp_pearce_gp_fwd(const svgp_pearce_bufs*, const double* eps_x, const double* eps_y, const double* state,
                       void* stream);
int svgp_pearce_gp_bwd(const svgp_pearce_bufs*, double seed_lh_scale, int accumulate, const double* state,
                       double* d_ls_x, double* d_ls_y, void* stream);
int svgp_pearce_elbo_assemble(int B, int T, const double* lh, const double* ce, const double* con_lh,
                              const double* row_recon, const double* row_ce, const double* tmask, const double* state,
                              double* out, void* stream);
int svgp_scale_rows(long long rows, int C, const double* w, double* x, void* stream);

/* ---- the same exact per-video GP with every n x n matrix in global memory (pearce_long.hip): 1 <= n <= T <= 2048 -------
 * Same svgp_pearce_bufs, same (T, B) frame-major per-frame buffers, same meaning of idx / tmask / seed_lh_scale /
 * accumulate, same randomness (eps_x / eps_y, or both NULL: Philox on state[SVGP_ST_RNG_CTR], counter (t B + b) 2 + c) and
 * the same results as svgp_pearce_gp_fwd/bwd up to rounding; svgp_pearce_elbo_assemble takes their lh / ce / row_ce.
 * Forward: A = K + diag(s2) built into bufs->Ai, svgp_spd_inverse_batched in place, then one pass over Ai:
 *   alpha = Ai y,  p_m = y - s2 alpha,  p_v = s2 - s2^2 diag(Ai),  lhood = -1/2 (n log 2pi + y.alpha + log det A).
 * Reverse: one pass over Ai -> ybar, s2bar.  want_dls != 0 additionally forms Ai D Ai with one svgp_dgemm_batched and
 *   d_ls_x / d_ls_y (+ bufs->dl_part (2,B)); want_dls == 0 leaves d_ls_x / d_ls_y / dl_part untouched (they may be NULL).
 *   A context set (idx != NULL) needs no product: its d_ls is always formed, whatever want_dls says.
 * work: svgp_pearce_long_workspace_elems(B, T, n, want_dls) doubles (0 for a shape the entry points refuse); scratch only,
 *   nothing in it is carried from one call to the next, so the full set and the context sets of a step may share the one
 *   sized for n = T -- provided the calls are ordered on one stream.  bufs->Ai, alpha, lh (and p_m, p_v, eps of the full
 *   set) written by the forward call are what the reverse call of the same set reads.
 * Refused with a message before any launch: NULL pointers, n < 1, n > T, T > 2048 (SVGP_ERR_UNSUPPORTED), B < 1, n != T
 * without idx.  Explicit stream, no allocation, no host synchronisation, capturable; no float atomics (bitwise
 * reproducible).                                                                                                          */
size_t svgp_pearce_long_workspace_elems(int B, int T, int n, int want_dls);
int svgp_pearce_long_fwd(const svgp_pearce_bufs*, const double* eps_x, const double* eps_y, const double* state,
                         double* work, void* stream);
int svgp_pearce_long_bwd(const svgp_pearce_bufs*, double seed_lh_scale, int accumulate, int want_dls, const double* state,
                         double* d_ls_x, double* d_ls_y, double* work, void* stream);

/* ---- moving-ball SVGP-VAE with more than 64 inducing points or more than 64 videos (ball_large.hip, gp_large.hip) ----------
 * BALL_experiment.py --elbo SVGPVAE_Hensman | SVGPVAE_Titsias beyond what the shared stage entry points accept with kl_form = 1
 * (m <= 64, at most 64 channels: those refusals stand).  Same mapping as above -- rows = the T frames, channels = the B videos,
 * N_train = T, one workspace per latent coordinate -- on the global-memory stages: (B, m, m) blocks, every m^3 contraction on
 * the float64 MFMA GEMM, blocked inverses.  ALL B videos are channels of one workspace (no chunks), so the batch-wide scalar of
 * the reference's KL (:135-137), the 1/B of the loss seed and the Philox counters (t B + b of coordinate c, state[SVGP_ST_RNG_CTR]
 * advanced by one between the coordinates) are those of the whole batch, and the results equal those of the m <= 64 path up to
 * rounding where both accept a shape.  The entry points take 1 <= m <= 2048 -- m <= 64 included, ON THE LARGE-M KERNELS: there is
 * no hand-over to the LDS stages inside the library; ball.sparse_engine_class picks the engine --, 1 <= B <=
 * SVGP_BALL_LARGE_MAX_VIDEOS, 1 <= T <= 16384, kl_form = 1, clip_pv = 2.  The struct carries no rank fields: the moving-ball KL
 * couples all videos of the batch, which is never sharded over ranks.
 *   svgp_ball_large_ws_layout_get: the workspace layout (svgp_mnist_ws_layout; the fields of the MNIST networks are empty, M2 /
 *     Qm absent as in every large-m workspace).  The caller writes ws.qnet_mu / qnet_var_raw / qnet_var (svgp_ball_head_fwd) and
 *     ws.zbar (svgp_ball_unpack_zbar) and reads ws.z, p_m, p_v, Si, ybar, s2bar.
 *   svgp_ball_large_workspace_elems: doubles of one workspace; 0 for a configuration the entry points refuse.
 *   svgp_ball_large_gp_fwd: one coordinate forward -- kernel matrices of (times, ip, *ls) -> statistics -> (Titsias statistics)
 *     -> factor stage incl. KL_l = 1/2 (log det terms - m + tr(Ki A_l) + B tr(Ki A_l A_l)) and tr(Ki A_l A_l) behind it in ws.KL
 *     -> row stage (eps (T, B), or NULL: Philox) -> (Titsias terms).
 *   svgp_ball_large_gp_bwd: the reverse of that call on the same workspace, from ws.zbar and the loss seeds in `state` down to
 *     ws.ybar, ws.s2bar, d_ip (m), d_ls (1).
 *   svgp_ball_large_elbo_assemble: svgp_ball_elbo_assemble on two such workspaces, out (7, B).
 * Explicit stream, no allocation, no host synchronisation, no float atomics (a repeated step is bitwise identical).  Refused with
 * a message before any launch: NULL cfg / pointers, m > 2048, B > SVGP_BALL_LARGE_MAX_VIDEOS (SVGP_ERR_UNSUPPORTED), kl_form != 1,
 * clip_pv != 2, non-positive sizes.                                                                                        */
#define SVGP_BALL_LARGE_MAX_VIDEOS 256
typedef struct {
    int32_t T, B, m;                  /* frames per video, videos per batch, inducing points */
    int32_t titsias, kl_form, clip_pv;
    double jitter;
} svgp_ball_large_cfg;
int svgp_ball_large_ws_layout_get(const svgp_ball_large_cfg* cfg, svgp_mnist_ws_layout* out);
long long svgp_ball_large_workspace_elems(const svgp_ball_large_cfg* cfg);
int svgp_ball_large_gp_fwd(const svgp_ball_large_cfg* cfg, const double* times, const double* ip, const double* ls,
                           const double* eps, double* ws, double* state, void* stream);
int svgp_ball_large_gp_bwd(const svgp_ball_large_cfg* cfg, const double* times, const double* ip, const double* ls, double* ws,
                           const double* state, double* d_ip, double* d_ls, void* stream);
int svgp_ball_large_elbo_assemble(const svgp_ball_large_cfg* cfg, const double* ws_x, const double* ws_y,
                                  const double* row_recon, const double* state, double* out, void* stream);

/* ---- deep SVIGP_Hensman baseline on rotated MNIST (svigp.hip): MNIST_experiment.py --elbo SVIGP_Hensman -------------
 * SVIGP_Hensman.variational_loss / approximate_posterior_params (SVIGP_Hensman_model.py:135-227) and the ELBO assembly
 * of forward_pass_deep_SVIGP_Hensman (:230-289) with free variational parameters loc (L,m), scale (L,m,m)
 * (S_l = scale_l scale_l^T) and a likelihood noise (1); kernel matrices from svgp_kernel_matrix_fwd, decoder =
 * svgp_mnist_decoder_fwd/bwd.  svgp_svigp_fwd: Z (b,L) = K_nm (K_mm + jI)^-1 loc_l (training mean vectors, and with
 * test-point kernel matrices the prediction of :292-339).  svgp_svigp_bwd: reverse pass of -elbo given the decoder's
 * Zbar (beta-ELBO seed, scaled here by n_pix / (2 noise^2)) and its squared-error partial sums; writes Kbar / Knbar /
 * knnbar for svgp_kernel_matrix_bwd and the gradients of loc, scale, noise.  svgp_svigp_assemble: out (7) = [elbo,
 * recon_loss / n_pix, KL_term, inside_elbo, 0, inside_recon, inside_kl].  ws: svgp_svigp_workspace_elems doubles;
 * ws[svgp_svigp_scale_offset] holds n_pix / (2 noise^2), the factor the decoder's weight gradients take
 * (svgp_scale_by_device_scalar).                                                                                    */
long long svgp_svigp_workspace_elems(int b, int m, int L);
long long svgp_svigp_scale_offset(int b, int m, int L);
int svgp_svigp_fwd(int b, int b_global, int m, int L, int n_pix, double jitter, const double* K, const double* Kn,
                   const double* knn, const double* loc, const double* scale, const double* noise, double* Z,
                   double* ws, void* stream);
int svgp_svigp_bwd(int b, int b_global, int m, int L, int n_pix, double N_train, const double* Kn, const double* loc,
                   const double* scale, const double* noise, double* Zbar, const double* part_sums, int n_part,
                   double* Kbar, double* Knbar, double* knnbar, double* d_loc, double* d_scale, double* d_noise,
                   double* ws, void* stream);
int svgp_svigp_assemble(int b, int b_global, int m, int L, int n_pix, double N_train, const double* noise,
                        const double* part_sums, int n_part, const double* ws, double* out, void* stream);
int svgp_scale_by_device_scalar(long long n, const double* f, double* x, void* stream);

/* ---- Casale GP-VAE baseline on rotated MNIST (casale.hip): MNIST_experiment.py --elbo GPVAE_Casale ---------------------
 * casaleGP.V_matrix / taylor_coeff (GPVAE_Casale_model.py:278-351) and the GP prior term of forward_pass_Casale (:134-142)
 * in H x H space, H = M Q.  The reference forms K_inv = (I - V (alpha I + V^T V)^-1 V^T) / alpha (N x N) and the Taylor
 * coefficients a (L,N), B (L,N,H), c (L); with K_inv V = V P and V^T A = U the same number is
 *   G = V^T V   P = (alpha I + G)^-1   W = V^T Z   U = P W   A = (Z - V U) / alpha            (A^T = a)
 *   GP_prior_term = sum(zb * A[idx]) - sum(A[idx] * (V[idx] U)) + L sum((V[idx] P) * V[idx])
 *                   + alpha/2 (-||A||_F^2 + L ((N - H) / alpha + tr P))
 * for the batch rows idx = [lo, hi) of the sorted train set, Z (N,L) the latent sample of all rows and zb (hi-lo, L) the
 * batch's own.  V[i, k Q + r] = ov[obj_idx[i], k] L_W[ang_idx[i], r] (ov row-normalised with cfg.normalize_obj), L_W the
 * Cholesky factor of K_W = ExpSinSquared(amplitude, l_GP, 2 pi) on the Q sorted unique train angles, no jitter (:301-302).
 * Rows are sorted by object: obj_idx is non-decreasing.  gp = [l_GP, amplitude, alpha, object_vectors (n_obj, M)], the
 * suffix of theta (svgp_casale_layout: th_l_GP).
 *   svgp_casale_v_fwd  : K_W, L_W (one workgroup) and V
 *   svgp_casale_gp_fwd : svgp_casale_v_fwd, then G, W (svgp_dgemm_splitk), P (svgp_spd_inverse_batched), U,
 *                        V[idx] P (svgp_dgemm_batched), one row kernel (V U, A and the row partials of the four sums) and
 *                        the scalar epilogue -> ws[terms] = [sum zb A, -sum A (V U), L sum (V P) V, ||A||^2, tr P, tr K_inv,
 *                        sum(c), GP_prior_term]
 *   svgp_casale_gp_bwd : reverse pass of seed * GP_prior_term: Zbar (N,L), zbbar (hi-lo,L), Vbar, the deterministic VJP of
 *                        the V build into ovbar (n_obj,M) and L_W (row-chunk partials, fixed order, no float atomics), the
 *                        Cholesky VJP Phi(L^T Lbar) with two triangular solves and the kernel VJP (one workgroup)
 *                        -> ws[grad_gp] = [l_GP, amplitude, alpha | object_vectors]; zero where cfg.train_gp / train_ov is 0
 *   svgp_casale_sample / _seeds : the two samples of a step from ONE encoder pass over all N rows (encode, :86-91: clip
 *                        [1e-3, 10]; forward_pass_Casale, :123-131: clip [1e-3, 100], log_var) and the combined seed w.r.t.
 *                        (mu, var_raw) of all N rows for svgp_mnist_encoder_bwd with cfg.clip_qs = 0
 *   svgp_casale_vae_sample / _vae_seeds : the plain-VAE objective of the `VAE` regime (SVGPVAE_model.py:718-782), batch rows
 *   svgp_casale_finalize : out (8) = [elbo, recon_loss, GP_prior_term, log_var, KL_term, 0, 0, 0] (:150-153); mode 1: the
 *                        plain-VAE scalars [elbo_VAE, recon_loss, 0, 0, KL_term] with the decoder's sigma_vae (mode 0 ignores
 *                        it); state[ADAM_T] += did_adam
 *   svgp_casale_predict_var : predict_test_set_Casale (:158-203): mean = K_*n A is one GEMM; var_i = k_ii - (|k_i|^2 -
 *                        r_i . (P r_i)) / alpha from K_*n (T,N), R = K_*n V and RP = R P (T,H each), one wave per test row;
 *                        the caller spreads var over the channels as the reference does (:194, sic: var[(i L + l) mod T])
 *   svgp_scale_f64     : x *= f
 * Refused: Q > 32, H > 2048, M > 128, L > 64 (SVGP_ERR_UNSUPPORTED); a batch range outside [0, N], NULL pointers
 * (SVGP_ERR_INVALID).  Plain launches on `stream`. */
typedef struct {
    int32_t N;             /* train rows                                                                    */
    int32_t n_obj;         /* rows of the object_vectors table                                              */
    int32_t Q;             /* unique train angles                                                           */
    int32_t M;             /* object-vector dimension; H = M Q                                              */
    int32_t L;             /* latent channels                                                               */
    int32_t b_cap;         /* largest batch (rows of the batch-sized fields)                                */
    int32_t normalize_obj; /* object_kernel_normalize                                                       */
    int32_t train_gp;      /* 0: l_GP, amplitude, alpha fixed (fixed_gp_params)                             */
    int32_t train_ov;      /* 1: object_vectors trainable (--ov_joint)                                      */
} svgp_casale_cfg;
/* theta offsets (encoder, decoder, l_GP, amplitude, alpha, object_vectors: the reference's creation order) and workspace
 * offsets (float64 elements) of every intermediate */
typedef struct {
    int64_t th_l_GP, th_amplitude, th_alpha, th_ov, n_enc, n_vae, n_total;
    int64_t K_W, L_W;                     /* (Q,Q) each                                                     */
    int64_t V, G, P, W, U, VU, A, VPb;    /* (N,H) (H,H) (H,H) (H,L) (H,L) (N,L) (N,L) (b,H)                */
    int64_t Z, zb, qvar_b;                /* (N,L) (b,L) (b,L): the two samples, the batch's clipped variance */
    int64_t part, terms, lv_part, n_lv;   /* (N,4) row partials; (8); per-workgroup log_var / KL partials   */
    int64_t Abar, Cm, Zbar, zbbar, Vbar;  /* (N,L) (N,L) (N,L) (b,L) (N,H)                                  */
    int64_t Ubar, Pbar, Wbar, T, Mbar;    /* (H,L) (H,H) (H,L) (H,H) (H,H): Mbar holds Mbar + Mbar^T        */
    int64_t part_alpha, trM;              /* (N) row partials of alphabar; (1) tr Mbar                      */
    int64_t LWbar_part, n_chunk, LWbar, KWbar; /* (n_chunk,Q,Q) partials over row chunks; (Q,Q); (Q,Q)      */
    int64_t grad_gp;                      /* (3 + n_obj M) = [l_GP, amplitude, alpha | object_vectors]      */
    int64_t logdet, scr_inv, scr_splitk, scr_splitk_len;
    int64_t total;
} svgp_casale_layout;
int svgp_casale_layout_get(const svgp_casale_cfg*, svgp_casale_layout* out);
int svgp_casale_v_fwd(const svgp_casale_cfg*, const double* gp, const double* angles, const int32_t* obj_idx,
                      const int32_t* ang_idx, double* ws, void* stream);
int svgp_casale_gp_fwd(const svgp_casale_cfg*, const double* gp, const double* angles, const int32_t* obj_idx,
                       const int32_t* ang_idx, const double* Z, const double* zb, int lo, int hi, double* ws, void* stream);
int svgp_casale_gp_bwd(const svgp_casale_cfg*, const double* gp, const double* angles, const int32_t* obj_idx,
                       const int32_t* ang_idx, const double* Z, const double* zb, int lo, int hi, double seed, double* ws,
                       void* stream);
int svgp_casale_sample(const svgp_casale_cfg*, int clip, int lo, int hi, const double* mu, const double* var_raw,
                       const double* eps_full, const double* eps_batch, double* z_dec, double* ws, void* stream);
int svgp_casale_seeds(const svgp_casale_cfg*, int clip, int lo, int hi, const double* var_raw, const double* eps_full,
                      const double* eps_batch, const double* dec_zbar, double c_logvar, double* ybar, double* s2bar,
                      double* ws, void* stream);
int svgp_casale_vae_sample(const svgp_casale_cfg*, int b, const double* mu, const double* var_raw, const double* eps,
                           double* z_dec, double* ws, void* stream);
int svgp_casale_vae_seeds(const svgp_casale_cfg*, int b, double scale, const double* mu, const double* var_raw,
                          const double* eps, const double* dec_zbar, double* ybar, double* s2bar, void* stream);
int svgp_casale_finalize(const svgp_casale_cfg*, int mode, int b, double beta, double sigma_vae, const double* dec_sums,
                         int did_adam, double* ws, double* out, double* state, void* stream);
int svgp_casale_predict_var(int T, int N, int H, const double* K_tn, const double* k_tt, const double* R, const double* RP,
                            const double* alpha, double* var, void* stream);
int svgp_scale_f64(long long n, double f, double* x, void* stream);

/* ---- Casale GP-VAE: posterior cache and conditional generation (casale_generate.hip) ----------------
 * predict_test_set_Casale (GPVAE_Casale_model.py:158-203) without the train set.  The posterior at a query row
 * x* = [id, angle, o*] depends on the train rows only through P = (alpha I + V^T V)^-1 (H,H) and U = P V^T Z (H,L) of the
 * block above, plus L_W (Q,Q).  With kappa_r = k_W(angle*, angle_r), lambda = L_W^-1 kappa (forward substitution) and
 * v*[k Q + r] = on*_k lambda_r (on* = o*, row-normalised with cfg.normalize_obj):  K_*n = v*^T V^T exactly, and
 *   mean* = v*^T U (L)      var* = k** - |v*|^2 + alpha v*^T P v*  (ONE scalar per row)      k** = amplitude^2 |on*|^2
 * which are K_*n K_inv Z and k** - k*^T K_inv k* of the reference.  z[i,l] = mean[i,l] + eps[i,l] sqrt(var[i]): row i's own
 * variance for all its channels -- NOT the reference's tiling var[(i L + l) mod T] (:194, sic), which is no function of the
 * query row; svgp_casale_predict_var's caller keeps that tiling.
 * The cache is ONE float64 array [angles (Q) | L_W (Q,Q) | U (H,L) | P (H,H)], each field on a 16-element boundary
 * (svgp_casale_cache_layout_get); P is stored as (P + P^T) / 2, symmetric bit for bit.
 *   svgp_casale_cache_build : from the latent rows Z (N,L) of the sorted train set: the front half of svgp_casale_gp_fwd
 *                        (svgp_casale_v_fwd, G, P, W, U on `ws`, the svgp_casale_layout workspace; no batch range, no row
 *                        kernel), then one kernel that writes the cache.  gp, angles, obj_idx, ang_idx as above.
 *   svgp_casale_generate : b query rows aux (b, 2+M) = [id, angle, o_1..o_M] -> images_out (b,28,28,1) = decode(z).  theta is
 *                        the flat parameter vector [encoder | decoder | l_GP, amplitude, alpha | object_vectors] (decoder at
 *                        n_enc, GP suffix at n_vae of svgp_casale_layout).  gather != 0: the object vector of a row is table row
 *                        (int)row[0] (a row whose id is outside [0, n_obj) gets NaN images and moments instead of a read
 *                        outside the table); gather == 0: the row's own columns 2:.  eps (b,L) may be NULL: z = mean.
 *                        mean_out (b,L) and var_out (b) may each be NULL.  H <= 256: exactly ONE launch for any b (kappa,
 *                        lambda, v*, both moments, the sample and the decoder per image in a workgroup that strides over the
 *                        images; decoder weights and L_W staged in LDS once).  256 < H <= 2048: per pass of 256 rows a row
 *                        kernel (v*, k**), svgp_dgemm_batched for v* P and v* U, a row-sum kernel, the decode launch.  Every
 *                        sum has a fixed order: a row gives the same bits wherever it stands in a batch of any size.
 *                        work: svgp_casale_generate_workspace_elems(cfg, b) doubles; 0 for H <= 256 (work may be NULL).
 *   svgp_casale_generate_route : the launches of one pass as text, one name per line in launch order, from the plan the call
 *                        itself walks; needs no device.
 * cfg: N, n_obj, Q, M, L, normalize_obj as for the block above (b_cap >= 1; train_gp / train_ov are not read).
 * Refused before any launch: svgp_casale_layout_get's refusals (Q > 32, H > 2048, M > 128, L > 64: SVGP_ERR_UNSUPPORTED);
 * NULL theta / cache / aux / images_out, b < 0, NULL work where the size is non-zero, gather with n_obj < 1
 * (SVGP_ERR_INVALID).  b = 0 returns SVGP_OK without a launch.  Plain launches on `stream`, no allocation, no
 * synchronisation. */
typedef struct {
    int64_t angles, L_W, U, P, total;
} svgp_casale_cache_layout;
int svgp_casale_cache_layout_get(const svgp_casale_cfg*, svgp_casale_cache_layout* out);
int svgp_casale_cache_build(const svgp_casale_cfg*, const double* gp, const double* angles, const int32_t* obj_idx,
                            const int32_t* ang_idx, const double* Z, double* ws, double* cache, void* stream);
long long svgp_casale_generate_workspace_elems(const svgp_casale_cfg*, long long b);
int svgp_casale_generate(const svgp_casale_cfg*, long long b, const double* theta, const double* cache, const double* aux,
                         int gather, const double* eps, double* images_out, double* mean_out, double* var_out, double* work,
                         void* stream);
int svgp_casale_generate_route(const svgp_casale_cfg*, char* buf, int cap);

/* ---- bias analysis of the inducing mean vector (bias.hip): MNIST_experiment.py --bias_analysis, supplement C.4 ----------
 * The mean vector of channel l, c K_mm (Sigma_l + jI)^-1 K_mb (y_l / noise_l) with c = N_train / b (SVGPVAE_model.py:345-370),
 * is ws[mu_hat] (L, m) of every step.  The reference appends it to a host list every step and averages the list at the end
 * of the epoch (MNIST_experiment.py:325-363, utils.py:922-948); here the sum stays on the device.
 * svgp_mean_vectors_accumulate: acc (L m + 1) doubles, zeroed by the caller at the start of the epoch:
 *   acc[i] += mu_hat[i] for i < L m, acc[L m] += 1 (the number of accumulated steps).  One thread per element, no atomics:
 *   after k calls acc[:L m] is the left-to-right float64 sum of the k inputs, bit for bit (the reference's `+=` order).
 * svgp_mean_vectors_bias: out (1 + L) doubles from acc and the whole-train-set vectors full (L, m), B = acc[L m]:
 *   out[1 + l] = sum_j |acc[l][j] / B - full[l][j]|   (a true division, utils.py:944-946)
 *   out[0]     = (sum_l out[1 + l]) / L               (np.mean, :948)
 *   One launch of one workgroup with a fixed summation order: the same bits on every run.  B = 0 gives NaN / infinity
 *   through the arithmetic; nothing traps.
 * Both: L < 1, m < 1 or a NULL pointer -> SVGP_ERR_INVALID, m > 2048 -> SVGP_ERR_UNSUPPORTED, before any launch.         */
int svgp_mean_vectors_accumulate(int L, int m, const double* mu_hat, double* acc, void* stream);
int svgp_mean_vectors_bias(int L, int m, const double* acc, const double* full, double* out, void* stream);

/* ---- cubic-spline image rotation (rotate.hip): the rotated-MNIST data set generator, utils.py:507-657 --------------------
 * svgp_rotate_cubic_f64: out[k][a] (H, W) = images[k] (H, W) rotated by the angle whose cosine and sine are cos_sin[a] =
 *   (c, s), as scipy.ndimage.rotate(image, angle, reshape=False) does with its defaults (order 3, mode 'constant', cval 0,
 *   prefilter on): the image is turned into cubic B-spline coefficients (pole sqrt(3) - 2, mirror boundary, axis 0 then
 *   axis 1), output pixel (i, j) reads the input at (off0 + c i + s j, off1 - s i + c j), off = cen - [[c, s], [-s, c]] cen,
 *   cen = ((H - 1) / 2, (W - 1) / 2), is 0 when a coordinate is below 0 or above H - 1 / W - 1, and otherwise the 4 x 4 sum
 *   of coefficients (taps mirrored with period 2 (len - 1)) times the two cubic weights.  The coordinate products and sums
 *   are rounded one by one (no fused multiply-add), so a pixel is inside here exactly when it is inside on the CPU; pass the
 *   cosines and sines of scipy.special.cosdg / sindg to get the quarter turns exact, as scipy's rotate does.
 *   images (n, H, W), cos_sin (A, 2), out (n, A, H, W), float64 device arrays.  One workgroup per image (the coefficients
 *   live in LDS and are computed once for all A angles); no allocation, no synchronisation, capturable.
 *   2 <= H, W <= 64 (else SVGP_ERR_UNSUPPORTED); n < 0, A < 1 or a NULL pointer -> SVGP_ERR_INVALID; all before any launch.
 *   n = 0 returns SVGP_OK and launches nothing.                                                                            */
int svgp_rotate_cubic_f64(int n, int H, int W, int A, const double* images, const double* cos_sin, double* out, void* stream);

/* ---- posterior cache and conditional generation (generate.hip) --------------------------------------
 * The GP posterior of mainSVGP.approximate_posterior_params (SVGPVAE_model.py:303-343) depends on the train set only through
 *   Sigma_l = K_mm + c S_l,  S_l = K_mn diag(1/var_l) K_nm,  v_l = K_mn (mu_l / var_l),  c = N_train / rows
 *   w_l = c (Sigma_l + jI)^-1 v_l   (L, m)          X_l = (Sigma_l + jI)^-1 - (K_mm + jI)^-1   (L, m, m)
 *   p_m[x,l] = k_x . w_l            p_v[x,l] = k_xx + k_x^T X_l k_x            k_x = K(x, inducing points)
 * so [w | X] is accumulated once over the train set in row chunks (no N-row workspace) and a query needs no train row.
 * The cache is ONE float64 array; svgp_mnist_cache_layout_get gives its offsets in elements (each field on a 16-element
 * boundary, as the workspace's): acc_S (L,m,m) and acc_v (L,m) the raw sums over the accumulated rows (the factor c is NOT in
 * them), acc_rows (1) their row count, then w and X.  m, L, M, n_obj, normalize_obj, jitter and N_train come from the cfg.
 *
 * svgp_gp_stats_accumulate: behind svgp_gp_stats_fwd on the same workspace and cfg (cfg->b rows): acc_S / acc_v += the
 *   statistics in ws.statA (m <= 64: the P row partials of a channel are added in index order first, as the consumers do on
 *   load), acc_rows += b; first != 0 overwrites instead.  One thread per element, no atomics: after k calls the value is the
 *   left-to-right float64 sum over the chunks.
 * svgp_mnist_cache_build: K_mm from theta, c = cfg->N_train / acc_rows read ON THE DEVICE, the two jittered inverses (m <= 64:
 *   one launch, the LDS sweep of the factor stage; beyond: svgp_spd_inverse_batched on the (L + 1) matrices), then w and X;
 *   X is written exactly symmetric ((D + D^T) / 2 of D = Sigma^-1 - K^-1).  work: svgp_mnist_cache_workspace_elems(cfg)
 *   doubles (0 for m <= 64: work may then be NULL).
 * svgp_mnist_generate: cfg->b query rows aux (b, 2+M) = [id, angle, o_1..o_M] -> images_out (b,28,28,1) = decode(z),
 *   z = p_m + eps sqrt(p_v); eps (b, L) may be NULL: z = p_m (no device generator, `state` is not an argument).  gather != 0:
 *   the object vector of a row is table[(int)row[0]] (needs n_obj > 0; a row whose id is outside [0, n_obj) gets NaN images
 *   and moments instead of an out-of-range read), gather == 0: the row's own columns 2:.  p_m_out / p_v_out (b, L) may each be
 *   NULL.  No image input, no loss.  m <= 64: exactly ONE launch for any b (kernel row, moments, sample and decoder per image in a
 *   workgroup that strides over the images; X is read through L2); 64 < m <= 2048: k_x by a bounds-checked kernel with the
 *   arithmetic of svgp_kernel_matrix_xy, K_x X_l and K_x w^T by svgp_dgemm_batched into `work`, a row-sum kernel, then the same
 *   generation kernel with z given.  The out-of-table rule above holds on both routes.  work:
 *   svgp_mnist_generate_workspace_elems(cfg) doubles, sized for max(cfg->b, cfg->b_cap) rows; 0 for m <= 64 (work may be NULL).
 * svgp_mnist_generate_route: the kernels of one svgp_mnist_generate call as text, one name per line in launch order, from the
 *   plan the call itself executes; needs no device.
 * All: svgp_check_cfg's refusals (m > 2048, L > 64, M > 128 -> SVGP_ERR_UNSUPPORTED), then NULL pointers, b < 1, gather with
 *   n_obj = 0, NULL work where the size is non-zero -> SVGP_ERR_INVALID; every refusal before any pointer is looked at and
 *   before any launch.  Explicit stream, no allocation, no synchronisation, capturable.                                     */
typedef struct {
    int64_t acc_S, acc_v, acc_rows, w, X, total;
} svgp_mnist_cache_layout;
int svgp_mnist_cache_layout_get(const svgp_mnist_cfg* cfg, svgp_mnist_cache_layout* out);
int svgp_gp_stats_accumulate(const svgp_mnist_cfg* cfg, const double* ws, double* cache, int first, void* stream);
long long svgp_mnist_cache_workspace_elems(const svgp_mnist_cfg* cfg);
int svgp_mnist_cache_build(const svgp_mnist_cfg* cfg, const double* theta, double* cache, double* work, void* stream);
long long svgp_mnist_generate_workspace_elems(const svgp_mnist_cfg* cfg);
int svgp_mnist_generate(const svgp_mnist_cfg* cfg, const double* theta, const double* cache, const double* aux, int gather,
                        const double* eps, double* images_out, double* p_m_out, double* p_v_out, double* work, void* stream);
int svgp_mnist_generate_route(const svgp_mnist_cfg* cfg, char* buf, int cap);

/* ---- SPRITES: latent rows of a new character from a posterior cache (sprites_generate.hip) ---------
 * The GP posterior of spritesSVGP.approximate_posterior_params_precomputed_GP_posterior_params (SVGPVAE_model.py:610-635)
 * depends on the train set only through  w_l = Sigma_l^-1 K_mn (mu_l / var_l)  (L, m)  and  X_l = Sigma_l^-1 - K_mm^-1
 * (L, m, m).  For the cfg->b query rows with kernel rows Kb (b, m) and prior variances kbb (b), per row i and channel l:
 *   p_m[i,l] = Kb[i,:] . w_l      p_v[i,l] = clamp(kbb[i] + Kb[i,:] X_l Kb[i,:]^T, clip_lo, clip_hi)
 *   z[i,l]   = p_m + eps[i,l] sqrt(p_v);  eps NULL: z = p_m (the decode of the posterior mean);  z NULL: not written.
 * A workgroup owns 64 rows of one channel, walks column tiles of Kb X_l on the f64 MFMA, multiplies each accumulator tile by the
 * matching Kb tile and keeps the row sums in registers: no buffer grows with b m.  m <= 256: ONE launch over all column tiles, no
 * workspace (work may be NULL).  m > 256: the column tiles of a (row block, channel) are dealt to S <= 16 workgroups (about 1024
 * workgroups in all; S = 1 where rows x channels alone give that many), each writes its partial row sums to work (S, b, L) and a
 * second launch adds the S partials of an element in index order, clamps and draws; ..._workspace_elems returns S b L (0 for
 * S = 1), at most 16 b L.  Of the outputs only their b L elements are written.  X is NOT assumed symmetric.  No atomics, fixed
 * summation order: the same inputs give the same bits.  A NaN in p_v stays a NaN through the clamp (torch.clamp).
 * ..._route: the kernels of one call as text, one name per line in launch order, from the same plan; needs no device.
 * Accepted: 1 <= m <= 2048, 1 <= L <= 64, b >= 1, clip_lo <= clip_hi.  Outside that, a NULL cfg, a NULL Kb / kbb / w / X /
 * p_m / p_v, or a NULL work where the size is non-zero: SVGP_ERR_INVALID with a message, before any launch.  Explicit stream,
 * no allocation, no synchronisation.                                                                                          */
typedef struct {
    int32_t b, m, L;
    double clip_lo, clip_hi;
} svgp_posterior_rows_cfg;
long long svgp_sprites_posterior_rows_workspace_elems(const svgp_posterior_rows_cfg* cfg);
int svgp_sprites_posterior_rows(const svgp_posterior_rows_cfg* cfg, const double* Kb, const double* kbb, const double* w,
                                const double* X, const double* eps, double* p_m, double* p_v, double* z, double* work,
                                void* stream);
int svgp_sprites_posterior_rows_route(const svgp_posterior_rows_cfg* cfg, char* buf, int cap);

/* ---- moving ball: fill dropped frames, resample in time (ball_predict.hip) --------------------------
 * The sparse-GP posterior of SVGP.approximate_posterior_params (SVGPVAE_model.py:142-171) at arbitrary query times tq (Q) -- any
 * reals, unsorted, inside or outside the frame times -- from the frames a mask keeps.  Per video b and latent coordinate, with
 * SE(a, b) = exp(-(a - b)^2 / (2 ls^2)), p = mask * reciprocal_no_nan(var) (a dropped frame has precision 0; where p = 0 the
 * product p mu counts as 0), K = SE(ip, ip), Kn = SE(times, ip), k = SE(tq, ip):
 *   Sig = K + Kn^T diag(p) Kn    Si = (Sig + jitter I)^-1    Ki = (K + jitter I)^-1    w = Si Kn^T (p mu)    X = Si - Ki
 *   p_m = k w      p_v = 1 + diag(k X k^T)  (reported unclamped)      z = p_m + eps sqrt(clamp(p_v, clip_lo, clip_hi))  (:701)
 * mu, var and mask are (T, B), the frame-major layout svgp_ball_head_fwd writes; mask (values 0 / 1) is shared by the two
 * coordinates, NULL = all ones.  eps and the outputs p_m, p_v, z are (Q, B) per coordinate.  eps NULL: z = p_m; z NULL: not written.
 * A video with every frame dropped gives the prior, p_m = 0 and p_v = 1.
 * svgp_ball_predict: 1 <= m <= 64, 1 <= T <= 16384, B, Q >= 1.  ONE launch, a workgroup per (video, coordinate): K in LDS, the
 *   frames streamed in order (no (T, m) matrix), both inverses by the same LDS sweep (X = 0 exactly for the all-dropped video), then
 *   the query times.  No workspace, no atomics, fixed summation order: the same inputs give the same bits, and a query time's
 *   outputs do not depend on its position in tq.
 * svgp_ball_predict_large: 1 <= m <= 2048, 1 <= T <= 2048: the same results up to rounding from svgp_se1d_kernel_matrix_fwd, a
 *   row-scaling kernel + svgp_dgemm_batched (Sig_b, Kn^T (p mu)), svgp_spd_inverse_batched on the Sig_b + jitter I of a chunk and on
 *   K + jitter I, a batched product (w), a subtraction (X) and svgp_sprites_posterior_rows with the videos of the chunk as channels
 *   (kbb = 1).  The videos are walked in chunks of 64 (one rows call each) and the query rows in chunks of 4096; work holds
 *   svgp_ball_predict_large_workspace_elems(cfg) doubles (0 for a refused cfg), which grows with neither B beyond 64 nor Q beyond
 *   4096.  The rows kernel gets an unbounded clip range and draws nothing: the clamp applies to the sample only and is taken by
 *   this entry's closing kernel.
 * svgp_ball_predict_route: the kernels (library entry points for the shared pieces) of one call as text, one name per line in
 *   launch order, from the same plan as the launch code; needs no device.  SVGP_ERR_INVALID when cap bytes do not hold the text.
 * Refused with a message before any launch: a NULL cfg / bufs / pointer (mask, eps_x/y and z_x/y excepted), B, T, m or Q < 1,
 *   clip_lo > clip_hi, NULL work (SVGP_ERR_INVALID); m or T beyond the entry's range (SVGP_ERR_UNSUPPORTED).
 * Explicit stream, no allocation, no synchronisation.                                                                          */
typedef struct {
    int32_t B, T, m, Q;
    double jitter, clip_lo, clip_hi;
} svgp_ball_predict_cfg;
typedef struct {
    const double *times, *tq;                 /* (T), (Q) */
    const double *ip_x, *ip_y;                /* (m) */
    const double *ls_x, *ls_y;                /* scalars */
    const double *mu_x, *mu_y, *var_x, *var_y;/* (T, B) */
    const double *mask;                       /* (T, B) or NULL */
    const double *eps_x, *eps_y;              /* (Q, B) or NULL */
    double *p_m_x, *p_m_y, *p_v_x, *p_v_y;    /* (Q, B) */
    double *z_x, *z_y;                        /* (Q, B) or NULL */
} svgp_ball_predict_bufs;
int svgp_ball_predict(const svgp_ball_predict_cfg* cfg, const svgp_ball_predict_bufs* bufs, void* stream);
long long svgp_ball_predict_large_workspace_elems(const svgp_ball_predict_cfg* cfg);
int svgp_ball_predict_large(const svgp_ball_predict_cfg* cfg, const svgp_ball_predict_bufs* bufs, double* work, void* stream);
int svgp_ball_predict_route(const svgp_ball_predict_cfg* cfg, int large, char* buf, int cap);

/* ---- moving ball, exact-GP baselines: fill dropped frames, resample in time (pearce_predict.hip) ------
 * build_1d_gp(X, Y, varY, X_test) (GPVAE_Pearce_model.py:8-86) with a general X_test: the exact per-video GP posterior at
 * arbitrary query times tq (Q) -- any finite reals, unsorted -- from the frames a mask keeps.  Per video b and latent coordinate c,
 * with SE(s, t) = exp(-(s - t)^2 / (2 ls_c^2)) and O the kept frames of the video (mask != 0, n of them; mask NULL keeps all):
 *   A = SE(t_O, t_O) + diag(var_O)  (no jitter, as in the reference)    alpha = A^-1 mu_O
 *   lh = -1/2 (n log 2pi + mu_O . alpha + log det A)                    k = SE(tq, t_O)
 *   p_m = k . alpha      p_v = 1 - k^T A^-1 k  (reported as computed)   z = p_m + eps sqrt(max(p_v, 0))
 * The reference takes sqrt(p_v) unguarded; the max(., 0) is this library's and applies to the sample only.  A dropped frame is
 * absent: its mu / var are never read (a NaN there reaches no output).  A video with every frame dropped gives the prior,
 * p_m = 0, p_v = 1, lh = 0.  mu, var and mask are (T, B), the frame-major layout svgp_ball_head_fwd writes; mask is shared by the
 * two coordinates.  eps and the outputs p_m, p_v, z are (Q, B) per coordinate, lh is (2, B).  eps NULL: z = p_m; z / lh NULL: not
 * written.
 * svgp_pearce_predict: 1 <= T <= 64, B, Q >= 1.  ONE launch, grid (B, 2, S): a workgroup compacts the kept frames of its video,
 *   builds A in LDS, inverts it in place (the LDS sweep of the training kernels, which also gives log det), forms alpha and serves
 *   its slice of the query times, a wave per query.  S query slices let a call with few videos and many query times fill the
 *   device; every slice repeats the inverse.  q_slices = 0: the launch plan chooses S (about 512 workgroups, at least four
 *   queries a slice); q_slices > 0 forces S.  No workspace, no atomics, fixed summation order: the same inputs give the same bits,
 *   and a query time's outputs depend neither on its position in tq nor on S.
 * svgp_pearce_predict_long: 1 <= T <= 2048: the same results up to rounding from global-memory pieces, both coordinates of 8
 *   videos per chunk: a kernel builds the masked full-size A (rows / columns of dropped frames are those of the identity: log det
 *   and the inverse of the kept block are unaffected), svgp_spd_inverse_batched inverts it in place, a row pass forms alpha, a
 *   reduction lh (not launched when lh is NULL); per chunk of 512 query rows a kernel forms the masked k, svgp_dgemm_batched
 *   k^T A^-1, and a closing kernel the row dot products and z.  work holds svgp_pearce_predict_long_workspace_elems(cfg) doubles
 *   (0 for a refused cfg), which grows with neither B beyond 8 nor Q beyond 512.  q_slices is checked and otherwise unused.
 * svgp_pearce_predict_route: the kernels (library entry points for the shared pieces) of one call as text, one name per line in
 *   launch order, from the same plan as the launch code; needs no device.  SVGP_ERR_INVALID when cap bytes do not hold the text.
 * Refused with a message before any launch: a NULL cfg / bufs / pointer (mask, eps_x/y, z_x/y and lh excepted), B, T or Q < 1,
 *   q_slices < 0 or > min(Q, 65535), NULL work (SVGP_ERR_INVALID); T beyond the entry's range (SVGP_ERR_UNSUPPORTED).
 * Explicit stream, no allocation, no synchronisation.                                                                          */
typedef struct {
    int32_t B, T, Q, q_slices;
} svgp_pearce_predict_cfg;
typedef struct {
    const double *times, *tq;                 /* (T), (Q) */
    const double *ls_x, *ls_y;                /* scalars */
    const double *mu_x, *mu_y, *var_x, *var_y;/* (T, B) */
    const double *mask;                       /* (T, B) or NULL */
    const double *eps_x, *eps_y;              /* (Q, B) or NULL */
    double *p_m_x, *p_m_y, *p_v_x, *p_v_y;    /* (Q, B) */
    double *z_x, *z_y;                        /* (Q, B) or NULL */
    double *lh;                               /* (2, B) or NULL */
} svgp_pearce_predict_bufs;
int svgp_pearce_predict(const svgp_pearce_predict_cfg* cfg, const svgp_pearce_predict_bufs* bufs, void* stream);
long long svgp_pearce_predict_long_workspace_elems(const svgp_pearce_predict_cfg* cfg);
int svgp_pearce_predict_long(const svgp_pearce_predict_cfg* cfg, const svgp_pearce_predict_bufs* bufs, double* work, void* stream);
int svgp_pearce_predict_route(const svgp_pearce_predict_cfg* cfg, int long_form, char* buf, int cap);

/* ---- moving ball: joint posterior over the query times, coherent sample paths (ball_predict_joint.hip) --
 * The full covariance of SVGP.approximate_posterior_params (SVGPVAE_model.py:141-171; the (batch, tmax, tmax) matrix B) at
 * arbitrary query times, and sample paths drawn with it.  With p, K, Kn, Sig, Si, Ki, w, X and k = SE(tq, ip) exactly those of
 * svgp_ball_predict above, per video b and latent coordinate:
 *   C   = SE(tq, tq) + k X k^T                 (Q x Q; diag C is svgp_ball_predict's p_v; nothing is clamped)
 *   Lc  = chol(C + path_jitter I)  lower       p_m = k w       z = p_m + Lc eps   (eps NULL: z = p_m)
 * Inputs as svgp_ball_predict's.  eps, p_m and z are (Q, B) per coordinate; cov and chol are (B, Q, Q) per coordinate, cov
 * symmetric bit for bit (one triangle is formed and mirrored), chol with its strict upper triangle zero.  eps, cov, chol and z may
 * each be NULL (not read / not written; without chol and without a draw no factor is taken).  A video with every frame dropped has
 * p_m = 0 exactly and cov = SE(tq, tq): paths from the prior.  A non-positive pivot gives NaN in that (video, coordinate)'s chol
 * and z only, the convention of svgp_potrf_batched: no error code, no host synchronisation.
 * svgp_ball_predict_joint: 1 <= m <= 64, 1 <= Q <= 64, 1 <= T <= 16384.  ONE launch, a workgroup per (video, coordinate), the
 *   Cholesky in LDS; no workspace, no atomics, fixed summation order: the same inputs give the same bits, and permuting tq
 *   permutes the rows and columns of cov bit for bit.
 * svgp_ball_predict_joint_large: m, T, Q <= 2048 (every shape of the fused entry included): per chunk of
 *   min(64, B, max(1, 2^22 / Q^2)) videos the steps of svgp_ball_predict_large up to X and w, svgp_se1d_kernel_matrix_fwd for k,
 *   svgp_dgemm_batched twice (k X, then (k X) k^T), a kernel that adds SE(tq, tq), mirrors the lower triangle, writes cov and adds
 *   path_jitter, svgp_potrf_batched (run with one step of iterative refinement on every panel solve, so that Lc Lc^T meets C +
 *   path_jitter I at the level of an unblocked factorisation for Q > 64 too), and a closing kernel (p_m, z, the copy of chol).  work holds
 *   svgp_ball_predict_joint_large_workspace_elems(cfg) doubles (0 for a refused cfg), which grows with neither B beyond a chunk nor
 *   its covariance block beyond 2^22 doubles.
 * svgp_ball_predict_joint_route: the kernels (library entry points for the shared pieces) of one call as text, one name per line
 *   in launch order, from the same plan as the launch code; needs no device.  SVGP_ERR_INVALID when cap bytes do not hold the text.
 * Refused with a message before any launch: a NULL cfg / bufs / pointer (mask, eps, cov, chol and z excepted), B, T, m or Q < 1,
 *   path_jitter < 0, NULL work (SVGP_ERR_INVALID); m, T or Q beyond the entry's range (SVGP_ERR_UNSUPPORTED).
 * Explicit stream, no allocation, no synchronisation.                                                                          */
typedef struct {
    int32_t B, T, m, Q;
    double jitter, path_jitter;
} svgp_ball_predict_joint_cfg;
typedef struct {
    const double *times, *tq;                 /* (T), (Q) */
    const double *ip_x, *ip_y;                /* (m) */
    const double *ls_x, *ls_y;                /* scalars */
    const double *mu_x, *mu_y, *var_x, *var_y;/* (T, B) */
    const double *mask;                       /* (T, B) or NULL */
    const double *eps_x, *eps_y;              /* (Q, B) or NULL */
    double *p_m_x, *p_m_y;                    /* (Q, B) */
    double *cov_x, *cov_y;                    /* (B, Q, Q) or NULL */
    double *chol_x, *chol_y;                  /* (B, Q, Q) or NULL */
    double *z_x, *z_y;                        /* (Q, B) or NULL */
} svgp_ball_predict_joint_bufs;
int svgp_ball_predict_joint(const svgp_ball_predict_joint_cfg* cfg, const svgp_ball_predict_joint_bufs* bufs, void* stream);
long long svgp_ball_predict_joint_large_workspace_elems(const svgp_ball_predict_joint_cfg* cfg);
int svgp_ball_predict_joint_large(const svgp_ball_predict_joint_cfg* cfg, const svgp_ball_predict_joint_bufs* bufs, double* work,
                                  void* stream);
int svgp_ball_predict_joint_route(const svgp_ball_predict_joint_cfg* cfg, int large, char* buf, int cap);

/* ---- moving ball: streamed posterior state, observe once and query often (ball_state.hip) -------------
 * The posterior of svgp_ball_predict / svgp_ball_predict_joint above with its state kept in device memory between calls.  It
 * depends on the frames only through two additive statistics per video b and latent coordinate c (0 = x, 1 = y),
 *   S = Kn^T diag(p) Kn  (m x m)        r = Kn^T (p mu)  (m)
 * with p, K, Kn, k of svgp_ball_predict.  Device state, both float64, part of this ABI:
 *   stats (B, 2, m m + m): per (b, c) the matrix S row-major, then r.  All zeros is "nothing observed", which is the prior; the
 *         caller zeroes it, there is no init entry.  Only svgp_ball_state_update writes it.
 *   post  (B, 2, m m + m): per (b, c) X = Si - Ki row-major, then w = Si r, with Si = ((K + S) + jitter I)^-1 and Ki = (K +
 *         jitter I)^-1.  Written by svgp_ball_state_finalize, read by the two queries.
 * Inducing points, length scales and jitter are not stored: pass the same ones to every entry.
 * svgp_ball_state_update:      stats += (S, r) of the T frames mu, var, mask (T, B) at times (T); mask NULL = all ones.  Any number
 *   of calls: no limit on the total number of frames.  Reads and writes stats only.
 * svgp_ball_state_finalize:    post from stats.  Zero stats give X = 0 and w = 0 exactly on the fused route.
 * svgp_ball_state_query:       p_m = k w, p_v = 1 + diag(k X k^T) (unclamped), z = p_m + eps sqrt(clamp(p_v, clip_lo, clip_hi)) at tq
 *   (Q), (Q, B) per coordinate, from post.  eps NULL: z = p_m; z NULL: not written.
 * svgp_ball_state_query_joint: p_m, cov, chol, z of svgp_ball_predict_joint_large from post, with its layouts, NULL rules (eps, cov,
 *   chol, z), NaN convention and refined factorisation; m, Q <= 2048, always from the library's global-memory pieces (cfg.large is
 *   not read): per chunk of min(64, B, max(1, 2^22 / Q^2)) videos a gather of w, svgp_se1d_kernel_matrix_fwd, svgp_dgemm_batched twice
 *   (X read in place from post), k_bpj_cov, svgp_potrf_batched (refined), k_bpj_finish.
 * cfg.large = 0, the fused routes, 1 <= m <= 64, ONE launch each, no workspace (work may be NULL), no atomics, fixed summation order:
 *   update (1 <= T <= 16384 a call): a workgroup per (video, coordinate) adds the frames in order with explicit fused multiply-adds to
 *     the elements it loaded from stats: feeding the frames in pieces gives the bits of one call, a frame with mask = 0 (whatever
 *     its mu holds) those of the call without it, an all-dropped call leaves stats unchanged.
 *   finalize: a workgroup per (video, coordinate), the LDS sweep of svgp_ball_predict on (K + S) + jitter I and K + jitter I.
 *   query: grid (B, 2, S): a workgroup loads X and w into LDS and serves its slice of the query times, 16 lanes per query.
 *     q_slices = 0: the library chooses S (about 512 workgroups, at least one round of 16 queries a slice); q_slices > 0 forces S, up
 *     to min(ceil(Q / 16), 65535).  A query's outputs depend neither on S nor on its position in tq.
 * cfg.large != 0, the large routes, 1 <= m <= 2048, on chunks of 64 videos with the steps of svgp_ball_predict_large:
 *   update (1 <= T <= 2048 a call): svgp_se1d_kernel_matrix_fwd, then per chunk k_bp_scale_rows and two svgp_dgemm_batched that
 *     accumulate into stats (beta = 1, the strides of the state layout).
 *   finalize: svgp_se1d_kernel_matrix_fwd (K), then per chunk k_bs_gather, k_bp_add_prior, svgp_spd_inverse_batched,
 *     svgp_dgemm_batched, k_bp_subtract, k_bs_scatter.
 *   query: per chunk k_bs_gather, then per 4096 query rows svgp_se1d_kernel_matrix_fwd, svgp_sprites_posterior_rows, k_bp_finish.
 * svgp_ball_state_workspace_elems(cfg, op): the doubles `work` holds for op (SVGP_BALL_STATE_*): 0 for the fused routes and for a
 *   refused cfg; it grows with neither B beyond a chunk nor Q beyond the chunk sizes above.
 * svgp_ball_state_route(cfg, op, buf, cap): the kernels (library entry points for the shared pieces) of one call as text, one name
 *   per line in launch order, from the same plan as the launch code; needs no device.
 * Each entry reads only its own fields of cfg and bufs: update B, T, m and times, mu, var, mask, stats; finalize B, m, jitter and
 * stats, post; query B, m, Q, q_slices, clip_lo / hi and tq, eps, post, p_m, p_v, z; the joint query B, m, Q, path_jitter and tq,
 * eps, post, p_m, cov, chol, z; all of them ip and ls.
 * Refused with a message before any launch: a NULL cfg / bufs / needed pointer, a needed size below 1, clip_lo > clip_hi,
 *   path_jitter < 0 or NaN, q_slices out of range, NULL work where the size is non-zero (SVGP_ERR_INVALID); m, T or Q beyond the
 *   route's range (SVGP_ERR_UNSUPPORTED).  Explicit stream, no allocation, no synchronisation.                                  */
#define SVGP_BALL_STATE_UPDATE      0
#define SVGP_BALL_STATE_FINALIZE    1
#define SVGP_BALL_STATE_QUERY       2
#define SVGP_BALL_STATE_QUERY_JOINT 3
typedef struct {
    int32_t B, T, m, Q;
    int32_t large;                            /* 0: the fused routes (m <= 64); otherwise the large routes */
    int32_t q_slices;                         /* fused query: 0 = the library chooses */
    double jitter, clip_lo, clip_hi, path_jitter;
} svgp_ball_state_cfg;
typedef struct {
    const double *times, *tq;                 /* (T), (Q) */
    const double *ip_x, *ip_y;                /* (m) */
    const double *ls_x, *ls_y;                /* scalars */
    const double *mu_x, *mu_y, *var_x, *var_y;/* (T, B) */
    const double *mask;                       /* (T, B) or NULL */
    const double *eps_x, *eps_y;              /* (Q, B) or NULL */
    double *stats, *post;                     /* (B, 2, m m + m) */
    double *p_m_x, *p_m_y, *p_v_x, *p_v_y;    /* (Q, B); p_v: the marginal query only */
    double *cov_x, *cov_y;                    /* (B, Q, Q) or NULL; the joint query only */
    double *chol_x, *chol_y;                  /* (B, Q, Q) or NULL; the joint query only */
    double *z_x, *z_y;                        /* (Q, B) or NULL */
} svgp_ball_state_bufs;
long long svgp_ball_state_workspace_elems(const svgp_ball_state_cfg* cfg, int op);
int svgp_ball_state_route(const svgp_ball_state_cfg* cfg, int op, char* buf, int cap);
int svgp_ball_state_update(const svgp_ball_state_cfg* cfg, const svgp_ball_state_bufs* bufs, double* work, void* stream);
int svgp_ball_state_finalize(const svgp_ball_state_cfg* cfg, const svgp_ball_state_bufs* bufs, double* work, void* stream);
int svgp_ball_state_query(const svgp_ball_state_cfg* cfg, const svgp_ball_state_bufs* bufs, double* work, void* stream);
int svgp_ball_state_query_joint(const svgp_ball_state_cfg* cfg, const svgp_ball_state_bufs* bufs, double* work, void* stream);

/* ---- runtime helpers: HIP graphs and events without going through torch ---------------------*/
int svgp_stream_create(void** stream_out);
/* HIP maps streams onto a small pool of hardware queues (GPU_MAX_HW_QUEUES) in creation order; two streams on one queue run
 * one after the other whatever the events say.  svgp_streams_overlap: *out = 1 iff a kernel on b runs BESIDE a kernel on a
 * (a ~40 us spin on a, an empty kernel on b; synchronises both).  svgp_side_streams_prepare: creates the library's two side
 * branches of `stream` now -- picked with that probe from up to 12 candidates -- instead of at the first step (which may
 * be under stream capture, where the probe cannot run).  SVGP_STREAM_PROBE=0 disables the probe.                          */
int svgp_streams_overlap(void* a, void* b, int* out);
int svgp_side_streams_prepare(void* stream);
int svgp_stream_destroy(void* stream);
int svgp_stream_sync(void* stream);
int svgp_graph_begin(void* stream);                       /* hipStreamBeginCapture               */
int svgp_graph_end(void* stream, void** graph_exec_out);  /* EndCapture + Instantiate            */
int svgp_graph_launch(void* graph_exec, void* stream);
int svgp_graph_destroy(void* graph_exec);
int svgp_event_create(void** event_out);
int svgp_event_record(void* event, void* stream);
int svgp_event_elapsed_ms(void* start, void* stop, float* ms_out); /* synchronises on `stop`      */
int svgp_event_destroy(void* event);

/* ---- plain VAE / conditional VAE on rotated MNIST (csrc/cvae.hip) ---------------------------------------------------------
 * forward_pass_standard_VAE_rotated_mnist (SVGPVAE_model.py:718-782) on mnistVAE (cvae = 0) or mnistCVAE (cvae = 1,
 * VAE_utils.py:165-258), float64.  aux is (b, 2) rows [id, angle]; only cvae = 1 reads it (it may be NULL otherwise).
 *   encoder   cvae: input channels [image, sin a, cos a]; three stride-2 valid 3 x 3 ELU convolutions, flatten to 32, cvae: concatenate
 *             [sin a, cos a] (34); dense to 2 L.  mu = enc[:, :L], var = exp(enc[:, L:]), with clip_qs clipped to [1e-3, 10] (the clip mask
 *             enters the reverse pass).  z = mu + eps sqrt(var); eps (b, L) given, or NULL: Philox on state[SVGP_ST_RNG_CTR], index n L + l,
 *             and the counter advances by one per call.
 *   decoder   cvae: [z, sin a, cos a] (L + 2); dense 128 -> (4, 4, 8), cvae: two constant planes -> (4, 4, 10); up 2x, conv same, ELU;
 *             up 2x, conv valid, ELU; up 2x, conv 8 -> 1 same, ELU.
 *   scalars   sq = sum (x - xhat)^2, KL = 0.5 (-b L - sum log var + sum var + sum mu^2), elbo = -(0.5 / sigma^2) sq - KL; they go to
 *             state[SVGP_ST_ELBO], [SVGP_ST_RECON_LOSS] = sq / 784, [SVGP_ST_KL_TERM] = KL.  The step minimises -elbo.
 * Parameters: the reference's variable-creation order under the names of svgp_mnist_param_layout (cvae = 1: enc_c1_w (3,3,3,8),
 * enc_d_w (34, 2L), dec_d_w (L+2, 128), dec_c1_w (3,3,10,8); 6 329 parameters at L = 16, 5 721 for cvae = 0, whose layout is the first
 * n_vae entries of svgp_mnist_param_layout); ip .. ov = n_total.
 * svgp_cvae_train_step: TWO launches (svgp_cvae_step_route prints them).  k_cvae_step_images: min(b, 256) workgroups, workgroup g walks
 *   the images g, g + grid, ... through forward and reverse with every activation in LDS (svgp_cvae_lds_bytes(cvae, L): the dynamic
 *   LDS of that launch, the same for every 1 <= L <= 64; -1 for other arguments); k_cvae_reduce_adam: grad (n_total) as fixed-order
 *   sums -- no float atomics, the same input gives the same bits --, TF1 Adam on state[SVGP_ST_LR] as svgp_adam_tf1_step computes it
 *   (adam = 0: theta and the moments stay untouched, adam_m / adam_v may be NULL), the scalars, SVGP_ST_ADAM_T += 1 with adam.
 *   cfg.store = 1 also writes ws.recon (b,28,28,1), ws.qnet_mu, ws.qnet_var, ws.z (b, L).
 * svgp_cvae_forward: the same forward with the stored fields and the scalars, no reverse pass.
 * svgp_cvae_encode: b rows -> mu, var (b, L) (clipped when cfg.clip_qs).  svgp_cvae_decode: z (b, L) and the angles of aux -> (b,28,28,1).
 * svgp_cvae_predict (predict_CVAE, SVGPVAE_model.py:785-820; cvae = 1 only, cfg.b = test rows): encodes the n_train train rows WITHOUT
 *   clipping, z_n = mu_n + eps_n sqrt(var_n) (eps (n_train, L) or NULL: Philox); test row t gets the mean of z_n over the train rows with
 *   aux_train[n, 0] == aux_test[t, 0] (a comparison of doubles, rows summed in ascending n; no such row: NaN, nothing read out of range),
 *   decoded at aux_test[t, 1]; *loss_out = mean over all test pixels of (x - xhat)^2.  Two launches (svgp_cvae_predict_route): the encoder
 *   over the train rows, then one in which a workgroup forms its test rows' means and decodes them.  work: svgp_cvae_predict_workspace_elems.
 * Refused before any launch: NULL cfg / pointers, b < 0, b > b_cap, cvae or store outside {0, 1}, sigma <= 0 (SVGP_ERR_INVALID);
 * L < 1 or L > 64 (SVGP_ERR_UNSUPPORTED).  b = 0 returns SVGP_OK without a launch.  Workspace offsets depend on b_cap, not on b. */
typedef struct {
    int32_t b, b_cap, L;
    int32_t cvae;       /* 0 = mnistVAE, 1 = mnistCVAE */
    int32_t clip_qs, store;
    double  sigma;      /* sigma_gaussian_decoder */
} svgp_cvae_cfg;
typedef struct {        /* offsets into ws, in float64 elements */
    int64_t part, sums;              /* (256, part_stride) convolution weight-gradient partials; (256, 2) [sq, KL] */
    int64_t a3, dpre, zx, dh0;       /* operand rows of the dense layers' weight gradients: (b, 32|34), (b, 2L), (b, L|L+2), (b, 128) */
    int64_t recon, qnet_mu, qnet_var, z;
    int64_t part_stride, total;
} svgp_cvae_ws_layout;
int svgp_cvae_param_layout_get(const svgp_cvae_cfg*, svgp_mnist_param_layout* out);
int svgp_cvae_ws_layout_get(const svgp_cvae_cfg*, svgp_cvae_ws_layout* out);
int svgp_cvae_lds_bytes(int cvae, int L);
int svgp_cvae_step_route(const svgp_cvae_cfg*, char* buf, int cap);
int svgp_cvae_predict_route(const svgp_cvae_cfg*, char* buf, int cap);
int svgp_cvae_train_step(const svgp_cvae_cfg*, double* theta, const double* images, const double* aux, const double* eps, double* ws,
                         double* grad, double* adam_m, double* adam_v, double* state, int adam, void* stream);
int svgp_cvae_forward(const svgp_cvae_cfg*, const double* theta, const double* images, const double* aux, const double* eps, double* ws,
                      double* state, void* stream);
int svgp_cvae_encode(const svgp_cvae_cfg*, const double* theta, const double* images, const double* aux, double* mu, double* var,
                     void* stream);
int svgp_cvae_decode(const svgp_cvae_cfg*, const double* theta, const double* z, const double* aux, double* images_out, void* stream);
long long svgp_cvae_predict_workspace_elems(const svgp_cvae_cfg*, long long n_train);
int svgp_cvae_predict(const svgp_cvae_cfg*, long long n_train, const double* theta, const double* images_train, const double* aux_train,
                      const double* eps, const double* images_test, const double* aux_test, double* work, double* recon_out,
                      double* loss_out, double* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVGPVAE_HIP_H */
