// Posterior cache and conditional generation for the Casale GP-VAE on rotated MNIST.
//
// Reference semantics: predict_test_set_Casale (GPVAE_Casale_model.py:158-203).  With V (N, H) of casale.hip, H = M Q,
//   P = (alpha I + V^T V)^-1 (H, H),   U = P V^T Z (H, L),   L_W = chol(K_W) on the Q train angles,
// the posterior at a query row x* = [id, angle, o*] needs no train row:
//   kappa_r = k_W(angle*, angle_r)      lambda = L_W^-1 kappa      v*[k Q + r] = on*_k lambda_r      (K_*n = v*^T V^T exactly)
//   mean* = v*^T U (L)      var* = k** - |v*|^2 + alpha v*^T P v*      k** = amplitude^2 |on*|^2
// svgp_casale_cache_build writes [angles | L_W | U | P] once from the latent rows Z (the front half of svgp_casale_gp_fwd);
// svgp_casale_generate turns query rows into images: one launch for H <= 256, a fixed list of five beyond.
#include "common.hpp"
#include "vae_dev.hpp"

extern "C" int svgp_dgemm_batched(int ta, int tb, int M, int N, int K, double alpha, const double* A, int lda,
                                  long long strideA, const double* B, int ldb, long long strideB, double beta,
                                  double* C, int ldc, long long strideC, int batch, void* stream);

namespace {

using namespace svgp_vae;

#define CG_QMAX 32             // svgp_casale_layout_get refuses Q beyond it
#define CG_LWS (CG_QMAX + 1)   // row stride of L_W in LDS: lane r reads L_W[r][j] of one column j, all on different banks
#define CG_HFUSED 256          // H up to which one launch does everything
#define CG_ROWS 256            // H beyond: query rows per pass of the five launches (the workspace holds 2 x CG_ROWS x H)
#define CG_MMAX 128

void cache_layout_fill(const svgp_casale_cfg* c, svgp_casale_cache_layout* o) {
    const int64_t Q = c->Q, H = (int64_t)c->M * c->Q, L = c->L;
    SvgpTake16 c16;      // 16-element boundaries, as the workspace's
    o->angles = c16.take(Q); o->L_W = c16.take(Q * Q); o->U = c16.take(H * L); o->P = c16.take(H * H);
    o->total = c16.p;
}

// cache = [angles | L_W | U | P], P written as (P + P^T) / 2: symmetric bit for bit (the sum of two doubles commutes)
__global__ __launch_bounds__(SVGP_BLOCK) void k_casale_cache_pack(int Q, int H, int L, const real* __restrict__ ang,
                                                                  const real* __restrict__ LW, const real* __restrict__ U,
                                                                  const real* __restrict__ P, real* __restrict__ c_ang,
                                                                  real* __restrict__ c_LW, real* __restrict__ c_U,
                                                                  real* __restrict__ c_P) {
    const long long nQ = Q, nL = (long long)Q * Q, nU = (long long)H * L, nP = (long long)H * H;
    long long i = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (i < nQ) { c_ang[i] = ang[i]; return; }
    i -= nQ;
    if (i < nL) { c_LW[i] = LW[i]; return; }
    i -= nL;
    if (i < nU) { c_U[i] = U[i]; return; }
    i -= nU;
    if (i < nP) {
        const long long r = i / H, q = i % H;
        c_P[i] = real(0.5) * (P[i] + P[q * H + r]);
    }
}

// ---- generation ---------------------------------------------------------------------------------------------------------------
struct CGenArgs {
    int b, Q, M, H, L, n_obj, normalize, gather;
    const real* th_dec;
    const real* gp;        // [l_GP, amplitude, alpha | object_vectors (n_obj, M)]
    const real* aux;       // (b, 2+M)
    const real* ang;       // (Q)
    const real* LW;        // (Q, Q) lower triangular
    const real* U;         // (H, L)
    const real* P;         // (H, H), symmetric bit for bit
    const real* eps;       // (b, L) or NULL
    const real* z;         // !GP: (b, L) samples formed by the row-sum kernel
    real* images;          // (b, 784)
    real* mean; real* var; // (b, L), (b) or NULL
};

// object vector of query row n, or nullptr when the row's id is outside the table
__device__ __forceinline__ const real* cgen_obj_row(const CGenArgs& a, int n) {
    return svgp_query_obj_row(a.aux, a.M, a.gather, a.gp + 3, a.n_obj, n);
}

// lambda = L_W^-1 kappa in the first wave: lane r holds x_r = kappa_r - sum_{j < r} L_W[r][j] lambda_j (j ascending), lane j
// broadcasts lambda_j = x_j / L_W[j][j].  ld: row stride of lw.  Every lane of the wave calls it; lanes >= Q carry zeros.
__device__ __forceinline__ real cgen_forward_subst(int Q, const real* lw, int ld, real kap) {
    const int r = threadIdx.x & 63;
    real x = r < Q ? kap : real(0), lam = 0;
    for (int j = 0; j < Q; ++j) {
        const real d = lw[j * ld + j];
        const real lj = __shfl(x, j, 64) / d;
        if (r == j) lam = lj;
        if (r > j && r < Q) x -= lw[r * ld + j] * lj;
    }
    return lam;
}

// One workgroup of VAE_NT threads walks images blockIdx.x, + gridDim.x, ... on the decoder forward piece of vae_dev.hpp (decoder weights,
// the effective up-convolution weights and here L_W staged in LDS once).  GP, per image: thread r < Q forms kappa_r, the first wave
// lambda, thread i < H v*_i; thread i < H then (sum_j P[j][i] v_j) v_i, j ascending (P is symmetric: the column walk is coalesced over i), thread
// 256 + l meanwhile sum_j v_j U[j][l], j ascending; thread l < L adds the H terms and the H squares in index order (every l the same
// sums from the same LDS words) and forms z.  Fixed order everywhere: a row gives the same bits wherever it stands in a batch of any
// size.  Rolled up-convolutions (fwd_valu<true>), as k_generate<true>: the unrolled ones exceed 256 VGPRs there and spill.
// !GP (H > 256): decode of the samples a.z only.
template <bool GP>
__global__ __launch_bounds__(VAE_NT) void k_casale_generate(CGenArgs a) {
    extern __shared__ __align__(16) real smem[];
    if constexpr (!GP) {
        decoder_fwd_rows(a.b, a.L, a.th_dec, a.z, a.images, blockIdx.x, gridDim.x, smem);
        return;
    }
    const DecOff od = dec_off(a.L);
    const DecFwdLds d = dec_fwd_carve<false>(smem, od.n);
    real* lw = d.We1 + DEC_NWE;      // CG_QMAX x CG_LWS
    real* lam = lw + CG_QMAX * CG_LWS;   // CG_QMAX
    real* on = lam + CG_QMAX;        // CG_MMAX: the normalised object vector
    real* vs = on + CG_MMAX;         // CG_HFUSED: v*
    real* qt = vs + CG_HFUSED;       // CG_HFUSED: terms of the quadratic form
    real* mn = qt + CG_HFUSED;       // 64: mean*
    real* sc = mn + 64;              // 2: k**
    const int Q = a.Q, M = a.M, H = a.H, L = a.L, st = 2 + a.M;
    for (int e = threadIdx.x; e < Q * Q; e += VAE_NT) lw[(e / Q) * CG_LWS + e % Q] = a.LW[e];
    decoder_fwd_stage(d, od, a.th_dec);
    for (int n = blockIdx.x; n < a.b; n += gridDim.x) {
        __syncthreads();
        const real* orow = cgen_obj_row(a, n);
        const real amp = a.gp[1], ls = a.gp[0], a2_ = amp * amp, inv_l2 = real(1) / (ls * ls), alpha = a.gp[2];
        const int t = threadIdx.x;
        if (t < 64) {            // (Q <= 32: one wave)
            const real kap = t < Q ? svgp_view_k(a.aux[(size_t)n * st + 1] - a.ang[t], a2_, inv_l2) : real(0);
            const real l = cgen_forward_subst(Q, lw, CG_LWS, kap);
            if (t < Q) lam[t] = l;
        } else if (t >= 128 && t < 128 + M) {
            const int k = t - 128;
            real v = __builtin_nan("");
            if (orow) v = orow[k] * (a.normalize ? real(1) / sqrt(svgp_dotM(orow, orow, M)) : real(1));
            on[k] = v;
        } else if (t == 256) {
            sc[0] = svgp_query_kxx(orow, M, a.normalize, a2_);
        }
        __syncthreads();
        if (t < H) vs[t] = on[t / Q] * lam[t % Q];
        __syncthreads();
        if (t < H) {
            const real* Pc = a.P + t;
            real r = 0;
#pragma unroll 4
            for (int j = 0; j < H; ++j) r += Pc[(size_t)j * H] * vs[j];
            qt[t] = r * vs[t];
        } else if (t >= CG_HFUSED && t < CG_HFUSED + L) {
            const int l = t - CG_HFUSED;
            real m_ = 0;
#pragma unroll 4
            for (int j = 0; j < H; ++j) m_ += vs[j] * a.U[(size_t)j * L + l];
            mn[l] = m_;
        }
        __syncthreads();
        if (t < L) {
            real qs = 0, vv = 0;
#pragma unroll 1
            for (int i = 0; i < H; ++i) { qs += qt[i]; vv += vs[i] * vs[i]; }
            const real var = sc[0] - vv + alpha * qs, m_ = mn[t];
            const size_t e = (size_t)n * L + t;
            if (a.mean) a.mean[e] = m_;
            if (a.var && t == 0) a.var[n] = var;
            d.z[t] = a.eps ? m_ + a.eps[e] * sqrt(var) : m_;
        }
        __syncthreads();
        decoder_fwd_layers<true>(d, od, L);
        lds_copy_out(a.images + (size_t)n * 784, d.out, 784);
    }
}

// LDS doubles of k_casale_generate<true> behind the decoder's part
#define CG_LDS_GP (CG_QMAX * CG_LWS + CG_QMAX + CG_MMAX + 2 * CG_HFUSED + 64 + 2)
static_assert((size_t)(dec_fwd_lds(dec_off(64).n, false) + CG_LDS_GP) * sizeof(real) <= SVGP_LDS_MAX_BYTES,
              "LDS of k_casale_generate<true> at L = 64, Q = 32, H = 256");

// H > 256: one wave per query row n of the pass: v* (H) and k**; a row whose id is outside the table gives a NaN row
__global__ __launch_bounds__(64) void k_casale_generate_rows(CGenArgs a, real* __restrict__ Vq, real* __restrict__ kss) {
    __shared__ real lam[CG_QMAX];
    const int n = blockIdx.x, t = threadIdx.x, Q = a.Q, M = a.M, H = a.H, st = 2 + a.M;
    const real* orow = cgen_obj_row(a, n);
    const real amp = a.gp[1], ls = a.gp[0], a2_ = amp * amp, inv_l2 = real(1) / (ls * ls);
    const real kap = t < Q ? svgp_view_k(a.aux[(size_t)n * st + 1] - a.ang[t], a2_, inv_l2) : real(0);
    const real l = cgen_forward_subst(Q, a.LW, Q, kap);
    if (t < Q) lam[t] = l;
    __syncthreads();
    const real inv = (orow && a.normalize) ? real(1) / sqrt(svgp_dotM(orow, orow, M)) : real(1);
    for (int h = t; h < H; h += 64) Vq[(size_t)n * H + h] = orow ? orow[h / Q] * inv * lam[h % Q] : __builtin_nan("");
    if (t == 0) kss[n] = svgp_query_kxx(orow, M, a.normalize, a2_);
}

// H > 256: thread (n, l): var = k** - sum_j v_j^2 + alpha sum_j (v* P)[j] v_j, j ascending; mean from the product v* U; z
__global__ __launch_bounds__(SVGP_BLOCK) void k_casale_generate_rowsum(CGenArgs a, const real* __restrict__ Vq,
                                                                       const real* __restrict__ VP, const real* __restrict__ kss,
                                                                       const real* __restrict__ mean_in, real* __restrict__ z) {
    const long long e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= (long long)a.b * a.L) return;
    const int n = (int)(e / a.L), l = (int)(e % a.L), H = a.H;
    const real* vr = Vq + (size_t)n * H;
    const real* pr = VP + (size_t)n * H;
    real qs = 0, vv = 0;
    for (int j = 0; j < H; ++j) { qs += pr[j] * vr[j]; vv += vr[j] * vr[j]; }
    const real var = kss[n] - vv + a.gp[2] * qs, m_ = mean_in[e];
    if (a.mean) a.mean[e] = m_;
    if (a.var && l == 0) a.var[n] = var;
    z[e] = a.eps ? m_ + a.eps[e] * sqrt(var) : m_;
}

// The launches of one pass of svgp_casale_generate, in order: the call walks this list, svgp_casale_generate_route prints it.
enum CGenOp { CGEN_FUSED, CGEN_ROWS, CGEN_PROD_P, CGEN_PROD_U, CGEN_ROWSUM, CGEN_DECODE };
const char* const CGEN_NAME[] = {"k_casale_generate", "k_casale_generate_rows", "svgp_dgemm_batched", "svgp_dgemm_batched",
                                 "k_casale_generate_rowsum", "k_casale_generate"};
int cgen_plan(const svgp_casale_cfg* c, CGenOp* ops) {
    if ((long long)c->M * c->Q <= CG_HFUSED) { ops[0] = CGEN_FUSED; return 1; }
    ops[0] = CGEN_ROWS; ops[1] = CGEN_PROD_P; ops[2] = CGEN_PROD_U; ops[3] = CGEN_ROWSUM; ops[4] = CGEN_DECODE;
    return 5;
}
struct CGenWork { int64_t Vq, VP, kss, mean, z, total; };
CGenWork cgen_work(const svgp_casale_cfg* c, long long b) {
    CGenWork o = {0, 0, 0, 0, 0, 0};
    const int64_t H = (int64_t)c->M * c->Q, L = c->L;
    if (H <= CG_HFUSED || b < 1) return o;
    const int64_t rows = b < CG_ROWS ? b : CG_ROWS;
    SvgpTake16 c16;
    o.Vq = c16.take(rows * H); o.VP = c16.take(rows * H); o.kss = c16.take(rows); o.mean = c16.take(rows * L); o.z = c16.take(rows * L);
    o.total = c16.p;
    return o;
}

}  // namespace

extern "C" int svgp_casale_cache_layout_get(const svgp_casale_cfg* c, svgp_casale_cache_layout* o) {
    svgp_casale_layout wl;
    int rc = svgp_casale_layout_get(c, &wl);       // refuses Q > 32, H > 2048, M > 128, L > 64
    if (rc) return rc;
    SVGP_REQUIRE(o != nullptr, SVGP_ERR_INVALID, "out is NULL");
    cache_layout_fill(c, o);
    return SVGP_OK;
}

extern "C" int svgp_casale_cache_build(const svgp_casale_cfg* c, const double* gp, const double* angles, const int32_t* obj_idx,
                                       const int32_t* ang_idx, const double* Z, double* ws, double* cache, void* stream) {
    svgp_casale_layout wl;
    int rc = svgp_casale_layout_get(c, &wl);
    if (rc) return rc;
    SVGP_REQUIRE(gp && angles && obj_idx && ang_idx && Z && ws && cache, SVGP_ERR_INVALID, "NULL device pointer");
    rc = svgp_casale_hspace_fwd(c, wl, gp, angles, obj_idx, ang_idx, Z, ws, stream);
    if (rc) return rc;
    svgp_casale_cache_layout cl;
    cache_layout_fill(c, &cl);
    const int Q = c->Q, H = c->M * c->Q, L = c->L;
    const long long tot = (long long)Q + (long long)Q * Q + (long long)H * L + (long long)H * H;
    hipLaunchKernelGGL(k_casale_cache_pack, dim3(svgp_blocks(tot)), dim3(SVGP_BLOCK), 0,
                       (hipStream_t)stream, Q, H, L, angles, ws + wl.L_W, ws + wl.U, ws + wl.P, cache + cl.angles, cache + cl.L_W,
                       cache + cl.U, cache + cl.P);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" long long svgp_casale_generate_workspace_elems(const svgp_casale_cfg* c, long long b) {
    svgp_casale_layout wl;
    if (svgp_casale_layout_get(c, &wl)) return 0;
    return cgen_work(c, b).total;
}

extern "C" int svgp_casale_generate_route(const svgp_casale_cfg* c, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    svgp_casale_layout wl;
    int rc = svgp_casale_layout_get(c, &wl);
    if (rc) return rc;
    CGenOp ops[8];
    const int n = cgen_plan(c, ops);
    int pos = 0;
    buf[0] = 0;
    for (int i = 0; i < n && !rc; ++i) rc = svgp_route_append(buf, cap, &pos, "%s\n", CGEN_NAME[ops[i]]);
    return rc;
}

extern "C" int svgp_casale_generate(const svgp_casale_cfg* c, long long b, const double* theta, const double* cache, const double* aux,
                                    int gather, const double* eps, double* images_out, double* mean_out, double* var_out,
                                    double* work, void* stream) {
    svgp_casale_layout wl;
    int rc = svgp_casale_layout_get(c, &wl);
    if (rc) return rc;
    SVGP_REQUIRE(b >= 0 && b <= 0x7fffffffLL / 784, SVGP_ERR_INVALID, "b = %lld query rows (0 <= b <= %lld)", b, 0x7fffffffLL / 784);
    SVGP_REQUIRE(theta && cache && aux && images_out, SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(!gather || c->n_obj >= 1, SVGP_ERR_INVALID, "gather needs an object-vector table (n_obj = %d)", c->n_obj);
    const CGenWork gw = cgen_work(c, b);
    SVGP_REQUIRE(gw.total == 0 || work, SVGP_ERR_INVALID, "work is NULL (H = %d needs %lld doubles)", c->M * c->Q, (long long)gw.total);
    if (b == 0) return SVGP_OK;
    svgp_casale_cache_layout cl;
    cache_layout_fill(c, &cl);
    const int H = c->M * c->Q, L = c->L;
    CGenArgs a;
    a.Q = c->Q; a.M = c->M; a.H = H; a.L = L; a.n_obj = c->n_obj; a.normalize = c->normalize_obj; a.gather = gather != 0;
    a.th_dec = theta + wl.n_enc; a.gp = theta + wl.n_vae;
    a.ang = cache + cl.angles; a.LW = cache + cl.L_W; a.U = cache + cl.U; a.P = cache + cl.P;
    a.z = work ? work + gw.z : nullptr;
    const int64_t n_dec = wl.n_vae - wl.n_enc;
    const size_t lds_dec = (size_t)dec_fwd_lds((int)n_dec, false) * sizeof(real);
    const size_t lds_gp = lds_dec + (size_t)CG_LDS_GP * sizeof(real);       // (L = 64: 16 587 doubles = 132 696 bytes, asserted above)
    hipStream_t st = (hipStream_t)stream;
    CGenOp ops[8];
    const int n = cgen_plan(c, ops);
    const long long step = n == 1 ? b : CG_ROWS;
    for (long long lo = 0; lo < b; lo += step) {
        const int bb = (int)(b - lo < step ? b - lo : step);
        a.b = bb;
        a.aux = aux + (size_t)lo * (2 + c->M);
        a.eps = eps ? eps + (size_t)lo * L : nullptr;
        a.images = images_out + (size_t)lo * 784;
        a.mean = mean_out ? mean_out + (size_t)lo * L : nullptr;
        a.var = var_out ? var_out + lo : nullptr;
        const dim3 grid(bb < SVGP_MAX_PART ? bb : SVGP_MAX_PART);
        for (int i = 0; i < n; ++i) {
            switch (ops[i]) {
            case CGEN_FUSED:
                rc = set_dyn_lds(k_casale_generate<true>, lds_gp);
                if (rc) return rc;
                hipLaunchKernelGGL(k_casale_generate<true>, grid, dim3(VAE_NT), lds_gp, st, a);
                SVGP_LAUNCH_CHECK();
                break;
            case CGEN_ROWS:
                hipLaunchKernelGGL(k_casale_generate_rows, dim3(bb), dim3(64), 0, st, a, work + gw.Vq, work + gw.kss);
                SVGP_LAUNCH_CHECK();
                break;
            case CGEN_PROD_P:       // (b, H) = v* P
                rc = svgp_dgemm_batched(0, 0, bb, H, H, 1.0, work + gw.Vq, H, 0, a.P, H, 0, 0.0, work + gw.VP, H, 0, 1, stream);
                if (rc) return rc;
                break;
            case CGEN_PROD_U:       // (b, L) = v* U
                rc = svgp_dgemm_batched(0, 0, bb, L, H, 1.0, work + gw.Vq, H, 0, a.U, L, 0, 0.0, work + gw.mean, L, 0, 1, stream);
                if (rc) return rc;
                break;
            case CGEN_ROWSUM:
                hipLaunchKernelGGL(k_casale_generate_rowsum, dim3(svgp_blocks((long long)bb * L)),
                                   dim3(SVGP_BLOCK), 0, st, a, work + gw.Vq, work + gw.VP, work + gw.kss, work + gw.mean, work + gw.z);
                SVGP_LAUNCH_CHECK();
                break;
            case CGEN_DECODE:
                rc = set_dyn_lds(k_casale_generate<false>, lds_dec);
                if (rc) return rc;
                hipLaunchKernelGGL(k_casale_generate<false>, grid, dim3(VAE_NT), lds_dec, st, a);
                SVGP_LAUNCH_CHECK();
                break;
            }
        }
    }
    return SVGP_OK;
}
