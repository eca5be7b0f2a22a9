// Posterior cache and conditional generation for the rotated-MNIST model.
//
// Reference semantics: mainSVGP.approximate_posterior_params (SVGPVAE_model.py:303-343) and
// bacthing_predict_SVGPVAE_rotated_mnist (:1026-1083).  The posterior at a query row x depends on the train set only through
//   w_l = c (Sigma_l + jI)^-1 v_l,   X_l = (Sigma_l + jI)^-1 - (K_mm + jI)^-1,   Sigma_l = K_mm + c S_l,
// so the statistics S_l, v_l are accumulated over the train rows in chunks (svgp_gp_stats_accumulate), [w | X] is formed once
// (svgp_mnist_cache_build) and a query is p_m = k_x . w_l, p_v = k_xx + k_x^T X_l k_x, z = p_m + eps sqrt(p_v), decode(z):
// one launch for m <= 64 (svgp_mnist_generate), no train row touched.
#include "common.hpp"
#include "vae_dev.hpp"

extern "C" int svgp_dgemm_batched(int ta, int tb, int M, int N, int K, double alpha, const double* A, int lda,
                                  long long strideA, const double* B, int ldb, long long strideB, double beta,
                                  double* C, int ldc, long long strideC, int batch, void* stream);
extern "C" size_t svgp_spd_inverse_workspace_elems(int m, int batch);
extern "C" int svgp_spd_inverse_batched(int m, int batch, double* A, double* logdet, double* work, void* stream);
extern "C" int svgp_kernel_matrix_xy(int M, int normalize, int nx, const double* x, int x_gather, int ny, const double* y,
                                     int y_gather, const double* table, const double* l_GP, const double* amplitude,
                                     int diag_only, double* out, void* stream);       // cache build: K_mm of the inducing points

namespace {

using namespace svgp_vae;

void cache_layout_fill(const svgp_mnist_cfg* c, svgp_mnist_cache_layout* o) {
    const int64_t m = c->m, L = c->L;
    SvgpTake16 c16;      // 16-element boundaries, as the workspace's
    o->acc_S = c16.take(L * m * m); o->acc_v = c16.take(L * m); o->acc_rows = c16.take(1);
    o->w = c16.take(L * m); o->X = c16.take(L * m * m);
    o->total = c16.p;
}

// ---- accumulation: element i of [S (L m m) | v (L m) | rows]; the P row partials of an element are added in index order first
// (part_sum of gp_kernels.hip), then acc = first ? s : acc + s.  One thread per element, plain loads and stores.
__global__ __launch_bounds__(SVGP_BLOCK) void k_stats_accumulate(long long nS, long long nv, int P, int first, real rows,
                                                                 const real* __restrict__ S, const real* __restrict__ v,
                                                                 real* __restrict__ accS, real* __restrict__ accv,
                                                                 real* __restrict__ acc_rows) {
    const long long i = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (i < nS + nv) {
        const bool isS = i < nS;
        const long long o = isS ? i : i - nS, stride = isS ? nS : nv;
        const real* src = isS ? S : v;
        real s = src[o];
        for (int pp = 1; pp < P; ++pp) s += src[o + pp * stride];
        real* dst = isS ? accS : accv;
        dst[o] = first ? s : dst[o] + s;
    } else if (i == nS + nv) {
        *acc_rows = first ? rows : *acc_rows + rows;
    }
}

// ---- cache build, m > 64: B (L + 1, m, m) = [K + c S_l + jI | K + jI], c = N_train / rows read on the device
__global__ __launch_bounds__(SVGP_BLOCK) void k_cache_sigma(int m, int L, real N_train, real jitter, const real* __restrict__ K,
                                                            const real* __restrict__ accS, const real* __restrict__ rows,
                                                            real* __restrict__ B) {
    const long long mm = (long long)m * m, i = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (i >= (L + 1) * mm) return;
    const long long o = i % mm;
    const int l = (int)(i / mm);
    const real jit = (o / m) == (o % m) ? jitter : real(0);
    const real c = N_train / rows[0];
    B[i] = l < L ? K[o] + c * accS[i] + jit : K[o] + jit;
}
// grid (m, L): row i of channel l.  w_l[i] = c sum_j Si_l[i][j] v_l[j] (each thread its j = t, t + 256, ... in order, block_sum),
// X_l[i][:] = ((Si_l - Ki)[i][:] + (Si_l - Ki)[:][i]) / 2
__global__ __launch_bounds__(SVGP_BLOCK) void k_cache_finish(int m, int L, real N_train, const real* __restrict__ Binv,
                                                             const real* __restrict__ accv, const real* __restrict__ rows,
                                                             real* __restrict__ w, real* __restrict__ X) {
    __shared__ real red[16];
    const int i = blockIdx.x, l = blockIdx.y;
    const size_t mm = (size_t)m * m;
    const real* Si = Binv + (size_t)l * mm;
    const real* Ki = Binv + (size_t)L * mm;
    const real c = N_train / rows[0];
    real s = 0;
    for (int j = threadIdx.x; j < m; j += SVGP_BLOCK) {
        s += Si[(size_t)i * m + j] * accv[(size_t)l * m + j];
        X[(size_t)l * mm + (size_t)i * m + j] =
            real(0.5) * ((Si[(size_t)i * m + j] - Ki[(size_t)i * m + j]) + (Si[(size_t)j * m + i] - Ki[(size_t)j * m + i]));
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) w[(size_t)l * m + i] = c * s;
}

// ---- generation ---------------------------------------------------------------------------------------------------------------
struct GenArgs {
    int b, m, L, M, n_obj, normalize, gather;
    const real* th_dec;
    const real* aux;       // (b, 2+M)
    const real* ip;        // (m, 2+M)
    const real* ov;        // (n_obj, M)
    const real* ls; const real* amp;
    const real* w;         // (L, m)
    const real* X;         // (L, m, m), symmetric bit for bit
    const real* eps;       // (b, L) or NULL
    const real* z;         // !GP: (b, L) samples formed by the row-sum kernel
    real* images;          // (b, 784)
    real* p_m; real* p_v;  // (b, L) or NULL
};

// object vector of query row n, or nullptr when the row's id is outside the table
__device__ __forceinline__ const real* gen_obj_row(const GenArgs& a, int n) {
    return svgp_query_obj_row(a.aux, a.M, a.gather, a.ov, a.n_obj, n);
}

// One workgroup of VAE_NT threads walks images blockIdx.x, + gridDim.x, ... on the decoder forward piece of vae_dev.hpp (decoder weights
// and the effective up-convolution weights staged in LDS once).  GP: per image, thread j < m forms k_x[j] (svgp_query_kx); thread
// (l, i) forms k_i sum_j X_l[j][i] k_j, j ascending (X is symmetric: the column walk is coalesced over i); thread l adds the
// m terms of channel l in index order, p_m = sum_j k_j w_l[j] in index order, z = p_m + eps sqrt(p_v).  Fixed order everywhere: a row
// gives the same bits wherever it stands in the batch.  The GP form runs the rolled up-convolutions (fwd_valu<true>: same FMA order, ~85
// VGPRs fewer): with the fully unrolled ones it needs more than 256 VGPRs and spills.  !GP (m > 64): decode of the samples a.z only.
template <bool GP>
__global__ __launch_bounds__(VAE_NT) void k_generate(GenArgs a) {
    extern __shared__ __align__(16) real smem[];
    if constexpr (!GP) {
        decoder_fwd_rows(a.b, a.L, a.th_dec, a.z, a.images, blockIdx.x, gridDim.x, smem);
        return;
    }
    const DecOff od = dec_off(a.L);
    const DecFwdLds d = dec_fwd_carve<false>(smem, od.n);
    real* kx = d.We1 + DEC_NWE;      // m (+ k_xx at kx[m])
    real* qt = kx + a.m + 1;         // L m terms of the quadratic forms
    decoder_fwd_stage(d, od, a.th_dec);
    const int m = a.m, L = a.L;
    for (int n = blockIdx.x; n < a.b; n += gridDim.x) {
        __syncthreads();
        const real* on = gen_obj_row(a, n);
        if ((int)threadIdx.x <= m) {
            const real amp = *a.amp, ls = *a.ls, a2_ = amp * amp, inv_l2 = real(1) / (ls * ls);
            real val;
            if (!on) {
                val = __builtin_nan("");
            } else if ((int)threadIdx.x < m) {
                val = svgp_query_kx(on, a.aux, n, a.ip, threadIdx.x, a.M, a.normalize, a2_, inv_l2);
            } else {
                val = svgp_query_kxx(on, a.M, a.normalize, a2_);
            }
            kx[threadIdx.x] = val;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < L * m; p += VAE_NT) {
            const int l = p / m, i = p % m;
            const real* Xl = a.X + (size_t)l * m * m + i;
            real r = 0;
#pragma unroll 4
            for (int j = 0; j < m; ++j) r += Xl[(size_t)j * m] * kx[j];
            qt[p] = r * kx[i];
        }
        __syncthreads();
        if ((int)threadIdx.x < L) {
            const int l = threadIdx.x;
            real qs = 0, pm = 0;
#pragma unroll 1
            for (int i = 0; i < m; ++i) qs += qt[l * m + i];
#pragma unroll 1
            for (int j = 0; j < m; ++j) pm += kx[j] * a.w[(size_t)l * m + j];
            const real pv = kx[m] + qs;
            const size_t e = (size_t)n * L + l;
            if (a.p_m) a.p_m[e] = pm;
            if (a.p_v) a.p_v[e] = pv;
            d.z[l] = a.eps ? pm + a.eps[e] * sqrt(pv) : pm;
        }
        __syncthreads();
        decoder_fwd_layers<true>(d, od, L);
        lds_copy_out(a.images + (size_t)n * 784, d.out, 784);
    }
}

// m > 64: K_x (b, m), element (n, j) with the expressions of k_kernel_matrix_xy; a gathered row whose id is outside the table gives a
// NaN row (gen_obj_row) instead of a read outside it, which the two products and the row sums carry into that row's outputs
__global__ __launch_bounds__(SVGP_BLOCK) void k_generate_kx(GenArgs a, real* __restrict__ Kx) {
    const long long idx = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (idx >= (long long)a.b * a.m) return;
    const int n = (int)(idx / a.m), j = (int)(idx % a.m);
    const real* on = gen_obj_row(a, n);
    if (!on) { Kx[idx] = __builtin_nan(""); return; }
    const real amp = *a.amp, ls = *a.ls;
    Kx[idx] = svgp_query_kx(on, a.aux, n, a.ip, j, a.M, a.normalize, amp * amp, real(1) / (ls * ls));
}

// m > 64: thread (n, l): p_v = k_xx + sum_j P_l[n][j] Kx[n][j], j ascending; p_m from the product K_x w^T; z
__global__ __launch_bounds__(SVGP_BLOCK) void k_generate_rowsum(GenArgs a, const real* __restrict__ Kx, const real* __restrict__ P,
                                                                const real* __restrict__ pm_in, real* __restrict__ z) {
    const long long e = (long long)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= (long long)a.b * a.L) return;
    const int n = (int)(e / a.L), l = (int)(e % a.L), m = a.m;
    const real* on = gen_obj_row(a, n);
    const real amp = *a.amp, kxx = svgp_query_kxx(on, a.M, a.normalize, amp * amp);
    const real* pr = P + ((size_t)l * a.b + n) * m;
    const real* kr = Kx + (size_t)n * m;
    real qs = 0;
    for (int j = 0; j < m; ++j) qs += pr[j] * kr[j];
    const real pm = !on ? __builtin_nan("") : pm_in[e], pv = kxx + qs;
    if (a.p_m) a.p_m[e] = pm;
    if (a.p_v) a.p_v[e] = pv;
    z[e] = a.eps ? pm + a.eps[e] * sqrt(pv) : pm;
}

static_assert((size_t)(dec_fwd_lds(dec_off(64).n, false) + SVGP_M_MAX + 1 + 64 * SVGP_M_MAX) * sizeof(real) <= SVGP_LDS_MAX_BYTES,
              "LDS of k_generate<true> at L = 64, m = SVGP_M_MAX");

// The launches of one svgp_mnist_generate call, in order: svgp_mnist_generate walks this list, svgp_mnist_generate_route prints it.
enum GenOp { GEN_FUSED, GEN_KX, GEN_PROD_X, GEN_PROD_W, GEN_ROWSUM, GEN_DECODE };
const char* const GEN_NAME[] = {"k_generate", "k_generate_kx", "svgp_dgemm_batched", "svgp_dgemm_batched", "k_generate_rowsum",
                                "k_generate"};
int gen_plan(const svgp_mnist_cfg* c, GenOp* ops) {
    if (c->m <= SVGP_M_MAX) { ops[0] = GEN_FUSED; return 1; }
    ops[0] = GEN_KX; ops[1] = GEN_PROD_X; ops[2] = GEN_PROD_W; ops[3] = GEN_ROWSUM; ops[4] = GEN_DECODE;
    return 5;
}
inline int64_t gen_rows_cap(const svgp_mnist_cfg* c) { return c->b_cap > c->b ? c->b_cap : c->b; }
struct GenWork { int64_t Kx, P, pm, z, total; };
GenWork gen_work(const svgp_mnist_cfg* c) {
    GenWork o = {0, 0, 0, 0, 0};
    if (c->m <= SVGP_M_MAX) return o;
    const int64_t b = gen_rows_cap(c), m = c->m, L = c->L;
    SvgpTake16 c16;
    o.Kx = c16.take(b * m); o.P = c16.take(L * b * m); o.pm = c16.take(b * L); o.z = c16.take(b * L);
    o.total = c16.p;
    return o;
}
struct CacheWork { int64_t K, B, logdet, inv, total; };
CacheWork cache_work(const svgp_mnist_cfg* c) {
    CacheWork o = {0, 0, 0, 0, 0};
    if (c->m <= SVGP_M_MAX) return o;
    const int64_t m = c->m, L = c->L;
    SvgpTake16 c16;
    o.K = c16.take(m * m); o.B = c16.take((L + 1) * m * m); o.logdet = c16.take(L + 1);
    o.inv = c16.take((int64_t)svgp_spd_inverse_workspace_elems((int)m, (int)L + 1));
    o.total = c16.p;
    return o;
}

}  // namespace

extern "C" int svgp_mnist_cache_layout_get(const svgp_mnist_cfg* c, svgp_mnist_cache_layout* o) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(o != nullptr, SVGP_ERR_INVALID, "out is NULL");
    cache_layout_fill(c, o);
    return SVGP_OK;
}

extern "C" int svgp_gp_stats_accumulate(const svgp_mnist_cfg* c, const double* ws, double* cache, int first, void* stream) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(ws && cache, SVGP_ERR_INVALID, "NULL device pointer");
    svgp_mnist_ws_layout wl;
    rc = svgp_mnist_ws_layout_get(c, &wl);
    if (rc) return rc;
    svgp_mnist_cache_layout cl;
    cache_layout_fill(c, &cl);
    const long long nS = (long long)c->L * c->m * c->m, nv = (long long)c->L * c->m;
    hipLaunchKernelGGL(k_stats_accumulate, dim3(svgp_blocks(nS + nv + 1)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, nS, nv, (int)wl.stat_parts,
                       first != 0, (real)c->b, ws + wl.S, ws + wl.v, cache + cl.acc_S, cache + cl.acc_v, cache + cl.acc_rows);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" long long svgp_mnist_cache_workspace_elems(const svgp_mnist_cfg* c) {
    if (svgp_check_cfg(c)) return 0;
    return cache_work(c).total;
}

extern "C" int svgp_mnist_cache_build(const svgp_mnist_cfg* c, const double* theta, double* cache, double* work, void* stream) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && cache, SVGP_ERR_INVALID, "NULL device pointer");
    const CacheWork cw = cache_work(c);
    SVGP_REQUIRE(cw.total == 0 || work, SVGP_ERR_INVALID, "work is NULL (m = %d needs %lld doubles)", c->m, (long long)cw.total);
    svgp_mnist_param_layout pl;
    rc = svgp_mnist_param_layout_get(c, &pl);
    if (rc) return rc;
    svgp_mnist_cache_layout cl;
    cache_layout_fill(c, &cl);
    const int m = c->m, L = c->L;
    if (m <= SVGP_M_MAX)
        return svgp_cache_build_small(c, pl, theta, cache + cl.acc_S, cache + cl.acc_v, cache + cl.acc_rows, cache + cl.w, cache + cl.X, stream);
    const double* ip = theta + pl.ip;
    rc = svgp_kernel_matrix_xy(c->M, c->normalize_obj, m, ip, 0, m, ip, 0, nullptr, theta + pl.l_GP, theta + pl.amplitude, 0, work + cw.K, stream);
    if (rc) return rc;
    const long long tot = (long long)(L + 1) * m * m;
    hipLaunchKernelGGL(k_cache_sigma, dim3(svgp_blocks(tot)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, m, L,
                       (real)c->N_train, (real)c->jitter, work + cw.K, cache + cl.acc_S, cache + cl.acc_rows, work + cw.B);
    SVGP_LAUNCH_CHECK();
    rc = svgp_spd_inverse_batched(m, L + 1, work + cw.B, work + cw.logdet, work + cw.inv, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cache_finish, dim3(m, L), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, m, L, (real)c->N_train, work + cw.B,
                       cache + cl.acc_v, cache + cl.acc_rows, cache + cl.w, cache + cl.X);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" long long svgp_mnist_generate_workspace_elems(const svgp_mnist_cfg* c) {
    if (svgp_check_cfg(c)) return 0;
    return gen_work(c).total;
}

extern "C" int svgp_mnist_generate_route(const svgp_mnist_cfg* c, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    GenOp ops[8];
    const int n = gen_plan(c, ops);
    int pos = 0;
    buf[0] = 0;
    for (int i = 0; i < n && !rc; ++i) rc = svgp_route_append(buf, cap, &pos, "%s\n", GEN_NAME[ops[i]]);
    return rc;
}

extern "C" int svgp_mnist_generate(const svgp_mnist_cfg* c, const double* theta, const double* cache, const double* aux, int gather,
                                   const double* eps, double* images_out, double* p_m_out, double* p_v_out, double* work, void* stream) {
    int rc = svgp_check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && cache && aux && images_out, SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(!gather || c->n_obj > 0, SVGP_ERR_INVALID, "gather needs an object-vector table (n_obj = %d)", c->n_obj);
    const GenWork gw = gen_work(c);
    SVGP_REQUIRE(gw.total == 0 || work, SVGP_ERR_INVALID, "work is NULL (m = %d needs %lld doubles)", c->m, (long long)gw.total);
    svgp_mnist_param_layout pl;
    rc = svgp_mnist_param_layout_get(c, &pl);
    if (rc) return rc;
    svgp_mnist_cache_layout cl;
    cache_layout_fill(c, &cl);
    const int b = c->b, m = c->m, L = c->L;
    GenArgs a;
    a.b = b; a.m = m; a.L = L; a.M = c->M; a.n_obj = c->n_obj; a.normalize = c->normalize_obj; a.gather = gather != 0;
    a.th_dec = theta + pl.n_enc; a.aux = aux; a.ip = theta + pl.ip; a.ov = theta + pl.ov; a.ls = theta + pl.l_GP; a.amp = theta + pl.amplitude;
    a.w = cache + cl.w; a.X = cache + cl.X; a.eps = eps; a.z = work ? work + gw.z : nullptr;
    a.images = images_out; a.p_m = p_m_out; a.p_v = p_v_out;
    const int64_t n_dec = pl.n_vae - pl.n_enc;
    const size_t lds_dec = (size_t)dec_fwd_lds((int)n_dec, false) * sizeof(real);
    // (the fused form runs for m <= 64 and svgp_check_cfg holds L <= 64: at most 18 954 doubles = 151 632 bytes, asserted above)
    const size_t lds_gp = lds_dec + (size_t)(m + 1 + (int64_t)L * m) * sizeof(real);
    const dim3 grid(svgp_n_part(c));
    hipStream_t st = (hipStream_t)stream;
    GenOp ops[8];
    const int n = gen_plan(c, ops);
    for (int i = 0; i < n; ++i) {
        switch (ops[i]) {
        case GEN_FUSED:
            rc = set_dyn_lds(k_generate<true>, lds_gp);
            if (rc) return rc;
            hipLaunchKernelGGL(k_generate<true>, grid, dim3(VAE_NT), lds_gp, st, a);
            SVGP_LAUNCH_CHECK();
            break;
        case GEN_KX:
            hipLaunchKernelGGL(k_generate_kx, dim3(svgp_blocks((long long)b * m)), dim3(SVGP_BLOCK), 0, st, a,
                               work + gw.Kx);
            SVGP_LAUNCH_CHECK();
            break;
        case GEN_PROD_X:        // P_l (b, m) = K_x X_l
            rc = svgp_dgemm_batched(0, 0, b, m, m, 1.0, work + gw.Kx, m, 0, a.X, m, (long long)m * m, 0.0, work + gw.P, m, (long long)b * m, L, stream);
            if (rc) return rc;
            break;
        case GEN_PROD_W:        // (b, L) = K_x w^T
            rc = svgp_dgemm_batched(0, 1, b, L, m, 1.0, work + gw.Kx, m, 0, a.w, m, 0, 0.0, work + gw.pm, L, 0, 1, stream);
            if (rc) return rc;
            break;
        case GEN_ROWSUM:
            hipLaunchKernelGGL(k_generate_rowsum, dim3(svgp_blocks((long long)b * L)), dim3(SVGP_BLOCK), 0, st, a,
                               work + gw.Kx, work + gw.P, work + gw.pm, work + gw.z);
            SVGP_LAUNCH_CHECK();
            break;
        case GEN_DECODE:
            rc = set_dyn_lds(k_generate<false>, lds_dec);
            if (rc) return rc;
            hipLaunchKernelGGL(k_generate<false>, grid, dim3(VAE_NT), lds_dec, st, a);
            SVGP_LAUNCH_CHECK();
            break;
        }
    }
    return SVGP_OK;
}
