// Casale GP-VAE baseline on rotated MNIST: the GP prior stage in H x H space (H = M Q), its reverse pass, the two latent
// samples of a step with their encoder seeds, the plain-VAE regime's glue and the prediction rows.
// Reference: GPVAE_Casale_model.py (casaleGP.V_matrix :278-309, taylor_coeff :311-351, forward_pass_Casale :96-155,
// predict_test_set_Casale :158-203); include/svgpvae_hip.h has the restatement these kernels evaluate.
//
// Dense products are the library's GEMMs (svgp_dgemm_batched, svgp_dgemm_splitk for the contractions over the N rows) and
// svgp_spd_inverse_batched; everything row-wise, the V build with its VJP and the Q x Q Cholesky with its VJP are the
// kernels below.  All sums have a fixed order (row partials + one closing workgroup): no float atomics.
#include "common.hpp"

namespace {

#define CAS_QMAX 32
#define CAS_CHUNK 64           // rows per workgroup of the L_W gradient partials

// ---------------------------------------------------------------------------------------------------------------
// K_W = amp^2 exp(-2 sin^2((a_i - a_j) / 2) / l^2) on the Q unique angles and its Cholesky factor; one workgroup
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGP_BLOCK) void k_kw_chol(int Q, const real* __restrict__ ang, const real* __restrict__ gp,
                                                        real* __restrict__ KW, real* __restrict__ LW) {
    __shared__ real Ls[CAS_QMAX][CAS_QMAX + 1];
    const real ls = gp[0], amp = gp[1], a2 = amp * amp, inv_l2 = real(1) / (ls * ls);
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {
        const int i = e / Q, j = e % Q;
        const real k = svgp_view_k(ang[i] - ang[j], a2, inv_l2);
        KW[e] = k;
        Ls[i][j] = k;
    }
    __syncthreads();
    for (int j = 0; j < Q; ++j) {          // right-looking, column by column
        if (threadIdx.x == 0) Ls[j][j] = sqrt(Ls[j][j]);
        __syncthreads();
        const real d = Ls[j][j];
        for (int i = j + 1 + threadIdx.x; i < Q; i += blockDim.x) Ls[i][j] /= d;
        __syncthreads();
        const int n = Q - j - 1;
        for (int e = threadIdx.x; e < n * n; e += blockDim.x) {
            const int i = j + 1 + e / n, k = j + 1 + e % n;
            if (k <= i) Ls[i][k] -= Ls[i][j] * Ls[k][j];
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {
        const int i = e / Q, j = e % Q;
        LW[e] = j <= i ? Ls[i][j] : real(0);
    }
}

__device__ __forceinline__ real cas_inv_norm(const real* o, int M, int normalize) {
    return normalize ? real(1) / sqrt(svgp_dotM(o, o, M)) : real(1);
}

// V[i, k Q + r] = ov[p_i, k] (/ |ov[p_i]|) L_W[q_i, r]
__global__ __launch_bounds__(SVGP_BLOCK) void k_v_build(int N, int Q, int M, int normalize, const real* __restrict__ ov,
                                                        const real* __restrict__ LW, const int* __restrict__ pi,
                                                        const int* __restrict__ qi, real* __restrict__ V) {
    const int H = M * Q;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)N * H) return;
    const int i = (int)(idx / H), h = (int)(idx % H), k = h / Q, r = h % Q;
    const real* o = ov + (size_t)pi[i] * M;
    V[idx] = o[k] * cas_inv_norm(o, M, normalize) * LW[qi[i] * Q + r];
}

// P = G + alpha I (the matrix the inverse overwrites)
__global__ __launch_bounds__(SVGP_BLOCK) void k_p_init(int H, const real* __restrict__ G, const real* __restrict__ alpha,
                                                       real* __restrict__ P) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)H * H) return;
    P[idx] = G[idx] + ((idx / H) == (idx % H) ? *alpha : real(0));
}
// X[i][i] += c1 * alpha
__global__ __launch_bounds__(SVGP_BLOCK) void k_add_diag(int H, real c1, const real* __restrict__ alpha, real* __restrict__ X) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H) X[(size_t)i * H + i] += c1 * *alpha;
}

// ---------------------------------------------------------------------------------------------------------------
// forward row kernel: one wave per row.  VU = V[i] U, A = (Z - VU) / alpha, partials [zb A, -A VU, (V P) V, A^2]
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGP_BLOCK) void k_rows_fwd(int N, int H, int L, int lo, int hi, const real* __restrict__ V,
                                                         const real* __restrict__ U, const real* __restrict__ Z,
                                                         const real* __restrict__ zb, const real* __restrict__ VPb,
                                                         const real* __restrict__ alpha, real* __restrict__ VU,
                                                         real* __restrict__ A, real* __restrict__ part) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (SVGP_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    const real* v = V + (size_t)i * H;
    const bool inb = i >= lo && i < hi;
    real s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    if (lane < L) {
        real vu = 0;
        for (int h = 0; h < H; ++h) vu += v[h] * U[(size_t)h * L + lane];
        const real a = (Z[(size_t)i * L + lane] - vu) / *alpha;
        VU[(size_t)i * L + lane] = vu;
        A[(size_t)i * L + lane] = a;
        s4 = a * a;
        if (inb) { s1 = zb[(size_t)(i - lo) * L + lane] * a; s2 = -a * vu; }
    }
    if (inb) {
        const real* vp = VPb + (size_t)(i - lo) * H;
        for (int h = lane; h < H; h += 64) s3 += vp[h] * v[h];
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); s4 = wave_sum(s4);
    if (lane == 0) {
        real* p = part + (size_t)i * 4;
        p[0] = s1; p[1] = s2; p[2] = s3 * (real)L; p[3] = s4;
    }
}

// terms = [sum zb A, -sum A VU, L sum (V P) V, |A|^2, tr P, tr K_inv, sum(c), GP_prior_term]; one workgroup
__global__ __launch_bounds__(SVGP_BLOCK) void k_fwd_final(int N, int H, int L, const real* __restrict__ part,
                                                          const real* __restrict__ P, const real* __restrict__ alpha,
                                                          real* __restrict__ terms) {
    __shared__ real red[16];
    real s[5] = {0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < N; i += blockDim.x)
        for (int k = 0; k < 4; ++k) s[k] += part[(size_t)i * 4 + k];
    for (int h = threadIdx.x; h < H; h += blockDim.x) s[4] += P[(size_t)h * H + h];
    for (int k = 0; k < 5; ++k) s[k] = block_sum(s[k], red);
    if (threadIdx.x == 0) {
        const real al = *alpha, trKinv = (real)(N - H) / al + s[4];
        const real csum = real(0.5) * (-s[3] + (real)L * trKinv);
        terms[0] = s[0]; terms[1] = s[1]; terms[2] = s[2]; terms[3] = s[3]; terms[4] = s[4]; terms[5] = trKinv;
        terms[6] = csum; terms[7] = s[0] + s[1] + s[2] + al * csum;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// reverse row kernel: one wave per row.  Abar, zbbar, Zbar = Abar / alpha, Cm = -Abar / alpha - [idx] seed A (so that
// Ubar = V^T Cm), Vbar = Cm U^T + [idx] 2 seed L V P, and the row partial of alphabar (-Abar . A / alpha)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGP_BLOCK) void k_rows_bwd(int N, int H, int L, int lo, int hi, real seed,
                                                         const real* __restrict__ U, const real* __restrict__ zb,
                                                         const real* __restrict__ VPb, const real* __restrict__ VU,
                                                         const real* __restrict__ A, const real* __restrict__ alpha,
                                                         real* __restrict__ Abar, real* __restrict__ Cm,
                                                         real* __restrict__ Zbar, real* __restrict__ zbbar,
                                                         real* __restrict__ Vbar, real* __restrict__ part_alpha) {
    __shared__ real cms[SVGP_BLOCK / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * (SVGP_BLOCK / 64) + w;
    const bool live = i < N, inb = live && i >= lo && i < hi;
    const real al = *alpha;
    real pa = 0;
    if (live && lane < L) {
        const size_t o = (size_t)i * L + lane;
        const real a = A[o];
        real ab = -seed * al * a;
        if (inb) {
            ab += seed * (zb[(size_t)(i - lo) * L + lane] - VU[o]);
            zbbar[(size_t)(i - lo) * L + lane] = seed * a;
        }
        const real cm = -ab / al - (inb ? seed * a : real(0));
        Abar[o] = ab; Zbar[o] = ab / al; Cm[o] = cm;
        cms[w][lane] = cm;
        pa = -ab * a / al;
    }
    __syncthreads();
    if (!live) return;
    pa = wave_sum(pa);
    if (lane == 0) part_alpha[i] = pa;
    const real f = real(2) * seed * (real)L;
    for (int h = lane; h < H; h += 64) {
        real acc = inb ? f * VPb[(size_t)(i - lo) * H + h] : real(0);
        for (int l = 0; l < L; ++l) acc += cms[w][l] * U[(size_t)h * L + l];
        Vbar[(size_t)i * H + h] = acc;
    }
}

// Mbar <- Mbar + Mbar^T in place: the thread of (i, j), j < i, owns both elements of its pair; the diagonal doubles
__global__ __launch_bounds__(SVGP_BLOCK) void k_msym(int H, real* __restrict__ Mb) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)H * H) return;
    const int i = (int)(idx / H), j = (int)(idx % H);
    if (j < i) {
        const real s = Mb[(size_t)i * H + j] + Mb[(size_t)j * H + i];
        Mb[(size_t)i * H + j] = s;
        Mb[(size_t)j * H + i] = s;
    } else if (j == i) {
        Mb[idx] *= real(2);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// VJP of the V build.  Object table: one workgroup (128 threads, thread k) per table row p; its rows are the contiguous
// range found by bisection in the non-decreasing obj_idx; summed in row order.  Through the normalisation:
// ovbar = (g - on (on . g)) / |ov|.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_ov_bwd(int N, int Q, int M, int normalize, int train_ov, const real* __restrict__ ov,
                                                const real* __restrict__ LW, const int* __restrict__ pi,
                                                const int* __restrict__ qi, const real* __restrict__ Vbar,
                                                real* __restrict__ ovbar) {
    __shared__ real red[16];
    __shared__ real dotv;
    const int p = blockIdx.x, k = threadIdx.x, H = M * Q;
    if (!train_ov) { if (k < M) ovbar[(size_t)p * M + k] = 0; return; }
    int a = 0, b = N;                       // first row with obj_idx >= p
    while (a < b) { const int m = (a + b) >> 1; if (pi[m] < p) a = m + 1; else b = m; }
    const int r0 = a;
    b = N;                                  // first row with obj_idx > p
    while (a < b) { const int m = (a + b) >> 1; if (pi[m] <= p) a = m + 1; else b = m; }
    const int r1 = a;
    real g = 0;
    if (k < M)
        for (int i = r0; i < r1; ++i) {
            const real* vb = Vbar + (size_t)i * H + (size_t)k * Q;
            const real* lw = LW + (size_t)qi[i] * Q;
            real s = 0;
            for (int r = 0; r < Q; ++r) s += vb[r] * lw[r];
            g += s;
        }
    if (normalize) {
        const real* o = ov + (size_t)p * M;
        const real inv = cas_inv_norm(o, M, 1);
        const real d = block_sum(k < M ? g * o[k] * inv : real(0), red);
        if (threadIdx.x == 0) dotv = d;
        __syncthreads();
        if (k < M) g = (g - o[k] * inv * dotv) * inv;
    }
    if (k < M) ovbar[(size_t)p * M + k] = g;
}

// L_W gradient partials: workgroup c takes rows [c CHUNK, (c + 1) CHUNK); element (q, r) = sum over its rows with
// ang_idx = q, in row order, of sum_k Vbar[i, k Q + r] on[p_i, k]
__global__ __launch_bounds__(SVGP_BLOCK) void k_lw_part(int N, int Q, int M, int normalize, const real* __restrict__ ov,
                                                        const int* __restrict__ pi, const int* __restrict__ qi,
                                                        const real* __restrict__ Vbar, real* __restrict__ part) {
    __shared__ real inv[CAS_CHUNK];
    const int i0 = blockIdx.x * CAS_CHUNK, cnt = min(CAS_CHUNK, N - i0), H = M * Q;
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) inv[t] = cas_inv_norm(ov + (size_t)pi[i0 + t] * M, M, normalize);
    __syncthreads();
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {
        const int q = e / Q, r = e % Q;
        real acc = 0;
        for (int t = 0; t < cnt; ++t) {
            const int i = i0 + t;
            if (qi[i] != q) continue;
            const real* o = ov + (size_t)pi[i] * M;
            const real* vb = Vbar + (size_t)i * H + r;
            real s = 0;
            for (int k = 0; k < M; ++k) s += vb[(size_t)k * Q] * o[k];
            acc += s * inv[t];
        }
        part[(size_t)blockIdx.x * Q * Q + e] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// closing workgroup of the reverse pass: Lbar = tril(sum of partials); Cholesky VJP Kbar = sym(L^-T Phi(L^T Lbar) L^-1);
// kernel VJP into l_GP, amplitude; alphabar from its four parts
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SVGP_BLOCK) void k_chol_bwd(int N, int H, int L, int Q, int n_chunk, int train_gp, real seed,
                                                         const real* __restrict__ ang, const real* __restrict__ gp,
                                                         const real* __restrict__ KW, const real* __restrict__ LW,
                                                         const real* __restrict__ part, const real* __restrict__ part_alpha,
                                                         const real* __restrict__ Msym, const real* __restrict__ terms,
                                                         real* __restrict__ LWbar, real* __restrict__ KWbar,
                                                         real* __restrict__ trM_out, real* __restrict__ grad) {
    __shared__ real Ls[CAS_QMAX][CAS_QMAX + 1], Lb[CAS_QMAX][CAS_QMAX + 1], X[CAS_QMAX][CAS_QMAX + 1], S[CAS_QMAX][CAS_QMAX + 1];
    __shared__ real red[16];
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {
        const int i = e / Q, j = e % Q;
        real acc = 0;
        for (int c = 0; c < n_chunk; ++c) acc += part[(size_t)c * Q * Q + e];
        if (j > i) acc = 0;                 // V reads the zeros above the diagonal of L_W: no gradient flows there
        LWbar[e] = acc;
        Lb[i][j] = acc;
        Ls[i][j] = LW[e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {          // X = Phi(L^T Lbar)
        const int i = e / Q, j = e % Q;
        real acc = 0;
        if (j <= i)
            for (int k = i; k < Q; ++k) acc += Ls[k][i] * Lb[k][j];
        X[i][j] = j < i ? acc : (j == i ? real(0.5) * acc : real(0));
    }
    __syncthreads();
    if ((int)threadIdx.x < Q) {              // L^T Y = X, column j = threadIdx.x, back substitution (in place)
        const int j = threadIdx.x;
        for (int i = Q - 1; i >= 0; --i) {
            real acc = X[i][j];
            for (int k = i + 1; k < Q; ++k) acc -= Ls[k][i] * X[k][j];
            X[i][j] = acc / Ls[i][i];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < Q) {              // S L = Y, row i = threadIdx.x
        const int i = threadIdx.x;
        for (int j = Q - 1; j >= 0; --j) {
            real acc = X[i][j];
            for (int k = j + 1; k < Q; ++k) acc -= S[i][k] * Ls[k][j];
            S[i][j] = acc / Ls[j][j];
        }
    }
    __syncthreads();
    const real ls = gp[0], amp = gp[1], al = gp[2];
    real g_ls = 0, g_amp = 0;
    for (int e = threadIdx.x; e < Q * Q; e += blockDim.x) {
        const int i = e / Q, j = e % Q;
        const real kb = real(0.5) * (S[i][j] + S[j][i]);
        KWbar[e] = kb;
        const real sn = sin(real(0.5) * (ang[i] - ang[j])), k = KW[e];
        g_ls += kb * k * real(4) * sn * sn / (ls * ls * ls);
        g_amp += kb * k * real(2) / amp;
    }
    g_ls = block_sum(g_ls, red);
    g_amp = block_sum(g_amp, red);
    real pa = 0, tm = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) pa += part_alpha[i];
    for (int h = threadIdx.x; h < H; h += blockDim.x) tm += real(0.5) * Msym[(size_t)h * H + h];
    pa = block_sum(pa, red);
    tm = block_sum(tm, red);
    if (threadIdx.x == 0) {
        *trM_out = tm;
        const real direct = seed * (real(0.5) * (-terms[3] + (real)L * terms[5]) - (real)L * (real)(N - H) / (real(2) * al));
        grad[0] = train_gp ? g_ls : real(0);
        grad[1] = train_gp ? g_amp : real(0);
        grad[2] = train_gp ? direct + pa + tm : real(0);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the two samples of a step from one encoder pass (mu, var_raw over all N rows) and log_var of the batch
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cas_pass(int clip, real vr, real hi) { return !clip || (vr >= 1e-3 && vr <= hi); }

__global__ __launch_bounds__(SVGP_BLOCK) void k_sample(int N, int L, int clip, int lo, int hi, const real* __restrict__ mu,
                                                       const real* __restrict__ var_raw, const real* __restrict__ eps_f,
                                                       const real* __restrict__ eps_b, real* __restrict__ Z,
                                                       real* __restrict__ zb, real* __restrict__ z_dec,
                                                       real* __restrict__ qvar_b, real* __restrict__ lv_part) {
    __shared__ real red[16];
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    real lv = 0;
    if (idx < (long long)N * L) {
        const int i = (int)(idx / L), l = (int)(idx % L);
        const real vr = var_raw[idx], m = mu[idx];
        const real v1 = clip ? clip_keep_nan(vr, 1e-3, 10.0) : vr;
        Z[idx] = m + eps_f[idx] * sqrt(v1);
        if (i >= lo && i < hi) {
            const size_t o = (size_t)(i - lo) * L + l;
            const real v2 = clip ? clip_keep_nan(vr, 1e-3, 100.0) : vr;
            const real z = m + eps_b[o] * sqrt(v2);
            zb[o] = z; z_dec[o] = z; qvar_b[o] = v2;
            lv = log(v2);
        }
    }
    lv = block_sum(lv, red);
    if (threadIdx.x == 0) lv_part[blockIdx.x] = lv;
}

// seed w.r.t. (mu, var_raw) of all N rows: Zbar through the full-set sample, [idx] the decoder's zbar + the GP stage's
// zbbar through the batch sample, and c_logvar d log(var_b)
__global__ __launch_bounds__(SVGP_BLOCK) void k_seeds(int N, int L, int clip, int lo, int hi, real c_lv,
                                                      const real* __restrict__ var_raw, const real* __restrict__ eps_f,
                                                      const real* __restrict__ eps_b, const real* __restrict__ Zbar,
                                                      const real* __restrict__ zbbar, const real* __restrict__ dec_zbar,
                                                      real* __restrict__ ybar, real* __restrict__ s2bar) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)N * L) return;
    const int i = (int)(idx / L), l = (int)(idx % L);
    const real vr = var_raw[idx], zbr = Zbar[idx];
    real yb = zbr, sb = 0;
    if (cas_pass(clip, vr, 10.0)) sb = zbr * eps_f[idx] / (real(2) * sqrt(clip ? clip_keep_nan(vr, 1e-3, 10.0) : vr));
    if (i >= lo && i < hi) {
        const size_t o = (size_t)(i - lo) * L + l;
        const real zt = dec_zbar[o] + zbbar[o];
        yb += zt;
        if (cas_pass(clip, vr, 100.0)) sb += zt * eps_b[o] / (real(2) * sqrt(vr)) + c_lv / vr;
    }
    ybar[idx] = yb;
    s2bar[idx] = sb;
}

// plain-VAE regime (SVGPVAE_model.py:746-776, no clipping): z = mu + eps sqrt(var); KL partials
__global__ __launch_bounds__(SVGP_BLOCK) void k_vae_sample(long long n, const real* __restrict__ mu,
                                                           const real* __restrict__ var, const real* __restrict__ eps,
                                                           real* __restrict__ z, real* __restrict__ kl_part) {
    __shared__ real red[16];
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    real kl = 0;
    if (idx < n) {
        const real m = mu[idx], v = var[idx];
        z[idx] = m + eps[idx] * sqrt(v);
        kl = real(0.5) * (v + m * m - real(1) - log(v));
    }
    kl = block_sum(kl, red);
    if (threadIdx.x == 0) kl_part[blockIdx.x] = kl;
}
// seeds of -elbo_VAE = scale / 784 * recon sq + KL: the decoder's zbar carries 1 / 784
__global__ __launch_bounds__(SVGP_BLOCK) void k_vae_seeds(long long n, real scale, const real* __restrict__ mu,
                                                          const real* __restrict__ var, const real* __restrict__ eps,
                                                          const real* __restrict__ dec_zbar, real* __restrict__ ybar,
                                                          real* __restrict__ s2bar) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const real zt = scale * dec_zbar[idx], v = var[idx];
    ybar[idx] = zt + mu[idx];
    s2bar[idx] = zt * eps[idx] / (real(2) * sqrt(v)) + real(0.5) * (real(1) - real(1) / v);
}

__global__ void k_cas_finalize(int mode, int L, int n_lv, real beta, real sigma_vae, int did_adam, const real* __restrict__ dec_sums,
                               const real* __restrict__ terms, const real* __restrict__ lv_part, real* __restrict__ out,
                               real* __restrict__ state) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    real lv = 0;
    for (int i = 0; i < n_lv; ++i) lv += lv_part[i];
    const real sq = dec_sums[2];
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (mode == 0) {         // GPVAE_Casale_model.py:150-153
        out[0] = sq / real(784) - (beta / (real)L) * (terms[7] + real(0.5) * lv);
        out[1] = sq / real(784); out[2] = terms[7]; out[3] = lv;
    } else {                 // SVGPVAE_model.py:776-780
        out[0] = -(real(0.5) / (sigma_vae * sigma_vae)) * sq - lv;
        out[1] = sq / real(784); out[4] = lv;
    }
    if (did_adam) state[SVGP_ST_ADAM_T] += real(1);
}

// var_i = k_ii - (|k_i|^2 - r_i . (P r_i)) / alpha; one wave per test row
__global__ __launch_bounds__(SVGP_BLOCK) void k_predict_var(int T, int N, int H, const real* __restrict__ Ktn,
                                                            const real* __restrict__ ktt, const real* __restrict__ R,
                                                            const real* __restrict__ RP, const real* __restrict__ alpha,
                                                            real* __restrict__ var) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * (SVGP_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= T) return;
    real kk = 0, rr = 0;
    for (int j = lane; j < N; j += 64) { const real k = Ktn[(size_t)i * N + j]; kk += k * k; }
    for (int h = lane; h < H; h += 64) rr += R[(size_t)i * H + h] * RP[(size_t)i * H + h];
    kk = wave_sum(kk); rr = wave_sum(rr);
    if (lane == 0) var[i] = ktt[i] - (kk - rr) / *alpha;
}

__global__ __launch_bounds__(SVGP_BLOCK) void k_scale(long long n, real f, real* __restrict__ x) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) x[idx] *= f;
}


int check_cfg(const svgp_casale_cfg* c) {
    SVGP_REQUIRE(c != nullptr, SVGP_ERR_INVALID, "casale cfg is NULL");
    SVGP_REQUIRE(c->N >= 1 && c->n_obj >= 1 && c->Q >= 1 && c->M >= 1 && c->L >= 1 && c->b_cap >= 1 && c->b_cap <= c->N,
                 SVGP_ERR_INVALID, "bad Casale shape N=%d n_obj=%d Q=%d M=%d L=%d b_cap=%d", c->N, c->n_obj, c->Q, c->M, c->L,
                 c->b_cap);
    SVGP_REQUIRE(c->Q <= CAS_QMAX, SVGP_ERR_UNSUPPORTED, "Q=%d unique angles: the one-workgroup Cholesky supports Q <= %d",
                 c->Q, CAS_QMAX);
    SVGP_REQUIRE(c->M <= 128, SVGP_ERR_UNSUPPORTED, "M=%d: object-vector dimension > 128 not supported", c->M);
    SVGP_REQUIRE((long long)c->M * c->Q <= SVGP_M_LIMIT, SVGP_ERR_UNSUPPORTED, "H = M Q = %lld: this build supports H <= %d",
                 (long long)c->M * c->Q, SVGP_M_LIMIT);
    SVGP_REQUIRE(c->L <= 64, SVGP_ERR_UNSUPPORTED, "L=%d: more than 64 latent channels not supported", c->L);
    return SVGP_OK;
}
int check_range(const svgp_casale_cfg* c, int lo, int hi) {
    SVGP_REQUIRE(lo >= 0 && hi > lo && hi <= c->N, SVGP_ERR_INVALID, "batch range [%d, %d) outside [0, N = %d]", lo, hi, c->N);
    SVGP_REQUIRE(hi - lo <= c->b_cap, SVGP_ERR_INVALID, "batch of %d rows exceeds b_cap=%d", hi - lo, c->b_cap);
    return SVGP_OK;
}

}  // namespace

extern "C" int svgp_casale_layout_get(const svgp_casale_cfg* c, svgp_casale_layout* o) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(o != nullptr, SVGP_ERR_INVALID, "out is NULL");
    const int64_t N = c->N, Q = c->Q, M = c->M, L = c->L, H = M * Q, b = c->b_cap;
    // the VAE prefix of theta is the MNIST step's (its layout does not depend on the GP part: m = M = 1, no object table)
    svgp_mnist_cfg vc = {};
    vc.b = vc.b_global = 1; vc.m = 1; vc.M = 1; vc.L = c->L; vc.N_train = 1.0;
    svgp_mnist_param_layout pl;
    rc = svgp_mnist_param_layout_get(&vc, &pl);
    if (rc) return rc;
    o->n_enc = pl.n_enc;
    o->n_vae = pl.n_vae;
    o->th_l_GP = o->n_vae; o->th_amplitude = o->n_vae + 1; o->th_alpha = o->n_vae + 2; o->th_ov = o->n_vae + 3;
    o->n_total = o->th_ov + (int64_t)c->n_obj * M;
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += (n + 15) / 16 * 16; return r; };
    o->K_W = take(Q * Q); o->L_W = take(Q * Q);
    o->V = take(N * H); o->G = take(H * H); o->P = take(H * H); o->W = take(H * L); o->U = take(H * L);
    o->VU = take(N * L); o->A = take(N * L); o->VPb = take(b * H);
    o->Z = take(N * L); o->zb = take(b * L); o->qvar_b = take(b * L);
    o->part = take(N * 4); o->terms = take(8);
    o->n_lv = (N * L + SVGP_BLOCK - 1) / SVGP_BLOCK; o->lv_part = take(o->n_lv);
    o->Abar = take(N * L); o->Cm = take(N * L); o->Zbar = take(N * L); o->zbbar = take(b * L); o->Vbar = take(N * H);
    o->Ubar = take(H * L); o->Pbar = take(H * H); o->Wbar = take(H * L); o->T = take(H * H); o->Mbar = take(H * H);
    o->part_alpha = take(N); o->trM = take(1);
    o->n_chunk = (N + CAS_CHUNK - 1) / CAS_CHUNK;
    o->LWbar_part = take(o->n_chunk * Q * Q); o->LWbar = take(Q * Q); o->KWbar = take(Q * Q);
    o->grad_gp = take(3 + (int64_t)c->n_obj * M);
    o->logdet = take(1);
    o->scr_inv = take((int64_t)svgp_spd_inverse_workspace_elems((int)H, 1));
    const long long s1 = svgp_dgemm_splitk_scratch_elems((int)H, (int)H, (int)N), s2 = svgp_dgemm_splitk_scratch_elems((int)H, (int)L, (int)N);
    o->scr_splitk_len = s1 > s2 ? s1 : s2;
    o->scr_splitk = take(o->scr_splitk_len);
    o->total = p;
    return SVGP_OK;
}

#define CAS_LAYOUT()                                   \
    svgp_casale_layout wl;                             \
    {                                                  \
        int rc_ = svgp_casale_layout_get(c, &wl);      \
        if (rc_) return rc_;                           \
    }
#define CAS_GEMM(...)                                  \
    do {                                               \
        int rc_ = svgp_dgemm_batched(__VA_ARGS__);     \
        if (rc_) return rc_;                           \
    } while (0)

extern "C" int svgp_casale_v_fwd(const svgp_casale_cfg* c, const double* gp, const double* angles, const int32_t* obj_idx,
                                 const int32_t* ang_idx, double* ws, void* stream) {
    CAS_LAYOUT();
    SVGP_REQUIRE(gp && angles && obj_idx && ang_idx && ws, SVGP_ERR_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = c->N, Q = c->Q, M = c->M, H = M * Q;
    hipLaunchKernelGGL(k_kw_chol, dim3(1), dim3(SVGP_BLOCK), 0, s, Q, angles, gp, ws + wl.K_W, ws + wl.L_W);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_v_build, dim3(svgp_blocks((long long)N * H)), dim3(SVGP_BLOCK), 0, s, N, Q, M, c->normalize_obj, gp + 3,
                       ws + wl.L_W, obj_idx, ang_idx, ws + wl.V);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

// The front half of svgp_casale_gp_fwd, which is all the posterior cache needs (casale_generate.hip): K_W, L_W, V, G, P, W, U
// from the latent rows Z; no batch range, no row kernel.  The caller has validated cfg and pointers.
int svgp_casale_hspace_fwd(const svgp_casale_cfg* c, const svgp_casale_layout& wl, const double* gp, const double* angles,
                           const int32_t* obj_idx, const int32_t* ang_idx, const double* Z, double* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int N = c->N, L = c->L, H = c->M * c->Q;
    const real* alpha = gp + 2;
    real *V = ws + wl.V, *P = ws + wl.P, *U = ws + wl.U;
    int rc = svgp_casale_v_fwd(c, gp, angles, obj_idx, ang_idx, ws, stream);
    if (rc) return rc;
    rc = svgp_dgemm_splitk(1, 0, H, H, N, 1.0, V, H, V, H, 0.0, ws + wl.G, H, ws + wl.scr_splitk, wl.scr_splitk_len, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_p_init, dim3(svgp_blocks((long long)H * H)), dim3(SVGP_BLOCK), 0, s, H, ws + wl.G, alpha, P);
    SVGP_LAUNCH_CHECK();
    rc = svgp_spd_inverse_batched(H, 1, P, ws + wl.logdet, ws + wl.scr_inv, stream);
    if (rc) return rc;
    rc = svgp_dgemm_splitk(1, 0, H, L, N, 1.0, V, H, Z, L, 0.0, ws + wl.W, L, ws + wl.scr_splitk, wl.scr_splitk_len, stream);
    if (rc) return rc;
    CAS_GEMM(0, 0, H, L, H, 1.0, P, H, 0, ws + wl.W, L, 0, 0.0, U, L, 0, 1, stream);
    return SVGP_OK;
}

extern "C" int svgp_casale_gp_fwd(const svgp_casale_cfg* c, const double* gp, const double* angles, const int32_t* obj_idx,
                                  const int32_t* ang_idx, const double* Z, const double* zb, int lo, int hi, double* ws,
                                  void* stream) {
    CAS_LAYOUT();
    int rc = check_range(c, lo, hi);
    if (rc) return rc;
    SVGP_REQUIRE(gp && angles && obj_idx && ang_idx && Z && zb && ws, SVGP_ERR_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = c->N, L = c->L, H = c->M * c->Q, b = hi - lo;
    const real* alpha = gp + 2;
    real *V = ws + wl.V, *P = ws + wl.P, *U = ws + wl.U;
    rc = svgp_casale_hspace_fwd(c, wl, gp, angles, obj_idx, ang_idx, Z, ws, stream);
    if (rc) return rc;
    CAS_GEMM(0, 0, b, H, H, 1.0, V + (size_t)lo * H, H, 0, P, H, 0, 0.0, ws + wl.VPb, H, 0, 1, stream);
    hipLaunchKernelGGL(k_rows_fwd, dim3((N + 3) / 4), dim3(SVGP_BLOCK), 0, s, N, H, L, lo, hi, V, U, Z, zb, ws + wl.VPb, alpha,
                       ws + wl.VU, ws + wl.A, ws + wl.part);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fwd_final, dim3(1), dim3(SVGP_BLOCK), 0, s, N, H, L, ws + wl.part, P, alpha, ws + wl.terms);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_gp_bwd(const svgp_casale_cfg* c, const double* gp, const double* angles, const int32_t* obj_idx,
                                  const int32_t* ang_idx, const double* Z, const double* zb, int lo, int hi, double seed,
                                  double* ws, void* stream) {
    CAS_LAYOUT();
    int rc = check_range(c, lo, hi);
    if (rc) return rc;
    SVGP_REQUIRE(gp && angles && obj_idx && ang_idx && Z && zb && ws, SVGP_ERR_INVALID, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int N = c->N, Q = c->Q, M = c->M, L = c->L, H = M * Q, b = hi - lo;
    const real* alpha = gp + 2;
    real *V = ws + wl.V, *P = ws + wl.P, *U = ws + wl.U, *W = ws + wl.W, *Vbar = ws + wl.Vbar, *Zbar = ws + wl.Zbar;
    real *Ubar = ws + wl.Ubar, *Pbar = ws + wl.Pbar, *Wbar = ws + wl.Wbar, *T = ws + wl.T, *Mb = ws + wl.Mbar;
    hipLaunchKernelGGL(k_rows_bwd, dim3((N + 3) / 4), dim3(SVGP_BLOCK), 0, s, N, H, L, lo, hi, seed, U, zb, ws + wl.VPb,
                       ws + wl.VU, ws + wl.A, alpha, ws + wl.Abar, ws + wl.Cm, Zbar, ws + wl.zbbar, Vbar, ws + wl.part_alpha);
    SVGP_LAUNCH_CHECK();
    // Ubar = V^T Cm;  Pbar = seed L V[idx]^T V[idx] + Ubar W^T + seed alpha L / 2 I
    rc = svgp_dgemm_splitk(1, 0, H, L, N, 1.0, V, H, ws + wl.Cm, L, 0.0, Ubar, L, ws + wl.scr_splitk, wl.scr_splitk_len, stream);
    if (rc) return rc;
    const real* Vb = V + (size_t)lo * H;
    CAS_GEMM(1, 0, H, H, b, seed * L, Vb, H, 0, Vb, H, 0, 0.0, Pbar, H, 0, 1, stream);
    CAS_GEMM(0, 1, H, H, L, 1.0, Ubar, L, 0, W, L, 0, 1.0, Pbar, H, 0, 1, stream);
    hipLaunchKernelGGL(k_add_diag, dim3(svgp_blocks(H)), dim3(SVGP_BLOCK), 0, s, H, seed * L * 0.5, alpha, Pbar);
    SVGP_LAUNCH_CHECK();
    // Wbar = P Ubar;  Mbar = -P Pbar P, kept as Mbar + Mbar^T
    CAS_GEMM(0, 0, H, L, H, 1.0, P, H, 0, Ubar, L, 0, 0.0, Wbar, L, 0, 1, stream);
    CAS_GEMM(0, 0, H, H, H, 1.0, Pbar, H, 0, P, H, 0, 0.0, T, H, 0, 1, stream);
    CAS_GEMM(0, 0, H, H, H, -1.0, P, H, 0, T, H, 0, 0.0, Mb, H, 0, 1, stream);
    hipLaunchKernelGGL(k_msym, dim3(svgp_blocks((long long)H * H)), dim3(SVGP_BLOCK), 0, s, H, Mb);
    SVGP_LAUNCH_CHECK();
    // Vbar += V (Mbar + Mbar^T) + Z Wbar^T;  Zbar += V Wbar
    CAS_GEMM(0, 0, N, H, H, 1.0, V, H, 0, Mb, H, 0, 1.0, Vbar, H, 0, 1, stream);
    CAS_GEMM(0, 1, N, H, L, 1.0, Z, L, 0, Wbar, L, 0, 1.0, Vbar, H, 0, 1, stream);
    CAS_GEMM(0, 0, N, L, H, 1.0, V, H, 0, Wbar, L, 0, 1.0, Zbar, L, 0, 1, stream);
    real* grad = ws + wl.grad_gp;
    hipLaunchKernelGGL(k_ov_bwd, dim3(c->n_obj), dim3(128), 0, s, N, Q, M, c->normalize_obj, c->train_ov, gp + 3, ws + wl.L_W,
                       obj_idx, ang_idx, Vbar, grad + 3);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lw_part, dim3((unsigned)wl.n_chunk), dim3(SVGP_BLOCK), 0, s, N, Q, M, c->normalize_obj, gp + 3, obj_idx,
                       ang_idx, Vbar, ws + wl.LWbar_part);
    SVGP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chol_bwd, dim3(1), dim3(SVGP_BLOCK), 0, s, N, H, L, Q, (int)wl.n_chunk, c->train_gp, seed, angles, gp,
                       ws + wl.K_W, ws + wl.L_W, ws + wl.LWbar_part, ws + wl.part_alpha, Mb, ws + wl.terms, ws + wl.LWbar,
                       ws + wl.KWbar, ws + wl.trM, grad);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_sample(const svgp_casale_cfg* c, int clip, int lo, int hi, const double* mu, const double* var_raw,
                                  const double* eps_full, const double* eps_batch, double* z_dec, double* ws, void* stream) {
    CAS_LAYOUT();
    int rc = check_range(c, lo, hi);
    if (rc) return rc;
    SVGP_REQUIRE(mu && var_raw && eps_full && eps_batch && z_dec && ws, SVGP_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(k_sample, dim3((unsigned)wl.n_lv), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, c->N, c->L, clip, lo, hi, mu,
                       var_raw, eps_full, eps_batch, ws + wl.Z, ws + wl.zb, z_dec, ws + wl.qvar_b, ws + wl.lv_part);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_seeds(const svgp_casale_cfg* c, int clip, int lo, int hi, const double* var_raw,
                                 const double* eps_full, const double* eps_batch, const double* dec_zbar, double c_logvar,
                                 double* ybar, double* s2bar, double* ws, void* stream) {
    CAS_LAYOUT();
    int rc = check_range(c, lo, hi);
    if (rc) return rc;
    SVGP_REQUIRE(var_raw && eps_full && eps_batch && dec_zbar && ybar && s2bar && ws, SVGP_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(k_seeds, dim3((unsigned)wl.n_lv), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, c->N, c->L, clip, lo, hi,
                       c_logvar, var_raw, eps_full, eps_batch, ws + wl.Zbar, ws + wl.zbbar, dec_zbar, ybar, s2bar);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_vae_sample(const svgp_casale_cfg* c, int b, const double* mu, const double* var_raw,
                                      const double* eps, double* z_dec, double* ws, void* stream) {
    CAS_LAYOUT();
    SVGP_REQUIRE(b >= 1 && b <= c->b_cap, SVGP_ERR_INVALID, "batch of %d rows outside [1, b_cap = %d]", b, c->b_cap);
    SVGP_REQUIRE(mu && var_raw && eps && z_dec && ws, SVGP_ERR_INVALID, "NULL device pointer");
    const long long n = (long long)b * c->L;
    hipLaunchKernelGGL(k_vae_sample, dim3(svgp_blocks(n)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, n, mu, var_raw, eps, z_dec,
                       ws + wl.lv_part);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_vae_seeds(const svgp_casale_cfg* c, int b, double scale, const double* mu, const double* var_raw,
                                     const double* eps, const double* dec_zbar, double* ybar, double* s2bar, void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(b >= 1 && b <= c->b_cap, SVGP_ERR_INVALID, "batch of %d rows outside [1, b_cap = %d]", b, c->b_cap);
    SVGP_REQUIRE(mu && var_raw && eps && dec_zbar && ybar && s2bar, SVGP_ERR_INVALID, "NULL device pointer");
    const long long n = (long long)b * c->L;
    hipLaunchKernelGGL(k_vae_seeds, dim3(svgp_blocks(n)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, n, scale, mu, var_raw, eps, dec_zbar,
                       ybar, s2bar);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_finalize(const svgp_casale_cfg* c, int mode, int b, double beta, double sigma_vae,
                                    const double* dec_sums, int did_adam, double* ws, double* out, double* state,
                                    void* stream) {
    CAS_LAYOUT();
    SVGP_REQUIRE(mode == 0 || mode == 1, SVGP_ERR_INVALID, "mode %d (0 or 1)", mode);
    SVGP_REQUIRE(b >= 1 && b <= c->b_cap, SVGP_ERR_INVALID, "batch of %d rows outside [1, b_cap = %d]", b, c->b_cap);
    SVGP_REQUIRE(mode == 0 || sigma_vae > 0, SVGP_ERR_INVALID, "sigma_vae = %g (> 0)", sigma_vae);
    SVGP_REQUIRE(dec_sums && ws && out && state, SVGP_ERR_INVALID, "NULL device pointer");
    const int n_lv = mode == 0 ? (int)wl.n_lv : (int)svgp_blocks((long long)b * c->L);
    hipLaunchKernelGGL(k_cas_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, mode, c->L, n_lv, beta, sigma_vae, did_adam,
                       dec_sums,
                       ws + wl.terms, ws + wl.lv_part, out, state);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_casale_predict_var(int T, int N, int H, const double* K_tn, const double* k_tt, const double* R,
                                       const double* RP, const double* alpha, double* var, void* stream) {
    SVGP_REQUIRE(T >= 1 && N >= 1 && H >= 1, SVGP_ERR_INVALID, "bad shape T=%d N=%d H=%d", T, N, H);
    SVGP_REQUIRE(K_tn && k_tt && R && RP && alpha && var, SVGP_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(k_predict_var, dim3((T + 3) / 4), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, T, N, H, K_tn, k_tt, R, RP,
                       alpha, var);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_scale_f64(long long n, double f, double* x, void* stream) {
    SVGP_REQUIRE(n >= 0 && x, SVGP_ERR_INVALID, "NULL device pointer");
    if (n == 0) return SVGP_OK;
    hipLaunchKernelGGL(k_scale, dim3(svgp_blocks(n)), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, n, f, x);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}
