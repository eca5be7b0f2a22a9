// Plain VAE and conditional VAE (mnistCVAE) on rotated MNIST: one image launch per training step.
//
// Reference semantics: forward_pass_standard_VAE_rotated_mnist (SVGPVAE_model.py:718-782), mnistVAE / mnistCVAE
// (VAE_utils.py:99-162, 165-258), KL_term_standard_normal_prior (:261-272), predict_CVAE (SVGPVAE_model.py:785-820),
// the step minimises -elbo (MNIST_experiment.py:205) with TF1 Adam.
//
// A VAE / CVAE step couples the images of a batch only through the sum of the weight gradients, so one workgroup carries an
// image through the whole step -- encoder forward, sample, decoder forward, decoder reverse, encoder reverse -- with every
// activation and pre-activation gradient in LDS (k_cvae_step_images).  What leaves the workgroup: one partial of the
// convolution weight gradients and one [sq, KL] pair per workgroup, and per image the two operand rows of each dense layer's
// weight gradient, which is an outer product ([a3, sin, cos]^T dpre and [z, sin, cos]^T dh0) that the second launch
// (k_cvae_reduce_adam) sums over rows in order.  That keeps the dense accumulators (3 552 doubles at L = 16, 13 056 at L = 64) and
// the dense weights themselves out of LDS, so ONE layout serves every L <= 64: the dense weights are read from global memory
// (L2-resident: every workgroup reads the same rows), four short products per image.
//
// mnistCVAE against mnistVAE: the encoder's first convolution is VALID, so its two constant planes [sin a, cos a] act as a
// per-image bias sin a * sum_taps w[:,:,1,:] + cos a * sum_taps w[:,:,2,:], and their weight gradient is the same for the nine
// taps: sin a (cos a) times the layer's bias gradient of that image.  The decoder's first up-convolution has SAME padding -- the
// planes are not a bias at the border -- so they are materialised: h0 is a (4, 4, 10) tile and the layer an UpConv3 with CIN = 10.
#include "common.hpp"

// Compiler only.  The image loop below runs some thirty phases, each a loop over `threadIdx.x + k NT` whose index arithmetic (pixel,
// channel, tap, parity class: divisions and address sums) does not depend on the image.  Left alone, the optimizer hoists all of it
// out of the image loop and keeps it live across every phase: 256 VGPRs and 600 - 1500 bytes of scratch per lane.  Here every read of
// threadIdx.x, in this file and in the device functions of vae_dev.hpp as this file instantiates them, goes through an empty volatile
// asm, so the arithmetic stays in its phase: 224 / 214 VGPRs, no scratch.  Other translation units are not affected.
struct CvaeTidX {
    __device__ __forceinline__ operator int() const {
        int v = __builtin_amdgcn_workitem_id_x();
        asm volatile("" : "+v"(v));
        return v;
    }
};
struct CvaeTid { CvaeTidX x; };
#define threadIdx (CvaeTid{})
#include "vae_dev.hpp"

namespace {

using namespace svgp_vae;

enum { CVAE_FULL = 0, CVAE_ENCODE = 1, CVAE_DECODE = 2, CVAE_PREDICT = 3 };

// offsets into theta (the reference's variable-creation order) and the derived counts
struct CvaeOff {
    int c1w, c1b, c2w, c2b, c3w, c3b, edw, edb, n_enc, ddw, ddb, dc1w, dc1b, dc2w, dc2b, dc3w, dc3b, n_total;
    int C1, NI, ZW, DC;      // encoder c1 input channels, encoder dense rows, decoder dense rows, decoder c1 input channels
    int n_ec, n_dc, npc;     // convolution parameters of the encoder [0, n_ec) and decoder [dc1w, n_total); npc = n_ec + n_dc
};
__host__ __device__ inline CvaeOff cvae_off(int cvae, int L) {
    CvaeOff o;
    o.C1 = cvae ? 3 : 1; o.NI = cvae ? 34 : 32; o.ZW = L + (cvae ? 2 : 0); o.DC = cvae ? 10 : 8;
    int p = 0;
    o.c1w = p; p += 9 * o.C1 * 8; o.c1b = p; p += 8; o.c2w = p; p += 576; o.c2b = p; p += 8; o.c3w = p; p += 576; o.c3b = p; p += 8;
    o.n_ec = p;
    o.edw = p; p += o.NI * 2 * L; o.edb = p; p += 2 * L; o.n_enc = p;
    o.ddw = p; p += o.ZW * 128; o.ddb = p; p += 128;
    o.dc1w = p; p += 9 * o.DC * 8; o.dc1b = p; p += 8; o.dc2w = p; p += 576; o.dc2b = p; p += 8; o.dc3w = p; p += 72; o.dc3b = p; p += 1;
    o.n_total = p; o.n_dc = p - o.dc1w; o.npc = o.n_ec + o.n_dc;
    return o;
}

template <bool CVAE>
struct Net {
    static constexpr int DC = CVAE ? 10 : 8;
    using E1 = Conv3<28, 1, 0, 2, 1, 8, 13>;      // channel 0 of the input; the constant planes enter through the bias
    using E2 = EncC2;
    using E3 = EncC3;
    using U1 = UpConv3<4, 1, DC, 8>;
    using U2 = UpC2;
    using U3 = UpC3;
    static constexpr int NWE = U1::NWE + U2::NWE + U3::NWE;
};

// ---- LDS map (doubles).  The same for every L <= 64: the L-dependent rows are sized for L = 64.
//   weights      we1 72 (channel 0 of enc_c1_w, CIN = 1 layout) | s1 8 | s2 8 (tap sums of channels 1, 2) | be1 8
//                we23 1168 (enc_c2_w | b | enc_c3_w | b, as in theta) | We1 | We2 | We3 (effective up-conv weights) | cb 32
//   activations  img 784 | a1 1352 | a2 288 | a3x 48 | mu 64 | var 64 | vraw 64 | eps 64 | zx 80 | beff 8 | h0x 160 | a1d 512
//                a2d 1568 | out 784 (the reconstruction, then d3 in place)
//   reverse      extra 1856 | d2 1568 | d1 512 | dh0x 160 | dz 64 | dpre 128 | d3e 32
//                a2d .. extra are contiguous: [extra | d2 | d1 | dh0x] = 4096 is the chunk scratch of UpC3's weight gradient (its
//                data gradient writes d2 afterwards), [a2d | out | extra) that of UpC2's (a2d and d3 are dead by then); the
//                encoder's d1e (1352) lies on d2, d2e (288) on d1; its small scratches use extra
//   accumulators ge1 96 (we1 72 | sin 8 | cos 8 | bias 8) | gtmp 8 | ge23 1168 | gWe1 | gWe2 | gWe3 | gcb 32
//   red 16
struct CvaeLds {
    real *we1, *s1, *s2, *be1, *we23, *We1, *We2, *We3, *cb;
    real *img, *a1, *a2, *a3x, *mu, *var, *vraw, *eps, *zx, *beff, *h0x, *a1d, *a2d, *out;
    real *extra, *d2, *d1, *dh0x, *dz, *dpre, *d3e;
    real *ge1, *gtmp, *ge23, *gWe1, *gWe2, *gWe3, *gcb;
    real* red;
};
#define CVAE_EXTRA 1856
static_assert(CVAE_EXTRA + 1568 + 512 + 160 == VAE_SCRATCH, "UpC3 weight-gradient scratch = extra | d2 | d1 | dh0x");
static_assert(1568 + 784 + CVAE_EXTRA >= VAE_SCRATCH, "UpC2 weight-gradient scratch = a2d | out | extra");
static_assert(72 * (VAE_NT / 72) <= CVAE_EXTRA, "first encoder layer's chunk scratch");

template <bool CVAE>
__host__ __device__ constexpr int cvae_lds_doubles(bool train) {
    using N = Net<CVAE>;
    int n = 72 + 8 + 8 + 8 + 1168 + N::NWE + 32;
    n += 784 + 1352 + 288 + 48 + 64 * 4 + 80 + 8 + 160 + 512 + 1568 + 784;
    if (train) n += CVAE_EXTRA + 1568 + 512 + 160 + 64 + 128 + 32 + 96 + 8 + 1168 + N::NWE + 32;
    return n + 16;
}
// the largest L the fused form serves is the library's ceiling: nothing in the map grows with L
static_assert(cvae_lds_doubles<true>(true) * 8 <= SVGP_LDS_MAX_BYTES && cvae_lds_doubles<false>(true) * 8 <= SVGP_LDS_MAX_BYTES,
              "fused step at L = 64");

// Zero, but not to the optimizer (compiler only).  The image loop forms its LDS pointers from smem + this, so that LDS operands which
// do not depend on the image (the B registers of the MFMA gather-GEMMs) are not loaded ahead of the loop and kept live through it.
// Measured on the CVAE step kernel before the threadIdx measure above: 748 -> 592 bytes of scratch per lane.
__device__ __forceinline__ int lds_opaque_zero() {
    int z = 0;
    asm volatile("" : "+s"(z));
    return z;
}

template <bool CVAE>
__device__ __forceinline__ CvaeLds cvae_carve(real* smem, bool train) {
    using N = Net<CVAE>;
    CvaeLds l;
    real* p = smem;
    auto take = [&](int n) { real* r = p; p += n; return r; };
    l.we1 = take(72); l.s1 = take(8); l.s2 = take(8); l.be1 = take(8); l.we23 = take(1168);
    l.We1 = take(N::U1::NWE); l.We2 = take(N::U2::NWE); l.We3 = take(N::U3::NWE); l.cb = take(32);
    l.img = take(784); l.a1 = take(1352); l.a2 = take(288); l.a3x = take(48); l.mu = take(64); l.var = take(64); l.vraw = take(64);
    l.eps = take(64); l.zx = take(80); l.beff = take(8); l.h0x = take(160); l.a1d = take(512); l.a2d = take(1568); l.out = take(784);
    if (train) {
        l.extra = take(CVAE_EXTRA); l.d2 = take(1568); l.d1 = take(512); l.dh0x = take(160); l.dz = take(64); l.dpre = take(128);
        l.d3e = take(32);
        l.ge1 = take(96); l.gtmp = take(8); l.ge23 = take(1168);
        l.gWe1 = take(N::U1::NWE); l.gWe2 = take(N::U2::NWE); l.gWe3 = take(N::U3::NWE); l.gcb = take(32);
    }
    l.red = take(16);
    return l;
}

struct CvaeArgs {
    int b, L, clip, store, mode, N, advance_rng;
    real inv_sigma2;
    const real* theta; const real* images; const real* aux; const real* eps; real* state;
    real* part; real* sums; real* A3; real* DPRE; real* ZX; real* DH0;     // training: partials and dense-gradient operands
    real* recon; real* qmu; real* qvar; real* z;                           // stored fields (NULL: not stored)
    const real* zin;                                                        // CVAE_DECODE: (b, L) latents; CVAE_PREDICT: (N, L) train samples
    const real* aux_train;                                                  // CVAE_PREDICT: (N, 2)
    real* loss;                                                             // CVAE_PREDICT: mean squared error over all test pixels
};

// weights of a workgroup, staged once
template <bool CVAE>
__device__ __forceinline__ void cvae_stage_weights(const CvaeLds& l, const CvaeOff& o, const real* __restrict__ th, bool enc, bool dec) {
    using N = Net<CVAE>;
    const int t = threadIdx.x;
    if (enc) {
        if (t < 72) l.we1[t] = th[o.c1w + ((t >> 3) * o.C1) * 8 + (t & 7)];
        if (t >= 128 && t < 136) {
            const int co = t - 128;
            real a = 0, c = 0;
            if (CVAE)
                for (int tap = 0; tap < 9; ++tap) { a += th[o.c1w + (tap * 3 + 1) * 8 + co]; c += th[o.c1w + (tap * 3 + 2) * 8 + co]; }
            l.s1[co] = a; l.s2[co] = c; l.be1[co] = th[o.c1b + co];
        }
        lds_copy_in(l.we23, th + o.c2w, 1168);
    }
    if (dec) {
        N::U1::build_weff(th + o.dc1w, l.We1);
        N::U2::build_weff(th + o.dc2w, l.We2);
        N::U3::build_weff(th + o.dc3w, l.We3);
        if (t >= 192 && t < 200) { l.cb[t - 192] = th[o.dc1b + t - 192]; l.cb[8 + t - 192] = th[o.dc2b + t - 192]; }
        if (t == 200) l.cb[16] = th[o.dc3b];
    }
}

// image n -> a1, a2, a3x, mu, var (clipped where asked), vraw, eps; ends with a barrier
template <bool CVAE>
__device__ __forceinline__ void cvae_encode_image(const CvaeLds& l, const CvaeOff& o, const CvaeArgs& a, int n, real sn, real cs,
                                                  bool use_rng, unsigned long long ctr) {
    using N = Net<CVAE>;
    const int t = threadIdx.x, L = a.L, twoL = 2 * L;
    lds_copy_in(l.img, a.images + (size_t)n * 784, 784);
    if (t < 8) l.beff[t] = CVAE ? l.be1[t] + sn * l.s1[t] + cs * l.s2[t] : l.be1[t];
    __syncthreads();
    N::E1::fwd(l.img, l.we1, l.beff, l.a1);
    __syncthreads();
    N::E2::fwd(l.a1, l.we23, l.we23 + 576, l.a2);
    __syncthreads();
    N::E3::fwd(l.a2, l.we23 + 584, l.we23 + 584 + 576, l.a3x);
    if (CVAE && t == 0) { l.a3x[32] = sn; l.a3x[33] = cs; }
    __syncthreads();
    if (t < twoL) {
        const real* __restrict__ W = a.theta + o.edw;
        real acc = a.theta[o.edb + t];
        for (int i = 0; i < o.NI; ++i) acc += l.a3x[i] * W[i * twoL + t];
        if (t < L) {
            l.mu[t] = acc;
            l.eps[t] = use_rng ? svgp_philox_normal(ctr, (unsigned long long)n * L + t) : (a.eps ? a.eps[(size_t)n * L + t] : real(0));
        } else {
            const real vr = exp(acc);
            l.vraw[t - L] = vr;
            l.var[t - L] = a.clip ? clip_keep_nan(vr, 1e-3, 10.0) : vr;
        }
    }
    __syncthreads();
}

// zx (and, CVAE, the angle) -> h0x, a1d, a2d, out; ends with a barrier
template <bool CVAE>
__device__ __forceinline__ void cvae_decode_image(const CvaeLds& l, const CvaeOff& o, const CvaeArgs& a, real sn, real cs) {
    using N = Net<CVAE>;
    const int t = threadIdx.x;
    if (t < 128) {
        const real* __restrict__ W = a.theta + o.ddw;
        real acc = a.theta[o.ddb + t];
        for (int i = 0; i < o.ZW; ++i) acc += l.zx[i] * W[i * 128 + t];
        l.h0x[(t >> 3) * N::DC + (t & 7)] = acc;
    }
    if (CVAE && t >= 128 && t < 144) { l.h0x[(t - 128) * N::DC + 8] = sn; l.h0x[(t - 128) * N::DC + 9] = cs; }
    __syncthreads();
    N::U1::template fwd_valu<true>(l.h0x, l.We1, l.cb, l.a1d);
    __syncthreads();
    N::U2::template fwd_valu<true>(l.a1d, l.We2, l.cb + 8, l.a2d);
    __syncthreads();
    N::U3::template fwd_valu<true>(l.a2d, l.We3, l.cb + 16, l.out);
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// launch 1 of the training step: workgroup g walks the images g, g + grid, ...
// ------------------------------------------------------------------------------------------
template <bool CVAE>
__global__ __launch_bounds__(VAE_NT) void k_cvae_step_images(CvaeArgs a) {
    extern __shared__ __align__(16) real smem[];
    using N = Net<CVAE>;
    const CvaeOff o = cvae_off(CVAE, a.L);
    const CvaeLds l0 = cvae_carve<CVAE>(smem, true);
    const int t = threadIdx.x, L = a.L, twoL = 2 * L;
    const bool use_rng = a.eps == nullptr;
    const unsigned long long ctr = use_rng ? (unsigned long long)a.state[SVGP_ST_RNG_CTR] : 0ULL;
    cvae_stage_weights<CVAE>(l0, o, a.theta, true, true);
    for (int i = t; i < 96 + 8 + 1168 + N::NWE + 32; i += VAE_NT) l0.ge1[i] = 0;      // ge1 .. gcb are contiguous
    real sq = 0, kl = 0;
    for (int n = blockIdx.x; n < a.b; n += gridDim.x) {
        __syncthreads();
        const CvaeLds l = cvae_carve<CVAE>(smem + lds_opaque_zero(), true);
        real sn = 0, cs = 0;
        if (CVAE) { const real ang = a.aux[(size_t)n * 2 + 1]; sn = sin(ang); cs = cos(ang); }
        cvae_encode_image<CVAE>(l, o, a, n, sn, cs, use_rng, ctr);
        if (t < L) {
            const real m = l.mu[t], v = l.var[t];
            const real z = m + l.eps[t] * sqrt(v);
            l.zx[t] = z;
            kl += -log(v) + v + m * m;
            if (a.store) { a.qmu[(size_t)n * L + t] = m; a.qvar[(size_t)n * L + t] = v; a.z[(size_t)n * L + t] = z; }
            a.ZX[(size_t)n * o.ZW + t] = z;
        }
        if (CVAE && t >= 64 && t < 66) {
            const real v = t == 64 ? sn : cs;
            l.zx[L + t - 64] = v;
            a.ZX[(size_t)n * o.ZW + L + t - 64] = v;
        }
        if (t >= 128 && t < 128 + o.NI) a.A3[(size_t)n * o.NI + t - 128] = l.a3x[t - 128];
        __syncthreads();
        cvae_decode_image<CVAE>(l, o, a, sn, cs);
        // squared error; d(-elbo)/d out = (out - x) / sigma^2, through the ELU: d3 in place of the reconstruction
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = t + k * VAE_NT;
            if (i < 784) {
                const real ov = l.out[i], px = l.img[i], df = px - ov;
                sq += df * df;
                if (a.store) a.recon[(size_t)n * 784 + i] = ov;
                l.out[i] = a.inv_sigma2 * (ov - px) * elu_grad_from_out(ov);
            }
        }
        __syncthreads();
        // ---- decoder reverse
        N::U3::bwd_weight_mfma(l.a2d, l.out, l.gWe3, l.gcb + 16, l.extra);      // (COUT = 1: chunked VALU form; ends with a barrier)
        N::U3::bwd_data_valu(l.out, l.We3, l.d2);
        __syncthreads();
        for (int i = t; i < 1568; i += VAE_NT) l.d2[i] *= elu_grad_from_out(l.a2d[i]);
        __syncthreads();
        N::U2::bwd_weight_valu(l.a1d, l.d2, l.gWe2, l.gcb + 8, l.a2d);           // scratch: a2d | out | extra
        N::U2::bwd_data_mfma(l.d2, l.We2, l.d1);
        __syncthreads();
        for (int i = t; i < 512; i += VAE_NT) l.d1[i] *= elu_grad_from_out(l.a1d[i]);
        __syncthreads();
        N::U1::bwd_weight_mfma(l.h0x, l.d1, l.gWe1, l.gcb, l.extra);
        N::U1::bwd_data_mfma(l.d1, l.We1, l.dh0x);
        __syncthreads();
        if (t < 128) a.DH0[(size_t)n * 128 + t] = l.dh0x[(t >> 3) * N::DC + (t & 7)];
        {   // dz[i] = sum_j dh0[j] W[i][j]: 8 lanes per latent channel, xor-shuffle combine
            const real* __restrict__ W = a.theta + o.ddw;
            const int i = t >> 3, p8 = t & 7;
            real acc = 0;
            if (i < L)
                for (int j = p8; j < 128; j += 8) acc += l.dh0x[(j >> 3) * N::DC + (j & 7)] * W[i * 128 + j];
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (i < L && p8 == 0) l.dz[i] = acc;
        }
        __syncthreads();
        // ---- sample and KL: d(-elbo)/d mu = dz + mu, d/d var = dz eps / (2 sqrt var) + (1 - 1/var) / 2, var = clip(exp(.))
        if (t < twoL) {
            real g;
            if (t < L) {
                g = l.dz[t] + l.mu[t];
            } else {
                const int j = t - L;
                const real v = l.var[j], vr = l.vraw[j];
                const bool pass = !a.clip || (vr >= 1e-3 && vr <= 10.0);
                g = pass ? (l.dz[j] * l.eps[j] * real(0.5) / sqrt(v) + real(0.5) * (real(1) - real(1) / v)) * vr : real(0);
            }
            l.dpre[t] = g;
            a.DPRE[(size_t)n * twoL + t] = g;
        }
        __syncthreads();
        {   // da3[i] = sum_j dpre[j] W[i][j], i < 32 (the two angle rows have no input gradient to carry): 16 lanes per row
            const real* __restrict__ W = a.theta + o.edw;
            const int i = t >> 4, p16 = t & 15;
            real acc = 0;
            for (int j = p16; j < twoL; j += 16) acc += l.dpre[j] * W[i * twoL + j];
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            acc += __shfl_xor(acc, 8, 64);
            if (p16 == 0) l.d3e[i] = acc * elu_grad_from_out(l.a3x[i]);
        }
        if (t < 8) l.gtmp[t] = 0;
        __syncthreads();
        // ---- encoder reverse (d1e on d2, d2e on d1)
        real* d2e = l.d1;
        real* d1e = l.d2;
        N::E3::bwd_weight(l.a2, l.d3e, l.ge23 + 584, l.ge23 + 584 + 576, l.extra);
        N::E3::bwd_data(l.d3e, l.we23 + 584, d2e);
        __syncthreads();
        for (int i = t; i < 288; i += VAE_NT) d2e[i] *= elu_grad_from_out(l.a2[i]);
        __syncthreads();
        N::E2::bwd_weight(l.a1, d2e, l.ge23, l.ge23 + 576, l.extra);
        N::E2::bwd_data(d2e, l.we23, d1e);
        __syncthreads();
        for (int i = t; i < 1352; i += VAE_NT) d1e[i] *= elu_grad_from_out(l.a1[i]);
        __syncthreads();
        N::E1::bwd_weight(l.img, d1e, l.ge1, l.gtmp, l.extra);                  // gtmp: this image's bias gradient; ends with a barrier
        if (t < 8) {
            const real gb = l.gtmp[t];
            l.ge1[88 + t] += gb;
            if (CVAE) { l.ge1[72 + t] += sn * gb; l.ge1[80 + t] += cs * gb; }
        }
    }
    __syncthreads();
    const CvaeLds& l = l0;
    const real sqt = block_sum(sq, l.red);
    const real klt = block_sum(kl, l.red);
    if (t == 0) { a.sums[blockIdx.x * 2] = sqt; a.sums[blockIdx.x * 2 + 1] = klt; }
    // the workgroup's partial: [encoder convolutions as in theta | decoder convolutions as in theta]
    real* part = a.part + (size_t)blockIdx.x * o.npc;
    if (t < 72) {
        const int tap = t >> 3, co = t & 7;
        part[o.c1w + (tap * o.C1) * 8 + co] = l.ge1[t];
        if (CVAE) { part[o.c1w + (tap * 3 + 1) * 8 + co] = l.ge1[72 + co]; part[o.c1w + (tap * 3 + 2) * 8 + co] = l.ge1[80 + co]; }
    }
    if (t >= 128 && t < 136) part[o.c1b + t - 128] = l.ge1[88 + t - 128];
    lds_copy_out(part + o.c2w, l.ge23, 1168);
    real* pd = part + o.n_ec;
    N::U1::fold_grad(l.gWe1, pd);
    N::U2::fold_grad(l.gWe2, pd + (o.dc2w - o.dc1w));
    N::U3::fold_grad(l.gWe3, pd + (o.dc3w - o.dc1w));
    if (t >= 192 && t < 200) { pd[o.dc1b - o.dc1w + t - 192] = l.gcb[t - 192]; pd[o.dc2b - o.dc1w + t - 192] = l.gcb[8 + t - 192]; }
    if (t == 200) pd[o.dc3b - o.dc1w] = l.gcb[16];
}

// scalars of a step from the per-workgroup [sq, KL] pairs, by the 256 threads of ONE workgroup (G <= 256); fixed order
__device__ __forceinline__ void cvae_scalars(int G, int b, int L, real inv_sigma2, const real* sums, real* state, int did_adam,
                                             int used_rng, real* red) {
    const int t = threadIdx.x;
    const real sq = block_sum(t < G ? sums[t * 2] : real(0), red);
    const real kp = block_sum(t < G ? sums[t * 2 + 1] : real(0), red);
    if (t == 0) {
        const real KL = real(0.5) * (-(real)b * (real)L + kp);
        state[SVGP_ST_ELBO] = -real(0.5) * inv_sigma2 * sq - KL;
        state[SVGP_ST_RECON_LOSS] = sq / real(784);
        state[SVGP_ST_KL_TERM] = KL;
        if (did_adam) state[SVGP_ST_ADAM_T] += real(1);
        if (used_rng) state[SVGP_ST_RNG_CTR] += real(1);
    }
}

// ------------------------------------------------------------------------------------------
// launch 2: a workgroup owns 16 consecutive parameters (the layout of k_grad_reduce): thread (il = tid % 16, ch = tid / 16) sums the
// rows w = ch, ch + 16, ... of parameter i = 16 blk + il -- the <= 256 partials of a convolution parameter, or for a dense weight
// (r, j) the outer-product rows left[n][r] right[n][j] of the b images -- and the 16 chunk sums are combined in chunk order through
// LDS: fixed order, the same input gives the same bits.  (One thread per parameter walking all rows: 25 workgroups at L = 16, each
// thread 256 loads one behind the other; the step was 125 us that way, NOTEBOOK.)  Then TF1 Adam as svgp_adam_tf1_step computes it; the workgroup that
// takes the last ticket writes the scalars and advances the counters (every other workgroup has read state[ADAM_T] by then, as in
// k_adam_tf1_finalize).
// ------------------------------------------------------------------------------------------
struct CvaeReduceArgs {
    int cvae, b, L, G, adam, used_rng;
    real inv_sigma2, beta1, beta2, eps;
    const real* part; const real* sums; const real* A3; const real* DPRE; const real* ZX; const real* DH0;
    real* theta; real* grad; real* mo; real* vo; real* state;
};
__global__ __launch_bounds__(SVGP_BLOCK) void k_cvae_reduce_adam(CvaeReduceArgs a) {
    __shared__ real s[16][17];
    __shared__ real red[16];
    __shared__ int last;
    const CvaeOff o = cvae_off(a.cvae, a.L);
    const int il = (int)threadIdx.x & 15, ch = (int)threadIdx.x >> 4;
    const int i = (int)blockIdx.x * 16 + il, twoL = 2 * a.L;
    const real tt = a.state[SVGP_ST_ADAM_T] + real(1);
    const real lr_t = a.state[SVGP_ST_LR] * sqrt(real(1) - pow(a.beta2, tt)) / (real(1) - pow(a.beta1, tt));
    real g = 0;
    if (i < o.n_total) {
        if (i < o.n_ec || i >= o.dc1w) {
            const real* p = a.part + (i < o.n_ec ? i : o.n_ec + i - o.dc1w);
#pragma unroll 4
            for (int w = ch; w < a.G; w += 16) g += p[(size_t)w * o.npc];
        } else if (i < o.edb) {
            const int r = (i - o.edw) / twoL, j = (i - o.edw) % twoL;
#pragma unroll 4
            for (int n = ch; n < a.b; n += 16) g += a.A3[(size_t)n * o.NI + r] * a.DPRE[(size_t)n * twoL + j];
        } else if (i < o.n_enc) {
            const int j = i - o.edb;
#pragma unroll 4
            for (int n = ch; n < a.b; n += 16) g += a.DPRE[(size_t)n * twoL + j];
        } else if (i < o.ddb) {
            const int r = (i - o.ddw) >> 7, j = (i - o.ddw) & 127;
#pragma unroll 4
            for (int n = ch; n < a.b; n += 16) g += a.ZX[(size_t)n * o.ZW + r] * a.DH0[(size_t)n * 128 + j];
        } else {
            const int j = i - o.ddb;
#pragma unroll 4
            for (int n = ch; n < a.b; n += 16) g += a.DH0[(size_t)n * 128 + j];
        }
    }
    s[ch][il] = g;
    __syncthreads();   // (also: every lane of this workgroup has read the state)
    if (ch == 0 && i < o.n_total) {
        real t = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) t += s[c][il];
        a.grad[i] = t;
        if (a.adam) {
            const real mi = a.beta1 * a.mo[i] + (real(1) - a.beta1) * t;
            const real vi = a.beta2 * a.vo[i] + (real(1) - a.beta2) * t * t;
            a.mo[i] = mi;
            a.vo[i] = vi;
            a.theta[i] -= lr_t * mi / (sqrt(vi) + a.eps);
        }
    }
    if (threadIdx.x == 0) {
        unsigned long long* ticket = reinterpret_cast<unsigned long long*>(a.state + SVGP_ST_TICKET);
        last = atomicAdd(ticket, 1ULL) == (unsigned long long)gridDim.x - 1ULL;
        if (last) *ticket = 0ULL;
    }
    __syncthreads();
    if (last) cvae_scalars(a.G, a.b, a.L, a.inv_sigma2, a.sums, a.state, a.adam, a.used_rng, red);
}

// the scalars alone (svgp_cvae_forward)
__global__ __launch_bounds__(SVGP_BLOCK) void k_cvae_scalars(int G, int b, int L, real inv_sigma2, const real* sums, real* state,
                                                             int used_rng) {
    __shared__ real red[16];
    cvae_scalars(G, b, L, inv_sigma2, sums, state, 0, used_rng, red);
}

// ------------------------------------------------------------------------------------------
// forward-only launch.  mode CVAE_FULL: the step's forward with its stored fields and [sq, KL] pairs; CVAE_ENCODE: rows -> mu,
// var (and z = mu + eps sqrt(var) where a.z is given); CVAE_DECODE: given latents -> images; CVAE_PREDICT: test row t -> mean
// of the train samples whose id equals the row's (ascending n; no such row: 0 / 0 = NaN) -> image at the row's angle, squared
// error against the test image; the workgroup with the last ticket forms the mean over all test pixels.
// ------------------------------------------------------------------------------------------
template <bool CVAE>
__global__ __launch_bounds__(VAE_NT) void k_cvae_fwd(CvaeArgs a) {
    extern __shared__ __align__(16) real smem[];
    const CvaeOff o = cvae_off(CVAE, a.L);
    const CvaeLds l0 = cvae_carve<CVAE>(smem, false);
    const int t = threadIdx.x, L = a.L, mode = a.mode;
    const bool enc = mode == CVAE_FULL || mode == CVAE_ENCODE, dec = mode != CVAE_ENCODE;
    const bool use_rng = enc && a.eps == nullptr && (mode == CVAE_FULL || a.z != nullptr);
    const unsigned long long ctr = use_rng ? (unsigned long long)a.state[SVGP_ST_RNG_CTR] : 0ULL;
    cvae_stage_weights<CVAE>(l0, o, a.theta, enc, dec);
    real sq = 0, kl = 0;
    for (int n = blockIdx.x; n < a.b; n += gridDim.x) {
        __syncthreads();
        const CvaeLds l = cvae_carve<CVAE>(smem + lds_opaque_zero(), false);
        real sn = 0, cs = 0;
        if (CVAE) { const real ang = a.aux[(size_t)n * 2 + 1]; sn = sin(ang); cs = cos(ang); }
        if (enc) {
            cvae_encode_image<CVAE>(l, o, a, n, sn, cs, use_rng, ctr);
            if (t < L) {
                const real m = l.mu[t], v = l.var[t];
                const real z = m + l.eps[t] * sqrt(v);
                l.zx[t] = z;
                kl += -log(v) + v + m * m;
                if (a.qmu) a.qmu[(size_t)n * L + t] = m;
                if (a.qvar) a.qvar[(size_t)n * L + t] = v;
                if (a.z) a.z[(size_t)n * L + t] = z;
            }
        } else if (mode == CVAE_DECODE) {
            if (t < L) l.zx[t] = a.zin[(size_t)n * L + t];
        } else {
            // the group mean of test row n.  The id column of the train rows is compared VAE_NT rows at a time, one row per thread
            // (coalesced, independent loads); thread l < L then adds the matching rows of the chunk in ascending order, so the sum
            // has the order of a single walk over n.  The flags lie on a1, which only the encoder uses.
            lds_copy_in(l.img, a.images + (size_t)n * 784, 784);
            const real id = a.aux[(size_t)n * 2];
            int* hit = reinterpret_cast<int*>(l.a1);
            real s = 0, cnt = 0;
            for (int base = 0; base < a.N; base += VAE_NT) {
                const int r = base + t;
                hit[t] = r < a.N && a.aux_train[(size_t)(r < a.N ? r : 0) * 2] == id;
                __syncthreads();
                if (t < L) {
                    const int m = a.N - base < VAE_NT ? a.N - base : VAE_NT;
                    for (int k = 0; k < m; ++k)
                        if (hit[k]) { s += a.zin[(size_t)(base + k) * L + t]; cnt += real(1); }
                }
                __syncthreads();
            }
            if (t < L) l.zx[t] = s / cnt;
        }
        if (!dec) continue;
        if (CVAE && t >= 64 && t < 66) l.zx[L + t - 64] = t == 64 ? sn : cs;
        __syncthreads();
        cvae_decode_image<CVAE>(l, o, a, sn, cs);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = t + k * VAE_NT;
            if (i < 784) {
                const real ov = l.out[i];
                if (a.recon) a.recon[(size_t)n * 784 + i] = ov;
                if (mode != CVAE_DECODE) { const real df = l.img[i] - ov; sq += df * df; }
            }
        }
    }
    if (mode == CVAE_ENCODE || mode == CVAE_DECODE) return;
    __syncthreads();
    const CvaeLds& l = l0;
    const real sqt = block_sum(sq, l.red);
    const real klt = block_sum(kl, l.red);
    if (t == 0) { a.sums[blockIdx.x * 2] = sqt; a.sums[blockIdx.x * 2 + 1] = klt; }
    if (mode != CVAE_PREDICT) return;
    __shared__ int last;
    __threadfence();
    __syncthreads();
    if (t == 0) {
        unsigned long long* ticket = reinterpret_cast<unsigned long long*>(a.state + SVGP_ST_TICKET);
        last = atomicAdd(ticket, 1ULL) == (unsigned long long)gridDim.x - 1ULL;
        if (last) *ticket = 0ULL;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    const volatile real* vs = a.sums;
    const real tot = block_sum(t < (int)gridDim.x ? vs[t * 2] : real(0), l.red);
    if (t == 0) {
        a.loss[0] = tot / ((real)a.b * real(784));
        if (a.advance_rng) a.state[SVGP_ST_RNG_CTR] += real(1);      // (the encoder launch before this one has read it)
    }
}

int check_cfg(const svgp_cvae_cfg* c) {
    SVGP_REQUIRE(c != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(c->b >= 0 && c->b <= c->b_cap, SVGP_ERR_INVALID, "need 0 <= b <= b_cap (b=%d b_cap=%d)", c->b, c->b_cap);
    SVGP_REQUIRE(c->cvae == 0 || c->cvae == 1, SVGP_ERR_INVALID, "cvae=%d (0 = mnistVAE, 1 = mnistCVAE)", c->cvae);
    SVGP_REQUIRE(c->store == 0 || c->store == 1, SVGP_ERR_INVALID, "store=%d (0 or 1)", c->store);
    SVGP_REQUIRE(c->sigma > 0, SVGP_ERR_INVALID, "sigma=%g: the decoder's standard deviation must be positive", c->sigma);
    SVGP_REQUIRE(c->L >= 1 && c->L <= 64, SVGP_ERR_UNSUPPORTED, "L=%d: 1 to 64 latent channels are supported", c->L);
    return SVGP_OK;
}

void ws_fill(const svgp_cvae_cfg* c, svgp_cvae_ws_layout* w) {
    const CvaeOff o = cvae_off(c->cvae, c->L);
    const int64_t cap = c->b_cap, L = c->L;
    SvgpTake16 c16;      // fields start on 128-byte boundaries
    w->part = c16.take((int64_t)SVGP_MAX_PART * o.npc); w->sums = c16.take(SVGP_MAX_PART * 2);
    w->a3 = c16.take(cap * o.NI); w->dpre = c16.take(cap * 2 * L); w->zx = c16.take(cap * o.ZW); w->dh0 = c16.take(cap * 128);
    w->recon = c16.take(cap * 784); w->qnet_mu = c16.take(cap * L); w->qnet_var = c16.take(cap * L); w->z = c16.take(cap * L);
    w->part_stride = o.npc;
    w->total = c16.p;
}

CvaeArgs make_args(const svgp_cvae_cfg* c, const double* theta, const double* images, const double* aux, const double* eps, double* ws,
                   double* state) {
    svgp_cvae_ws_layout w;
    ws_fill(c, &w);
    CvaeArgs a;
    memset(&a, 0, sizeof(a));
    a.b = c->b; a.L = c->L; a.clip = c->clip_qs != 0; a.store = c->store; a.mode = CVAE_FULL;
    a.inv_sigma2 = 1.0 / (c->sigma * c->sigma);
    a.theta = theta; a.images = images; a.aux = aux; a.eps = eps; a.state = state;
    if (ws) {
        a.part = ws + w.part; a.sums = ws + w.sums; a.A3 = ws + w.a3; a.DPRE = ws + w.dpre; a.ZX = ws + w.zx; a.DH0 = ws + w.dh0;
        a.recon = ws + w.recon; a.qmu = ws + w.qnet_mu; a.qvar = ws + w.qnet_var; a.z = ws + w.z;
    }
    return a;
}

template <bool CVAE>
int launch_fwd(const CvaeArgs& a, int rows, hipStream_t st) {
    const size_t lds = (size_t)cvae_lds_doubles<CVAE>(false) * sizeof(real);
    int rc = set_dyn_lds(k_cvae_fwd<CVAE>, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cvae_fwd<CVAE>, dim3(rows < SVGP_MAX_PART ? rows : SVGP_MAX_PART), dim3(VAE_NT), lds, st, a);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

int route_text(const char* const* names, int n, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int pos = 0, rc = SVGP_OK;
    buf[0] = 0;
    for (int i = 0; i < n && !rc; ++i) rc = svgp_route_append(buf, cap, &pos, "%s\n", names[i]);
    return rc;
}

}  // namespace

extern "C" int svgp_cvae_param_layout_get(const svgp_cvae_cfg* c, svgp_mnist_param_layout* out) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(out != nullptr, SVGP_ERR_INVALID, "out is NULL");
    const CvaeOff o = cvae_off(c->cvae, c->L);
    out->enc_c1_w = o.c1w; out->enc_c1_b = o.c1b; out->enc_c2_w = o.c2w; out->enc_c2_b = o.c2b; out->enc_c3_w = o.c3w;
    out->enc_c3_b = o.c3b; out->enc_d_w = o.edw; out->enc_d_b = o.edb; out->n_enc = o.n_enc;
    out->dec_d_w = o.ddw; out->dec_d_b = o.ddb; out->dec_c1_w = o.dc1w; out->dec_c1_b = o.dc1b; out->dec_c2_w = o.dc2w;
    out->dec_c2_b = o.dc2b; out->dec_c3_w = o.dc3w; out->dec_c3_b = o.dc3b; out->n_vae = o.n_total;
    out->ip = out->l_GP = out->amplitude = out->ov = o.n_total;      // no GP variables
    out->n_total = o.n_total;
    return SVGP_OK;
}

extern "C" int svgp_cvae_ws_layout_get(const svgp_cvae_cfg* c, svgp_cvae_ws_layout* out) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(out != nullptr, SVGP_ERR_INVALID, "out is NULL");
    ws_fill(c, out);
    return SVGP_OK;
}

extern "C" int svgp_cvae_lds_bytes(int cvae, int L) {
    if ((cvae != 0 && cvae != 1) || L < 1 || L > 64) return -1;
    return (cvae ? cvae_lds_doubles<true>(true) : cvae_lds_doubles<false>(true)) * (int)sizeof(real);
}

extern "C" int svgp_cvae_step_route(const svgp_cvae_cfg* c, char* buf, int cap) {
    int rc = check_cfg(c);
    if (rc) return rc;
    const char* names[2] = {c->cvae ? "k_cvae_step_images<CVAE>" : "k_cvae_step_images<VAE>", "k_cvae_reduce_adam"};
    return route_text(names, c->b == 0 ? 0 : 2, buf, cap);
}

extern "C" int svgp_cvae_predict_route(const svgp_cvae_cfg* c, char* buf, int cap) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(c->cvae == 1, SVGP_ERR_INVALID, "conditional generation needs cvae = 1");
    const char* names[2] = {"k_cvae_fwd<CVAE>:encode", "k_cvae_fwd<CVAE>:predict"};
    return route_text(names, 2, buf, cap);
}

extern "C" int svgp_cvae_train_step(const svgp_cvae_cfg* c, double* theta, const double* images, const double* aux, const double* eps,
                                    double* ws, double* grad, double* adam_m, double* adam_v, double* state, int adam, void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && images && ws && grad && state && (aux || !c->cvae), SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(!adam || (adam_m && adam_v), SVGP_ERR_INVALID, "NULL device pointer (Adam moments)");
    if (c->b == 0) return SVGP_OK;
    const CvaeOff o = cvae_off(c->cvae, c->L);
    const CvaeArgs a = make_args(c, theta, images, aux, eps, ws, state);
    const int G = c->b < SVGP_MAX_PART ? c->b : SVGP_MAX_PART;
    hipStream_t st = (hipStream_t)stream;
    if (c->cvae) {
        const size_t lds = (size_t)cvae_lds_doubles<true>(true) * sizeof(real);
        rc = set_dyn_lds(k_cvae_step_images<true>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cvae_step_images<true>, dim3(G), dim3(VAE_NT), lds, st, a);
    } else {
        const size_t lds = (size_t)cvae_lds_doubles<false>(true) * sizeof(real);
        rc = set_dyn_lds(k_cvae_step_images<false>, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cvae_step_images<false>, dim3(G), dim3(VAE_NT), lds, st, a);
    }
    SVGP_LAUNCH_CHECK();
    CvaeReduceArgs r;
    r.cvae = c->cvae; r.b = c->b; r.L = c->L; r.G = G; r.adam = adam != 0; r.used_rng = eps == nullptr;
    r.inv_sigma2 = a.inv_sigma2; r.beta1 = 0.9; r.beta2 = 0.999; r.eps = 1e-8;
    r.part = a.part; r.sums = a.sums; r.A3 = a.A3; r.DPRE = a.DPRE; r.ZX = a.ZX; r.DH0 = a.DH0;
    r.theta = theta; r.grad = grad; r.mo = adam_m; r.vo = adam_v; r.state = state;
    hipLaunchKernelGGL(k_cvae_reduce_adam, dim3((o.n_total + 15) / 16), dim3(SVGP_BLOCK), 0, st, r);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_cvae_forward(const svgp_cvae_cfg* c, const double* theta, const double* images, const double* aux, const double* eps,
                                 double* ws, double* state, void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && images && ws && state && (aux || !c->cvae), SVGP_ERR_INVALID, "NULL device pointer");
    if (c->b == 0) return SVGP_OK;
    const CvaeArgs a = make_args(c, theta, images, aux, eps, ws, state);      // stores on whatever cfg.store says
    rc = c->cvae ? launch_fwd<true>(a, c->b, (hipStream_t)stream) : launch_fwd<false>(a, c->b, (hipStream_t)stream);
    if (rc) return rc;
    const int G = c->b < SVGP_MAX_PART ? c->b : SVGP_MAX_PART;
    hipLaunchKernelGGL(k_cvae_scalars, dim3(1), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, G, c->b, c->L, a.inv_sigma2, a.sums, state,
                       eps == nullptr ? 1 : 0);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_cvae_encode(const svgp_cvae_cfg* c, const double* theta, const double* images, const double* aux, double* mu,
                                double* var, void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && images && mu && var && (aux || !c->cvae), SVGP_ERR_INVALID, "NULL device pointer");
    if (c->b == 0) return SVGP_OK;
    CvaeArgs a = make_args(c, theta, images, aux, nullptr, nullptr, nullptr);
    a.mode = CVAE_ENCODE; a.qmu = mu; a.qvar = var;
    return c->cvae ? launch_fwd<true>(a, c->b, (hipStream_t)stream) : launch_fwd<false>(a, c->b, (hipStream_t)stream);
}

extern "C" int svgp_cvae_decode(const svgp_cvae_cfg* c, const double* theta, const double* z, const double* aux, double* images_out,
                                void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(theta && z && images_out && (aux || !c->cvae), SVGP_ERR_INVALID, "NULL device pointer");
    if (c->b == 0) return SVGP_OK;
    CvaeArgs a = make_args(c, theta, nullptr, aux, nullptr, nullptr, nullptr);
    a.mode = CVAE_DECODE; a.zin = z; a.recon = images_out;
    return c->cvae ? launch_fwd<true>(a, c->b, (hipStream_t)stream) : launch_fwd<false>(a, c->b, (hipStream_t)stream);
}

extern "C" long long svgp_cvae_predict_workspace_elems(const svgp_cvae_cfg* c, long long n_train) {
    if (check_cfg(c) || n_train < 0) return -1;
    return (n_train * c->L + 15) / 16 * 16 + 2 * SVGP_MAX_PART;
}

extern "C" int svgp_cvae_predict(const svgp_cvae_cfg* c, long long n_train, const double* theta, const double* images_train,
                                 const double* aux_train, const double* eps, const double* images_test, const double* aux_test,
                                 double* work, double* recon_out, double* loss_out, double* state, void* stream) {
    int rc = check_cfg(c);
    if (rc) return rc;
    SVGP_REQUIRE(c->cvae == 1, SVGP_ERR_INVALID, "conditional generation needs cvae = 1");
    SVGP_REQUIRE(n_train >= 0 && n_train <= 0x7fffffffLL / 784, SVGP_ERR_INVALID, "n_train = %lld train rows", n_train);
    SVGP_REQUIRE(theta && aux_test && images_test && work && recon_out && loss_out && state, SVGP_ERR_INVALID, "NULL device pointer");
    SVGP_REQUIRE(n_train == 0 || (images_train && aux_train), SVGP_ERR_INVALID, "NULL device pointer");
    if (c->b == 0) return SVGP_OK;
    double* ztr = work;
    double* sums = work + (n_train * c->L + 15) / 16 * 16;
    svgp_cvae_cfg ce = *c;
    ce.clip_qs = 0;                 // predict_CVAE encodes without clipping (SVGPVAE_model.py:806-808)
    if (n_train > 0) {
        ce.b = ce.b_cap = (int)n_train;
        CvaeArgs e = make_args(&ce, theta, images_train, aux_train, eps, nullptr, state);
        e.mode = CVAE_ENCODE; e.z = ztr;
        rc = launch_fwd<true>(e, (int)n_train, (hipStream_t)stream);
        if (rc) return rc;
    }
    CvaeArgs p = make_args(c, theta, images_test, aux_test, nullptr, nullptr, state);
    p.mode = CVAE_PREDICT; p.N = (int)n_train; p.zin = ztr; p.aux_train = aux_train; p.recon = recon_out; p.loss = loss_out; p.sums = sums;
    p.advance_rng = eps == nullptr && n_train > 0;
    return launch_fwd<true>(p, c->b, (hipStream_t)stream);
}
