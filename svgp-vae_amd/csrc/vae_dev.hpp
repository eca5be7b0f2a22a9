// Device code of the mnistVAE kernels (vae_mnist.hip) that other translation units instantiate too: the decoder's
// weight-gradient work rides as extra workgroups of the GP reverse factor launch (gp_kernels.hip), which runs
// SVGP_BLOCK = 256 threads per workgroup, so every helper takes its thread count NT as a template argument.
#pragma once
#include "common.hpp"

namespace svgp_vae {

#define VAE_NT 512          // threads per workgroup of the VAE kernels (8 waves: 2 per SIMD)
#define VAE_SCRATCH 4096    // reals of LDS scratch for the weight-gradient chunk reduction

typedef double d4v_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// In-LDS gather-GEMM on the f64 MFMA: the conv im2col-GEMMs of the per-image kernels.
//   gg_fwd  : out[(y*osy+ooy)*Wo + x*osx+oox][co] = epi(bias[co] + sum_t sum_ci in[(y*sy+oy_t)*Wi + x*sx+ox_t][ci] W_t[ci][co])
//             A[i = pixel][k = ci] gathered per lane (zero outside the tile), B[k = ci][j = co] from LDS weights,
//             one v_mfma_f64_16x16x4 per (tap, 4 channels); a wave owns 16 consecutive pixels of the iteration space.
//             TW: weights stored [co][ci] are read transposed (data gradient).
//   gg_wgrad: gW_t[ci][co] += sum_pixels in_t[pixel][ci] * dout[pixel][co]; A[i = ci][k = pixel], B[k = pixel][j = co];
//             a wave owns whole taps, so the LDS accumulators need no atomics.
// SI / SO: doubles between consecutive pixels of `in` / `out` (packed: CI / CO).  A gather is one ds_read_b64 per lane, serviced as
// two half waves of 16 pixels x 2 channels.  With input stride 2 and 8 packed doubles per pixel, neighbouring pixels of a half wave are
// 128 bytes apart and the sixteen fall on two 16-byte windows of the 256-byte bank row: 7 distinct addresses on the busiest bank in
// the mean (tools/lds_bank_model.py).  Every gather of a group is issued before the first MFMA, so the group's MFMA chain waits for
// all of them: these conflicts do NOT hide under the 64-cycle issue of the f64 MFMA -- the stride-2 data reverses of the fused decoder
// launch are 3.9 and 2.3 us of its phase timeline (NOTEBOOK 14.5d) -- and that launch pads the pixel stride (SI = 9: 2 in the mean).
// ---------------------------------------------------------------------------------------------
template <int NTAP, bool TW, bool ELU_BIAS, int CI, int CO, int NT = VAE_NT, int SI = CI, int SO = CO>
__device__ __forceinline__ void gg_fwd(const real* in, int Hi, int Wi, int Hs, int Ws, int sy, int sx,
                                       const int (&oy)[NTAP], const int (&ox)[NTAP], const int (&woff)[NTAP],
                                       const real* W, int ldw, const real* bias, real* out, int Wo, int osy, int osx,
                                       int ooy, int oox) {
    constexpr int KQ = (CI + 3) / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = NT >> 6, r = lane & 15, q = lane >> 4;
    const int NP = Hs * Ws, ngrp = (NP + 15) >> 4;
    // B operands (weights) do not depend on the pixel group: fetched once, unconditionally (clamped index + select)
    real breg[NTAP * KQ];
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) {
            const int c = kq * 4 + q, cc = c < CI ? c : CI - 1, rc = r < CO ? r : CO - 1;
            const real v = W[woff[t] + (TW ? rc * ldw + cc : cc * ldw + rc)];
            breg[t * KQ + kq] = (c < CI && r < CO) ? v : real(0);
        }
    for (int grp = wave; grp < ngrp; grp += nwave) {
        const int pa = grp * 16 + r;
        const bool pv = pa < NP;
        const int ya = pv ? pa / Ws : 0, xa = pv ? pa % Ws : 0;
        // Padded input stride: the tap addresses are formed from this one value, which the empty asm makes the compiler form per group.
        // Without it the sixteen `pixel * SI` of a one-group layer are hoisted out of the caller's image loop and live through its
        // MFMA phases (174 VGPRs in the fused decoder launch, 160 with it); the validity masks stay hoisted -- they are scalar.
        // Pinning `pa` itself un-hoists those too: 218.  Packed, `pb` is dead and the address expression is the one that always stood.
        int pb = ya * sy * Wi + xa * sx;
        if constexpr (SI != CI) asm volatile("" : "+v"(pb));
        // A operands of the whole group first (independent LDS reads in flight together), then the MFMA chain
        real areg[NTAP * KQ];
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int iy = ya * sy + oy[t], ix = xa * sx + ox[t];
            const bool valid = pv && ((unsigned)iy < (unsigned)Hi) && ((unsigned)ix < (unsigned)Wi);
            const real* ap = in + (valid ? (SI != CI ? pb + oy[t] * Wi + ox[t] : iy * Wi + ix) * SI : 0);
#pragma unroll
            for (int kq = 0; kq < KQ; ++kq) {
                const int c = kq * 4 + q, cc = c < CI ? c : CI - 1;
                const real v = ap[cc];
                areg[t * KQ + kq] = (valid && c < CI) ? v : real(0);
            }
        }
        d4v_t acc = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < NTAP * KQ; ++i) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[i], breg[i], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int po = grp * 16 + q + 4 * e;
            if (po < NP && r < CO) {
                const int y = po / Ws, x = po % Ws;
                real v = acc[e];
                if (ELU_BIAS) v = elu_f(v + bias[r]);
                out[((y * osy + ooy) * Wo + x * osx + oox) * SO + r] = v;
            }
        }
    }
}

// Operands of a boundary-tested tap in the rolled VALU forward below, the idiom of gg_fwd: the caller clamps the address (element 0
// of the tile for a tap outside it), the N operands are loaded unconditionally -- contiguous, so they vectorise (ds_read_b128) -- and
// the caller selects `valid ? v : 0` afterwards.  Written as `valid ? p[i] : 0` each element compiles to a ds_read_b64 in an
// exec-masked block of its own (8 of them and 16 exec writes per tap trip).  The empty asm is for the compiler only: without it the
// optimizer sinks the loads back under the test.  Only UpConv3::fwd_valu<true> uses it: the fused decoder launch is 1.3 - 1.5 us
// shorter with it, the unrolled forward, bwd_data_valu and the two VALU weight-gradient forms measured slower.
template <int N>
__device__ __forceinline__ void tap_operands(real (&v)[N], const real* p) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[i];
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}
// ... with the tap's weights in the same group (UpConv3::fwd_valu<true, true>, the fused decoder launch only): N x COG values at
// wk[ci * COUT + g], issued before the first wait, so a tap trip is ONE LDS round trip (with the weights read behind the pin it is
// two: the activations' lgkmcnt(0), then the weights').  They are read as 16-byte vectors -- (ci, g = 0..1) for COG = 2, (ci, ci + 1)
// for a single output channel -- because plain loads of two neighbouring doubles compile to ds_read2_b64, the 128 B/clk form.
// `wk` MUST be 16-byte aligned: the vector type tells the compiler so, and a ds_read_b128 off 16 bytes is replayed at ~64 cycles.
// UpConv3 asserts the strides; the caller asserts the base where it forms it (dec_fwd_bwd_we_offset).  A kernel whose We is only
// 8-byte aligned (k_generate: an odd count of doubles in front of it) must not take this form.
typedef double d2v_t __attribute__((ext_vector_type(2)));
template <int N, int COG, int COUT>
__device__ __forceinline__ void tap_operand_group(real (&v)[N], real (&wv)[N * COG], const real* p, const real* wk) {
    static_assert(COG == 2 || (COG == 1 && COUT == 1 && N % 2 == 0), "weights of a tap as 16-byte vectors");
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[i];
    if constexpr (COG == 2) {
#pragma unroll
        for (int ci = 0; ci < N; ++ci) {
            const d2v_t w2 = *reinterpret_cast<const d2v_t*>(wk + ci * COUT);
            wv[2 * ci] = w2.x; wv[2 * ci + 1] = w2.y;
        }
    } else {
#pragma unroll
        for (int ci = 0; ci < N; ci += 2) {
            const d2v_t w2 = *reinterpret_cast<const d2v_t*>(wk + ci);
            wv[ci] = w2.x; wv[ci + 1] = w2.y;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
#pragma unroll
    for (int i = 0; i < N * COG; ++i) asm volatile("" : "+v"(wv[i]));
}

struct TapP { int oy, ox, woff, ooy, oox; };
template <int NTAP, int CI, int CO, int NT, typename TapFn>
__device__ __forceinline__ void gg_wgrad(const real* in, int Hi, int Wi, int Hs, int Ws, int sy, int sx, TapFn tapfn,
                                         const real* dout, int Wo, int osy, int osx, real* gW) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = NT >> 6, r = lane & 15, q = lane >> 4;
    const int NP = Hs * Ws;
    const int rci = r < CI ? r : CI - 1, rco = r < CO ? r : CO - 1;
#pragma unroll 1
    for (int t = wave; t < NTAP; t += nwave) {
        const TapP tp = tapfn(t);
        d4v_t acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < NP; k0 += 16) {       // four k-steps per trip, operands fetched together
            real av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = k0 + 4 * u + q;
                const bool pv = p < NP;
                const int y = pv ? p / Ws : 0, x = pv ? p % Ws : 0;
                const int iy = y * sy + tp.oy, ix = x * sx + tp.ox;
                const bool valid = pv && ((unsigned)iy < (unsigned)Hi) && ((unsigned)ix < (unsigned)Wi);
                const real a0 = in[(valid ? (iy * Wi + ix) * CI : 0) + rci];
                const real b0 = dout[((y * osy + tp.ooy) * Wo + x * osx + tp.oox) * CO + rco];
                av[u] = (valid && r < CI) ? a0 : real(0);
                bv[u] = (pv && r < CO) ? b0 : real(0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ci = q + 4 * e;
            if (ci < CI && r < CO) gW[tp.woff + ci * CO + r] += acc[e];
        }
    }
}

// bias gradient: gb[co] += sum_pixels dpre[p][co]; 32 pixel chunks per channel combined through scratch
template <int NPIX, int COUT, int NT = VAE_NT>
__device__ __forceinline__ void bias_grad(const real* dpre, real* gb, real* scratch) {
    constexpr int BCH = 32;
    if (threadIdx.x < BCH * COUT) {
        const int co = threadIdx.x % COUT, chunk2 = threadIdx.x / COUT;
        real s = 0;
        for (int p = chunk2; p < NPIX; p += BCH) s += dpre[p * COUT + co];
        scratch[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < COUT) {
        real t = 0;
#pragma unroll
        for (int c = 0; c < BCH; ++c) t += scratch[c * COUT + threadIdx.x];
        gb[threadIdx.x] += t;
    }
    __syncthreads();
}

// 3x3 convolution, stride STRIDE, no padding, no upsampling (the mnistVAE encoder layers, VAE_utils.py:117-122)
// on an LDS-resident NHWC tile, via the MFMA gather-GEMMs above.
template <int HS, int UPS, int PAD, int STRIDE, int CIN, int COUT, int HOUT, int NT = VAE_NT>
struct Conv3 {
    static_assert(UPS == 1 && PAD == 0 && STRIDE == 2, "encoder layers: stride-2 valid convolutions");
    static constexpr int NW = 9 * CIN * COUT;
    static constexpr int NPIX = HOUT * HOUT;

    static __device__ void fwd(const real* in, const real* w, const real* bias, real* out) {
        if constexpr (CIN == 1) {
            // one input channel (first encoder layer): 9 MACs per output; the MFMA gather-GEMM would use 1 of 4 k-lanes
            for (int it = threadIdx.x; it < NPIX * COUT; it += NT) {
                const int co = it % COUT, p = it / COUT, y = p / HOUT, x = p % HOUT;
                real acc = bias[co];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) acc += in[(2 * y + ky) * HS + 2 * x + kx] * w[(ky * 3 + kx) * COUT + co];
                out[it] = elu_f(acc);
            }
            return;
        }
        const int oy[9] = {0, 0, 0, 1, 1, 1, 2, 2, 2}, ox[9] = {0, 1, 2, 0, 1, 2, 0, 1, 2};
        int wo[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) wo[t] = t * CIN * COUT;
        gg_fwd<9, false, true, CIN, COUT, NT>(in, HS, HS, HOUT, HOUT, 2, 2, oy, ox, wo, w, COUT, bias, out, HOUT, 1, 1, 0, 0);
    }

    // din[iy][ix][ci] = sum_{ky,kx: (iy-ky), (ix-kx) even} dpre[(iy-ky)/2][(ix-kx)/2][co] w[ky][kx][ci][co]:
    // four input-parity classes, each a gather-GEMM with the taps of matching parity
    static __device__ void bwd_data(const real* dpre, const real* w, real* din) {
        // parity 0: ky in {0, 2} (offsets 0, -1);  parity 1: ky = 1 (offset 0)
        {   // (py, px) = (0, 0): 4 taps
            const int oy[4] = {0, 0, -1, -1}, ox[4] = {0, -1, 0, -1};
            const int wo[4] = {(0 * 3 + 0) * CIN * COUT, (0 * 3 + 2) * CIN * COUT, (2 * 3 + 0) * CIN * COUT, (2 * 3 + 2) * CIN * COUT};
            gg_fwd<4, true, false, COUT, CIN, NT>(dpre, HOUT, HOUT, (HS + 1) / 2, (HS + 1) / 2, 1, 1, oy, ox, wo, w, COUT, nullptr,
                                              din, HS, 2, 2, 0, 0);
        }
        {   // (0, 1): ky in {0,2}, kx = 1
            const int oy[2] = {0, -1}, ox[2] = {0, 0};
            const int wo[2] = {(0 * 3 + 1) * CIN * COUT, (2 * 3 + 1) * CIN * COUT};
            gg_fwd<2, true, false, COUT, CIN, NT>(dpre, HOUT, HOUT, (HS + 1) / 2, HS / 2, 1, 1, oy, ox, wo, w, COUT, nullptr, din,
                                              HS, 2, 2, 0, 1);
        }
        {   // (1, 0): ky = 1, kx in {0,2}
            const int oy[2] = {0, 0}, ox[2] = {0, -1};
            const int wo[2] = {(1 * 3 + 0) * CIN * COUT, (1 * 3 + 2) * CIN * COUT};
            gg_fwd<2, true, false, COUT, CIN, NT>(dpre, HOUT, HOUT, HS / 2, (HS + 1) / 2, 1, 1, oy, ox, wo, w, COUT, nullptr, din,
                                              HS, 2, 2, 1, 0);
        }
        {   // (1, 1): ky = kx = 1
            const int oy[1] = {0}, ox[1] = {0};
            const int wo[1] = {(1 * 3 + 1) * CIN * COUT};
            gg_fwd<1, true, false, COUT, CIN, NT>(dpre, HOUT, HOUT, HS / 2, HS / 2, 1, 1, oy, ox, wo, w, COUT, nullptr, din, HS, 2,
                                              2, 1, 1);
        }
    }

    // gw += sum_pixels in * dpre ; gb += sum_pixels dpre.  Ends with a barrier.
    static __device__ void bwd_weight(const real* in, const real* dpre, real* gw, real* gb, real* scratch) {
        if constexpr (CIN == 1) {
            // one input channel (first encoder layer): 9 * COUT outputs of NPIX MACs each.  On the MFMA this uses 1 of 16
            // rows (9.7 us of the 23.4 us launch, in-kernel timestamps); here thread = (output o = tap * COUT + co, pixel
            // chunk), the chunks are combined through LDS in fixed order (2.7 us incl. the bias gradient).
            constexpr int NO = 9 * COUT, NCH = NT / NO;
            static_assert(NCH >= 1 && NO * NCH <= VAE_SCRATCH, "chunk layout");
            const int o = threadIdx.x % NO, ch = threadIdx.x / NO, t = o / COUT, co = o % COUT, ky = t / 3, kx = t % 3;
            if (ch < NCH) {
                real acc = 0;
                for (int p = ch; p < NPIX; p += NCH) {
                    const int y = p / HOUT, x = p % HOUT;
                    acc += in[(2 * y + ky) * HS + 2 * x + kx] * dpre[p * COUT + co];
                }
                scratch[ch * NO + o] = acc;
            }
            __syncthreads();
            if (threadIdx.x < NO) {
                real tsum = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) tsum += scratch[c * NO + threadIdx.x];
                gw[threadIdx.x] += tsum;           // raw layout (ky, kx, 0, co) = o
            }
            __syncthreads();
        } else {
            auto tapfn = [](int t) { return TapP{t / 3, t % 3, t * CIN * COUT, 0, 0}; };
            gg_wgrad<9, CIN, COUT, NT>(in, HS, HS, HOUT, HOUT, 2, 2, tapfn, dpre, HOUT, 1, 1, gw);
        }
        bias_grad<NPIX, COUT, NT>(dpre, gb, scratch);
    }
};

// ---------------------------------------------------------------------------------------------
// UpSampling2D(2) + 3x3 convolution (stride 1, PAD 0|1) as FOUR parity-specific 2x2 convolutions on
// the low-resolution stored input (HS x HS x CIN): for output row y, base = y - PAD, parity
// pi = base & 1, Y = base >> 1, the three taps ky read source rows Y + T(pi,ky) with
// T(pi,k) = (k + pi >= 2), so taps sharing a source row are pre-summed into effective weights
//   We[pi_y][pi_x][ty][tx][ci][co] = sum_{ky: T(pi_y,ky)=ty} sum_{kx: T(pi_x,kx)=tx} w[ky][kx][ci][co].
// 4 taps instead of 9 in the forward, 16 instead of 36 in the data gradient, and the weight gradient
// is accumulated on We (folded back to w once per workgroup).  Mathematically identical to the
// reference's UpSampling2D + Conv2D (VAE_utils.py:132-140); summation order differs (1e-16 level).
// ---------------------------------------------------------------------------------------------
// WCS: distance in doubles between the four parity classes of the We image that fwd_valu, bwd_data_valu and bwd_data_mfma READ
// (build_weff, fold_grad and the weight-gradient forms keep the packed layout, which is also that of ws.dec_weff).  Packed, the class
// stride is 0 mod the 256-byte bank row, and the lanes of one ds_read_b128 group -- neighbouring output pixels, hence different
// classes -- read different addresses on the same banks.  The fused decoder launch pads it (dec_weff_lds_index below).
// Pixel strides, in doubles, of the LDS activations (packed by default; the fused decoder launch pads three, dec_act_* below):
// FIS / FOS: of `in` / `out` of fwd_valu;  RIS: of `dpre` of bwd_data_mfma;  ROS: of `din` of bwd_data_mfma and bwd_data_valu.
template <int HS, int PAD, int CIN, int COUT, int NT = VAE_NT, int WCS = 4 * CIN * COUT, int FIS = CIN, int FOS = COUT,
          int RIS = COUT, int ROS = CIN>
struct UpConv3 {
    static_assert(FIS >= CIN && FOS >= COUT && RIS >= COUT && ROS >= CIN, "pixel strides of the LDS activations");
    static constexpr int HOUT = 2 * HS - 2 + 2 * PAD;
    static constexpr int NPIX = HOUT * HOUT;
    static constexpr int NWE = 16 * CIN * COUT;          // effective weights
    static constexpr int NWC = 4 * CIN * COUT;           // ... of one parity class
    static constexpr int LWE = 3 * WCS + NWC;            // doubles of the LDS image with class stride WCS (= NWE when packed)
    // every 16-byte weight read of fwd_valu<true, true> starts at an even count of doubles from We, which its caller keeps 16-byte aligned
    static_assert(WCS >= NWC && WCS % 2 == 0 && (CIN * COUT) % 2 == 0, "class stride of the LDS weight image");
    // packed index (class, tap, ci, co) -> index in the image with class stride WCS
    static __host__ __device__ constexpr int lds_index(int e) { return (e / NWC) * WCS + e % NWC; }
    static constexpr int NW = 9 * CIN * COUT;            // raw weights
    static constexpr int COG = (COUT % 2 == 0) ? 2 : 1;
    static constexpr int NCG = COUT / COG;
    static constexpr int CIG = (CIN % 2 == 0) ? 2 : 1;
    static constexpr int NIG = CIN / CIG;
    static __device__ __forceinline__ int T(int pi, int k) { return (k + pi >= 2) ? 1 : 0; }

    // We (LDS) from raw w (global or LDS)
    static __device__ void build_weff(const real* w, real* We) {
        static_assert(WCS == NWC, "packed layout");
        for (int e = threadIdx.x; e < NWE; e += NT) {
            const int co = e % COUT, ci = (e / COUT) % CIN, tap = (e / (COUT * CIN)) % 4, cls = e / (COUT * CIN * 4);
            const int ty = tap >> 1, tx = tap & 1, py = cls >> 1, px = cls & 1;
            real s = 0;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    if (T(py, ky) == ty && T(px, kx) == tx) s += w[((ky * 3 + kx) * CIN + ci) * COUT + co];
            We[e] = s;
        }
    }
    // raw-weight gradient from the effective-weight gradient: gw[ky][kx] = sum_classes gWe[cls][T,T]
    static __device__ void fold_grad(const real* gWe, real* gw) {
        static_assert(WCS == NWC, "packed layout");
        for (int e = threadIdx.x; e < NW; e += NT) {
            const int co = e % COUT, ci = (e / COUT) % CIN, kx = (e / (COUT * CIN)) % 3, ky = e / (COUT * CIN * 3);
            real s = 0;
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px)
                    s += gWe[(((py * 2 + px) * 4 + T(py, ky) * 2 + T(px, kx)) * CIN + ci) * COUT + co];
            gw[e] = s;
        }
    }

    // ---- VALU variants (register-tiled LDS loops): faster than the MFMA forms where the tile would be mostly
    //      padding (single output channel) or the gather arithmetic dominates; chosen per layer from ablation timings
    // out = elu(conv(up(in)) + bias); item = (output pixel, group of COG channels)
    // ROLL: the two tap loops stay loops (one tap of CIN x COG FMAs per trip) instead of hoisting the 32 activation and 64 weight
    // LDS loads of an item: ~85 VGPRs fewer, same FMA order per output (bias, then ty, tx, ci), so the same bits.  For kernels that
    // must stay within 168 VGPRs (decoder_fwd_bwd_data_images below).  Its activations come through tap_operands (unconditional
    // vector loads, select afterwards); the unrolled form keeps the predicated reads, with which it is faster.
    // WVEC (with ROLL): the tap's weights join the activations' group as 16-byte vector loads (tap_operand_group).  Only for a We that
    // is 16-byte aligned -- the caller's static_assert, where it forms the pointer; the default is the form for any 8-byte aligned We.
    template <bool ROLL = false, bool WVEC = false>
    static __device__ void fwd_valu(const real* in, const real* We, const real* bias, real* out) {
        static_assert(ROLL || !WVEC, "the grouped weight reads exist in the rolled form only");
        static_assert(!ROLL || FIS % 2 == 0, "the 16-byte activation reads of the rolled form start at even counts of doubles");
        constexpr int TAP_UNROLL = ROLL ? 1 : 2;     // 1: no unrolling; 2 = the trip count: full
        for (int it = threadIdx.x; it < NPIX * NCG; it += NT) {
            const int cg = it % NCG, p = it / NCG, x = p % HOUT, y = p / HOUT;
            const int by = y - PAD, bx = x - PAD, py = by & 1, px = bx & 1, Y = by >> 1, X = bx >> 1;
            real acc[COG];
#pragma unroll
            for (int g = 0; g < COG; ++g) acc[g] = bias[cg * COG + g];
            const real* wc = We + (py * 2 + px) * WCS + cg * COG;
#pragma unroll TAP_UNROLL
            for (int ty = 0; ty < 2; ++ty) {
                const int sy = Y + ty;
                const bool vy = (unsigned)sy < (unsigned)HS;
#pragma unroll TAP_UNROLL
                for (int tx = 0; tx < 2; ++tx) {
                    const int sx = X + tx;
                    const bool valid = vy && ((unsigned)sx < (unsigned)HS);
                    const real* src = in + (valid ? (sy * HS + sx) * FIS : 0);
                    const real* wk = wc + (ty * 2 + tx) * CIN * COUT;
                    if constexpr (WVEC) {
                        real av[CIN], wv[CIN * COG];
                        tap_operand_group<CIN, COG, COUT>(av, wv, src, wk);
#pragma unroll
                        for (int ci = 0; ci < CIN; ++ci) {
                            const real a = valid ? av[ci] : real(0);
#pragma unroll
                            for (int g = 0; g < COG; ++g) acc[g] += a * wv[ci * COG + g];
                        }
                    } else {
                        real av[CIN];
                        if constexpr (ROLL) tap_operands(av, src);
#pragma unroll
                        for (int ci = 0; ci < CIN; ++ci) {
                            real a;
                            if constexpr (ROLL) a = valid ? av[ci] : real(0);
                            else a = valid ? src[ci] : real(0);
#pragma unroll
                            for (int g = 0; g < COG; ++g) acc[g] += a * wk[ci * COUT + g];
                        }
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < COG; ++g) out[p * FOS + cg * COG + g] = elu_f(acc[g]);
        }
    }

    // din (HS x HS x CIN) from dpre (HOUT x HOUT x COUT); item = (stored pixel, group of CIG channels)
    static __device__ void bwd_data_valu(const real* dpre, const real* We, real* din) {
        for (int it = threadIdx.x; it < HS * HS * NIG; it += NT) {
            const int ig = it % NIG, ps = it / NIG, Xs = ps % HS, Ys = ps / HS;
            real acc[CIG];
#pragma unroll
            for (int g = 0; g < CIG; ++g) acc[g] = 0;
#pragma unroll 1
            for (int cy = 0; cy < 4; ++cy) {            // (pi_y, ty)
                const int py = cy >> 1, ty = cy & 1;
                const int y = 2 * (Ys - ty) + py + PAD;
                const bool vy = (unsigned)y < (unsigned)HOUT;
#pragma unroll
                for (int cx = 0; cx < 4; ++cx) {        // (pi_x, tx)
                    const int px = cx >> 1, tx = cx & 1;
                    const int x = 2 * (Xs - tx) + px + PAD;
                    const bool valid = vy && ((unsigned)x < (unsigned)HOUT);
                    const real* dp = dpre + (valid ? (y * HOUT + x) * COUT : 0);
                    // (packed: the expression as it always stood -- written the other way the same sum compiles to other code)
                    const real* wk = WCS == NWC ? We + (((py * 2 + px) * 4 + ty * 2 + tx) * CIN + ig * CIG) * COUT
                                                : We + (py * 2 + px) * WCS + ((ty * 2 + tx) * CIN + ig * CIG) * COUT;
#pragma unroll
                    for (int co = 0; co < COUT; ++co) {
                        const real d = valid ? dp[co] : real(0);
#pragma unroll
                        for (int g = 0; g < CIG; ++g) acc[g] += d * wk[g * COUT + co];
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < CIG; ++g) din[ps * ROS + ig * CIG + g] = acc[g];
        }
    }

    // gWe += sum_pixels in * dpre ; gb += sum_pixels dpre.  item = (class, tap, ci, pixel chunk) -> COUT
    // outputs; chunks combined through `scratch` (>= VAE_SCRATCH reals) in fixed order.  Ends with a barrier.
    static __device__ void bwd_weight_valu(const real* in, const real* dpre, real* gWe, real* gb, real* scratch) {
        static_assert(WCS == NWC, "packed layout");
        constexpr int NTC = 16 * CIN;
        constexpr int NCH0 = NT / NTC, NCH1 = VAE_SCRATCH / NWE;
        constexpr int NCH = NCH0 < NCH1 ? (NCH0 < 1 ? 1 : NCH0) : NCH1;
        constexpr int NG = HS + 1;                      // candidate Y (and X) values: -1 .. HS-1
        const int tc = threadIdx.x % NTC, chunk = threadIdx.x / NTC;
        if (chunk < NCH) {
            const int ci = tc % CIN, tap = (tc / CIN) % 4, cls = tc / (CIN * 4);
            const int ty = tap >> 1, tx = tap & 1, py = cls >> 1, px = cls & 1;
            real acc[COUT];
#pragma unroll
            for (int co = 0; co < COUT; ++co) acc[co] = 0;
#pragma unroll 2
            for (int idx = chunk; idx < NG * NG; idx += NCH) {
                const int Y = idx / NG - 1, X = idx % NG - 1;
                const int y = 2 * Y + py + PAD, x = 2 * X + px + PAD, sy = Y + ty, sx = X + tx;
                const bool valid = ((unsigned)y < (unsigned)HOUT) && ((unsigned)x < (unsigned)HOUT) &&
                                   ((unsigned)sy < (unsigned)HS) && ((unsigned)sx < (unsigned)HS);
                const real a = valid ? in[(sy * HS + sx) * CIN + ci] : real(0);
                const real* dp = dpre + (valid ? (y * HOUT + x) * COUT : 0);
#pragma unroll
                for (int co = 0; co < COUT; ++co) acc[co] += a * dp[co];
            }
#pragma unroll
            for (int co = 0; co < COUT; ++co) scratch[chunk * NWE + tc * COUT + co] = acc[co];
        }
        __syncthreads();
        for (int widx = threadIdx.x; widx < NWE; widx += NT) {
            real s = 0;
#pragma unroll
            for (int c = 0; c < NCH; ++c) s += scratch[c * NWE + widx];
            gWe[widx] += s;
        }
        __syncthreads();
        constexpr int BCH = 32;
        if (threadIdx.x < BCH * COUT) {
            const int co = threadIdx.x % COUT, chunk2 = threadIdx.x / COUT;
            real s = 0;
            for (int p = chunk2; p < NPIX; p += BCH) s += dpre[p * COUT + co];
            scratch[threadIdx.x] = s;
        }
        __syncthreads();
        if (threadIdx.x < COUT) {
            real t = 0;
#pragma unroll
            for (int c = 0; c < BCH; ++c) t += scratch[c * COUT + threadIdx.x];
            gb[threadIdx.x] += t;
        }
        __syncthreads();
    }

    // din (HS x HS x CIN) from dpre (HOUT x HOUT x COUT): one 16-tap gather-GEMM with input stride 2 over dpre
    static __device__ void bwd_data_mfma(const real* dpre, const real* We, real* din) {
        int oy[16], ox[16], wo[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int py = (t >> 3) & 1, ty = (t >> 2) & 1, px = (t >> 1) & 1, tx = t & 1;
            oy[t] = py + PAD - 2 * ty;
            ox[t] = px + PAD - 2 * tx;
            wo[t] = (py * 2 + px) * WCS + (ty * 2 + tx) * CIN * COUT;
        }
        gg_fwd<16, true, false, COUT, CIN, NT, RIS, ROS>(dpre, HOUT, HOUT, HS, HS, 2, 2, oy, ox, wo, We, COUT, nullptr, din, HS, 1, 1, 0,
                                                         0);
    }

    // gWe += sum_pixels in * dpre ; gb += sum_pixels dpre.  Ends with a barrier.
    static __device__ void bwd_weight_mfma(const real* in, const real* dpre, real* gWe, real* gb, real* scratch) {
        static_assert(WCS == NWC, "packed layout");
        if (COUT >= 2) {
            // 16 (class, tap) pairs = 16 "taps" of one gather-GEMM over the HOUT/2 x HOUT/2 class grid
            auto tapfn = [](int t) {
                const int opy = (t >> 3) & 1, opx = (t >> 2) & 1, ty = (t >> 1) & 1, tx = t & 1;
                const int by = opy - PAD, bx = opx - PAD, py = by & 1, px = bx & 1;
                return TapP{(by - py) / 2 + ty, (bx - px) / 2 + tx, ((py * 2 + px) * 4 + ty * 2 + tx) * CIN * COUT, opy, opx};
            };
            gg_wgrad<16, CIN, COUT, NT>(in, HS, HS, HOUT / 2, HOUT / 2, 1, 1, tapfn, dpre, HOUT, 2, 2, gWe);
        } else {
            // single output channel: item = (class, tap, pixel chunk), 32 chunks; all CIN inputs of a pixel per item
            constexpr int NCH = NT / 16;
            constexpr int NG = HS + 1;                  // candidate Y (and X): -1 .. HS-1
            const int ct = threadIdx.x & 15, chunk = threadIdx.x >> 4;
            const int cls = ct >> 2, tap = ct & 3, ty = tap >> 1, tx = tap & 1, py = cls >> 1, px = cls & 1;
            real acc[CIN];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0;
            for (int idx = chunk; idx < NG * NG; idx += NCH) {
                const int Y = idx / NG - 1, X = idx % NG - 1;
                const int y = 2 * Y + py + PAD, x = 2 * X + px + PAD, sy = Y + ty, sx = X + tx;
                const bool valid = ((unsigned)y < (unsigned)HOUT) && ((unsigned)x < (unsigned)HOUT) &&
                                   ((unsigned)sy < (unsigned)HS) && ((unsigned)sx < (unsigned)HS);
                const real d = valid ? dpre[y * HOUT + x] : real(0);
                const real* ip = in + (valid ? (sy * HS + sx) * CIN : 0);
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) acc[ci] += ip[ci] * d;
            }
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) scratch[chunk * (16 * CIN) + ct * CIN + ci] = acc[ci];
            __syncthreads();
            for (int widx = threadIdx.x; widx < 16 * CIN; widx += NT) {
                real s = 0;
#pragma unroll 8
                for (int c = 0; c < NCH; ++c) s += scratch[c * (16 * CIN) + widx];
                gWe[widx] += s;
            }
        }
        __syncthreads();
        bias_grad<NPIX, COUT, NT>(dpre, gb, scratch);
    }
};

template <int NT> using UpC1T = UpConv3<4, 1, 8, 8, NT>;
using UpC1 = UpC1T<VAE_NT>;     // (4,4,8)  -> up 8x8   -> same  -> (8,8,8)
template <int NT> using UpC2T = UpConv3<8, 0, 8, 8, NT>;
using UpC2 = UpC2T<VAE_NT>;     // (8,8,8)  -> up 16x16 -> valid -> (14,14,8)
template <int NT> using UpC3T = UpConv3<14, 1, 8, 1, NT>;
using UpC3 = UpC3T<VAE_NT>;    // (14,14,8)-> up 28x28 -> same  -> (28,28,1)
#define DEC_NWE 2176   // 1024 + 1024 + 128
static_assert(UpC1::NWE + UpC2::NWE + UpC3::NWE == DEC_NWE, "effective weights of the three up-convolutions");

using EncC1 = Conv3<28, 1, 0, 2, 1, 8, 13>;
using EncC2 = Conv3<13, 1, 0, 2, 8, 8, 6>;
using EncC3 = Conv3<6, 1, 0, 2, 8, 8, 2>;

__device__ __forceinline__ void lds_copy_in(real* dst, const real* __restrict__ src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
__device__ __forceinline__ void lds_copy_out(real* __restrict__ dst, const real* src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
// ... from an 8-channel array kept at pixel stride S in LDS (dec_act_index below) to its packed global copy
template <int S>
__device__ __forceinline__ void lds_copy_out_px(real* __restrict__ dst, const real* src, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[S == 8 ? i : (i >> 3) * S + (i & 7)];
}
__device__ __forceinline__ void lds_zero(real* dst, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = 0;
}

// Staging in two halves (the chain kernels of the m <= 64 step).  lds_copy_in above compiles to one global load, a full wait and
// the LDS store per pass -- ceil(n / NT) dependent round trips per array, the arrays one after another.  Here the loads of a GROUP of
// arrays are issued first and stored afterwards, so a group costs one round trip.  The rule: the loads of a group sit in one basic
// block (an unconditional load from an index kept inside the array and a predicated store; no branch per element),
// and the thread count is the template parameter (the callers run with exactly NT threads), never blockDim.x, which is itself a
// load from the dispatch packet.
// A lane past the end loads the element its first pass loads (a line that pass fetches anyway), not the array's last one: of a weight
// array every workgroup of the launch reads the same addresses, and whole passes of lanes on ONE of them queue up at a single L2
// channel (NOTEBOOK 14.5c).
template <int N, int NT>
__device__ __forceinline__ int stage_spare() { return N >= NT ? (int)threadIdx.x : min((int)threadIdx.x, N - 1); }
// Compile-time count N: stage_issue returns the ceil(N / NT) values of this thread, stage_commit stores them.
template <int N, int NT>
struct StageRegs {
    static constexpr int C = (N + NT - 1) / NT;
    real v[C];
};
template <int N, int NT>
__device__ __forceinline__ StageRegs<N, NT> stage_issue(const real* __restrict__ src) {
    StageRegs<N, NT> r;
#pragma unroll
    for (int k = 0; k < StageRegs<N, NT>::C; ++k) {
        const int i = (int)threadIdx.x + k * NT;
        r.v[k] = src[(k + 1) * NT <= N || i < N ? i : stage_spare<N, NT>()];
    }
    return r;
}
template <int N, int NT>
__device__ __forceinline__ void stage_commit(real* dst, const StageRegs<N, NT>& r) {
#pragma unroll
    for (int k = 0; k < StageRegs<N, NT>::C; ++k) {
        const int i = (int)threadIdx.x + k * NT;
        if ((k + 1) * NT <= N || i < N) dst[i] = r.v[k];
    }
}
// Run-time count n >= 1 (the weights: their size depends on L): straight-line chunks of CH loads in flight per thread, then the CH
// stores.  Loads issued by the caller before this call stay in flight through the first chunk and are complete after it.
template <int NT, int CH>
__device__ __forceinline__ void stage_chunk(real* dst, const real* __restrict__ src, int n, int c0) {
    const int base = c0 + (int)threadIdx.x, spare = min(base, n - 1);
    real r[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) r[k] = src[base + k * NT < n ? base + k * NT : spare];
    // (compiler only: behind its store's test a load needs no clamp, and the optimizer would sink it there -- a round trip of its own)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
    for (int k = 0; k < CH; ++k)
        if (base + k * NT < n) dst[base + k * NT] = r[k];
}
template <int NT, int CH = 8>
__device__ __forceinline__ void stage_copy(real* dst, const real* __restrict__ src, int n) {
    // The first chunk stands outside the loop: inside it, the wait for the registers that the previous trip loaded lands in front
    // of the chunk's loads, and on the first trip that wait would be for the caller's group.
    stage_chunk<NT, CH>(dst, src, n, 0);
    for (int c0 = CH * NT; c0 < n; c0 += CH * NT) stage_chunk<NT, CH>(dst, src, n, c0);      // (uniform trip count: a scalar branch)
}

// In-kernel phase timeline (tools/decoder_phase_probe.py).  The PROBE instances of the two longest launches of the config-2 step
// stamp wall_clock64() -- the constant 100 MHz counter, the same on every CU, so the rows of different workgroups share one time
// axis -- at each phase; thread 0 of a workgroup writes slot k of the workgroup's row with an ordinary store, the last slot holds
// where the workgroup ran and what it was.  The buffer is the caller's and nothing else reads it.  The product instances
// (PROBE = false) contain none of this: a stamp compiles to nothing and the row pointer is never formed.
#define SVGP_PROBE_DEC_SLOTS 16      // k_decoder_fwd_bwd_data: 0 entry .. 14 exit (include/svgpvae_hip.h has the list), 15 place
#define SVGP_PROBE_FB_SLOTS 8        // k_gp_factor_bwd: 0 entry, 1 staged, 2 UpC3, 3 UpC2, 4 UpC1 + dense, 5 partial stored, 6 exit, 7 place
template <bool PROBE>
__device__ __forceinline__ void probe_stamp(unsigned long long* row, int k) {
    if constexpr (PROBE) {
        if (threadIdx.x == 0) row[k] = wall_clock64();
    }
}
// bits 0..31 HW_ID (compute unit: bits 8..15), bits 32..35 XCC_ID, bits 56..59 `detail`, bits 60..63 `role`
template <bool PROBE>
__device__ __forceinline__ void probe_place(unsigned long long* row, int k, int role, int detail) {
    if constexpr (PROBE) {
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        if (threadIdx.x == 0)
            row[k] = (unsigned long long)hw | ((unsigned long long)(xcc & 15u) << 32) | ((unsigned long long)(detail & 15) << 56) |
                     ((unsigned long long)(role & 15) << 60);
    }
}

struct EncOff { int c1w, c1b, c2w, c2b, c3w, c3b, dw, db, n; };
struct DecOff { int dw, db, c1w, c1b, c2w, c2b, c3w, c3b, n; };

__device__ __host__ inline EncOff enc_off(int L) {
    EncOff o; int p = 0;
    o.c1w = p; p += 72; o.c1b = p; p += 8; o.c2w = p; p += 576; o.c2b = p; p += 8;
    o.c3w = p; p += 576; o.c3b = p; p += 8; o.dw = p; p += 32 * 2 * L; o.db = p; p += 2 * L; o.n = p;
    return o;
}
__device__ __host__ constexpr DecOff dec_off(int L) {
    DecOff o = {}; int p = 0;
    o.dw = p; p += L * 128; o.db = p; p += 128; o.c1w = p; p += 576; o.c1b = p; p += 8;
    o.c2w = p; p += 576; o.c2b = p; p += 8; o.c3w = p; p += 72; o.c3b = p; p += 1; o.n = p;
    return o;
}

// ------------------------------------------------------------------------------------------
// Decoder forward z -> dense -> UpC1 -> UpC2 -> UpC3 -> out of ONE image in LDS: the map and the pieces of k_decoder_fwd
// (vae_mnist.hip), k_generate (generate.hip) and k_casale_generate (casale_generate.hip).
// LDS: w n_dec | z 64 | h0 128 | a1 512 | a2 1568 | out 784 | [red 16] | We1 We2 We3; a kernel's own arrays start at We1 + DEC_NWE.
// red (the scratch of block_sum) exists in k_decoder_fwd only.
// ------------------------------------------------------------------------------------------
struct DecFwdLds { real *w, *z, *h0, *a1, *a2, *out, *red, *We1, *We2, *We3; };
__host__ __device__ constexpr int dec_fwd_lds(int n_dec, bool red) {
    return n_dec + 64 + 128 + 512 + 1568 + 784 + (red ? 16 : 0) + DEC_NWE;
}
static_assert(dec_fwd_lds(dec_off(64).n, false) == 14793 && dec_fwd_lds(dec_off(64).n, true) == 14809, "decoder forward map at L = 64");
template <bool RED>
__device__ __forceinline__ DecFwdLds dec_fwd_carve(real* smem, int n_dec) {
    DecFwdLds l;
    l.w = smem; l.z = l.w + n_dec; l.h0 = l.z + 64; l.a1 = l.h0 + 128; l.a2 = l.a1 + 512; l.out = l.a2 + 1568;
    l.red = RED ? l.out + 784 : nullptr;
    l.We1 = l.out + 784 + (RED ? 16 : 0); l.We2 = l.We1 + UpC1::NWE; l.We3 = l.We2 + UpC2::NWE;
    return l;
}
// theta's decoder part into l.w, then the effective weights of the three up-convolutions from the LDS copy (one coalesced read of
// the raw weights).  k_decoder_fwd stages in its own, measured load order instead.
__device__ __forceinline__ void decoder_fwd_stage(const DecFwdLds& l, const DecOff& od, const real* th_dec) {
    lds_copy_in(l.w, th_dec, od.n);
    __syncthreads();
    UpC1::build_weff(l.w + od.c1w, l.We1);
    UpC2::build_weff(l.w + od.c2w, l.We2);
    UpC3::build_weff(l.w + od.c3w, l.We3);
}
// l.z -> l.out, a barrier behind each of the four layers (the caller's barrier stands between its writes of l.z and this).
// ROLLED: fwd_valu<ROLLED>, the same FMA order in ~85 VGPRs fewer
template <bool ROLLED>
__device__ __forceinline__ void decoder_fwd_layers(const DecFwdLds& l, const DecOff& od, int L) {
    if (threadIdx.x < 128) {
        real acc = l.w[od.db + threadIdx.x];
        for (int i = 0; i < L; ++i) acc += l.z[i] * l.w[od.dw + i * 128 + threadIdx.x];
        l.h0[threadIdx.x] = acc;
    }
    __syncthreads();
    UpC1::fwd_valu<ROLLED>(l.h0, l.We1, l.w + od.c1b, l.a1);
    __syncthreads();
    UpC2::fwd_valu<ROLLED>(l.a1, l.We2, l.w + od.c2b, l.a2);
    __syncthreads();
    UpC3::fwd_valu<ROLLED>(l.a2, l.We3, l.w + od.c3b, l.out);
    __syncthreads();
}
// decode only: one workgroup of VAE_NT threads turns rows first, first + stride, ... of z (b, L) in global memory into images (b, 784).
// LDS: dec_fwd_lds(n_dec, false) reals
__device__ __forceinline__ void decoder_fwd_rows(int b, int L, const real* th_dec, const real* zg, real* images, int first, int stride,
                                                 real* smem) {
    const DecOff od = dec_off(L);
    const DecFwdLds l = dec_fwd_carve<false>(smem, od.n);
    decoder_fwd_stage(l, od, th_dec);
    for (int n = first; n < b; n += stride) {
        __syncthreads();
        if ((int)threadIdx.x < L) l.z[threadIdx.x] = zg[(size_t)n * L + threadIdx.x];
        __syncthreads();
        decoder_fwd_layers<false>(l, od, L);
        lds_copy_out(images + (size_t)n * 784, l.out, 784);
    }
}


// ------------------------------------------------------------------------------------------
// Decoder reverse pass in two halves (round 6).  The DATA half (k_decoder_bwd_data, vae_mnist.hip) is the chain
// d recon -> d2 -> d1 -> dh0 -> zbar that the GP reverse stages wait for; it stores the pre-activation gradients
// d2 (14,14,8), d1 (8,8,8), dh0 (128) of every image.  The WEIGHT half below needs only those and the stored forward
// activations and feeds nothing but the closing gradient reduction, so it runs as extra workgroups ("riders") of a launch
// that leaves most of the chip idle anyway: the reverse factor stage (L workgroups on 256 CUs, gp_kernels.hip).
// One rider = NT threads walking images slot, slot + n_slots, ... for ONE group of layers; weight gradients accumulate in LDS (the
// convolutions' on the effective parity-class weights); one partial (raw-parameter layout, od.n reals) per slot, its ranges
// written by the slot's riders, summed over slots in fixed order by svgp_mnist_grad_reduce.  LDS: dec_wgrad_lds(NT, L, n_types).
// Reference semantics: tf.gradients of VAE_utils.py:128-141,154-162 w.r.t. the decoder variables (MNIST_experiment.py:202-205).
// ------------------------------------------------------------------------------------------
struct DecWgradArgs {
    int b, L, geco, n_slots, n_types;    // riders = n_slots * n_types; rider r: partial slot r / n_types, layer group r % n_types
    real inv_bglobal;
    const real* state; const real* images; const real* z; const real* h0; const real* a1; const real* a2; const real* recon;
    const real* d2; const real* d1; const real* dh0;
    real* part;                          // (n_slots, od.n)
};
// Layer groups of a rider (bit 0: UpC3, bit 1: UpC2, bit 2: UpC1 + dense).  n_types 1: one rider per image does everything;
// 2: {UpC3} | {UpC2, UpC1, dense}; 3: one group each.  The groups of a slot write disjoint ranges of the same partial.
__host__ __device__ constexpr int dec_wgrad_mask(int n_types, int ty) { return n_types == 1 ? 7 : n_types == 2 ? (ty == 0 ? 1 : 6) : (1 << ty); }
// LDS reals of one rider: inputs + accumulators of its groups + bias accumulators + the chunk-reduction scratch
// (NT / 16 chunks x 128 for UpC3, NT / 128 chunks x 1024 for UpC2, 256 for the bias sums alone)
__host__ __device__ constexpr int dec_wgrad_lds_mask(int nt, int L, int mask) {
    return ((mask & 1) ? 1568 + 784 + 128 : 0) + ((mask & 2) ? 512 + 1568 + 1024 : 0) +
           ((mask & 4) ? 128 + 512 + 128 + 64 + 1024 + L * 128 + 128 : 0) + 32 + ((mask & 3) ? (nt <= 256 ? 2048 : 4096) : 256);
}
__host__ __device__ constexpr int dec_wgrad_lds(int nt, int L, int n_types) {
    int mx = 0;
    for (int ty = 0; ty < n_types; ++ty) {
        const int v = dec_wgrad_lds_mask(nt, L, dec_wgrad_mask(n_types, ty));
        mx = v > mx ? v : mx;
    }
    return mx;
}

template <int NT, bool PROBE = false, bool EXCL = false>
__device__ __forceinline__ void decoder_wgrad_rider(const DecWgradArgs& a, int rider, real* smem, unsigned long long* probe = nullptr) {
    static_assert(NT >= 256 && NT <= 512, "bias / chunk layouts are sized for 256..512 threads");
    const DecOff od = dec_off(a.L);
    // Riders are numbered TYPE-major, heaviest layer group first (UpC2: 113 K MACs per image, UpC3: 56 K, UpC1 + dense: 39 K): a launch that
    // cannot hold all of them at once (the reverse factor launch: 848 workgroups for 768 slots) then starts its LAST riders, the ones
    // that wait for a slot, on the lightest group.  (Slot-major, types interleaved: the late riders included UpC2 ones and the launch
    // ended with them, 20.5 us against 17.2 for the channel chain alone.)
    const int tyo = rider / a.n_slots, slot = rider - tyo * a.n_slots;
    const int ty = a.n_types == 3 ? (tyo == 0 ? 1 : tyo == 1 ? 0 : 2) : a.n_types == 2 ? 1 - tyo : 0;
    const int mask = dec_wgrad_mask(a.n_types, ty);
    const int ndense = a.L * 128;
    real* p = smem;
    auto take = [&](int n) { real* r = p; p += n; return r; };
    real *a2 = nullptr, *d3 = nullptr, *gWe3 = nullptr, *a1 = nullptr, *d2 = nullptr, *gWe2 = nullptr, *h0 = nullptr, *d1 = nullptr,
         *dh0 = nullptr, *z = nullptr, *gWe1 = nullptr, *dacc = nullptr;
    if (mask & 1) { a2 = take(1568); d3 = take(784); gWe3 = take(128); }
    if (mask & 2) { a1 = take(512); d2 = take(1568); gWe2 = take(1024); }
    if (mask & 4) { h0 = take(128); d1 = take(512); dh0 = take(128); z = take(64); gWe1 = take(1024); dacc = take(ndense + 128); }
    real* gb = take(32);             // c1b (8) | c2b (8) | c3b (1)
    real* scratch = p;
    // One group of loads per image: every operand of the rider's layer groups is issued before the first wait (stage_issue: unconditional
    // loads from indices kept inside the arrays) and stored to LDS afterwards, one round trip instead of one per pass of NT threads and
    // array.  The first image's group flies while the accumulators are zeroed, a later image's during the products of the one before.
    // The values wait in ONE register set rv.  EXCL (the reverse factor launch: always the three-type layout, a rider runs exactly one
    // layer group): the groups share its first registers -- 15 doubles at NT = 256 instead of 29 with every group live, which is what
    // keeps that kernel at three workgroups per CU.  Otherwise (n_types 1 or 2: a rider may run several groups) each group has its own.
    const int t = threadIdx.x;
    constexpr int C1568 = StageRegs<1568, NT>::C, C784 = StageRegs<784, NT>::C, C512 = StageRegs<512, NT>::C, C128 = StageRegs<128, NT>::C;
    constexpr int N1 = C1568 + 2 * C784, N2 = C512 + C1568, N4 = 2 * C128 + C512 + 1;
    constexpr int O1 = 0, O2 = EXCL ? 0 : N1, O4 = EXCL ? 0 : N1 + N2;
    constexpr int NV = EXCL ? (N1 > N2 ? (N1 > N4 ? N1 : N4) : (N2 > N4 ? N2 : N4)) : N1 + N2 + N4;
    real rv[NV];
    auto put = [&](auto r, int off) {
#pragma unroll
        for (int k = 0; k < decltype(r)::C; ++k) rv[off + k] = r.v[k];
    };
    auto issue = [&](int n) {
        if (mask & 1) {
            put(stage_issue<1568, NT>(a.a2 + (size_t)n * 1568), O1);
            put(stage_issue<784, NT>(a.recon + (size_t)n * 784), O1 + C1568);
            put(stage_issue<784, NT>(a.images + (size_t)n * 784), O1 + C1568 + C784);
        }
        if (mask & 2) {
            put(stage_issue<512, NT>(a.a1 + (size_t)n * 512), O2);
            put(stage_issue<1568, NT>(a.d2 + (size_t)n * 1568), O2 + C512);
        }
        if (mask & 4) {
            put(stage_issue<128, NT>(a.h0 + (size_t)n * 128), O4);
            put(stage_issue<512, NT>(a.d1 + (size_t)n * 512), O4 + C128);
            put(stage_issue<128, NT>(a.dh0 + (size_t)n * 128), O4 + C128 + C512);
            rv[O4 + 2 * C128 + C512] = a.z[(size_t)n * a.L + (t < a.L ? t : a.L - 1)];
        }
    };
    auto commit = [&](real* dst, auto tag, int off) {      // tag: an empty StageRegs type carrier
        decltype(tag) r;
#pragma unroll
        for (int k = 0; k < decltype(tag)::C; ++k) r.v[k] = rv[off + k];
        stage_commit(dst, r);
    };
    if (slot < a.b) issue(slot);
    if (mask & 1) for (int i = threadIdx.x; i < 128; i += NT) gWe3[i] = 0;
    if (mask & 2) for (int i = threadIdx.x; i < 1024; i += NT) gWe2[i] = 0;
    if (mask & 4) for (int i = threadIdx.x; i < 1024 + ndense + 128; i += NT) gWe1[i] = 0;     // gWe1 | dacc (contiguous)
    if (threadIdx.x < 32) gb[threadIdx.x] = 0;
    const real gscale = (a.geco ? a.state[SVGP_ST_LAGRANGE] * a.inv_bglobal : real(1)) / real(784);
    for (int n = slot; n < a.b; n += a.n_slots) {
        __syncthreads();
        if (mask & 1) {
#pragma unroll
            for (int k = 0; k < C784; ++k) {
                const int i = t + k * NT;
                const real o = rv[O1 + C1568 + k];
                if (i < 784) d3[i] = real(2) * gscale * (o - rv[O1 + C1568 + C784 + k]) * elu_grad_from_out(o);
            }
            commit(a2, StageRegs<1568, NT>(), O1);
        }
        if (mask & 2) {
            commit(d2, StageRegs<1568, NT>(), O2 + C512);
            commit(a1, StageRegs<512, NT>(), O2);
        }
        if (mask & 4) {
            commit(d1, StageRegs<512, NT>(), O4 + C128);
            commit(h0, StageRegs<128, NT>(), O4);
            commit(dh0, StageRegs<128, NT>(), O4 + C128 + C512);
            if (t < a.L) z[t] = rv[O4 + 2 * C128 + C512];
        }
        if (n + a.n_slots < a.b) issue(n + a.n_slots);      // the next image of this slot: one image ahead
        __syncthreads();
        // (probe slots 1..4 are those of the rider's LAST image; the products end with a barrier)
        probe_stamp<PROBE>(probe, 1);       // staged
        if (mask & 1) UpC3T<NT>::bwd_weight_mfma(a2, d3, gWe3, gb + 16, scratch);     // COUT = 1: chunked VALU form inside
        probe_stamp<PROBE>(probe, 2);       // UpC3
        if (mask & 2) UpC2T<NT>::bwd_weight_valu(a1, d2, gWe2, gb + 8, scratch);
        probe_stamp<PROBE>(probe, 3);       // UpC2
        if (mask & 4) {
            UpC1T<NT>::bwd_weight_mfma(h0, d1, gWe1, gb, scratch);
            for (int o = threadIdx.x; o < ndense; o += NT) dacc[o] += z[o >> 7] * dh0[o & 127];
            if (threadIdx.x < 128) dacc[ndense + threadIdx.x] += dh0[threadIdx.x];
        }
        if constexpr (PROBE) __syncthreads();
        probe_stamp<PROBE>(probe, 4);       // UpC1 + dense
    }
    __syncthreads();
    real* part = a.part + (size_t)slot * od.n;
    if (mask & 1) {
        UpC3T<NT>::fold_grad(gWe3, part + od.c3w);
        if (threadIdx.x == 0) part[od.c3b] = gb[16];
    }
    if (mask & 2) {
        UpC2T<NT>::fold_grad(gWe2, part + od.c2w);
        if (threadIdx.x < 8) part[od.c2b + threadIdx.x] = gb[8 + threadIdx.x];
    }
    if (mask & 4) {
        UpC1T<NT>::fold_grad(gWe1, part + od.c1w);
        if (threadIdx.x < 8) part[od.c1b + threadIdx.x] = gb[threadIdx.x];
        for (int o = threadIdx.x; o < ndense; o += NT) part[od.dw + o] = dacc[o];
        if (threadIdx.x < 128) part[od.db + threadIdx.x] = dacc[ndense + threadIdx.x];
    }
    if constexpr (PROBE) {                  // partial stored: every wave's stores have left
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        probe_place<PROBE>(probe, 7, 3, mask);
    }
    probe_stamp<PROBE>(probe, 5);
}

// ------------------------------------------------------------------------------------------
// decoder reverse, DATA half: d loss / d recon -> d2, d1, dh0 (stored for the weight half) -> zbar.  The chain the GP
// reverse stages wait for; the weight gradients (decoder_wgrad_rider above) ride in a later launch.  One workgroup of VAE_NT
// threads walks images first, first + stride, ...  PRE: the effective up-convolution weights come from ws.dec_weff (74 KB of
// LDS: two workgroups per CU -- the launch that also carries the deferred (A_hat + jI)^-1, svgp_mnist_decoder_bwd_data_pre_aji,
// relies on that); otherwise they are rebuilt from the raw weights (84 KB).
// Reference semantics: tf.gradients of VAE_utils.py:128-141,154-162 (MNIST_experiment.py:202-205).
// ------------------------------------------------------------------------------------------
struct DecBwdDataArgs {
    int b, L, geco;
    real inv_bglobal;
    const real* state; const real* th_dec; const real* images; const real* a1g; const real* a2g; const real* recon;
    real* d2g; real* d1g; real* dh0g; real* zbar;
    const real* weff;
};
__host__ __device__ constexpr int dec_bwd_data_lds(int L, int n_dec, bool pre) {
    return L * 128 + DEC_NWE + 512 + 1568 + 784 + 1568 + 512 + 128 + (pre ? 0 : n_dec - L * 128 - 128);
}
template <bool PRE>
__device__ __forceinline__ void decoder_bwd_data_images(const DecBwdDataArgs& a, int first, int stride, real* smem) {
    const DecOff od = dec_off(a.L);
    real* w = smem;                  // dense weights only: L*128
    real* We1 = w + a.L * 128;         // effective weights
    real* We2 = We1 + UpC1::NWE;
    real* We3 = We2 + UpC2::NWE;
    real* a1 = We3 + UpC3::NWE;      // 512
    real* a2 = a1 + 512;             // 1568
    real* d3 = a2 + 1568;            // 784
    real* d2 = d3 + 784;             // 1568
    real* d1 = d2 + 1568;            // 512
    real* dh0 = d1 + 512;            // 128
    real* raw = dh0 + 128;           // raw conv weights (+ biases), staged once: od.n - od.c1w
    // one group of loads: the first image's a1, a2, reconstruction and pixels, the effective (or raw) weights, the dense weights
    // (image `first` exists for every workgroup -- the grids have min(b, 256) image workgroups; nf keeps a larger grid inside the arrays)
    const int nf = first < a.b ? first : a.b - 1;
    auto ra1 = stage_issue<512, VAE_NT>(a.a1g + (size_t)nf * 512);
    auto ra2 = stage_issue<1568, VAE_NT>(a.a2g + (size_t)nf * 1568);
    auto rrec = stage_issue<784, VAE_NT>(a.recon + (size_t)nf * 784);
    auto rpx = stage_issue<784, VAE_NT>(a.images + (size_t)nf * 784);
    if (PRE) {
        const auto rwe = stage_issue<DEC_NWE, VAE_NT>(a.weff);
        stage_copy<VAE_NT>(w, a.th_dec + od.dw, a.L * 128);
        stage_commit<DEC_NWE, VAE_NT>(We1, rwe);
    } else {
        constexpr int NRAW = 576 + 8 + 576 + 8 + 72 + 1;     // od.n - od.c1w
        const auto rraw = stage_issue<NRAW, VAE_NT>(a.th_dec + od.c1w);
        stage_copy<VAE_NT>(w, a.th_dec + od.dw, a.L * 128);
        stage_commit<NRAW, VAE_NT>(raw, rraw);
        __syncthreads();
        UpC1::build_weff(raw, We1);
        UpC2::build_weff(raw + (od.c2w - od.c1w), We2);
        UpC3::build_weff(raw + (od.c3w - od.c1w), We3);
    }
    const real gscale = (a.geco ? a.state[SVGP_ST_LAGRANGE] * a.inv_bglobal : real(1)) / real(784);
    for (int n = first; n < a.b; n += stride) {
        __syncthreads();
        if (n != first) {                // later images: one group per image
            ra1 = stage_issue<512, VAE_NT>(a.a1g + (size_t)n * 512);
            ra2 = stage_issue<1568, VAE_NT>(a.a2g + (size_t)n * 1568);
            rrec = stage_issue<784, VAE_NT>(a.recon + (size_t)n * 784);
            rpx = stage_issue<784, VAE_NT>(a.images + (size_t)n * 784);
        }
        stage_commit<512, VAE_NT>(a1, ra1);
        stage_commit<1568, VAE_NT>(a2, ra2);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = (int)threadIdx.x + k * VAE_NT;
            const real o = rrec.v[k];
            if (i < 784) d3[i] = real(2) * gscale * (o - rpx.v[k]) * elu_grad_from_out(o);
        }
        __syncthreads();
        UpC3::bwd_data_valu(d3, We3, d2);
        __syncthreads();
        for (int i = threadIdx.x; i < 1568; i += blockDim.x) {
            const real v = d2[i] * elu_grad_from_out(a2[i]);
            d2[i] = v;
            a.d2g[(size_t)n * 1568 + i] = v;
        }
        svgp_lds_barrier();             // (the stores to d2g / d1g / dh0g are for a later launch: no wave waits for them here)
        UpC2::bwd_data_mfma(d2, We2, d1);
        svgp_lds_barrier();
        for (int i = threadIdx.x; i < 512; i += blockDim.x) {
            const real v = d1[i] * elu_grad_from_out(a1[i]);
            d1[i] = v;
            a.d1g[(size_t)n * 512 + i] = v;
        }
        svgp_lds_barrier();
        UpC1::bwd_data_mfma(d1, We1, dh0);
        svgp_lds_barrier();
        if (threadIdx.x < 128) a.dh0g[(size_t)n * 128 + threadIdx.x] = dh0[threadIdx.x];
        // zbar[i] = sum_j dh0[j] w[i][j]: 8 lanes per latent channel, xor-shuffle combine
        {
            const int i = threadIdx.x >> 3, part8 = threadIdx.x & 7;
            real acc = 0;
            if (i < a.L)
                for (int j = part8; j < 128; j += 8) acc += dh0[j] * w[i * 128 + j];
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (i < a.L && part8 == 0) a.zbar[(size_t)n * a.L + i] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// decoder forward + reverse DATA half in one image loop (m <= 64 training step, SVGP_DEC_FUSE): what svgp_mnist_decoder_fwd_pre
// followed by svgp_mnist_decoder_bwd_data_pre compute, same expressions in the same order, hence the same bits.  Workgroup n of the
// second launch consumed only what workgroup n of the first produced: here a1, a2, recon and the weights stay in LDS between the
// halves, the image pixels stay in registers (thread t owns pixels t and t + 512: squared error AND d3), d3 overwrites the
// reconstruction in place.  Only the dense weights, the biases and ws.dec_weff are staged (the raw convolution weights are never
// read in the `_pre` form): dec_fwd_bwd_lds(L) reals, 75.9 KB at L = 16, so two workgroups fit a CU (the rider form,
// k_decoder_fwd_bwd_data in gp_kernels.hip, relies on that and on <= 168 VGPRs: the forward runs its rolled-tap form).
// The LDS image of ws.dec_weff is NOT a copy: the staging loop places class c of a layer at c * WCS instead of c * 4 CIN COUT
// (UpC1L / UpC2L / UpC3L and dec_weff_lds_index below; 54 doubles of padding in all), which is what the rolled forward's 16-byte
// weight reads need to be conflict-free, and the three layers' forward, the VALU data reverse of UpC3 and the `wo` tables of the two
// MFMA data reverses address it through the same WCS.  A tap trip of the forward is one group of LDS reads (tap_operand_group: 4
// activation + 8 weight ds_read_b128 in UpC1 / UpC2, 4 + 4 in UpC3) with counted waits.  NOTEBOOK 14.5e.
// The z / pixel loads of an image are issued one image ahead (the first: before the weight staging).  The staging behind them is
// still lds_copy_in: twelve dependent round trips.  Staged in groups (stage_issue / stage_copy above) the launch with its riders was
// no faster stand-alone and the straight-line form cost six registers (170 > 168), so this kernel kept the loops (NOTEBOOK 14.5c).
// The phase timeline (PROBE, NOTEBOOK 14.5d) puts entry -> weights staged at 3.0 us of the launch's 26, launch ramp included; with
// the branch-free forward the kernel is at 160 - 162 VGPRs and the straight-line group fits (166 / 166 / 165): it shortens the launch
// without riders by 0.4 us and the launch with riders, the form the step runs, by nothing (25.89 against 25.87 us), so the loops stay
// (NOTEBOOK 14.5d).
// PROBE: the phase-timeline instance (probe_stamp above); `probe` is the workgroup's row of stamps.
// The squared-error partial of a workgroup goes to part_sums[4 * first + 2].
// ------------------------------------------------------------------------------------------
struct DecFwdBwdArgs {
    int b, L, geco;
    real inv_bglobal;
    const real* state; const real* th_dec; const real* images; const real* zg; const real* weff;
    real* h0g; real* a1g; real* a2g; real* recon; real* part_sums;
    real* d2g; real* d1g; real* dh0g; real* zbar;
};
// The LDS image of the effective weights in this launch: ws.dec_weff with the class stride of each layer padded, so that the four
// parity classes fall on disjoint windows of the 64-bank (256-byte) row of ds_read_b128.  In UpC1 / UpC2 the 16 lanes of a read
// group are 4 output pixels x 4 channel pairs: a class needs 4 x 16 B = 64 B per (tap, ci), so the stride is 64 B past a multiple
// of the row (256 + 8 doubles).  In UpC3 a lane is a pixel and a class needs 16 B per (tap, ci pair): 32 + 2 doubles.  Lanes of one
// class read one address per channel pair (broadcast), lanes of different classes no common bank.  Only this launch uses the image;
// ws.dec_weff itself, the riders and every other kernel keep the packed layout.
// The same launch pads the PIXEL stride of three of its 8-channel activation arrays (packed: 8 doubles), for the reads that gather
// pixels a fixed distance apart (tools/lds_bank_model.py has the conflict degrees, NOTEBOOK 14.5f the measurements):
//   d2 (14 x 14), read by the UpC2 data reverse: ds_read_b64 of 16 pixels x 2 channels, input stride 2.  Packed, two neighbours are
//      128 bytes apart: 7.2 distinct addresses on the busiest bank in the mean; at 9 doubles 2.2.
//   d1 (8 x 8), read by the UpC1 data reverse, the same gather: 7.1 -> 2.1.
//   a2 (14 x 14), read by the UpC3 forward: ds_read_b128 of 16 output pixels = 8 to 9 source pixels 64 bytes apart, so pixels sx and
//      sx + 4 share banks: 3.0 -> 1.3 at 10 doubles (even: the 16-byte reads stay aligned).
// Only the LDS side moves: a2g, d2g and d1g keep the packed layout (dec_act_index in the copy-outs and the two elu' passes), and the
// arithmetic is untouched.  DEC_ACT_STRIDE_*: overridable on the compiler's command line to measure a piece alone (8 = packed).
#ifndef DEC_ACT_STRIDE_D2
#define DEC_ACT_STRIDE_D2 9
#endif
#ifndef DEC_ACT_STRIDE_D1
#define DEC_ACT_STRIDE_D1 9
#endif
#ifndef DEC_ACT_STRIDE_A2
#define DEC_ACT_STRIDE_A2 10
#endif
constexpr int DEC_S_D2 = DEC_ACT_STRIDE_D2, DEC_S_D1 = DEC_ACT_STRIDE_D1, DEC_S_A2 = DEC_ACT_STRIDE_A2;
static_assert(DEC_S_D2 >= 8 && DEC_S_D1 >= 8 && DEC_S_A2 >= 8 && DEC_S_A2 % 2 == 0, "pixel strides of d2, d1, a2 in the fused launch");
// packed index i = pixel * 8 + channel of an 8-channel activation array -> index at pixel stride S
template <int S>
__host__ __device__ constexpr int dec_act_index(int i) { return S == 8 ? i : (i >> 3) * S + (i & 7); }
using UpC1L = UpConv3<4, 1, 8, 8, VAE_NT, 256 + 8, 8, 8, DEC_S_D1, 8>;                 // h0 -> a1;  d1 -> dh0
using UpC2L = UpConv3<8, 0, 8, 8, VAE_NT, 256 + 8, 8, DEC_S_A2, DEC_S_D2, DEC_S_D1>;   // a1 -> a2;  d2 -> d1
using UpC3L = UpConv3<14, 1, 8, 1, VAE_NT, 32 + 2, DEC_S_A2, 1, 1, DEC_S_D2>;          // a2 -> recon;  d3 -> d2
#define DEC_LWE (UpC1L::LWE + UpC2L::LWE + UpC3L::LWE)      // 1048 + 1048 + 134 = 2230
static_assert(UpC1L::LWE % 2 == 0 && UpC2L::LWE % 2 == 0, "the three images start 16-byte aligned");
// offset in the image (doubles from We1) of element e of layer 0..2, packed index (class, tap, ci, co); e = NWE gives the layer's end
__host__ __device__ constexpr int dec_weff_lds_offset(int layer, int e) {
    return layer == 0   ? (e < UpC1::NWE ? UpC1L::lds_index(e) : UpC1L::LWE)
           : layer == 1 ? UpC1L::LWE + (e < UpC2::NWE ? UpC2L::lds_index(e) : UpC2L::LWE)
                        : UpC1L::LWE + UpC2L::LWE + (e < UpC3::NWE ? UpC3L::lds_index(e) : UpC3L::LWE);
}
// ... of element i of ws.dec_weff (the three layers back to back)
__host__ __device__ constexpr int dec_weff_lds_index(int i) {
    return i < UpC1::NWE               ? dec_weff_lds_offset(0, i)
           : i < UpC1::NWE + UpC2::NWE ? dec_weff_lds_offset(1, i - UpC1::NWE)
                                       : dec_weff_lds_offset(2, i - UpC1::NWE - UpC2::NWE);
}
// doubles in front of the image in the launch's LDS block: dense weights L * 128 | dense bias 128 | convolution biases 32
__host__ __device__ constexpr int dec_fwd_bwd_we_offset(int L) { return L * 128 + 128 + 32; }
// even for every L (128 L is even whatever L is: checking two consecutive L covers the constant): with the block 16-byte aligned
// (`extern __shared__ __align__(16)`) We1, and with the even LWE above We2 and We3, are 16-byte aligned, as fwd_valu<true, true> needs
static_assert(dec_fwd_bwd_we_offset(1) % 2 == 0 && dec_fwd_bwd_we_offset(2) % 2 == 0 && 128 % 2 == 0, "We1 16-byte aligned");
__host__ __device__ constexpr int dec_fwd_bwd_lds(int L) {
    return dec_fwd_bwd_we_offset(L) + DEC_LWE + 64 + 128 + 512 + 1568 + 784 + 1568 + 512 + 128 + 16;
}
static_assert(dec_fwd_bwd_lds(16) * 8 <= 80 * 1024, "two workgroups per CU at L = 16");
// The arrays of the block: offset and extent in doubles, pixel stride (0: no pixel structure), and the live interval in terms of the
// probe stamps 1..14 of the image loop below -- stamp k closes phase k, every phase ends in a barrier, and an array is live from the
// phase of its first write to the phase of its last read of an image.  The sum above is the PACKED map's and stays the footprint
// (77 744 bytes at L = 16: two workgroups per CU); the padding of a2 and d2 (392 + 196 doubles at strides 10 and 9) is paid for by two
// aliases of arrays that are never live together, and what remains (52 doubles behind `red`) is unused:
//   d1 lies in the d3 block: d3 is last read by the UpC3 data reverse (phase 8), d1 first written by the UpC2 data reverse (10);
//   dh0 lies on h0: h0 is last read by its copy-out (phase 7), dh0 first written by the UpC1 data reverse (12).
// Each interval lies inside one trip of the image loop (first <= last, written before read in every trip), so a workgroup that walks
// several images meets the aliased blocks in the same order every time: d3 (6..8) | d1 (10..12) | d3 of the next image, ...
enum { DEC_LDS_DENSE = 0, DEC_LDS_WEFF, DEC_LDS_Z, DEC_LDS_H0, DEC_LDS_A1, DEC_LDS_A2, DEC_LDS_D3, DEC_LDS_D2, DEC_LDS_D1, DEC_LDS_DH0,
       DEC_LDS_RED, DEC_LDS_NARRAYS };
struct DecLdsArray { int offset, extent, stride, first, last; };
__host__ __device__ constexpr DecLdsArray dec_fwd_bwd_lds_array(int L, int which) {
    const int z = dec_fwd_bwd_we_offset(L) + DEC_LWE, a2 = z + 64 + 128 + 512, d3 = a2 + 196 * DEC_S_A2, d2 = d3 + 784;
    switch (which) {
    case DEC_LDS_DENSE: return {0, dec_fwd_bwd_we_offset(L), 0, 1, 13};   // dense weights | dense bias | convolution biases: staged once
    case DEC_LDS_WEFF: return {dec_fwd_bwd_we_offset(L), DEC_LWE, 0, 1, 12};   // effective weights: staged once, last the UpC1 data reverse
    case DEC_LDS_Z: return {z, 64, 0, 2, 3};                              // z (2) -> dense (3)
    case DEC_LDS_H0: return {z + 64, 128, 8, 3, 7};                       // dense (3) -> UpC1 forward (4), copy-out (7)
    case DEC_LDS_A1: return {z + 64 + 128, 512, 8, 4, 11};                // UpC1 forward (4) -> UpC2 forward (5), copy-out (7), d1 elu' (11)
    case DEC_LDS_A2: return {a2, 196 * DEC_S_A2, DEC_S_A2, 5, 9};         // UpC2 forward (5) -> UpC3 forward (6), copy-out (7), d2 elu' (9)
    case DEC_LDS_D3: return {d3, 784, 1, 6, 8};                           // reconstruction (6), d3 in place (7) -> UpC3 data reverse (8)
    case DEC_LDS_D2: return {d2, 196 * DEC_S_D2, DEC_S_D2, 8, 10};        // UpC3 data reverse (8), elu' (9) -> UpC2 data reverse (10)
    case DEC_LDS_D1: return {d3, 64 * DEC_S_D1, DEC_S_D1, 10, 12};        // UpC2 data reverse (10), elu' (11) -> UpC1 data reverse (12)
    case DEC_LDS_DH0: return {z + 64, 128, 8, 12, 13};                    // UpC1 data reverse (12) -> store, z-bar (13)
    case DEC_LDS_RED: return {d2 + 196 * DEC_S_D2, 16, 0, 14, 14};        // the squared-error sum, after the loop
    default: return {-1, -1, -1, -1, -1};
    }
}
static_assert(64 * DEC_S_D1 <= 784, "d1 inside the d3 block");
static_assert(dec_fwd_bwd_lds_array(1, DEC_LDS_RED).offset + 16 <= dec_fwd_bwd_lds(1) &&
              dec_fwd_bwd_lds_array(2, DEC_LDS_RED).offset + 16 <= dec_fwd_bwd_lds(2), "the padded map inside the packed footprint");
static_assert(dec_fwd_bwd_lds_array(1, DEC_LDS_A2).offset % 2 == 0 && dec_fwd_bwd_lds_array(2, DEC_LDS_A2).offset % 2 == 0,
              "a2 16-byte aligned (the activation reads of UpC3L::fwd_valu<true, true>)");
// index in its block of packed element i (pixel * channels + channel) of array `which`; only a2, d2 and d1 are not the identity
__host__ __device__ constexpr int dec_fwd_bwd_lds_index(int which, int i) {
    return which == DEC_LDS_A2 ? dec_act_index<DEC_S_A2>(i) : which == DEC_LDS_D2 ? dec_act_index<DEC_S_D2>(i)
           : which == DEC_LDS_D1 ? dec_act_index<DEC_S_D1>(i) : i;
}
template <bool PROBE = false>
__device__ __forceinline__ void decoder_fwd_bwd_data_images(const DecFwdBwdArgs& a, int first, int stride, real* smem,
                                                            unsigned long long* probe = nullptr) {
    const DecOff od = dec_off(a.L);
    real* w = smem;                  // dense weights L*128 | dense bias 128 (contiguous in theta)
    real* db = w + a.L * 128;
    real* cb = db + 128;             // c1b (8) | c2b (8) | c3b (1)
    real* We1 = smem + dec_fwd_bwd_we_offset(a.L);   // = cb + 32: effective weights, padded class strides (dec_weff_lds_index), 16-byte aligned
    real* We2 = We1 + UpC1L::LWE;
    real* We3 = We2 + UpC2L::LWE;
    // (dec_fwd_bwd_lds_array above: the map the host entries report, with each array's live interval in probe stamps)
    real* z = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_Z).offset;       // 64                                     live  2 ..  3
    real* h0 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_H0).offset;     // 128                                          3 ..  7
    real* a1 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_A1).offset;     // 512                                          4 .. 11
    real* a2 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_A2).offset;     // 196 pixels x DEC_S_A2                        5 ..  9
    real* d3 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_D3).offset;     // 784: the reconstruction, then d3 in place    6 ..  8
    real* d2 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_D2).offset;     // 196 pixels x DEC_S_D2                        8 .. 10
    real* d1 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_D1).offset;     // 64 pixels x DEC_S_D1, IN THE d3 BLOCK       10 .. 12
    real* dh0 = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_DH0).offset;   // 128, ON h0                                  12 .. 13
    real* red = smem + dec_fwd_bwd_lds_array(a.L, DEC_LDS_RED).offset;   // 16                                          14
    const int t = threadIdx.x;
    const real lag = a.geco ? a.state[SVGP_ST_LAGRANGE] : real(0);
    // image `first` exists for every workgroup (the grid has min(b, 256) image workgroups)
    real zr = t < a.L ? a.zg[(size_t)first * a.L + t] : real(0);
    real px0 = a.images[(size_t)first * 784 + t];
    real px1 = t + VAE_NT < 784 ? a.images[(size_t)first * 784 + t + VAE_NT] : real(0);
    lds_copy_in(w, a.th_dec + od.dw, a.L * 128 + 128);
    if (t < 8) { cb[t] = a.th_dec[od.c1b + t]; cb[8 + t] = a.th_dec[od.c2b + t]; }
    if (t == 0) cb[16] = a.th_dec[od.c3b];
    for (int i = t; i < DEC_NWE; i += blockDim.x) We1[dec_weff_lds_index(i)] = a.weff[i];     // lds_copy_in with the index remap
    const real gscale = (a.geco ? lag * a.inv_bglobal : real(1)) / real(784);
    real sq = 0;
    // (probe slots 2..13 are those of the workgroup's LAST image)
    for (int n = first; n < a.b; n += stride) {
        __syncthreads();
        if (n == first) probe_stamp<PROBE>(probe, 1);       // weight staging
        if (t < a.L) z[t] = zr;
        __syncthreads();
        probe_stamp<PROBE>(probe, 2);       // z
        if (t < 128) {
            real acc = db[t];
            for (int i = 0; i < a.L; ++i) acc += z[i] * w[i * 128 + t];
            h0[t] = acc;
        }
        __syncthreads();
        probe_stamp<PROBE>(probe, 3);       // dense
        UpC1L::fwd_valu<true, true>(h0, We1, cb, a1);
        __syncthreads();
        probe_stamp<PROBE>(probe, 4);       // UpC1 forward
        UpC2L::fwd_valu<true, true>(a1, We2, cb + 8, a2);
        __syncthreads();
        probe_stamp<PROBE>(probe, 5);       // UpC2 forward
        UpC3L::fwd_valu<true, true>(a2, We3, cb + 16, d3);
        __syncthreads();
        probe_stamp<PROBE>(probe, 6);       // UpC3 forward
        lds_copy_out(a.h0g + (size_t)n * 128, h0, 128);
        lds_copy_out(a.a1g + (size_t)n * 512, a1, 512);
        lds_copy_out_px<DEC_S_A2>(a.a2g + (size_t)n * 1568, a2, 1568);
        {   // pixels t and t + 512: reconstruction out, squared error, d3 in place (each element read and written by its one owner)
            const real o = d3[t];
            a.recon[(size_t)n * 784 + t] = o;
            const real df = px0 - o;
            sq += df * df;
            d3[t] = real(2) * gscale * (o - px0) * elu_grad_from_out(o);
            if (t + VAE_NT < 784) {
                const real o1 = d3[t + VAE_NT];
                a.recon[(size_t)n * 784 + t + VAE_NT] = o1;
                const real df1 = px1 - o1;
                sq += df1 * df1;
                d3[t + VAE_NT] = real(2) * gscale * (o1 - px1) * elu_grad_from_out(o1);
            }
        }
        {   // the next image's z and pixels: in flight during the reverse half
            const int nn = n + stride;
            if (nn < a.b) {
                zr = t < a.L ? a.zg[(size_t)nn * a.L + t] : real(0);
                px0 = a.images[(size_t)nn * 784 + t];
                px1 = t + VAE_NT < 784 ? a.images[(size_t)nn * 784 + t + VAE_NT] : real(0);
            }
        }
        __syncthreads();
        probe_stamp<PROBE>(probe, 7);       // copy-outs, squared error, d3, next image's loads issued
        UpC3L::bwd_data_valu(d3, We3, d2);
        __syncthreads();
        probe_stamp<PROBE>(probe, 8);       // UpC3 data-reverse
        int tl = t;
        if constexpr (DEC_S_D2 != 8 || DEC_S_A2 != 8 || DEC_S_D1 != 8) asm volatile("" : "+v"(tl));
        for (int i = t, il = tl; i < 1568; i += VAE_NT, il += VAE_NT) {
            const int j = dec_act_index<DEC_S_D2>(il);
            const real v = d2[j] * elu_grad_from_out(a2[dec_act_index<DEC_S_A2>(il)]);
            d2[j] = v;
            a.d2g[(size_t)n * 1568 + i] = v;
        }
        svgp_lds_barrier();             // (the stores to d2g / d1g / dh0g are for a later launch: no wave waits for them here)
        probe_stamp<PROBE>(probe, 9);       // d2 = d2 * elu', stored
        UpC2L::bwd_data_mfma(d2, We2, d1);
        svgp_lds_barrier();
        probe_stamp<PROBE>(probe, 10);      // UpC2 data-reverse
        if constexpr (DEC_S_D1 != 8) asm volatile("" : "+v"(tl));
        for (int i = t; i < 512; i += VAE_NT) {
            const int j = dec_act_index<DEC_S_D1>(tl);
            const real v = d1[j] * elu_grad_from_out(a1[i]);
            d1[j] = v;
            a.d1g[(size_t)n * 512 + i] = v;
        }
        svgp_lds_barrier();
        probe_stamp<PROBE>(probe, 11);      // d1 = d1 * elu', stored
        UpC1L::bwd_data_mfma(d1, We1, dh0);
        svgp_lds_barrier();
        probe_stamp<PROBE>(probe, 12);      // UpC1 data-reverse
        if (t < 128) a.dh0g[(size_t)n * 128 + t] = dh0[t];
        // zbar[i] = sum_j dh0[j] w[i][j]: 8 lanes per latent channel, xor-shuffle combine
        {
            const int i = t >> 3, part8 = t & 7;
            real acc = 0;
            if (i < a.L)
                for (int j = part8; j < 128; j += 8) acc += dh0[j] * w[i * 128 + j];
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (i < a.L && part8 == 0) a.zbar[(size_t)n * a.L + i] = acc;
        }
        if constexpr (PROBE) __syncthreads();
        probe_stamp<PROBE>(probe, 13);      // z-bar
    }
    const real tot = block_sum(sq, red);
    if (t == 0) a.part_sums[first * 4 + 2] = tot;
    probe_stamp<PROBE>(probe, 14);          // exit
}

// ------------------------------------------------------------------------------------------
// encoder reverse: (ybar, s2bar) -> encoder weight-gradient partials; one workgroup of NT threads walks images first,
// first + stride, ...; partial slot = first.  LDS: enc_bwd_lds(n_enc) reals (75 KB at L = 16: the launch that carries the
// kernel-matrix VJP as well, svgp_mnist_encoder_bwd_km, holds a VJP workgroup and an image workgroup on one CU).
// Reference semantics: tf.gradients of VAE_utils.py:112-126,143-152 w.r.t. the encoder variables (MNIST_experiment.py:202-205).
// ------------------------------------------------------------------------------------------
struct EncBwdArgs {
    int b, L, clip;
    const real* th_enc; const real* images; const real* a1g; const real* a2g; const real* a3g; const real* var_raw;
    const real* ybar; const real* s2bar;
    real* part;                          // (n_part, eo.n)
};
#define ENC_BWD_SCRATCH 512              // 72 outputs x 7 pixel chunks of the first layer's weight gradient; 256 for the bias sums
__host__ __device__ constexpr int enc_bwd_lds(int n_enc) {
    return 2 * n_enc + 784 + 1352 + 288 + 32 + 1352 + 288 + 32 + 128 + ENC_BWD_SCRATCH;
}

template <int NT>
__device__ __forceinline__ void encoder_bwd_images(const EncBwdArgs& a, int first, int stride, real* smem) {
    const int L = a.L;
    const EncOff eo = enc_off(L);
    real* w = smem;                  // eo.n
    real* g = w + eo.n;              // eo.n   gradient accumulators
    real* img = g + eo.n;            // 784
    real* a1 = img + 784;            // 1352
    real* a2 = a1 + 1352;            // 288
    real* a3 = a2 + 288;             // 32
    real* d1 = a3 + 32;              // 1352
    real* d2 = d1 + 1352;            // 288
    real* d3 = d2 + 288;             // 32
    real* dout = d3 + 32;            // 2L (<=128)
    real* scratch = dout + 128;      // ENC_BWD_SCRATCH
    using C1 = Conv3<28, 1, 0, 2, 1, 8, 13, NT>;
    using C2 = Conv3<13, 1, 0, 2, 8, 8, 6, NT>;
    using C3 = Conv3<6, 1, 0, 2, 8, 8, 2, NT>;
    static_assert(72 * (NT / 72) <= ENC_BWD_SCRATCH, "first-layer chunk scratch");
    static_assert(NT >= 128, "thread j stages dout[j], j < 2L <= 128");
    const int twoL = 2 * L, t = threadIdx.x;
    // One group of loads per image: pixels, a1, a2, a3 and the three inputs of dout[t] (10 values per thread; all three of the last
    // unconditional, from clamped rows).  The first image's group is issued ahead of the weight staging and flies with its first chunk.
    const int jy = t < L ? t : L - 1, jv = t < L ? 0 : t < twoL ? t - L : L - 1;
    StageRegs<784, NT> rimg; StageRegs<1352, NT> ra1; StageRegs<288, NT> ra2; StageRegs<32, NT> ra3;
    real ryb, rvr, rsb;
    auto issue = [&](int n) {
        rimg = stage_issue<784, NT>(a.images + (size_t)n * 784);
        ra1 = stage_issue<1352, NT>(a.a1g + (size_t)n * 1352);
        ra2 = stage_issue<288, NT>(a.a2g + (size_t)n * 288);
        ra3 = stage_issue<32, NT>(a.a3g + (size_t)n * 32);
        ryb = a.ybar[(size_t)n * L + jy];
        rvr = a.var_raw[(size_t)n * L + jv];
        rsb = a.s2bar[(size_t)n * L + jv];
    };
    issue(first < a.b ? first : a.b - 1);
    stage_copy<NT>(w, a.th_enc, eo.n);
    for (int i = t; i < eo.n; i += NT) g[i] = 0;
    for (int n = first; n < a.b; n += stride) {
        __syncthreads();
        if (n != first) issue(n);
        stage_commit<784, NT>(img, rimg);
        stage_commit<1352, NT>(a1, ra1);
        stage_commit<288, NT>(a2, ra2);
        stage_commit<32, NT>(a3, ra3);
        if (t < twoL) {
            const bool pass = !a.clip || (rvr >= 1e-3 && rvr <= 10.0);
            dout[t] = t < L ? ryb : pass ? rsb * rvr : real(0);
        }
        __syncthreads();
        // dense: weight / bias gradients and da3
        for (int o = threadIdx.x; o < 32 * twoL; o += NT) g[eo.dw + o] += a3[o / twoL] * dout[o % twoL];
        for (int j = threadIdx.x; j < twoL; j += NT) g[eo.db + j] += dout[j];
        if (threadIdx.x < 32) {
            real acc = 0;
            for (int j = 0; j < twoL; ++j) acc += dout[j] * w[eo.dw + threadIdx.x * twoL + j];
            d3[threadIdx.x] = acc * elu_grad_from_out(a3[threadIdx.x]);
        }
        __syncthreads();
        C3::bwd_weight(a2, d3, g + eo.c3w, g + eo.c3b, scratch);
        C3::bwd_data(d3, w + eo.c3w, d2);
        __syncthreads();
        for (int i = threadIdx.x; i < 288; i += NT) d2[i] *= elu_grad_from_out(a2[i]);
        __syncthreads();
        C2::bwd_weight(a1, d2, g + eo.c2w, g + eo.c2b, scratch);
        C2::bwd_data(d2, w + eo.c2w, d1);
        __syncthreads();
        for (int i = threadIdx.x; i < 1352; i += NT) d1[i] *= elu_grad_from_out(a1[i]);
        __syncthreads();
        C1::bwd_weight(img, d1, g + eo.c1w, g + eo.c1b, scratch);
    }
    __syncthreads();
    lds_copy_out(a.part + (size_t)first * eo.n, g, eo.n);
}

}  // namespace svgp_vae

// vae_mnist.hip: the weight half's arguments from a configuration + workspace (riders of the reverse factor launch, gp_kernels.hip)
svgp_vae::DecWgradArgs svgp_make_dec_wgrad_args(const svgp_mnist_cfg* c, const svgp_mnist_ws_layout& wl, const double* images,
                                                double* ws, const double* state, int n_types);
svgp_vae::DecBwdDataArgs svgp_make_dec_bwd_data_args(const svgp_mnist_cfg* c, const svgp_mnist_ws_layout& wl, const double* theta,
                                                     const double* images, double* ws, const double* state);
svgp_vae::EncBwdArgs svgp_make_enc_bwd_args(const svgp_mnist_cfg* c, const svgp_mnist_ws_layout& wl, const double* theta,
                                            const double* images, double* ws);
