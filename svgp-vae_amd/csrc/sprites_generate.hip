// SPRITES conditional generation from a posterior cache: the latent rows of a new character in one call.
//
// Reference semantics: spritesSVGP.approximate_posterior_params_precomputed_GP_posterior_params (SVGPVAE_model.py:610-635) and the
// clip / draw of predict_SVGPVAE_sprites_test_character (:1180-1183).  With w_l = Sigma_l^-1 K_mn (mu_l / var_l) (L, m) and
// X_l = Sigma_l^-1 - K_mm^-1 (L, m, m) formed once from the train set, a query row i with kernel row k_i = Kb[i, :] has
//   p_m[i, l] = k_i . w_l      p_v[i, l] = clamp(kbb[i] + k_i^T X_l k_i, clip_lo, clip_hi)      z = p_m + eps sqrt(p_v)
// X is used as written: nothing here assumes it symmetric (the jitter-free K_mm^-1 comes from a pivoted LU).
//
// Tiling.  Workgroup (rb, l) of 256 threads owns the PR_BR = 64 rows [64 rb, 64 rb + 64) of channel l and walks the 64-wide column
// tiles of T = Kb[rows, :] X_l, each a K loop over panels of 16 on the f64 MFMA (waves 2 x 2, 32 x 32 accumulators each).  When a
// column tile is complete its accumulators are multiplied by the matching Kb tile and added to eight per-lane row sums that live
// in registers across all column tiles; T itself is never stored.  p_m rides in the first column tile: the threads that stage the
// Kb panel multiply what they hold in registers by w_l.  Panels go from global memory to LDS through registers, two in flight.
// At the end the row sums are added over the 16 lanes of a row (xor shuffles), over the two waves that share the rows (LDS) and
// the epilogue writes the (b, L) outputs.  Every sum has a fixed order: the same inputs give the same bits, there is no atomic.
//
// Column split.  Up to m = 256 that is the whole call: one launch, no workspace.  Beyond, the grid of (row blocks, L) alone leaves
// the device unevenly filled (288 rows x 64 channels: 320 workgroups on 256 CUs), so the column tiles of a (row block, channel) are
// dealt to S <= 16 workgroups (rows_split: about 1024 workgroups in all); each writes its partial row sums to work (S, b, L) and
// k_sprites_posterior_finish adds the S partials of an element in index order, clamps and draws: two launches, S b L doubles.
#include "common.hpp"

namespace {

constexpr int PR_BR = 64;            // rows of a workgroup
constexpr int PR_BN = 64;            // columns of a column tile
constexpr int PR_GK = 16;            // K panel
constexpr int PR_LD = 80;            // LDS row stride of a panel (k-major): 80 mod 32 = 16, the four k rows of a fragment read fall
                                     // on disjoint bank halves
constexpr int PR_L_MAX = 64;

struct RowsArgs {
    int b, m, L;
    real lo, hi;
    const real* Kb; const real* kbb; const real* w; const real* X; const real* eps;
    real* p_m; real* p_v; real* z;
    int S; real* part;      // S > 1: column split, partial row sums (S, b, L)
};

__global__ __launch_bounds__(256, 2) void k_sprites_posterior_rows(RowsArgs a) {
    using MF = SvgpMfma<real>;
    __shared__ real As[2][PR_GK * PR_LD];
    __shared__ real Bs[2][PR_GK * PR_LD];
    __shared__ real red[2][PR_BR];
    __shared__ real pms[PR_BR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int m = a.m, l = blockIdx.y;
    const long long i0 = (long long)blockIdx.x * PR_BR;
    const real* __restrict__ Kb = a.Kb;
    const real* __restrict__ Xl = a.X + (size_t)l * m * m;
    const real* __restrict__ wl = a.w + (size_t)l * m;
    const int NK = (m + PR_GK - 1) / PR_GK, NJ = (m + PR_BN - 1) / PR_BN;
    const int sp = blockIdx.z, jt0 = sp * NJ / a.S, jt1 = (sp + 1) * NJ / a.S, NP = NK * (jt1 - jt0);      // this workgroup's column tiles
    // staging maps: Kb panel (64 rows x 16 k): row = tid / 4, k = tid % 4 + 4 c; X panel (16 k x 64 j): k = tid / 16, j = tid % 16 + 16 c
    const int ar = tid >> 2, ak = tid & 3, bk = tid >> 4, bj = tid & 15;
    const long long arow = i0 + ar;
    const bool arow_ok = arow < a.b;
    // a panel on its way from global memory to LDS: the Kb and X elements this thread stages, w_l beside them in the first column tile
    struct Regs { real a[4], b[4], w[4]; int jt; };
    real pm = 0;
    auto fetch = [&](Regs& R, int jt, int kp) {
        const int k0 = kp * PR_GK, j0 = jt * PR_BN;
        R.jt = jt;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = k0 + ak + 4 * c;
            R.a[c] = (arow_ok && k < m) ? Kb[(size_t)arow * m + k] : real(0);
            if (jt == 0) R.w[c] = k < m ? wl[k] : real(0);
        }
        const int kx = k0 + bk;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + bj + 16 * c;
            R.b[c] = (kx < m && j < m) ? Xl[(size_t)kx * m + j] : real(0);
        }
    };
    auto stage = [&](const Regs& R, int buf) {
#pragma unroll
        for (int c = 0; c < 4; ++c) As[buf][(ak + 4 * c) * PR_LD + ar] = R.a[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) Bs[buf][bk * PR_LD + bj + 16 * c] = R.b[c];
        if (R.jt == 0) {    // p_m rides in the first column tile (of split 0): this thread's k = ak + 4 c of every panel, ascending
#pragma unroll
            for (int c = 0; c < 4; ++c) pm += R.a[c] * R.w[c];
        }
    };
    auto next = [&](int& jt, int& kp) { if (++kp == NK) { kp = 0; ++jt; } };
    MF::acc_t acc[2][2];
    real rs[2][4];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rs[x][e] = 0;
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = MF::acc_t{0, 0, 0, 0};
    }
    // Two panels in flight: while panel p is multiplied out of LDS buffer cur, panel p + 1 waits in one register set (its loads were
    // issued a whole panel earlier) and the loads of panel p + 2 are issued into the other; after the MFMAs panel p + 1 goes to the
    // other LDS buffer.  One barrier per panel.  The two register sets swap roles, so the loop is unrolled by two.
    Regs R0, R1;
    int fj = jt0, fk = 0;                // the next panel to fetch
    fetch(R0, fj, fk); next(fj, fk);
    stage(R0, 0);
    if (NP > 1) { fetch(R0, fj, fk); next(fj, fk); }
    __syncthreads();
    int cur = 0, jt = jt0, kp = 0;       // the panel in buffer cur: K panel kp of column tile jt
    auto panel = [&](int p, const Regs& Rn, Regs& Rf) {      // Rn holds panel p + 1, Rf takes panel p + 2
        if (p + 2 < NP) { fetch(Rf, fj, fk); next(fj, fk); }
        const real* Ab = As[cur] + wi + r;
        const real* Bb = Bs[cur] + wj + r;
#pragma unroll
        for (int s = 0; s < PR_GK / 4; ++s) {
            real av[2], bv[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) av[x] = Ab[(4 * s + q) * PR_LD + 16 * x];
#pragma unroll
            for (int y = 0; y < 2; ++y) bv[y] = Bb[(4 * s + q) * PR_LD + 16 * y];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y) acc[x][y] = MF::mma(av[x], bv[y], acc[x][y]);
        }
        if (kp == NK - 1) {              // column tile complete: rs += T tile o Kb tile, then the accumulators start over
            const int j0 = jt * PR_BN;
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long long gi = i0 + wi + 16 * x + MF::row(q, e);
                        const int gj = j0 + wj + 16 * y + r;
                        if (gi < a.b && gj < m) rs[x][e] += acc[x][y][e] * Kb[(size_t)gi * m + gj];
                        acc[x][y][e] = 0;
                    }
        }
        if (p + 1 < NP) stage(Rn, cur ^ 1);
        __syncthreads();                 // buffer cur is read, buffer cur ^ 1 is written
        cur ^= 1;
        next(jt, kp);
    };
    for (int p = 0; p < NP; p += 2) {
        panel(p, R0, R1);
        if (p + 1 < NP) panel(p + 1, R1, R0);
    }
    // row sums: over the 16 lanes of a row, then over the two waves (wj = 0, 32) that share the rows; p_m: over the 4 threads of a row
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            real s = rs[x][e];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
            if (r == 0) red[wave & 1][wi + 16 * x + MF::row(q, e)] = s;
        }
    pm += __shfl_xor(pm, 1, 64);
    pm += __shfl_xor(pm, 2, 64);
    if (ak == 0) pms[ar] = pm;
    __syncthreads();
    if (tid < PR_BR) {
        const long long gi = i0 + tid;
        if (gi < a.b) {
            const size_t e = (size_t)gi * a.L + l;
            const real mean = pms[tid], qs = red[0][tid] + red[1][tid];
            if (sp == 0) a.p_m[e] = mean;
            if (a.S > 1) {
                a.part[(size_t)sp * a.b * a.L + e] = qs;
            } else {
                const real pv = clip_keep_nan(a.kbb[gi] + qs, a.lo, a.hi);
                a.p_v[e] = pv;
                if (a.z) a.z[e] = a.eps ? mean + a.eps[e] * sqrt(pv) : mean;
            }
        }
    }
}

// column split: element e = (i, l): the S partial row sums in index order, clamp, draw (p_m was written by split 0)
__global__ __launch_bounds__(SVGP_BLOCK) void k_sprites_posterior_finish(RowsArgs a) {
    const size_t n = (size_t)a.b * a.L, e = (size_t)blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (e >= n) return;
    real qs = a.part[e];
    for (int s = 1; s < a.S; ++s) qs += a.part[(size_t)s * n + e];
    const real pv = clip_keep_nan(a.kbb[e / a.L] + qs, a.lo, a.hi);
    a.p_v[e] = pv;
    if (a.z) a.z[e] = a.eps ? a.p_m[e] + a.eps[e] * sqrt(pv) : a.p_m[e];
}

// workgroups a (row block, channel) is dealt to: 1 up to m = 256 (one launch), else enough for about 1024 workgroups in all
int rows_split(const svgp_posterior_rows_cfg* c) {
    if (c->m <= 256) return 1;
    const long long base = (long long)((c->b + PR_BR - 1) / PR_BR) * c->L, want = (1024 + base - 1) / base;
    const int NJ = (c->m + PR_BN - 1) / PR_BN;
    const int S = want < 16 ? (int)want : 16;
    return S < NJ ? S : NJ;
}

int rows_check(const svgp_posterior_rows_cfg* c) {
    SVGP_REQUIRE(c != nullptr, SVGP_ERR_INVALID, "cfg is NULL");
    SVGP_REQUIRE(c->b >= 1, SVGP_ERR_INVALID, "need 1 <= b (b=%d)", c->b);
    SVGP_REQUIRE(c->m >= 1 && c->m <= SVGP_M_LIMIT, SVGP_ERR_INVALID, "need 1 <= m <= %d (m=%d)", SVGP_M_LIMIT, c->m);
    SVGP_REQUIRE(c->L >= 1 && c->L <= PR_L_MAX, SVGP_ERR_INVALID, "need 1 <= L <= %d (L=%d)", PR_L_MAX, c->L);
    SVGP_REQUIRE(c->clip_lo <= c->clip_hi, SVGP_ERR_INVALID, "need clip_lo <= clip_hi (%g, %g)", c->clip_lo, c->clip_hi);
    return SVGP_OK;
}

}  // namespace

extern "C" long long svgp_sprites_posterior_rows_workspace_elems(const svgp_posterior_rows_cfg* c) {
    if (rows_check(c)) return 0;
    const int S = rows_split(c);
    return S > 1 ? (long long)S * c->b * c->L : 0;      // the partial row sums of a column split; nothing grows with m
}

extern "C" int svgp_sprites_posterior_rows_route(const svgp_posterior_rows_cfg* c, char* buf, int cap) {
    SVGP_REQUIRE(buf && cap >= 1, SVGP_ERR_INVALID, "bad argument");
    int rc = rows_check(c);
    if (rc) return rc;
    int pos = 0;
    return svgp_route_append(buf, cap, &pos, rows_split(c) > 1 ? "%s\nk_sprites_posterior_finish\n" : "%s\n", "k_sprites_posterior_rows");
}

extern "C" int svgp_sprites_posterior_rows(const svgp_posterior_rows_cfg* c, const double* Kb, const double* kbb, const double* w,
                                           const double* X, const double* eps, double* p_m, double* p_v, double* z, double* work,
                                           void* stream) {
    int rc = rows_check(c);
    if (rc) return rc;
    SVGP_REQUIRE(Kb && kbb && w && X && p_m && p_v, SVGP_ERR_INVALID, "NULL device pointer");
    const int S = rows_split(c);
    SVGP_REQUIRE(S == 1 || work, SVGP_ERR_INVALID, "work is NULL (b = %d, m = %d, L = %d needs %lld doubles)", c->b, c->m, c->L,
                 (long long)S * c->b * c->L);
    RowsArgs a;
    a.b = c->b; a.m = c->m; a.L = c->L; a.lo = c->clip_lo; a.hi = c->clip_hi;
    a.Kb = Kb; a.kbb = kbb; a.w = w; a.X = X; a.eps = eps; a.p_m = p_m; a.p_v = p_v; a.z = z; a.S = S; a.part = work;
    const dim3 grid((unsigned)((c->b + PR_BR - 1) / PR_BR), (unsigned)c->L, (unsigned)S);
    hipLaunchKernelGGL(k_sprites_posterior_rows, grid, dim3(256), 0, (hipStream_t)stream, a);
    SVGP_LAUNCH_CHECK();
    if (S > 1) {
        const size_t n = (size_t)c->b * c->L;
        hipLaunchKernelGGL(k_sprites_posterior_finish, dim3(svgp_blocks((long long)n)), dim3(SVGP_BLOCK), 0,
                           (hipStream_t)stream, a);
        SVGP_LAUNCH_CHECK();
    }
    return SVGP_OK;
}
