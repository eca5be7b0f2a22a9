// In-place inverse of a small SPD matrix held in LDS, shared by the exact per-video GP of ball.hip and the moving-ball
// predictor of ball_predict.hip.  Device code only; include after common.hpp.
#pragma once

// Thread layout (256 threads), CW = 32 (n <= 32) or 64 columns: column j = tid & (CW-1), row lane i0 = tid / CW of RL = 256 / CW;
// a thread owns the elements (i0 + RL r, j).
// in-place Gauss-Jordan inverse of an SPD n x n LDS matrix (leading dimension ld, n <= 64), no pivoting; returns log det
template <int CW>
__device__ real lds_spd_inverse(real* A, int ld, int n, real* pivbuf) {
    constexpr int RL = 256 / CW, RMAX = CW / RL;
    const int j = threadIdx.x & (CW - 1), i0 = threadIdx.x / CW;
    real logdet = 0;
    for (int k = 0; k < n; ++k) {
        __syncthreads();
        const real piv = A[k * ld + k], ip = real(1) / piv;
        const real rowk = j < n ? A[k * ld + j] : real(0);
        real f[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) { const int i = i0 + RL * r; f[r] = i < n ? A[i * ld + k] * ip : real(0); }
        if (threadIdx.x == 0) pivbuf[k] = piv;           // the logs are taken once, in parallel, after the sweep
        __syncthreads();
        if (j < n) {
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                const int i = i0 + RL * r;
                if (i < n && i != k) A[i * ld + j] = (j == k) ? -f[r] : A[i * ld + j] - f[r] * rowk;
            }
            if (i0 == 0) A[k * ld + j] = (j == k) ? ip : rowk * ip;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {                              // n <= 64: one wave, fixed-order shuffle sum
        const real lg = wave_sum((int)threadIdx.x < n ? log(pivbuf[threadIdx.x]) : real(0));
        if (threadIdx.x == 0) pivbuf[0] = lg;
    }
    __syncthreads();
    logdet = pivbuf[0];
    __syncthreads();
    return logdet;
}
