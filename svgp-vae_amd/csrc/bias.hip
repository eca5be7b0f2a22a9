// Bias analysis of the inducing mean vector (supplement C.4; MNIST_experiment.py:325-363, utils.py:922-948): the running sum of
// the per-step mean vectors mu_hat (L, m) over an epoch, kept on the device, and at the epoch's end its distance from the
// whole-train-set vector.
#include "common.hpp"

namespace {

// acc (n + 1): element i < n += x[i], element n (the step count) += 1.  One thread per element, plain loads and stores: after k
// launches acc is the left-to-right float64 sum of the k inputs, the order of the reference's `+=` (utils.py:937-942).
__global__ void k_mean_vectors_accumulate(int n, const real* __restrict__ x, real* __restrict__ acc) {
    const int i = blockIdx.x * SVGP_BLOCK + threadIdx.x;
    if (i < n) acc[i] += x[i];
    else if (i == n) acc[n] += real(1);
}

// ONE workgroup.  Channel by channel: thread t adds the terms |acc[l][j] / B - full[l][j]| of j = t, t + 256, ... in that order,
// the 256 partial sums are folded in LDS by halves; thread 0 stores the channel sum and adds it to the total in channel order.
// Nothing depends on timing or on the grid, so a repeated call gives the same bits.  B = 0: 0 / 0 and x / 0 do what IEEE says.
__global__ void __launch_bounds__(SVGP_BLOCK) k_mean_vectors_bias(int L, int m, const real* __restrict__ acc,
                                                                  const real* __restrict__ full, real* __restrict__ out) {
    __shared__ real red[SVGP_BLOCK];
    const int t = threadIdx.x;
    const real B = acc[(size_t)L * m];
    real total = real(0);
    for (int l = 0; l < L; ++l) {
        const real* a = acc + (size_t)l * m;
        const real* f = full + (size_t)l * m;
        real s = real(0);
        for (int j = t; j < m; j += SVGP_BLOCK) s += fabs(a[j] / B - f[j]);
        red[t] = s;
        __syncthreads();
        for (int h = SVGP_BLOCK / 2; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) {
            out[1 + l] = red[0];
            total += red[0];
        }
        __syncthreads();        // red[] is rewritten by the next channel
    }
    if (t == 0) out[0] = total / (real)L;
}

int check_shape(int L, int m) {
    SVGP_REQUIRE(L >= 1 && m >= 1, SVGP_ERR_INVALID, "bad shape L=%d m=%d", L, m);
    SVGP_REQUIRE(m <= SVGP_M_LIMIT, SVGP_ERR_UNSUPPORTED, "m=%d inducing points: this build supports m <= %d", m, SVGP_M_LIMIT);
    return SVGP_OK;
}

}  // namespace

extern "C" int svgp_mean_vectors_accumulate(int L, int m, const double* mu_hat, double* acc, void* stream) {
    int rc = check_shape(L, m);
    if (rc) return rc;
    SVGP_REQUIRE(mu_hat && acc, SVGP_ERR_INVALID, "NULL device pointer");
    const long long n = (long long)L * m;
    SVGP_REQUIRE(n < (1LL << 30), SVGP_ERR_UNSUPPORTED, "L * m = %lld elements: more than 2^30 are not supported", n);
    const int nblk = (int)((n + 1 + SVGP_BLOCK - 1) / SVGP_BLOCK);
    hipLaunchKernelGGL(k_mean_vectors_accumulate, dim3(nblk), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, (int)n, mu_hat, acc);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}

extern "C" int svgp_mean_vectors_bias(int L, int m, const double* acc, const double* full, double* out, void* stream) {
    int rc = check_shape(L, m);
    if (rc) return rc;
    SVGP_REQUIRE(acc && full && out, SVGP_ERR_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(k_mean_vectors_bias, dim3(1), dim3(SVGP_BLOCK), 0, (hipStream_t)stream, L, m, acc, full, out);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}
