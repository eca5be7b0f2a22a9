// Cubic-spline image rotation of the rotated-MNIST data set generator (utils.py:564-576: `ndimage.rotate(image, angle,
// reshape=False)` once per image and angle).  The semantics are scipy's defaults: order 3, mode 'constant', cval 0, prefilter on
// (DESIGN.md section 9c has the steps).  One workgroup per source image: the image goes to LDS, is turned into its B-spline
// coefficients in place (columns, then rows: one thread per line runs the recursion), and then every thread sweeps the
// A x H x W output pixels, reading the 4 x 4 coefficients of each from LDS.  The prefilter so runs once per image, not per angle.
#include "common.hpp"

#define SVGP_ROT_MAX 64        // H, W <= 64: 64 rows of pitch 65 doubles, 33 KB of LDS

// The helpers are host-and-device so that a host program can run the very same arithmetic; the library itself has no host path.
namespace {

// Row pitch in doubles: odd, so that the 32 lanes of a half-wave that walk 32 ROWS in step (the row pass) fall on 32 different
// 8-byte bank pairs (ds_read_b64: bank = (byte address / 4) mod 64).
__host__ __device__ inline int rot_pitch(int W) { return W | 1; }

// In-place cubic B-spline prefilter of one line c[0], c[st], ..., c[(n - 1) st], n >= 2, mirror boundary (period 2 (n - 1)): gain,
// the causal recursion c_i += z c_{i-1} started from the exact mirror sum, then c_i = z (c_{i+1} - c_i) downwards.
__host__ __device__ inline void rot_prefilter_line(real* c, int n, int st) {
    const real z = sqrt(real(3)) - real(2), gain = (real(1) - z) * (real(1) - real(1) / z);
    real zn1 = real(1);                                  // z^(n-1)
    for (int i = 0; i < n - 1; ++i) zn1 *= z;
    for (int i = 0; i < n; ++i) c[i * st] *= gain;
    real acc = c[0] + zn1 * c[(n - 1) * st], zi = z;
    for (int i = 1; i < n - 1; ++i) {
        acc += zi * (c[i * st] + zn1 * c[(n - 1 - i) * st]);
        zi *= z;
    }
    acc /= real(1) - zn1 * zn1;
    c[0] = acc;
    for (int i = 1; i < n; ++i) {
        acc = c[i * st] + z * acc;
        c[i * st] = acc;
    }
    acc = (z * c[(n - 2) * st] + acc) * z / (z * z - real(1));
    c[(n - 1) * st] = acc;
    for (int i = n - 2; i >= 0; --i) {
        acc = z * (acc - c[i * st]);
        c[i * st] = acc;
    }
}

// Input coordinates of output pixel (i, j) for the rotation matrix [[c, s], [-s, c]] about the image centre.  Every product and
// sum is rounded on its own, in the order of scipy's C loop (offset, + i * m0, + j * m1): the inside / outside decision below is
// then made on the same IEEE results as on the CPU.  A fused multiply-add here moves border pixels in and out of the image at
// the quarter turns.  HIP's __dmul_rn / __dadd_rn are the plain operators, which the compiler contracts like any other; what
// keeps the operations apart is the pragma (the build's -ffp-contract default honours it).
__host__ __device__ inline void rot_coords(int H, int W, real c, real s, int i, int j, real* cc0, real* cc1) {
#pragma clang fp contract(off)
    const real cen0 = real(H - 1) * real(0.5), cen1 = real(W - 1) * real(0.5);
    const real p00 = c * cen0, p01 = s * cen1, p10 = -s * cen0, p11 = c * cen1;
    const real off0 = cen0 - (p00 + p01), off1 = cen1 - (p10 + p11);
    const real i0 = real(i) * c, j0 = real(j) * s, i1 = real(i) * -s, j1 = real(j) * c;
    *cc0 = (off0 + i0) + j0;
    *cc1 = (off1 + i1) + j1;
}

// tap index idx in [-1, len + 1] folded into [0, len - 1] by reflection about the end samples (period 2 (len - 1)), len >= 2
__host__ __device__ inline int rot_mirror(int idx, int len) {
    const int period = 2 * len - 2, m = (idx + period) % period;
    return m < len ? m : period - m;
}

// cubic B-spline weights of the taps f - 1 .. f + 2 at the fraction x = cc - f
__host__ __device__ inline void rot_weights(real x, real* w) {
    const real y = real(1) - x;
    w[0] = y * y * y / real(6);
    w[1] = (x * x * (x - real(2)) * real(3) + real(4)) / real(6);
    w[2] = (y * y * (y - real(2)) * real(3) + real(4)) / real(6);
    w[3] = x * x * x / real(6);
}

// One output pixel from the coefficient image coef (H rows of `pitch` doubles).
__host__ __device__ inline real rot_sample(const real* coef, int pitch, int H, int W, real c, real s, int i, int j) {
    real cc0, cc1;
    rot_coords(H, W, c, s, i, j, &cc0, &cc1);
    // outside: below 0 or above the last sample on either axis (a NaN coordinate is outside too: nothing is indexed with it)
    if (!(cc0 >= real(0) && cc0 <= real(H - 1) && cc1 >= real(0) && cc1 <= real(W - 1))) return real(0);
    const real f0 = floor(cc0), f1 = floor(cc1);
    real w0[4], w1[4];
    rot_weights(cc0 - f0, w0);
    rot_weights(cc1 - f1, w1);
    int col[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) col[b] = rot_mirror((int)f1 - 1 + b, W);
    real t = real(0);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const real* row = coef + rot_mirror((int)f0 - 1 + a, H) * pitch;
#pragma unroll
        for (int b = 0; b < 4; ++b) t += row[col[b]] * w0[a] * w1[b];
    }
    return t;
}

__global__ void __launch_bounds__(SVGP_BLOCK) k_rotate_cubic(int H, int W, int A, const real* __restrict__ images,
                                                             const real* __restrict__ cos_sin, real* __restrict__ out) {
    extern __shared__ __align__(16) real rot_coef[];     // H x rot_pitch(W)
    const int t = threadIdx.x, P = rot_pitch(W), HW = H * W;
    const real* src = images + (size_t)blockIdx.x * HW;
    for (int p = t; p < HW; p += SVGP_BLOCK) rot_coef[(p / W) * P + p % W] = src[p];
    __syncthreads();
    if (t < W) rot_prefilter_line(rot_coef + t, H, P);           // axis 0: down the columns
    __syncthreads();
    if (t < H) rot_prefilter_line(rot_coef + t * P, W, 1);       // axis 1: along the rows
    __syncthreads();
    // thread t writes elements t, t + 256, ... of this image's (A, H, W) block; (a, p) follow the element without a division
    real* dst = out + (size_t)blockIdx.x * A * HW;
    int a = 0, p = t;
    while (p >= HW) { p -= HW; ++a; }
    for (size_t o = t; a < A; o += SVGP_BLOCK) {
        dst[o] = rot_sample(rot_coef, P, H, W, cos_sin[2 * a], cos_sin[2 * a + 1], p / W, p % W);
        p += SVGP_BLOCK;
        while (p >= HW) { p -= HW; ++a; }
    }
}

}  // namespace

extern "C" int svgp_rotate_cubic_f64(int n, int H, int W, int A, const double* images, const double* cos_sin, double* out,
                                     void* stream) {
    SVGP_REQUIRE(n >= 0 && A >= 1, SVGP_ERR_INVALID, "bad shape n=%d A=%d", n, A);
    SVGP_REQUIRE(H >= 2 && W >= 2 && H <= SVGP_ROT_MAX && W <= SVGP_ROT_MAX, SVGP_ERR_UNSUPPORTED,
                 "image of %d x %d: this build rotates 2 <= H, W <= %d", H, W, SVGP_ROT_MAX);
    if (n == 0) return SVGP_OK;
    SVGP_REQUIRE(images && cos_sin && out, SVGP_ERR_INVALID, "NULL device pointer");
    const size_t lds = (size_t)H * rot_pitch(W) * sizeof(real);
    hipLaunchKernelGGL(k_rotate_cubic, dim3(n), dim3(SVGP_BLOCK), lds, (hipStream_t)stream, H, W, A, images, cos_sin, out);
    SVGP_LAUNCH_CHECK();
    return SVGP_OK;
}
