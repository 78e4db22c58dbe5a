// losses.hip — the two volume regularisers of the SDF head as one launch per direction each (gfx950).
//
// (1) the eikonal regulariser
//
// Reference: loss/eikonal_loss.py:19-22 (EikonalLoss.eikonal_loss): mean over all ray samples of (||grad sdf||_2 - 1)^2 on the (R * S, 3)
// per-sample metre gradients of the render (7.4 M rows per nuscenes_occ iteration).  torch runs it as a norm REDUCTION over a
// dimension of three (67 us), sub, pow, mean forward and pow / norm backward (a copy, div, mul, masked_fill): ~0.26 ms per
// iteration for 88 MB of input.  Here: forward = one streaming pass writing one partial sum per block (the caller adds the
// partials: deterministic), backward = one streaming pass
//     d/dg = scale * 2 (||g|| - 1) g / ||g||      (0 where g = 0, as torch's norm backward),   scale read from device memory.
#include "so_device.h"
#include <algorithm>

namespace {

constexpr int kEikRowsPerThread = 4;
// Below this squared norm (2^-100: 24 bits above float32's smallest normal) x^2 + y^2 + z^2 is subnormal or zero, and the
// backward takes the row's direction from a rescaled copy: a row of magnitude 1e-25 has the gradient -2 scale g / ||g|| like
// every other short row (float64 says so), not the 0 that sqrtf(0) would give it.  Rows above it keep the plain formula's bits.
constexpr float kEikTinySq = 7.888609052210118e-31f;

__global__ __launch_bounds__(256) void eikonal_fwd_kernel(const float *__restrict__ g, float *__restrict__ partial, long long n) {
    __shared__ float red[4];
    float s = 0.0f;
    const long long stride = (long long)gridDim.x * 256;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        const float x = g[3 * r], y = g[3 * r + 1], z = g[3 * r + 2];
        const float d = sqrtf((x * x + y * y) + z * z) - 1.0f;
        s += d * d;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void eikonal_bwd_kernel(const float *__restrict__ g, const float *__restrict__ scale,
                                                          float *__restrict__ gg, long long n) {
    const float sc = 2.0f * scale[0];
    const long long stride = (long long)gridDim.x * 256;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        const float x = g[3 * r], y = g[3 * r + 1], z = g[3 * r + 2];
        const float ss = (x * x + y * y) + z * z;
        const float nn = sqrtf(ss);
        const float f = nn > 0.0f ? sc * (nn - 1.0f) / nn : 0.0f;
        float gx = f * x, gy = f * y, gz = f * z;
        if (ss < kEikTinySq) {                 // the squared norm lost bits or underflowed (|g| < 2^-50): the direction g / ||g|| from
            gx = gy = gz = 0.0f;               // the row scaled by a power of two (exact); only g = 0 has no direction
            const float m = fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z));
            if (m > 0.0f) {
                int e;
                (void)frexpf(m, &e);
                const float xs = ldexpf(x, -e), ys = ldexpf(y, -e), zs = ldexpf(z, -e);     // largest component in [0.5, 1)
                const float ns = sqrtf((xs * xs + ys * ys) + zs * zs);
                const float k = sc * (ldexpf(ns, e) - 1.0f);
                gx = k * (xs / ns); gy = k * (ys / ns); gz = k * (zs / ns);
            }
        }
        gg[3 * r] = gx; gg[3 * r + 1] = gy; gg[3 * r + 2] = gz;
    }
}

int so_eik_blocks(long long n) {
    return (int)std::max<long long>(1, std::min<long long>(2048, (n + 256LL * kEikRowsPerThread - 1) / (256LL * kEikRowsPerThread)));
}

// (2) Compact second differences of the SDF volume (H, W, D) along h, w, d (NeuSHead's `second_grad`, consumed by
// SecondGradLoss = mean |.|, loss/second_grad_loss.py:6-19): out = [ (s[2:] - 2 s[1:-1]) + s[:-2] ] for the three axes,
// flattened and concatenated, in the float order torch evaluates `s[2:] - 2 * s[1:-1] + s[:-2]`.  torch: 9 slices, 12
// elementwise kernels and a cat forward; 9 zero fills, 9 strided copies and 9 accumulations of the full volume backward.
// Backward here is the gather form (each voxel collects its <= 9 taps): no atomics, deterministic.
struct Sec2Args {
    const float *s;
    float *out;            // forward: (n0 + n1 + n2)
    const float *g_out;    // backward
    float *g_s;            // backward: (H, W, D)
    int H, W, D;
    long long n0, n1, n2;  // (H-2) W D, H (W-2) D, H W (D-2); 0 when the axis is shorter than 3
};

__global__ __launch_bounds__(256) void second_diff_fwd_kernel(Sec2Args a) {
    const long long tot = a.n0 + a.n1 + a.n2;
    const long long WD = (long long)a.W * a.D;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) {
        long long i, stride;
        if (e < a.n0) {                                   // (H-2, W, D): flat index = its position in s
            i = e; stride = WD;
        } else if (e < a.n0 + a.n1) {                     // (H, W-2, D)
            const long long r = e - a.n0, per = (long long)(a.W - 2) * a.D;
            const long long h = r / per, wd = r - h * per;
            i = h * WD + wd; stride = a.D;
        } else {                                          // (H, W, D-2)
            const long long r = e - a.n0 - a.n1, hw = r / (a.D - 2), d = r - hw * (a.D - 2);
            i = hw * a.D + d; stride = 1;
        }
        a.out[e] = (a.s[i + 2 * stride] - 2.0f * a.s[i + stride]) + a.s[i];
    }
}

__global__ __launch_bounds__(256) void second_diff_bwd_kernel(Sec2Args a) {
    const long long M = (long long)a.H * a.W * a.D, WD = (long long)a.W * a.D;
    for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
        const int h = (int)(m / WD);
        const long long wd = m - (long long)h * WD;
        const int w = (int)(wd / a.D), d = (int)(wd - (long long)w * a.D);
        float g = 0.0f;
        // axis tap t of output index q contributes coefficient (1, -2, 1)[t] to voxel q + t
        auto axis = [&](int x, int n, const float *go, long long base, long long step) {
            if (n < 3) return;
            if (x <= n - 3) g += go[base];                           // t = 0: q = x
            if (x >= 1 && x <= n - 2) g += -2.0f * go[base - step];  // t = 1: q = x - 1
            if (x >= 2) g += go[base - 2 * step];                    // t = 2: q = x - 2
        };
        axis(h, a.H, a.g_out, m, WD);
        axis(w, a.W, a.g_out + a.n0, (long long)h * (a.W - 2) * a.D + (long long)w * a.D + d, a.D);
        axis(d, a.D, a.g_out + a.n0 + a.n1, ((long long)h * a.W + w) * (a.D - 2) + d, 1);
        a.g_s[m] = g;
    }
}

int so_sec2_fill(Sec2Args &a, const float *s, int H, int W, int D) {
    SO_REQUIRE(H >= 1 && W >= 1 && D >= 1 && (long long)H * W * D < (1LL << 40), "second_diff: bad volume shape (%d, %d, %d)", H, W, D);
    a.s = s; a.H = H; a.W = W; a.D = D;
    a.n0 = H >= 3 ? (long long)(H - 2) * W * D : 0;
    a.n1 = W >= 3 ? (long long)H * (W - 2) * D : 0;
    a.n2 = D >= 3 ? (long long)H * W * (D - 2) : 0;
    return 0;
}

}  // namespace

extern "C" size_t selfocc_second_diff_size(int32_t H, int32_t W, int32_t D) {
    Sec2Args a;
    if (so_sec2_fill(a, nullptr, H, W, D)) return 0;
    return (size_t)(a.n0 + a.n1 + a.n2);
}

extern "C" int selfocc_second_diff_fwd(const float *sdf, float *out, int32_t H, int32_t W, int32_t D, void *stream) {
    Sec2Args a;
    if (int rc = so_sec2_fill(a, sdf, H, W, D)) return rc;
    const long long tot = a.n0 + a.n1 + a.n2;
    if (tot == 0) return 0;
    SO_REQUIRE(sdf && out, "second_diff_fwd: NULL pointer");
    a.out = out; a.g_out = nullptr; a.g_s = nullptr;
    hipLaunchKernelGGL(second_diff_fwd_kernel, dim3((unsigned)std::min<long long>(8192, (tot + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return so_launch_status();
}

extern "C" int selfocc_second_diff_bwd(const float *g_out, float *g_sdf, int32_t H, int32_t W, int32_t D, void *stream) {
    Sec2Args a;
    if (int rc = so_sec2_fill(a, nullptr, H, W, D)) return rc;
    SO_REQUIRE(g_out && g_sdf, "second_diff_bwd: NULL pointer");
    a.out = nullptr; a.g_out = g_out; a.g_s = g_sdf;
    const long long M = (long long)H * W * D;
    hipLaunchKernelGGL(second_diff_bwd_kernel, dim3((unsigned)std::min<long long>(8192, (M + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return so_launch_status();
}

extern "C" int selfocc_eikonal_partials(int64_t n) { return n <= 0 ? 0 : so_eik_blocks(n); }

extern "C" int selfocc_eikonal_fwd(const float *grad, float *partial, int64_t n, void *stream) {
    SO_REQUIRE(n >= 0, "eikonal_fwd: negative size");
    if (n == 0) return 0;
    SO_REQUIRE(grad && partial, "eikonal_fwd: NULL pointer");
    hipLaunchKernelGGL(eikonal_fwd_kernel, dim3((unsigned)so_eik_blocks(n)), dim3(256), 0, (hipStream_t)stream, grad, partial,
                       (long long)n);
    return so_launch_status();
}

extern "C" int selfocc_eikonal_bwd(const float *grad, const float *scale, float *g_grad, int64_t n, void *stream) {
    SO_REQUIRE(n >= 0, "eikonal_bwd: negative size");
    if (n == 0) return 0;
    SO_REQUIRE(grad && scale && g_grad, "eikonal_bwd: NULL pointer");
    hipLaunchKernelGGL(eikonal_bwd_kernel, dim3((unsigned)so_eik_blocks(n)), dim3(256), 0, (hipStream_t)stream, grad, scale, g_grad,
                       (long long)n);
    return so_launch_status();
}
