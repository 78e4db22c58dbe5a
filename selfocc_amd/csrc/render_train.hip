// render_train.hip — sample-parallel SDF ray march for the TRAINING API of selfocc_render_fwd
// (per-sample outputs weights / ts / deltas / sdf / grad requested: NeuSHead.forward,
// model/head/neus_head/neus_head.py:531-577, 640).
//
// The per-ray march of render_fwd.hip gives one ray to a lane.  That is the right shape for
// evaluation (2.16 M rays), and the wrong one for training: the shipped configs train on 48 x 100
// rays x 6 cameras = 28 800 rays x 256 samples — 450 wavefronts on a chip with 8 192 wave slots, each
// walking 256 dependent steps and writing its per-sample tensors with a stride of S floats between
// lanes (2.35 ms per iteration in the round-1 profile, almost all of it latency).
//
// Here a LANE OWNS A SAMPLE: the 64 lanes of a wave are 64 consecutive samples of one ray, the
// 1 / 2 / 4 waves of a ray group cover up to 256 samples per pass.
//   * everything per sample (bin edges incl. jitter, position, meter -> grid, trilinear value +
//     gradient, NeuS alpha, colour / semantic lookup) is the CANONICAL arithmetic of so_device.h,
//     independent of the other samples: sdf / grad / ts / deltas are bit-identical to the oracle;
//   * the transmittance T_i = prod_{j<i} (1 - alpha_j + 1e-7) is an exclusive prefix product:
//     a 6-step wave scan, the wave totals of a ray combined through LDS, a running carry across
//     passes when S > 64 * waves-per-ray.  (A scan multiplies in a different order than the
//     reference's cumprod: weights agree to ~1e-7 relative, not bit for bit.)
//   * per-ray outputs (depth, acc, rgb, sem, max-depth) are wave reductions of the per-sample terms;
//   * every per-sample store is a coalesced 256-byte row segment.
#include "so_device.h"
#include "sh_device.h"
#include "ray_device.h"

namespace {

// so_gather_feat (render_fwd.hip) with four scalar fmaf per 16 bytes where that one issues two packed FMAs: merging the two changes 27 training kernels
template <int NF, bool BF16>
SO_DEVFN void so_train_feat(const void *__restrict__ vol, int H, int W, int D, const so_cell &c, const float wk[8],
                            float f[NF > 0 ? NF : 1]) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const int h = c.h0 + (kk >> 2), w = c.w0 + ((kk >> 1) & 1), d = c.d0 + (kk & 1);
        const bool in = (h >= 0) && (h < H) && (w >= 0) && (w < W) && (d >= 0) && (d < D);
        const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1), dc = min(max(d, 0), D - 1);
        const size_t vox = ((size_t)hc * W + wc) * D + dc;
        const float wgt = in ? wk[kk] : 0.0f;
        if constexpr (!BF16) {
            const float4 *p = (const float4 *)((const float *)vol + vox * NF);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const float4 t = p[q];
                f[4 * q + 0] = fmaf(t.x, wgt, f[4 * q + 0]);
                f[4 * q + 1] = fmaf(t.y, wgt, f[4 * q + 1]);
                f[4 * q + 2] = fmaf(t.z, wgt, f[4 * q + 2]);
                f[4 * q + 3] = fmaf(t.w, wgt, f[4 * q + 3]);
            }
        } else {
            const uint2 *p = (const uint2 *)((const uint16_t *)vol + vox * NF);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const uint2 t = p[q];
                f[4 * q + 0] = fmaf(__uint_as_float(t.x << 16), wgt, f[4 * q + 0]);
                f[4 * q + 1] = fmaf(__uint_as_float(t.x & 0xffff0000u), wgt, f[4 * q + 1]);
                f[4 * q + 2] = fmaf(__uint_as_float(t.y << 16), wgt, f[4 * q + 2]);
                f[4 * q + 3] = fmaf(__uint_as_float(t.y & 0xffff0000u), wgt, f[4 * q + 3]);
            }
        }
    }
}

// WPR = waves per ray (1, 2 or 4); a 256-thread block serves 4 / WPR rays.  MK = mapping kind (so_locate_k).
// The body is render_train_body.h.  NB > 0 (render_sh_samples_kernel): spherical-harmonics colour with NB basis functions
// (sh_device.h), NF = the row stride of the coefficients; the fold of so_sh_gather replaces so_train_feat and everything that
// is not colour is the same code.
template <int NF, bool BF16, int WPR, int MK = SO_MAP_LINEAR>
__global__ __launch_bounds__(256) void render_fwd_samples_kernel(so_render_args a) {
    constexpr int NB = NF < 0 ? 1 : 0;   // no spherical harmonics (spelled value-dependent: the NB > 0 branches are never instantiated)
    constexpr bool MASKED = false;
#include "render_train_body.h"
}
template <int NB, int WPR, int MK>
__global__ __launch_bounds__(256) void render_sh_samples_kernel(so_render_args a) {
    constexpr int NF = so_sh_stride(NB);
    constexpr bool BF16 = false;
    constexpr bool MASKED = false;
#include "render_train_body.h"
}
// any class count from 2 to 21: float32 rows of NF = 8, 12, 16, 20, 24 floats that hold a.n_sem in [NF - 6, NF - 3]
// logits and up to three pad channels, which SO_SEM_ON keeps out of the soft-max
template <int NF, int WPR, int MK>
__global__ __launch_bounds__(256) void render_ns_samples_kernel(so_render_args a) {
    constexpr int NB = NF < 0 ? 1 : 0;
    constexpr bool BF16 = false;
    constexpr bool MASKED = true;
#include "render_train_body.h"
}
template <int NF, int WPR, int MK>
int launch_ns_samples_w(const so_render_args &a, hipStream_t st) {
    constexpr int RPB = 4 / WPR;
    hipLaunchKernelGGL((render_ns_samples_kernel<NF, WPR, MK>), dim3((a.n_rays + RPB - 1) / RPB), dim3(256), 0, st, a);
    return so_launch_status();
}
template <int NF, int MK>
int launch_ns_samples(const so_render_args &a, hipStream_t st) {
    if (a.n_samples <= 64) return launch_ns_samples_w<NF, 1, MK>(a, st);
    if (a.n_samples <= 128) return launch_ns_samples_w<NF, 2, MK>(a, st);
    return launch_ns_samples_w<NF, 4, MK>(a, st);
}

template <int NB, int WPR, int MK>
int launch_sh_samples_w(const so_render_args &a, hipStream_t st) {
    constexpr int RPB = 4 / WPR;
    hipLaunchKernelGGL((render_sh_samples_kernel<NB, WPR, MK>), dim3((a.n_rays + RPB - 1) / RPB), dim3(256), 0, st, a);
    return so_launch_status();
}
template <int NB, int MK>
int launch_sh_samples(const so_render_args &a, hipStream_t st) {
    if (a.n_samples <= 64) return launch_sh_samples_w<NB, 1, MK>(a, st);
    if (a.n_samples <= 128) return launch_sh_samples_w<NB, 2, MK>(a, st);
    return launch_sh_samples_w<NB, 4, MK>(a, st);
}

template <int NF, bool BF16, int WPR, int MK = SO_MAP_LINEAR>
int launch_samples_w(const so_render_args &a, hipStream_t st) {
    constexpr int RPB = 4 / WPR;
    hipLaunchKernelGGL((render_fwd_samples_kernel<NF, BF16, WPR, MK>), dim3((a.n_rays + RPB - 1) / RPB), dim3(256), 0, st, a);
    return so_launch_status();
}

}  // namespace

// called by selfocc_render_fwd (render_fwd.hip) for launches that request per-sample outputs
template <int NF, bool BF16>
int so_render_fwd_samples(const so_render_args &a, hipStream_t st) {
    if (a.map.kind == SO_MAP_UPSCALE) {
        if constexpr (NF == 24 && BF16) {
            SO_REQUIRE(false, "the 'linear_upscale' mapping is built for n_rgb + n_sem = 0, 3, 8 and float32 24 (got bfloat16 24)");
        } else {
            if (a.n_samples <= 64) return launch_samples_w<NF, BF16, 1, SO_MAP_UPSCALE>(a, st);
            if (a.n_samples <= 128) return launch_samples_w<NF, BF16, 2, SO_MAP_UPSCALE>(a, st);
            return launch_samples_w<NF, BF16, 4, SO_MAP_UPSCALE>(a, st);
        }
    }
    if (a.n_samples <= 64) return launch_samples_w<NF, BF16, 1>(a, st);
    if (a.n_samples <= 128) return launch_samples_w<NF, BF16, 2>(a, st);
    return launch_samples_w<NF, BF16, 4>(a, st);
}

template int so_render_fwd_samples<0, false>(const so_render_args &, hipStream_t);
template int so_render_fwd_samples<4, false>(const so_render_args &, hipStream_t);
template int so_render_fwd_samples<4, true>(const so_render_args &, hipStream_t);
template int so_render_fwd_samples<8, false>(const so_render_args &, hipStream_t);
template int so_render_fwd_samples<24, false>(const so_render_args &, hipStream_t);
template int so_render_fwd_samples<24, true>(const so_render_args &, hipStream_t);

// the spherical-harmonics launches of the training API (called by selfocc_render_fwd)
template <int NB>
int so_render_sh_samples(const so_render_args &a, hipStream_t st) {
    return a.map.kind == SO_MAP_UPSCALE ? launch_sh_samples<NB, SO_MAP_UPSCALE>(a, st) : launch_sh_samples<NB, SO_MAP_LINEAR>(a, st);
}
template int so_render_sh_samples<1>(const so_render_args &, hipStream_t);
template int so_render_sh_samples<4>(const so_render_args &, hipStream_t);
template int so_render_sh_samples<9>(const so_render_args &, hipStream_t);

// the masked launches of the training API (called by selfocc_render_fwd)
template <int NF>
int so_render_ns_samples(const so_render_args &a, hipStream_t st) {
    return a.map.kind == SO_MAP_UPSCALE ? launch_ns_samples<NF, SO_MAP_UPSCALE>(a, st) : launch_ns_samples<NF, SO_MAP_LINEAR>(a, st);
}
template int so_render_ns_samples<8>(const so_render_args &, hipStream_t);
template int so_render_ns_samples<12>(const so_render_args &, hipStream_t);
template int so_render_ns_samples<16>(const so_render_args &, hipStream_t);
template int so_render_ns_samples<20>(const so_render_args &, hipStream_t);
template int so_render_ns_samples<24>(const so_render_args &, hipStream_t);
