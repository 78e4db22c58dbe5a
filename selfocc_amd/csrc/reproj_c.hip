// reproj_c.hip — the fused temporal reprojection term of reproj.hip on images of ANY channel count C (the `dims` knob of
// ReprojLossMonoMultiNewCombine / ReprojLossMonoMultiNew: feature-metric reprojection on (C, Hi, Wi) feature maps).
// Semantics: those of selfocc_reproj_fwd / _bwd with 3 replaced by C (include/selfocc_hip.h).  reproj.hip keeps the
// 3-channel planar kernel untouched; this unit is what runs when dims != 3.
//
// Layout: the warped images are CHANNEL-LAST, (Hi, Wi, img_stride) with img_stride % 4 == 0 and a 16-byte aligned base, so
// that one bilinear tap of four channels is ONE 16-byte load; a planar layout costs 8 x C scattered 4-byte loads per sample.
// Consecutive samples of a ray fall on neighbouring pixels of an epipolar line, so the rows a wave reads share cache lines.
//
// Hardware mapping: one wavefront per ray, lane l owns M = 1, 2, 4, 8 >= ceil(S / 64) consecutive samples — reproj_kernel's
// mapping, with project / eff_weight / wsum from the shared reproj_device.h, so the weight sums keep their order and
// `wnorm` / `any_valid` are bit for bit those of selfocc_reproj_fwd on the same geometry.
//   Phase 1  geometry, masks and weights; no image is read.  Kept per sample: the two clamped sampling coordinates per frame,
//            the two masks, the effective weight and its scale.
//   Phase 2  the channels in groups of four.  Per sample and frame four 16-byte taps; across groups only per-sample scalars
//            live on (the two partial |.| sums; in the backward also the dot product g_combine . comb_s).  `combine` leaves
//            per group after a wave reduction.  Nothing of width C is ever live: the register need does not depend on C.
// Channels C .. img_stride-1 of a pixel are padding: they are loaded with their group and dropped by a select before any
// arithmetic, so a NaN there reaches no output.  No atomics; every sum has a fixed order (results are run-to-run identical).
#include <cstdint>
#include "so_device.h"
#include "reproj_device.h"

namespace {

// sample_pixel (:140-152) + grid_sample's un-normalisation and border clip: pixel -> clamped source coordinate.
// The coordinate arithmetic of reproj.hip's sample_rgb, operation for operation.
SO_DEVFN float src_coord(float p, float img_size, int n) {
    float x = ((((p / img_size) * 2.0f - 1.0f) + 1.0f) / 2.0f) * (float)(n - 1);
    return fminf(fmaxf(x, 0.0f), (float)(n - 1));
}

// the four bilinear taps of channels c0 .. c0+3 at clamped (x, y) of a channel-last image -> out[4]
SO_DEVFN void sample4(const float *__restrict__ img, int Hi, int Wi, int stride, int c0, float x, float y, float out[4]) {
    const float fx = floorf(x), fy = floorf(y);
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = min(x0 + 1, Wi - 1), y1 = min(y0 + 1, Hi - 1);
    const bool x1in = (x0 + 1 <= Wi - 1), y1in = (y0 + 1 <= Hi - 1);
    const float wx1 = x - fx, wx0 = (fx + 1.0f) - x, wy1 = y - fy, wy0 = (fy + 1.0f) - y;
    const float nw = wx0 * wy0, ne = x1in ? wx1 * wy0 : 0.0f, sw = y1in ? wx0 * wy1 : 0.0f,
                se = (x1in && y1in) ? wx1 * wy1 : 0.0f;
    const float *p = img + c0;
    const float4 q00 = *reinterpret_cast<const float4 *>(p + ((size_t)y0 * Wi + x0) * stride);
    const float4 q01 = *reinterpret_cast<const float4 *>(p + ((size_t)y0 * Wi + x1) * stride);
    const float4 q10 = *reinterpret_cast<const float4 *>(p + ((size_t)y1 * Wi + x0) * stride);
    const float4 q11 = *reinterpret_cast<const float4 *>(p + ((size_t)y1 * Wi + x1) * stride);
    const float a00[4] = {q00.x, q00.y, q00.z, q00.w}, a01[4] = {q01.x, q01.y, q01.z, q01.w};
    const float a10[4] = {q10.x, q10.y, q10.z, q10.w}, a11[4] = {q11.x, q11.y, q11.z, q11.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float acc = a00[k] * nw;
        acc = acc + a01[k] * ne;
        acc = acc + a10[k] * sw;
        acc = acc + a11[k] * se;
        out[k] = acc;
    }
}

template <int M, bool BWD>
__global__ __launch_bounds__(256) void reproj_c_kernel(so_reproj_c_args a, const float *__restrict__ g_l1,
                                                       const float *__restrict__ g_comb, float *__restrict__ g_weights) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.R) return;
    const float u = a.pix[2 * (size_t)ray], v = a.pix[2 * (size_t)ray + 1];
    const float eps = 1.1920928955078125e-07f;

    // ---- phase 1: geometry, masks, weights ----------------------------------------------------------------------------
    float xp[M], yp[M], xn[M], yn[M], w[M], sc[M];
    bool mp[M], mn[M], live[M];
    float ws_l = 0.0f, valid_l = 0.0f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int i = lane * M + j;
        live[j] = i < a.S;
        const size_t o = (size_t)ray * a.S + (live[j] ? i : a.S - 1);
        const float t = a.ts[o];
        float px, py, qx, qy;
        project(a.T_prev, u, v, t, a.img_h, a.img_w, px, py, mp[j]);
        project(a.T_next, u, v, t, a.img_h, a.img_w, qx, qy, mn[j]);
        bool any = ((mp[j] ? 1.0f : 0.0f) + (mn[j] ? 1.0f : 0.0f)) > 0.0f;
        w[j] = eff_weight(a, o, any, sc[j]);
        if (!live[j]) { w[j] = 0.0f; sc[j] = 0.0f; any = false; }
        ws_l += w[j];
        valid_l += any ? 1.0f : 0.0f;
        xp[j] = src_coord(px, a.img_w, a.Wi); yp[j] = src_coord(py, a.img_h, a.Hi);
        xn[j] = src_coord(qx, a.img_w, a.Wi); yn[j] = src_coord(qy, a.img_h, a.Hi);
    }
    const float wtot_raw = wsum(ws_l);
    const float wtot = fmaxf(wtot_raw, eps);  // clamp_min(finfo.eps) (:182)
    const float inv_w = 1.0f / wtot;
    if constexpr (!BWD) {
        if (a.wnorm) {
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (live[j]) a.wnorm[(size_t)ray * a.S + lane * M + j] = w[j] * inv_w;
        }
    }

    // ---- phase 2: the channels, four at a time ------------------------------------------------------------------------
    const float *__restrict__ cur = a.curr + (size_t)ray * a.C;
    float ap[M], an[M], dot[M];        // per sample: sum_c |curr - warped| of each frame; g_combine . comb_s (backward)
#pragma unroll
    for (int j = 0; j < M; ++j) { ap[j] = 0.0f; an[j] = 0.0f; dot[j] = 0.0f; }
    for (int c0 = 0; c0 < a.C; c0 += 4) {
        bool on[4];
        float cu[4], gc[4], cl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            on[k] = c0 + k < a.C;
            cu[k] = on[k] ? cur[c0 + k] : 0.0f;
            gc[k] = 0.0f;
            cl[k] = 0.0f;
            if constexpr (BWD) {
                if (g_comb && on[k]) gc[k] = g_comb[(size_t)ray * a.C + c0 + k];
            }
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
            float rp[4], rn[4];
            sample4(a.img_prev, a.Hi, a.Wi, a.img_stride, c0, xp[j], yp[j], rp);
            sample4(a.img_next, a.Hi, a.Wi, a.img_stride, c0, xn[j], yn[j], rn);
            const float cnt = fmaxf((mp[j] ? 1.0f : 0.0f) + (mn[j] ? 1.0f : 0.0f), 1.0f);
            const float wn = w[j] * inv_w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float p = on[k] ? rp[k] : 0.0f, n = on[k] ? rn[k] : 0.0f;   // a pad channel is dropped here
                ap[j] = ap[j] + fabsf(cu[k] - p);
                an[j] = an[j] + fabsf(cu[k] - n);
                const float comb = ((mp[j] ? p : 0.0f) + (mn[j] ? n : 0.0f)) / cnt;
                if constexpr (BWD) dot[j] = dot[j] + gc[k] * comb;
                else cl[k] = fmaf(wn, comb, cl[k]);
            }
        }
        if constexpr (!BWD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = wsum(cl[k]);
                if (lane == 0 && on[k] && a.combine) a.combine[(size_t)ray * a.C + c0 + k] = s;
            }
        }
    }

    // ---- per-sample diff, then the per-ray sums: reproj_kernel's -------------------------------------------------------
    const float fc = (float)a.C;
    float diff[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        float dp = ap[j] / fc, dn = an[j] / fc;
        if (!mp[j]) dp = 0.0f;
        if (!mn[j]) dn = 0.0f;
        const float cnt = fmaxf((mp[j] ? 1.0f : 0.0f) + (mn[j] ? 1.0f : 0.0f), 1.0f);
        diff[j] = (dp + dn) / cnt;
    }
    if constexpr (!BWD) {
        float l1_l = 0.0f;
#pragma unroll
        for (int j = 0; j < M; ++j) l1_l = fmaf(w[j] * inv_w, diff[j], l1_l);
        const float l1 = wsum(l1_l);
        const float nvalid = wsum(valid_l);
        if (lane == 0) {
            if (a.l1) a.l1[ray] = l1;
            if (a.any_valid) a.any_valid[ray] = nvalid > 0.0f ? 1.0f : 0.0f;
        }
    } else {
        // L = sum_s wn_s a_s,  a_s = g_l1 diff_s + g_comb . comb_s,  wn = w / max(sum w, eps)
        const float gl = g_l1 ? g_l1[ray] : 0.0f;
        float as[M], abar_l = 0.0f;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            as[j] = fmaf(gl, diff[j], dot[j]);
            abar_l = fmaf(w[j] * inv_w, as[j], abar_l);
        }
        const float abar = (wtot_raw > eps) ? wsum(abar_l) : 0.0f;  // clamped denominator is a constant
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (!live[j]) continue;
            g_weights[(size_t)ray * a.S + lane * M + j] = sc[j] * (as[j] - abar) * inv_w;
        }
    }
}

// every refusal is decided here, on the host, before any HIP call
int validate(const so_reproj_c_args &a) {
    SO_REQUIRE(a.R >= 0, "reproj_c: need R >= 0");
    SO_REQUIRE(a.C >= 1 && a.C <= 512, "reproj_c: need 1 <= C <= 512 (C = %d)", (int)a.C);
    SO_REQUIRE(a.img_stride >= a.C && a.img_stride % 4 == 0,
               "reproj_c: img_stride must be a multiple of 4 and >= C (img_stride = %d, C = %d)", (int)a.img_stride, (int)a.C);
    SO_REQUIRE(a.S >= 1 && a.S <= 512, "reproj_c: need 1 <= S <= 512 (S = %d)", (int)a.S);
    if (a.R == 0) return 0;
    SO_REQUIRE(a.weights && a.ts && a.pix && a.curr && a.T_prev && a.T_next && a.img_prev && a.img_next,
               "reproj_c: NULL input pointer");
    SO_REQUIRE(((uintptr_t)a.img_prev & 15) == 0 && ((uintptr_t)a.img_next & 15) == 0,
               "reproj_c: img_prev / img_next must be 16-byte aligned");
    SO_REQUIRE(a.Hi >= 1 && a.Wi >= 1 && a.Hi <= (1 << 24) && a.Wi <= (1 << 24) && a.img_h > 0 && a.img_w > 0,
               "reproj_c: bad image size");
    return 0;
}

template <bool BWD>
int launch(const so_reproj_c_args &a, const float *g_l1, const float *g_comb, float *g_w, hipStream_t st) {
    const int m = (a.S + 63) / 64;              // the instance selfocc_reproj_fwd takes for this S: same lane ownership
    const int blocks = (a.R + 3) / 4;
#define SO_L(MM) hipLaunchKernelGGL((reproj_c_kernel<MM, BWD>), dim3(blocks), dim3(256), 0, st, a, g_l1, g_comb, g_w)
    if (m <= 1) SO_L(1);
    else if (m <= 2) SO_L(2);
    else if (m <= 4) SO_L(4);
    else SO_L(8);
#undef SO_L
    return so_launch_status();
}

}  // namespace

extern "C" int selfocc_reproj_c_fwd(const so_reproj_c_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    if (validate(*args)) return -1;
    if (args->R == 0) return 0;
    return launch<false>(*args, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int selfocc_reproj_c_bwd(const so_reproj_c_args *args, const float *g_l1, const float *g_combine,
                                    float *g_weights, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    if (validate(*args)) return -1;
    if (args->R == 0) return 0;
    SO_REQUIRE(g_weights != nullptr, "reproj_c_bwd: g_weights is NULL");
    return launch<true>(*args, g_l1, g_combine, g_weights, (hipStream_t)stream);
}
