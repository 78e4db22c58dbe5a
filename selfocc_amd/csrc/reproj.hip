// reproj.hip — fused temporal reprojection photometric term for gfx950 (MI355X): ONE kernel behind both pairs of entries,
// selfocc_reproj_fwd / _bwd (planar 3-channel images) and selfocc_reproj_c_fwd / _bwd (channel-last images of any channel
// count C: the `dims` knob of ReprojLossMonoMultiNewCombine / ReprojLossMonoMultiNew, feature-metric reprojection).
//
// Replaces, per camera, the per-SAMPLE part of ReprojLossMonoMultiNewCombine.reproj_loss
// (loss/reproj_loss_mono_multi_new_combine.py:108-201), which the reference runs as ~40
// elementwise / index kernels over R*S = 1.2 M samples per camera:
//   (u t, v t, t, 1) -> img2prevImg / img2nextImg -> perspective divide (eps 1e-5) -> in-image
//   mask (:118-133) -> F.grid_sample(prev / next image, bilinear, border, align_corners=True)
//   (:140-152) -> L1 vs the current colour, masked mean over the two frames (:166-176) ->
//   weights masked + renormalised per ray (index_add_/gather, :178-184) -> per-ray weighted L1
//   (:186-187) and weighted composite colour (:190-201) -> "no valid sample" ray filter (:223-225).
// SSIM, the auto-mask minimum and the mean stay in torch on the tiny (R, C) lattice images.
//
// Image forms.  The form is a template argument and shows in ONE place, the tap fetch (sample4); nothing else branches on it.
//   planar        (3, Hi, Wi), any base alignment: C is the compile-time 3, a tap of a channel group is 3 scalar loads and
//                 the group's fourth slot is off at compile time.
//   channel-last  (Hi, Wi, img_stride) with img_stride % 4 == 0 and a 16-byte aligned base, C and img_stride from the
//                 arguments: one bilinear tap of four channels is ONE 16-byte load (a planar layout would cost 8 x C scattered
//                 4-byte loads per sample).  Channels C .. img_stride-1 of a pixel are padding: they are loaded with their
//                 group and dropped by a select before any arithmetic, so a NaN there reaches no output.
//
// Hardware mapping: one wavefront per ray, lane l owns M = 1, 2, 4, 8 >= ceil(S / 64) consecutive samples (consecutive
// samples of a ray project onto neighbouring pixels of an epipolar line, so the taps of a wave land in a few cache lines);
// the per-ray sums are wavefront-shuffle reductions; weights / ts are read as contiguous runs.  project / eff_weight / wsum
// come from reproj_device.h, which reproj_pick.hip shares.
//   Phase 1  geometry, masks and weights; no image is read.  Kept per sample: the two clamped sampling coordinates per frame,
//            the two masks, the effective weight and its scale.
//   Phase 2  the channels in groups of four.  Per sample and frame four taps; across groups only per-sample scalars live on
//            (the two partial |.| sums; in the backward also the dot product g_combine . comb_s).  `combine` leaves per group
//            after a wave reduction.  Nothing of width C is ever live: the register need does not depend on C.
// Nothing per-sample is written in the forward pass; backward recomputes the taps.  No atomics; every sum has a fixed order
// (results are run-to-run identical), and that order is the same in both forms: at C = 3 the two pairs of entries agree in
// every output bit of the forward and in every gradient value.  (A planar kernel of its own once summed g_combine . comb_s
// without the leading +0 of `dot`: against it, only the sign of an exactly zero gradient can differ.)
#include <cstdint>
#include "so_device.h"
#include "reproj_device.h"

namespace {

// sample_pixel (:140-152) + grid_sample's un-normalisation and border clip: pixel -> clamped source coordinate
SO_DEVFN float src_coord(float p, float img_size, int n) {
    // pixel / img_size * 2 - 1, then un-normalise ((c + 1) / 2) * (size - 1)
    float x = ((((p / img_size) * 2.0f - 1.0f) + 1.0f) / 2.0f) * (float)(n - 1);
    return fminf(fmaxf(x, 0.0f), (float)(n - 1));  // border: clip coordinates
}

// F.grid_sample(bilinear, padding_mode='border', align_corners=True) at clamped (x, y): channels c0 .. c0+3 -> out[4].
// PLANAR: c0 == 0, the image is (3, Hi, Wi) and out[3] = 0 (a slot the caller has switched off).
template <bool PLANAR>
SO_DEVFN void sample4(const float *__restrict__ img, int Hi, int Wi, int stride, int c0, float x, float y, float out[4]) {
    const float fx = floorf(x), fy = floorf(y);
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = min(x0 + 1, Wi - 1), y1 = min(y0 + 1, Hi - 1);
    const bool x1in = (x0 + 1 <= Wi - 1), y1in = (y0 + 1 <= Hi - 1);
    const float wx1 = x - fx, wx0 = (fx + 1.0f) - x, wy1 = y - fy, wy0 = (fy + 1.0f) - y;
    const float nw = wx0 * wy0, ne = x1in ? wx1 * wy0 : 0.0f, sw = y1in ? wx0 * wy1 : 0.0f,
                se = (x1in && y1in) ? wx1 * wy1 : 0.0f;
    const size_t o00 = (size_t)y0 * Wi + x0, o01 = (size_t)y0 * Wi + x1, o10 = (size_t)y1 * Wi + x0, o11 = (size_t)y1 * Wi + x1;
    float a00[4], a01[4], a10[4], a11[4];
    if constexpr (PLANAR) {
        const size_t plane = (size_t)Hi * Wi;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float *p = img + k * plane;
            a00[k] = p[o00]; a01[k] = p[o01]; a10[k] = p[o10]; a11[k] = p[o11];
        }
        a00[3] = a01[3] = a10[3] = a11[3] = 0.0f;
    } else {
        const float *p = img + c0;
        const float4 q00 = *reinterpret_cast<const float4 *>(p + o00 * stride);
        const float4 q01 = *reinterpret_cast<const float4 *>(p + o01 * stride);
        const float4 q10 = *reinterpret_cast<const float4 *>(p + o10 * stride);
        const float4 q11 = *reinterpret_cast<const float4 *>(p + o11 * stride);
        a00[0] = q00.x; a00[1] = q00.y; a00[2] = q00.z; a00[3] = q00.w;
        a01[0] = q01.x; a01[1] = q01.y; a01[2] = q01.z; a01[3] = q01.w;
        a10[0] = q10.x; a10[1] = q10.y; a10[2] = q10.z; a10[3] = q10.w;
        a11[0] = q11.x; a11[1] = q11.y; a11[2] = q11.z; a11[3] = q11.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float acc = a00[k] * nw;
        acc = acc + a01[k] * ne;
        acc = acc + a10[k] * sw;
        acc = acc + a11[k] * se;
        out[k] = acc;
    }
}

template <int M, bool BWD, bool PLANAR>
__global__ __launch_bounds__(256) void reproj_kernel(so_reproj_c_args a, const float *__restrict__ g_l1,
                                                     const float *__restrict__ g_comb, float *__restrict__ g_weights) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.R) return;
    const int C = PLANAR ? 3 : a.C;
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
        bool any = ((mp[j] ? 1.0f : 0.0f) + (mn[j] ? 1.0f : 0.0f)) > 0.0f;   // general_mask: at least one frame valid
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
    const float *__restrict__ cur = a.curr + (size_t)ray * C;
    float ap[M], an[M], dot[M];        // per sample: sum_c |curr - warped| of each frame; g_combine . comb_s (backward)
#pragma unroll
    for (int j = 0; j < M; ++j) { ap[j] = 0.0f; an[j] = 0.0f; dot[j] = 0.0f; }
    for (int c0 = 0; c0 < C; c0 += 4) {
        bool on[4];
        float cu[4], gc[4], cl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            on[k] = c0 + k < C;
            cu[k] = on[k] ? cur[c0 + k] : 0.0f;
            gc[k] = 0.0f;
            cl[k] = 0.0f;
            if constexpr (BWD) {
                if (g_comb && on[k]) gc[k] = g_comb[(size_t)ray * C + c0 + k];
            }
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
            float rp[4], rn[4];
            sample4<PLANAR>(a.img_prev, a.Hi, a.Wi, a.img_stride, c0, xp[j], yp[j], rp);
            sample4<PLANAR>(a.img_next, a.Hi, a.Wi, a.img_stride, c0, xn[j], yn[j], rn);
            const float cnt = fmaxf((mp[j] ? 1.0f : 0.0f) + (mn[j] ? 1.0f : 0.0f), 1.0f);
            const float wn = w[j] * inv_w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float p = on[k] ? rp[k] : 0.0f, n = on[k] ? rn[k] : 0.0f;   // a pad channel is dropped here
                ap[j] = ap[j] + fabsf(cu[k] - p);      // in channel order from +0: ((|c0-r0| + |c1-r1|) + |c2-r2|) at C = 3;
                an[j] = an[j] + fabsf(cu[k] - n);      // a slot that is off adds an exact +0
                const float comb = ((mp[j] ? p : 0.0f) + (mn[j] ? n : 0.0f)) / cnt;
                if constexpr (BWD) dot[j] = dot[j] + gc[k] * comb;
                else cl[k] = fmaf(wn, comb, cl[k]);
            }
        }
        if constexpr (!BWD) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = wsum(cl[k]);
                if (lane == 0 && on[k] && a.combine) a.combine[(size_t)ray * C + c0 + k] = s;
            }
        }
    }

    // ---- per-sample diff (masked mean |curr - warped| over the valid frames), then the per-ray sums --------------------
    const float fc = (float)C;
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

// selfocc_reproj_fwd / _bwd's struct as the kernel's argument: C = 3; img_stride is not read by the planar form
so_reproj_c_args from_planar(const so_reproj_args &p) {
    so_reproj_c_args a = {};
    a.weights = p.weights; a.ts = p.ts; a.deltas = p.deltas;
    a.pix = p.pix; a.curr = p.curr_rgb;
    a.T_prev = p.T_prev; a.T_next = p.T_next;
    a.img_prev = p.img_prev; a.img_next = p.img_next;
    a.R = p.R; a.S = p.S; a.Hi = p.Hi; a.Wi = p.Wi; a.C = 3; a.img_stride = 4;
    a.img_h = p.img_h; a.img_w = p.img_w;
    a.l1 = p.l1; a.combine = p.rgb_combine; a.any_valid = p.any_valid; a.wnorm = p.wnorm;
    return a;
}

// Every refusal of either pair of entries is decided here, on the host, before any HIP call; then the launch.  The planar
// form takes an image base of any alignment (its taps are scalar loads).
template <bool BWD>
int run(const so_reproj_c_args &a, bool planar, const float *g_l1, const float *g_comb, float *g_w, void *stream) {
    const char *who = planar ? "reproj" : "reproj_c";
    SO_REQUIRE(a.R >= 0, "%s: need R >= 0", who);
    SO_REQUIRE(a.C >= 1 && a.C <= 512, "%s: need 1 <= C <= 512 (C = %d)", who, (int)a.C);
    SO_REQUIRE(a.img_stride >= a.C && a.img_stride % 4 == 0,
               "%s: img_stride must be a multiple of 4 and >= C (img_stride = %d, C = %d)", who, (int)a.img_stride, (int)a.C);
    SO_REQUIRE(a.S >= 1 && a.S <= 512, "%s: need 1 <= S <= 512 (S = %d)", who, (int)a.S);
    if (a.R == 0) return 0;
    SO_REQUIRE(a.weights && a.ts && a.pix && a.curr && a.T_prev && a.T_next && a.img_prev && a.img_next,
               "%s: NULL input pointer", who);
    SO_REQUIRE(planar || ((((uintptr_t)a.img_prev | (uintptr_t)a.img_next) & 15) == 0),
               "%s: img_prev / img_next must be 16-byte aligned", who);
    SO_REQUIRE(a.Hi >= 1 && a.Wi >= 1 && a.Hi <= (1 << 24) && a.Wi <= (1 << 24) && a.img_h > 0 && a.img_w > 0,
               "%s: bad image size", who);
    SO_REQUIRE(!BWD || g_w != nullptr, "%s_bwd: g_weights is NULL", who);
    const int blocks = (a.R + 3) / 4;
    so_with_const<bool, true, false>(planar, [&](auto PL) {
        so_with_samples_per_lane(a.S, [&](auto MM) {
            hipLaunchKernelGGL((reproj_kernel<decltype(MM)::value, BWD, decltype(PL)::value>), dim3(blocks), dim3(256), 0,
                               (hipStream_t)stream, a, g_l1, g_comb, g_w);
        });
    });
    return so_launch_status();
}

}  // namespace

extern "C" int selfocc_reproj_fwd(const so_reproj_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    return run<false>(from_planar(*args), true, nullptr, nullptr, nullptr, stream);
}

extern "C" int selfocc_reproj_bwd(const so_reproj_args *args, const float *g_l1, const float *g_rgb_combine,
                                  float *g_weights, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    return run<true>(from_planar(*args), true, g_l1, g_rgb_combine, g_weights, stream);
}

extern "C" int selfocc_reproj_c_fwd(const so_reproj_c_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    return run<false>(*args, false, nullptr, nullptr, nullptr, stream);
}

extern "C" int selfocc_reproj_c_bwd(const so_reproj_c_args *args, const float *g_l1, const float *g_combine,
                                    float *g_weights, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    return run<true>(*args, false, g_l1, g_combine, g_weights, stream);
}
