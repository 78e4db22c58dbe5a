// reproj_pick.hip — per ray and temporal frame, the sample that carries the most warped-photometric weight, and a
// per-sample value (the SDF) read there: the `sdf_loss` term of ReprojLossMonoMultiNew
// (loss/reproj_loss_mono_multi_new.py:265-270: argmax of prev_weight / next_weight, gather of sample_sdf).
//
// ONE launch per camera serves both frames.  The pick depends on geometry and weights only, so no image is read:
// per sample one load of weight / delta / t, two projections, and per ray 4 values written instead of the two (R, S)
// normalised-weight tensors an argmax in torch would need.
//
// Definition (tests/test_reproj_pick_gpu.py holds the kernel to it bit for bit).  For frame f, wn_i is the normalised
// weight selfocc_reproj_fwd writes to `wnorm` when the OTHER frame's transform maps behind the camera (what
// ReprojLossMonoMultiNew passes; for t > 0 such a frame is valid nowhere, so a sample is valid iff frame f sees it).
// The arithmetic is reproj_kernel's, through the shared reproj_device.h: the same project / eff_weight, the same lane
// ownership (lane l owns M consecutive samples, M = 1, 2, 4, 8 >= ceil(S / 64)), lane-local sum in sample order, the
// 32-to-1 butterfly, max(sum, eps) and one reciprocal.  Then, sequentially,
//     j = 0, best = wn_0;  for i = 1 .. S-1: if (wn_i > best) { best = wn_i; j = i; }
// i.e. the smallest index among equal maxima, 0 for a fully masked ray, and a NaN never wins (a NaN wn_0 keeps j = 0).
#include "so_device.h"
#include "reproj_device.h"

namespace {

constexpr int NONE = 0x7fffffff;

// wave arg-max of (value, index): the larger value, on equal values the smaller index.  No NaN ever enters `v`.
SO_DEVFN void wargmax(float &v, int &i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

template <int M>
__global__ __launch_bounds__(256) void reproj_pick_kernel(so_reproj_pick_args a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= a.R) return;
    const float u = a.pix[2 * (size_t)ray], v = a.pix[2 * (size_t)ray + 1];
    const float eps = 1.1920928955078125e-07f;

    float w[2][M];
    bool live[M];
    float ws_l[2] = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int i = lane * M + j;
        live[j] = i < a.S;
        const size_t o = (size_t)ray * a.S + (live[j] ? i : a.S - 1);
        const float t = a.ts[o];
        float px, py, sc;
        bool ok[2];
        project(a.T_prev, u, v, t, a.img_h, a.img_w, px, py, ok[0]);
        project(a.T_next, u, v, t, a.img_h, a.img_w, px, py, ok[1]);
        const float base = eff_weight(a, o, true, sc);     // w or w / delta; the mask below is eff_weight's own select
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            w[f][j] = (ok[f] && live[j]) ? base : 0.0f;
            ws_l[f] += w[f][j];
        }
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const float wtot = fmaxf(wsum(ws_l[f]), eps);
        const float inv_w = 1.0f / wtot;
        float best = -INFINITY, wn0 = 0.0f;
        int idx = NONE;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const float wn = w[f][j] * inv_w;
            if (j == 0) wn0 = wn;
            if (live[j] && wn > best) { best = wn; idx = lane * M + j; }
        }
        wargmax(best, idx);
        // nothing above -inf (every wn NaN or -inf), or a NaN in front that the sequential rule never replaces: sample 0
        const float first = __shfl(wn0, 0, 64);
        if (idx == NONE || first != first) idx = 0;
        if (lane == 0) {
            a.pick_index[2 * (size_t)ray + f] = idx;
            a.pick_value[2 * (size_t)ray + f] = a.values[(size_t)ray * a.S + idx];
        }
    }
}

// dense d / d values: the ray's row is zero except g[r][f] at pick_index[r][f]; summed where both frames picked one sample
__global__ __launch_bounds__(256) void reproj_pick_bwd_kernel(const int32_t *__restrict__ pick_index,
                                                              const float *__restrict__ g_pick, float *__restrict__ g_values,
                                                              int R, int S) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + wave;
    if (ray >= R) return;
    const int j0 = pick_index[2 * (size_t)ray], j1 = pick_index[2 * (size_t)ray + 1];
    const float g0 = g_pick[2 * (size_t)ray], g1 = g_pick[2 * (size_t)ray + 1];
    for (int i = lane; i < S; i += 64) {
        float g = 0.0f;
        if (i == j0) g += g0;
        if (i == j1) g += g1;
        g_values[(size_t)ray * S + i] = g;
    }
}

}  // namespace

extern "C" int selfocc_reproj_pick_fwd(const so_reproj_pick_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_reproj_pick_args &a = *args;
    SO_REQUIRE(a.R >= 0 && a.S >= 1 && a.S <= 512, "reproj_pick: need R >= 0, 1 <= S <= 512");
    SO_REQUIRE(a.weights && a.ts && a.values && a.pix && a.T_prev && a.T_next, "reproj_pick: NULL input pointer");
    SO_REQUIRE(a.pick_index && a.pick_value, "reproj_pick: NULL output pointer");
    SO_REQUIRE(a.img_h > 0 && a.img_w > 0, "reproj_pick: bad image size");
    if (a.R == 0) return 0;
    const int blocks = (a.R + 3) / 4;
    so_with_samples_per_lane(a.S, [&](auto MM) {    // the instance selfocc_reproj_fwd takes for this S: same lane ownership
        hipLaunchKernelGGL((reproj_pick_kernel<decltype(MM)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    });
    return so_launch_status();
}

extern "C" int selfocc_reproj_pick_bwd(const int32_t *pick_index, const float *g_pick_value, float *g_values, int32_t R,
                                       int32_t S, void *stream) {
    SO_REQUIRE(R >= 0 && S >= 1 && S <= 512, "reproj_pick_bwd: need R >= 0, 1 <= S <= 512");
    SO_REQUIRE(pick_index && g_pick_value && g_values, "reproj_pick_bwd: NULL pointer");
    if (R == 0) return 0;
    hipLaunchKernelGGL(reproj_pick_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, pick_index,
                       g_pick_value, g_values, (int)R, (int)S);
    return so_launch_status();
}
