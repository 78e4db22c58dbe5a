// reproj_device.h — what the sampling kernel (reproj.hip: both image forms, all four entries) and reproj_pick.hip share: the
// per-sample geometry and weight arithmetic and the samples-per-lane ladder.  ONE definition, so that the pick kernel's
// normalised weights are, bit for bit, the ones selfocc_reproj_fwd / selfocc_reproj_c_fwd write to `wnorm`.
// Line numbers refer to the reference's loss/reproj_loss_mono_multi_new_combine.py.
#pragma once
#include "so_device.h"

// Host: the samples-per-lane instance of S (1 <= S <= 512) as a compile-time constant, f(so_int<M>) with M the smallest of
// 1, 2, 4, 8 that has 64 M >= S.  Lane l of a ray's wave owns samples l M .. l M + M - 1 in every kernel launched through it.
template <class F>
static inline void so_with_samples_per_lane(int S, F &&f) {
    const int m = (S + 63) / 64;
    so_with_const<int, 1, 2, 4, 8>(m <= 2 ? m : m <= 4 ? 4 : 8, f);
}

namespace {

SO_DEVFN void project(const float *__restrict__ T, float u, float v, float t, float img_h, float img_w,
                      float &px, float &py, bool &ok) {
    // cal_pixel (:118-133): trans @ (u t, v t, t, 1)
    const float x = u * t, y = v * t;
    const float p0 = ((T[0] * x + T[1] * y) + T[2] * t) + T[3];
    const float p1 = ((T[4] * x + T[5] * y) + T[6] * t) + T[7];
    const float p2 = ((T[8] * x + T[9] * y) + T[10] * t) + T[11];
    const float den = fmaxf(1e-5f, p2);
    px = p0 / den;
    py = p1 / den;
    ok = (p2 > 0.0f) && (px > 0.0f) && (px < img_w) && (py > 0.0f) && (py < img_h);
}

SO_DEVFN float wsum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// effective weight of a sample: optional w / delta (:111-116), then general-mask zeroing (:178-179)
template <class Args>
SO_DEVFN float eff_weight(const Args &a, size_t o, bool any, float &scale) {
    float w = a.weights[o];
    scale = 1.0f;
    if (a.deltas) {
        const float eps = 1.1920928955078125e-07f;
        const float d = a.deltas[o];
        scale = (d < eps) ? 0.0f : 1.0f / fmaxf(d, eps);
        w = (d < eps) ? 0.0f : w / fmaxf(d, eps);
    }
    if (!any) { w = 0.0f; scale = 0.0f; }
    return w;
}

}  // namespace
