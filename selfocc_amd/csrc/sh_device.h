// sh_device.h — spherical-harmonics colour of the render kernels (so_render_args::sh_deg / sh_act), degrees 0 - 2.
//
// Contract: include/selfocc_hip.h above so_render_args (reference: model/head/utils/sh_render.py:35-94).
//   raw_c = sum_k Y_k(dir) * f[c * NB + k],   NB = (sh_deg + 1)^2 basis functions, coefficients colour-major;
//   rgb_c = relu(raw_c + 0.5)  or  sigmoid(raw_c).
// The reduction over k is linear, so it is folded into the trilinear gather: per corner the NB * 3 coefficients stream
// through registers 16 bytes at a time and go straight into THREE sums weighted by (trilinear weight x Y_k).  Nothing of
// width 3 * NB stays live: a 28-channel gather with the accumulators of the 4-channel one.
// Canonical order (-ffp-contract=off): every rounding below is spelled out; the host mirror is selfocc_amd/sh.py.
#pragma once
#include "so_device.h"

// NB (1, 4, 9) of a validated launch; feature row stride of NB basis functions (3 * NB rounded up to 4 floats)
__host__ __device__ constexpr int so_sh_stride(int NB) { return (3 * NB + 3) & ~3; }

// a launch with colour that is not "degree 0 with relu": it runs the kernels of this header's users
static inline bool so_sh_launch(const so_render_args &a) { return a.n_rgb == 3 && (a.sh_deg != 0 || a.sh_act != SO_SH_RELU); }

template <int NB>
SO_DEVFN void so_sh_basis(float x, float y, float z, float Y[NB]) {
    static_assert(NB == 1 || NB == 4 || NB == 9, "SH degrees 0 - 2");
    Y[0] = 0.28209479177387814f;
    if constexpr (NB >= 4) {
        Y[1] = -0.4886025119029199f * y;
        Y[2] = 0.4886025119029199f * z;
        Y[3] = -0.4886025119029199f * x;
    }
    if constexpr (NB >= 9) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = 1.0925484305920792f * (x * y);
        Y[5] = -1.0925484305920792f * (y * z);
        Y[6] = 0.31539156525252005f * ((2.0f * zz - xx) - yy);
        Y[7] = -1.0925484305920792f * (x * z);
        Y[8] = 0.5462742152960396f * (xx - yy);
    }
}

// activation and its derivative with respect to raw
SO_DEVFN float so_sh_act(float raw, int act) {
    return act == SO_SH_SIGMOID ? so_sigmoid(raw) : fmaxf(raw + 0.5f, 0.0f);
}
SO_DEVFN float so_sh_dact(float raw, int act) {
    if (act == SO_SH_SIGMOID) {
        const float s = so_sigmoid(raw);
        return s * (1.0f - s);
    }
    return (raw + 0.5f > 0.0f) ? 1.0f : 0.0f;
}

// raw[c] = sum over the 8 corners (zero padding outside the volume) and the NB basis functions of
// (wk[corner] * Y[k]) * vol[corner][c * NB + k]; float32 volume with rows of so_sh_stride(NB) floats
template <int NB>
SO_DEVFN void so_sh_gather(const void *__restrict__ vol, int H, int W, int D, const so_cell &c, const float wk[8],
                           const float Y[NB], float raw[3]) {
    constexpr int ST = so_sh_stride(NB);
    raw[0] = 0.0f; raw[1] = 0.0f; raw[2] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const int h = c.h0 + (kk >> 2), w = c.w0 + ((kk >> 1) & 1), d = c.d0 + (kk & 1);
        const bool in = (h >= 0) && (h < H) && (w >= 0) && (w < W) && (d >= 0) && (d < D);
        const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1), dc = min(max(d, 0), D - 1);
        const size_t vox = ((size_t)hc * W + wc) * D + dc;
        const float wgt = in ? wk[kk] : 0.0f;
        const float4 *p = (const float4 *)((const float *)vol + vox * ST);
        float s[3] = {0.0f, 0.0f, 0.0f};     // this corner's sum_k Y_k f[c][k]
#pragma unroll
        for (int q = 0; q < ST / 4; ++q) {
            const float4 t = p[q];
            const float e[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = 4 * q + r;               // compile-time after unrolling
                if (ch < 3 * NB) s[ch / NB] = fmaf(Y[ch % NB], e[r], s[ch / NB]);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) raw[k] = fmaf(wgt, s[k], raw[k]);
    }
}
