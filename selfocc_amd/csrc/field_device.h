// field_device.h — what the kernels of the fused tri-plane -> volume MLP share (field.hip: the two forwards and the C entry
// points; field_bwd_w.hip: the float32-MFMA backward; field_bwd_b3.hip: the bf16 x 3 backward).  Everything here is inlined:
// a helper stays only while scripts/kernel_isa_diff.py shows the kernels that use it unchanged.
#pragma once
#include "so_device.h"
#include <hip/hip_bf16.h>
#include <cstdlib>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// C layout of a 32 x 32 MFMA result: register v of lane (column i = lane & 31, half = lane >> 5) holds this row
SO_DEVFN int so_crow(int v, int half) { return (v & 3) + 8 * (v >> 2) + 4 * half; }

// torch.nn.Softplus(beta=1, threshold=20): x > 20 ? x : log1p(exp(x)).  Two evaluations whose bits differ, so both stay.
// The libm form (both forwards, the float32 backward):
SO_DEVFN float so_softplus(float x) {
    const float e = __expf(x);
    // log1p(e): alternating series below 0.05 (remainder e^5/5 < 7e-8 relative 1.3e-6), log(1 + e) above
    const float series = e * (1.0f - e * (0.5f - e * (0.33333334f - 0.25f * e)));
    const float lg = __logf(1.0f + e);
    const float r = e < 0.05f ? series : lg;
    return x > 20.0f ? x : r;
}
// The raw-instruction form (the bf16 x 3 backward): 1 + e >= 1 is never denormal, so v_log_f32 / v_exp_f32 without the
// denormal-range scaling that __logf emits under -fno-fast-math — 26 -> 14 vector instructions per evaluation, 192 evaluations
// per voxel row pair
SO_DEVFN float so_softplus_raw(float x) {
    const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f);
    const float series = e * (1.0f - e * (0.5f - e * (0.33333334f - 0.25f * e)));
    const float lg = __builtin_amdgcn_logf(1.0f + e) * 0.69314718055994531f;
    const float r = e < 0.05f ? series : lg;
    return x > 20.0f ? x : r;
}
SO_DEVFN float so_exp_neg_raw(float z) { return __builtin_amdgcn_exp2f(z * -1.44269504088896341f); }     // exp(-z)

// x = a1 + a2 + a3 exactly: the three-way bfloat16 split of linear_fwd.hip
SO_DEVFN void so_split3(const float (&x)[8], bf16x8 &a1, bf16x8 &a2, bf16x8 &a3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 b1 = (__bf16)x[j];
        const float r1 = x[j] - (float)b1;
        const __bf16 b2 = (__bf16)r1;
        const float r2 = r1 - (float)b2;
        a1[j] = b1; a2[j] = b2; a3[j] = (__bf16)r2;
    }
}

// acc += A B with A = a1 + a2 + a3, B = b1 + b2 + b3 (all exact), the six products with i + j <= 4, small terms first
SO_DEVFN void so_mfma6(f32x16 &acc, const bf16x8 &a1, const bf16x8 &a2, const bf16x8 &a3, const bf16x8 &b1, const bf16x8 &b2,
                       const bf16x8 &b3) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);
}

// ---- backward -----------------------------------------------------------------------------------------------------------
struct FieldBwdArgs {
    const float *hw, *zh, *wz;
    int H, W, D;
    const float *w1, *b1, *w2;      // (C, C), (C), (out_dim, C)
    int out_dim;
    const float *g_sdf;             // (M) or NULL
    const float *g_feat;            // (M, feat_stride) or NULL
    int feat_stride;
    float *g_hw, *g_zh, *g_wz;      // zero-initialised, accumulated
    float *g_w1, *g_b1, *g_w2, *g_b2;
    int n_tiles;                    // PH * PW * PD patches of 4 x 4 x 2 voxels
    int PW, PD;
    int dbg;                        // dev switch SELFOCC_FIELD_BWD_DBG: 1 = no zh / wz plane-gradient atomics (b3 only; timing)
};
// the two launchers behind selfocc_field_volume_bwd (field.hip checks the arguments and fills the struct)
int so_field_volume_bwd_w(const FieldBwdArgs &a, int C, hipStream_t st);      // field_bwd_w.hip: float32 MFMA, C = 64 / 96 / 128
int so_field_volume_bwd_b3(const FieldBwdArgs &a, hipStream_t st);            // field_bwd_b3.hip: bf16 x 3, C = 96

// A tile = a 4 (h) x 4 (w) x 2 (d) patch of voxels, tiles numbered d-patches fastest; row r of the tile = voxel
// (r >> 3, (r >> 1) & 3, r & 1) of the patch.  Every plane row (h, w) / (d, h) / (w, d) is then shared by 2 / 4 / 4 rows of the
// tile whose C-layout registers sit in one lane (or its partner half), and the scatter adds them up before it issues an atomic:
// 32 plane-row atomics per tile instead of 66 with 32 consecutive voxels.
SO_DEVFN void so_patch_origin(int tile, int PW, int PD, int &h_b, int &w_b, int &d_b) {
    const int pd = tile % PD, tq = tile / PD;
    const int pw = tq % PW, ph = tq / PW;
    h_b = 4 * ph; w_b = 4 * pw; d_b = 2 * pd;
}
// linear index (h W + w) D + d of patch voxel (hh_, ww_, dd_), clamped into the volume when dead; FULL: the patch lies inside
template <class Idx, bool FULL>
SO_DEVFN Idx so_patch_voxel(int h_b, int w_b, int d_b, int hh_, int ww_, int dd_, int H, int W, int D, bool &live) {
    const int hh = h_b + hh_, ww = w_b + ww_, dd = d_b + dd_;
    if constexpr (FULL) {
        live = true;
        return ((Idx)hh * W + ww) * D + dd;
    } else {
        live = (hh < H) & (ww < W) & (dd < D);
        return ((Idx)min(hh, H - 1) * W + min(ww, W - 1)) * D + min(dd, D - 1);
    }
}
// C-layout register v of lane half = patch voxel  dd = v & 1,  ww = 2 half + ((v >> 1) & 1),  hh = v >> 2: inside the volume?
SO_DEVFN bool so_creg_live(int v, int half, int h_b, int w_b, int d_b, int H, int W, int D) {
    return (h_b + (v >> 2) < H) & (w_b + 2 * half + ((v >> 1) & 1) < W) & (d_b + (v & 1) < D);
}
// d-walk: tile slot sid of n_slots takes a CONTIGUOUS range of tiles (a column of (h, w) patches after the other) and carries
// the 16 hw rows of its current column across the column's d-patches: 16 + 16 / PD instead of 32 plane-row atomics per tile,
// and g_hw no longer depends on the order in which the d-patches of a column arrive
SO_DEVFN void so_tile_range(int n_tiles, int sid, int n_slots, int &t_lo, int &t_hi) {
    t_lo = (int)((long long)n_tiles * sid / n_slots);
    t_hi = (int)((long long)n_tiles * (sid + 1) / n_slots);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// a switch of the environment, read at every call (a test can flip it inside one process)
static inline int so_field_env(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
