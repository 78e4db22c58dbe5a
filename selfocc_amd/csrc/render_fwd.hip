// render_fwd.hip — fused SDF ray-march renderer for gfx950 (MI355X).
//
// One launch replaces, per ray batch, the whole chain the reference runs as dozens of
// torch ops + cuda_gridsample_grad2 inside the sdfstudio fork:
//   ray generation -> AABB collider -> S uniform samples -> meter2grid -> trilinear
//   lookup of the SDF / colour / semantic volume (+ analytic gradient) -> NeuS alpha ->
//   transmittance -> weights -> depth / acc / rgb / sem / max-depth.
// No per-sample tensor touches HBM: launches that ask for the per-sample training outputs go to the sample-parallel
// kernels of render_train.hip (dispatch below).  Ray construction, the box collider and the bin edges are
// those of ray_device.h, shared with render_train.hip and render_bwd.hip; the marches a kernel can run are `enum class March`.
//
// Mapping to the hardware: one ray per lane; in pixel-grid mode a 64-lane wavefront owns
// an 8x8 pixel tile so that, at every march step, the 64 gathers of a wave fall into a
// handful of neighbouring voxels (L1/L2 hits; the volume itself is read from HBM once).
// The transmittance recurrence is then a per-lane scalar chain — no cross-lane scan is
// needed on this path (render_bwd.hip, which must reverse the recurrence, is the kernel
// that scans across lanes).
#include "render_row.h"
#include "ray_device.h"

// render_train.hip
int so_render_fwd_samples(const so_render_args &a, hipStream_t st);

namespace {

// The pixel-grid ray of so_ray_of (ray_device.h), operation for operation, for kernels whose block sits on ONE camera: a
// different code shape on purpose (scalar loads of the camera matrix), not a second definition of the rule.
SO_DEVFN RayGeom so_pixel_ray(const so_render_args &a, int cam, int ix, int iy) {
    // the camera matrix is read-only for the launch and `cam` is block-uniform: constant address space, i.e. scalar loads
    // into SGPRs, also where `a` was re-read through an opaque pointer (so_march_fast_ahead's canonical cell)
    typedef const __attribute__((address_space(4))) float *so_const_fptr;
    const so_const_fptr M = (so_const_fptr)(a.img2lidar + cam * 16);
    float u = (float)ix * a.sx + a.ox;
    float v = (float)iy * a.sy + a.oy;
    RayGeom g;
    g.ox = M[3]; g.oy = M[7]; g.oz = M[11];
    float dx = (M[0] * u + M[1] * v) + M[2];
    float dy = (M[4] * u + M[5] * v) + M[6];
    float dz = (M[8] * u + M[9] * v) + M[10];
    g.dn = sqrtf((dx * dx + dy * dy) + dz * dz);  // neus_head.py:326
    g.dx = dx / g.dn; g.dy = dy / g.dn; g.dz = dz / g.dn;
    return g;
}

template <int NF, bool BF16>
SO_DEVFN void so_gather_feat(const void *__restrict__ vol, int H, int W, int D, const so_cell &c,
                             const float wk[8], float f[NF > 0 ? NF : 1]) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        int h = c.h0 + (kk >> 2), w = c.w0 + ((kk >> 1) & 1), d = c.d0 + (kk & 1);
        bool in = (h >= 0) && (h < H) && (w >= 0) && (w < W) && (d >= 0) && (d < D);
        int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1), dc = min(max(d, 0), D - 1);
        size_t vox = ((size_t)hc * W + wc) * D + dc;
        float wgt = in ? wk[kk] : 0.0f;
        if constexpr (!BF16) {
            const float4 *p = (const float4 *)((const float *)vol + vox * NF);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                float4 t = p[q];
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], t.x, t.y,
                              t.z, t.w, wgt);
            }
        } else {
            const uint2 *p = (const uint2 *)((const uint16_t *)vol + vox * NF);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                uint2 t = p[q];
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], __uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u),
                              __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u), wgt);
            }
        }
    }
}


// ---- buffer-resource loads: one 32-bit lane offset + a uniform (SGPR) corner offset ----------
typedef float so_f2v __attribute__((ext_vector_type(2)));
typedef float so_f4v __attribute__((ext_vector_type(4)));
typedef unsigned so_u2v __attribute__((ext_vector_type(2)));
SO_DEVFN __amdgpu_buffer_rsrc_t so_make_rsrc(const void *p, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, (int)(bytes > 0xfffffffcull ? 0xfffffffcull : bytes), 0x00020000);
}
SO_DEVFN so_f2v so_bload2(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(so_f2v, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
SO_DEVFN so_f4v so_bload4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(so_f4v, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
SO_DEVFN so_u2v so_bload2u(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(so_u2v, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}

// so_gather_sdf (zero padding outside the volume) on buffer loads: one 32-bit lane offset per (h, w) column instead of a
// 64-bit address pair — the rare paths of the SDF-only marcher use it, where the four address pairs were what set the
// kernel's register peak (75 -> 70 VGPRs: 7 waves / SIMD instead of 6)
SO_DEVFN void so_gather_sdf_buf(__amdgpu_buffer_rsrc_t rs, int H, int W, int D, int h0, int w0, int d0, float v[8]) {
    const int d0c = min(max(d0, 0), D - 2);
    const bool dlo_in = (unsigned)d0 < (unsigned)D, dhi_in = (unsigned)(d0 + 1) < (unsigned)D;
    const bool lo_first = (d0 == d0c), hi_first = (d0 + 1 == d0c);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int h = h0 + (q >> 1), w = w0 + (q & 1);
        const bool in = ((unsigned)h < (unsigned)H) && ((unsigned)w < (unsigned)W);
        const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1);
        const so_f2v pr = so_bload2(rs, (unsigned)((hc * W + wc) * D + d0c) * 4u, 0u);
        const float lo = lo_first ? pr.x : pr.y, hi = hi_first ? pr.x : pr.y;
        v[2 * q] = (in && dlo_in) ? lo : 0.0f;
        v[2 * q + 1] = (in && dhi_in) ? hi : 0.0f;
    }
}

// all 8 corners in range (wave-uniform precondition): 8 uniform corner bases + one lane offset
template <int NF, bool BF16>
SO_DEVFN void so_gather_feat_interior(__amdgpu_buffer_rsrc_t rf, int W, int D, unsigned cell,
                                      const float wk[8], float f[NF > 0 ? NF : 1]) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
    constexpr unsigned VB = BF16 ? NF * 2u : NF * 4u;   // bytes per voxel
    const unsigned off = cell * VB;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
        const unsigned corner = ((unsigned)(kk >> 2) * W * D + (unsigned)((kk >> 1) & 1) * D + (kk & 1)) * VB;  // uniform
        const float wgt = wk[kk];
        if constexpr (!BF16) {
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const so_f4v t = so_bload4(rf, off + q * 16u, corner);
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], t.x, t.y,
                              t.z, t.w, wgt);
            }
        } else {
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const so_u2v t = so_bload2u(rf, off + q * 8u, corner);
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], __uint_as_float(t.x << 16), __uint_as_float(t.x & 0xffff0000u),
                              __uint_as_float(t.y << 16), __uint_as_float(t.y & 0xffff0000u), wgt);
            }
        }
    }
}

// ROW: the feature row (render_row.h).  MK: the mapping kind (SO_MAP_LINEAR / SO_MAP_UPSCALE), a compile-time choice of so_locate_k
template <class ROW, int MK>
SO_DEVFN void so_march_exact(const so_render_args &a, int ray, const RayGeom &g) {
    constexpr int NF = ROW::NF, NB = ROW::NB, NSEM = ROW::NSEM;
    constexpr bool BF16 = ROW::BF16, MASKED = ROW::MASKED;
    const int nsem = MASKED ? a.n_sem : NSEM;                // wave-uniform
    float Y[NB > 0 ? NB : 1];                   // the ray's basis: once, before the march
    if constexpr (NB > 0) so_sh_basis<NB>(g.dx, g.dy, g.dz, Y);
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int S = a.n_samples;
    float tnear, tfar;
    so_collide(a, g, tnear, tfar);

    float T = 1.0f, acc = 0.0f, dsum = 0.0f;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    float sem[NSEM > 0 ? NSEM : 1];
#pragma unroll
    for (int k = 0; k < NSEM; ++k) sem[k] = 0.0f;
    float best_q = -INFINITY, best_t = 0.0f;
    const float eps32 = 1.1920928955078125e-07f;

    float t_end = so_edge(a, ray, 0, tnear, tfar);
    for (int i = 0; i < S; ++i) {
        float t_start = t_end;
        t_end = so_edge(a, ray, i + 1, tnear, tfar);
        float delta = t_end - t_start;
        float t_mid = (t_start + t_end) / 2.0f;
        float px, py, pz;
        so_sample_point(a, g, t_start, t_end, px, py, pz);
        so_cell c = so_locate_k<MK>(a.map, px, py, pz);
        float v[8], wk[8];
        so_gather_sdf(a.sdf_vol, H, W, D, c, v);
        float sdf = so_trilerp_sdf(c, v, wk);
        float gx, gy, gz;
        so_trilerp_grad(c, v, gx, gy, gz);
        float alpha = so_neus_alpha(g, sdf, gx, gy, gz, delta, so_inv_s(a));
        float w = alpha * T;
        T = T * ((1.0f - alpha) + 1e-7f);

        acc = acc + w;
        dsum = dsum + w * t_mid;

        float tz = t_mid / g.dn, dz_ = delta / g.dn;
        float wq = (dz_ < eps32) ? 0.0f : w;
        float q = wq / fmaxf(dz_, eps32);
        if (q > best_q) { best_q = q; best_t = tz; }

        if constexpr (NB > 0) {
            float raw[3];
            so_sh_gather<NB>(a.feat_vol, H, W, D, c, wk, Y, raw);
#pragma unroll
            for (int k = 0; k < 3; ++k) rgb[k] = fmaf(w, so_sh_act(raw[k], a.sh_act), rgb[k]);
        } else if constexpr (NF > 0) {
            float f[NF];
            so_gather_feat<NF, BF16>(a.feat_vol, H, W, D, c, wk, f);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float col = fmaxf(0.28209479177387814f * f[k] + 0.5f, 0.0f);  // sh_render.py:84-91
                rgb[k] = fmaf(w, col, rgb[k]);
            }
            if constexpr (NSEM > 0) {
                float m = f[3];
#pragma unroll
                for (int k = 1; k < NSEM; ++k) if (SO_SEM_ON(k)) m = fmaxf(m, f[3 + k]);
                float e[NSEM], den = 0.0f;
#pragma unroll
                for (int k = 0; k < NSEM; ++k) {
                    if (SO_SEM_ON(k)) { e[k] = so_expf(f[3 + k] - m); den = den + e[k]; }
                    else e[k] = 0.0f;
                }
                float wd = w / den;
#pragma unroll
                for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) sem[k] = fmaf(wd, e[k], sem[k]);
            }
        }
    }

    float depth = dsum / (acc + 1e-10f);
    if (a.flags & SO_FLAG_DEPTH_DIV_NORM) depth = depth / g.dn;
    if (a.depth) a.depth[ray] = depth;
    if (a.acc) a.acc[ray] = acc;
    if (a.max_depth) a.max_depth[ray] = best_t;
    if (a.nears) a.nears[ray] = tnear;
    if (a.fars) a.fars[ray] = tfar;
    if constexpr (NF > 0) {
        if (a.rgb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float bg = 0.0f;
                if (a.bkgd_mode == SO_BKGD_CONST) bg = a.bkgd[k];
                else if (a.bkgd_mode == SO_BKGD_PER_RAY) bg = a.bkgd_rays[3 * (size_t)ray + k];
                float r = rgb[k];
                if (a.bkgd_mode != SO_BKGD_NONE) r = r + bg * (1.0f - acc);
                if (a.flags & SO_FLAG_CLAMP_RGB) r = fminf(fmaxf(r, 0.0f), 1.0f);
                a.rgb[3 * (size_t)ray + k] = r;
            }
        }
        if constexpr (NSEM > 0) {
            if (a.sem) {
#pragma unroll
                for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) a.sem[(size_t)ray * nsem + k] = sem[k];
            }
        }
    }
}


// ---------------------------------------------------------------------------------------
// Fast march (default): identical algorithm, cheaper arithmetic.
//   * single-segment linear axes make the grid coordinate affine in t: g(t) = G0 + Gd * t,
//     three fmas per sample instead of three divide chains + normalise/un-normalise;
//   * sigmoid = rcp(1 + exp2(.)) on the hardware transcendental unit (v_exp_f32/v_rcp_f32);
//   * nested lerps (value + analytic gradient share the 4 d-axis differences);
//   * constant step => argmax_s(w / delta) == argmax_s(w);
//   * wave-level early termination once every lane's transmittance is < 1e-10
//     (everything still to come would add < 1e-10 to any output).
// Deviates from the canonical order by a few ulp per op; parity tests bound it.
// ---------------------------------------------------------------------------------------
struct AxisK { float k1, k0; };
#define SO_HOSTDEVFN __host__ __device__ __forceinline__    // launch constants: the same expression on either side
SO_HOSTDEVFN AxisK so_axis_affine(const so_axis &A) {
    AxisK k;
    k.k1 = A.size0 / A.range0;
    k.k0 = (A.off0 + A.off1) - A.start * k.k1;
    return k;
}

SO_DEVFN float so_fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
SO_DEVFN float so_fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// wave-wide AND of a per-lane predicate: one v_cmp + one scalar compare (HIP's __all() goes through a select)
SO_DEVFN bool so_all(bool p) { return __builtin_amdgcn_ballot_w64(p) == __builtin_amdgcn_ballot_w64(true); }
// wave-wide AND of p && q && r: one ballot per compare, combined in SGPRs.  so_all(p & q & r) materialises the combined lane
// mask through a VGPR (v_cndmask + v_cmp) before the ballot: two VALU instructions per use.
SO_DEVFN bool so_all3(bool p, bool q, bool r) {
    return (__builtin_amdgcn_ballot_w64(p) & __builtin_amdgcn_ballot_w64(q) & __builtin_amdgcn_ballot_w64(r)) ==
           __builtin_amdgcn_ballot_w64(true);
}
// (h * W + w) * D + d for in-range cells with full-rate 24-bit multiplies (v_mad_u32_u24); the 32-bit / 64-bit
// integer multiplies the compiler picks for plain ints are quarter rate.  Needs H * W < 2^24, D < 2^24.
// The first multiply-add is written out: from __umul24(h0, W) + w0 the compiler forms the quarter-rate v_mad_u64_u32.
// The value differs from the plain expression only where h0 or W leave 24 bits, i.e. for cells that are never addressed.
SO_DEVFN unsigned so_cell_index(int h0, int w0, int d0, int W, int D) {
    unsigned hw;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(hw) : "v"(h0), "s"(W), "v"(w0));
    return __umul24(hw, (unsigned)D) + (unsigned)d0;
}
SO_DEVFN int so_floor_i(float x) {   // (int)floorf(x) in one instruction
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// NeuS alpha = (sig(a) - sig(b) + 1e-5) / (sig(a) + 1e-5), a = (sdf - half) s, b = (sdf + half) s, half <= 0,
// rewritten with ea = exp(-a), eb = exp(-b) >= ea so that no two nearly equal sigmoids are subtracted:
//     alpha = ((eb - ea) / (1 + eb) + 1e-5 (1 + ea)) / (1 + 1e-5 (1 + ea))
// (two reciprocals instead of three; exact algebra).  xs = sdf * s * log2(e), hs = half * s * log2(e) <= 0.
// The exponents are clamped at 60: 2^60 keeps every term finite and alpha is 1 to ~1e-13 there already.
SO_DEVFN float so_alpha_fast(float xs, float hs) {
    const float ea = so_fast_exp2(fminf(hs - xs, 60.0f)), eb = so_fast_exp2(fminf(-hs - xs, 60.0f));
    const float p = 1.0f + ea;
    const float num = fmaf(eb - ea, so_fast_rcp(1.0f + eb), 1e-5f * p);
    const float den = fmaf(1e-5f, p, 1.0f);
    return fminf(num * so_fast_rcp(den), 1.0f);
}

// Value and voxel-unit gradient of the trilinear SDF in the fast path's nested-lerp order (d, then w, then h; the
// gradients reuse the differences), on packed FP32.  The corners travel as the pairs pk = (v[k], v[k + 4]), h = 0 in the low
// and h = 1 in the high half — the order the brick records store them in (sdf_brickify_kernel) — so the d- and w-level lerps
// and the e0 / e1 terms of the d gradient run two-wide with fd / fw broadcast from a low half; the h level combines the two
// halves of one pair and stays scalar (a half-swapping form otherwise).  Each half of a packed op is exactly
// the scalar op it replaces (a packed FMA rounds like fmaf): the results are bit-identical to the scalar sequence.
SO_DEVFN void so_trilerp_fast_pk(so_f32x2 p0, so_f32x2 p1, so_f32x2 p2, so_f32x2 p3, float fh, float fw, float fd,
                                 float &sdf, float &gvh, float &gvw, float &gvd) {
    const so_f32x2 bd = {fd, fd}, bw = {fw, fw};
    const so_f32x2 dda = p1 - p0, ddb = p3 - p2;                        // (dd0, dd2), (dd1, dd3)
    const so_f32x2 ca = __builtin_elementwise_fma(bd, dda, p0);         // (c0, c2)
    const so_f32x2 cb = __builtin_elementwise_fma(bd, ddb, p2);         // (c1, c3)
    const so_f32x2 dw = cb - ca;                                        // (dw0, dw1)
    const so_f32x2 b = __builtin_elementwise_fma(bw, dw, ca);           // (b0, b1)
    const so_f32x2 e = __builtin_elementwise_fma(bw, ddb - dda, dda);   // (e0, e1)
    gvh = b[1] - b[0];
    sdf = fmaf(fh, gvh, b[0]);
    gvw = fmaf(fh, dw[1] - dw[0], dw[0]);
    gvd = fmaf(fh, e[1] - e[0], e[0]);
}

// ---- free-space skip codes --------------------------------------------------------------------
// A sample whose two sigmoid arguments both exceed 17.5 has exp(-arg) < 2^-25, so 1 + exp(-arg) == 1.0f and
// BOTH sigmoids are exactly 1.0f in float32, in the canonical order as well: alpha is the constant
// kAlphaFree = (0 + 1e-5f) / (1 + 1e-5f), no matter what the SDF value or gradient is.  Inside one voxel cell
// the trilinear SDF is >= the smallest corner m and |cos| <= |grad| <= G (per-axis maxima of the edge
// differences), so every sample of a ray with step dt inside the cell is such a sample whenever
//     (m - G dt / 2) inv_s >= 17.5   <=>   dt <= 2 (m - 17.5 / inv_s) / G =: allow_dt(cell).
// The brick re-pack pass stores allow_dt per cell as one byte in units of so_skip_unit() (rounded down, the ray's
// own dt is rounded up), and a wave whose 64 lanes all sit in such cells composites the constant alpha without
// touching the corners: same results, ~1/4 of the vector instructions of a full step.
constexpr float kSkipArg = 17.5f;
constexpr float kAlphaFree = 1e-5f / (1.0f + 1e-5f);
SO_HOSTDEVFN float so_skip_unit(const float aabb[6], int n_samples) {   // metres per code step: box diagonal / S / 255
    const float ex = aabb[3] - aabb[0], ey = aabb[4] - aabb[1], ez = aabb[5] - aabb[2];
    return sqrtf(ex * ex + ey * ey + ez * ez) / ((float)n_samples * 255.0f);
}

// ---- launch constants ---------------------------------------------------------------------------
// What the skip marchers (so_march_fast_ahead) and the brick pass need of a launch and no ray or cell changes, computed once
// on the host and passed by value as a kernel argument, instead of once per wave (three IEEE divisions for the axes, a
// square root and a division for the skip unit) or per cell (sdf_brickify_kernel: four divisions and a square root).  The
// host evaluates the device's own float32 expressions (so_axis_affine, so_skip_unit, the face margin as in so_march_fast):
// IEEE division and square root are correctly rounded on either side and the library is built without contraction, so
// every field is bit for bit what the kernels computed themselves — so_march_fast still does, and the tests that hold the
// two routes equal compare host against device.  Nothing here depends on inv_s, which may live on the device alone.
struct so_launch_consts {
    AxisK kh, kw, kd;             // so_axis_affine of the three axes
    float skip_unit;              // so_skip_unit
    float face_m;                 // near-face margin in grid units (see so_march_fast)
    float n_samples_f;            // (float)S
    unsigned n_cells;             // H * W * D
    unsigned codes_off;           // byte offset of the skip codes in the brick workspace: n_cells * 16
    unsigned row_off;             // byte offset from a cell's record to that of (h, w + 1, d): D * 16
};
so_launch_consts so_make_launch_consts(const so_render_args &a) {
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    so_launch_consts c;
    c.kh = so_axis_affine(a.map.h); c.kw = so_axis_affine(a.map.w); c.kd = so_axis_affine(a.map.d);
    c.skip_unit = so_skip_unit(a.aabb, a.n_samples);
    const int maxdim = H > W ? (H > D ? H : D) : (W > D ? W : D);
    c.face_m = 3.0f * 1.1920929e-7f * (float)(1u << (32 - __builtin_clz((unsigned)maxdim)));
    c.n_samples_f = (float)a.n_samples;
    c.n_cells = (unsigned)(H * W * D);
    c.codes_off = c.n_cells * 16u;
    c.row_off = (unsigned)D * 16u;
    return c;
}


// ---- LDS staging of the wavefront's voxel neighbourhood -----------------------------------
// At one march step the 64 rays of an 8x8 pixel tile sit within ~1 voxel of each other, so
// their 64 x 8 corner fetches hit the same <= 4x4x4 voxels: through the vector L1 that is
// 64 x 8 x NF*4 B of traffic per step (the measured limiter: 86 % of the 64 B/clk/CU L1
// rate at NF = 24).  Instead the wave loads the 4x4x4 block once (lane l <-> voxel l, NF/4
// coalesced 16-B loads), parks it in LDS (row stride NF+4 dwords: 16 conflict-free 16-B
// slots) and every lane reads its 8 corners with ds_read_b128 (256 B/clk/CU).
// A wave whose cells span more than 3 along an axis takes the direct path (wave-uniform).
SO_DEVFN unsigned so_wave_or(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);  // row_bcast:15
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);  // row_bcast:31
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int NF>
struct StageGeom {
    // dwords per staged voxel: an ODD multiple of 4 => 16-B aligned rows landing on all 16 16-B bank slots
    static constexpr int kStride = ((NF / 4) & 1) ? NF : NF + 4;
    static constexpr int kWaveDwords = 64 * kStride;
};

// returns true (wave-uniform) and fills hmin/wmin/dmin when the wave's clamped low corners
// span <= 2 cells per axis, i.e. all corners live in the 4x4x4 block at (hmin, wmin, dmin)
SO_DEVFN bool so_stage_box(int h0, int w0, int d0, int H, int W, int D, int &hmin, int &wmin, int &dmin) {
    const int lh = min(max(h0, 0), H - 1), lw = min(max(w0, 0), W - 1), ld = min(max(d0, 0), D - 1);
    const int bh = __builtin_amdgcn_readfirstlane(lh), bw = __builtin_amdgcn_readfirstlane(lw),
              bd = __builtin_amdgcn_readfirstlane(ld);
    const int oh = lh - bh + 4, ow = lw - bw + 4, od = ld - bd + 4;      // expected in [0, 9]
    const bool bad = ((unsigned)oh > 9u) || ((unsigned)ow > 9u) || ((unsigned)od > 9u);
    const unsigned m = bad ? 0x80000000u : ((1u << oh) | (1u << (10 + ow)) | (1u << (20 + od)));
    const unsigned u = so_wave_or(m);
    if (u & 0x80000000u) return false;
    const unsigned fh = u & 0x3ffu, fw = (u >> 10) & 0x3ffu, fd = (u >> 20) & 0x3ffu;
    const int lo_h = __builtin_ctz(fh), lo_w = __builtin_ctz(fw), lo_d = __builtin_ctz(fd);
    const int hi_h = 31 - __builtin_clz(fh), hi_w = 31 - __builtin_clz(fw), hi_d = 31 - __builtin_clz(fd);
    if (hi_h - lo_h > 2 || hi_w - lo_w > 2 || hi_d - lo_d > 2) return false;
    hmin = bh - 4 + lo_h; wmin = bw - 4 + lo_w; dmin = bd - 4 + lo_d;
    return true;
}

template <int NF, bool BF16>
SO_DEVFN void so_gather_feat_staged(__amdgpu_buffer_rsrc_t rf, const void *__restrict__ vol, int H, int W, int D,
                                    int h0, int w0, int d0, int hmin, int wmin, int dmin, const float wk[8],
                                    float *lds, int lane, unsigned lane_vox, bool pref, const so_f4v blk[NF / 4],
                                    bool all_interior, float f[NF]) {
    static_assert(!BF16, "staged path: float32 feature volume");
    constexpr int ST = StageGeom<NF>::kStride;
    {   // lane <-> voxel (i, j, k) of the block: registers prefetched a step ahead, or (block touching the
        // volume edge) loaded here with clamped coordinates (duplicates are harmless)
        float4 *dst = (float4 *)(lds + lane * ST);
        so_f4v t[NF / 4];
        if (pref) {
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) t[q] = blk[q];
        } else if (hmin + 3 < H && wmin + 3 < W && dmin + 3 < D) {   // whole block inside the volume (uniform)
            const unsigned vo = ((unsigned)((hmin * W + wmin) * D + dmin) + lane_vox) * (NF * 4u);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) t[q] = so_bload4(rf, vo + q * 16u, 0u);
        } else {
            const int vh = min(hmin + (lane >> 4), H - 1), vw = min(wmin + ((lane >> 2) & 3), W - 1),
                      vd = min(dmin + (lane & 3), D - 1);
            const so_f4v *src = (const so_f4v *)((const float *)vol + ((size_t)(vh * W + vw) * D + vd) * NF);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) t[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < NF / 4; ++q) dst[q] = make_float4(t[q].x, t[q].y, t[q].z, t[q].w);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0f;
    if (all_interior) {
        // no padding anywhere: the 8 corners sit at compile-time offsets from ONE lane address
        const float *p0 = lds + (((h0 - hmin) * 4 + (w0 - wmin)) * 4 + (d0 - dmin)) * ST;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const float4 *p = (const float4 *)(p0 + ((kk >> 2) * 16 + ((kk >> 1) & 1) * 4 + (kk & 1)) * ST);
            const float wgt = wk[kk];
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const float4 t = p[q];
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], t.x, t.y,
                              t.z, t.w, wgt);
            }
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int h = h0 + (kk >> 2), w = w0 + ((kk >> 1) & 1), d = d0 + (kk & 1);
            const bool in = ((unsigned)h < (unsigned)H) && ((unsigned)w < (unsigned)W) && ((unsigned)d < (unsigned)D);
            const int li = ((min(max(h, 0), H - 1) - hmin) * 4 + (min(max(w, 0), W - 1) - wmin)) * 4 +
                           (min(max(d, 0), D - 1) - dmin);
            const float wgt = in ? wk[kk] : 0.0f;
            const float4 *p = (const float4 *)(lds + li * ST);
#pragma unroll
            for (int q = 0; q < NF / 4; ++q) {
                const float4 t = p[q];
                so_fma4_bcast(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3], t.x, t.y,
                              t.z, t.w, wgt);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next step's stores must not overtake these reads
}

// The launch arguments re-read from the kernarg segment through a pointer the optimiser cannot see through (the kernels
// take so_render_args as their FIRST parameter): only the fields used are loaded (s_load), where they are used, and nothing
// is shared with (or hoisted out of a loop as) the copy the kernel started with.
SO_DEVFN so_render_args so_reload_args() {
    typedef const __attribute__((address_space(4))) uint32_t *so_kernarg_ptr;
    so_kernarg_ptr ka = (so_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    so_render_args ac;
    static_assert(sizeof(ac) % 4 == 0, "so_render_args is dword-sized");
#pragma unroll
    for (unsigned k = 0; k < sizeof(ac) / 4; ++k) ((uint32_t *)&ac)[k] = ka[k];
    return ac;
}

// what `fetch` leaves in registers for one march step
template <int NF>
struct FastStep {
    float fh, fw, fd, fi;         // fractional grid coordinates, step index as float
    int h0, w0, d0;               // cell
    unsigned cell;                // linear index of the low corner
    bool all_interior;            // wave-uniform: no lane needs padding at this step
    float v[8];                   // SDF corners (d fastest)
    unsigned code;                // free-space skip code of the cell (0 = never skip)
    bool boxed, pref;             // wave-uniform: LDS staging applies / block already loaded
    int hmin, wmin, dmin;         // staged block origin
    so_f4v blk[NF >= 4 ? NF / 4 : 1];
};

// `geom()` returns the lane's ray; it is called once up front and again inside the (rare) canonical cell
// fallback, so that origin / direction / far need not stay in registers across the march loop.
template <class ROW, bool STAGED, bool FACE_SAFE, class GeomFn>
SO_DEVFN void so_march_fast(const so_render_args &a, int ray, GeomFn geom, bool store = true,
                             float *lds = nullptr, int lane = 0, float *sem_lds = nullptr) {
    static_assert(ROW::NB == 0, "the fast march renders degree-0 relu colour");
    constexpr int NF = ROW::NF, NSEM = ROW::NSEM;
    constexpr bool BF16 = ROW::BF16, MASKED = ROW::MASKED;
    const int nsem = MASKED ? a.n_sem : NSEM;   // wave-uniform (see so_march_exact)
    // The staged 24-channel float32 kernel keeps its 21 semantic accumulators in LDS (sem_lds[k * 256 + thread];
    // read-modify-write of a lane-private slot; ds_add_f32 measured 5 x slower) instead of registers: at 2 waves / SIMD the 256-VGPR budget was 14 - 19 registers short and the spills
    // went through the texture path the march is bound by (32 scratch accesses per sample beside 9 real loads).
    constexpr bool SEM_LDS = STAGED && NSEM >= 16;
    const RayGeom g = geom(a);
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int S = a.n_samples;
    float tnear, tfar;
    so_collide(a, g, tnear, tfar);
    const float dt = (tfar - tnear) / (float)S;
    const float inv_dn = 1.0f / g.dn;

    const AxisK kh = so_axis_affine(a.map.h), kw = so_axis_affine(a.map.w), kd = so_axis_affine(a.map.d);
    // grid coordinate along the ray: g(t) = G0 + Gd * t   (h <-> y, w <-> x, d <-> z)
    const float t_off = (a.sample_pos == SO_SAMPLE_AT_START) ? tnear : tnear + 0.5f * dt;
    const float Gdh = g.dy * kh.k1, Gdw = g.dx * kw.k1, Gdd = g.dz * kd.k1;
    const float G0h = fmaf(g.oy, kh.k1, kh.k0) + Gdh * t_off;
    const float G0w = fmaf(g.ox, kw.k1, kw.k0) + Gdw * t_off;
    const float G0d = fmaf(g.oz, kd.k1, kd.k0) + Gdd * t_off;
    const float s2 = so_inv_s(a) * 1.44269504088896341f;  // exp(-x s) = exp2(-x s log2 e)
    const float hdt = 0.5f * dt;
    const float hdt_s2 = hdt * s2;

    float T = 1.0f, acc = 0.0f, dsum = 0.0f;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    float sem[(NSEM > 0 && !SEM_LDS) ? NSEM : 1];
    if constexpr (SEM_LDS) {
#pragma unroll
        for (int k = 0; k < NSEM; ++k) sem_lds[k * 256] = 0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < NSEM; ++k) sem[k] = 0.0f;
    }
    float best_w = -1.0f, best_t = 0.0f;
    const float *__restrict__ vol = a.sdf_vol;
    const __amdgpu_buffer_rsrc_t rs = so_make_rsrc(vol, (size_t)H * W * D * 4);
    const unsigned sD = (unsigned)D * 4u, sWD = (unsigned)W * D * 4u;
    const bool use_brick = a.sdf_brick != nullptr;                       // uniform
    const unsigned n_cells = (unsigned)(H * W * D);
    // brick workspace = 16-B records of every cell (sdf_brickify_kernel), then one skip-code byte per cell
    const __amdgpu_buffer_rsrc_t rb = so_make_rsrc(a.sdf_brick, use_brick ? (size_t)n_cells * 17 : 0);
    const unsigned lane_vox = (unsigned)(((lane >> 4) * W + ((lane >> 2) & 3)) * D + (lane & 3));  // block voxel of this lane
    const __amdgpu_buffer_rsrc_t rf = so_make_rsrc(a.feat_vol, NF > 0 ? (size_t)H * W * D * NF * (BF16 ? 2 : 4) : 0);
    // free-space skipping (see so_skip_unit): SDF-only launches
    constexpr bool CAN_SKIP = NF == 0;
    const bool use_skip = CAN_SKIP && use_brick && !(a.flags & SO_FLAG_NO_SKIP);          // uniform
    // the ray's own step, rounded UP to skip-code units (>= 1; > 255 never skips)
    const int rcode = use_skip ? max((int)ceilf(dt / so_skip_unit(a.aabb, S)), 1) : 0x7fffffff;
    // Cell selection.  g(t) above differs from the canonical divide chain by <= ~1.5 ulp of the coordinate; a
    // sample within face_m of a voxel face could therefore land in the neighbouring cell, where the trilinear
    // GRADIENT (hence alpha) differs.  Such lanes (~2e-4 of all samples) recompute their position in the
    // canonical order, so the fast path picks the same cell as the canonical path / the reference, always.
    const int maxdim = max(H, max(W, D));
    const float face_m = 3.0f * 1.1920929e-7f * (float)(1u << (32 - __builtin_clz((unsigned)maxdim)));

    // SDF-only kernels test for face proximity only on the steps that actually interpolate (a skipped step's
    // alpha is the same constant on either side of a face) and patch the sample up inside `consume`
    constexpr bool FACE_LATE = FACE_SAFE && NF == 0;
    auto near_face = [&](float fh, float fw, float fd) __attribute__((always_inline)) {
        return fmaxf(fmaxf(fabsf(fh - 0.5f), fabsf(fw - 0.5f)), fabsf(fd - 0.5f)) > 0.5f - face_m;
    };
    // the sample's cell in the canonical order: the operation sequence of so_edge / so_locate (= so_march_exact =
    // the oracle), specialised to what the fast path already requires (no jitter, single-segment axes).
    auto canon_cell = [&](const int i) __attribute__((always_inline)) {
        if constexpr (NF < 8) {
            // light kernels: from the ray that stays live in registers; ~6 IEEE divisions, no memory access
            const float b0 = so_bin(i, S);
            const float t_start = b0 * tfar + (1.0f - b0) * tnear;
            float px, py, pz;
            if (a.sample_pos == SO_SAMPLE_AT_START) {
                px = g.ox + g.dx * t_start; py = g.oy + g.dy * t_start; pz = g.oz + g.dz * t_start;
            } else {
                const float b1 = so_bin(i + 1, S);
                const float tt = t_start + (b1 * tfar + (1.0f - b1) * tnear);
                px = g.ox + (g.dx * tt) / 2.0f; py = g.oy + (g.dy * tt) / 2.0f; pz = g.oz + (g.dz * tt) / 2.0f;
            }
            return so_locate(a.map, px, py, pz);
        } else {
            // 20+ feature channels: registers are the scarce resource (2 waves / SIMD).  The ray and the launch
            // arguments are re-derived inside this rare branch from arguments re-read from the kernarg segment
            // (so_reload_args), otherwise every mapping / camera constant is hoisted out of the march loop into ~40 SGPRs.
            const so_render_args ac = so_reload_args();
            const RayGeom gc = geom(ac);
            float tn, tf;
            so_collide(ac, gc, tn, tf);
            const float t_start = so_edge(ac, ray, i, tn, tf);
            float px, py, pz;
            if (ac.sample_pos == SO_SAMPLE_AT_START) {
                px = gc.ox + gc.dx * t_start; py = gc.oy + gc.dy * t_start; pz = gc.oz + gc.dz * t_start;
            } else {
                const float tt = t_start + so_edge(ac, ray, i + 1, tn, tf);
                px = gc.ox + (gc.dx * tt) / 2.0f; py = gc.oy + (gc.dy * tt) / 2.0f; pz = gc.oz + (gc.dz * tt) / 2.0f;
            }
            return so_locate(ac.map, px, py, pz);
        }
    };

    constexpr bool PIPE = NF < 8;   // see the loop below
    // ---- stage 1: geometry of step i + every global load it needs, issued one step ahead ------
    auto fetch = [&](const int i, FastStep<NF> &st) __attribute__((always_inline)) {
        st.fi = (float)i;
        const float step = st.fi * dt;
        const float gh = fmaf(Gdh, step, G0h), gw = fmaf(Gdw, step, G0w), gd = fmaf(Gdd, step, G0d);
        st.fh = __builtin_amdgcn_fractf(gh); st.fw = __builtin_amdgcn_fractf(gw); st.fd = __builtin_amdgcn_fractf(gd);
        int h0 = so_floor_i(gh), w0 = so_floor_i(gw), d0 = so_floor_i(gd);
        if constexpr (FACE_SAFE && !FACE_LATE) {   // feature kernels: before the staging box / gathers are set up
            if (__any(near_face(st.fh, st.fw, st.fd))) {
                if (near_face(st.fh, st.fw, st.fd)) {
                    const so_cell c = canon_cell(i);
                    h0 = c.h0; w0 = c.w0; d0 = c.d0;
                    st.fh = c.fh1; st.fw = c.fw1; st.fd = c.fd1;
                }
            }
        }
        st.h0 = h0; st.w0 = w0; st.d0 = d0;
        // a wave whose 64 cells are all strictly inside the volume (the common case) needs no
        // clamps / padding selects and addresses its 4 (h, w) columns as ONE 32-bit lane offset +
        // 4 uniform (SGPR) offsets of a buffer resource; otherwise zero padding: clamp + select
        const bool interior = ((unsigned)h0 < (unsigned)(H - 1)) & ((unsigned)w0 < (unsigned)(W - 1)) &
                              ((unsigned)d0 < (unsigned)(D - 1));
        st.all_interior = so_all(interior);
        st.cell = so_cell_index(h0, w0, d0, W, D);     // only used when every lane is interior
        st.code = 0u;
        if (st.all_interior) {
            if (use_brick) {   // 8 corners = the records of cells (h, w, d) and (h, w + 1, d): 2 wide loads instead of 4 gathers
                const unsigned vo = st.cell * 16u;
                const so_f4v lo = so_bload4(rb, vo, 0u), hi = so_bload4(rb, vo, (unsigned)D * 16u);
                if constexpr (CAN_SKIP) {
                    if (use_skip) st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, st.cell, n_cells * 16u, 0);
                }
                st.v[0] = lo.x; st.v[4] = lo.y; st.v[1] = lo.z; st.v[5] = lo.w;   // record order: see sdf_brickify_kernel
                st.v[2] = hi.x; st.v[6] = hi.y; st.v[3] = hi.z; st.v[7] = hi.w;
            } else {
                const unsigned vo = st.cell * 4u;
                const so_f2v p00 = so_bload2(rs, vo, 0u), p01 = so_bload2(rs, vo, sD);
                const so_f2v p10 = so_bload2(rs, vo, sWD), p11 = so_bload2(rs, vo, sWD + sD);
                st.v[0] = p00.x; st.v[1] = p00.y; st.v[2] = p01.x; st.v[3] = p01.y;
                st.v[4] = p10.x; st.v[5] = p10.y; st.v[6] = p11.x; st.v[7] = p11.y;
            }
        } else {
            const int d0c = min(max(d0, 0), D - 2);
            const bool dlo_in = (unsigned)d0 < (unsigned)D, dhi_in = (unsigned)(d0 + 1) < (unsigned)D;
            const bool lo_first = (d0 == d0c), hi_first = (d0 + 1 == d0c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int h = h0 + (q >> 1), w = w0 + (q & 1);
                const bool in = ((unsigned)h < (unsigned)H) && ((unsigned)w < (unsigned)W);
                const int hc = min(max(h, 0), H - 1), wc = min(max(w, 0), W - 1);
                const so_f2u pr = *(const so_f2u *)(vol + ((hc * W + wc) * D + d0c));
                const float lo = lo_first ? pr.x : pr.y, hi = hi_first ? pr.x : pr.y;
                st.v[2 * q] = (in && dlo_in) ? lo : 0.0f;
                st.v[2 * q + 1] = (in && dhi_in) ? hi : 0.0f;
            }
        }
        st.boxed = false; st.pref = false;
        if constexpr (STAGED) {
            st.boxed = so_stage_box(h0, w0, d0, H, W, D, st.hmin, st.wmin, st.dmin);
            if (PIPE && st.boxed && st.hmin + 3 < H && st.wmin + 3 < W && st.dmin + 3 < D) {   // block inside the volume
                const unsigned vo = ((unsigned)((st.hmin * W + st.wmin) * D + st.dmin) + lane_vox) * (NF * 4u);
#pragma unroll
                for (int q = 0; q < NF / 4; ++q) st.blk[q] = so_bload4(rf, vo + q * 16u, 0u);
                st.pref = true;
            }
        }
    };

    // ---- stage 2: interpolation, NeuS alpha, compositing of step i ----------------------------
    auto consume = [&](const int i, FastStep<NF> &st) __attribute__((always_inline)) {
        const float fi = st.fi;
        const float *v = st.v;
        float w, sdf = 0.0f, gvw = 0.0f, gvd = 0.0f, gvh = 0.0f;
        bool skip = false;
        if constexpr (CAN_SKIP) skip = so_all((int)st.code >= rcode);   // every lane in saturated free space
        if (skip) {
            w = kAlphaFree * T;
            T = T * ((1.0f - kAlphaFree) + 1e-7f);
        } else {
            if constexpr (FACE_LATE) {
                if (__any(near_face(st.fh, st.fw, st.fd))) {
                    if (near_face(st.fh, st.fw, st.fd)) {
                        const so_cell c = canon_cell(i);
                        if (c.h0 != st.h0 || c.w0 != st.w0 || c.d0 != st.d0) {   // the canonical order lands next door
                            so_gather_sdf(vol, H, W, D, c, st.v);
                            st.fh = c.fh1; st.fw = c.fw1; st.fd = c.fd1;
                            st.h0 = c.h0; st.w0 = c.w0; st.d0 = c.d0;
                        }
                    }
                }
            }
            const float fh = st.fh, fw = st.fw, fd = st.fd;
            // nested lerps: d, then w, then h; gradients in voxel units reuse the differences
            const float dd0 = v[1] - v[0], dd1 = v[3] - v[2], dd2 = v[5] - v[4], dd3 = v[7] - v[6];
            const float c0 = fmaf(fd, dd0, v[0]), c1 = fmaf(fd, dd1, v[2]);
            const float c2 = fmaf(fd, dd2, v[4]), c3 = fmaf(fd, dd3, v[6]);
            const float dw0 = c1 - c0, dw1 = c3 - c2;
            const float b0 = fmaf(fw, dw0, c0), b1 = fmaf(fw, dw1, c2);
            const float dh0 = b1 - b0;
            sdf = fmaf(fh, dh0, b0);
            gvw = fmaf(fh, dw1 - dw0, dw0);
            const float e0 = fmaf(fw, dd1 - dd0, dd0), e1 = fmaf(fw, dd3 - dd2, dd2);
            gvd = fmaf(fh, e1 - e0, e0);
            gvh = dh0;

            // NeuS alpha; cos = dir . grad_metres = sum_axis gv_axis * (dir_axis * slope_axis)
            const float cosv = fmaf(gvd, Gdd, fmaf(gvw, Gdw, gvh * Gdh));
            const float alpha = so_alpha_fast(sdf * s2, fminf(cosv, 0.0f) * hdt_s2);
            w = alpha * T;
            T = T * ((1.0f - alpha) + 1e-7f);
        }

        const float t_mid = fmaf(fi, dt, tnear + hdt);
        acc = acc + w;
        dsum = fmaf(w, t_mid, dsum);
        if (w > best_w) { best_w = w; best_t = t_mid; }

        if constexpr (NF > 0) {
            so_cell c;
            c.h0 = st.h0; c.w0 = st.w0; c.d0 = st.d0;
            float wk[8];
            const float fh = st.fh, fw = st.fw, fd = st.fd;
            const float fh0 = 1.0f - fh, fw0 = 1.0f - fw, fd0 = 1.0f - fd;
            const float ww0 = fw0 * fh0, ww1 = fw * fh0, ww2 = fw0 * fh, ww3 = fw * fh;
            wk[0] = fd0 * ww0; wk[1] = fd * ww0; wk[2] = fd0 * ww1; wk[3] = fd * ww1;
            wk[4] = fd0 * ww2; wk[5] = fd * ww2; wk[6] = fd0 * ww3; wk[7] = fd * ww3;
            float f[NF];
            bool done = false;
            if constexpr (STAGED) {
                if (st.boxed) {
                    so_gather_feat_staged<NF, BF16>(rf, a.feat_vol, H, W, D, st.h0, st.w0, st.d0, st.hmin, st.wmin,
                                                    st.dmin, wk, lds, lane, lane_vox, st.pref, st.blk,
                                                    st.all_interior, f);
                    done = true;
                }
            }
            if (!done) {
                if (st.all_interior) so_gather_feat_interior<NF, BF16>(rf, W, D, st.cell, wk, f);
                else so_gather_feat<NF, BF16>(a.feat_vol, H, W, D, c, wk, f);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float col = fmaxf(fmaf(0.28209479177387814f, f[k], 0.5f), 0.0f);
                rgb[k] = fmaf(w, col, rgb[k]);
            }
            if constexpr (NSEM > 0) {
                float m = f[3];
#pragma unroll
                for (int k = 1; k < NSEM; ++k) if (SO_SEM_ON(k)) m = fmaxf(m, f[3 + k]);
                float e[NSEM], den = 0.0f;
#pragma unroll
                for (int k = 0; k < NSEM; ++k) {
                    if (SO_SEM_ON(k)) {
                        e[k] = so_fast_exp2((f[3 + k] - m) * 1.44269504088896341f);
                        den = den + e[k];
                    } else {
                        e[k] = 0.0f;
                    }
                }
                const float wd = w * so_fast_rcp(den);
                if constexpr (SEM_LDS) {
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) sem_lds[k * 256] = fmaf(wd, e[k], sem_lds[k * 256]);      // lane-private slot
                } else {
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) sem[k] = fmaf(wd, e[k], sem[k]);
                }
            }
        }
    };

    // Light kernels (NF < 8) run a two-stage software pipeline with ping-pong register sets: the
    // global loads of step i + 1 are in flight while step i is interpolated and composited.  With
    // 24 feature channels the second register set spills (measured 12.5 ms vs 4.4 ms), so the
    // heavy kernels fetch and consume the same step.
    if constexpr (PIPE) {
        FastStep<NF> A, B;
        fetch(0, A);
        for (int i = 0;;) {
            if (i + 1 < S) fetch(i + 1, B);
            consume(i, A);
            if (++i >= S) break;
            if (so_all(T < 1e-10f)) break;
            if (i + 1 < S) fetch(i + 1, A);
            consume(i, B);
            if (++i >= S) break;
            if (so_all(T < 1e-10f)) break;
        }
    } else {
        for (int i = 0; i < S; ++i) {
            FastStep<NF> A;
            fetch(i, A);
            consume(i, A);
            if (so_all(T < 1e-10f)) break;
        }
    }

    const float eps32 = 1.1920928955078125e-07f;
    if (dt * inv_dn < eps32) best_t = tnear + hdt;  // degenerate ray: all w/delta == 0 -> index 0
    if (!store) return;
    float depth = dsum * so_fast_rcp(acc + 1e-10f);
    if (a.flags & SO_FLAG_DEPTH_DIV_NORM) depth = depth * inv_dn;
    if (a.depth) a.depth[ray] = depth;
    if (a.acc) a.acc[ray] = acc;
    if (a.max_depth) a.max_depth[ray] = best_t * inv_dn;
    if (a.nears) a.nears[ray] = tnear;
    if (a.fars) a.fars[ray] = tfar;
    if constexpr (NF > 0) {
        if (a.rgb) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float bg = 0.0f;
                if (a.bkgd_mode == SO_BKGD_CONST) bg = a.bkgd[k];
                else if (a.bkgd_mode == SO_BKGD_PER_RAY) bg = a.bkgd_rays[3 * (size_t)ray + k];
                float r = rgb[k];
                if (a.bkgd_mode != SO_BKGD_NONE) r = r + bg * (1.0f - acc);
                if (a.flags & SO_FLAG_CLAMP_RGB) r = fminf(fmaxf(r, 0.0f), 1.0f);
                a.rgb[3 * (size_t)ray + k] = r;
            }
        }
        if constexpr (NSEM > 0) {
            if (a.sem) {
#pragma unroll
                for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) a.sem[(size_t)ray * nsem + k] = SEM_LDS ? sem_lds[k * 256] : sem[k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// SDF-only per-ray launches with free-space skipping (the depth-evaluation path, bench.py).
// PMC of the general march on this workload: the vector-L1 path is the limiter (TA address FIFO full, waves
// parked in s_waitcnt), not the vector ALU — and a skipped step still fetched its corner records,
// because the skip code arrived together with it.  Here the skip code runs ONE step ahead of the records:
//     per step i:  decide skip(i) from code(i) (already here)
//                  position of step i + 1, issue its 1-byte code load
//                  only if not skipping: the two 16-byte record loads of step i, then interpolate + alpha
//                  composite
// A skipped step moves 1 byte per lane through the L1 instead of 33.  The general step is not software-pipelined beyond
// that: measurements showed it insensitive to load/compute overlap inside a wave (8 waves / SIMD hide it).  The one loop
// that is pipelined is low mode's (`low` below), whose steps know their successor's cell ten instructions into the trip.
//
// Free-space steps come in long runs (mean 33 steps at inv_s 20), and inside a run three tests of the general
// step have a known outcome, so a run loop (`run` below) composites the steps after a skipped one without them:
//   * the interior test: a lane's grid coordinate is monotone in the step index on every axis, so a wave that is interior
//     at steps lo and hi is interior at every step between; [i_lo, i_hi] is found once per wave with the test itself;
//   * the best-weight compare: T does not grow inside a run, so w = kAlphaFree * T does not exceed the run's first w;
//   * the exit test: see kRunExitFreeSteps.
// The same range splits the march into three phases: the steps before i_lo and from i_hi on run the general step, the steps
// between a copy of it compiled without the interior test, the all_interior flags and the range compares (the wave-uniform
// scalar work and branches of a step whose outcome is known there).
// What a lane computes at a step, and every wave-wide decision, is what the step-by-step form computes: same outputs, bit for bit.
// ---------------------------------------------------------------------------------------
// The exit: a wave leaves the march once no later step can change a bit of what it stores.
// so_march_fast leaves when every lane has T < 1e-10, "whatever comes adds less than 1e-10 to any output", which is far
// below what float32 registers: next to acc ~ 1 a weight under 2^-25 is already lost.  A lane is SPENT at the end of a step
// when every later step of its march leaves acc, dsum, best_w and best_t as they are, and the wave leaves when all its lanes
// are spent (or the old test holds, so the rule is a superset of the old one by construction).  With u = 2^-24, at the end
// of a step with the lane's T, acc, dsum, best_w, the lane is spent if
//     (a) T * 2^25 < acc,   (b) fl((T * 2^26) * tb) < |dsum|,   (c) T <= best_w,
// tb = max(|t_mid(0)|, |t_mid(S - 1)|).  The proof:
//   * T does not grow and stays >= 0.  A step multiplies T by fl(fl(1 - alpha) + 1e-7f).  so_alpha_fast never returns NaN
//     (its fminf's drop a NaN operand: a NaN corner or slope gives alpha ~ 1) and returns alpha in [~0.99e-5, 1]: eb >= ea up
//     to an ulp of v_exp_f32, so num >= 1e-5 p - 6e-8 and den = 1 + 1e-5 p, and the final fminf caps it.  A free step has
//     alpha = kAlphaFree ~ 1e-5.  Either way the factor lies in [1e-7, 1 - 9e-6]: below 1, so the rounded product is <= T,
//     and not negative.  Every later weight is w = fl(alpha * T') <= T' <= T, with T' the T of that later step.
//   * acc: (a) in real numbers is T < acc * 2^-25 (the scaling of T <= 1 by 2^25 is exact, for a subnormal T as well), and
//     acc * 2^-25 is less than half an ulp of acc (acc < 2^(e + 1), half an ulp is 2^(e - 24)).  So 0 <= w < ulp(acc) / 2 and
//     fl(acc + w) == acc.  (acc * 2^-25 rather than the exponent of acc: one multiply instead of an and / or pair, and it
//     costs at most a factor 2 of T, 0.7 of the ~17 e-foldings.)
//   * dsum: fma(w, t_mid, dsum) rounds dsum + w * t_mid once.  t_mid(fi) = fma(fi, dt, tnear + hdt) is monotone in fi
//     (dt > 0: so_collide makes tfar > tnear), so |t_mid| <= tb at every step, and |w * t_mid| <= T * tb.  T * 2^26 is exact
//     and the product with tb is rounded once, so (b) gives T * tb < |dsum| 2^-26 (1 + 2 u): half of |dsum| 2^-25, which is
//     itself under half an ulp of dsum; the factor 2 carries the rounding of the product and the case t_mid < 0 < dsum with
//     dsum a power of two, where the spacing below dsum is half the spacing above.  A product that underflows has
//     T * tb < 2^-152, which no fma registers.  (b) is false at dsum == 0.
//   * best weight: w <= T <= best_w, so `w > best_w` stays false and neither best_w nor best_t is written.
//     (In practice (b) is the condition that decides: dsum <= ~acc * tb makes it imply (a) with its factor 2 to spare, and
//     best_w >= acc / S makes (a) imply (c) for any S below 2^25.  (a) and (c) cost three instructions of the rare block and
//     keep the proof free of both estimates.)
//   * monotonicity: while (a) - (c) hold nothing on their right-hand sides changes and T only falls, so they hold at every
//     later step too: the induction goes through, and the test may be made at any step, or late.
//   * NaN or inf in acc, dsum, tb or best_w (T itself is finite, see above): a NaN makes its compare false, so the lane is
//     not spent and the wave stays; an infinite acc or dsum stays what it is under a finite addend.  The old test does not
//     look at them at all.
//   * Nothing stored reads T: depth, acc, max_depth come from acc, dsum, best_t; nears / fars from the collider.
// (a) needs T < acc * 2^-25 < 2^-24 = kSpentPre (acc < 2: it is 1 - T up to the 1e-7 per step that the factor adds), and
// 1e-10 < kSpentPre, so the hot path keeps ONE compare against one wave-uniform constant, `all lanes T < kSpentPre`, where it
// had `all lanes T < 1e-10`; (a) - (c) are evaluated, in a block laid out behind the loops, on the few closing steps of a wave
// at which that pre-test holds.  -DSO_NO_SPENT_EXIT builds the 1e-10 rule alone, for A/B runs.
//
// A run of n free steps multiplies T by ((1 - kAlphaFree) + 1e-7f) n times, each product rounded: by more than
// (1 - 1e-5)^n, which is > 0.54 for n <= 60 000 (a normal T: each rounding costs at most 1 - 2^-24), and adds n weights of at
// most kAlphaFree * T each to acc, 0.6 T in all, each sum rounded (at most 1 + 60 000 * 2^-24 < 1.004 in all).  Take a lane
// that enters a run of at most that many steps with T >= 2e-10 and T * 2^24 >= acc.  To its end T' >= 0.54 T > 1e-10, and
// acc' <= 1.004 (acc + 0.6 T) <= 1.004 (2^24 + 0.6) T < 0.54 * 2^25 T <= T' * 2^25: condition (a) fails, the lane is not
// spent.  Neither the old nor the new test can hold while the wave has such a lane, so the run needs no exit test.  (With
// acc < 2 every lane at or above 2 * kSpentPre is such a lane, and so are the lanes within a factor 2 above the level at
// which (a) begins to hold.  With SO_NO_SPENT_EXIT the lane is one with T >= 2e-10, as in the parent.)
constexpr int kRunExitFreeSteps = 60000;
#ifdef SO_NO_SPENT_EXIT
constexpr bool kSpentExit = false;
constexpr float kSpentPre = 1e-10f;
#else
constexpr bool kSpentExit = true;
constexpr float kSpentPre = 0x1p-24f;
#endif
constexpr int kSureScan = 8;   // steps tried from either end of the march for the sure-interior range
// Low mode of the sure loop (see `low` in so_march_fast_ahead); -DSO_NO_LOW_MODE builds the marcher without it, for A/B runs.
#ifdef SO_NO_LOW_MODE
constexpr bool kLowMode = false;
#else
constexpr bool kLowMode = true;
#endif
// Low mode loads the records of the next low step under the current one; -DSO_NO_LOW_PREFETCH builds the loop that loads a
// step's records at the top of its own trip, for A/B runs.
#ifdef SO_NO_LOW_PREFETCH
constexpr bool kLowPrefetch = false;
#else
constexpr bool kLowPrefetch = true;
#endif
// kLowC lies 15 * 2^-24 relative below kSkipArg * log2(e) = 25.2471632...: see the proof in `low`
constexpr float kLowC = 25.24714f;

struct AheadStep {
    float gh, gw, gd, fi;         // grid coordinates (the fractions are taken only by the steps that interpolate)
    int h0, w0, d0;
    unsigned cell, code;
    bool all_interior;            // wave-uniform; not kept by the steps inside the sure range
};

template <bool FACE_SAFE, class GeomFn>
SO_DEVFN void so_march_fast_ahead(const so_render_args &a, const so_launch_consts &c, int ray, GeomFn geom) {
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int S = a.n_samples;
    const RayGeom g = geom(a);
    // The unit direction, parked for the rare canonical-cell block (canon_cell) in a slot of LDS that only this lane writes
    // and reads (no barrier: the wave's own LDS operations complete in order).  3 KB per block; the kernel has no other LDS.
    __shared__ float s_dir[FACE_SAFE ? 3 * 256 : 1];
    int wave_slot = 0;                       // wave-uniform: the wave's first slot
    if constexpr (FACE_SAFE) {
        wave_slot = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
        s_dir[threadIdx.x] = g.dx; s_dir[256 + threadIdx.x] = g.dy; s_dir[512 + threadIdx.x] = g.dz;
    }
    float tnear, tfar;
    so_collide(a, g, tnear, tfar);
    // the launch's constants come from the host (so_launch_consts); what depends on the ray or on inv_s is computed here
    const float dt = (tfar - tnear) / c.n_samples_f;
    const float inv_dn = 1.0f / g.dn;
    const AxisK kh = c.kh, kw = c.kw, kd = c.kd;
    const float t_off = (a.sample_pos == SO_SAMPLE_AT_START) ? tnear : tnear + 0.5f * dt;
    const float Gdh = g.dy * kh.k1, Gdw = g.dx * kw.k1, Gdd = g.dz * kd.k1;
    const float G0h = fmaf(g.oy, kh.k1, kh.k0) + Gdh * t_off;
    const float G0w = fmaf(g.ox, kw.k1, kw.k0) + Gdw * t_off;
    const float G0d = fmaf(g.oz, kd.k1, kd.k0) + Gdd * t_off;
    const float s2 = so_inv_s(a) * 1.44269504088896341f;
    const float hdt = 0.5f * dt, hdt_s2 = hdt * s2;
    const float *__restrict__ vol = a.sdf_vol;
    const unsigned n_cells = c.n_cells, codes_off = c.codes_off, row_off = c.row_off;
    const __amdgpu_buffer_rsrc_t rb = so_make_rsrc(a.sdf_brick, (size_t)n_cells * 17);   // 16-B records, then the code bytes
    const __amdgpu_buffer_rsrc_t rs = so_make_rsrc(vol, (size_t)n_cells * 4);
    const int rcode = max((int)ceilf(dt / c.skip_unit), 1);
    const float face_m = c.face_m;

    float T = 1.0f, acc = 0.0f, dsum = 0.0f, best_w = -1.0f, best_t = 0.0f;
    bool low_hint_a = false, low_hint_b = false;     // wave-uniform: set by the two steps of the sure loop's body (low mode)
    const float low_thr = kLowC * so_fast_rcp(s2);   // low mode: a corner at or under it is under the brick pass's 17.5 / inv_s

    // The exit test of every loop (wave-uniform): see kSpentPre.  The bound on |t_mid| is made inside the rare block from
    // what the loops keep live anyway; nothing of the test stays in a register across a step.
    auto over_now = [&]() __attribute__((always_inline)) {
        if (__builtin_expect(!so_all(T < kSpentPre), 1)) return false;
        if constexpr (!kSpentExit) return true;
        // the last step's index through an operand the optimiser cannot see through: the bound is loop-invariant, and
        // hoisted in front of the loops it costs a VGPR across all of them
        int last = S - 1;
        asm volatile("" : "+s"(last));
        const float t_first = tnear + hdt;
        const float tb = fmaxf(fabsf(t_first), fabsf(fmaf((float)last, dt, t_first)));
        return so_all3(T * 0x1p25f < acc, (T * 0x1p26f) * tb < fabsf(dsum), T <= best_w) || so_all(T < 1e-10f);
    };

    // position and cell of step i
    auto place = [&](const int i, AheadStep &st) __attribute__((always_inline)) {
        st.fi = (float)i;
        const float step = st.fi * dt;
        const float gh = fmaf(Gdh, step, G0h), gw = fmaf(Gdw, step, G0w), gd = fmaf(Gdd, step, G0d);
        st.gh = gh; st.gw = gw; st.gd = gd;
        const int h0 = so_floor_i(gh), w0 = so_floor_i(gw), d0 = so_floor_i(gd);
        st.h0 = h0; st.w0 = w0; st.d0 = d0;
        st.cell = so_cell_index(h0, w0, d0, W, D);
    };
    auto interior = [&](const AheadStep &st) __attribute__((always_inline)) {   // wave-uniform
        return so_all3((unsigned)st.h0 < (unsigned)(H - 1), (unsigned)st.w0 < (unsigned)(W - 1), (unsigned)st.d0 < (unsigned)(D - 1));
    };
    // The steps [i_lo, i_hi] at which every lane of the wave is certainly interior: `interior` holds at both ends, hence
    // (monotone coordinates: fi * dt, the fma and the floor are each monotone in i) in between.  The ends are looked for
    // within kSureScan steps of the march's ends; a wave that has none there (rays that graze the volume) gets the empty
    // range and tests every step.
    int i_lo = S, i_hi = -1;
    {
        AheadStep p;
        const int n = min(kSureScan, S);
#pragma nounroll
        for (int k = 0; k < n; ++k) {
            place(k, p);
            if (interior(p)) { i_lo = k; break; }
        }
        if (i_lo < S) {
#pragma nounroll
            for (int k = S - 1; k >= S - n && k >= i_lo; --k) {
                place(k, p);
                if (interior(p)) { i_hi = k; break; }
            }
        }
        if (i_hi < 0) i_lo = S;
    }
    // Locate step i.  In the sure range (IN_SURE) the wave is interior without a test: the code load is unconditional and
    // st.all_interior is neither written nor read.  Outside it the interior test runs at every step (at i_lo and i_hi it is
    // the evaluation that found the range, so it is true there).
    auto locate = [&](const int i, AheadStep &st, auto in_sure) __attribute__((always_inline)) {
        place(i, st);
        if constexpr (decltype(in_sure)::value) {
            st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, st.cell, codes_off, 0);
        } else {
            st.all_interior = interior(st);
            st.code = 0u;
            if (st.all_interior) st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, st.cell, codes_off, 0);
        }
    };
    auto near_face = [&](float fh, float fw, float fd) __attribute__((always_inline)) {
        return fmaxf(fmaxf(fabsf(fh - 0.5f), fabsf(fw - 0.5f)), fabsf(fd - 0.5f)) > 0.5f - face_m;
    };
    // The sample's cell in the canonical order (see so_march_fast).  Only tnear / tfar stay live across the loop: the ray
    // and the mapping are re-derived inside this rare branch from launch arguments re-read from the kernarg segment
    // (so_reload_args) — otherwise the direction stays in VGPRs and every mapping / camera constant in SGPRs across the
    // march loop (71 VGPRs / 104 SGPRs: 7 waves / SIMD).  The phases are fenced off from one another so that only one
    // phase's constants are in SGPRs at a time.  The origin comes from geom(), the code that made the ray up front, and the
    // unit direction from the lane's LDS slot, where the prelude parked what geom() gave it (re-deriving it here cost the
    // camera-matrix loads, a sqrt and three divisions); the phases are so_locate's: the same values, bit for bit.
    auto canon_cell = [&](const int i) __attribute__((always_inline)) {
        RayGeom gc = geom(so_reload_args());     // the origin only: the direction's arithmetic is dead code
        {
            // the lane's slot, rebuilt here (mbcnt) from an operand the optimiser cannot see through, so that neither the lane
            // index nor an LDS address is computed ahead of the loops and kept in a register across them
            unsigned ones = ~0u;
            asm volatile("" : "+s"(ones));
            const unsigned lane = __builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
            const float *slot = s_dir + (wave_slot + lane);
            gc.dx = slot[0]; gc.dy = slot[256]; gc.dz = slot[512];
        }
        __builtin_amdgcn_sched_barrier(0);
        float px, py, pz;
        {
            const so_render_args ac = so_reload_args();
            const int n = ac.n_samples;
            const float b0 = so_bin(i, n);
            const float t_start = b0 * tfar + (1.0f - b0) * tnear;
            if (ac.sample_pos == SO_SAMPLE_AT_START) {
                px = gc.ox + gc.dx * t_start; py = gc.oy + gc.dy * t_start; pz = gc.oz + gc.dz * t_start;
            } else {
                const float b1 = so_bin(i + 1, n);
                const float tt = t_start + (b1 * tfar + (1.0f - b1) * tnear);
                px = gc.ox + (gc.dx * tt) / 2.0f; py = gc.oy + (gc.dy * tt) / 2.0f; pz = gc.oz + (gc.dz * tt) / 2.0f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float slope;
        // every launch that reaches this march has single-segment axes (so_fast_eligible: size1 == 0).  Saying so takes
        // so_axis_m2g's second segment out of the block: a per-lane branch, two divisions and two kernarg dwords per axis
        auto axis = [](so_axis A) __attribute__((always_inline)) { A.size1 = 0.0f; return A; };
        const float gh = so_grid_coord(so_axis_m2g(axis(so_reload_args().map.h), py, slope), so_reload_args().map.h.tot_len);
        __builtin_amdgcn_sched_barrier(0);
        const float gw = so_grid_coord(so_axis_m2g(axis(so_reload_args().map.w), px, slope), so_reload_args().map.w.tot_len);
        __builtin_amdgcn_sched_barrier(0);
        const float gd = so_grid_coord(so_axis_m2g(axis(so_reload_args().map.d), pz, slope), so_reload_args().map.d.tot_len);
        return so_cell_of(gh, gw, gd);
    };

    // Returns whether the step skipped (wave-uniform).  IN_SURE: steps i and i + 1 both lie in the sure range.
    auto step = [&](const int i, AheadStep &cur, AheadStep &nxt, auto in_sure, bool &hint) __attribute__((always_inline)) {
        constexpr bool IN_SURE = decltype(in_sure)::value;
        bool skip;
        if constexpr (IN_SURE) {
            const auto free_lanes = __builtin_amdgcn_ballot_w64((int)cur.code >= rcode);
            skip = free_lanes == __builtin_amdgcn_ballot_w64(true);
            // the hint that opens low mode (below): no lane of the step could skip.  Scalar work on the compare the step makes
            // anyway; a wrong hint costs one unproven low step, never a wrong result.
            if constexpr (kLowMode) hint = free_lanes == 0;
            locate(i + 1, nxt, in_sure);
        } else {
            skip = cur.all_interior && so_all((int)cur.code >= rcode);
            if (i + 1 < S) locate(i + 1, nxt, in_sure);
        }
        float w;
        if (skip) {
            w = kAlphaFree * T;
            T = T * ((1.0f - kAlphaFree) + 1e-7f);
        } else {
            float fh = __builtin_amdgcn_fractf(cur.gh), fw = __builtin_amdgcn_fractf(cur.gw), fd = __builtin_amdgcn_fractf(cur.gd);
            so_f32x2 p0, p1, p2, p3;
            auto gather = [&](int h0, int w0, int d0) __attribute__((always_inline)) {
                float v[8];
                so_gather_sdf_buf(rs, H, W, D, h0, w0, d0, v);
                p0 = so_f32x2{v[0], v[4]}; p1 = so_f32x2{v[1], v[5]}; p2 = so_f32x2{v[2], v[6]}; p3 = so_f32x2{v[3], v[7]};
            };
            // A step with no lane near a face (all but ~2 % of the interpolated wave-steps) falls through both
            // branches below, from the test to its record loads; the near-face block is marked unlikely and laid out behind the
            // loop body.  It is decided before any corner is loaded, so that no corner is live across the canonical
            // recomputation.  (With the record loads written into both arms of an if / else instead of behind the `moved_any`
            // flag the compiler keeps the flag, adds three register copies and a vmcnt(0) in front of the loads: 3.7 % slower.)
            bool moved_any = false;              // wave-uniform
            if (FACE_SAFE && __builtin_expect(__any(near_face(fh, fw, fd)), 0)) {
                int h0 = cur.h0, w0 = cur.w0, d0 = cur.d0;
                bool moved = false;
                if (near_face(fh, fw, fd)) {
                    const so_cell c = canon_cell(i);
                    moved = (c.h0 != h0) | (c.w0 != w0) | (c.d0 != d0);   // the canonical order lands next door
                    h0 = moved ? c.h0 : h0; w0 = moved ? c.w0 : w0; d0 = moved ? c.d0 : d0;
                    fh = moved ? c.fh1 : fh; fw = moved ? c.fw1 : fw; fd = moved ? c.fd1 : fd;
                }
                // a moved lane reads its new cell from the volume, the wave's other lanes the same corner values
                // there as in their brick records
                moved_any = __any(moved);
                if (moved_any) gather(h0, w0, d0);
            }
            if (__builtin_expect(!moved_any, 1)) {
                if (IN_SURE || cur.all_interior) {
                    {   // the records of cells (h, w, d) and (h, w + 1, d) = the four corner pairs, in the register order
                        // so_trilerp_fast_pk takes them
                        // (issuing these loads before locate() above, to run it under them, measured 9 % SLOWER)
                        const so_f4v lo = so_bload4(rb, cur.cell * 16u, 0u), hi = so_bload4(rb, cur.cell * 16u, row_off);
                        p0 = lo.xy; p1 = lo.zw; p2 = hi.xy; p3 = hi.zw;
                    }
                } else {
                    gather(cur.h0, cur.w0, cur.d0);
                }
            }
            float sdf, dh0, gvw, gvd;
            so_trilerp_fast_pk(p0, p1, p2, p3, fh, fw, fd, sdf, dh0, gvw, gvd);
            const float cosv = fmaf(gvd, Gdd, fmaf(gvw, Gdw, dh0 * Gdh));
            const float alpha = so_alpha_fast(sdf * s2, fminf(cosv, 0.0f) * hdt_s2);
            w = alpha * T;
            T = T * ((1.0f - alpha) + 1e-7f);
        }
        const float t_mid = fmaf(cur.fi, dt, tnear + hdt);
        acc = acc + w;
        dsum = fmaf(w, t_mid, dsum);
        if (w > best_w) { best_w = w; best_t = t_mid; }
        return skip;
    };

    // Low mode of the sure loop.  Interpolated steps come in long stretches that hug a surface, and in most of them some lane's
    // cell has a corner under the saturation level 17.5 / inv_s, where the brick pass gives code 0 (its `slack > 0` fails):
    // the wave cannot skip, and the code byte loaded for the step could only say so.  A low step is located without the code
    // load (place), loads its records, and PROVES from them that the parent interpolated it; a step it cannot prove loads
    // its code after all, takes the parent's decision and hands back to the sure loop.  A proven step is two vector-memory
    // instructions instead of three and a few vector and scalar instructions shorter than a sure step (no code compare, one
    // loop); what a lane composites is what step() composites, in the same order.  
    //   The proof: some lane's corner v0 = lo.x is at or under low_thr = fl(kLowC * rcp(s2)).  The brick pass gives code 0
    // unless the cell's smallest corner m exceeds q = fl(17.5 / inv_s), and m <= v0.  With u = 2^-24: v_rcp_f32 is good to one
    // ulp, so low_thr <= (kLowC / s2) (1 + 2 u) (1 + u); s2 = fl(inv_s * fl(log2 e)) >= inv_s log2 e (1 - u)^2; and
    // q >= (17.5 / inv_s) (1 - u).  Hence v0 <= low_thr implies v0 <= q whenever kLowC <= 17.5 log2 e (1 - 6 u - O(u^2)), and
    // kLowC lies 15 u below 17.5 log2 e.  Edge cases agree with the brick pass: inv_s <= 0 gives every cell code 0, whatever is
    // claimed; a NaN corner or a NaN inv_s compares false, not proven; an infinite s2 gives low_thr = 0 against q = 0; an s2 so
    // small that rcp or the product overflows gives low_thr = inf where q is infinite or the slack NaN as well.  No division:
    // inv_s may live on the device alone, and tests/test_render_prelude_cpu.py pins the kernel's division count.
    // (The 8-corner minimum proves 95.5 % of the bench frame's interpolated wave-steps against 94.0 % for v0 alone and costs 4
    // more vector instructions per step: measured slower.  The interpolated sdf proves nothing: a rounded nested lerp can
    // undershoot m.)
    //   On entry `st` holds step i, placed (its code is not looked at), i_lo <= i.  Steps i with i + 1 < i_hi only, so that
    // the sure loop finds the range's end the way it always does.  A step with a lane near a face goes back to the sure loop
    // untouched: the canonical-cell block exists once, there.  On return `st` is the located step i, code included, unless
    // the march is over (returns true).
    auto low = [&](int &i, AheadStep &st) __attribute__((always_inline)) {
        // One loop, one exit: every reason to leave is folded into `go` (a loop with several exits gets an exit number from
        // the compiler, made in a VGPR and read back with v_readfirstlane on every trip).  The next step's near-face test is
        // taken at the end of a trip, for the same reason.
        //   The loop is software-pipelined.  A trip used to issue its two record loads first and wait
        // for them nine instructions later: one vector-L1 round trip per step with nothing of the wave's own under it.  Now a
        // trip places step i + 1 first and issues ITS records into a second register set, then interpolates step i from the
        // set the trip before loaded: every pair has a whole trip to arrive.  The loads of step i + 1 are unconditional; a
        // trip runs only with i + 1 < i_hi, so the cell is an interior one of the sure range whatever becomes of the step.
        // -DSO_NO_LOW_PREFETCH builds the loop that loads a step's records in its own trip.
        struct so_f3 { float h, w, d; };
        using so_f3r = so_f3 &;
        auto fractions = [&]() __attribute__((always_inline)) {
            return so_f3{__builtin_amdgcn_fractf(st.gh), __builtin_amdgcn_fractf(st.gw), __builtin_amdgcn_fractf(st.gd)};
        };
        so_f3 f0 = fractions(), f1;
        bool coded = false;                  // st.code is on its way
        bool go = i + 1 < i_hi && !(FACE_SAFE && __any(near_face(f0.h, f0.w, f0.d)));
        // One trip: step i from its records (lo, hi); with kLowPrefetch the records of step i + 1 are issued into (nlo, nhi)
        // as soon as its cell is placed, ahead of the first use of (lo, hi).
        auto trip = [&](so_f4v &lo, so_f4v &hi, so_f4v &nlo, so_f4v &nhi, so_f3r f, so_f3r nf) __attribute__((always_inline)) {
            if constexpr (!kLowPrefetch) { lo = so_bload4(rb, st.cell * 16u, 0u); hi = so_bload4(rb, st.cell * 16u, row_off); }
            float t_mid = fmaf(st.fi, dt, tnear + hdt);
            asm volatile("" : "+v"(t_mid));      // here, while st.fi is the step's: computed later it keeps a copy of st.fi alive
            ++i;
            place(i, st);
            if constexpr (kLowPrefetch) {
                // i <= i_hi - 1 here: an interior cell of the sure range, whatever becomes of the step
                nlo = so_bload4(rb, st.cell * 16u, 0u); nhi = so_bload4(rb, st.cell * 16u, row_off);
                __builtin_amdgcn_sched_barrier(0);      // the scheduler otherwise sinks the pair under this step's arithmetic
                nf = fractions();                       // here: the coordinates need not outlive the loads (see the exit)
            }
            const bool proven = __any(lo.x <= low_thr);
            float sdf, dh0, gvw, gvd;
            so_trilerp_fast_pk(lo.xy, lo.zw, hi.xy, hi.zw, f.h, f.w, f.d, sdf, dh0, gvw, gvd);
            const float cosv = fmaf(gvd, Gdd, fmaf(gvw, Gdw, dh0 * Gdh));
            float alpha = so_alpha_fast(sdf * s2, fminf(cosv, 0.0f) * hdt_s2);
            if (__builtin_expect(!proven, 0)) {
                // the parent's decision, from the code of the step (its cell placed once more: the hot path keeps only the
                // next step's) and with the next step's code on its way
                AheadStep was;
                place(i - 1, was);
                const unsigned code = __builtin_amdgcn_raw_buffer_load_b8(rb, was.cell, codes_off, 0);
                unsigned next_cell = st.cell;
                if constexpr (kLowPrefetch) {       // placed once more as well: the hot path keeps no cell past its loads
                    int ia = i;
                    asm volatile("" : "+s"(ia));
                    AheadStep now;
                    place(ia, now);
                    next_cell = now.cell;
                }
                st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, next_cell, codes_off, 0);
                if (so_all((int)code >= rcode)) alpha = kAlphaFree;    // skipped: the constant alpha, as step() composites it
                coded = true;
            }
            const float w = alpha * T;
            T = T * ((1.0f - alpha) + 1e-7f);
            acc = acc + w;
            dsum = fmaf(w, t_mid, dsum);
            if (w > best_w) { best_w = w; best_t = t_mid; }
            if constexpr (!kLowPrefetch) nf = fractions();
            go = !coded && !over_now() && i + 1 < i_hi && !(FACE_SAFE && __any(near_face(nf.h, nf.w, nf.d)));
        };
        so_f4v lo0, hi0, lo1, hi1;
        if constexpr (kLowPrefetch) {
            // The body twice, the two record sets ping-ponged: no register copies, and the wait in front of a trip's first
            // use is a counted one that leaves the younger pair in flight.  One exit test per half, both to the same place;
            // the pair in flight at the exit is dropped (the sure loop loads the step's records itself if it interpolates).
            if (go) {
                lo0 = so_bload4(rb, st.cell * 16u, 0u); hi0 = so_bload4(rb, st.cell * 16u, row_off);
#pragma nounroll
                for (;;) {
                    trip(lo0, hi0, lo1, hi1, f0, f1);
                    if (!go) break;
                    trip(lo1, hi1, lo0, hi0, f1, f0);
                    if (!go) break;
                }
                // `st` is step i's again from its index alone (an operand the optimiser cannot see through): nothing of a
                // placed step but its cell and fi stays in a register across a trip, and the two halves need no copies
                int ii = i;
                asm volatile("" : "+s"(ii));
                place(ii, st);
            }
        } else {
#pragma nounroll
            while (go) trip(lo0, hi0, lo1, hi1, f0, f0);
        }
        if (over_now()) return true;   // false on entry: the caller has just tested it
        if (!coded) st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, st.cell, codes_off, 0);
        return false;
    };

    // The run loop, entered from the sure loop only.  On entry step i - 1 skipped and passed the exit test, `st` holds step
    // i, located, and i_lo <= i <= i_hi.  It composites steps i, i + 1, ... while they skip and the step after them is inside
    // the sure range (so that `st`, re-located in place after each decision, needs no interior test), then hands `st` = the
    // located step i back to the caller.  Returns true when the march is over.
    auto run = [&](int &i, AheadStep &st) __attribute__((always_inline)) {
        auto free_step = [&]() __attribute__((always_inline)) {
            const float t_mid = fmaf(st.fi, dt, tnear + hdt);
            ++i;
            place(i, st);
            st.code = __builtin_amdgcn_raw_buffer_load_b8(rb, st.cell, codes_off, 0);
            const float w = kAlphaFree * T;
            T = T * ((1.0f - kAlphaFree) + 1e-7f);
            acc = acc + w;
            dsum = fmaf(w, t_mid, dsum);
        };
        // some lane keeps the wave's exit test false: kRunExitFreeSteps
        const bool kept = kSpentExit ? (__builtin_amdgcn_ballot_w64(T * 0x1p24f >= acc) & __builtin_amdgcn_ballot_w64(T >= 2e-10f)) != 0
                                     : !so_all(T < 2e-10f);
        if (S <= kRunExitFreeSteps && kept) {
            while (i < i_hi && so_all((int)st.code >= rcode)) free_step();
        } else {
            while (i < i_hi && so_all((int)st.code >= rcode)) {
                free_step();
                if (over_now()) return true;
            }
        }
        return false;
    };

    // Three phases.  Head, steps [0, i_lo), and tail, steps [i_hi, S): the general step, which tests the interior at every
    // step; at most kSureScan steps each, so they run as a rolled loop that moves the located step back (A = B) instead of
    // ping-ponging.  A wave without a sure range has i_lo = S and marches in the head loop alone.  Between them the sure loop,
    // steps i with i_lo <= i and i + 1 <= i_hi: no interior test, no all_interior flag, no range compare, the record loads
    // on the brick path; the located steps ping-pong between A and B, and skipped steps continue in the run loop.  Whichever
    // loop composites a step, the lane computes what the general step computes.
    // (Head and tail as ONE loop around the sure loop, 15.0 KB instead of 19.0 KB of code, needs 71 VGPRs instead of 63: what
    // either loop keeps in registers is then live across both.  DESIGN 3.1, round 10.)
    {
        constexpr std::false_type general{};
        constexpr std::true_type in_sure{};
        AheadStep A, B;
        locate(0, A, general);
        int i = 0;
        bool over = false, unused_hint = false;
        auto gen = [&](int end) __attribute__((always_inline)) {
#pragma nounroll
            while (i < end) {
                step(i, A, B, general, unused_hint);
                if (++i >= S || over_now()) { over = true; break; }
                A = B;
            }
        };
        gen(i_lo);
        if (!over) {
            while (i < i_hi) {
                const bool sa = step(i, A, B, in_sure, low_hint_a);
                ++i;
                if (over_now() || (sa && run(i, B))) { over = true; break; }
                if (i >= i_hi) { A = B; break; }        // the tail takes its located step from A
                const bool sb = step(i, B, A, in_sure, low_hint_b);
                ++i;
                if (over_now() || (sb && run(i, A))) { over = true; break; }
                // Low mode opens here only, on A, so that the loop has one copy of it, and after two steps in a row in which
                // no lane could skip (the hint of step()).  A low step that the code skipped hands the skipping step back,
                // and the step above takes it to the run loop.
                if constexpr (kLowMode) {
                    if (low_hint_a && low_hint_b && low(i, A)) { over = true; break; }
                }
            }
            if (!over) { A.all_interior = true; gen(S); }
        }
    }

    const float eps32 = 1.1920928955078125e-07f;
    if (dt * inv_dn < eps32) best_t = tnear + hdt;
    float depth = dsum * so_fast_rcp(acc + 1e-10f);
    if (a.flags & SO_FLAG_DEPTH_DIV_NORM) depth = depth * inv_dn;
    if (a.depth) a.depth[ray] = depth;
    if (a.acc) a.acc[ray] = acc;
    if (a.max_depth) a.max_depth[ray] = best_t * inv_dn;
    if (a.nears) a.nears[ray] = tnear;
    if (a.fars) a.fars[ray] = tfar;
}

// The march a kernel runs: a compile-time choice of the dispatch below.
enum class March {
    Canonical,          // so_march_exact: the oracle's operation order (SO_FLAG_EXACT, jitter, two-segment axes)
    Fast,               // so_march_fast
    FastFaceSafe,       // so_march_fast with canonical cell selection near voxel faces
    Skip,               // so_march_fast_ahead, the code-ahead skip marcher (SDF-only launches with brick + skip codes)
    SkipFaceSafe,       // so_march_fast_ahead with canonical cell selection near voxel faces
    CanonicalUpscale,   // so_march_exact under the 'linear_upscale' mapping (g(t) is not affine: no fast path, no brick, no skip)
};
constexpr bool so_is_fast(March m) { return m == March::Fast || m == March::FastFaceSafe; }
constexpr bool so_is_skip(March m) { return m == March::Skip || m == March::SkipFaceSafe; }
constexpr bool so_face_safe(March m) { return m == March::FastFaceSafe || m == March::SkipFaceSafe; }
// the fast march with the wave's voxel neighbourhood staged in LDS (so_gather_feat_staged): pixel-grid launches only
template <class ROW>
constexpr bool so_is_staged(March m) { return so_is_fast(m) && !ROW::BF16 && ROW::NF >= 4; }

// a spherical-harmonics row has the canonical marches only; the skip marchers have kernels of their own (so_launch_consts)
template <class ROW, March MODE, class GeomFn>
SO_DEVFN void so_march(const so_render_args &a, int ray, GeomFn geom) {
    static_assert(!so_is_skip(MODE), "skip marcher: the kernels that take so_launch_consts");
    if constexpr (MODE == March::CanonicalUpscale) {
        so_march_exact<ROW, SO_MAP_UPSCALE>(a, ray, geom(a));
    } else if constexpr (so_is_fast(MODE)) {
        so_march_fast<ROW, false, so_face_safe(MODE)>(a, ray, geom);
    } else {
        so_march_exact<ROW, SO_MAP_LINEAR>(a, ray, geom(a));
    }
}


// re-pack of the SDF volume for the fast path.  record[cell(h, w, d)] = (v[h][w][d], v[h + 1][w][d], v[h][w][d + 1], v[h + 1][w][d + 1]),
// 16 bytes: the (h = 0, h = 1) corner pairs of so_trilerp_fast_pk at w = 0.  The pairs at w = 1 are the record of cell
// (h, w + 1, d), D records further on, so a cell's 8 corners are two 16-B loads and no corner is stored twice along w.
// Indices are clamped at the upper faces (only interior cells are ever read).  After the records, codes[cell] = the
// free-space skip code of the cell (see so_skip_unit), 0 when skipping is off.
// A thread owns a cell: threadIdx.x = d, threadIdx.y = w within the block's columns, blockIdx.x = h, so no index is divided
// and a wave stores 64 consecutive records.  (A thread per 4 d-cells with float4 row loads measured slower, 13.2 us against
// the 10.9 us of the 32-byte pass: its record stores were 64 bytes apart from lane to lane.)  With D % 4 == 0 (uniform) the
// 4 code bytes of an aligned quad of lanes leave as one dword.
__global__ __launch_bounds__(256) void sdf_brickify_kernel(const float *__restrict__ vol, float *__restrict__ brick,
                                                           int H, int W, int D, so_render_args a, int with_codes,
                                                           so_launch_consts c) {
    const int h = blockIdx.x, h1 = min(h + 1, H - 1);
    const size_t n_cells = (size_t)H * W * D;
    uint8_t *codes = (uint8_t *)(brick + n_cells * 4);
    // blockDim.x is a power of two: with D % 4 == 0 the lanes 4 q .. 4 q + 3 of a wave hold 4 consecutive cells of one column
    const bool quads = (D & 3) == 0 && (blockDim.x & 3) == 0;
    const float kd = c.kd.k1, kw = c.kw.k1, kh = c.kh.k1;      // size0 / range0 of each axis, from the host
    for (int w = blockIdx.y * blockDim.y + threadIdx.y; w < W; w += gridDim.y * blockDim.y) {
        const int w1 = min(w + 1, W - 1);
        const float *r00 = vol + ((size_t)h * W + w) * D, *r01 = vol + ((size_t)h * W + w1) * D;
        const float *r10 = vol + ((size_t)h1 * W + w) * D, *r11 = vol + ((size_t)h1 * W + w1) * D;
        for (int d = threadIdx.x; d < D; d += blockDim.x) {
            const int d1 = min(d + 1, D - 1);
            const float v0 = r00[d], v1 = r00[d1], v2 = r01[d], v3 = r01[d1];
            const float v4 = r10[d], v5 = r10[d1], v6 = r11[d], v7 = r11[d1];
            const size_t cell = ((size_t)h * W + w) * D + d;
            ((float4 *)brick)[cell] = make_float4(v0, v4, v1, v5);
            unsigned code = 0u;
            if (with_codes) {
                const float m = fminf(fminf(fminf(v0, v1), fminf(v2, v3)), fminf(fminf(v4, v5), fminf(v6, v7)));
                // per-axis bound of the metre gradient anywhere in the cell: the partial derivative of a trilinear
                // function is a bilinear blend of the 4 edge differences along that axis
                const float gd = fmaxf(fmaxf(fabsf(v1 - v0), fabsf(v3 - v2)), fmaxf(fabsf(v5 - v4), fabsf(v7 - v6))) * kd;
                const float gw = fmaxf(fmaxf(fabsf(v2 - v0), fabsf(v3 - v1)), fmaxf(fabsf(v6 - v4), fabsf(v7 - v5))) * kw;
                const float gh = fmaxf(fmaxf(fabsf(v4 - v0), fabsf(v5 - v1)), fmaxf(fabsf(v6 - v2), fabsf(v7 - v3))) * kh;
                const float G = sqrtf((gd * gd + gw * gw) + gh * gh) * 1.001f + 1e-20f;
                const float slack = m - kSkipArg / so_inv_s(a);                       // metres above the saturation level
                if (slack > 0.0f && so_inv_s(a) > 0.0f) {
                    const float allow = 2.0f * slack / G / c.skip_unit;   // in code units
                    code = (unsigned)fminf(floorf(allow * 0.999f), 255.0f);
                }
            }
            if (quads) {
                // the codes of the lane's quad (quad_perm broadcasts of its lanes 1, 2, 3), stored by its lane 0
                const unsigned c1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)code, 0x55, 0xf, 0xf, false);
                const unsigned c2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)code, 0xaa, 0xf, 0xf, false);
                const unsigned c3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)code, 0xff, 0xf, 0xf, false);
                if ((d & 3) == 0) *(unsigned *)(codes + cell) = code | (c1 << 8) | (c2 << 16) | (c3 << 24);
            } else {
                codes[cell] = (uint8_t)code;
            }
        }
    }
}

// pixel-grid rays: a block is a 16x16 pixel tile of one camera, each of its four waves an 8x8 sub-tile
struct TilePixel { int cam, ix, iy, wave, lane; };
SO_DEVFN TilePixel so_tile_pixel(int tiles_x, int tiles_y) {
    const int b = blockIdx.x;
    const int cam = b / (tiles_x * tiles_y);
    const int tb = b - cam * tiles_x * tiles_y;
    const int ty = tb / tiles_x, tx = tb - ty * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    return {cam, tx * 16 + (wave & 1) * 8 + (lane & 7), ty * 16 + (wave >> 1) * 8 + (lane >> 3), wave, lane};
}

// The feature-carrying kernels of the degree-0 rows ask for 2 waves / SIMD.
template <class ROW>
constexpr int so_min_blocks() { return (ROW::NB == 0 && ROW::NF >= 8) ? 2 : 1; }

// explicit rays: one ray per thread, linear order
template <class ROW, March MODE>
__global__ __launch_bounds__(256, so_min_blocks<ROW>()) void render_fwd_explicit(so_render_args a) {
    int ray = blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= a.n_rays) return;
    auto geom = [&](const so_render_args &a) __attribute__((always_inline)) { return so_explicit_ray(a, ray); };
    so_march<ROW, MODE>(a, ray, geom);
}

template <class ROW, March MODE>
SO_DEVFN void pixgrid_body(const so_render_args &a, int tiles_x, int tiles_y) {
    const TilePixel p = so_tile_pixel(tiles_x, tiles_y);
    const int cam = p.cam, wave = p.wave, lane = p.lane;
    int ix = p.ix, iy = p.iy;
    if constexpr (so_is_staged<ROW>(MODE)) {
        // every lane keeps marching (the LDS staging is a whole-wave operation): lanes beyond the
        // lattice edge shadow the nearest real pixel and only skip the final store
        constexpr int NF = ROW::NF;
        __shared__ __attribute__((aligned(16))) float s_stage[4 * StageGeom<NF>::kWaveDwords];
        const bool real = (ix < a.nx) && (iy < a.ny);
        ix = min(ix, a.nx - 1); iy = min(iy, a.ny - 1);
        int ray = (cam * a.ny + iy) * a.nx + ix;
        auto geom = [&](const so_render_args &a) __attribute__((always_inline)) { return so_pixel_ray(a, cam, ix, iy); };
        constexpr int NSEM_LDS = NF - 3 >= 16 ? NF - 3 : 0;          // so_march_fast::SEM_LDS
        __shared__ float s_sem[NSEM_LDS > 0 ? NSEM_LDS * 256 : 1];
        so_march_fast<ROW, true, so_face_safe(MODE)>(a, ray, geom, real, s_stage + wave * StageGeom<NF>::kWaveDwords, lane,
                                                     s_sem + threadIdx.x);
    } else {
        if (ix >= a.nx || iy >= a.ny) return;
        int ray = (cam * a.ny + iy) * a.nx + ix;
        auto geom = [&](const so_render_args &a) __attribute__((always_inline)) { return so_pixel_ray(a, cam, ix, iy); };
        so_march<ROW, MODE>(a, ray, geom);
    }
}

template <class ROW, March MODE>
__global__ __launch_bounds__(256, so_min_blocks<ROW>()) void render_fwd_pixgrid(so_render_args a, int tiles_x, int tiles_y) {
    if constexpr (ROW::NB > 0) {
        // A spherical-harmonics row keeps the spelling its kernels shipped with: the pixel map written out and the ray passed
        // by value.  Through pixgrid_body the compiler commutes the operands of one scalar multiply and one add in these six
        // kernels (the same instructions in another order); this way all of them stay the code they were.
        const int b = blockIdx.x;
        const int cam = b / (tiles_x * tiles_y);
        const int tb = b - cam * tiles_x * tiles_y;
        const int ty = tb / tiles_x, tx = tb - ty * tiles_x;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int ix = tx * 16 + (wave & 1) * 8 + (lane & 7);
        const int iy = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
        if (ix >= a.nx || iy >= a.ny) return;
        const int ray = (cam * a.ny + iy) * a.nx + ix;
        so_march_exact<ROW, MODE == March::CanonicalUpscale ? SO_MAP_UPSCALE : SO_MAP_LINEAR>(a, ray, so_pixel_ray(a, cam, ix, iy));
    } else {
        pixgrid_body<ROW, MODE>(a, tiles_x, tiles_y);
    }
}

// The skip marchers: overloads of the two kernel templates that take the launch's constants from the host.  `a` stays the
// first argument, at the start of the kernarg segment, where so_reload_args reads it.
template <class ROW, March MODE>
__global__ __launch_bounds__(256, 1) void render_fwd_explicit(so_render_args a, so_launch_consts c) {
    static_assert(so_is_skip(MODE) && ROW::NF == 0 && ROW::NB == 0, "skip marcher: SDF-only launches");
    int ray = blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= a.n_rays) return;
    auto geom = [&](const so_render_args &a) __attribute__((always_inline)) { return so_explicit_ray(a, ray); };
    so_march_fast_ahead<so_face_safe(MODE)>(a, c, ray, geom);
}
// Pixel grid (bench.py's kernel): launched on a 3-D grid, so the block reads its tile and camera from blockIdx where
// so_tile_pixel divides the linear index twice (two v_rcp_iflag -> v_readfirstlane round trips in front of any ray work).
// The grid is (tiles_x, n_cams, tiles_y): blocks are dispatched x fastest, then the camera, then the tile row, so tile row r
// of every camera runs before row r + 1 of any.  The cameras of a rig share their vertical layout — rays that leave through
// the walls or the ceiling at the top (long free runs, cheap waves), rays that meet the ground below (long interpolated
// stretches, waves three times as dear) — so the waves resident together are of one kind and the launch passes from
// one kind to the other once, where the camera-by-camera order does it once per camera.  Measured:
// 1.2 % faster at inv_s 20 and 10 % at inv_s 200; mixing the kinds on purpose (rows alternately from the two ends of the
// image) is 4 % SLOWER.  With one camera the order is the linear one.  Which ray goes to which lane of which wave does not
// depend on the order: a wave is the same 8 x 8 tile.  -DSO_NO_ROW_ORDER builds the grid (tiles_x, tiles_y, n_cams), the
// camera-by-camera order, for A/B runs.
#ifdef SO_NO_ROW_ORDER
constexpr bool kRowsOutermost = false;
#else
constexpr bool kRowsOutermost = true;
#endif
// At 8 waves / SIMD the kernel needs <= 64 VGPRs AND <= 80 SGPRs: a CU admits
// floor(800 / (ceil(sgpr / 16) * 16 + 16)) blocks of 256 threads, 7 at 82 - 96 SGPRs although the compiler's occupancy says 8.
// Left alone the allocator spends 84 (constants the rare canonical branch needs, hoisted); capped it fits in 80 without spilling.
template <class ROW, March MODE>
__global__ __launch_bounds__(256, 1) __attribute__((amdgpu_num_sgpr(80))) void render_fwd_pixgrid(so_render_args a, so_launch_consts c) {
    static_assert(so_is_skip(MODE) && ROW::NF == 0 && ROW::NB == 0, "skip marcher: SDF-only launches");
    const int cam = kRowsOutermost ? blockIdx.y : blockIdx.z, row = kRowsOutermost ? blockIdx.z : blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ix = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), iy = row * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (ix >= a.nx || iy >= a.ny) return;
    const int ray = (cam * a.ny + iy) * a.nx + ix;
    auto geom = [&](const so_render_args &a) __attribute__((always_inline)) { return so_pixel_ray(a, cam, ix, iy); };
    so_march_fast_ahead<so_face_safe(MODE)>(a, c, ray, geom);
}
// gridDim.y and gridDim.z end at 65 535
bool so_skip_grid_fits(const so_render_args &a) {
    return a.ray_mode == SO_RAYS_EXPLICIT || ((a.ny + 15) / 16 <= 65535 && a.n_cams <= 65535);
}

template <class ROW, March MODE>
int launch_fwd(const so_render_args &a, hipStream_t st) {
    const int tiles_x = (a.nx + 15) / 16, tiles_y = (a.ny + 15) / 16;
    if constexpr (so_is_skip(MODE)) {
        const so_launch_consts c = so_make_launch_consts(a);
        if (a.ray_mode == SO_RAYS_EXPLICIT) {
            hipLaunchKernelGGL((render_fwd_explicit<ROW, MODE>), dim3((a.n_rays + 255) / 256), dim3(256), 0, st, a, c);
        } else {
            const dim3 grid = kRowsOutermost ? dim3(tiles_x, a.n_cams, tiles_y) : dim3(tiles_x, tiles_y, a.n_cams);
            hipLaunchKernelGGL((render_fwd_pixgrid<ROW, MODE>), grid, dim3(256), 0, st, a, c);
        }
    } else if (a.ray_mode == SO_RAYS_EXPLICIT) {
        int blocks = (a.n_rays + 255) / 256;
        hipLaunchKernelGGL((render_fwd_explicit<ROW, MODE>), dim3(blocks), dim3(256), 0, st, a);
    } else {
        int blocks = tiles_x * tiles_y * a.n_cams;
        hipLaunchKernelGGL((render_fwd_pixgrid<ROW, MODE>), dim3(blocks), dim3(256), 0, st, a, tiles_x, tiles_y);
    }
    return so_launch_status();
}

// the fast march's re-pack of the SDF volume (sdf_brickify_kernel)
void so_launch_brickify(const so_render_args &a, hipStream_t st, int with_codes) {
    // threadIdx.x = d (a power of two of them), threadIdx.y = w; blockIdx.x = h
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    int qx = 1;
    while (qx < D && qx < 256) qx *= 2;
    const int wy = 256 / qx;
    hipLaunchKernelGGL(sdf_brickify_kernel, dim3(H, min((W + wy - 1) / wy, 65535)), dim3(qx, wy), 0, st, a.sdf_vol, a.sdf_brick,
                       H, W, D, a, with_codes, so_make_launch_consts(a));
}

// the fast march needs g(t) affine in t (no jitter, single-segment axes, the linear mapping kind) and so_cell_index's 24 bits
bool so_fast_eligible(const so_render_args &a) {
    return !(a.flags & SO_FLAG_EXACT) && a.jitter_mode == SO_JITTER_NONE && a.map.kind == SO_MAP_LINEAR &&
           a.map.h.size1 == 0.0f && a.map.w.size1 == 0.0f && a.map.d.size1 == 0.0f &&
           (long long)a.map.h.tot_len * a.map.w.tot_len < (1 << 24) && a.map.d.tot_len < (1 << 24);
}

// the march of a launch without per-sample outputs.  Built per row: the degree-0 unmasked rows have every march, the masked
// rows are always face-safe (SO_FLAG_NO_FACE_SAFE, an A/B switch of the shipped widths, is ignored), the spherical-harmonics
// rows march canonically.
// (SO_FLAG_RAY_PER_LANE, the A/B route of rounds 2 - 4 through ray-per-lane per-sample kernels, is accepted and ignored
// since ABI v30: 48 instantiations nobody shipped)
template <class ROW, int MK>
int dispatch(const so_render_args &a, hipStream_t st) {
    // 'linear_upscale': the canonical march with the upscale mapping (no brick re-pack, no skip codes)
    if constexpr (MK == SO_MAP_UPSCALE) return launch_fwd<ROW, March::CanonicalUpscale>(a, st);
    else if constexpr (ROW::NB > 0) return launch_fwd<ROW, March::Canonical>(a, st);
    else {
        if (!so_fast_eligible(a)) return launch_fwd<ROW, March::Canonical>(a, st);
        constexpr bool CAN_SKIP = ROW::NF == 0;
        if (a.sdf_brick) so_launch_brickify(a, st, (CAN_SKIP && !(a.flags & SO_FLAG_NO_SKIP)) ? 1 : 0);
        const bool face_safe = ROW::MASKED || !(a.flags & SO_FLAG_NO_FACE_SAFE);
        if constexpr (CAN_SKIP) {
            // a lattice too tall or with too many cameras for the skip marcher's 3-D grid takes the step-by-step march
            if (a.sdf_brick && !(a.flags & (SO_FLAG_NO_SKIP | SO_FLAG_NO_AHEAD)) && so_skip_grid_fits(a))
                return face_safe ? launch_fwd<ROW, March::SkipFaceSafe>(a, st) : launch_fwd<ROW, March::Skip>(a, st);
        }
        if constexpr (!ROW::MASKED) {
            if (!face_safe) return launch_fwd<ROW, March::Fast>(a, st);
        }
        return launch_fwd<ROW, March::FastFaceSafe>(a, st);
    }
}

}  // namespace

int so_validate_mapping(const so_mapping &m) {
    SO_REQUIRE(m.kind == SO_MAP_LINEAR || m.kind == SO_MAP_UPSCALE, "mapping: unknown kind %d (0 = linear, 1 = linear_upscale)",
               (int)m.kind);
    const so_axis *ax[3] = {&m.h, &m.w, &m.d};
    const so_upscale_axis *ux[3] = {&m.uh, &m.uw, &m.ud};
    for (int i = 0; i < 3; ++i) {
        SO_REQUIRE(ax[i]->tot_len >= 2, "mapping axis %d: tot_len must be >= 2", i);
        SO_REQUIRE(ax[i]->size0 > 0 && ax[i]->range0 > 0, "mapping axis %d: size0/range0 must be > 0", i);
        if (m.kind == SO_MAP_LINEAR) {
            SO_REQUIRE(ax[i]->size1 == 0 || ax[i]->range1 > 0, "mapping axis %d: range1 must be > 0", i);
        } else {
            // the reference divides by increase_unit and takes sqrt(c^2 + 2 o / increase_unit): both need it > 0,
            // and increase_unit = (range_outer - outer * unit) * 2 / outer / (outer + 1) needs outer >= 1
            SO_REQUIRE(ax[i]->size1 >= 1, "linear_upscale axis %d: outer cells must be >= 1 (got %g)", i, (double)ax[i]->size1);
            SO_REQUIRE(ux[i]->unit > 0 && __builtin_isfinite(ux[i]->unit), "linear_upscale axis %d: unit must be > 0 (got %g)", i,
                       (double)ux[i]->unit);
            SO_REQUIRE(ux[i]->inc > 0 && __builtin_isfinite(ux[i]->inc),
                       "linear_upscale axis %d: increase unit must be > 0 (got %g): the outer range must exceed outer * unit",
                       i, (double)ux[i]->inc);
        }
    }
    return 0;
}

namespace {
template <int MK>
__global__ __launch_bounds__(256) void meter2grid_kernel(so_mapping m, const float *__restrict__ xyz, int n, int normalize,
                                                         float *__restrict__ hwd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gh, gw, gd, sh, sw, sd;
    so_m2g<MK>(m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], gh, gw, gd, sh, sw, sd);
    if (normalize) {
        gh = gh / (float)(m.h.tot_len - 1); gw = gw / (float)(m.w.tot_len - 1); gd = gd / (float)(m.d.tot_len - 1);
    }
    hwd[3 * (size_t)i] = gh; hwd[3 * (size_t)i + 1] = gw; hwd[3 * (size_t)i + 2] = gd;
}
}  // namespace

extern "C" int selfocc_meter2grid(const so_mapping *map, const float *xyz, int n, int normalize, float *hwd, void *stream) {
    SO_REQUIRE(map != nullptr, "map is NULL");
    if (so_validate_mapping(*map)) return -1;
    SO_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return 0;
    SO_REQUIRE(xyz != nullptr && hwd != nullptr, "xyz / hwd is NULL");
    const dim3 grid((unsigned)((n + 255) / 256));
    if (map->kind == SO_MAP_UPSCALE)
        hipLaunchKernelGGL(meter2grid_kernel<SO_MAP_UPSCALE>, grid, dim3(256), 0, (hipStream_t)stream, *map, xyz, n, normalize, hwd);
    else
        hipLaunchKernelGGL(meter2grid_kernel<SO_MAP_LINEAR>, grid, dim3(256), 0, (hipStream_t)stream, *map, xyz, n, normalize, hwd);
    return so_launch_status();
}

int so_validate_render(const so_render_args &a) {
    if (so_validate_mapping(a.map)) return -1;
    SO_REQUIRE(a.sdf_vol != nullptr, "sdf_vol is NULL");
    SO_REQUIRE(a.n_samples >= 1, "n_samples must be >= 1");
    SO_REQUIRE(a.n_rays >= 0, "n_rays must be >= 0");
    SO_REQUIRE(a.n_rgb == 0 || a.n_rgb == 3, "n_rgb must be 0 or 3 (the colour outputs; sh_deg sets the coefficient count)");
    SO_REQUIRE(a.n_sem >= 0, "n_sem must be >= 0");
    SO_REQUIRE(a.n_sem == 0 || a.n_rgb == 3, "semantic channels require n_rgb == 3");
    SO_REQUIRE(a.sh_deg >= 0 && a.sh_deg <= 2, "sh_deg %d is not built (built: sh_deg 0, 1, 2)", (int)a.sh_deg);
    SO_REQUIRE(a.sh_act == SO_SH_RELU || a.sh_act == SO_SH_SIGMOID, "sh_act %d is unknown (0 = relu, 1 = sigmoid)", (int)a.sh_act);
    if (a.n_rgb + a.n_sem > 0) {
        SO_REQUIRE(a.feat_vol != nullptr, "feat_vol is NULL but n_rgb + n_sem > 0");
        SO_REQUIRE(a.feat_dtype == SO_DTYPE_F32 || a.feat_dtype == SO_DTYPE_BF16, "bad feat_dtype");
        SO_REQUIRE(a.feat_stride % 4 == 0 && a.feat_stride >= a.n_rgb + a.n_sem,
                   "feat_stride must be a multiple of 4 and >= n_rgb + n_sem");
    }
    if (so_sh_launch(a)) {
        const int n_coef = 3 * (a.sh_deg + 1) * (a.sh_deg + 1);
        SO_REQUIRE(a.n_sem == 0, "sh_deg > 0 / sh_act = sigmoid with n_sem = %d semantic channels is not built (built: n_sem = 0)",
                   (int)a.n_sem);
        SO_REQUIRE(a.feat_dtype == SO_DTYPE_F32, "sh_deg > 0 / sh_act = sigmoid with a bfloat16 feature volume is not built (built: float32)");
        SO_REQUIRE(a.feat_stride == so_sh_stride(n_coef / 3), "sh_deg = %d reads %d coefficients: feat_stride must be %d (got %d)",
                   (int)a.sh_deg, n_coef, so_sh_stride(n_coef / 3), (int)a.feat_stride);
    }
    if (a.n_sem > 0 && !so_sh_launch(a)) {   // rows [r, g, b, logit_0 .. logit_{n_sem - 1}, pad]: n_sem = 2 .. 21
        const int stride = so_row_width(a.n_sem);
        SO_REQUIRE(a.n_sem != 1, "n_sem = 1 is not built (built: n_sem 0 and 2 .. 21): one class renders `acc`");
        SO_REQUIRE(a.n_sem <= 21, "n_sem = %d is not built (built: n_sem 0 and 2 .. 21): the binned backward record and the "
                   "32-lanes-per-sample brick kernel end at 24 channels", (int)a.n_sem);
        SO_REQUIRE(a.feat_stride == stride, "n_sem = %d semantic channels: feat_stride must be %d = 3 + n_sem rounded up to 4 (got %d)",
                   (int)a.n_sem, stride, (int)a.feat_stride);
        SO_REQUIRE(a.feat_dtype == SO_DTYPE_F32 || a.n_sem == 21, "bfloat16 feature volumes with semantic channels are built for "
                   "n_sem = 21, feat_stride = 24 only (got n_sem = %d)", (int)a.n_sem);
    }
    if (a.ray_mode == SO_RAYS_EXPLICIT) {
        SO_REQUIRE(a.n_rays == 0 || (a.origins && a.dirs), "explicit rays need origins and dirs");
    } else if (a.ray_mode == SO_RAYS_PIXEL_GRID) {
        SO_REQUIRE(a.img2lidar != nullptr, "pixel-grid rays need img2lidar");
        SO_REQUIRE(a.n_cams >= 0 && a.nx >= 0 && a.ny >= 0, "bad pixel grid");
        SO_REQUIRE((int64_t)a.n_cams * a.nx * a.ny == a.n_rays, "n_rays != n_cams * ny * nx");
    } else {
        SO_REQUIRE(false, "bad ray_mode %d", a.ray_mode);
    }
    SO_REQUIRE(a.jitter_mode >= SO_JITTER_NONE && a.jitter_mode <= SO_JITTER_EDGES, "bad jitter_mode %d", (int)a.jitter_mode);
    SO_REQUIRE(a.jitter_mode == SO_JITTER_NONE || a.t_rand, "jitter or explicit edges requested but t_rand is NULL");
    SO_REQUIRE(a.bkgd_mode != SO_BKGD_PER_RAY || a.bkgd_rays, "per-ray background but bkgd_rays is NULL");
    SO_REQUIRE(a.sample_pos == SO_SAMPLE_AT_START || a.sample_pos == SO_SAMPLE_AT_MID, "bad sample_pos");
    return 0;
}

extern "C" int selfocc_render_fwd(const so_render_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_render_args &a = *args;
    if (so_validate_render(a)) return -1;
    if (a.n_rays == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    // training API: the sample-parallel kernels of render_train.hip (a lane per sample, canonical arithmetic)
    if (a.weights || a.ts || a.deltas || a.sdf || a.grad) return so_render_fwd_samples(a, st);
    return so_with_row_and_map(a, [&](auto row, auto mk) { return dispatch<decltype(row), decltype(mk)::value>(a, st); });
}
