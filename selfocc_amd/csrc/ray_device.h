// ray_device.h — the ray geometry of the render kernels: ONE definition for render_fwd.hip (per-ray march), render_train.hip
// (sample-parallel forward), render_bwd.hip (backward + its counting pre-pass), render_upsample.hip and, through
// sdf_walk_device.h, render_median.hip and render_normal.hip.
//
// Ray construction, the box collider and the bin edges decide which voxel cell a sample lands in, so the translation
// units must agree on them operation for operation, and with oracle/oracle_render.c (-ffp-contract=off, every
// rounding spelled out).  A one-ulp difference gives a gradient for another cell than the forward used.
#pragma once
#include "so_device.h"

struct RayGeom {
    float ox, oy, oz, dx, dy, dz, dn;
};

// explicit rays: origin, unit direction and the norm the direction was divided by (1 when not given)
SO_DEVFN RayGeom so_explicit_ray(const so_render_args &a, int ray) {
    RayGeom g;
    g.ox = a.origins[3 * (size_t)ray]; g.oy = a.origins[3 * (size_t)ray + 1]; g.oz = a.origins[3 * (size_t)ray + 2];
    g.dx = a.dirs[3 * (size_t)ray]; g.dy = a.dirs[3 * (size_t)ray + 1]; g.dz = a.dirs[3 * (size_t)ray + 2];
    g.dn = a.dir_norm ? a.dir_norm[ray] : 1.0f;
    return g;
}

// the ray of a linear ray index under either ray_mode.  Pixel grid: RaySampler 'fixed' / 'cellular' lattice
// (ray_sampler.py:23-31, 58-68) and Img2LiDAR.forward (img2lidar.py:58-69): origin = M[:3,3], dir = M[:3,:3] (u,v,1).
// The camera matrix is read with plain loads: the camera differs between the lanes of a wave here.  Kernels whose camera is
// block-uniform use so_pixel_ray (render_fwd.hip), the same arithmetic on scalar loads.
SO_DEVFN RayGeom so_ray_of(const so_render_args &a, int ray) {
    if (a.ray_mode == SO_RAYS_PIXEL_GRID) {
        const int per_cam = a.nx * a.ny;
        const int cam = ray / per_cam, rem = ray - cam * per_cam;
        const int iy = rem / a.nx, ix = rem - iy * a.nx;
        const float *M = a.img2lidar + cam * 16;
        const float u = (float)ix * a.sx + a.ox;
        const float v = (float)iy * a.sy + a.oy;
        RayGeom g;
        g.ox = M[3]; g.oy = M[7]; g.oz = M[11];
        const float dx = (M[0] * u + M[1] * v) + M[2];
        const float dy = (M[4] * u + M[5] * v) + M[6];
        const float dz = (M[8] * u + M[9] * v) + M[10];
        g.dn = sqrtf((dx * dx + dy * dy) + dz * dz);  // neus_head.py:326
        g.dx = dx / g.dn; g.dy = dy / g.dn; g.dz = dz / g.dn;
        return g;
    }
    return so_explicit_ray(a, ray);
}

// AABBBoxCollider (sdfstudio / nerfstudio scene_colliders, upstream)
SO_DEVFN void so_collide(const so_render_args &a, const RayGeom &g, float &tnear, float &tfar) {
    const float fx = 1.0f / (g.dx + 1e-6f), fy = 1.0f / (g.dy + 1e-6f), fz = 1.0f / (g.dz + 1e-6f);
    const float t1 = (a.aabb[0] - g.ox) * fx, t2 = (a.aabb[3] - g.ox) * fx;
    const float t3 = (a.aabb[1] - g.oy) * fy, t4 = (a.aabb[4] - g.oy) * fy;
    const float t5 = (a.aabb[2] - g.oz) * fz, t6 = (a.aabb[5] - g.oz) * fz;
    tnear = fmaxf(fmaxf(fminf(t1, t2), fminf(t3, t4)), fminf(t5, t6));
    tfar = fminf(fminf(fmaxf(t1, t2), fmaxf(t3, t4)), fmaxf(t5, t6));
    tnear = fmaxf(tnear, a.near_plane);
    tfar = fmaxf(tfar, tnear + 1e-6f);
}

// torch.linspace(0, 1, n + 1)[j] in float32 (ATen RangeFactories: symmetric halves)
SO_DEVFN float so_bin(int j, int n) {
    const float step = 1.0f / (float)n;
    return (j < (n + 1) / 2) ? step * (float)j : fmaf(-step, (float)(n - j), 1.0f);
}

// normalised bin edge j of a ray, in [0, 1]: UniformSampler (spaced sampler, train_stratified jitter optional), or, with
// SO_JITTER_EDGES, the caller's own edge read back from t_rand (n_rays, n_samples + 1) (render_upsample.hip writes such rows)
SO_DEVFN float so_edge_unit(const so_render_args &a, int ray, int j) {
    const int n = a.n_samples;
    if (a.jitter_mode == SO_JITTER_EDGES) return a.t_rand[(size_t)ray * (n + 1) + j];
    float b = so_bin(j, n);
    if (a.jitter_mode != SO_JITTER_NONE) {
        const float lo = (j == 0) ? b : (b + so_bin(j - 1, n)) / 2.0f;
        const float hi = (j == n) ? b : (so_bin(j + 1, n) + b) / 2.0f;
        const float tr = (a.jitter_mode == SO_JITTER_SINGLE) ? a.t_rand[ray] : a.t_rand[(size_t)ray * (n + 1) + j];
        b = lo + (hi - lo) * tr;
    }
    return b;
}

// metric position of a normalised edge, everywhere
SO_DEVFN float so_edge_metric(float b, float tnear, float tfar) { return b * tfar + (1.0f - b) * tnear; }

// bin edge j of a ray in metres along it
SO_DEVFN float so_edge(const so_render_args &a, int ray, int j, float tnear, float tfar) {
    return so_edge_metric(so_edge_unit(a, ray, j), tnear, tfar);
}

// ---- the canonical per-sample arithmetic ------------------------------------------------
// so_sample_point and so_neus_alpha are the sample of so_march_exact (render_fwd.hip) and so_walk_ray (sdf_walk_device.h).
// render_train.hip and render_bwd.hip (sample_cell) spell the same operations out in their own bodies and must agree with
// these two, operation for operation.  They are NOT rewritten on top of them: the substitution was tried and compared with
// scripts/kernel_isa_diff.py, and it changed the generated code of 73 of render_train.hip's 81 kernels and of 33 of
// render_bwd.hip's 230.  The training hot path does not move for a tidier source.

// position of the sample of the bin [t_start, t_end]: its start, or its middle (so_render_args::sample_pos)
SO_DEVFN void so_sample_point(const so_render_args &a, const RayGeom &g, float t_start, float t_end, float &px, float &py, float &pz) {
    if (a.sample_pos == SO_SAMPLE_AT_START) {
        px = g.ox + g.dx * t_start; py = g.oy + g.dy * t_start; pz = g.oz + g.dz * t_start;
    } else {
        const float tt = t_start + t_end;
        px = g.ox + (g.dx * tt) / 2.0f; py = g.oy + (g.dy * tt) / 2.0f; pz = g.oz + (g.dz * tt) / 2.0f;
    }
}

// NeuS alpha (sdfstudio NeuS get_alpha, cos anneal ratio 1) of a sample with value `sdf`, gradient (gx, gy, gz) and bin length
// `delta`, clamped to [0, 1]
SO_DEVFN float so_neus_alpha(const RayGeom &g, float sdf, float gx, float gy, float gz, float delta, float inv_s) {
    const float cosv = (g.dx * gx + g.dy * gy) + g.dz * gz;
    const float icos = fminf(cosv, 0.0f);
    const float half = (icos * delta) * 0.5f;
    const float prev_cdf = so_sigmoid((sdf - half) * inv_s);
    const float next_cdf = so_sigmoid((sdf + half) * inv_s);
    const float alpha = ((prev_cdf - next_cdf) + 1e-5f) / (prev_cdf + 1e-5f);
    return fminf(fmaxf(alpha, 0.0f), 1.0f);
}

// ---- host side: what every entry point that embeds an so_render_args shares ------------------
// the checks of selfocc_render_fwd on the struct (render_fwd.hip); 0 when it is accepted, else the error is set
int so_validate_render(const so_render_args &a);

// The struct as a geometry-only entry point (render_median / render_normal / render_upsample) reads it: SDF volume, mapping,
// rays and sampling.  The feature fields, the colour basis, the background, the flags, every output pointer and the brick are
// ignored, whatever they hold; what is left goes through so_validate_render.
static inline so_render_args so_geometry_only(so_render_args a) {
    a.feat_vol = nullptr;
    a.feat_dtype = SO_DTYPE_F32; a.feat_stride = 0; a.n_rgb = 0; a.n_sem = 0;
    a.sh_deg = 0; a.sh_act = SO_SH_RELU;
    a.bkgd_mode = SO_BKGD_NONE; a.bkgd_rays = nullptr;
    a.flags = 0;
    a.depth = a.acc = a.rgb = a.sem = a.max_depth = a.nears = a.fars = nullptr;
    a.weights = a.ts = a.deltas = a.sdf = a.grad = nullptr;
    a.sdf_brick = nullptr;
    return a;
}

// 64-lane butterfly sums, every lane gets the total. Two orders, named for the lane distances they pair: float addition is
// not associative, and render_train.hip (1, 2, .. 32) and render_bwd.hip (32, 16, .. 1) each keep the order they shipped with.
SO_DEVFN float so_wave_sum_1to32(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}
SO_DEVFN float so_wave_sum_32to1(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
