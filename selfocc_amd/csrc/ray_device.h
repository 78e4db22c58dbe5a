// ray_device.h — the ray geometry of the render kernels: ONE definition for render_fwd.hip (per-ray march), render_train.hip
// (sample-parallel forward), render_bwd.hip (backward + its counting pre-pass), render_median.hip and render_upsample.hip.
//
// Ray construction, the box collider and the bin edges decide which voxel cell a sample lands in, so the three translation
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

// 64-lane butterfly sums, every lane gets the total.  Two orders, named for the lane distances they pair: float addition is
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
