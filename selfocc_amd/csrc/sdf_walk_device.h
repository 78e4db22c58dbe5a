// sdf_walk_device.h — the one-ray-per-lane canonical SDF march that reproduces the per-sample `weights` of selfocc_render_fwd
// BIT FOR BIT, for the geometry-only outputs that are defined from those weights: render_median.hip (median depth) and
// render_normal.hip (rendered normal).  An output is a policy struct OUT:
//
//   struct OUT {                     // an aggregate of the output pointers and nothing else
//       struct state {               // one ray's accumulators, in registers
//           state(const so_render_args &a);
//           bool visit(const RayGeom &g, const so_walk_sample &s);     // sample s of the ray; true = the ray is finished
//           void store(const OUT &out, int ray) const;
//       };
//   };
//
// and so_walk_launch<OUT>(a, stream, the pointers) runs render_walk_kernel<mapping kind, OUT> over the rays of `a`.  Geometry only (SDF volume,
// no colour / semantic row), so one kernel per mapping kind serves every head.
//
// Canonical arithmetic (so_device.h / ray_device.h: the operation sequence of so_march_exact).  The loop ends for a wave when
// every lane's `visit` has returned true or the samples are used up.
//
// The transmittance.  The per-sample weights come from the sample-parallel kernel (render_train.hip), where T_i is an
// exclusive prefix PRODUCT over lanes: a 6-step Hillis-Steele scan inside each 64-sample wave segment, the segment totals
// multiplied in order, a carry across passes of 64 * WPR samples.  Float multiplication is not associative, so a lane that
// simply multiplied T along its ray would get weights a few 1e-7 off (and, on a few rays in 1e5, another median sample).  The
// lane therefore replays that scan's product TREE for its own ray: level k of the scan combines a value with the level-k value
// 2^k samples back, so the lane keeps the last 2^k values of every level (1 + 2 + .. + 32 = 63 registers, shifted by one per
// sample) and does the same six multiplications per sample the scan does.  No LDS, no cross-lane traffic.  If render_train.hip
// changes its scan, this file follows; nothing else has to.
#pragma once
#include "ray_device.h"

// what a ray's consumer sees of sample i: the middle of its bin (metres along the ray), its weight and its SDF gradient
struct so_walk_sample {
    int i;
    float t_mid, w, gx, gy, gz;
};

// one level of the scan for one sample: q = the level-K value of sample l, h[2^K - 1 ..] = the level-K values of the 2^K
// samples before it (newest first).  Returns the level-(K + 1) value: render_train.hip's `if (lane >= m) incl = incl * up`.
template <int K>
SO_DEVFN float so_scan_level(float q, float (&h)[63], int l) {
    constexpr int M = 1 << K, O = M - 1;
    const float old = h[O + M - 1];
#pragma unroll
    for (int j = M - 1; j > 0; --j) h[O + j] = h[O + j - 1];
    h[O] = q;
    return l >= M ? q * old : q;
}

template <int MK, class Visit>
SO_DEVFN void so_walk_ray(const so_render_args &a, int ray, const RayGeom &g, Visit visit) {
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int S = a.n_samples;
    const int seg_per_pass = S <= 64 ? 1 : (S <= 128 ? 2 : 4);      // render_train.hip: waves per ray
    const float inv_s = so_inv_s(a);
    float tnear, tfar;
    so_collide(a, g, tnear, tfar);

    float h[63];
#pragma unroll
    for (int k = 0; k < 63; ++k) h[k] = 1.0f;
    float carry = 1.0f, before = 1.0f, excl = 1.0f;    // transmittance entering the pass / the segment / the sample
    int l = 0, seg = 0;
    bool stop = false;

    float t_end = so_edge(a, ray, 0, tnear, tfar);
    for (int i = 0; i < S && !stop; ++i) {
        const float t_start = t_end;
        t_end = so_edge(a, ray, i + 1, tnear, tfar);
        const float delta = t_end - t_start;
        so_walk_sample s;
        s.i = i;
        s.t_mid = (t_start + t_end) / 2.0f;
        float px, py, pz;
        so_sample_point(a, g, t_start, t_end, px, py, pz);
        const so_cell cell = so_locate_k<MK>(a.map, px, py, pz);
        float v[8], wk[8];
        so_gather_sdf(a.sdf_vol, H, W, D, cell, v);
        const float sdf = so_trilerp_sdf(cell, v, wk);
        so_trilerp_grad(cell, v, s.gx, s.gy, s.gz);
        const float alpha = so_neus_alpha(g, sdf, s.gx, s.gy, s.gz, delta, inv_s);
        const float fstep = (1.0f - alpha) + 1e-7f;

        const float T = (carry * before) * excl;
        s.w = alpha * T;
        stop = visit(s);

        // the scan's inclusive product of this segment up to sample l: the transmittance factor of the next sample
        float q = fstep;
        q = so_scan_level<0>(q, h, l);
        q = so_scan_level<1>(q, h, l);
        q = so_scan_level<2>(q, h, l);
        q = so_scan_level<3>(q, h, l);
        q = so_scan_level<4>(q, h, l);
        q = so_scan_level<5>(q, h, l);
        excl = q;
        if (++l == 64) {                      // segment total: into `before`; at the end of a pass into `carry`
            l = 0;
            excl = 1.0f;
            before = before * q;
            if (++seg == seg_per_pass) { seg = 0; carry = carry * before; before = 1.0f; }
        }
    }
}

// P...: the members of OUT, the output pointers, as kernel arguments of their own.  With OUT itself as the argument the
// rendered normal measured 0.04 ms (0.7 %) slower than the kernel it replaces; with the pointers apart most of that is gone
// (DESIGN.md section 3.23).
template <int MK, class OUT, class... P>
__global__ __launch_bounds__(256) void render_walk_kernel(so_render_args a, P __restrict__... p, int tiles_x, int tiles_y) {
    const OUT out{p...};
    int ray;
    if (a.ray_mode == SO_RAYS_PIXEL_GRID) {
        // a block owns a 16 x 16 pixel tile of one camera, a wave an 8 x 8 quarter of it: the 64 gathers of a march step
        // fall into a handful of neighbouring cells
        const int per_cam = tiles_x * tiles_y;
        const int cam = blockIdx.x / per_cam, t = blockIdx.x - cam * per_cam;
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int ix = tx * 16 + (wave & 1) * 8 + (lane & 7), iy = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
        if (ix >= a.nx || iy >= a.ny) return;
        ray = (cam * a.ny + iy) * a.nx + ix;
    } else {
        ray = blockIdx.x * 256 + threadIdx.x;
        if (ray >= a.n_rays) return;
    }
    const RayGeom g = so_ray_of(a, ray);
    typename OUT::state st(a);
    so_walk_ray<MK>(a, ray, g, [&](const so_walk_sample &s) { return st.visit(g, s); });
    st.store(out, ray);
}

// the launch of an `a` that so_validate_render accepted, with n_rays > 0; p...: the members of OUT, in order
template <class OUT, class... P>
int so_walk_launch(const so_render_args &a, hipStream_t st, P... p) {
    int blocks, tiles_x = 0, tiles_y = 0;
    if (a.ray_mode == SO_RAYS_PIXEL_GRID) {
        tiles_x = (a.nx + 15) / 16; tiles_y = (a.ny + 15) / 16;
        blocks = tiles_x * tiles_y * a.n_cams;
    } else {
        blocks = (a.n_rays + 255) / 256;
    }
    if (a.map.kind == SO_MAP_UPSCALE)
        hipLaunchKernelGGL((render_walk_kernel<SO_MAP_UPSCALE, OUT, P...>), dim3(blocks), dim3(256), 0, st, a, p..., tiles_x, tiles_y);
    else
        hipLaunchKernelGGL((render_walk_kernel<SO_MAP_LINEAR, OUT, P...>), dim3(blocks), dim3(256), 0, st, a, p..., tiles_x, tiles_y);
    return so_launch_status();
}
