// render_normal.hip — the rendered surface normal of the SDF ray march (selfocc_render_normal): sdfstudio's `normal_vis`, the
// `vis_normal` of the reference's render dicts (neus_head.py:358, 379, 414, 463), read by the vis_* scripts.
//
//   r_i = sqrtf((gx*gx + gy*gy) + gz*gz);   d_i = fmaxf(r_i, 1e-12f);   n_i = (gx / d_i, gy / d_i, gz / d_i)
//   N = 0;  for i = 0 .. S - 1:  N = N + w_i * n_i        (multiply, then add: no fused multiply-add)
//   normal_vis = (N + 1.0f) / 2.0f
//
// with w_i / (gx, gy, gz)_i the per-sample `weights` / `grad` of selfocc_render_fwd, BIT FOR BIT: the result is defined from
// those numbers, so a caller that holds the per-sample tensors and one that asks this kernel get
// the same pixel.  `grad` is what so_trilerp_grad returns for the sample's cell (render_train.hip writes it unchanged).
//
// A kernel of its own behind an entry point of its own, built like render_median.hip: nothing that exists is touched.
// Geometry only (SDF volume, no colour / semantic row), so one kernel per mapping kind serves every head.
//
// One ray per lane, canonical arithmetic (so_device.h / ray_device.h: the operation sequence of so_march_exact), every ray
// marches all S samples.  N depends on every w_i, and behind a surface a w_i under the replayed tree is small, not an exact
// zero (each step factor carries + 1e-7f; T is an exact 0 only once the product underflows), so there is no early exit.
//
// The transmittance is the sample-parallel kernel's (render_train.hip): an exclusive prefix PRODUCT over lanes, a 6-step
// Hillis-Steele scan inside each 64-sample wave segment, the segment totals multiplied in order, a carry across passes of
// 64 * WPR samples.  The lane replays that scan's product TREE for its own ray, as render_median.hip does (see there): the
// last 2^k values of every level k (63 registers, shifted by one per sample), the same six multiplications per sample.
#include "ray_device.h"

// render_fwd.hip
int so_validate_render(const so_render_args &a);

namespace {

// one level of the scan for one sample (render_median.hip: the same ten lines): q = the level-K value of sample l,
// h[2^K - 1 ..] = the level-K values of the 2^K samples before it (newest first).  Returns the level-(K + 1) value:
// render_train.hip's `if (lane >= m) incl = incl * up`.
template <int K>
SO_DEVFN float so_scan_level(float q, float (&h)[63], int l) {
    constexpr int M = 1 << K, O = M - 1;
    const float old = h[O + M - 1];
#pragma unroll
    for (int j = M - 1; j > 0; --j) h[O + j] = h[O + j - 1];
    h[O] = q;
    return l >= M ? q * old : q;
}

template <int MK>
__global__ __launch_bounds__(256) void render_normal_kernel(so_render_args a, float *__restrict__ normal_vis, int tiles_x, int tiles_y) {
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
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    int l = 0, seg = 0;

    float t_end = so_edge(a, ray, 0, tnear, tfar);
    for (int i = 0; i < S; ++i) {
        const float t_start = t_end;
        t_end = so_edge(a, ray, i + 1, tnear, tfar);
        const float delta = t_end - t_start;
        float px, py, pz;
        if (a.sample_pos == SO_SAMPLE_AT_START) {
            px = g.ox + g.dx * t_start; py = g.oy + g.dy * t_start; pz = g.oz + g.dz * t_start;
        } else {
            const float tt = t_start + t_end;
            px = g.ox + (g.dx * tt) / 2.0f; py = g.oy + (g.dy * tt) / 2.0f; pz = g.oz + (g.dz * tt) / 2.0f;
        }
        const so_cell cell = so_locate_k<MK>(a.map, px, py, pz);
        float v[8], wk[8];
        so_gather_sdf(a.sdf_vol, H, W, D, cell, v);
        const float sdf = so_trilerp_sdf(cell, v, wk);
        float gx, gy, gz;
        so_trilerp_grad(cell, v, gx, gy, gz);
        // NeuS alpha (sdfstudio NeuS get_alpha, cos anneal ratio 1), canonical order
        const float cosv = (g.dx * gx + g.dy * gy) + g.dz * gz;
        const float icos = fminf(cosv, 0.0f);
        const float half = (icos * delta) * 0.5f;
        const float prev_cdf = so_sigmoid((sdf - half) * inv_s);
        const float next_cdf = so_sigmoid((sdf + half) * inv_s);
        float alpha = ((prev_cdf - next_cdf) + 1e-5f) / (prev_cdf + 1e-5f);
        alpha = fminf(fmaxf(alpha, 0.0f), 1.0f);
        const float fstep = (1.0f - alpha) + 1e-7f;

        const float T = (carry * before) * excl;
        const float w = alpha * T;
        // F.normalize(grad, p=2, eps=1e-12), weighted into the ray's sum
        const float r = sqrtf((gx * gx + gy * gy) + gz * gz);
        const float d = fmaxf(r, 1e-12f);
        nx = nx + w * (gx / d);
        ny = ny + w * (gy / d);
        nz = nz + w * (gz / d);

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
    float *o = normal_vis + 3 * (size_t)ray;
    o[0] = (nx + 1.0f) / 2.0f;
    o[1] = (ny + 1.0f) / 2.0f;
    o[2] = (nz + 1.0f) / 2.0f;
}

template <int MK>
int launch_normal(const so_render_args &a, float *nv, hipStream_t st) {
    int blocks, tiles_x = 0, tiles_y = 0;
    if (a.ray_mode == SO_RAYS_PIXEL_GRID) {
        tiles_x = (a.nx + 15) / 16; tiles_y = (a.ny + 15) / 16;
        blocks = tiles_x * tiles_y * a.n_cams;
    } else {
        blocks = (a.n_rays + 255) / 256;
    }
    hipLaunchKernelGGL(render_normal_kernel<MK>, dim3(blocks), dim3(256), 0, st, a, nv, tiles_x, tiles_y);
    return so_launch_status();
}

}  // namespace

extern "C" int selfocc_render_normal(const so_render_normal_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    SO_REQUIRE(args->normal_vis != nullptr, "normal_vis is NULL: nothing to compute");
    so_render_args a = args->fwd;
    SO_REQUIRE(a.n_samples >= 1, "n_samples must be >= 1 (got %d)", (int)a.n_samples);
    SO_REQUIRE(a.n_rays >= 0, "n_rays must be >= 0 (got %d)", (int)a.n_rays);
    // the normal is geometry only: the feature fields, the background and every output pointer of the embedded struct are
    // ignored, whatever they hold; what is read goes through the checks of selfocc_render_fwd
    a.feat_vol = nullptr;
    a.feat_dtype = SO_DTYPE_F32; a.feat_stride = 0; a.n_rgb = 0; a.n_sem = 0;
    a.sh_deg = 0; a.sh_act = SO_SH_RELU;
    a.bkgd_mode = SO_BKGD_NONE; a.bkgd_rays = nullptr;
    a.flags = 0;
    a.depth = a.acc = a.rgb = a.sem = a.max_depth = a.nears = a.fars = nullptr;
    a.weights = a.ts = a.deltas = a.sdf = a.grad = nullptr;
    a.sdf_brick = nullptr;
    if (so_validate_render(a)) return -1;
    if (a.n_rays == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (a.map.kind == SO_MAP_UPSCALE) return launch_normal<SO_MAP_UPSCALE>(a, args->normal_vis, st);
    return launch_normal<SO_MAP_LINEAR>(a, args->normal_vis, st);
}
