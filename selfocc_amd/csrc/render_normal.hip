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
// An entry point of its own on the shared walker (sdf_walk_device.h: one ray per lane, canonical arithmetic, the replayed
// transmittance tree of render_train.hip).  Every ray marches all S samples: N depends on every w_i, and behind a surface a
// w_i under the replayed tree is small, not an exact zero (each step factor carries + 1e-7f; T is an exact 0 only once the
// product underflows), so there is no early exit.
#include "sdf_walk_device.h"

namespace {

struct so_normal_out {
    float *normal_vis;
    struct state {
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        SO_DEVFN state(const so_render_args &) {}
        // F.normalize(grad, p=2, eps=1e-12), weighted into the ray's sum
        SO_DEVFN bool visit(const RayGeom &, const so_walk_sample &s) {
            const float r = sqrtf((s.gx * s.gx + s.gy * s.gy) + s.gz * s.gz);
            const float d = fmaxf(r, 1e-12f);
            nx = nx + s.w * (s.gx / d);
            ny = ny + s.w * (s.gy / d);
            nz = nz + s.w * (s.gz / d);
            return false;
        }
        SO_DEVFN void store(const so_normal_out &out, int ray) const {
            float *o = out.normal_vis + 3 * (size_t)ray;
            o[0] = (nx + 1.0f) / 2.0f;
            o[1] = (ny + 1.0f) / 2.0f;
            o[2] = (nz + 1.0f) / 2.0f;
        }
    };
};

}  // namespace

extern "C" int selfocc_render_normal(const so_render_normal_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    SO_REQUIRE(args->normal_vis != nullptr, "normal_vis is NULL: nothing to compute");
    SO_REQUIRE(args->fwd.n_samples >= 1, "n_samples must be >= 1 (got %d)", (int)args->fwd.n_samples);
    SO_REQUIRE(args->fwd.n_rays >= 0, "n_rays must be >= 0 (got %d)", (int)args->fwd.n_rays);
    const so_render_args a = so_geometry_only(args->fwd);
    if (so_validate_render(a)) return -1;
    if (a.n_rays == 0) return 0;
    return so_walk_launch<so_normal_out>(a, (hipStream_t)stream, args->normal_vis);
}
