// render_median.hip — median depth of the SDF ray march (selfocc_render_median): upstream nerfstudio's
// DepthRenderer(method="median"), the third depth target of eval_depth.py (`--depth_metric_tgt median`, eval_depth.py:178-218).
//
//   c_i = c_{i-1} + w_i (float32, sample order);   j = the first i with c_i >= 0.5f, S - 1 when there is none;
//   median_depth = ts_j,  median_index = j
//
// with w_i / ts_i the per-sample `weights` / `ts` of selfocc_render_fwd, BIT FOR BIT: the result is defined from those numbers
// (DESIGN.md section 3.16), so a caller that holds the per-sample tensors and one that asks this kernel get the same ray.
//
// An entry point of its own on the shared walker (sdf_walk_device.h: one ray per lane, canonical arithmetic, the replayed
// transmittance tree of render_train.hip).  A lane that has found its j stops; the loop ends for a wave when no lane is left
// (first crossing: a ray that hits a surface stops at the surface, only sky rays walk all S samples).
#include "sdf_walk_device.h"

namespace {

struct so_median_out {
    float *median_depth;
    int32_t *median_index;
    struct state {
        float c = 0.0f, tz = 0.0f;
        int j;
        SO_DEVFN state(const so_render_args &a) : j(a.n_samples - 1) {}
        SO_DEVFN bool visit(const RayGeom &g, const so_walk_sample &s) {
            tz = s.t_mid / g.dn;
            c = c + s.w;
            if (c >= 0.5f) { j = s.i; return true; }
            return false;
        }
        SO_DEVFN void store(const so_median_out &out, int ray) const {
            if (out.median_depth) out.median_depth[ray] = tz;
            if (out.median_index) out.median_index[ray] = j;
        }
    };
};

}  // namespace

extern "C" int selfocc_render_median(const so_render_median_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    SO_REQUIRE(args->median_depth != nullptr || args->median_index != nullptr,
               "median_depth and median_index are both NULL: nothing to compute");
    SO_REQUIRE(args->fwd.n_samples >= 1, "n_samples must be >= 1 (got %d)", (int)args->fwd.n_samples);
    SO_REQUIRE(args->fwd.n_rays >= 0, "n_rays must be >= 0 (got %d)", (int)args->fwd.n_rays);
    const so_render_args a = so_geometry_only(args->fwd);
    if (so_validate_render(a)) return -1;
    if (a.n_rays == 0) return 0;
    return so_walk_launch<so_median_out>(a, (hipStream_t)stream, args->median_depth, args->median_index);
}
