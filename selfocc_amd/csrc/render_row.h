// render_row.h — the feature-row formats of the render kernels: ONE compile-time descriptor and ONE host-side ladder for
// render_fwd.hip (per-ray march), render_train.hip (sample-parallel forward) and render_bwd.hip (backward).
//
// A row is what the feature volume holds per voxel: NF floats (float32) or NF bfloat16.  Every render kernel is a template
// over its row; so_with_row is the only place that maps a launch to one, and the only place (with so_validate_render) that
// knows how wide the row of a class count or of a spherical-harmonics degree is.
#pragma once
#include <type_traits>
#include "so_device.h"
#include "sh_device.h"

// NB == 0: [r, g, b, logit_0 .., pad] with degree-0 relu colour; NF = 0 (SDF only), 4 (colour) or 3 + classes rounded up to 4.
//   MASKED: the row holds a.n_sem in [NF - 6, NF - 3] logits and up to three pad channels, which SO_SEM_ON
//   (so_device.h) keeps out of the soft-max and the outputs; unmasked rows have exactly NF - 3 classes.
// NB > 0: spherical-harmonics colour with NB basis functions (sh_device.h): 3 * NB coefficients, colour-major, in NF floats.
template <int NF_, bool BF16_, int NB_ = 0, bool MASKED_ = false>
struct so_row {
    static constexpr int NF = NF_, NB = NB_;
    static constexpr bool BF16 = BF16_, MASKED = MASKED_;
    static constexpr int NSEM = (NB == 0 && NF > 4) ? NF - 3 : 0;   // semantic channels of the row (its capacity when MASKED)
    static_assert(NF % 4 == 0 && (NB == 0 || (NF == so_sh_stride(NB) && !BF16 && !MASKED)), "row format");
};
template <int NB>
using so_sh_row = so_row<so_sh_stride(NB), false, NB>;
template <int MK>
using so_map_kind = std::integral_constant<int, MK>;

// floats per voxel of a row with n_sem classes: r, g, b, the logits, rounded up to 16 bytes
constexpr int so_row_width(int n_sem) { return (3 + n_sem + 3) & ~3; }

// f(so_row<..>{}) for the row of a launch that so_validate_render accepts; returns what f returns
template <class F>
auto so_with_row(const so_render_args &a, F &&f) -> decltype(f(so_row<0, false>{})) {
    const int nf = a.n_rgb + a.n_sem;
    const bool bf = a.feat_dtype == SO_DTYPE_BF16;
    if (nf == 0) return f(so_row<0, false>{});
    if (so_sh_launch(a)) return a.sh_deg == 0 ? f(so_sh_row<1>{}) : (a.sh_deg == 1 ? f(so_sh_row<4>{}) : f(so_sh_row<9>{}));
    if (nf == 3) return bf ? f(so_row<4, true>{}) : f(so_row<4, false>{});
    // so_validate_render: n_sem in 2 .. 21, float32 rows, bfloat16 at 21 classes only
    if (nf == 8) return f(so_row<8, false>{});                 // the shipped widths: rows without a pad channel
    if (nf == 24) return bf ? f(so_row<24, true>{}) : f(so_row<24, false>{});
    switch (so_row_width(a.n_sem)) {                           // any other class count: the masked row of its width
        case 8: return f(so_row<8, false, 0, true>{});
        case 12: return f(so_row<12, false, 0, true>{});
        case 16: return f(so_row<16, false, 0, true>{});
        case 20: return f(so_row<20, false, 0, true>{});
        default: return f(so_row<24, false, 0, true>{});
    }
}

// f(row, so_map_kind<..>{}) for the row and the mapping kind of a launch; the refusals that depend on the row are here.
// 'linear_upscale' is built for every row but bfloat16 24.
template <class F>
int so_with_row_and_map(const so_render_args &a, F &&f) {
    SO_REQUIRE(a.n_rgb + a.n_sem != 3 || so_sh_launch(a) || a.feat_stride == 4, "n_rgb=3, n_sem=0 requires feat_stride == 4");
    return so_with_row(a, [&](auto row) -> int {
        using ROW = decltype(row);
        if (a.map.kind == SO_MAP_UPSCALE) {
            if constexpr (ROW::NF == 24 && ROW::BF16) {
                SO_REQUIRE(false, "the 'linear_upscale' mapping is built for n_rgb + n_sem = 0, 3, 8 and float32 24 (got bfloat16 24)");
            } else {
                return f(row, so_map_kind<SO_MAP_UPSCALE>{});
            }
        }
        return f(row, so_map_kind<SO_MAP_LINEAR>{});
    });
}
