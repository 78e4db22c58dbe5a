/*
 * selfocc_hip.h — C ABI of the MI355X-native SelfOcc hot path (libselfocc_hip.so).
 *
 * Every entry point is the drop-in replacement of one native/third-party op the
 * reference (huang-yh/SelfOcc @ 2024-10-08) calls on its hot path.  Citations are
 * relative to the reference tree.  Conventions shared by all entry points:
 *
 *   - plain pointers + sizes only; all data pointers are DEVICE pointers (HBM);
 *     the *_args structs themselves live in HOST memory and are read during the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call
 *     is stream-ordered, does not synchronise, does not allocate, keeps no state;
 *   - the caller allocates all outputs; output pointers that are NULL are skipped;
 *   - return value: 0 = launched, <0 = argument error (see selfocc_last_error()),
 *     >0 = the hipError_t of a failed launch;
 *   - thread-safe / re-entrant (the last-error string is thread-local).
 */
#ifndef SELFOCC_HIP_H
#define SELFOCC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SELFOCC_ABI_VERSION 35

int selfocc_abi_version(void);
const char *selfocc_last_error(void);

/* ------------------------------------------------------------------------------------
 * Grid <-> metre mapping.  Replaces GridMeterMapping / LinearMapping.meter2grid
 * (model/encoder/bevformer/mappings.py:97-150).  One piece-wise linear axis:
 *     c = m - start;  a = |c|;
 *     g_abs = size1 == 0 ? a / range0 * size0
 *           : a > range0 ? size0 + (a - range0) / range1 * size1 : a / range0 * size0;
 *     g = (sign(c) * g_abs + off0) + off1          (off0/off1 = size0/size1 unless *_half)
 * Axis order everywhere: h <-> metre y, w <-> metre x, d <-> metre z.
 * ---------------------------------------------------------------------------------- */
typedef struct so_axis {
    float size0, size1;   /* cells in the inner / outer segment                        */
    float range0, range1; /* metres covered by the inner / outer segment               */
    float off0, off1;     /* grid offset of the axis centre (0,0 for *_half and for d) */
    float start;          /* metre coordinate of grid 0 on the d axis, 0 for h / w     */
    int32_t tot_len;      /* number of grid points along the axis                      */
} so_axis;

/* Mapping kinds.  The zero-initialised kind is the piece-wise linear form above, so a
 * caller that fills only h / w / d keeps its meaning.
 *
 * SO_MAP_UPSCALE is NonLinearMapping ('linear_upscale', mappings.py:199-288): uniform inner
 * cells, outer cells that grow by `inc` metres each.  Per axis, in float32, in this order:
 *   h / w (metre y / x, symmetric):  a = |m|
 *   d     (metre z, one-sided):      a = m - start
 *     base  = min(a / unit, size0)                     (size0 = inner cells)
 *     o     = relu(a - range0)                         (range0 = metres of the inner part)
 *     k     = floor(sqrt(c2 + (2 * o) / inc) - c)
 *     resi  = (o - k * unit) - ((inc * k) * (k + 1)) / 2
 *     g_abs = (base + k) + resi / (unit + (k + 1) * inc)
 *   h / w: g = (sign(m) * g_abs + off0) + off1        (off0 / off1 = inner / outer cells)
 *   d:     g = g_abs
 * The axis fields read: size0 / size1 = inner / outer cells, range0 = metres of the inner part
 * (range_inner, or z1 - z0), range1 = metres of the outer part, start = z0 on d (0 on h / w).
 * d grid / d metre is 1 / unit inside and 1 / (unit + (k + 1) * inc) in outer cell k. */
#define SO_MAP_LINEAR 0
#define SO_MAP_UPSCALE 1

/* constants of one 'linear_upscale' axis, computed in double on the host, stored as float32 */
typedef struct so_upscale_axis {
    float unit; /* metres per inner cell (hw_unit / z_unit)                   */
    float inc;  /* growth of the cell size per outer cell (increase_unit)     */
    float c;    /* 0.5 + unit / inc                                           */
    float c2;   /* (0.5 + unit / inc) ** 2                                    */
} so_upscale_axis;

typedef struct so_mapping {
    so_axis h, w, d;
    int32_t kind;                /* SO_MAP_LINEAR or SO_MAP_UPSCALE                  */
    int32_t _pad[3];             /* the kind fields take 64 bytes: the fields after
                                    so_mapping keep their offsets mod 64              */
    so_upscale_axis uh, uw, ud;  /* kind == SO_MAP_UPSCALE only                      */
} so_mapping;

/* Device form of meter2grid(xyz, normalize) for either mapping kind: xyz (n, 3) metres
 * (x, y, z) -> hwd (n, 3) grid coordinates (h, w, d), divided by tot_len - 1 when
 * `normalize` is non-zero.  Both pointers are device memory. */
int selfocc_meter2grid(const so_mapping *map, const float *xyz, int n, int normalize, float *hwd, void *stream);

/* ------------------------------------------------------------------------------------
 * SDF volume rendering.  Replaces the sdfstudio-fork NeuSCustomModel.__call__ that
 * NeuSHead drives (model/head/neus_head/neus_head.py:353,394,531) together with the
 * head's own post-math (:366-374, 430-438, 571-587) and, in pixel-grid mode, RaySampler
 * 'fixed'/'cellular' + Img2LiDAR (model/head/nerfacc_head/ray_sampler.py:23-68,
 * img2lidar.py:58-69).
 *
 * Volume layout in HBM (ours; the reference materialises (1, C, H, W, D)):
 *     sdf_vol  [H][W][D]               float32
 *     feat_vol [H][W][D][feat_stride]  float32 or bf16 (raw colour coefficients then
 *                                      semantic logits), feat_stride >= n_rgb + n_sem
 * ---------------------------------------------------------------------------------- */
enum {
    SO_RAYS_EXPLICIT = 0, /* origins / dirs / dir_norm arrays, one entry per ray       */
    SO_RAYS_PIXEL_GRID = 1 /* rays generated in-kernel from img2lidar + a pixel lattice */
};
enum { SO_SAMPLE_AT_START = 0, SO_SAMPLE_AT_MID = 1 };
enum { SO_BKGD_NONE = 0, SO_BKGD_CONST = 1, SO_BKGD_PER_RAY = 2 };
enum {
    SO_JITTER_NONE = 0, SO_JITTER_SINGLE = 1, SO_JITTER_PER_BIN = 2,
    SO_JITTER_EDGES = 3 /* no uniform bins: t_rand is (n_rays, n_samples + 1) NORMALISED edges b in [0, 1], non-decreasing along
                           a ray, and edge j lies at b * tfar + (1 - b) * tnear (selfocc_render_upsample writes such rows).
                           Always the canonical march; the edges are constants (no gradient). */
};
enum {
    SO_FLAG_DEPTH_DIV_NORM = 1, /* depth /= ||K^-1 (u,v,1)|| (z-depth, as the fork does) */
    SO_FLAG_CLAMP_RGB = 2,      /* eval: clamp rgb to [0,1]                              */
    SO_FLAG_EXACT = 4,          /* canonical IEEE operation order (bit-exact with oracle/): slower.
                                   Default is the fast path: per-ray affine grid coordinates (within
                                   ~1.5 ulp of the canonical divide chain; a sample closer than that
                                   to a voxel face re-derives its cell canonically, so the SAME cell
                                   as the canonical path is used at every interpolated sample),
                                   hardware exp2 / rcp, a cancellation-free form of the NeuS alpha,
                                   exact free-space skipping (see sdf_brick).  Parity of the fast
                                   path with the canonical one is stated and measured in DESIGN.md
                                   section 4 / tests/test_render_gpu.py (whole benchmarked frame:
                                   depth within 1e-4 relative on every ray that accumulates > 0.05). */
    SO_FLAG_NO_SKIP = 8,        /* fast path: do not skip saturated free-space samples (A/B switch) */
    SO_FLAG_RAY_PER_LANE = 64,  /* accepted and IGNORED since ABI 30 (rounds 2 - 4: per-sample launches through ray-per-lane
                                   kernels, an A/B switch nobody shipped; per-sample outputs always come from the
                                   sample-parallel training kernel)                                  */
    SO_FLAG_NO_AHEAD = 32,      /* fast path: general march even where the code-ahead skip marcher applies (A/B) */
    SO_FLAG_NO_FACE_SAFE = 16   /* fast path: never re-derive cells near voxel faces: ~6 % faster on
                                   the SDF-only kernel, but ~1e-4 of the rays (those with a sample
                                   within an ulp of a face, where the trilinear GRADIENT jumps) may
                                   then differ from the canonical result by more than 1e-4          */
};
enum { SO_DTYPE_F32 = 0, SO_DTYPE_BF16 = 1 };
/* activation of the spherical-harmonics colour (so_render_args::sh_act) */
enum { SO_SH_RELU = 0, SO_SH_SIGMOID = 1 };

/* View-dependent colour (so_render_args::sh_deg / sh_act; model/head/utils/sh_render.py:35-94 of the reference).
 * With n_rgb == 3 the first n_coef = 3 * n_basis, n_basis = (sh_deg + 1)^2, channels of a voxel row are spherical-
 * harmonics coefficients, COLOUR-MAJOR: channel c * n_basis + k is basis k of colour c.  Per sample, with f the
 * trilinearly interpolated channels and (x, y, z) the unit direction the march itself uses (explicit rays: dirs[ray];
 * pixel grid: the normalised M[:3,:3] (u, v, 1)), not negated:
 *     raw_c = sum_k Y_k(x, y, z) * f[c * n_basis + k]
 *     rgb_c = relu(raw_c + 0.5)   (SO_SH_RELU)     or     sigmoid(raw_c)   (SO_SH_SIGMOID)
 *     Y_0 = C0                                    C0 = 0.28209479177387814
 *     Y_1 = -C1 y,  Y_2 = C1 z,  Y_3 = -C1 x      C1 = 0.4886025119029199
 *     Y_4 = C2a xy, Y_5 = -C2a yz, Y_6 = C2b (2 zz - xx - yy), Y_7 = -C2a xz, Y_8 = C2c (xx - yy)
 *                                                 C2a = 1.0925484305920792, C2b = 0.31539156525252005, C2c = 0.5462742152960396
 * sh_deg = 0 with SO_SH_RELU is rgb = relu(C0 * raw + 0.5), the formula of every earlier ABI version: the zero-
 * initialised pair keeps its meaning and runs the kernels it always ran.  Everything after the colour (compositing,
 * background, SO_FLAG_CLAMP_RGB, depth / acc / max-depth / per-sample outputs) does not depend on sh_deg / sh_act.
 * Built: sh_deg 0 - 2, both activations, float32 feat_vol, n_sem == 0 whenever sh_deg > 0 or sh_act != SO_SH_RELU,
 *     feat_stride = 4 / 12 / 28 for sh_deg 0 / 1 / 2 (n_coef rounded up to a multiple of 4; pad channels are never read
 *     and their gradient stays zero).
 * These launches always march in the canonical operation order (SO_FLAG_EXACT changes nothing for them).
 * The two fields sit at the END of so_render_args, after everything a caller of the earlier layout fills, and
 * SELFOCC_ABI_VERSION is unchanged: a caller that zero-initialises the struct gets the behaviour it always got. */

/* Semantic classes (so_render_args::n_sem, with sh_deg == 0, sh_act == SO_SH_RELU, n_rgb == 3).  Built: n_sem = 0 and every
 * n_sem from 2 to 21.  A voxel row is [r, g, b, logit_0 .. logit_{n_sem - 1}, pad] and feat_stride MUST be 3 + n_sem rounded
 * up to a multiple of 4: 8 (2 - 5 classes), 12 (6 - 9), 16 (10 - 13), 20 (14 - 17) or 24 (18 - 21).  The up to three pad
 * channels may hold anything: they are never read into a result, and a backward never writes their gradient (it stays what
 * the caller put there: zero).  sem and g_sem are (n_rays, n_sem), without a pad.  5 and 21 classes (rows without a pad) run
 * the kernels they always ran; the other class counts run the render kernels on the masked row of their width, which compare the last
 * three channels with n_sem.  Those march face-safe: SO_FLAG_NO_FACE_SAFE is ignored for them.
 * Refused on the host, by name in selfocc_last_error(): n_sem == 1 (one class renders `acc`), n_sem >= 22 (the binned backward
 * record and the 32-lanes-per-sample brick kernel end at 24 channels), any other feat_stride, a bfloat16 feat_vol at a class
 * count other than 21, and n_sem > 0 together with sh_deg > 0 or SO_SH_SIGMOID.  No field is added and SELFOCC_ABI_VERSION is
 * unchanged. */

typedef struct so_render_args {
    /* --- field ------------------------------------------------------------------- */
    so_mapping map;
    const float *sdf_vol;
    const void *feat_vol; /* NULL when n_rgb + n_sem == 0 */
    int32_t feat_dtype;   /* SO_DTYPE_* */
    int32_t feat_stride;
    int32_t n_rgb;        /* 0 or 3 colour OUTPUTS; the colour channels read follow from sh_deg (below) */
    int32_t n_sem;        /* semantic classes; per-sample softmax, weight-composited    */
    /* --- rays -------------------------------------------------------------------- */
    int32_t ray_mode;     /* SO_RAYS_* */
    int32_t n_rays;       /* explicit: number of rays; pixel grid: n_cams * ny * nx     */
    const float *origins;   /* (n_rays, 3)                                              */
    const float *dirs;      /* (n_rays, 3) unit length                                  */
    const float *dir_norm;  /* (n_rays)  norm of the un-normalised direction            */
    const float *img2lidar; /* (n_cams, 4, 4) row-major pixel*depth -> world            */
    int32_t n_cams, nx, ny;
    float sx, sy, ox, oy;   /* pixel (u, v) = (ix * sx + ox, iy * sy + oy)              */
    /* --- sampling ---------------------------------------------------------------- */
    float aabb[6];          /* xmin ymin zmin xmax ymax zmax (box collider)             */
    float near_plane;
    int32_t n_samples;
    int32_t sample_pos;     /* SO_SAMPLE_AT_* : where the field is evaluated            */
    int32_t jitter_mode;    /* SO_JITTER_*                                              */
    const float *t_rand;    /* (n_rays) or (n_rays, n_samples + 1) uniform [0,1);
                               SO_JITTER_EDGES: the (n_rays, n_samples + 1) edges        */
    /* --- NeuS -------------------------------------------------------------------- */
    float inv_s;
    /* --- compositing ------------------------------------------------------------- */
    int32_t bkgd_mode;
    float bkgd[3];
    const float *bkgd_rays; /* (n_rays, 3) */
    int32_t flags;
    /* --- per-ray outputs --------------------------------------------------------- */
    float *depth;     /* (n_rays)                                                      */
    float *acc;       /* (n_rays)                                                      */
    float *rgb;       /* (n_rays, 3)                                                   */
    float *sem;       /* (n_rays, n_sem)                                               */
    float *max_depth; /* (n_rays)  ts[argmax_s w / delta]   (neus_head.py:430-438)     */
    float *nears;     /* (n_rays)                                                      */
    float *fars;      /* (n_rays)                                                      */
    /* --- per-sample outputs (training API, neus_head.py:567-577, 640) ------------- */
    float *weights;   /* (n_rays, n_samples)                                           */
    float *ts;        /* (n_rays, n_samples)  mid-point / dir_norm                     */
    float *deltas;    /* (n_rays, n_samples)  (end - start) / dir_norm                 */
    float *sdf;       /* (n_rays, n_samples)                                           */
    float *grad;      /* (n_rays, n_samples, 3)  d sdf / d (x, y, z) in metres         */
    /* --- optional workspace --------------------------------------------------------- */
    float *sdf_brick; /* scratch of H*W*D*17 bytes (16-B aligned; a larger one is fine) or NULL.  When
                         given, the fast path first re-packs sdf_vol into one 16-B record per cell, the
                         4 corners of its w-low face, so that the 8 corners of a cell are the records of
                         cells (h, w, d) and (h, w + 1, d) (2 x 16-B loads per sample instead of 4 x 8-B gathers),
                         followed by one "free-space skip" byte per cell: the largest ray step for
                         which every sample inside the cell has both NeuS sigmoids saturated to
                         exactly 1.0f (alpha is then the constant 1e-5 / (1 + 1e-5) in the
                         canonical float32 order too), so SDF-only per-ray launches composite
                         such samples without interpolating.  The re-pack kernel is launched by
                         selfocc_render_fwd on the same stream before the march.              */
    const float *inv_s_dev; /* optional DEVICE pointer to inv_s (1 float).  When non-NULL the kernels read
                         inv_s from it and ignore the host value above: a training loop whose inv_s is
                         a learnable parameter (exp(10 * variance), neus_head.py:631-633) never has to
                         read it back to the host (no stream sync, nothing to go stale).       */
    /* --- view-dependent colour (see above); zero = degree 0 with relu ------------------ */
    int32_t sh_deg;         /* 0, 1 or 2: 3 / 12 / 27 coefficient channels                             */
    int32_t sh_act;         /* SO_SH_*                                                                  */
} so_render_args;

int selfocc_render_fwd(const so_render_args *args, void *stream);

/* Backward of selfocc_render_fwd with respect to the volume(s) and inv_s.  Ray
 * geometry carries no gradient (the reference's rays come from constant matrices).
 * Upstream gradients that are NULL count as zero.  g_sdf_vol / g_feat_vol must be
 * zero-initialised by the caller (atomically accumulated). */
typedef struct so_render_bwd_args {
    so_render_args fwd;       /* same inputs as the forward call (outputs ignored)     */
    const float *g_depth;     /* (n_rays)                                              */
    const float *g_acc;       /* (n_rays)                                              */
    const float *g_rgb;       /* (n_rays, 3)                                           */
    const float *g_sem;       /* (n_rays, n_sem)                                       */
    const float *g_weights;   /* (n_rays, n_samples)                                   */
    const float *g_sdf;       /* (n_rays, n_samples)                                   */
    const float *g_grad;      /* (n_rays, n_samples, 3)                                */
    float *g_sdf_vol;         /* [H][W][D]                                             */
    float *g_feat_vol;        /* [H][W][D][feat_stride] float32                        */
    float *g_inv_s;           /* (1)                                                   */
    /* Optional scratch for the BRICK-BINNED volume-gradient scatter (round 4).  NULL: every sample adds its
     * 8 corner rows to g_sdf_vol / g_feat_vol with device-scope float atomics (on MI355X each one is a write
     * through the fabric: 3.1 GB of them for a 165 MB gradient at the nuscenes_occ training shape).  Given
     * (>= selfocc_render_bwd_ws_bytes() bytes, 256-B aligned): a counting pre-pass gives every sample a slot in
     * brick order (bricks of 4 x 4 x 8 CELLS); the ray kernel writes one record per sample at its slot (cell,
     * fractions, d L / d feature row, SDF coefficients: 32 / 64 / 128 B at 0 / 3-8 / 20-24 channels); one
     * workgroup per (brick, <= chunk samples) streams its records, sums them into the brick's 5 x 5 x 9-voxel
     * tile in LDS — a DOUBLE tile: ds_add_f64 issues ~12 x faster than ds_add_f32 on gfx950 — and adds the
     * tile's non-zero rows to the gradient once.  A sample whose cell lies outside the volume contributes
     * nothing in either mode.  Same sums, different (still unspecified) float addition order.              */
    void *scatter_ws;
    uint64_t scatter_ws_bytes;
} so_render_bwd_args;

int selfocc_render_bwd(const so_render_bwd_args *args, void *stream);
/* bytes of so_render_bwd_args::scatter_ws for this call.  0 = the call is outside the binned path's range — pass
 * NULL then (the atomic path runs): args == NULL, n_rays <= 0 or n_samples <= 0, an axis longer than 1021 grid
 * points, n_rays * n_samples >= 2^31, or a channel count other than 0 / 3 / 8 / 20 / 24.  Spherical-harmonics launches
 * (sh_deg > 0 or sh_act != SO_SH_RELU) use the 64-byte record at every degree: it carries d L / d raw_c (3 floats) and the
 * ray's unit direction (3 floats) in place of a d L / d feature row, and the brick kernel expands Y_k from the direction. */
size_t selfocc_render_bwd_ws_bytes(const so_render_bwd_args *args);

/* Median depth of the march: upstream nerfstudio's DepthRenderer(method="median"), the `ms_depths_median` eval_depth.py reads
 * (eval_depth.py:178-218).  Per ray, with w_i / ts_i the per-sample `weights` / `ts` selfocc_render_fwd writes for the same
 * inputs (the same bits):
 *     c_0 = w_0,  c_i = c_{i-1} + w_i                  float32, in sample order
 *     j   = the smallest i with c_i >= 0.5f;  n_samples - 1 when there is none (a NaN sum never reaches 0.5)
 *     median_depth = ts_j        median_index = j
 * One launch of a kernel of its own (csrc/render_median.hip): one ray per lane, canonical arithmetic whatever SO_FLAG_EXACT
 * says, and a ray stops marching at its j.  It reads the SDF volume only: of `fwd`, the mapping, sdf_vol, the ray fields,
 * the sampling fields (aabb, near_plane, n_samples, sample_pos, jitter_mode, t_rand), inv_s and inv_s_dev are used;
 * feat_vol, feat_dtype, feat_stride, n_rgb, n_sem, sh_deg, sh_act, bkgd_*, flags, sdf_brick and every output pointer of `fwd`
 * are ignored.  Refused by name: both outputs NULL, n_samples < 1, n_rays < 0, and what selfocc_render_fwd refuses among
 * the fields that are read.  n_rays == 0 succeeds without a launch.  A new entry point: SELFOCC_ABI_VERSION is unchanged. */
typedef struct so_render_median_args {
    so_render_args fwd;        /* inputs as for selfocc_render_fwd; outputs and feature fields ignored */
    float   *median_depth;     /* (n_rays) or NULL */
    int32_t *median_index;     /* (n_rays) or NULL */
} so_render_median_args;
int selfocc_render_median(const so_render_median_args *args, void *stream);

/* Rendered surface normal of the march: sdfstudio's `normal_vis`, the `vis_normal` of the reference's render dicts
 * (neus_head.py:358, 379, 414, 463).  Per ray, with w_i the per-sample `weights` and g_i = (gx, gy, gz)_i the per-sample `grad`
 * selfocc_render_fwd writes for the same inputs (the same bits; `grad` is the trilinear SDF gradient of the sample's cell):
 *     r_i  = sqrtf((gx*gx + gy*gy) + gz*gz)            float32, this order
 *     d_i  = fmaxf(r_i, 1e-12f)                        F.normalize(p=2, eps=1e-12)
 *     n_i  = (gx / d_i, gy / d_i, gz / d_i)            three IEEE divisions
 *     N    = 0;  for i = 0 .. n_samples - 1 in sample order:  N = N + w_i * n_i     multiply, then add; no fused multiply-add
 *     normal_vis = (N + 1.0f) / 2.0f                   (n_rays, 3)
 * One launch of a kernel of its own (csrc/render_normal.hip): one ray per lane, canonical arithmetic whatever SO_FLAG_EXACT
 * says, every ray marches all n_samples samples; a ray that misses the box by more than a cell (corners outside the volume read
 * as 0: zero gradients) gives (0.5, 0.5, 0.5).  It reads the SDF volume only: of `fwd`, the mapping, sdf_vol, the ray fields, the sampling fields (aabb,
 * near_plane, n_samples, sample_pos, jitter_mode, t_rand), inv_s and inv_s_dev are used; feat_vol, feat_dtype, feat_stride,
 * n_rgb, n_sem, sh_deg, sh_act, bkgd_*, flags, sdf_brick and every output pointer of `fwd` are ignored.  Refused by name:
 * args NULL, normal_vis NULL, n_samples < 1, n_rays < 0, and what selfocc_render_fwd refuses among the fields that are read.
 * n_rays == 0 succeeds without a launch.  A new entry point: SELFOCC_ABI_VERSION is unchanged. */
typedef struct so_render_normal_args {
    so_render_args fwd;        /* inputs as for selfocc_render_fwd; outputs and feature fields ignored */
    float *normal_vis;         /* (n_rays, 3) */
} so_render_normal_args;
int selfocc_render_normal(const so_render_normal_args *args, void *stream);

/* NeuS hierarchical up-sampling: the coarse-to-fine sampler of NeuS (a declared restatement of upstream sdfstudio's NeuSSampler
 * + nerfstudio's PDFSampler).  Per ray, with the collider's tnear / tfar, S0 = fwd.n_samples,
 * M = n_importance, K = n_steps, m = M / K (integer division), one number r_k in [0, 1) per step (0.5 when u_rand is NULL):
 *   state: normalised edges b[0..n], non-decreasing, n samples.  Start: n = S0, b[j] = the uniform bin edge j with the
 *          SO_JITTER_SINGLE / SO_JITTER_PER_BIN jitter when asked (what the march itself uses).  Metric position of an edge,
 *          everywhere: t = b * tfar + (1 - b) * tnear.
 *   for k = 0 .. K - 1, s = base_variance * 2^k:
 *     1. f_i = trilinear SDF at o + d * t_i, i = 0 .. n - 1 (always the sample start, whatever sample_pos says)
 *     2. for i = 0 .. n - 2:  delta_i = t_{i+1} - t_i,  mid = (f_i + f_{i+1}) * 0.5,  cos_i = (f_{i+1} - f_i) / (delta_i + 1e-5),
 *        c_i = clip(min(cos_{i-1}, cos_i), -1e3, 0) with cos_{-1} = 0,  e- = mid - c_i delta_i * 0.5,  e+ = mid + c_i delta_i * 0.5,
 *        alpha_i = (sigmoid(e- s) - sigmoid(e+ s) + 1e-5) / (sigmoid(e- s) + 1e-5)
 *     3. w_i = alpha_i prod_{j<i} (1 - alpha_j + 1e-7) for i <= n - 2,  w_{n-1} = 0
 *     4. w_i += 1e-5;  W = sum w;  pad = max(0, 1e-5 - W);  w_i += pad / n;  W += pad;
 *        cdf_0 = 0,  cdf_{i+1} = min(1, cdf_i + w_i / W)
 *     5. u_j = lin_j + r_k / (m + 1), j = 0 .. m, lin = linspace(0, 1 - 1 / (m + 1), m + 1) in float32;
 *        idx = number of cdf entries <= u_j;  lo = clamp(idx - 1, 0, n),  hi = clamp(idx, 0, n);
 *        q = (u_j - cdf_lo) / (cdf_hi - cdf_lo), 0 when the denominator is 0, clipped to [0, 1];  p_j = b_lo + q (b_hi - b_lo)
 *     6. the new edges are sort(b[0..n-1] U p[0..m-1]) followed by max(b[n], p[m]);  n <- n + m
 * Result: S_tot = S0 + K m samples, S_tot + 1 edges per ray in `edges`, to be marched with SO_JITTER_EDGES.  With M = 0, K = 0
 * or m = 0 no step runs and `edges` receives the S0 + 1 start edges.  One wave per ray, no atomics: the same inputs give the
 * same bits on every launch.  Of `fwd`, the mapping, sdf_vol, the ray fields, aabb, near_plane, n_samples, jitter_mode and
 * t_rand are read; feature fields, inv_s and outputs are ignored.  Refused by name: edges NULL, n_samples < 1, negative
 * n_importance / n_steps, n_steps > 8, S_tot > 256 (what the per-sample forward and the backward take), base_variance not
 * positive, SO_JITTER_EDGES as the start, and what selfocc_render_fwd refuses among the fields read.  n_rays == 0 succeeds
 * without a launch.  A new entry point: SELFOCC_ABI_VERSION is unchanged. */
typedef struct so_render_upsample_args {
    so_render_args fwd;        /* inputs as for selfocc_render_fwd; outputs and feature fields ignored */
    int32_t n_importance;      /* M */
    int32_t n_steps;           /* K */
    float base_variance;       /* inv_s of step 0; doubled every step */
    const float *u_rand;       /* (n_steps, n_rays) uniform [0, 1), or NULL: 0.5 */
    float *edges;              /* (n_rays, S_tot + 1) normalised edges */
} so_render_upsample_args;
int selfocc_render_upsample(const so_render_upsample_args *args, void *stream);

/* ------------------------------------------------------------------------------------
 * Multi-scale deformable attention.  Replaces mmcv==2.0.1
 * MultiScaleDeformableAttnFunction.apply(value, spatial_shapes, level_start_index,
 * sampling_locations, attention_weights, im2col_step) at the reference call sites
 * model/encoder/bevformer/attention/image_cross_attention.py:340-342 and
 * model/encoder/tpvformer/attention/cross_view_hybrid_attention.py:111-113.
 *
 *   out[b,q,h*d+c] = sum_{l,p} attw[b,q,h,l,p] * bilinear(value_l[b, :, h, c], loc[b,q,h,l,p])
 *
 * Three forms share one argument struct (fields a form does not name are ignored):
 *   SO_MSDA_PLAIN  mmcv's op: value (bs,nv,heads,d) float32, loc (bs,nq,heads,L,P,2) (x, y) in [0,1],
 *                  attw (bs,nq,heads,L,P), out (bs,nq,heads*d); d = 4, 8, 16 or 32.
 *   SO_MSDA_FUSED  the reference's prologue inside the kernels (softmax over the L*P logits of a (query, head);
 *                  loc = ref + off / (W_l, H_l); image_cross_attention.py:314-328, cross_view_hybrid_attention.py:88-99),
 *                  in both directions: sampling locations / attention weights are never materialised.
 *                  off_raw (bs,nq,heads,L,P,2), logits (bs,nq,heads,L*P), out (bs,nq,heads*d).
 *   SO_MSDA_CROSS  the camera loop: BEVCrossAttention's re-batch -> offset / weight linears -> MSDA -> scatter-add ->
 *                  divide-by-count (bevformer/attention/image_cross_attention.py:90-136) as ONE launch per direction.
 *                  The offsets and logits depend on the query only; each (query, head) loops over the cameras that
 *                  see it, in camera order:
 *                    out[q] = sum_{cam: vis[cam][q]} msda(value[cam], ref[cam][q] + off[q] / (W_l, H_l), softmax(logits[q]))
 *                             / max(#visible cams, 1)
 *                  value (cams,nv,heads,d), off_raw (nq,heads,L,P,2), logits (nq,heads,L*P), out (nq,heads*d);
 *                  batch size 1 (as the reference's masks).
 * FUSED and CROSS: d = 8, 16 or 32 (bfloat16 value: 16 only), L*P <= 256.
 * ---------------------------------------------------------------------------------- */
enum { SO_MSDA_PLAIN = 0, SO_MSDA_FUSED = 1, SO_MSDA_CROSS = 2 };

/* Layout of `value` (and of `g_value`) for the fused / camera-loop forms — the ones this repo's own encoder
 * modules call, so the layout is theirs to choose; the plain form keeps mmcv's.
 *   SO_VALUE_PIXEL_MAJOR (bs, nv, heads, d): mmcv.  A 128-byte cache line holds one pixel of TWO heads.
 *   SO_VALUE_HEAD_MAJOR  (bs, heads, nv, d): a line holds two horizontally adjacent pixels of ONE head, i.e. usually
 *   both x-corners of a bilinear footprint; the gathers of the hw-plane cross-attention run 0.34 ms instead of 0.50. */
enum { SO_VALUE_PIXEL_MAJOR = 0, SO_VALUE_HEAD_MAJOR = 1 };

typedef struct so_msda_args {
    int32_t form;           /* SO_MSDA_*                                                                    */
    int32_t bs;             /* batch size; the number of cameras for SO_MSDA_CROSS (>= 1)                   */
    int32_t nv;             /* pixels of all levels of one value map                                        */
    int32_t nq;             /* queries                                                                      */
    int32_t heads, d;       /* heads, channels per head                                                     */
    int32_t L, P;           /* levels, sampling points per level                                            */
    int32_t value_layout;   /* SO_VALUE_* (FUSED / CROSS; PLAIN: pixel-major)                               */
    int32_t value_dtype;    /* SO_DTYPE_F32, or SO_DTYPE_BF16 (FUSED / CROSS) = bfloat16 STORAGE of `value`: the
                               arithmetic is float32 on the exactly widened values, g_value stays float32; halves the
                               64-byte corner segments the gathers move.  Results equal the float32 kernels run on
                               bf16-rounded values; against unrounded values the relative error is ~2^-9 (opt-in:
                               BASELINE configs[1] allows bf16 storage, the reference computes MSDA in f32)       */
    int32_t value_stride;   /* CROSS forward: floats between consecutive pixels of a pixel-major `value` (0 = dense,
                               heads*d; else a multiple of 4 >= heads*d): lets `value` be a column block of a wider
                               matrix, e.g. the three TPV planes' value projections computed by ONE GEMM with
                               N = 3 * heads * d.  0 everywhere else                                          */
    int32_t ref_kind;       /* FUSED: 0: ref (bs,nq,L,2)   1: ref (bs,nq,P,2)   2: ref (bs,nq,L,P,2)           */
    int32_t ol_stride;      /* FUSED / CROSS (ABI 32): floats between consecutive QUERY rows of off_raw and logits (and of
                               g_off / g_logits).  0 = the dense tensors above.  3 * heads * L * P (or more, even) = ONE row
                               per query [heads*L*P*2 raw offsets | heads*L*P logits], i.e. the output of the
                               `sampling_offsets` and `attention_weights` Linears computed as ONE projection with the two
                               weights stacked (image_cross_attention.py:296-312 reads the same `query` twice); `logits` =
                               `off_raw` + 2 * heads * L * P then (8-byte aligned), and the backward writes the gradient of
                               that merged row, which is what ONE input-gradient and ONE weight-gradient pass of the stacked
                               Linear consume                                                                  */
    int32_t g_value_stride; /* FUSED / CROSS backward (ABI 32): 0 = g_value has the layout of `value`.  > 0 (>= heads*d) =
                               g_value is written PIXEL-major into rows of that many floats — (bs, nv) rows, this op's
                               heads * d channels starting at the pointer —, i.e. straight into a column block of the
                               row-major gradient of the (stacked) value projection: no head-major -> row-major
                               transposing copy before its weight- / input-gradient passes                     */
    const void *value;      /* float32 or bfloat16 per value_dtype                                          */
    const int32_t *shapes;  /* (L, 2) [H_l, W_l]                                                            */
    const int32_t *starts;  /* (L) first pixel of each level                                                */
    const int32_t *host_shapes; /* HOST copy of `shapes` for the banded backward's work decomposition; the
                               plain backward without it takes the global-atomic scatter                      */
    const float *loc;       /* PLAIN: (bs,nq,heads,L,P,2)                                                   */
    const float *attw;      /* PLAIN: (bs,nq,heads,L,P)                                                     */
    const float *ref;       /* FUSED: per ref_kind;  CROSS: (cams,nq,P,2)                                   */
    const uint8_t *vis;     /* CROSS: (cams,nq), non-zero = the camera sees the query                       */
    const float *off_raw;   /* FUSED / CROSS: raw sampling-offset linear output                             */
    const float *logits;    /* FUSED / CROSS: attention logits before the softmax                           */
    float *out;             /* forward output                                                               */
    /* --- backward --------------------------------------------------------------------------------------------- */
    const float *g_out;     /* gradient of `out` (CROSS: of the camera MEAN)                                */
    float *g_value;         /* zero-initialised by the caller (accumulated); CROSS: sums over the visible cameras / count */
    float *g_loc, *g_attw;  /* PLAIN                                                                        */
    float *g_off, *g_logits; /* FUSED / CROSS: gradients w.r.t. the RAW linear outputs, laid out as off_raw / logits:
                               g_off = (d out / d loc) / (W_l, H_l), g_logits = aw (g_aw - sum aw g_aw) (softmax backward),
                               with the softmax / sampling locations recomputed in registers                   */
    /* Banded (output-stationary) scatter of grad_value (PLAIN with host_shapes; always for FUSED / CROSS): the
     * sampling points are counting-sorted by (batch, head, level, band of rows); a block owns one band of one level's
     * map in LDS and adds the points of its list with ds_add_f64 — no global atomics in the scatter, grad_value
     * accumulated in double and rounded once per list segment (same results as the atomic scatter up to summation
     * order).  Needs host_shapes (L <= 8) and a 16-byte aligned device workspace of selfocc_msda_ws_bytes() bytes
     * (26 bytes per sampling point: a 2-byte row key, a 16-byte record, two 4-byte list slots; plus 28 KB of counters
     * per (batch, head, level); contents undefined before and after).  PLAIN falls back to the atomic scatter when
     * selfocc_msda_banded_supported() is 0; FUSED / CROSS then fail.                                             */
    void *workspace;
    uint64_t workspace_bytes;
} so_msda_args;

int selfocc_msda_fwd(const so_msda_args *args, void *stream);
int selfocc_msda_bwd(const so_msda_args *args, void *stream);
/* bytes of so_msda_args::workspace for these sizes (0: bad sizes); reads form, bs, nq, heads, L and P only */
size_t selfocc_msda_ws_bytes(const so_msda_args *args);
/* 1: the banded scatter applies to these shapes, 0: it does not (a level wider than the LDS tile, more than 1024
 * bands per level or 8 levels, >= 2^30 sampling points), -1: bad arguments.  Reads the form, the sizes and
 * host_shapes only. */
int selfocc_msda_banded_supported(const so_msda_args *args);
/* What selfocc_msda_fwd / _bwd would decide for this call, without launching anything: reads the form, the sizes,
 * value_dtype and host_shapes (may be NULL: the band entries stay 0), no device pointer.  Writes SO_MSDA_PLAN_INTS ints:
 *   [SO_MSDA_PLAN_LOG2_GROUP]  log2 of the lanes per (query, head) group of this form's forward (and of the fused / camera-loop
 *                              backward point kernel): with d and value_dtype, the kernel instantiation
 *   [SO_MSDA_PLAN_BANDED]      1: the banded scatter applies (selfocc_msda_banded_supported)
 *   [SO_MSDA_PLAN_COUNT_HERE]  CROSS backward: the point kernel counts the sort's buckets itself (else a separate pass does)
 *   [SO_MSDA_PLAN_BIN_VIS]     CROSS backward: the sort skips invisible (camera, query) pairs by `vis` (else keys are preset)
 *   [SO_MSDA_PLAN_BANDS + l]   bands level l < min(L, 8) is cut into,  [SO_MSDA_PLAN_ROWS + l]  map rows per band
 * Returns -1 with selfocc_last_error() for sizes the checks refuse and for shapes no kernel is built for.  A new entry point:
 * SELFOCC_ABI_VERSION is unchanged. */
enum { SO_MSDA_PLAN_LOG2_GROUP = 0, SO_MSDA_PLAN_BANDED = 1, SO_MSDA_PLAN_COUNT_HERE = 2, SO_MSDA_PLAN_BIN_VIS = 3,
       SO_MSDA_PLAN_BANDS = 4, SO_MSDA_PLAN_ROWS = 12, SO_MSDA_PLAN_INTS = 20 };
int selfocc_msda_plan(const so_msda_args *args, int32_t *out);

/* ------------------------------------------------------------------------------------
 * Dense SDF / semantic query on a regular metre lattice + Occ3D occupancy tail.
 * Replaces NeuSHead.get_uniform_sdf -> field.forward_geonetwork / forward_sdfnetwork
 * (model/head/neus_head/neus_head.py:265-293) and the resample / threshold / argmax /
 * LUT of eval_iou.py:211-250.
 * ---------------------------------------------------------------------------------- */
typedef struct so_query_args {
    so_mapping map;
    const float *sdf_vol;
    const void *feat_vol;
    int32_t feat_dtype, feat_stride, n_rgb, n_sem;
    const float *xyz;     /* (n, 3) metre positions                                    */
    int32_t n;
    float *sdf;           /* (n)                                                       */
    float *sem_logits;    /* (n, n_sem) raw logits (forward_geonetwork h[..., 4:])     */
    int32_t *sem_argmax;  /* (n)                                                       */
} so_query_args;

int selfocc_field_query(const so_query_args *args, void *stream);

/* Backward of selfocc_field_query with respect to the volume(s) (the reference differentiates
 * get_uniform_sdf through F.grid_sample: model/head/neus_head/neus_head.py:532-538 feeds
 * `uniform_sdf` to SoftSparsityLoss, loss/sparsity_loss.py:67-81):
 *   g_sdf (n) -> g_sdf_vol [H][W][D];  g_logits (n, n_sem) -> g_feat_vol [H][W][D][feat_stride] float32
 * (channels n_rgb .. n_rgb + n_sem - 1).  Either pair may be NULL.  The volume gradients are
 * ACCUMULATED (atomic adds): zero-initialise them.  Outputs of `args` (sdf, sem_*) are ignored. */
int selfocc_field_query_bwd(const so_query_args *args, const float *g_sdf, const float *g_logits,
                            float *g_sdf_vol, float *g_feat_vol, void *stream);

/* SDF gradient d sdf / d metre at arbitrary metre positions (csrc/field_grad.hip).
 *   SO_GRAD_ANALYTIC   the gradient the render kernels define for a sample at that position (so_locate_k, so_gather_sdf,
 *                      so_trilerp_grad of so_device.h: cell, corner differences and d grid / d metre slope, zero padding)
 *   SO_GRAD_NUMERICAL  central differences (sdfstudio's use_numerical_gradients): for each axis k, p+- = x with
 *                      x_k +- delta in float32, s+- = the value selfocc_field_query returns at p+-,
 *                      grad_k = (0.5f * (s+ - s-)) / delta in that association
 * q.map, q.sdf_vol, q.xyz and q.n are read; q.sdf may be NULL, and when given it is selfocc_field_query's value bit for bit;
 * the feature / logit / arg-max fields of q are ignored.  Argument checks are host logic and run before any HIP call; n == 0
 * succeeds without a launch.  New entry points and a new struct: SELFOCC_ABI_VERSION is unchanged. */
#define SO_GRAD_ANALYTIC 0
#define SO_GRAD_NUMERICAL 1
typedef struct so_field_grad_args {
    so_query_args q;
    float *grad;          /* (n, 3) d sdf / d metre (x, y, z)                          */
    int32_t mode;         /* SO_GRAD_ANALYTIC or SO_GRAD_NUMERICAL                     */
    float delta;          /* metres, > 0; SO_GRAD_NUMERICAL only                       */
} so_field_grad_args;

int selfocc_field_grad(const so_field_grad_args *args, void *stream);

/* Backward of selfocc_field_grad with respect to the SDF volume (both modes are linear in it): g_sdf (n) and / or g_grad (n, 3),
 * either may be NULL, are scattered to the 8 corners of the point's cell (analytic) or of each of the 6 taps' cells (numerical;
 * g_sdf to the point's own cell).  g_sdf_vol [H][W][D] is ACCUMULATED (atomic adds): zero-initialise it.  Positions carry no
 * gradient.  The outputs of `args` (q.sdf, grad) are ignored. */
int selfocc_field_grad_bwd(const so_field_grad_args *args, const float *g_sdf, const float *g_grad, float *g_sdf_vol,
                           void *stream);

/* ------------------------------------------------------------------------------------
 * Tri-plane -> dense volume: the head's pre_compute_density_color(representation)
 * (sdfstudio-fork SDFCustomField, driven from model/head/neus_head/neus_head.py:295-306;
 * in-repo analogue BEVNeRF, model/head/nerfacc_head/bev_nerf.py:74-95), forward only:
 *   x[h,w,d,:] = hw[h,w,:] + zh[d,h,:] + wz[w,d,:]                        hw (H*W, C)  zh (D*H, C)  wz (W*D, C)
 *   out = Linear_out(Softplus(Linear_hidden(Softplus(x))))  (n_hidden = 1; n_hidden = 0 drops the hidden layer)
 *   sdf[h,w,d] = out[0];  feat[h,w,d,0..out_dim-2] = out[1..], channels up to feat_stride zero-filled.
 * Weights in torch.nn.Linear layout: w_hidden (C, C), w_out (out_dim, C).  C in {64, 96, 128},
 * out_dim <= 32, feat_stride <= 31.  One fused MFMA-f32 kernel (exact float32 arithmetic); the
 * H*W*D x C intermediate is never materialised. */
int selfocc_field_volume_fwd(const float *hw, const float *zh, const float *wz, int32_t H, int32_t W,
                             int32_t D, int32_t C, const float *w_hidden, const float *b_hidden,
                             int32_t n_hidden, const float *w_out, const float *b_out, int32_t out_dim,
                             float *sdf, void *feat, int32_t feat_dtype, int32_t feat_stride, void *stream);

/* Backward of selfocc_field_volume_fwd (C in {64, 96, 128}, one hidden layer, float32 feature volume): g_sdf (H*W*D)
 * and g_feat (H*W*D, feat_stride) -> gradients of the three planes and of the two linear layers (all seven
 * outputs zero-initialised by the caller, accumulated).  Nothing of the forward is needed: the kernel
 * recomputes the activations per 32-voxel tile (a 4 x 4 x 2 patch; any (H, W, D), ragged patches masked).
 * g_sdf / g_feat may be NULL (treated as zero); out_dim in 1..32, any feat_stride >= out_dim - 1.
 * One width-generic float32-MFMA kernel serves C = 64 / 96 / 128; C = 96 takes the bf16 x 3 kernel instead (float32-level
 * accuracy) unless SELFOCC_FIELD_BWD_B3=0 (read at every call), feat_stride is not a multiple of 4, or the volume needs
 * 64-bit indices.  Any other width returns < 0 ("embed_dims must be 64, 96 or 128") without touching a buffer. */
int selfocc_field_volume_bwd(const float *hw, const float *zh, const float *wz, int32_t H, int32_t W,
                             int32_t D, int32_t C, const float *w_hidden, const float *b_hidden,
                             const float *w_out, int32_t out_dim, const float *g_sdf, const float *g_feat,
                             int32_t feat_stride, float *g_hw, float *g_zh, float *g_wz, float *g_w_hidden,
                             float *g_b_hidden, float *g_w_out, float *g_b_out, void *stream);

/* Occ3D evaluation tail, eval_iou.py:211-250: trilinear resample (F.grid_sample,
 * align_corners=True, zero padding — bit-exact with torch's CPU kernel) of the dense SDF
 * grid (+ optional semantic logits) at the ego-frame Occ3D lattice, threshold, border crop,
 * argmax + openseed2nuscenes LUT (utils/metric_util.py:37-64), occupancy * semantics.
 *   grid    [H][W][D] float32           logits [H][W][D][C] float32 (NULL: no semantics)
 *   coords  (n, 3) normalised [0,1] along (H, W, D) of `grid`; n = n0 * n1 * n2 lattice
 *   crop    {lo0, hi0, lo1, hi1, lo2, hi2}: output index i_k outside [lo_k, n_k - hi_k) -> 0
 *   density != 0 selects (value >= thresh) (eval_iou.py:205-206,227) instead of (<=). */
typedef struct so_occ_args {
    const float *grid;
    const float *logits;
    int32_t H, W, D, C;
    const float *coords;
    int32_t n0, n1, n2;
    int32_t crop[6];
    float thresh;
    int32_t density;
    const int32_t *lut; /* (C) class LUT applied to the argmax, NULL = identity */
    float *sampled;     /* (n) resampled scalar, optional                        */
    int32_t *occ;       /* (n) 0 / 1                                             */
    int32_t *sem;       /* (n) occ * lut[argmax_c logits], optional              */
} so_occ_args;

int selfocc_occ_resample(const so_occ_args *args, void *stream);

/* Integer confusion counts of MeanIoU._after_step (utils/metric_util.py:90-121):
 * counts (3, n_cls + 1) int64 rows = seen / correct / positive; last column = the
 * binary "non-empty" class.  mask may be NULL.  counts are accumulated (+=). */
int selfocc_iou_counts(const int32_t *pred, const int32_t *target, const uint8_t *mask,
                       int64_t n, const int32_t *class_indices, int32_t n_cls,
                       int32_t empty_label, unsigned long long *counts, void *stream);

/* The eikonal regulariser (/root/reference/loss/eikonal_loss.py:19-22): sum over the n rows of grad (n, 3) float32 of
 * (||grad_i||_2 - 1)^2 as selfocc_eikonal_partials(n) per-block partial sums (the caller adds them: a fixed order, so the
 * result is deterministic; the mean is that sum / n), and its gradient g_grad_i = 2 * scale[0] * (||grad_i|| - 1) grad_i /
 * ||grad_i|| (0 where the norm is 0, as torch's norm backward), `scale` a 1-element DEVICE tensor (upstream gradient / n:
 * no host read-back).  Returns 0 / SELFOCC_ERR_*. */
int selfocc_eikonal_partials(int64_t n);
int selfocc_eikonal_fwd(const float *grad, float *partial, int64_t n, void *stream);
int selfocc_eikonal_bwd(const float *grad, const float *scale, float *g_grad, int64_t n, void *stream);

/* `y = identity + dropout(x)` of the attention / FFN outputs (mmcv: `self.dropout(output) + identity`,
 * /root/reference/model/encoder/bevformer/attention/image_cross_attention.py:137-139,
 * tpvformer/attention/cross_view_hybrid_attention.py:119-124) in one pass, and its backward g_x = keep ? g / (1 - p) : 0.
 * Element i is kept iff a counter-based hash of (seed, i) maps to >= p (keep probability 1 - p, as torch's dropout; not
 * torch's Philox stream), so no mask is stored: pass the SAME seed to the backward call.  n elements of float32,
 * 16-byte aligned pointers; y may alias x or identity. */
int selfocc_dropout_add_fwd(const float *x, const float *identity, float *y, int64_t n, float p, uint64_t seed, void *stream);
int selfocc_dropout_bwd(const float *g, float *g_x, int64_t n, float p, uint64_t seed, void *stream);

/* Compact second differences of the SDF volume (H, W, D) along h, w, d — NeuSHead's `second_grad`, the input of
 * SecondGradLoss (/root/reference/loss/second_grad_loss.py:6-19; this repo's declared compact form):
 * out = concat over the axes of ((s[2:] - 2 s[1:-1]) + s[:-2]).flatten(), selfocc_second_diff_size(H, W, D) floats (0: bad
 * shape), bit-identical to the torch expression; backward: g_sdf (H, W, D) = the transposed stencil applied to g_out, gather
 * form (deterministic, overwrites g_sdf).  Returns 0 / SELFOCC_ERR_*. */
size_t selfocc_second_diff_size(int32_t H, int32_t W, int32_t D);
int selfocc_second_diff_fwd(const float *sdf, float *out, int32_t H, int32_t W, int32_t D, void *stream);
int selfocc_second_diff_bwd(const float *g_out, float *g_sdf, int32_t H, int32_t W, int32_t D, void *stream);

/* ------------------------------------------------------------------------------------
 * SSIM term of the photometric losses (class SSIM, loss/reproj_loss_mono_multi_new_combine.py:26-66;
 * also loss/rgb_loss_ms.py): reflection pad 1, 3x3 means, out = clamp((1 - SSIM) / 2, 0, 1), (N, C, H, W).
 * x / y are addressed through element strides (n, c, h, w) — the call sites pass channel-last views; out,
 * g_out, g_x, g_y are contiguous.  g_x or g_y may be NULL.  H, W >= 2. */
int selfocc_ssim_fwd(const float *x, const float *y, const int64_t *x_strides, const int64_t *y_strides,
                     int32_t N, int32_t C, int32_t H, int32_t W, float *out, void *stream);
int selfocc_ssim_bwd(const float *x, const float *y, const int64_t *x_strides, const int64_t *y_strides,
                     int32_t N, int32_t C, int32_t H, int32_t W, const float *g_out, float *g_x, float *g_y,
                     void *stream);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the last dimension of a contiguous (rows, C) float32 tensor — the `norm` steps of
 * TPVFormerLayer / BEVFormerLayer (mmcv build_norm_layer(dict(type='LN')) in the reference:
 * model/encoder/tpvformer/tpvformer_encoder_layer.py, bevformer_encoder_layer.py), biased variance,
 * y = (x - mean) / sqrt(var + eps) * gamma + beta.  C a multiple of 4 in [4, 128].
 * mean / rstd (rows) are optional outputs of the forward (both or neither) and inputs of the backward.
 * The backward writes dx (rows, C), dgamma (C), dbeta (C) (overwritten, deterministic) and needs
 * selfocc_layernorm_bwd_workspace(rows, C) bytes of device scratch.
 * x, y, dy, dx, gamma and beta must be 16-byte aligned (the kernels move float4s): the forward and backward entries, grouped
 * and not, refuse any other pointer before anything is launched, and the message names it.
 * ---------------------------------------------------------------------------------- */
int selfocc_layernorm_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean,
                          float *rstd, int64_t rows, int32_t C, float eps, void *stream);
size_t selfocc_layernorm_bwd_workspace(int64_t rows, int32_t C);
int selfocc_layernorm_bwd(const float *x, const float *gamma, const float *mean, const float *rstd,
                          const float *dy, float *dx, float *dgamma, float *dbeta, int64_t rows, int32_t C,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Row groups of a (rows, C) tensor: group g owns rows row_start[g] .. row_start[g + 1] - 1.  1 <= n_groups <= 8,
 * row_start[0] = 0, non-decreasing, row_start[n_groups] = rows; a group may be empty.  Passed BY VALUE: host constants
 * that travel in the kernel arguments (no device upload, no synchronisation). */
typedef struct so_row_groups {
    int32_t n_groups;
    int64_t row_start[9];
} so_row_groups;

/* The LayerNorm above with one (gamma, beta) pair PER ROW GROUP — the reference's MultiPlaneNorm
 * (model/encoder/tpvformer/modules/split_norm.py: one norm layer per TPV plane) on the concatenated planes in ONE launch
 * per direction.  gamma / beta / dgamma / dbeta are (n_groups, C); x, y, dy, dx, mean, rstd as above.  A workgroup serves
 * rows of one group only; the backward keeps per-group partial sums and adds them in a fixed order (deterministic, no
 * atomics); an empty group gets dgamma = dbeta = 0.  With n_groups = 1 the results are bit-identical to the ungrouped
 * entry points.  selfocc_layernorm_grouped_supported: 1 / 0 / < 0 (bad table: message in selfocc_last_error()), host
 * logic only; every argument check of the other entries happens before anything touches the device. */
int selfocc_layernorm_grouped_supported(int64_t rows, int32_t C, so_row_groups groups);
int selfocc_layernorm_fwd_grouped(const float *x, const float *gamma, const float *beta, float *y, float *mean,
                                  float *rstd, int64_t rows, int32_t C, float eps, so_row_groups groups, void *stream);
size_t selfocc_layernorm_bwd_grouped_workspace(int64_t rows, int32_t C, so_row_groups groups);
int selfocc_layernorm_bwd_grouped(const float *x, const float *gamma, const float *mean, const float *rstd,
                                  const float *dy, float *dx, float *dgamma, float *dbeta, int64_t rows, int32_t C,
                                  so_row_groups groups, void *workspace, size_t workspace_bytes, void *stream);

/* The image features as the encoders' `value`: n_levels maps (B, N, C, h_l, w_l) float32 -> out (N, sum h_l w_l, B, C) with
 * out[n][start_l + p][b][c] = (feats[l][b][n][c][p] + cams_embeds[n][c]) + level_embeds[l][c]
 * (/root/reference/model/encoder/tpvformer/tpvformer_encoder.py:261-277, bevformer/bevformer_encoder.py:194-210: two
 * broadcast adds per level + cat + permute).  `feats`: HOST array of n_levels device pointers; host_hw[l] = h_l * w_l.
 * 1 <= n_levels <= 8, C <= 512.  Returns 0 / SELFOCC_ERR_*. */
int selfocc_flatten_feats(const float *const *feats, const int32_t *host_hw, int32_t n_levels, int32_t B, int32_t N, int32_t C,
                          const float *cams_embeds, const float *level_embeds, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * CameraAwareSE fused with the flatten above (model/encoder/tpvformer/modules/camera_se_net.py and its call site
 * tpvformer_encoder.py:258-277): the per-camera gate and the 1x1 `context_conv`, then the camera / level embeddings, as ONE
 * batched GEMM from the maps as they lie in memory to the encoders' `value`:
 *     out[n][start_l + p][b][c] = sum_k w[c][k] gate[b*N+n][k] feats[l][b][n][k][p] + bias[c] + cams_embeds[n][c] + level_embeds[l][c]
 * feats: HOST array of n_levels device pointers to (B, N, M, h_l, w_l) float32 maps, host_hw[l] = h_l * w_l >= 1 (any
 * pixel count); gate (B*N, M); w (C, M); bias (C); cams_embeds (N, C); level_embeds (>= n_levels, C); out (N, sum hw, B, C).
 * Backward, from g = d out (N, sum hw, B, C):
 *     d_feats[l][b][n][k][p] = sum_c w[c][k] gate[b*N+n][k] g[n][start_l + p][b][c]      (d_feats NULL or d_feats[l] NULL: skipped)
 *     dwc[b*N+n][c][k]       = sum_{l, p} g[n][start_l + p][b][c] feats[l][b][n][k][p]   (the UNGATED map; (B*N, C, M))
 *     colsum[l][n][c]        = sum_{p in level l, b} g[n][start_l + p][b][c]             ((n_levels, N, C))
 * from which the caller folds d w = sum_bn dwc * gate, d gate = sum_c dwc * w, d bias / d embeddings = sums of colsum.
 * float32 (v_mfma_f32_16x16x4_f32: exact fmaf chains); the backward is deterministic (chunk partials in `workspace`, added in
 * a fixed order; no float atomics).  Maps, gradients, out, g and the workspace must be 16-byte aligned.
 * supported (selfocc_camera_se_supported: 1 / 0, host logic only): C in {32, 64, 96, 128}, M = C or 2 C with M <= 192,
 * 1 <= n_levels <= 8, B, N >= 1 with B * N < 65535.  workspace: selfocc_camera_se_flatten_bwd_workspace(...) bytes (0: unsupported).
 * Returns 0 / SELFOCC_ERR_*; every argument check happens before anything touches the device.
 * ---------------------------------------------------------------------------------- */
int selfocc_camera_se_supported(int32_t B, int32_t N, int32_t C, int32_t M, int32_t n_levels);
int selfocc_camera_se_flatten_fwd(const float *const *feats, const int32_t *host_hw, int32_t n_levels, int32_t B, int32_t N,
                                  int32_t C, int32_t M, const float *gate, const float *w, const float *bias,
                                  const float *cams_embeds, const float *level_embeds, float *out, void *stream);
size_t selfocc_camera_se_flatten_bwd_workspace(const int32_t *host_hw, int32_t n_levels, int32_t B, int32_t N, int32_t C,
                                               int32_t M);
int selfocc_camera_se_flatten_bwd(const float *g, const float *const *feats, const int32_t *host_hw, int32_t n_levels, int32_t B,
                                  int32_t N, int32_t C, int32_t M, const float *gate, const float *w, float *const *d_feats,
                                  float *dwc, float *colsum, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * The three tall-Linear passes below with one weight PER ROW GROUP (so_row_groups, by value) — the reference's MultiPlaneFFN
 * (model/encoder/tpvformer/modules/split_fpn.py: one mmcv FFN per TPV plane) on the concatenated planes, ONE launch each:
 * group g's rows use w[g] (N, K), bias[g] (N), and write dw[g] (N, K), db[g] (N).  The kernels are the ungrouped ones with a
 * group selection in front: a workgroup (forward / dgrad: a persistent block; wgrad: a row chunk) serves rows of one group
 * only, so W is staged once per block and a chunk never straddles a group; the wgrad's fixed-order reduction runs per group
 * (an empty group gets dw = db = 0).  Deterministic, no atomics.  Every other argument is its ungrouped twin's.
 *   forward: w_group_stride = N * K (weights and biases stacked on a leading axis) or 0 (one shared w / bias);
 *            ln_group_stride = N (ln_gamma / ln_beta stacked) or 0 (shared): a shared projection followed by a per-group
 *            LayerNorm is one launch too.
 *   dgrad:   workspace = selfocc_linear_dgrad_grouped_workspace(N, K, groups) bytes (every group's split planes of W^T).
 *   wgrad:   workspace = selfocc_linear_wgrad_grouped_workspace(T, N, K, groups) bytes.
 * *_grouped_supported: 1 / 0 / < 0 (bad table), host logic only; argument checks come before anything touches the device.
 * ---------------------------------------------------------------------------------- */
int selfocc_linear_fwd_grouped_supported(int64_t T, int32_t N, int32_t K, so_row_groups groups);
int selfocc_linear_fwd_grouped(const float *x, const float *w, const float *bias, const float *residual, int32_t ldr,
                               const float *ln_gamma, const float *ln_beta, float ln_eps, float *y, int32_t ldy, float *y_pre,
                               float *mean, float *rstd, int64_t T, int32_t N, int32_t K, uint32_t flags, so_row_groups groups,
                               int64_t w_group_stride, int64_t ln_group_stride, void *stream);
int selfocc_linear_dgrad_grouped_supported(int64_t T, int32_t N, int32_t K, so_row_groups groups);
size_t selfocc_linear_dgrad_grouped_workspace(int32_t N, int32_t K, so_row_groups groups);
int selfocc_linear_dgrad_grouped(const float *dy, const float *w, float *dx, int64_t T, int32_t N, int32_t K, so_row_groups groups,
                                 void *workspace, int64_t workspace_bytes, void *stream);
int selfocc_linear_wgrad_grouped_supported(int64_t T, int32_t N, int32_t K, so_row_groups groups);
size_t selfocc_linear_wgrad_grouped_workspace(int64_t T, int32_t N, int32_t K, so_row_groups groups);
int selfocc_linear_wgrad_grouped(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                                 so_row_groups groups, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * point_sampling of the TPV / BEV encoders (model/encoder/bevformer/utils.py:114-170): project the pillar reference
 * points into every camera.
 *   ref (B, D, Q, 3) metres; lidar2img (B, N, 4, 4) row-major; focal_x / focal_y (N) or NULL (the reference's
 *   optional `focal_ratios_*` metas); img_h / img_w = metas['img_shape'][:2]
 *   cam (N, B, Q, D, 2): (u / img_w, v / img_h) (x focal ratios), u = c0 / max(c2, 1e-5), c = lidar2img (x, y, z, 1)
 *   mask (N, B, Q, D) u8: c2 > 1e-5 and 0 < u, v < 1 (before the focal ratios, as in the reference)
 *   visible (N, B, Q) u8 or NULL: mask.any(-1)
 * The image-augmentation branch (post_rots / post_trans) stays host-side torch.
 * ---------------------------------------------------------------------------------- */
int selfocc_point_sampling(const float *ref, const float *lidar2img, const float *focal_x, const float *focal_y,
                           float *cam, uint8_t *mask, uint8_t *visible, int32_t B, int32_t D, int32_t Q, int32_t N,
                           float img_h, float img_w, void *stream);

/* ------------------------------------------------------------------------------------
 * Weight and bias gradient of a Linear layer with very many rows (the encoder's projections: 66 k - 180 k rows,
 * K = 96 / 192 inputs, N = 96 .. 2304 outputs; torch autograd through mmcv / nn.Linear in the reference, e.g.
 * model/encoder/tpvformer/attention/image_cross_attention.py:130-160) in one pass over dy and x:
 *     dw (N, K) = dy (T, N)^T x (T, K)          db (N) = column sums of dy   (db may be NULL)
 * float32 (MFMA f32 = exact fmaf chains), deterministic (fixed summation order).  K must be 32, 64, 96, 128 or 192
 * (selfocc_linear_wgrad_supported); workspace = selfocc_linear_wgrad_workspace(T, N, K) bytes of device scratch.
 * ---------------------------------------------------------------------------------- */
int selfocc_linear_wgrad_supported(int64_t T, int32_t N, int32_t K);
size_t selfocc_linear_wgrad_workspace(int64_t T, int32_t N, int32_t K);
int selfocc_linear_wgrad(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------
 * Forward of the same tall-skinny projections with the elementwise steps that follow them in TPVFormerLayer /
 * BEVFormerLayer folded into the epilogue (mmcv Linear / FFN / build_norm_layer(dict(type='LN')) under torch in the
 * reference: model/encoder/bevformer/attention/image_cross_attention.py:130-136 `output_proj` + `dropout(slots) +
 * residual`, mmcv FFN `identity + layers(x)`, tpvformer/tpvformer_encoder_layer.py:150-219 `norm`):
 *     y (T, N; row stride ldy) = LN?( relu?( x (T, K) w (N, K)^T + bias ) + residual (T, N; row stride ldr) )
 *   bias, residual: NULL = absent.  flags: SO_LINEAR_RELU (applied before the residual, as FFN does).
 *   ln_gamma / ln_beta (N) non-NULL: LayerNorm over the N outputs (biased variance, eps = ln_eps), N <= 96; then the
 *   optional outputs y_pre (T, N: the LayerNorm input), mean / rstd (T) are what selfocc_layernorm_bwd consumes.
 * float32 (MFMA f32 = exact fmaf chains; only the summation order differs from a BLAS).  K must be 32, 64, 96, 128
 * or 192 (selfocc_linear_fwd_supported).
 * ---------------------------------------------------------------------------------- */
enum { SO_LINEAR_RELU = 1, SO_LINEAR_BF16X1 = 2 };
/* SO_LINEAR_BF16X1 — the opt-in one-product bfloat16 mode of every tall-Linear pass (off by default; Python: LINEAR_BF16).
 * Definition: with the flag a pass computes exactly what it computes without it on the operands bf16_rne(a), bf16_rne(b) taken
 * as float32 values (bf16_rne = round to nearest even, the (__bf16) conversion so_split3 uses for its first plane):
 *     forward  y  = LN?( relu?( x^ W^^T + bias ) + residual )
 *     dgrad    dx = dy^ W^
 *     wgrad    dW = dy^^T x^,   db = the column sums of the ROUNDED dy^
 * bias, residual, gamma and beta stay float32 and unrounded; outputs are float32; accumulation is float32 in the kernel's own
 * order; the epilogues are the default's.  ONE bf16 MFMA per 32 k instead of the six of the exact three-way split, one
 * conversion per loaded value instead of the split, one W plane in LDS (forward) or in the workspace (dgrad): about three
 * decimal digits (2^-9 relative per operand) for less arithmetic.  What the flag computes does not depend on the shape through
 * the dispatch: a flagged launch ALWAYS runs a one-product kernel — the f32-MFMA kernels (linear_fwd16_kernel,
 * linear_wgrad_kernel) never serve it, SELFOCC_LINEAR_B3=0 does not apply to it, and the wgrad at K = 128, which the default
 * leaves to the f32-MFMA kernel, has one-product instances of its own (the decision taken for K = 128: built, not refused; K = 192
 * runs as two halves of three column tiles with the default's one tile row).  So every *_supported query answers the same for both
 * modes and has no flagged twin.  The flag is bit 2 of the `flags` of selfocc_linear_fwd / _fwd_heads / _fwd_grouped; the
 * backward passes take it through the *_flags twins below (the entries without `flags` are those with flags = 0).  The twins
 * refuse any other bit ("unknown flags"); the *_workspace_flags queries then return 0.  Workspaces: dgrad a third of the
 * default's; wgrad never more than the default's (the default sizes are valid upper bounds). */
int selfocc_linear_fwd_supported(int64_t T, int32_t N, int32_t K);
int selfocc_linear_fwd(const float *x, const float *w, const float *bias, const float *residual, int32_t ldr,
                       const float *ln_gamma, const float *ln_beta, float ln_eps, float *y, int32_t ldy, float *y_pre,
                       float *mean, float *rstd, int64_t T, int32_t N, int32_t K, uint32_t flags, void *stream);
/* The `value_proj` of the deformable attentions (image_cross_attention.py:262-266, mmcv MultiScaleDeformableAttention)
 * with the output written HEAD-MAJOR, the layout the MSDA kernels gather fastest from (SO_VALUE_HEAD_MAJOR), by the
 * projection itself:  x (T, K) = T / nv batch items (cameras) of nv pixels;  N = G * 96 output columns = G groups (one
 * attention module each: e.g. the three TPV planes' value_proj stacked) of 6 heads x 16 channels;
 *     y (G, T / nv, 6, nv, 16):   y[g][b][h][pix][c] = relu?(x[b * nv + pix] . w[96 g + 16 h + c] + bias[...])
 * nv >= 16, T a multiple of nv, T * N < 2^31, y 16-byte aligned (written as float4).  flags: SO_LINEAR_RELU. */
int selfocc_linear_fwd_heads(const float *x, const float *w, const float *bias, float *y, int64_t T, int32_t N, int32_t K,
                             int32_t nv, uint32_t flags, void *stream);

/* Input gradient of a tall Linear: dx (T, K) = dy (T, N) W (N, K), W as nn.Linear stores it (out_features N x in_features K).
 * Replaces the `grad_output @ weight` GEMM torch's autograd runs for every nn.Linear of the encoder
 * (/root/reference/model/encoder/tpvformer/tpvformer_encoder.py:257-291 -> mmcv FFN / MSDeformableAttention projections,
 * /root/reference/model/encoder/tpvformer/attention/image_cross_attention.py:296-345); same bf16 three-way split as
 * selfocc_linear_fwd (float32-level accuracy); W is split and transposed into `workspace` first (one tiny launch), the
 * reduction over N then runs in 32-wide steps with dy streamed once.
 * supported: N % 8 == 0, 8 <= N <= 4096; K in {96, 192, 288, 384}.  Returns 0 / SELFOCC_ERR_*. */
int selfocc_linear_dgrad_supported(int64_t T, int32_t N, int32_t K);
size_t selfocc_linear_dgrad_workspace(int32_t N, int32_t K);   /* bytes: the three bf16 planes of W^T, 16-byte aligned */
int selfocc_linear_dgrad(const float *dy, const float *w, float *dx, int64_t T, int32_t N, int32_t K, void *workspace,
                         int64_t workspace_bytes, void *stream);

/* The backward passes with `flags` (0 or SO_LINEAR_BF16X1, see there): the entries above and the grouped ones are these with
 * flags = 0.  workspace: the matching *_workspace_flags(..., flags) bytes.  Every argument check — unknown flag bits, shape,
 * NULL pointers, workspace size — happens on the host before anything touches the device. */
size_t selfocc_linear_dgrad_workspace_flags(int32_t N, int32_t K, uint32_t flags);
int selfocc_linear_dgrad_flags(const float *dy, const float *w, float *dx, int64_t T, int32_t N, int32_t K, void *workspace,
                               int64_t workspace_bytes, uint32_t flags, void *stream);
size_t selfocc_linear_dgrad_grouped_workspace_flags(int32_t N, int32_t K, so_row_groups groups, uint32_t flags);
int selfocc_linear_dgrad_grouped_flags(const float *dy, const float *w, float *dx, int64_t T, int32_t N, int32_t K,
                                       so_row_groups groups, void *workspace, int64_t workspace_bytes, uint32_t flags, void *stream);
size_t selfocc_linear_wgrad_workspace_flags(int64_t T, int32_t N, int32_t K, uint32_t flags);
int selfocc_linear_wgrad_flags(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                               void *workspace, size_t workspace_bytes, uint32_t flags, void *stream);
size_t selfocc_linear_wgrad_grouped_workspace_flags(int64_t T, int32_t N, int32_t K, so_row_groups groups, uint32_t flags);
int selfocc_linear_wgrad_grouped_flags(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                                       so_row_groups groups, void *workspace, size_t workspace_bytes, uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------
 * Fused temporal reprojection photometric term: replaces the per-sample part of
 * ReprojLossMonoMultiNewCombine.reproj_loss (loss/reproj_loss_mono_multi_new_combine.py
 * :108-187 and the weighted colour composite :190-201) for one camera.
 * so_reproj_args is the planar 3-channel form of so_reproj_c_args (below, which states the
 * semantics): C = 3, curr_rgb / rgb_combine are its curr / combine, and
 *   img_* (3, Hi, Wi) planar float32, of ANY base alignment (no img_stride).
 * Both forms run one kernel and share every refusal but those of C, img_stride and the
 * image alignment, which the planar form cannot fail.
 * ---------------------------------------------------------------------------------- */
typedef struct so_reproj_args {
    const float *weights, *ts, *deltas; /* deltas may be NULL (:111-116)               */
    const float *pix, *curr_rgb;
    const float *T_prev, *T_next;
    const float *img_prev, *img_next;
    int32_t R, S, Hi, Wi;
    float img_h, img_w;                 /* self.img_size used for masks + normalisation */
    float *l1, *rgb_combine, *any_valid;
    float *wnorm;                       /* (R, S) renormalised weights, saved for bwd   */
} so_reproj_args;

int selfocc_reproj_fwd(const so_reproj_args *args, void *stream);

/* d loss / d weights given d loss / d l1 and d loss / d rgb_combine. */
int selfocc_reproj_bwd(const so_reproj_args *args, const float *g_l1,
                       const float *g_rgb_combine, float *g_weights, void *stream);

/* ------------------------------------------------------------------------------------
 * The fused temporal reprojection term on images of C channels (the `dims` knob of both reprojection losses, e.g. the
 * feature-metric loss on (C, Hi, Wi) feature maps).  This comment is the contract of selfocc_reproj_fwd / _bwd as well.
 *   weights, ts (R, S); deltas (R, S) or NULL; pix (R, 2) pixel (u, v); curr (R, C) = the current image at the ray pixels;
 *   T_prev / T_next (4,4) row-major; img_prev / img_next CHANNEL-LAST (Hi, Wi, img_stride) float32, base 16-byte aligned,
 *   img_stride % 4 == 0 and >= C.  Channels C .. img_stride-1 of a pixel are padding: no output depends on them (a NaN
 *   there reaches none).
 * Projection, perspective divide (eps 1e-5), in-image masks against (img_h, img_w), w / delta, general-mask zeroing, the
 * clamped per-ray renormalisation and any_valid read no image: `wnorm` and `any_valid` are bit for bit those of
 * selfocc_reproj_fwd on the same geometry, at every C.  Per sample and frame f the warped value is
 * grid_sample(bilinear, border, align_corners=True) of the frame's image at pixel / (img_w, img_h), and
 *   diff_f = (sum_c |curr_c - warped_c|) / C,   diff = (m_prev diff_prev + m_next diff_next) / max(m_prev + m_next, 1),
 *   comb_c = (m_prev warped_prev_c + m_next warped_next_c) / max(m_prev + m_next, 1),
 *   l1 = sum_s w'_s diff_s,   combine_c = sum_s w'_s comb_s,c      (w' = masked, per-ray renormalised weights).
 * Backward: g_weights_s = sc_s (a_s - abar) / wtot with a_s = g_l1 diff_s + g_combine . comb_s, abar = sum_s w'_s a_s
 * (0 when the weight sum sits on its clamp), sc_s the sample's 1 / delta (1 without deltas; 0 when masked); the taps are
 * recomputed, nothing per-sample is stored by the forward.  g_l1 / g_combine may be NULL (taken as zero).
 * No floating-point atomics: results are run-to-run identical.  l1 / combine / any_valid / wnorm may each be NULL.
 * Refused on the host, before any HIP call, by name in selfocc_last_error(): C outside 1..512; img_stride < C or not a
 * multiple of 4; S outside 1..512; a NULL input; an image base that is not 16-byte aligned; a bad image size (Hi, Wi
 * outside 1..2^24, img_h or img_w <= 0); g_weights NULL in the backward.  R == 0 succeeds without a launch (after the
 * checks of C, img_stride and S).  New entry points: SELFOCC_ABI_VERSION is unchanged.
 * ---------------------------------------------------------------------------------- */
typedef struct so_reproj_c_args {
    const float *weights, *ts, *deltas;   /* (R, S); deltas may be NULL                                  */
    const float *pix, *curr;              /* (R, 2) pixel (u, v); (R, C) current image at the ray pixels */
    const float *T_prev, *T_next;         /* (4, 4) row-major                                            */
    const float *img_prev, *img_next;     /* CHANNEL-LAST (Hi, Wi, img_stride) float32, 16-byte aligned  */
    int32_t R, S, Hi, Wi, C, img_stride;  /* 1 <= C <= 512; img_stride % 4 == 0, img_stride >= C         */
    float img_h, img_w;
    float *l1, *combine, *any_valid;      /* (R), (R, C), (R)                                            */
    float *wnorm;                         /* (R, S) or NULL                                              */
} so_reproj_c_args;

int selfocc_reproj_c_fwd(const so_reproj_c_args *args, void *stream);

int selfocc_reproj_c_bwd(const so_reproj_c_args *args, const float *g_l1, const float *g_combine /* (R, C) */,
                         float *g_weights /* (R, S) */, void *stream);

/* ------------------------------------------------------------------------------------
 * Per ray and temporal frame, the sample with the largest warped-photometric weight, and a per-sample value read
 * there: the sdf_loss term of ReprojLossMonoMultiNew (loss/reproj_loss_mono_multi_new.py:265-270).  One launch per
 * camera serves both frames; no image is read.
 *   weights, ts, values (R, S); deltas (R, S) or NULL; pix (R, 2); T_prev / T_next (4,4) row-major; 1 <= S <= 512.
 * For frame f (0 = prev, 1 = next) wn_i is bit for bit the `wnorm` selfocc_reproj_fwd writes for the same inputs
 * when the other frame's transform maps behind the camera (ts > 0), and
 *   j = 0, best = wn_0;  for i = 1 .. S-1: if (wn_i > best) { best = wn_i; j = i; }
 * (smallest index among equal maxima; 0 for a fully masked ray; a NaN never wins).
 *   pick_index[r][f] = j,  pick_value[r][f] = values[r * S + j].
 * R == 0 succeeds without a launch (after the argument checks).  New entry points: SELFOCC_ABI_VERSION is unchanged.
 * ---------------------------------------------------------------------------------- */
typedef struct so_reproj_pick_args {
    const float *weights, *ts, *deltas; /* deltas may be NULL                           */
    const float *values;                /* (R, S) what is read at the pick (sample SDF) */
    const float *pix;
    const float *T_prev, *T_next;
    int32_t R, S;
    float img_h, img_w;
    int32_t *pick_index;                /* (R, 2)                                       */
    float *pick_value;                  /* (R, 2)                                       */
} so_reproj_pick_args;

int selfocc_reproj_pick_fwd(const so_reproj_pick_args *args, void *stream);

/* dense d loss / d values (R, S), every element written: zero, plus g_pick_value[r][f] at pick_index[r][f] (the two
 * summed where both frames picked the same sample).  No memset, no atomics. */
int selfocc_reproj_pick_bwd(const int32_t *pick_index, const float *g_pick_value, float *g_values, int32_t R, int32_t S,
                            void *stream);

/* ------------------------------------------------------------------------------------
 * Depth-evaluation metric tail: DepthMetric._after_step (utils/metric_util.py:247-349) and
 * compute_depth_errors_torch (:424-444) for one frame, in ONE launch (one workgroup per camera).
 *   pred (N, h, w) f32 rendered depth; loc (N, n, 2) f32 normalised (u, v), 8-byte aligned;
 *   gt (N, n) f32; mask (N, n) u8, nonzero = valid.  n < 2^24 (counts exact in f32).
 * Gather: bit-identical to torch's GPU F.grid_sample(pred, loc * 2 - 1, bilinear, border,
 * align_corners=True).  Median: lower median of the masked gt / sampled pred (torch.median).
 * Outputs (each optional; at least one requested):
 *   accumulators: abs_rel .. a3, scaling (n_types, N) f32 and count (1,) f32, added into (+=),
 *     row raw_row for 'raw', median_row for 'median' (-1: type not evaluated); all or none;
 *   errors (N, 7) f32 = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 of the raw prediction;
 *   sampled (N, n) f32 = the gathered depth at every location;
 *   medians (N, 2) f32 = (median gt, median sampled pred) of the masked points.
 * A camera with no valid point gives NaN for its metric entries (its 'raw' scaling still
 * counts 1).  ws: selfocc_depth_metric_ws_bytes(args) bytes of device memory (NULL if 0).
 * ---------------------------------------------------------------------------------- */
typedef struct so_depth_metric_args {
    const float *pred;
    const float *loc;
    const float *gt;
    const uint8_t *mask;
    int32_t N, h, w, n;
    int32_t n_types, raw_row, median_row, _pad;
    float *abs_rel, *sq_rel, *rmse, *rmse_log, *a1, *a2, *a3, *scaling;
    float *count;
    float *errors;
    float *sampled;
    float *medians;
    void *ws;
    uint64_t ws_bytes;
} so_depth_metric_args;

size_t selfocc_depth_metric_ws_bytes(const so_depth_metric_args *args);
int selfocc_depth_metric(const so_depth_metric_args *args, void *stream);

/* ------------------------------------------------------------------------------------
 * Occupancy metric tail of eval_iou_kitti.py (:166-190): the counters of IoU (utils/metric_util.py:168-233),
 * SSCMetrics (utils/scenerf_metric.py:43-188) and, optionally, MeanIoU (selfocc_iou_counts layout) in ONE
 * streaming pass over an (H, W, D) volume, n = H * W * D < 2^31.  Every counter is exact int64, added (+=).
 *   prediction p: pred (integer, pred_dtype SO_LBL_U8 / I32 / I64; bool = u8) OR sdf f32 with
 *     p = (sdf <= thresh) (NaN -> 0) and crop {lo_h, hi_h, lo_w, hi_w, lo_d, hi_d}: index i_k outside
 *     [lo_k, n_k - hi_k) -> 0 (as so_occ_args.crop).  occ (n) int32 receives that p (sdf form only).
 *   label t: gt of gt_dtype (SO_LBL_F32 / U8 / I32 / I64), read at (h, W - 1 - w, d) when flip_gt.  A float
 *     label that is not an integer equals no class; it is > 0 / == 0 / == 255 as the float compares.
 *   iou (3) seen, correct, positive: over voxels inside iou_mask (NULL: all), seen = #(t != iou_empty and
 *     t != iou_ignore; iou_ignore < 0: no ignore label), correct = sum of p over the seen voxels, positive =
 *     sum of p.  Kitti form: iou_empty = 0, iou_ignore = 255; Occ3D form: 17, -1.
 *   completion (3) tp, fp, fn of (t > 0, p > 0); semantic (3, n_classes) tp, fp, fn per class j < n_classes
 *     (1 <= n_classes <= 256): t == p in range -> tp[t]; else fp[p], fn[t] for those in range.  Both over the
 *     voxels with nonempty (NULL: all) and t != 255; completion also needs nonsurface.  ssc_keep255 = 1 counts a
 *     t == 255 voxel as (t, p) = (0, 0) instead (SSCMetrics.get_score_* called directly).
 *   miou (3, n_miou + 1), the MeanIoU counts of p_m = p * lut[sem] against t over t != 255: miou_map (256)
 *     maps a label value to its column (-1: none; injective), column n_miou is t / p_m != miou_empty.  sem
 *     (n) int64 indexes lut (n_lut entries, negative from the end); an index out of range gives p_m = 0 and
 *     counts into bad (if given).
 *   d_range (2) int32: (min, max) of the d index over t not in {0, 255}, (-1, -1) if none; needs ws.
 *   ws (4) uint32 device scratch, zero before the first call; every call leaves it zero again.  Calls that
 *     share a ws must be ordered (one stream).
 * At least one of iou / completion / semantic / miou / d_range / occ.  No host synchronisation. */
enum { SO_LBL_F32 = 0, SO_LBL_U8 = 1, SO_LBL_I32 = 2, SO_LBL_I64 = 3 };

typedef struct so_ssc_metric_args {
    int32_t H, W, D;
    int32_t pred_dtype;
    const void *pred;
    const float *sdf;
    float thresh;
    int32_t crop[6];
    int32_t gt_dtype;
    const void *gt;
    int32_t flip_gt;
    int32_t iou_empty, iou_ignore;
    int32_t n_classes;
    int32_t ssc_keep255;
    int32_t n_lut;
    const uint8_t *nonempty;
    const uint8_t *nonsurface;
    const uint8_t *iou_mask;
    const int64_t *sem;
    const int32_t *lut;
    const int32_t *miou_map;
    int32_t n_miou, miou_empty;
    const int64_t *coords; /* (n_coords, 3): selfocc_iou_coords only */
    int64_t n_coords;
    unsigned long long *iou;
    unsigned long long *completion;
    unsigned long long *semantic;
    unsigned long long *miou;
    unsigned long long *bad;
    int32_t *d_range;
    int32_t *occ;
    uint32_t *ws;
} so_ssc_metric_args;

int selfocc_ssc_metric(const so_ssc_metric_args *args, void *stream);

/* IoU._after_step(outputs, coords) (metric_util.py:189-199): iou[0] += n_coords, iou[1] += sum of pred at the
 * (n_coords, 3) int64 rows of coords (each in [-size, size) along (H, W, D), negative from the end, duplicates
 * counted as often as they occur), iou[2] += sum of pred.  A row out of range is skipped and counted into bad
 * (required).  Uses H, W, D, pred, pred_dtype, coords, n_coords, iou, bad. */
int selfocc_iou_coords(const so_ssc_metric_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SELFOCC_HIP_H */
