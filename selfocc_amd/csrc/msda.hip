// msda.hip — multi-scale deformable attention sampling for gfx950 (MI355X).
//
// Drop-in for mmcv==2.0.1 MultiScaleDeformableAttnFunction (ms_deform_attn_forward /
// _backward) at the reference call sites
//   model/encoder/bevformer/attention/image_cross_attention.py:340-342
//   model/encoder/tpvformer/attention/cross_view_hybrid_attention.py:111-113
//
//   out[b,q,h*D+c] = sum_{l,p} A[b,q,h,l,p] * bilinear(V_l[b, :, h, c], loc[b,q,h,l,p])
//   h_im = loc_y * H_l - 0.5, w_im = loc_x * W_l - 0.5, zero padding outside the map.
//
// Hardware mapping (not mmcv's thread-per-output-channel): A LANE OWNS A SAMPLING POINT, A TEAM GATHERS IT.
//   * the L*P points of one (b, q, head) are consecutive in memory, so the loc / attw (or raw offset /
//     logit) streams — ~80 % of the compulsory bytes — are read fully coalesced, once, and the bilinear
//     set-up is done once per point, not once per channel lane;
//   * d/4 adjacent lanes (a channel team) walk through their d/4 points together, each lane fetching its own
//     16-byte quarter of every corner: a wave-level load touches 16 corner segments instead of 64 (the L1 tag
//     rate, not bytes, bounds the gather); the point record travels through the team with DPP quad permutes;
//   * the teams of a group combine with a static reduce-scatter over wavefront shuffles;
//   * fused forms do the reference's prologue (softmax, loc = ref + off / (W, H)) in registers, in inference
//     and training; the camera-loop forms replace BEVCrossAttention's re-batch / scatter-add / mean;
//   * backward: a point kernel (grad_loc / grad_attw or the raw-output gradients; keys + records in band
//     order) and a banded, output-stationary scatter of grad_value through ds_add_f64 in LDS — no global atomics
//     in the scatter (selfocc_msda_bwd keeps the global-atomic form for callers without host shapes / workspace).
#include "so_device.h"
#include <algorithm>
#include <type_traits>

namespace {

#include "msda_device.h"

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
template <int D, int LOGG>
__global__ __launch_bounds__(256) void msda_fwd_kernel(const float *__restrict__ value,
                                                       const int32_t *__restrict__ shapes,
                                                       const int32_t *__restrict__ starts,
                                                       const float *__restrict__ loc,
                                                       const float *__restrict__ attw,
                                                       float *__restrict__ out, MsdaDims dm) {
    constexpr int G = 1 << LOGG;             // lanes per (b, q, head) group; host: G >= QL
    constexpr int QL = D / 4, LOGQ = so_ilog2(QL);
    constexpr int NJ = LOGG > LOGQ ? LOGG - LOGQ : 0;
    const int LP = dm.L * dm.P;
    const int groups_per_block = 256 / G;
    const long long n_groups = (long long)dm.bs * dm.nq * dm.heads;
    const long long gid = (long long)so_xcd_block() * groups_per_block + (threadIdx.x / G);
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < n_groups;  // whole groups are live or dead; exchanges stay in-group
    int h, b;
    long long bq, gq;
    so_split_group_head_outer(live ? gid : 0, dm, h, b, bq, gq);
    const int pix_stride = so_pix_stride(dm, D);
    const int s = gl & (QL - 1);
    const float *vb = value + so_value_base(dm, D, b, h, 0) + 4 * s;

    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r0 = 0; r0 < LP; r0 += G) {   // uniform trip count: the team exchanges need every lane
        const int pt = r0 + gl;
        MsdaPoint mp = so_point_none();
        if (live && pt < LP) {
            const int l = so_level_of(pt, dm.P, dm.L);
            const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
            const size_t idx = (size_t)gq * LP + pt;
            const float2 xy = *(const float2 *)(loc + 2 * idx);
            mp = so_point_setup(xy.x, xy.y, attw[idx], Hl, Wl, starts[l] * pix_stride, pix_stride);
        }
        so_team_gather<D>(vb, mp, acc);
    }
    so_group_reduce_store<NJ, LOGQ>(acc, gl >> LOGQ, live, out + (size_t)gq * D + 4 * s);
}

// ---------------------------------------------------------------------------------------
// fused forward (inference): the prologue the reference runs as separate torch kernels around the
// op — softmax over the L*P attention logits of a (query, head) and
// loc = reference + offset / (W_l, H_l) (bevformer/attention/image_cross_attention.py:314-328,
// tpvformer/attention/cross_view_hybrid_attention.py:88-99) — happens in registers, so the
// 100-400 MB `sampling_locations` / `attention_weights` tensors are never written or re-read.
//   ref_kind 0: ref (bs, nq, L, 2)      (mmcv base class)
//            1: ref (bs, nq, P, 2)      (one anchor per point, all levels: BEVDeformableAttention)
//            2: ref (bs, nq, L, P, 2)   (CrossViewHybridAttention)
// ---------------------------------------------------------------------------------------
template <int D, int LOGG, typename VT>
__global__ __launch_bounds__(256, SO_MSDA_FWD_WAVES(D)) void msda_fused_fwd_kernel(const VT *__restrict__ value,
                                                             const int32_t *__restrict__ shapes,
                                                             const int32_t *__restrict__ starts,
                                                             const float *__restrict__ ref, int ref_kind,
                                                             const float *__restrict__ off_raw,
                                                             const float *__restrict__ logits,
                                                             float *__restrict__ out, MsdaDims dm) {
    constexpr int G = 1 << LOGG;
    constexpr int QL = D / 4, LOGQ = so_ilog2(QL);
    constexpr int NJ = LOGG > LOGQ ? LOGG - LOGQ : 0;
    constexpr int MAXR = so_maxr(LOGG);   // points per lane (host guarantees L * P <= MAXR * G)
    const int LP = dm.L * dm.P;
    const int groups_per_block = 256 / G;
    const long long n_groups = (long long)dm.bs * dm.nq * dm.heads;
    const long long gid = (long long)so_xcd_block() * groups_per_block + (threadIdx.x / G);
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < n_groups;
    int h, b;
    long long bq, gq;                                   // b * nq + q; (b, q, h) index of the group
    so_split_group_head_outer(live ? gid : 0, dm, h, b, bq, gq);
    const int pix_stride = so_pix_stride(dm, D);
    const int s = gl & (QL - 1);
    const VT *vb = value + so_value_base(dm, D, b, h, 0) + 4 * s;

    // softmax over the group's L * P logits
    float lg[MAXR];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? logits[so_lg_index(dm, bq, h, LP, pt)] : -INFINITY;
        mx = fmaxf(mx, lg[r]);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float den = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        lg[r] = (gl + r * G < LP) ? __expf(lg[r] - mx) : 0.0f;
        den += lg[r];
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) den += __shfl_xor(den, m, 64);
    const float iden = 1.0f / den;

    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        if (r * G >= LP) break;   // uniform
        const int pt = gl + r * G;
        MsdaPoint mp = so_point_none();
        if (live && pt < LP) {
            const int l = so_level_of(pt, dm.P, dm.L);
            const int pp = pt - l * dm.P;
            const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
            const float2 o = *(const float2 *)(off_raw + so_off_index(dm, bq, h, LP, pt));
            size_t ri;
            if (ref_kind == 1) ri = (size_t)bq * dm.P + pp;
            else if (ref_kind == 2) ri = ((size_t)bq * dm.L + l) * dm.P + pp;
            else ri = (size_t)bq * dm.L + l;
            const float2 rf = *(const float2 *)(ref + 2 * ri);
            const float lx = rf.x + o.x / (float)Wl, ly = rf.y + o.y / (float)Hl;
            mp = so_point_setup(lx, ly, lg[r] * iden, Hl, Wl, starts[l] * pix_stride, pix_stride);
        }
        so_team_gather<D>(vb, mp, acc);
    }
    so_group_reduce_store<NJ, LOGQ>(acc, gl >> LOGQ, live, out + (size_t)gq * D + 4 * s);
}

// ---------------------------------------------------------------------------------------
// camera-loop forward (inference) — the whole of BEVCrossAttention's sampling stage
// (bevformer/attention/image_cross_attention.py:90-136) in one launch.  The reference re-batches the
// queries each camera sees into (cams, max_len) (a host sync for max_len, python double loops), runs the
// offset / weight linears and MSDA on the padded re-batch, scatter-adds the result back per camera and
// divides by the number of cameras that saw the query.  But the offsets and attention logits are
// functions of the QUERY only — every camera's copy of a query produces the same ones; only the
// reference points and the value map differ per camera.  So here a (query, head) group does the
// softmax and the offsets once and loops over the cameras that see the query, accumulating the
// sampled output in registers in camera order (the order of the reference's `slots +=`), and divides
// by the visible-camera count at the end: no index lists, no padding, no atomics, no host sync,
// and the two linears run on nq rows instead of cams * max_len.
//   value (cams, nv, heads, D)   ref (cams, nq, P, 2)   vis (cams, nq) u8   off_raw (nq, heads, L, P, 2)
//   logits (nq, heads, L*P)      out (nq, heads*D) = sum_{cam visible} msda_cam(q) / max(#visible, 1)
// ---------------------------------------------------------------------------------------
template <int D, int LOGG, typename VT>
__global__ __launch_bounds__(256, SO_MSDA_CROSS_WAVES(D, LOGG)) void msda_cross_fwd_kernel(const VT *__restrict__ value,
                                                             const int32_t *__restrict__ shapes,
                                                             const int32_t *__restrict__ starts,
                                                             const float *__restrict__ ref,
                                                             const uint8_t *__restrict__ vis,
                                                             const float *__restrict__ off_raw,
                                                             const float *__restrict__ logits,
                                                             float *__restrict__ out, int cams, MsdaDims dm) {
    constexpr int G = 1 << LOGG;
    constexpr int QL = D / 4, LOGQ = so_ilog2(QL);
    constexpr int NJ = LOGG > LOGQ ? LOGG - LOGQ : 0;
    constexpr int MAXR = so_maxr(LOGG);   // points per lane (host guarantees L * P <= MAXR * G)
    const int LP = dm.L * dm.P;
    const int groups_per_block = 256 / G;
    const int n_groups = dm.nq * dm.heads;                       // < 2^31 (validated)
    const int gid = (int)so_xcd_block() * groups_per_block + (threadIdx.x / G);
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < n_groups;
    const int gq0 = live ? gid : 0;                            // head-outer order, see so_split_group_head_outer
    const int h = gq0 / dm.nq, q = gq0 - h * dm.nq;
    const int gq = q * dm.heads + h;
    const int pix_stride = so_pix_stride(dm, D);     // `value` may be head-major or a column block of a wider matrix
    const int s = gl & (QL - 1);
    const VT *vb = value + so_value_base(dm, D, 0, h, 0) + 4 * s;
    const int cam_stride = (int)(so_value_base(dm, D, 1, h, 0) - so_value_base(dm, D, 0, h, 0));   // < 2^31 (validated)

    // softmax over the group's L * P logits; raw offsets of the lane's own points, already / (W_l, H_l)
    float lg[MAXR], ox[MAXR], oy[MAXR];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? logits[so_lg_index(dm, q, h, LP, pt)] : -INFINITY;
        mx = fmaxf(mx, lg[r]);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float den = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? __expf(lg[r] - mx) : 0.0f;
        den += lg[r];
        ox[r] = oy[r] = 0.0f;
        if (pt < LP) {
            const int l = so_level_of(pt, dm.P, dm.L);
            const float2 o = *(const float2 *)(off_raw + so_off_index(dm, q, h, LP, pt));
            ox[r] = o.x / (float)shapes[2 * l + 1];
            oy[r] = o.y / (float)shapes[2 * l];
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) den += __shfl_xor(den, m, 64);
    const float iden = 1.0f / den;

    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int count = 0;
    for (int cam = 0; cam < cams; ++cam) {
        const bool seen = live && vis[(size_t)cam * dm.nq + q] != 0;
        count += seen ? 1 : 0;
        if (!__any(seen)) continue;                      // no group of this wave sees the camera
        const int cam_off = cam * cam_stride;
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
            if (r * G >= LP) break;   // uniform
            const int pt = gl + r * G;
            MsdaPoint mp = so_point_none();
            if (seen && pt < LP) {
                const int l = so_level_of(pt, dm.P, dm.L);
                const int pp = pt - l * dm.P;
                const float2 rf = *(const float2 *)(ref + 2 * (((size_t)cam * dm.nq + q) * dm.P + pp));
                mp = so_point_setup(rf.x + ox[r], rf.y + oy[r], lg[r] * iden, shapes[2 * l], shapes[2 * l + 1],
                                    cam_off + starts[l] * pix_stride, pix_stride);
            }
            if constexpr (LOGG >= 5) {
                const int steps = so_compact_points<D, LOGG>(mp);
                so_team_gather_steps<D>(vb, mp, acc, steps);
            } else {
                so_team_gather<D>(vb, mp, acc);
            }
        }
    }
    // mean over the cameras that saw the query (image_cross_attention.py:133-135: count clamped to >= 1)
    const float cnt = (float)max(count, 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = acc[c] / cnt;
    so_group_reduce_store<NJ, LOGQ>(acc, gl >> LOGQ, live, out + (size_t)gq * D + 4 * s);
}

// ---------------------------------------------------------------------------------------
// backward.  Phase 1: lane per sampling point (no cross-lane reduction): the 4 corner . g_out
// dot products give grad_attw and grad_loc (coalesced per-point stores).  Phase 2: the
// grad_value scatter is TRANSPOSED so that D consecutive lanes own the D contiguous channels
// of one point's corner: an atomic instruction then touches 64 / D segments of D * 4 bytes
// instead of 64 scattered dwords (the scalar-per-lane form measured 15 G atomics/s, 100x
// slower than the forward).  Point parameters travel from the owner lane by wavefront shuffle.
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void msda_bwd_kernel(const float *__restrict__ value,
                                                       const int32_t *__restrict__ shapes,
                                                       const int32_t *__restrict__ starts,
                                                       const float *__restrict__ loc,
                                                       const float *__restrict__ attw,
                                                       const float *__restrict__ g_out,
                                                       float *__restrict__ g_value,
                                                       float *__restrict__ g_loc,
                                                       float *__restrict__ g_attw, MsdaDims dm) {
    const int LP = dm.L * dm.P;
    const long long n_pts = (long long)dm.bs * dm.nq * dm.heads * LP;
    const long long idx = (long long)so_xcd_block() * blockDim.x + threadIdx.x;
    const bool live = idx < n_pts;
    const long long idc = live ? idx : n_pts - 1;
    long long gq;
    int pt;
    if (n_pts < (1LL << 31)) {   // uniform: 32-bit division
        const unsigned g = (unsigned)idc / (unsigned)LP;
        gq = g;
        pt = (int)((unsigned)idc - g * (unsigned)LP);
    } else {
        gq = idc / LP;
        pt = (int)(idc - gq * LP);
    }
    int h, b;
    long long bq_unused;
    so_split_group(gq, n_pts, dm.nq, dm.heads, h, b, bq_unused);
    const int l = so_level_of(pt, dm.P, dm.L);
    const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
    const int pix_stride = so_pix_stride(dm, D);
    const float2 xy = *(const float2 *)(loc + 2 * idc);
    const float aw = attw[idc];
    const Bilin bl = so_bilinear_setup(xy.x, xy.y, Hl, Wl, pix_stride);
    const int vbase = (int)so_value_base(dm, D, b, h, starts[l]);  // < 2^31 (validated)
    float ga = 0.0f, gx = 0.0f, gy = 0.0f;
    float wsc[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // weight * attention weight of each corner (0: skip)
    if (live && bl.any) {
        const float *vl = value + vbase;
        float go[D];
        const float4 *gp = (const float4 *)(g_out + (size_t)gq * D);
#pragma unroll
        for (int q = 0; q < D / 4; ++q) {
            const float4 t = gp[q];
            go[4 * q] = t.x; go[4 * q + 1] = t.y; go[4 * q + 2] = t.z; go[4 * q + 3] = t.w;
        }
        float dot[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dot[k] = 0.0f;
            if (bl.valid[k]) {
                const float4 *p = (const float4 *)(vl + bl.off[k]);
                wsc[k] = bl.w[k] * aw;
#pragma unroll
                for (int q = 0; q < D / 4; ++q) {
                    const float4 t = p[q];
                    dot[k] = fmaf(t.x, go[4 * q], dot[k]);
                    dot[k] = fmaf(t.y, go[4 * q + 1], dot[k]);
                    dot[k] = fmaf(t.z, go[4 * q + 2], dot[k]);
                    dot[k] = fmaf(t.w, go[4 * q + 3], dot[k]);
                }
            }
        }
        // d out / d attw = bilinear value . g_out ;  d / d (w_im, h_im) from the weight derivatives
        ga = (bl.w[0] * dot[0] + bl.w[1] * dot[1]) + (bl.w[2] * dot[2] + bl.w[3] * dot[3]);
        const float gw = (bl.hh * (dot[1] - dot[0])) + (bl.lh * (dot[3] - dot[2]));
        const float gh = (bl.hw * (dot[2] - dot[0])) + (bl.lw * (dot[3] - dot[1]));
        gx = (float)Wl * gw * aw;
        gy = (float)Hl * gh * aw;
    }
    if (live) {
        g_attw[idx] = ga;
        *(float2 *)(g_loc + 2 * idx) = make_float2(gx, gy);
    }

    // ---- phase 2: transposed scatter of grad_value -------------------------------------------
    constexpr int PPI = 64 / D;                 // points served per atomic instruction
    const int lane = threadIdx.x & 63;
    const int sub = lane % D, grp = lane / D;
    const int gq32 = (int)gq;                    // < 2^31 (validated: bs * nq * heads * D < 2^31)
    int offs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) offs[k] = vbase + bl.off[k];
    for (int j = 0; j < 64 / PPI; ++j) {
        const int src = j * PPI + grp;          // owner lane of the point this lane now serves
        const int q_src = __shfl(gq32, src, 64);
        float w_src[4];
        int o_src[4];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w_src[k] = __shfl(wsc[k], src, 64);
            o_src[k] = __shfl(offs[k], src, 64);
            any |= (w_src[k] != 0.0f);
        }
        if (any) {
            const float goc = g_out[(size_t)q_src * D + sub];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (w_src[k] != 0.0f) unsafeAtomicAdd(g_value + o_src[k] + sub, w_src[k] * goc);
        }
    }
}


// ---------------------------------------------------------------------------------------
// backward, banded (output-stationary) form.
//
// grad_value is 64 scattered float adds per sampling point (4 corners x 16 channels): 1.6 G adds per
// call at the nuscenes_occ hw-plane shape, ~110 per output element and ~2300 per element on the
// 12x25 level.  Measured on MI355X (scripts/micro/atomics2.hip): global_atomic_add_f32 sustains
// ~330 G lane-ops/s chip-wide (one dword per L2 channel per clock; ~90 G/s when the rows of one
// instruction share a line), ds_add_f32 only ~200 G/s (~3 clocks per LANE), but ds_add_f64 runs
// at 3.7 T lane-ops/s.  So the scatter goes through LDS in double precision, and to make every
// add an LDS add the work is split by OUTPUT: a block owns a band of rows of one level's map of one
// (batch, head), keeps it in LDS as f64, and looks only at the sampling points that touch the band.
//
//   kernel 1 (points):  lane per sampling point; channel teams gather the 4 corners (as in the
//       forward), dot them with g_out -> grad_attw / grad_loc; also writes a 2-byte key per point
//       (the corner row floor(h_im), or "outside") into keys[b][h][l][q][p] and a 16-byte record
//       (bilinear fractions, attention weight, corner row / column).
//   kernels 2-4 (bins): counting sort of the point indices by (b, h, level, band of rows, class) — see
//       "binned band scatter" below.
//   kernel 5 (bands):   block = one segment of one band's index list.  For every 64 entries: lanes rebuild
//       the bilinear weights of their own point, then 16-lane rows (one channel per lane) add
//       w * attw * g_out into the band with ds_add_f64.  The band is flushed once (float atomics, so
//       that the segments of one band can share it).
// Besides the rate, f64 accumulation makes a band's sums order-independent to ~1e-16 relative (only the
// float flush of several segments into one band is order-dependent).
// ---------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void msda_bwd_point_kernel(const float *__restrict__ value,
                                                             const int32_t *__restrict__ shapes,
                                                             const int32_t *__restrict__ starts,
                                                             const float *__restrict__ loc,
                                                             const float *__restrict__ attw,
                                                             const float *__restrict__ g_out,
                                                             float *__restrict__ g_loc, float *__restrict__ g_attw,
                                                             int16_t *__restrict__ keys, float4 *__restrict__ recs,
                                                             MsdaDims dm) {
    constexpr int QL = D / 4;
    const int LP = dm.L * dm.P;
    const long long n_pts = (long long)dm.bs * dm.nq * dm.heads * LP;
    const long long idx = (long long)so_xcd_block() * blockDim.x + threadIdx.x;
    const bool live = idx < n_pts;
    const long long idc = live ? idx : n_pts - 1;
    long long gq;
    int pt;
    if (n_pts < (1LL << 31)) {   // uniform: 32-bit division
        const unsigned g = (unsigned)idc / (unsigned)LP;
        gq = g;
        pt = (int)((unsigned)idc - g * (unsigned)LP);
    } else {
        gq = idc / LP;
        pt = (int)(idc - gq * LP);
    }
    int h, b;
    long long bq;
    so_split_group(gq, n_pts, dm.nq, dm.heads, h, b, bq);
    const int l = so_level_of(pt, dm.P, dm.L);
    const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
    const int pix_stride = so_pix_stride(dm, D);
    const float2 xy = *(const float2 *)(loc + 2 * idc);
    const float aw = attw[idc];
    const Bilin bl = so_bilinear_setup(xy.x, xy.y, Hl, Wl, pix_stride);
    const int vbase = (int)so_value_base(dm, D, b, h, starts[l]);  // < 2^31 (validated)
    int goff[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) goff[k] = vbase + bl.off[k];
    const int s = threadIdx.x & (QL - 1);
    float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    so_bwd_team_dots<D>(value, MsdaGoRows{g_out, (int)gq}, s, goff, dot, QL);
    if (!live) return;
    float ga = 0.0f, gx = 0.0f, gy = 0.0f;
    if (bl.any) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dot[k] = bl.valid[k] ? dot[k] : 0.0f;
        // d out / d attw = bilinear value . g_out ;  d / d (w_im, h_im) from the weight derivatives
        ga = (bl.w[0] * dot[0] + bl.w[1] * dot[1]) + (bl.w[2] * dot[2] + bl.w[3] * dot[3]);
        const float gw = (bl.hh * (dot[1] - dot[0])) + (bl.lh * (dot[3] - dot[2]));
        const float gh = (bl.hw * (dot[2] - dot[0])) + (bl.lw * (dot[3] - dot[1]));
        gx = (float)Wl * gw * aw;
        gy = (float)Hl * gh * aw;
    }
    g_attw[idx] = ga;
    *(float2 *)(g_loc + 2 * idx) = make_float2(gx, gy);
    const int q = (int)(bq - (long long)b * dm.nq);
    const int p = pt - l * dm.P;
    // everything the band kernel needs of this point, in ITS order (points of one (b, h, level) contiguous)
    const size_t ki = ((((size_t)b * dm.heads + h) * dm.L + l) * dm.nq + q) * dm.P + p;
    keys[ki] = (int16_t)(bl.any ? bl.h_low : kKeyOutside);
    recs[ki] = make_float4(bl.lh, bl.lw, aw, so_band_cell(bl.h_low, bl.w_low));
}

// ---------------------------------------------------------------------------------------
// fused backward, point part (training): the counterpart of msda_fused_fwd_kernel.  Recomputes the
// softmax and loc = ref + off / (W_l, H_l) in registers (nothing but value / ref / off_raw / logits was
// saved by the forward), gathers the corners by channel teams, and writes the gradients of the RAW
// linear outputs directly:
//     g_off   = (d out / d loc) / (W_l, H_l)
//     g_logit = aw (g_aw - sum_group aw g_aw)                     (softmax backward, group reduction on shuffles)
// plus the keys / records of the banded grad_value scatter.  Replaces, per call, the torch kernels for
// softmax, off / normalizer, + ref and their three backward kernels, and the 100-400 MB loc / weight
// tensors with their gradients.
// ---------------------------------------------------------------------------------------
// plan of the counting sort that follows the point kernels (see msda_bin_kernel below); the training point kernels count
// their own hits with it
constexpr int kMaxBands = 1024;            // bands per level (host falls back to the atomic kernel beyond)
constexpr int kBinKeysPerBlock = 256 * 32;

// n / d for any 32-bit n without a division (Granlund & Montgomery round-up method; host computes m, l from d)
struct SoFastDiv {
    unsigned m;
    int l;
};
SO_DEVFN int so_fastdiv(int n, SoFastDiv f) {
    if (f.l == 0) return n;                      // d == 1
    const unsigned t = __umulhi(f.m, (unsigned)n);
    return (int)((t + (((unsigned)n - t) >> 1)) >> (f.l - 1));
}

struct MsdaBinPlan {
    float inv_rows[8];   // 1 / rows[l] (host-computed: the bin kernels and the counting point kernels classify with the same float)
    int rows[8];      // rows per band of level l
    int bands[8];     // bands of level l
    int band0[9];     // first band of level l within a (batch, head)
    int nbands;       // bands per (batch, head)
    int seg;          // list entries per band-kernel block
    SoFastDiv divP;   // key index -> query
};

template <int D, int LOGG, typename VT>
__global__ __launch_bounds__(256) void msda_fused_bwd_point_kernel(const VT *__restrict__ value,
                                                                   const int32_t *__restrict__ shapes,
                                                                   const int32_t *__restrict__ starts,
                                                                   const float *__restrict__ ref, int ref_kind,
                                                                   const float *__restrict__ off_raw,
                                                                   const float *__restrict__ logits,
                                                                   const float *__restrict__ g_out,
                                                                   float *__restrict__ g_off, float *__restrict__ g_logits,
                                                                   int16_t *__restrict__ keys, float4 *__restrict__ recs,
                                                                   MsdaDims dm) {
    constexpr int G = 1 << LOGG;
    constexpr int QL = D / 4;
    constexpr int MAXR = so_maxr(LOGG);
    const int LP = dm.L * dm.P;
    const int groups_per_block = 256 / G;
    const long long n_groups = (long long)dm.bs * dm.nq * dm.heads;
    const long long gid = (long long)so_xcd_block() * groups_per_block + (threadIdx.x / G);
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < n_groups;
    int h, b;
    long long bq, gq;                                   // b * nq + q; (b, q, h) index of the group
    so_split_group_head_outer(live ? gid : 0, dm, h, b, bq, gq);
    const int q = (int)(bq - (long long)b * dm.nq);
    const int pix_stride = so_pix_stride(dm, D);
    const int s = gl & (QL - 1);

    float lg[MAXR];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? logits[so_lg_index(dm, bq, h, LP, pt)] : -INFINITY;
        mx = fmaxf(mx, lg[r]);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float den = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        lg[r] = (gl + r * G < LP) ? __expf(lg[r] - mx) : 0.0f;
        den += lg[r];
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) den += __shfl_xor(den, m, 64);
    const float iden = 1.0f / den;

    float4 go = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) go = *(const float4 *)(g_out + (size_t)gq * D + 4 * s);
    float ga[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) ga[r] = 0.0f;
    float sum_l = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        if (r * G >= LP) break;   // uniform
        const int pt = gl + r * G;
        const bool own = live && pt < LP;
        const int ptc = own ? pt : 0;
        const int l = so_level_of(ptc, dm.P, dm.L);
        const int pp = ptc - l * dm.P;
        const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
        const size_t oidx = so_off_index(dm, bq, h, LP, ptc);
        const float2 o = *(const float2 *)(off_raw + oidx);
        size_t ri;
        if (ref_kind == 1) ri = (size_t)bq * dm.P + pp;
        else if (ref_kind == 2) ri = ((size_t)bq * dm.L + l) * dm.P + pp;
        else ri = (size_t)bq * dm.L + l;
        const float2 rf = *(const float2 *)(ref + 2 * ri);
        const float lx = rf.x + o.x / (float)Wl, ly = rf.y + o.y / (float)Hl;
        const float aw = lg[r] * iden;
        const Bilin bl = so_bilinear_setup(lx, ly, Hl, Wl, pix_stride);
        const int vbase = (int)so_value_base(dm, D, b, h, starts[l]);
        int goff[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) goff[k] = own ? vbase + bl.off[k] : 0;
        float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        so_bwd_team_dots<D>(value, go, s, goff, dot, QL);
        if (own) {
            float gx = 0.0f, gy = 0.0f;
            if (bl.any) {
#pragma unroll
                for (int k = 0; k < 4; ++k) dot[k] = bl.valid[k] ? dot[k] : 0.0f;
                ga[r] = (bl.w[0] * dot[0] + bl.w[1] * dot[1]) + (bl.w[2] * dot[2] + bl.w[3] * dot[3]);
                const float gw = (bl.hh * (dot[1] - dot[0])) + (bl.lh * (dot[3] - dot[2]));
                const float gh = (bl.hw * (dot[2] - dot[0])) + (bl.lw * (dot[3] - dot[1]));
                gx = (float)Wl * gw * aw;
                gy = (float)Hl * gh * aw;
            }
            // loc = ref + off / (W, H)  =>  g_off = g_loc / (W, H)
            *(float2 *)(g_off + oidx) = make_float2(gx / (float)Wl, gy / (float)Hl);
            sum_l = fmaf(aw, ga[r], sum_l);
            const size_t ki = ((((size_t)b * dm.heads + h) * dm.L + l) * dm.nq + q) * dm.P + pp;
            keys[ki] = (int16_t)(bl.any ? bl.h_low : kKeyOutside);
            recs[ki] = make_float4(bl.lh, bl.lw, aw, so_band_cell(bl.h_low, bl.w_low));
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) sum_l += __shfl_xor(sum_l, m, 64);
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        if (live && pt < LP) g_logits[so_lg_index(dm, bq, h, LP, pt)] = (lg[r] * iden) * (ga[r] - sum_l);
    }
}

// ---------------------------------------------------------------------------------------
// camera-loop backward, point part (training counterpart of msda_cross_fwd_kernel):
//   out[q] = (1 / cnt_q) sum_{cam sees q} msda_cam(q)      with shared offsets / logits per query.
// g_off and g_logits are sums over the visible cameras (divided by cnt); keys / records are written per
// (cam, h, level, q, p) for the visible cameras only (the key array is pre-filled with "outside"), the
// record's weight already divided by cnt, and the band kernel reads the shared g_out row (go_shared).
// ---------------------------------------------------------------------------------------
template <int D, int LOGG, typename VT>
// (no register cap: with min-waves 4 the compiler holds the kernel at 105 / 101 registers instead of 115 / 111 and the
// iteration loses 1.3 ms — fewer corner gathers in flight per wave; 5 / 6 waves spill)
__global__ __launch_bounds__(256) void msda_cross_bwd_point_kernel(const VT *__restrict__ value,
                                                                   const int32_t *__restrict__ shapes,
                                                                   const int32_t *__restrict__ starts,
                                                                   const float *__restrict__ ref,
                                                                   const uint8_t *__restrict__ vis,
                                                                   const float *__restrict__ off_raw,
                                                                   const float *__restrict__ logits,
                                                                   const float *__restrict__ g_out,
                                                                   float *__restrict__ g_off, float *__restrict__ g_logits,
                                                                   int16_t *__restrict__ keys, float4 *__restrict__ recs,
                                                                   int cams, MsdaDims dm, int32_t *__restrict__ bin_cnt,
                                                                   MsdaBinPlan plan) {
    constexpr int G = 1 << LOGG;
    constexpr int QL = D / 4;
    constexpr int MAXR = so_maxr(LOGG);
    const int LP = dm.L * dm.P;
    const int groups_per_block = 256 / G;
    const int n_groups = dm.nq * dm.heads;
    // bin_cnt != NULL: the kernel also does the counting pass of the sort (msda_bin_kernel<false>): an LDS histogram over
    // (head of the block: at most two, camera, band, class), flushed once per block — the keys are in registers here
    extern __shared__ int hist_s[];                              // [2 heads][cams][nbands][2]
    const int blk0 = (int)so_xcd_block() * groups_per_block;
    const int h_first = min(blk0, n_groups - 1) / dm.nq;
    const int nh = bin_cnt != nullptr ? 2 * cams * plan.nbands * 2 : 0;
    for (int e = threadIdx.x; e < nh; e += 256) hist_s[e] = 0;
    if (bin_cnt != nullptr) __syncthreads();
    const int gid = blk0 + (threadIdx.x / G);
    const int gl = threadIdx.x & (G - 1);
    const bool live = gid < n_groups;
    const int gq0 = live ? gid : 0;                            // head-outer order, see so_split_group_head_outer
    const int h = gq0 / dm.nq, q = gq0 - h * dm.nq;
    const int gq = q * dm.heads + h;
    const int pix_stride = so_pix_stride(dm, D);
    const int s = gl & (QL - 1);

    float lg[MAXR], ox[MAXR], oy[MAXR];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? logits[so_lg_index(dm, q, h, LP, pt)] : -INFINITY;
        mx = fmaxf(mx, lg[r]);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    float den = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        lg[r] = (pt < LP) ? __expf(lg[r] - mx) : 0.0f;
        den += lg[r];
        ox[r] = oy[r] = 0.0f;
        if (pt < LP) {
            const int l = so_level_of(pt, dm.P, dm.L);
            const float2 o = *(const float2 *)(off_raw + so_off_index(dm, q, h, LP, pt));
            ox[r] = o.x / (float)shapes[2 * l + 1];
            oy[r] = o.y / (float)shapes[2 * l];
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) den += __shfl_xor(den, m, 64);
    const float iden = 1.0f / den;

    int count = 0;
    for (int cam = 0; cam < cams; ++cam) count += (live && vis[(size_t)cam * dm.nq + q] != 0) ? 1 : 0;
    const float cnt = (float)max(count, 1);

    float4 go = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) go = *(const float4 *)(g_out + (size_t)gq * D + 4 * s);
    float ga[MAXR], gxs[MAXR], gys[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) ga[r] = gxs[r] = gys[r] = 0.0f;
    for (int cam = 0; cam < cams; ++cam) {
        const bool seen = live && vis[(size_t)cam * dm.nq + q] != 0;
        if (!__any(seen)) continue;                      // no group of this wave sees the camera
#pragma unroll
        for (int r = 0; r < MAXR; ++r) {
            if (r * G >= LP) break;   // uniform
            const int pt = gl + r * G;
            const bool own = seen && pt < LP;
            const int ptc = own ? pt : 0;
            const int l = so_level_of(ptc, dm.P, dm.L);
            const int pp = ptc - l * dm.P;
            const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
            const float2 rf = *(const float2 *)(ref + 2 * (((size_t)cam * dm.nq + q) * dm.P + pp));
            const float aw = lg[r] * iden;
            const Bilin bl = so_bilinear_setup(rf.x + ox[r], rf.y + oy[r], Hl, Wl, pix_stride);
            const int vbase = (int)so_value_base(dm, D, cam, h, starts[l]);
            int goff[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) goff[k] = own ? vbase + bl.off[k] : 0;
            float dot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            // whole-wave groups: the points that touch the map move to the front (see so_compact_points), the teams
            // compute their corner dots there, and the dots travel back to the lanes that own the points
            int steps = QL, dst = 0;
            bool moved = false;
            if constexpr (LOGG >= 5) {
                steps = so_compact_plan<D, LOGG>(own && bl.any, dst, moved);
                if (moved) {   // wave-uniform
#pragma unroll
                    for (int c = 0; c < 4; ++c) goff[c] = __builtin_amdgcn_ds_permute(dst, goff[c]);
                }
            }
            // (so_bwd_team_dots written out: through the helper 8 of these 20 kernels compile to another schedule)
            if (steps > 0) so_bwd_team_step<D, 0>(value, go, s, goff, dot);
            if constexpr (QL > 1) { if (steps > 1) so_bwd_team_step<D, 1>(value, go, s, goff, dot); }
            if constexpr (QL > 2) {
                if (steps > 2) so_bwd_team_step<D, 2>(value, go, s, goff, dot);
                if (steps > 3) so_bwd_team_step<D, 3>(value, go, s, goff, dot);
            }
            if constexpr (QL > 4) {
                if (steps > 4) so_bwd_team_step<D, 4>(value, go, s, goff, dot);
                if (steps > 5) so_bwd_team_step<D, 5>(value, go, s, goff, dot);
                if (steps > 6) so_bwd_team_step<D, 6>(value, go, s, goff, dot);
                if (steps > 7) so_bwd_team_step<D, 7>(value, go, s, goff, dot);
            }
            if (moved) {   // wave-uniform
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    dot[c] = __int_as_float(__builtin_amdgcn_ds_bpermute(dst, __float_as_int(dot[c])));
            }
            const size_t ki = ((((size_t)cam * dm.heads + h) * dm.L + l) * dm.nq + q) * dm.P + pp;
            if (own && !bl.any) keys[ki] = (int16_t)kKeyOutside;   // every key of a visited (camera, query) is written
            if (own && bl.any) {
#pragma unroll
                for (int k = 0; k < 4; ++k) dot[k] = bl.valid[k] ? dot[k] : 0.0f;
                ga[r] += (bl.w[0] * dot[0] + bl.w[1] * dot[1]) + (bl.w[2] * dot[2] + bl.w[3] * dot[3]);
                const float gw = (bl.hh * (dot[1] - dot[0])) + (bl.lh * (dot[3] - dot[2]));
                const float gh = (bl.hw * (dot[2] - dot[0])) + (bl.lw * (dot[3] - dot[1]));
                gxs[r] += ((float)Wl * gw * aw) / (float)Wl;
                gys[r] += ((float)Hl * gh * aw) / (float)Hl;
                keys[ki] = (int16_t)bl.h_low;
                recs[ki] = make_float4(bl.lh, bl.lw, aw / cnt, so_band_cell(bl.h_low, bl.w_low));
                if (bin_cnt != nullptr) {      // the classification of msda_bin_kernel, on the key in the register
                    int band0 = 0;
                    float inv_rows = plan.inv_rows[0];
                    for (int k = 1; k < 8; ++k)
                        if (k == l) { band0 = plan.band0[k]; inv_rows = plan.inv_rows[k]; }
                    const int key = bl.h_low;
                    const bool va = key >= 0 && key < Hl, vb = key + 1 >= 0 && key + 1 < Hl;
                    const int ba = (int)(((float)key + 0.5f) * inv_rows), bb = (int)(((float)key + 1.5f) * inv_rows);
                    int *hb = hist_s + (((h - h_first) * cams + cam) * plan.nbands + band0) * 2;
                    if (va && vb && ba == bb) {
                        atomicAdd(hb + 2 * ba, 1);
                    } else {
                        if (va) atomicAdd(hb + 2 * ba + 1, 1);
                        if (vb) atomicAdd(hb + 2 * bb + 1, 1);
                    }
                }
            }
        }
    }
    if (bin_cnt != nullptr) {
        __syncthreads();
        for (int e = threadIdx.x; e < nh; e += 256) {
            const int c = hist_s[e];
            if (c == 0) continue;
            const int per_head = cams * plan.nbands * 2;
            const int hr = e / per_head, rem = e - hr * per_head;
            const int cam = rem / (plan.nbands * 2), bc = rem - cam * (plan.nbands * 2);
            atomicAdd(bin_cnt + ((size_t)(cam * dm.heads + h_first + hr) * plan.nbands) * 2 + bc, c);
        }
    }
    float sum_l = 0.0f;
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        ga[r] = ga[r] / cnt;
        sum_l = fmaf(lg[r] * iden, ga[r], sum_l);
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) sum_l += __shfl_xor(sum_l, m, 64);
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        const int pt = gl + r * G;
        if (live && pt < LP) {
            g_logits[so_lg_index(dm, q, h, LP, pt)] = (lg[r] * iden) * (ga[r] - sum_l);
            *(float2 *)(g_off + so_off_index(dm, q, h, LP, pt)) = make_float2(gxs[r] / cnt, gys[r] / cnt);
        }
    }
}

// two block shapes: 512 threads + 52 KB tile (two blocks per CU: one block's zero / flush phases overlap the other's
// adds) and 1024 threads + 103 KB tile (one block per CU, 2x taller bands: fewer points straddle two bands)
constexpr int band_tile_bytes(int threads) { return threads == 512 ? 52 * 1024 : 103 * 1024; }

// ---------------------------------------------------------------------------------------
// binned band scatter.  Round 1 let every band block stream its level's keys and pick out its hits: O(bands x keys),
// and measured on the training iteration 57 % of that kernel's time was the scan alone (no hit processed), 35 % the
// per-hit work, 8 % the LDS atomics.  Now the keys are read three times in total, by a counting sort by
// (batch, head, level, band, class):
//   bin<false>: LDS histogram of a block of keys -> global counters        (class FULL: both corner rows in the band,
//   scan:       exclusive scan of the counters, work items per band                EDGE: one corner row; a point whose
//   bin<true>:  same histogram, reserve space, write the point indices             rows straddle two bands is listed in both)
// and the band kernel walks its own index list: no scan, no rings, no ballots; bands nobody touches cost nothing
// (not even the tile zero / flush), long lists are cut into segments of `seg` entries (one block each).
// Training iteration (16 calls): 15.6 ms -> 8.1 ms; the band kernel now runs at the ds_add_f64 rate measured by
// scripts/micro/atomics2.hip (~10.6 clk per 64-lane instruction).
// ---------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void msda_bin_kernel(const int16_t *__restrict__ keys, const int32_t *__restrict__ shapes,
                                                       int32_t *__restrict__ cnt, int32_t *__restrict__ cursor,
                                                       const int32_t *__restrict__ off, int32_t *__restrict__ list,
                                                       const unsigned char *__restrict__ vis, int bpb, MsdaDims dm,
                                                       MsdaBinPlan plan) {
    // vis != NULL (camera loop, P >= 4): keys of (camera, query) pairs with vis == 0 were never written — not read here
    __shared__ int hist[2 * kMaxBands];
    __shared__ int base_s[FILL ? 2 * kMaxBands : 1];
    const long long bhl = blockIdx.x / bpb;
    const int chunk = blockIdx.x - (int)(bhl * bpb);
    const int l = (int)(bhl % dm.L);
    const long long bh = bhl / dm.L;
    int bands_l = plan.bands[0], band0 = 0;
    float inv_rows = plan.inv_rows[0];
    for (int k = 1; k < 8; ++k)
        if (k == l) { bands_l = plan.bands[k]; band0 = plan.band0[k]; inv_rows = plan.inv_rows[k]; }
    const int Hl = shapes[2 * l];
    const long long n = (long long)dm.nq * dm.P;                      // keys of one (b, h, l)
    const long long kbase = bhl * n;
    // the block's keys: an 8-byte aligned window of kBinKeysPerBlock keys, clipped to this (b, h, l)
    const long long win = (kbase & ~3LL) + (long long)chunk * kBinKeysPerBlock;
    const long long lo = max(kbase, win), hi = min(kbase + n, win + kBinKeysPerBlock);
    const long long bucket0 = (bh * plan.nbands + band0) * 2;         // bucket = (band id) * 2 + class
    for (int i = threadIdx.x; i < 2 * bands_l; i += 256) hist[i] = 0;

    // every lane loads its keys ONCE (4 consecutive keys = 8 aligned bytes per step, all steps in flight together);
    // keys outside [lo, hi) and keys of invisible (camera, query) pairs become "outside" in the registers
    constexpr int IT = kBinKeysPerBlock / (256 * 4);
    constexpr unsigned kNone = 0x80008000u;
    uint2 kk[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const long long p = win + (long long)(it * 256 + (int)threadIdx.x) * 4;
        kk[it] = make_uint2(kNone, kNone);
        if (p + 3 < lo || p >= hi) continue;
        bool v0 = true, v1 = true;     // visibility of the queries of the first / last key (P >= 4: at most two)
        int qsplit = 0;
        if (vis != nullptr) {
            const unsigned char *vb = vis + (size_t)(bh / dm.heads) * dm.nq;
            const int e0 = (int)(max(p, lo) - kbase), e1 = (int)(min(p + 3, hi - 1) - kbase);
            const int q0 = so_fastdiv(e0, plan.divP), q1 = so_fastdiv(e1, plan.divP);
            v0 = vb[q0] != 0;
            v1 = vb[q1] != 0;
            qsplit = q1 * dm.P;        // first key of the last query
        }
        if (!v0 && !v1) continue;
        uint2 t = *(const uint2 *)(keys + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long gi = p + k;
            const bool dead = gi < lo || gi >= hi || !((int)(gi - kbase) < qsplit ? v0 : v1);
            if (dead) {
                unsigned &w = (k & 2) ? t.y : t.x;
                w = (k & 1) ? ((w & 0x0000ffffu) | 0x80000000u) : ((w & 0xffff0000u) | 0x00008000u);
            }
        }
        kk[it] = t;
    }
    __syncthreads();

    // pass(emit): emit(bucket-in-level, key index) per list entry.  (One LDS atomic per lane and entry: aggregating the
    // lanes of a wave that want the same bucket measured 2.5x slower — the pillar points of a query span many rows.)
    auto pass = [&](auto emit) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            if (kk[it].x == kNone && kk[it].y == kNone) continue;
            const int e4 = (int)(win - kbase) + (it * 256 + (int)threadIdx.x) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int key = (int)(short)(((k & 2) ? kk[it].y : kk[it].x) >> (16 * (k & 1)));
                if (key == kKeyOutside) continue;
                const bool va = key >= 0 && key < Hl, vb = key + 1 >= 0 && key + 1 < Hl;
                const int ba = (int)(((float)key + 0.5f) * inv_rows), bb = (int)(((float)key + 1.5f) * inv_rows);
                const int e = e4 + k;
                if (va && vb && ba == bb) {
                    emit(2 * ba, e);
                } else {
                    if (va) emit(2 * ba + 1, e);
                    if (vb) emit(2 * bb + 1, e);
                }
            }
        }
    };
    pass([&](int i, int) { atomicAdd(&hist[i], 1); });
    __syncthreads();
    if constexpr (!FILL) {
        for (int i = threadIdx.x; i < 2 * bands_l; i += 256) {
            const int c = hist[i];
            if (c) atomicAdd(&cnt[bucket0 + i], c);
        }
    } else {
        for (int i = threadIdx.x; i < 2 * bands_l; i += 256) {
            const int c = hist[i];
            base_s[i] = c ? off[bucket0 + i] + atomicAdd(&cursor[bucket0 + i], c) : 0;
            hist[i] = 0;
        }
        __syncthreads();
        pass([&](int i, int e) { list[base_s[i] + atomicAdd(&hist[i], 1)] = e; });
    }
}

// one block: off[bucket] = first list entry of the bucket (a band's EDGE list follows its FULL list),
// item0[band] = first work item of the band (ceil(entries / seg) items), item0[n_bands] = number of items
__global__ __launch_bounds__(1024) void msda_bin_scan_kernel(const int32_t *__restrict__ cnt, int32_t *__restrict__ off,
                                                             int32_t *__restrict__ item0, int n_bands, int seg) {
    __shared__ int se[1024], si[1024];
    const int t = threadIdx.x;
    const int per = (n_bands + 1023) / 1024;
    const int b0 = min(n_bands, t * per), b1 = min(n_bands, b0 + per);
    int ne = 0, ni = 0;
    for (int b = b0; b < b1; ++b) {
        const int c = cnt[2 * b] + cnt[2 * b + 1];
        ne += c;
        ni += (c + seg - 1) / seg;
    }
    se[t] = ne; si[t] = ni;
    __syncthreads();
    for (int m = 1; m < 1024; m <<= 1) {
        const int ae = t >= m ? se[t - m] : 0, ai = t >= m ? si[t - m] : 0;
        __syncthreads();
        se[t] += ae; si[t] += ai;
        __syncthreads();
    }
    int pe = se[t] - ne, pi = si[t] - ni;     // exclusive prefixes of this thread's run
    for (int b = b0; b < b1; ++b) {
        const int cf = cnt[2 * b], c = cf + cnt[2 * b + 1];
        off[2 * b] = pe;
        off[2 * b + 1] = pe + cf;
        item0[b] = pi;
        pe += c;
        pi += (c + seg - 1) / seg;
    }
    if (t == 1023) item0[n_bands] = si[1023];
}

template <int D, int kBandThreads>
__global__ __launch_bounds__(kBandThreads) void msda_bwd_band_list_kernel(const int32_t *__restrict__ shapes,
                                                                          const int32_t *__restrict__ starts,
                                                                          const float *__restrict__ g_out,
                                                                          float *__restrict__ g_value,
                                                                          const float4 *__restrict__ recs,
                                                                          const int32_t *__restrict__ cnt,
                                                                          const int32_t *__restrict__ off,
                                                                          const int32_t *__restrict__ item0,
                                                                          const int32_t *__restrict__ list, int n_bands,
                                                                          MsdaDims dm, MsdaBinPlan plan) {
    constexpr int ROWS = 64 / D;        // sampling points served per atomic instruction
    constexpr int NJ = 64 / ROWS;       // row steps per batch of 64 points (= D)
    constexpr int NW = kBandThreads / 64;
    extern __shared__ __attribute__((aligned(16))) double tile[];
    __shared__ int4 recP[kBandThreads];     // band-local element offsets of the 4 (or 2) corners
    __shared__ float4 recW[kBandThreads];   // corner weight x attention weight
    __shared__ int recQ[kBandThreads];      // (b, q, h) group index: row of g_out

    const int item = blockIdx.x;
    if (item >= item0[n_bands]) return;
    int lo_b = 0, hi_b = n_bands;           // largest band id with item0[id] <= item (uniform: scalar loads)
    while (hi_b - lo_b > 1) {
        const int mid = (lo_b + hi_b) >> 1;
        if (item0[mid] <= item) lo_b = mid; else hi_b = mid;
    }
    const int band_id = lo_b;
    const int segi = item - item0[band_id];
    const int bh = band_id / plan.nbands, rb = band_id - bh * plan.nbands;
    const int h = bh % dm.heads, b = bh / dm.heads;
    int l = 0;
    for (int k = 1; k < dm.L; ++k) l += (rb >= plan.band0[k]);
    int rows_l = plan.rows[0], first = 0;
    for (int k = 1; k < 8; ++k)
        if (k == l) { rows_l = plan.rows[k]; first = plan.band0[k]; }
    const int band = rb - first;
    const int Hl = shapes[2 * l], Wl = shapes[2 * l + 1];
    const int y0 = band * rows_l, y1 = min(Hl, y0 + rows_l);
    const int n_tile = (y1 - y0) * Wl * D;
    const int cF = cnt[2 * band_id], cE = cnt[2 * band_id + 1];
    const int32_t *mine = list + off[2 * band_id];        // FULL entries [0, cF), EDGE entries [cF, cF + cE)
    const int s0 = segi * plan.seg, s1 = min(cF + cE, s0 + plan.seg);

    for (int e = threadIdx.x; e < n_tile; e += kBandThreads) tile[e] = 0.0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wave0 = threadIdx.x & ~63;
    const int sub = lane % D, row = lane / D;
    const long long kbase = (((long long)b * dm.heads + h) * dm.L + l) * (long long)dm.nq * dm.P;

    // n <= 64 list entries starting at `pos` -> band
    auto process = [&](auto cls, int pos, int n) {
        constexpr int C = decltype(cls)::value;     // 0: FULL, 1: EDGE
        float4 w4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int4 p4 = make_int4(0, 0, 0, 0);
        int gq32 = 0;
        if (lane < n) {
            const int e = mine[pos + lane];
            const int q = so_fastdiv(e, plan.divP);
            const float4 rc = recs[kbase + e];
            const MsdaBandRec u = so_band_unpack(rc);
            const int h_low = u.h_low, w_low = u.w_low;
            const float lh = u.lh, lw = u.lw, aw = u.aw;
            const float hh = 1.0f - lh, hw = 1.0f - lw;
            const bool c0 = w_low >= 0, c1 = w_low + 1 <= Wl - 1;
            const int x0 = max(w_low, 0), x1 = min(w_low + 1, Wl - 1);
            if (C == 0) {
                const int r0 = (h_low - y0) * Wl, r1 = r0 + Wl;
                w4 = make_float4(c0 ? (hh * hw) * aw : 0.0f, c1 ? (hh * lw) * aw : 0.0f,
                                 c0 ? (lh * hw) * aw : 0.0f, c1 ? (lh * lw) * aw : 0.0f);
                p4 = make_int4((r0 + x0) * D, (r0 + x1) * D, (r1 + x0) * D, (r1 + x1) * D);
            } else {
                // the one corner row inside the band: the lower one (h_low + 1 == y0) or the upper one (h_low == y1 - 1)
                const bool lower = h_low < y0;
                const int ry = lower ? h_low + 1 : h_low;
                const float wy = lower ? lh : hh;
                const int r0 = (ry - y0) * Wl;
                w4 = make_float4(c0 ? (wy * hw) * aw : 0.0f, c1 ? (wy * lw) * aw : 0.0f, 0.0f, 0.0f);
                p4 = make_int4((r0 + x0) * D, (r0 + x1) * D, 0, 0);
            }
            gq32 = dm.go_shared ? q * dm.heads + h : (int)(((long long)b * dm.nq + q) * dm.heads + h);
        }
        recW[threadIdx.x] = w4;
        recP[threadIdx.x] = p4;
        recQ[threadIdx.x] = gq32;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float goc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) goc[j] = g_out[(size_t)recQ[wave0 + j * ROWS + row] * D + sub];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int src = wave0 + j * ROWS + row;
            const float4 ws = recW[src];
            const int4 ps = recP[src];
            // unconditional: a corner outside the map carries weight 0 (adds 0.0 to the band's first pixel)
            unsafeAtomicAdd(&tile[ps.x + sub], (double)(ws.x * goc[j]));
            unsafeAtomicAdd(&tile[ps.y + sub], (double)(ws.y * goc[j]));
            if (C == 0) {
                unsafeAtomicAdd(&tile[ps.z + sub], (double)(ws.z * goc[j]));
                unsafeAtomicAdd(&tile[ps.w + sub], (double)(ws.w * goc[j]));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    const int f0 = s0, f1 = min(s1, cF);              // FULL part of the segment
    for (int p = f0 + wv * 64; p < f1; p += NW * 64) process(std::integral_constant<int, 0>{}, p, min(64, f1 - p));
    const int e0 = max(s0, cF), e1 = s1;              // EDGE part
    for (int p = e0 + wv * 64; p < e1; p += NW * 64) process(std::integral_constant<int, 1>{}, p, min(64, e1 - p));
    __syncthreads();

    const int pix_stride = so_pix_stride(dm, D);
    float *gl = g_value + so_value_base(dm, D, b, h, (long long)starts[l] + (long long)y0 * Wl);
    for (int e = threadIdx.x; e < n_tile; e += kBandThreads) {
        const double v = tile[e];
        if (v != 0.0) unsafeAtomicAdd(gl + (size_t)(e / D) * pix_stride + (e % D), (float)v);
    }
}

}  // namespace

// Lanes per (b, q, head) group: a power of two G >= d / 4 (whole channel teams) with rounds = ceil(LP / G)
// <= max_rounds; among those the one that wastes the fewest lane-rounds (LP = 36 on G = 64 idles 44 % of the
// lanes, on G = 16 x 3 rounds 25 %), larger G on ties (fewer rounds).  Used by the plain forward only: the fused
// kernels redo their prologue every round and measured slower with more rounds.
static void so_pick_group(int LP, int d, int max_rounds, int &G, int &logG) {
    int best_l = 6;
    double best_u = -1.0;
    for (int lg = 0; lg <= 6; ++lg) {
        const int g = 1 << lg;
        if (g < d / 4) continue;
        const int rounds = (LP + g - 1) / g;
        if (rounds > max_rounds && lg < 6) continue;
        const double u = (double)LP / ((double)rounds * g);
        if (u >= best_u - 1e-12) { best_u = u; best_l = lg; }
    }
    logG = best_l;
    G = 1 << best_l;
}

// Fused kernels: a lane holds at most so_maxr(log2 G) points; among the group sizes that allows, the best lane
// utilisation LP / (rounds * G), ties to the larger group (fewest rounds: the softmax exchanges are per group, the
// prologue per round).  L * P = 36 (the shipped self-attention) -> G = 8, 5 rounds, 90 % live lanes (64 lanes: 56 %).
static void so_pick_group_fused(int LP, int d, int &G, int &logG) {
    int best_l = 6;
    double best_u = -1.0;
    for (int lg = 6; lg >= 0; --lg) {
        const int g = 1 << lg;
        if (g < d / 4) break;
        const int rounds = (LP + g - 1) / g;
        if (rounds > so_maxr(lg)) { if (lg >= 4) continue; else break; }
        const double u = (double)LP / ((double)rounds * g);
        if (u > best_u + 1e-12) { best_u = u; best_l = lg; }
    }
    logG = best_l;
    G = 1 << best_l;
}

// The (D, log2 G, value type) combinations of the fused / camera-loop families that can be launched: D = 8, 16, 32 channels per
// head (the shipped lifters use 16; the plain mmcv-boundary op keeps 4), whole channel teams (G >= D / 4: so_pick_group_fused
// never returns less), bfloat16 `value` for D = 16 only.  Round 4 instantiated all 4 x 7 x 2 = 56 per family (224 kernels, 6 MB).
// so_with_msda_shape is that table: it calls fn(D, LOGG, value type) with compile-time values (arguments of a generic lambda).
template <int V>
using so_int = std::integral_constant<int, V>;
template <class T>
struct so_type_tag { using type = T; };

// fn(so_int<D>) for the head width of a validated call (so_msda_check_sizes: 4, 8, 16 or 32)
template <class F>
static int so_with_msda_d(int d, F &&fn) {
    switch (d) {
        case 4: return fn(so_int<4>{});
        case 8: return fn(so_int<8>{});
        case 16: return fn(so_int<16>{});
        default: return fn(so_int<32>{});
    }
}

// fn(so_int<LOGG>) for LOGG = logG within LGMIN .. 6
template <int LGMIN, class F>
static int so_with_msda_logg(int logG, F &&fn) {
    if constexpr (LGMIN < 6) {
        if (logG <= LGMIN) return fn(so_int<LGMIN>{});
        return so_with_msda_logg<LGMIN + 1>(logG, fn);
    } else {
        return fn(so_int<6>{});
    }
}

// plain forward: whole channel teams (so_pick_group returns G >= D / 4): 22 of the 4 x 7 combinations can be reached
template <class F>
static int so_with_msda_plain_shape(int d, int logG, F &&fn) {
    SO_REQUIRE((1 << logG) >= d / 4, "msda_fwd: group of %d lanes for %d channels", 1 << logG, d);
    return so_with_msda_d(d, [&](auto dd) {
        return so_with_msda_logg<so_ilog2(decltype(dd)::value / 4)>(logG, [&](auto lg) { return fn(dd, lg); });
    });
}

template <class F>
static int so_with_msda_shape(int d, int logG, bool bf16, F &&fn) {
    if (d == 16) {
        SO_REQUIRE(logG >= 2, "msda: group of %d lanes for 16 channels", 1 << logG);
        if (bf16) return so_with_msda_logg<2>(logG, [&](auto lg) { return fn(so_int<16>{}, lg, so_type_tag<uint16_t>{}); });
        return so_with_msda_logg<2>(logG, [&](auto lg) { return fn(so_int<16>{}, lg, so_type_tag<float>{}); });
    }
    SO_REQUIRE(!bf16, "msda: bfloat16 value is built for 16 channels per head only (got %d)", d);
    SO_REQUIRE(d == 8 || d == 32,
               "msda fused / camera-loop forms: channels per head must be 8, 16 or 32 (got %d); the plain form takes 4", d);
    SO_REQUIRE(logG >= (d == 8 ? 1 : 3), "msda: bad group");
    if (d == 8) return so_with_msda_logg<1>(logG, [&](auto lg) { return fn(so_int<8>{}, lg, so_type_tag<float>{}); });
    return so_with_msda_logg<3>(logG, [&](auto lg) { return fn(so_int<32>{}, lg, so_type_tag<float>{}); });
}

// ---- banded backward -------------------------------------------------------------------------
static size_t so_band_key_bytes(long long n_pts) { return (size_t)((n_pts + 8) * 2 + 15) / 16 * 16; }
// counters of the binned scatter: cnt / cursor / off per bucket (2 per band), item0 per band (+ 1)
static size_t so_bin_counter_bytes(int bs, int heads, int L) {
    const size_t nb = (size_t)bs * heads * L * kMaxBands;
    return ((7 * nb + 1) * 4 + 15) / 16 * 16;
}
// per point: 2 (key) + 16 (record) + 8 (index lists: a point is in <= 2 bands) bytes
static size_t so_band_ws_bytes(int bs, int nq, int heads, int L, int P) {
    const long long n_pts = (long long)bs * nq * heads * L * P;
    return so_band_key_bytes(n_pts) + (size_t)n_pts * 16 + so_bin_counter_bytes(bs, heads, L) + (size_t)n_pts * 8;
}

namespace {
constexpr int kBandBlock = 512;     // threads of the band kernel (its 52 KB tile: two blocks per CU)
constexpr int kBandSeg = 4096;      // list entries per band-kernel block

struct BandSetup {
    MsdaBinPlan bin;
    int tile_px;   // pixels of the largest band
    bool ok;       // false: a level is wider than the LDS tile or needs > kMaxBands bands, or the index space overflows
};

// bands: as many rows as the tile holds (the fewer bands, the fewer points straddle two)
int so_band_setup(const int32_t *host_shapes, int bs, int nq, int heads, int d, int L, int P, BandSetup &bsu) {
    MsdaBinPlan &bp = bsu.bin;
    const int cap_px = band_tile_bytes(kBandBlock) / (8 * d);
    bsu.ok = L <= 8;
    bsu.tile_px = 0;
    int nb = 0;
    for (int l = 0; l < 8; ++l) { bp.rows[l] = 1; bp.bands[l] = 0; bp.band0[l] = 0; bp.inv_rows[l] = 1.0f; }
    for (int l = 0; l < L && bsu.ok; ++l) {
        const int Hl = host_shapes[2 * l], Wl = host_shapes[2 * l + 1];
        SO_REQUIRE(Hl >= 0 && Wl >= 0 && Hl < 32767 && Wl < 32767, "msda banded: bad level shape (%d, %d)", Hl, Wl);
        bp.band0[l] = nb;
        if (Hl == 0 || Wl == 0) continue;
        if (Wl > cap_px) { bsu.ok = false; break; }
        bp.rows[l] = std::min(Hl, cap_px / Wl);
        bp.inv_rows[l] = 1.0f / (float)bp.rows[l];
        bp.bands[l] = (Hl + bp.rows[l] - 1) / bp.rows[l];
        if (bp.bands[l] > kMaxBands) { bsu.ok = false; break; }
        nb += bp.bands[l];
        bsu.tile_px = std::max(bsu.tile_px, bp.rows[l] * Wl);
    }
    for (int l = L; l <= 8; ++l) bp.band0[std::min(l, 8)] = nb;
    bp.nbands = nb;
    bp.seg = kBandSeg;
    int lg = 0;
    while ((1LL << lg) < P) ++lg;
    bp.divP.l = lg;
    bp.divP.m = (unsigned)((((1ULL << lg) - (unsigned)P) << 32) / (unsigned)P + 1);
    const long long n_pts = (long long)bs * nq * heads * L * P;
    if (nb == 0 || (long long)bs * heads * nb >= (1LL << 28) || 2 * n_pts >= (1LL << 31) ||
        (long long)nq * P >= (1LL << 31))
        bsu.ok = false;
    return 0;
}

struct BandWorkspace {
    int16_t *keys;
    float4 *recs;
    int32_t *counters;   // cnt[2 nb] cursor[2 nb] off[2 nb] item0[nb + 1], nb = bands actually used
    int32_t *list;       // 2 * n_pts entries
    long long n_pts;
};

BandWorkspace so_band_workspace(void *workspace, int bs, int nq, int heads, int L, int P) {
    const long long n_pts = (long long)bs * nq * heads * L * P;
    BandWorkspace w;
    w.keys = (int16_t *)workspace;
    w.recs = (float4 *)((char *)workspace + so_band_key_bytes(n_pts));
    w.counters = (int32_t *)((char *)w.recs + (size_t)n_pts * 16);
    w.list = (int32_t *)((char *)w.counters + so_bin_counter_bytes(bs, heads, L));
    w.n_pts = n_pts;
    return w;
}

// counting sort + band scatter (after a point kernel filled keys / recs).  vis != NULL: camera loop, the keys of
// invisible (camera, query) pairs are unwritten and must not be read (needs P >= 4, see msda_bin_kernel)
int so_band_scatter(const int32_t *shapes, const int32_t *starts, const float *g_out, float *g_value,
                    const BandWorkspace &w, const BandSetup &bsu, MsdaDims dm, int d, const unsigned char *vis,
                    hipStream_t st, bool counted = false, int gv_stride = 0) {
    const MsdaBinPlan &bp = bsu.bin;
    // g_value in its own layout (round 6): rows of gv_stride floats per pixel, this op's heads * d channels at the pointer —
    // a column block of the row-major gradient of a (stacked) value projection, whatever layout `value` itself was gathered from
    MsdaDims dm_g = dm;
    if (gv_stride > 0) { dm_g.hm = 0; dm_g.vs = gv_stride; }
    const int nb = dm.bs * dm.heads * bp.nbands;                 // bands over all (batch, head)
    int32_t *cnt = w.counters, *cursor = cnt + 2 * (size_t)nb, *off = cursor + 2 * (size_t)nb, *item0 = off + 2 * (size_t)nb;
    const long long n = (long long)dm.nq * dm.P;
    const int bpb = (int)((n + 3 + kBinKeysPerBlock - 1) / kBinKeysPerBlock);   // windows start 8-byte aligned: <= 3 keys early
    const long long bin_blocks = (long long)dm.bs * dm.heads * dm.L * bpb;
    const long long max_items = nb + (2 * w.n_pts) / bp.seg;
    SO_REQUIRE(bin_blocks < (1LL << 31) && max_items < (1LL << 31), "msda banded: grid too large");
    if (!counted) {      // counted: the point kernel zeroed-and-filled cnt (and zeroed cursor) already
        (void)hipMemsetAsync(cnt, 0, (size_t)nb * 4 * sizeof(int32_t), st);     // cnt and cursor
        hipLaunchKernelGGL(msda_bin_kernel<false>, dim3((unsigned)bin_blocks), dim3(256), 0, st, w.keys, shapes, cnt,
                           cursor, off, w.list, vis, bpb, dm, bp);
    }
    hipLaunchKernelGGL(msda_bin_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, off, item0, nb, bp.seg);
    hipLaunchKernelGGL(msda_bin_kernel<true>, dim3((unsigned)bin_blocks), dim3(256), 0, st, w.keys, shapes, cnt,
                       cursor, off, w.list, vis, bpb, dm, bp);
    const size_t shm = (size_t)bsu.tile_px * d * sizeof(double);
    // the grid is an upper bound (every point in two bands): blocks past item0[nb] return at once
    so_with_msda_d(d, [&](auto dd) {
        constexpr int D = decltype(dd)::value;
        // per launch: the attribute is per device (a process may drive several GPUs)
        (void)hipFuncSetAttribute((const void *)msda_bwd_band_list_kernel<D, kBandBlock>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, band_tile_bytes(kBandBlock));
        hipLaunchKernelGGL((msda_bwd_band_list_kernel<D, kBandBlock>), dim3((unsigned)max_items), dim3(kBandBlock), shm, st,
                           shapes, starts, g_out, g_value, w.recs, cnt, off, item0, w.list, nb, dm_g, bp);
        return 0;
    });
    return so_launch_status();
}

// ---- the argument checks -----------------------------------------------------------------------
// the form and the sizes: everything selfocc_msda_banded_supported reads besides host_shapes
int so_msda_check_sizes(const so_msda_args *a) {
    SO_REQUIRE(a != nullptr, "msda: args is NULL");
    SO_REQUIRE(a->form == SO_MSDA_PLAIN || a->form == SO_MSDA_FUSED || a->form == SO_MSDA_CROSS,
               "msda: form must be SO_MSDA_PLAIN, SO_MSDA_FUSED or SO_MSDA_CROSS (got %d)", a->form);
    SO_REQUIRE(a->form != SO_MSDA_CROSS || a->bs >= 1, "msda (camera loop): bs = cams must be >= 1");
    SO_REQUIRE(a->bs >= 0 && a->nq >= 0 && a->nv >= 0, "msda: negative size");
    SO_REQUIRE(a->heads >= 1 && a->L >= 1 && a->P >= 1, "msda: heads, L, P must be >= 1");
    SO_REQUIRE(a->d == 4 || a->d == 8 || a->d == 16 || a->d == 32,
               "msda: channels per head must be 4, 8, 16 or 32 (got %d)", a->d);
    return 0;
}

// every check of selfocc_msda_fwd / _bwd, before anything is launched: first what every form shares, then what one
// form adds, then (for a call with work to do) the pointers it reads and writes
int so_msda_check(const so_msda_args *args, bool bwd) {
    if (so_msda_check_sizes(args)) return -1;
    const so_msda_args &a = *args;
    const bool plain = a.form == SO_MSDA_PLAIN, cross = a.form == SO_MSDA_CROSS;
    const int hd = a.heads * a.d, LP = a.L * a.P;
    SO_REQUIRE((long long)a.bs * a.nq * a.heads * LP < (1LL << 40), "msda: problem too large");
    SO_REQUIRE((long long)a.bs * a.nv * hd < (1LL << 31) && (long long)a.bs * a.nq * hd < (1LL << 31),
               "msda: value / output tensors must have < 2^31 elements");
    SO_REQUIRE(a.value_stride == 0 || (cross && !bwd), "msda: value_stride is for the camera-loop forward only (got %d)",
               a.value_stride);
    if (plain) {
        SO_REQUIRE(a.value_layout == SO_VALUE_PIXEL_MAJOR && a.value_dtype == SO_DTYPE_F32,
                   "msda (plain): value must be float32 and pixel-major");
        SO_REQUIRE(!bwd || a.g_value_stride == 0, "msda (plain): g_value_stride must be 0");
    } else {
        SO_REQUIRE(a.value_dtype == SO_DTYPE_F32 || a.value_dtype == SO_DTYPE_BF16, "msda: bad value_dtype");
        SO_REQUIRE(a.value_layout == SO_VALUE_PIXEL_MAJOR || a.value_layout == SO_VALUE_HEAD_MAJOR,
                   "msda: bad value_layout");
        SO_REQUIRE(a.form != SO_MSDA_FUSED || (a.ref_kind >= 0 && a.ref_kind <= 2), "msda: ref_kind must be 0, 1 or 2");
        SO_REQUIRE(LP <= 256, "msda: L * P must be <= 256 for the fused / camera-loop forms (got %d); use the plain form", LP);
        // off_raw / logits: dense tensors, or one merged [offsets | logits] projection row per query
        SO_REQUIRE(a.ol_stride == 0 || (a.ol_stride >= 3 * a.heads * LP && a.ol_stride % 2 == 0),
                   "msda: ol_stride must be 0 (dense) or an even number >= 3 * heads * L * P = %d (got %d)",
                   3 * a.heads * LP, a.ol_stride);
        SO_REQUIRE(a.ol_stride == 0 || ((((uintptr_t)a.off_raw) | (bwd ? (uintptr_t)a.g_off : 0)) & 7) == 0,
                   "msda: off_raw and g_off must be 8-byte aligned with an ol_stride");
        SO_REQUIRE((long long)(cross ? 1 : a.bs) * a.nq * a.ol_stride < (1LL << 40), "msda: offsets / logits too large");
        SO_REQUIRE(!bwd || a.g_value_stride == 0 || (a.g_value_stride >= hd && (long long)a.bs * a.nv * a.g_value_stride < (1LL << 31)),
                   "msda: g_value_stride must be 0 or >= heads * d with bs * nv * stride < 2^31 (got %d)", a.g_value_stride);
    }
    if (cross) {
        SO_REQUIRE(a.value_layout == SO_VALUE_PIXEL_MAJOR || a.value_stride == 0,
                   "msda (camera loop): head-major values are dense: value_stride must be 0");
        SO_REQUIRE(a.value_stride == 0 || (a.value_stride >= hd && a.value_stride % 4 == 0),
                   "msda (camera loop): value_stride must be 0 or a multiple of 4 >= heads * d");
        SO_REQUIRE((long long)a.bs * a.nv * (a.value_stride ? a.value_stride : hd) < (1LL << 31),
                   "msda (camera loop): value must span < 2^31 floats");
        SO_REQUIRE((long long)a.nq * a.heads < (1LL << 31), "msda (camera loop): nq * heads must be < 2^31");
    }
    if (a.bs == 0 || a.nq == 0) return 0;   // nothing to do: no pointer is read
#define SO_NEED(p) SO_REQUIRE(a.p != nullptr, "msda: " #p " is NULL")
    SO_NEED(value); SO_NEED(shapes); SO_NEED(starts);
    if (plain) { SO_NEED(loc); SO_NEED(attw); }
    else { SO_NEED(ref); SO_NEED(off_raw); SO_NEED(logits); }
    if (cross) SO_NEED(vis);
    if (!bwd) {
        SO_NEED(out);
        return 0;
    }
    SO_NEED(g_out); SO_NEED(g_value);
    if (plain) { SO_NEED(g_loc); SO_NEED(g_attw); }
    else { SO_NEED(g_off); SO_NEED(g_logits); }
#undef SO_NEED
    if (plain && a.host_shapes == nullptr) return 0;   // the global-atomic scatter: no workspace
    SO_REQUIRE(a.host_shapes != nullptr, "msda: host_shapes is NULL (host copy of the (L, 2) level shapes)");
    SO_REQUIRE(a.L <= 8, "msda: the banded backward takes at most 8 levels (got %d)", a.L);
    const size_t need = so_band_ws_bytes(a.bs, a.nq, a.heads, a.L, a.P);
    SO_REQUIRE(a.workspace != nullptr && a.workspace_bytes >= need, "msda: workspace too small (%llu bytes, need %zu)",
               (unsigned long long)a.workspace_bytes, need);
    SO_REQUIRE(((uintptr_t)a.workspace & 15) == 0, "msda: workspace must be 16-byte aligned");
    return 0;
}

// what the kernels see of a call: the camera-loop forward addresses one camera's value at a time (bs = 1), its backward
// shares the rows of g_out between the cameras
MsdaDims so_msda_dims(const so_msda_args &a, bool bwd) {
    const bool cross = a.form == SO_MSDA_CROSS;
    MsdaDims dm{cross && !bwd ? 1 : a.bs, a.nv, a.nq, a.heads, a.L, a.P, cross && bwd ? 1 : 0, a.value_stride, a.value_layout};
    if (a.form != SO_MSDA_PLAIN) {
        const int LP = a.L * a.P;
        dm.off_ld = a.ol_stride ? a.ol_stride : a.heads * LP * 2;
        dm.lg_ld = a.ol_stride ? a.ol_stride : a.heads * LP;
    }
    return dm;
}

// the two host decisions of the camera-loop backward (selfocc_msda_bwd; reported by selfocc_msda_plan).  gpb: groups per block
struct CrossBwdPlan {
    bool bin_vis;        // the bin kernels skip invisible (camera, query) pairs by `vis`; else their keys are preset to "outside"
    bool count_here;     // the point kernel counts the sort's buckets in an LDS histogram of hist_need bytes
    size_t hist_need;
};

CrossBwdPlan so_cross_bwd_plan(const so_msda_args &a, const BandSetup &bsu, int gpb) {
    CrossBwdPlan cp;
    cp.bin_vis = a.P >= 4;
    cp.hist_need = (size_t)2 * a.bs * bsu.bin.nbands * 2 * sizeof(int);
    cp.count_here = a.nq >= gpb && cp.hist_need <= 32 * 1024;
    return cp;
}
}  // namespace

extern "C" size_t selfocc_msda_ws_bytes(const so_msda_args *a) {
    if (a == nullptr || a->form < SO_MSDA_PLAIN || a->form > SO_MSDA_CROSS || a->bs < 0 || a->nq < 0 || a->heads < 1 ||
        a->L < 1 || a->P < 1)
        return 0;
    return so_band_ws_bytes(a->bs, a->nq, a->heads, a->L, a->P);
}

extern "C" int selfocc_msda_banded_supported(const so_msda_args *a) {
    if (so_msda_check_sizes(a)) return -1;
    SO_REQUIRE(a->host_shapes != nullptr, "msda banded: host_shapes is NULL");
    if (a->L > 8) return 0;
    BandSetup bsu;
    if (so_band_setup(a->host_shapes, a->bs, a->nq, a->heads, a->d, a->L, a->P, bsu)) return -1;
    return bsu.ok ? 1 : 0;
}

extern "C" int selfocc_msda_fwd(const so_msda_args *args, void *stream) {
    if (so_msda_check(args, false)) return -1;
    const so_msda_args &a = *args;
    if (a.bs == 0 || a.nq == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const MsdaDims dm = so_msda_dims(a, false);
    const long long n_groups = (long long)dm.bs * a.nq * a.heads;
    if (a.nv == 0)   // nothing to sample: every point is outside every (empty) map
        return (int)hipMemsetAsync(a.out, 0, (size_t)n_groups * a.d * sizeof(float), st);
    const int LP = a.L * a.P, d = a.d;
    int G = 1, logG = 0;
    if (a.form == SO_MSDA_PLAIN)
        so_pick_group(LP, d, 8, G, logG);
    else
        so_pick_group_fused(LP, d, G, logG);
    const int gpb = 256 / G;
    const long long blocks = (n_groups + gpb - 1) / gpb;
    SO_REQUIRE(blocks < (1LL << 31), "msda_fwd: grid too large");
    const bool bf16 = a.value_dtype == SO_DTYPE_BF16;
    const dim3 grid((unsigned)blocks), block(256);
    int rc;
    if (a.form == SO_MSDA_PLAIN) {
        rc = so_with_msda_plain_shape(d, logG, [&](auto dd, auto lg) {
            hipLaunchKernelGGL((msda_fwd_kernel<decltype(dd)::value, decltype(lg)::value>), grid, block, 0, st,
                               (const float *)a.value, a.shapes, a.starts, a.loc, a.attw, a.out, dm);
            return 0;
        });
    } else {
        rc = so_with_msda_shape(d, logG, bf16, [&](auto dd, auto lg, auto vt) {
            constexpr int D = decltype(dd)::value, LG = decltype(lg)::value;
            using VT = typename decltype(vt)::type;
            if (a.form == SO_MSDA_FUSED) {
                hipLaunchKernelGGL((msda_fused_fwd_kernel<D, LG, VT>), grid, block, 0, st, (const VT *)a.value, a.shapes, a.starts,
                                   a.ref, a.ref_kind, a.off_raw, a.logits, a.out, dm);
            } else {
                hipLaunchKernelGGL((msda_cross_fwd_kernel<D, LG, VT>), grid, block, 0, st, (const VT *)a.value, a.shapes, a.starts,
                                   a.ref, a.vis, a.off_raw, a.logits, a.out, a.bs, dm);
            }
            return 0;
        });
    }
    return rc ? rc : so_launch_status();
}

extern "C" int selfocc_msda_bwd(const so_msda_args *args, void *stream) {
    if (so_msda_check(args, true)) return -1;
    const so_msda_args &a = *args;
    if (a.bs == 0 || a.nq == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const MsdaDims dm = so_msda_dims(a, true);
    const int d = a.d, LP = a.L * a.P;
    const long long n_pts = (long long)a.bs * a.nq * a.heads * LP;
    BandSetup bsu{};
    if (a.host_shapes != nullptr && so_band_setup(a.host_shapes, a.bs, a.nq, a.heads, d, a.L, a.P, bsu)) return -1;
    if (a.form == SO_MSDA_PLAIN) {
        const float *value = (const float *)a.value;
        const long long pblocks = (n_pts + 255) / 256;
        SO_REQUIRE(pblocks < (1LL << 31), "msda_bwd: grid too large");
        if (!bsu.ok) {   // no host shapes, or the banded scatter does not apply: global float atomics
            so_with_msda_d(d, [&](auto dd) {
                hipLaunchKernelGGL((msda_bwd_kernel<decltype(dd)::value>), dim3((unsigned)pblocks), dim3(256), 0, st, value,
                                   a.shapes, a.starts, a.loc, a.attw, a.g_out, a.g_value, a.g_loc, a.g_attw, dm);
                return 0;
            });
            return so_launch_status();
        }
        const BandWorkspace w = so_band_workspace(a.workspace, a.bs, a.nq, a.heads, a.L, a.P);
        so_with_msda_d(d, [&](auto dd) {
            hipLaunchKernelGGL((msda_bwd_point_kernel<decltype(dd)::value>), dim3((unsigned)pblocks), dim3(256), 0, st, value,
                               a.shapes, a.starts, a.loc, a.attw, a.g_out, a.g_loc, a.g_attw, w.keys, w.recs, dm);
            return 0;
        });
        return so_band_scatter(a.shapes, a.starts, a.g_out, a.g_value, w, bsu, dm, d, nullptr, st);
    }
    // fused / camera loop: the banded scatter is part of the op
    SO_REQUIRE(bsu.ok, "msda_bwd: the banded scatter does not apply to these shapes "
                       "(check selfocc_msda_banded_supported and use the plain form)");
    const long long rows = (long long)(a.form == SO_MSDA_CROSS ? 1 : a.bs) * a.nq;   // query rows of off_raw / logits
    if (a.nv == 0) {   // every point is outside every (empty) map: all gradients are zero
        if (a.ol_stride)   // merged rows: [offsets | logits] of a query are adjacent
            return (int)hipMemset2DAsync(a.g_off, (size_t)a.ol_stride * sizeof(float), 0, (size_t)3 * a.heads * LP * sizeof(float),
                                         (size_t)rows, st);
        (void)hipMemsetAsync(a.g_off, 0, (size_t)rows * a.heads * LP * 2 * sizeof(float), st);
        return (int)hipMemsetAsync(a.g_logits, 0, (size_t)rows * a.heads * LP * sizeof(float), st);
    }
    const BandWorkspace w = so_band_workspace(a.workspace, a.bs, a.nq, a.heads, a.L, a.P);
    int G = 1, logG = 0;
    so_pick_group_fused(LP, d, G, logG);
    const int gpb = 256 / G;
    const long long blocks = (rows * a.heads + gpb - 1) / gpb;
    SO_REQUIRE(blocks < (1LL << 31), "msda_bwd: grid too large");
    const bool bf16 = a.value_dtype == SO_DTYPE_BF16;
    const dim3 grid((unsigned)blocks), block(256);
    if (a.form == SO_MSDA_FUSED) {
        // (counting the sort's buckets inside this kernel, as the camera loop does, measured slower here: 454 -> 570 us for
        // 58 us of msda_bin_kernel<false>: 32 groups per block contend for the few buckets of one plane)
        if (so_with_msda_shape(d, logG, bf16, [&](auto dd, auto lg, auto vt) {
                using VT = typename decltype(vt)::type;
                hipLaunchKernelGGL((msda_fused_bwd_point_kernel<decltype(dd)::value, decltype(lg)::value, VT>), grid, block, 0, st,
                                   (const VT *)a.value, a.shapes, a.starts, a.ref, a.ref_kind, a.off_raw, a.logits, a.g_out,
                                   a.g_off, a.g_logits, w.keys, w.recs, dm);
                return 0;
            }))
            return -1;
        return so_band_scatter(a.shapes, a.starts, a.g_out, a.g_value, w, bsu, dm, d, nullptr, st, false, a.g_value_stride);
    }
    const int cams = a.bs;
    // the point kernel writes the keys of every (camera, query) pair it visits; the bin kernels skip the others by
    // `vis` (P >= 4), otherwise the unvisited keys are preset to "outside"
    const CrossBwdPlan cp = so_cross_bwd_plan(a, bsu, gpb);
    const unsigned char *bin_vis = cp.bin_vis ? a.vis : nullptr;
    if (bin_vis == nullptr) (void)hipMemsetD16Async((hipDeviceptr_t)w.keys, (unsigned short)0x8000, (size_t)n_pts, st);
    // the point kernel does the sort's counting pass itself (an LDS histogram per block, flushed once) when a block's groups
    // span at most two heads and the histogram fits: saves one pass over the keys (msda_bin_kernel<false>, 0.9 ms per iteration)
    const bool count_here = cp.count_here;
    const size_t hist_bytes = count_here ? cp.hist_need : 0;
    if (count_here) {
        const size_t nb_all = (size_t)cams * a.heads * bsu.bin.nbands;
        (void)hipMemsetAsync(w.counters, 0, nb_all * 4 * sizeof(int32_t), st);      // cnt and cursor, before the counting kernel
    }
    if (so_with_msda_shape(d, logG, bf16, [&](auto dd, auto lg, auto vt) {
            using VT = typename decltype(vt)::type;
            hipLaunchKernelGGL((msda_cross_bwd_point_kernel<decltype(dd)::value, decltype(lg)::value, VT>), grid, block, hist_bytes,
                               st, (const VT *)a.value, a.shapes, a.starts, a.ref, a.vis, a.off_raw, a.logits, a.g_out, a.g_off,
                               a.g_logits, w.keys, w.recs, cams, dm, count_here ? w.counters : nullptr, bsu.bin);
            return 0;
        }))
        return -1;
    return so_band_scatter(a.shapes, a.starts, a.g_out, a.g_value, w, bsu, dm, d, bin_vis, st, count_here, a.g_value_stride);
}

// What the two entries above would decide for this call, without launching anything: host arithmetic only, no pointer but
// host_shapes is read.  The tests ask it which kernel instantiation and which branches a case reaches.
extern "C" int selfocc_msda_plan(const so_msda_args *a, int32_t *out) {
    if (so_msda_check_sizes(a)) return -1;
    SO_REQUIRE(out != nullptr, "msda_plan: out is NULL");
    for (int i = 0; i < SO_MSDA_PLAN_INTS; ++i) out[i] = 0;
    const int LP = a->L * a->P;
    int G = 1, logG = 0;
    if (a->form == SO_MSDA_PLAIN) {
        so_pick_group(LP, a->d, 8, G, logG);
        if (so_with_msda_plain_shape(a->d, logG, [](auto, auto) { return 0; })) return -1;
    } else {
        SO_REQUIRE(a->value_dtype == SO_DTYPE_F32 || a->value_dtype == SO_DTYPE_BF16, "msda: bad value_dtype");
        SO_REQUIRE(LP <= 256, "msda: L * P must be <= 256 for the fused / camera-loop forms (got %d); use the plain form", LP);
        so_pick_group_fused(LP, a->d, G, logG);
        if (so_with_msda_shape(a->d, logG, a->value_dtype == SO_DTYPE_BF16, [](auto, auto, auto) { return 0; })) return -1;
    }
    out[SO_MSDA_PLAN_LOG2_GROUP] = logG;
    if (a->host_shapes == nullptr) return 0;
    BandSetup bsu{};
    if (so_band_setup(a->host_shapes, a->bs, a->nq, a->heads, a->d, a->L, a->P, bsu)) return -1;
    out[SO_MSDA_PLAN_BANDED] = bsu.ok ? 1 : 0;
    if (a->form == SO_MSDA_CROSS && bsu.ok) {   // as selfocc_msda_bwd decides them
        const CrossBwdPlan cp = so_cross_bwd_plan(*a, bsu, 256 / G);
        out[SO_MSDA_PLAN_COUNT_HERE] = cp.count_here ? 1 : 0;
        out[SO_MSDA_PLAN_BIN_VIS] = cp.bin_vis ? 1 : 0;
    }
    for (int l = 0; l < a->L && l < 8; ++l) {
        out[SO_MSDA_PLAN_BANDS + l] = bsu.bin.bands[l];
        out[SO_MSDA_PLAN_ROWS + l] = bsu.bin.rows[l];
    }
    return 0;
}
