// render_bwd.hip — backward of the fused SDF ray-march renderer for gfx950 (MI355X).
//
// What the reference gets from autograd through ~40 torch ops + cuda_gridsample_grad2's
// double-backward: d loss / d volume (SDF + colour/semantic channels) and
// d loss / d inv_s, given upstream gradients of every differentiable output of
// selfocc_render_fwd: depth, acc, rgb, sem, per-sample weights, per-sample sdf and the
// per-sample metre gradient (eikonal term).
//
// Hardware mapping: ONE WAVEFRONT PER RAY, lane l owns the M = ceil(S / 64) consecutive
// samples [l*M, (l+1)*M).  All per-sample state lives in registers; the two recurrences
//   transmittance  T_i = prod_{j<i} f_j,            f_j = 1 - alpha_j + 1e-7   (forward)
//   E_i = Gw_{i+1} alpha_{i+1} + f_{i+1} E_{i+1}                                 (reverse)
// are scans over wavefront shuffles (the reverse one composes affine maps, so there is no
// division by the tiny f_i that a "suffix sum / f_i" formulation would need).
// d L / d alpha_i = T_i (Gw_i - E_i), Gw_i = total derivative of the loss wrt weight i.
// The volume gradient is a scatter of 8 (+ 8 * n_feat) hardware float atomics per sample.
#include "so_device.h"
#include "sh_device.h"
#include "ray_device.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int kMaxM = 8;  // samples per lane: S <= 512

template <int NF, bool BF16>
SO_DEVFN void load_feat(const void *vol, size_t vox, float f[NF > 0 ? NF : 1]) {
    if constexpr (!BF16) {
        const float4 *p = (const float4 *)((const float *)vol + vox * NF);
#pragma unroll
        for (int q = 0; q < NF / 4; ++q) {
            const float4 t = p[q];
            f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
        }
    } else {
        const uint2 *p = (const uint2 *)((const uint16_t *)vol + vox * NF);
#pragma unroll
        for (int q = 0; q < NF / 4; ++q) {
            const uint2 t = p[q];
            f[4 * q] = __uint_as_float(t.x << 16); f[4 * q + 1] = __uint_as_float(t.x & 0xffff0000u);
            f[4 * q + 2] = __uint_as_float(t.y << 16); f[4 * q + 3] = __uint_as_float(t.y & 0xffff0000u);
        }
    }
}

// ---- brick-binned scatter (so_render_bwd_args::scatter_ws) -----------------------------------------------
// The volume is cut into bricks of kBH x kBW x kBD CELLS; the voxels a brick's samples touch are the
// (kBH + 1)(kBW + 1)(kBD + 1) tile that shares its upper faces with the neighbouring bricks.
//   rb_count_kernel   one wave per ray: every sample's cell (same code as the ray kernel) -> its brick; counts the samples
//                     per (brick, shard): runs of consecutive samples with one counter, summed per 16-ray block in LDS first
//   rb_scan1 / scan2  counts -> slot cursors per (brick, shard) and a list of work items (brick, <= chunk samples)
//   render_bwd_kernel<.., BIN = true>  takes the slots of its runs (one returning atomic per run, issued early) and
//                     writes ONE RECORD PER SAMPLE AT ITS SLOT, i.e. in brick order.  A record is RECF floats:
//                         [0 .. NCH)        d L / d (interpolated feature channel)
//                         [RECF - 8]        ds                (coefficient of the trilinear weights in d L / d sdf corner)
//                         [RECF - 7]        packed cell       ((h0 + 2) << 20 | (w0 + 2) << 10 | (d0 + 2), as bits; indices clamped to [-2, 1021])
//                         [RECF - 6 .. -4]  fh1, fw1, fd1     (fractions inside the cell)
//                         [RECF - 3 .. -1]  qx, qy, qz        (coefficients of the weights' axis derivatives)
//   rb_brick_kernel   one workgroup per item: streams the item's records, sums them into the brick's tile in LDS and
//                     adds the tile's non-zero rows to the gradient volumes: (items x touched rows) row atomics instead
//                     of (sample runs x 8).  The tile is DOUBLE: ds_add_f64 issues in ~15 clocks per 64-lane
//                     instruction on gfx950, ds_add_f32 in ~190 (scripts/micro/lds_atomic_types.hip; the first version
//                     of this kernel, with a float tile, took 7.7 ms).
constexpr int kBH = 4, kBW = 4, kBD = 8;
constexpr int kTH = kBH + 1, kTW = kBW + 1, kTD = kBD + 1;
constexpr int kTileVox = kTH * kTW * kTD;   // 225
constexpr int kInvsSlots = 1024;
constexpr int kShards = 32;  // counters per brick (shard = bits 8.. of the sample index): the bricks around the cameras
                             // are entered by every ray, and same-address device atomics serialise
SO_DEVFN int rb_shard(long long sample) { return (int)(sample >> 8) & (kShards - 1); }

// NB > 0 (spherical harmonics): the record's feature part is {g_raw[3], dx, dy, dz, 0, 0} at every degree, and a sample is
// served by 32 lanes of the brick kernel (3 * NB <= 27 coefficient channels)
template <int NF, int NB = 0>
struct RbRec {
    static constexpr int NCH = NB > 0 ? 3 * NB : (NF == 4 ? 3 : NF);                 // feature channels with a gradient
    static constexpr int RECF = NB > 0 ? 16 : (NF >= 12 ? 32 : (NF >= 4 ? 16 : 8));  // floats per record (>= NF + 8)
    static constexpr int LPG = NB > 0 ? 32 : RECF;                                    // lanes per sample in rb_brick_kernel
    static constexpr int RW = NCH + 1;                                                // tile row: features then the sdf column
};

struct RbBin {
    float *rec;        // [n_rays * n_samples][RECF], in brick order
    int *counts;       // [n_bricks][kShards] (zeroed per call, together with invs_part and n_items)
    float *invs_part;  // [kInvsSlots]     partial sums of d L / d inv_s
    int *n_items;      // [1]
    int *cursor;       // [n_bricks][kShards] next free slot
    int2 *blk_tot;     // [ceil(n_bricks / 1024)] (samples, items) per scan block
    int4 *items;       // [max_items] {brick, begin, end, -}
    int nbh, nbw, nbd, chunk;
    int dbg;           // dev switches (SELFOCC_RB_DBG): 1 = no accumulation, 2 = no flush, 4 = no run merging, 8 = the ray kernel
                       // does not write the feature part of its records, 16 = the brick kernel does not read it (timing only:
                       // 8 + 16 = the traffic of a 32-byte record, profiles/r5_c_render_bwd_record_bound.txt)
};

SO_DEVFN int rb_key(const RbBin &b, const so_cell &c, int H, int W, int D) {
    const int bh = min(max(c.h0, 0), H - 1) / kBH, bw = min(max(c.w0, 0), W - 1) / kBW, bd = min(max(c.d0, 0), D - 1) / kBD;
    return (bh * b.nbw + bw) * b.nbd + bd;
}

// the cell of sample i: ONE definition for the ray kernel and the counting pre-pass (they must agree on every sample's
// brick; the ray, its collider bounds and the bin edges are those of ray_device.h)
template <int MK = SO_MAP_LINEAR>
SO_DEVFN so_cell sample_cell(const so_render_args &a, const RayGeom &g, float t0, float t1) {
    float px, py, pz;
    if (a.sample_pos == SO_SAMPLE_AT_START) {
        px = g.ox + g.dx * t0; py = g.oy + g.dy * t0; pz = g.oz + g.dz * t0;
    } else {
        const float tt = t0 + t1;
        px = g.ox + (g.dx * tt) / 2.0f; py = g.oy + (g.dy * tt) / 2.0f; pz = g.oz + (g.dz * tt) / 2.0f;
    }
    return so_locate_k<MK>(a.map, px, py, pz);
}

// run of consecutive lanes with one key: returns the run's length at its head lane (0 elsewhere) and the head's lane
SO_DEVFN int rb_run(int key, int lane, int &head_lane) {
    const int prev = __shfl_up(key, 1, 64);
    const bool head = (lane == 0) || (key != prev);
    const unsigned long long hm = __ballot(head);
    const unsigned long long upto = hm & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));   // heads at lanes <= mine
    head_lane = 63 - __clzll((long long)upto);
    if (!head) return 0;
    const unsigned long long later = (lane == 63) ? 0ull : (hm >> (lane + 1));
    return later ? __ffsll((long long)later) : 64 - lane;
}

// WPR = waves per ray.  WPR == 1: a wave owns a ray and M * 64 samples (4 rays per block).  WPR == 4: the
// block's four waves share one ray, wave w taking step (j * 4 + w) — at the shipped 256 samples per ray
// that is M = 1, which cuts the per-sample register state 4x (the M = 4 form needed > 256 VGPRs: one wave
// per SIMD, latency-bound); scan carries and per-ray sums cross the waves through a few floats of LDS.
// (Measured and dropped, round 4: forcing the 24-channel BIN instantiation to 3 / 4 waves per SIMD with
// amdgpu_waves_per_eu — 168 / 128 VGPRs, 296 / 484 B of scratch — 0.98 -> 1.67 / 1.96 ms: the spills land in the corner loops.)
// MK = mapping kind (so_locate_k): the 'linear_upscale' instances differ only in sample_cell
// NB > 0: spherical-harmonics colour with NB basis functions (sh_device.h), NF = the row stride of the coefficients.
// d L / d f[c * NB + k] = g_raw_c * Y_k is rank one per sample: the atomic scatter expands it into the row it parks in LDS,
// the binned scatter stores g_raw[3] and the ray's unit direction in a 64-byte record and leaves the expansion to the brick kernel.
template <int NF, bool BF16, int M, int WPR, bool BIN, int MK = SO_MAP_LINEAR>
__global__ __launch_bounds__(256) void render_bwd_kernel(so_render_bwd_args ba, RbBin bin) {
    constexpr int NB = NF < 0 ? 1 : 0;   // no spherical harmonics (spelled value-dependent: the NB > 0 branches are never instantiated)
    constexpr bool MASKED = false;
#include "render_bwd_body.h"
}
template <int NB, int M, int WPR, bool BIN, int MK>
__global__ __launch_bounds__(256) void render_bwd_sh_kernel(so_render_bwd_args ba, RbBin bin) {
    constexpr int NF = so_sh_stride(NB);
    constexpr bool BF16 = false;
    constexpr bool MASKED = false;
#include "render_bwd_body.h"
}
// any class count from 2 to 21: float32 rows of NF = 8, 12, 16, 20, 24 floats with a.n_sem in [NF - 6, NF - 3] logits
// and up to three pad channels.  The binned scatter shares rb_brick_kernel<NF> with the unmasked widths: a pad channel's
// record entry is an exact 0, which the brick kernel does not add.
template <int NF, int M, int WPR, bool BIN, int MK>
__global__ __launch_bounds__(256) void render_ns_bwd_kernel(so_render_bwd_args ba, RbBin bin) {
    constexpr int NB = NF < 0 ? 1 : 0;
    constexpr bool BF16 = false;
    constexpr bool MASKED = true;
#include "render_bwd_body.h"
}

// ---- the binned scatter's own kernels ---------------------------------------------------------------------
// one wave per ray (the ray's geometry once per lane, then S / 64 steps of 64 consecutive samples), 16 rays per block.
// Neighbouring rays cross the same bricks, and every ray starts in the bricks around the cameras: the block first sums its
// runs in a small LDS table (direct-mapped on the counter index; a collision goes to memory directly) and adds each
// occupied slot to the global counter once.  (0.24 ms with one atomic per run and 8 shards, 0.16 - 0.22 ms with 32 shards,
// with or without the table: what is left is the ~30 IEEE divisions per sample of the canonical cell, which the pass must
// repeat exactly.)
constexpr int kCountWaves = 16, kCountSlots = 1024;
template <int MK>
SO_DEVFN void rb_count_body(const so_render_args &a, const RbBin &b) {
    __shared__ int tkey[kCountSlots], tcnt[kCountSlots];
    for (int k = threadIdx.x; k < kCountSlots; k += kCountWaves * 64) { tkey[k] = -1; tcnt[k] = 0; }
    __syncthreads();
    const int ray = blockIdx.x * kCountWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ray < a.n_rays) {   // wave-uniform
        const int S = a.n_samples;
        const RayGeom g = so_ray_of(a, ray);
        float tn, tf;
        so_collide(a, g, tn, tf);
        const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int smp = s0 + lane;
            int key = -1;
            if (smp < S) {
                const so_cell c = sample_cell<MK>(a, g, so_edge(a, ray, smp, tn, tf), so_edge(a, ray, smp + 1, tn, tf));
                key = rb_key(b, c, H, W, D) * kShards + rb_shard((long long)ray * S + smp);
            }
            int hl;
            const int run = rb_run(key, lane, hl);
            if (run > 0 && key >= 0) {
                const int slot = (key * 0x9E3779B1u) >> 22;                  // 10 bits
                const int old = atomicCAS(&tkey[slot], -1, key);
                if (old == -1 || old == key) atomicAdd(&tcnt[slot], run);
                else atomicAdd(b.counts + key, run);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kCountSlots; k += kCountWaves * 64)
        if (tkey[k] >= 0 && tcnt[k] > 0) atomicAdd(b.counts + tkey[k], tcnt[k]);
}
__global__ __launch_bounds__(kCountWaves * 64) void rb_count_kernel(so_render_args a, RbBin b) { rb_count_body<SO_MAP_LINEAR>(a, b); }
__global__ __launch_bounds__(kCountWaves * 64) void rb_count_up_kernel(so_render_args a, RbBin b) { rb_count_body<SO_MAP_UPSCALE>(a, b); }

// counts -> cursors + items, in two launches of ceil(n_bricks / 1024) blocks: per-block totals, then the scan proper
__global__ __launch_bounds__(1024) void rb_scan1_kernel(RbBin b) {
    __shared__ int sc[16], sn[16];
    const int nb = b.nbh * b.nbw * b.nbd;
    const int k = blockIdx.x * 1024 + threadIdx.x;
    int c = 0;
    if (k < nb) {
        const int4 *p = (const int4 *)(b.counts + (size_t)k * kShards);
#pragma unroll
        for (int q = 0; q < kShards / 4; ++q) {
            const int4 x = p[q];
            c += (x.x + x.y) + (x.z + x.w);
        }
    }
    int n = (c + b.chunk - 1) / b.chunk;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { c += __shfl_xor(c, m, 64); n += __shfl_xor(n, m, 64); }
    if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = c; sn[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int cc = 0, nn = 0;
        for (int w = 0; w < 16; ++w) { cc += sc[w]; nn += sn[w]; }
        b.blk_tot[blockIdx.x] = make_int2(cc, nn);
    }
}

__global__ __launch_bounds__(1024) void rb_scan2_kernel(RbBin b) {
    __shared__ int sc[1024], sn[1024];
    static_assert(kShards % 4 == 0, "int4 loads");
    const int t = threadIdx.x;
    const int nb = b.nbh * b.nbw * b.nbd;
    const int k = blockIdx.x * 1024 + t;
    int cs[kShards];
    int c = 0;
    if (k < nb) {
        const int4 *p = (const int4 *)(b.counts + (size_t)k * kShards);
#pragma unroll
        for (int q = 0; q < kShards / 4; ++q) {
            const int4 x = p[q];
            cs[4 * q] = x.x; cs[4 * q + 1] = x.y; cs[4 * q + 2] = x.z; cs[4 * q + 3] = x.w;
        }
#pragma unroll
        for (int sh = 0; sh < kShards; ++sh) c += cs[sh];
    }
    const int n = (c + b.chunk - 1) / b.chunk;
    int c0 = 0, n0 = 0;   // totals of the earlier blocks
    for (int q = 0; q < (int)blockIdx.x; ++q) { const int2 v = b.blk_tot[q]; c0 += v.x; n0 += v.y; }
    sc[t] = c; sn[t] = n;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scans (samples, items)
        const int oc = t >= d ? sc[t - d] : 0, on = t >= d ? sn[t - d] : 0;
        __syncthreads();
        sc[t] += oc; sn[t] += on;
        __syncthreads();
    }
    if (k < nb) {
        const int coff = c0 + sc[t] - c;
        int noff = n0 + sn[t] - n;
        int run = coff;
        int4 *qv = (int4 *)(b.cursor + (size_t)k * kShards);   // a brick's shards are consecutive ranges of the sorted order
#pragma unroll
        for (int q = 0; q < kShards / 4; ++q) {
            int4 x;
            x.x = run; run += cs[4 * q]; x.y = run; run += cs[4 * q + 1]; x.z = run; run += cs[4 * q + 2]; x.w = run; run += cs[4 * q + 3];
            qv[q] = x;
        }
        for (int o = 0; o < c; o += b.chunk) b.items[noff++] = make_int4(k, coff + o, coff + min(o + b.chunk, c), 0);
    }
    if (blockIdx.x == gridDim.x - 1 && t == 1023) b.n_items[0] = n0 + sn[1023];
}

// One workgroup per item: the item's records (contiguous) summed into the brick's tile in LDS, the tile added to the volumes.
// Y_k(x, y, z) for a lane-varying k (a register array indexed by it would live in scratch)
SO_DEVFN float rb_sh_one(int k, float x, float y, float z) {
    switch (k) {
        case 0: return 0.28209479177387814f;
        case 1: return -0.4886025119029199f * y;
        case 2: return 0.4886025119029199f * z;
        case 3: return -0.4886025119029199f * x;
        case 4: return 1.0925484305920792f * (x * y);
        case 5: return -1.0925484305920792f * (y * z);
        case 6: return 0.31539156525252005f * ((2.0f * (z * z) - x * x) - y * y);
        case 7: return -1.0925484305920792f * (x * z);
        default: return 0.5462742152960396f * (x * x - y * y);
    }
}

// NB > 0: spherical-harmonics records (RbRec<NF, NB>): 32 lanes per sample, lane `sub` < 3 * NB owns coefficient channel sub and
// expands g_raw[sub / NB] * Y_(sub % NB)(direction) itself; the last 8 lanes of the 32 ALSO own one sdf corner each.
template <int NF, int NT>
__global__ __launch_bounds__(NT) void rb_brick_kernel(RbBin b, float *__restrict__ g_sdf_vol, float *__restrict__ g_feat_vol,
                                                      float *__restrict__ g_inv_s, int H, int W, int D) {
    constexpr int NB = NF < 0 ? 1 : 0;   // no spherical harmonics
#include "render_bwd_brick_body.h"
}
template <int NB, int NT>
__global__ __launch_bounds__(NT) void rb_brick_sh_kernel(RbBin b, float *__restrict__ g_sdf_vol, float *__restrict__ g_feat_vol,
                                                         float *__restrict__ g_inv_s, int H, int W, int D) {
    constexpr int NF = so_sh_stride(NB);
#include "render_bwd_brick_body.h"
}

inline size_t rb_align(size_t x) { return (x + 255) & ~(size_t)255; }

inline size_t rb_bricks(const so_render_args &a, RbBin *b) {
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int nbh = (H + kBH - 1) / kBH, nbw = (W + kBW - 1) / kBW, nbd = (D + kBD - 1) / kBD;
    if (b) { b->nbh = nbh; b->nbw = nbw; b->nbd = nbd; }
    return (size_t)nbh * nbw * nbd;
}

// workspace carve-up; returns the total size (base may be NULL to size only)
template <int NF, int NB = 0>
size_t rb_layout(const so_render_args &a, int chunk, char *base, RbBin *out, int *max_items) {
    RbBin b;
    const size_t nb = rb_bricks(a, &b);
    b.chunk = chunk;
    b.dbg = 0;
    const size_t total = (size_t)a.n_rays * a.n_samples;
    const size_t mi = (total + chunk - 1) / chunk + nb;
    size_t off = 0;
    b.counts = (int *)(base + off); off += nb * kShards * 4;
    b.invs_part = (float *)(base + off); off += kInvsSlots * 4;
    b.n_items = (int *)(base + off); off += 4;       // [0, here) is cleared per call (rb_zeroed_bytes)
    off = rb_align(off);
    b.cursor = (int *)(base + off); off = rb_align(off + nb * kShards * 4);
    b.blk_tot = (int2 *)(base + off); off = rb_align(off + ((nb + 1023) / 1024) * 8);
    b.items = (int4 *)(base + off); off = rb_align(off + mi * 16);
    b.rec = (float *)(base + off); off = rb_align(off + total * RbRec<NF, NB>::RECF * 4);
    if (out) *out = b;
    if (max_items) *max_items = (int)mi;
    return off;
}

inline size_t rb_zeroed_bytes(const so_render_args &a) { return rb_bricks(a, nullptr) * kShards * 4 + kInvsSlots * 4 + 4; }

inline int rb_env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}
inline int rb_chunk() { static const int c = max(256, rb_env_int("SELFOCC_RB_CHUNK", 4096)); return c; }

inline bool rb_in_range(const so_render_args &a) {
    return a.map.h.tot_len <= 1021 && a.map.w.tot_len <= 1021 && a.map.d.tot_len <= 1021 &&
           (size_t)a.n_rays * a.n_samples < ((size_t)1 << 31);
}

template <int NF, bool BF16, bool BIN, int MK, int NB = 0, bool MASKED = false>
int launch_ray(const so_render_bwd_args &ba, const RbBin &bin, hipStream_t st) {
    const int S = ba.fwd.n_samples;
    const int m = (S + 63) / 64;
    if (m >= 3) {   // four waves per ray: M = ceil(m / 4) steps per wave
        const int blocks = ba.fwd.n_rays;
#define SO_L(MM)                                                                                                        \
    do {                                                                                                                \
        if constexpr (MASKED) hipLaunchKernelGGL((render_ns_bwd_kernel<NF, MM, 4, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin); \
        else if constexpr (NB > 0) hipLaunchKernelGGL((render_bwd_sh_kernel<NB, MM, 4, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin); \
        else hipLaunchKernelGGL((render_bwd_kernel<NF, BF16, MM, 4, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin);  \
    } while (0)
        if (m <= 4) SO_L(1);
        else SO_L(2);
#undef SO_L
    } else {
        const int blocks = (ba.fwd.n_rays + 3) / 4;
#define SO_L(MM)                                                                                                        \
    do {                                                                                                                \
        if constexpr (MASKED) hipLaunchKernelGGL((render_ns_bwd_kernel<NF, MM, 1, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin); \
        else if constexpr (NB > 0) hipLaunchKernelGGL((render_bwd_sh_kernel<NB, MM, 1, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin); \
        else hipLaunchKernelGGL((render_bwd_kernel<NF, BF16, MM, 1, BIN, MK>), dim3(blocks), dim3(256), 0, st, ba, bin);  \
    } while (0)
        if (m <= 1) SO_L(1);
        else SO_L(2);
#undef SO_L
    }
    return so_launch_status();
}

template <int NF, bool BF16, int MK, int NB = 0, bool MASKED = false>
int launch_mk(const so_render_bwd_args &ba, hipStream_t st) {
    const so_render_args &a = ba.fwd;
    const bool binned = ba.scatter_ws != nullptr && rb_in_range(a) && (ba.g_sdf_vol || ba.g_feat_vol);
    if (!binned) return launch_ray<NF, BF16, false, MK, NB, MASKED>(ba, RbBin{}, st);
    RbBin bin;
    int max_items = 0;
    const size_t need = rb_layout<NF, NB>(a, rb_chunk(), (char *)ba.scatter_ws, &bin, &max_items);
    bin.dbg = rb_env_int("SELFOCC_RB_DBG", 0);
    SO_REQUIRE(ba.scatter_ws_bytes >= need, "render_bwd: scatter_ws holds %llu bytes, selfocc_render_bwd_ws_bytes() asks for %llu",
               (unsigned long long)ba.scatter_ws_bytes, (unsigned long long)need);
    SO_REQUIRE(((uintptr_t)ba.scatter_ws & 255) == 0, "render_bwd: scatter_ws must be 256-byte aligned");
    hipError_t e = hipMemsetAsync(ba.scatter_ws, 0, rb_zeroed_bytes(a), st);
    SO_REQUIRE(e == hipSuccess, "render_bwd: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const unsigned sblocks = (unsigned)((rb_bricks(a, nullptr) + 1023) / 1024);
    hipLaunchKernelGGL((MK == SO_MAP_UPSCALE ? rb_count_up_kernel : rb_count_kernel), dim3((unsigned)((a.n_rays + kCountWaves - 1) / kCountWaves)),
                       dim3(kCountWaves * 64), 0, st, a, bin);
    hipLaunchKernelGGL(rb_scan1_kernel, dim3(sblocks), dim3(1024), 0, st, bin);
    hipLaunchKernelGGL(rb_scan2_kernel, dim3(sblocks), dim3(1024), 0, st, bin);
    if (int rc = launch_ray<NF, BF16, true, MK, NB, MASKED>(ba, bin, st)) return rc;
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const size_t lds = (size_t)kTileVox * RbRec<NF, NB>::RW * 8;
    if constexpr (NB > 0) {
        static const hipError_t attr_sh = hipFuncSetAttribute((const void *)rb_brick_sh_kernel<NB, 512>,
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)attr_sh;
        hipLaunchKernelGGL((rb_brick_sh_kernel<NB, 512>), dim3(max_items), dim3(512), lds, st, bin, ba.g_sdf_vol, ba.g_feat_vol,
                           ba.g_inv_s, H, W, D);
    } else {
        // 512 threads per item (SELFOCC_RB_THREADS chose among 256 / 512 / 1024 while the kernel was tuned: 512 won at every shape)
        static const hipError_t attr = hipFuncSetAttribute((const void *)rb_brick_kernel<NF, 512>,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)attr;
        hipLaunchKernelGGL((rb_brick_kernel<NF, 512>), dim3(max_items), dim3(512), lds, st, bin, ba.g_sdf_vol, ba.g_feat_vol,
                           ba.g_inv_s, H, W, D);
    }
    return so_launch_status();
}

// the mapping kind picks the instances ('linear_upscale' is built for the widths of the forward's upscale route)
template <int NF, bool BF16>
int launch_m(const so_render_bwd_args &ba, hipStream_t st) {
    if (ba.fwd.map.kind == SO_MAP_UPSCALE) {
        if constexpr (NF == 24 && BF16) {
            SO_REQUIRE(false, "the 'linear_upscale' mapping is built for n_rgb + n_sem = 0, 3, 8 and float32 24 (got bfloat16 24)");
        } else {
            return launch_mk<NF, BF16, SO_MAP_UPSCALE>(ba, st);
        }
    }
    return launch_mk<NF, BF16, SO_MAP_LINEAR>(ba, st);
}

template <int NF>
int launch_ns(const so_render_bwd_args &ba, hipStream_t st) {
    if (ba.fwd.map.kind == SO_MAP_UPSCALE) return launch_mk<NF, false, SO_MAP_UPSCALE, 0, true>(ba, st);
    return launch_mk<NF, false, SO_MAP_LINEAR, 0, true>(ba, st);
}

template <int NB>
int launch_sh(const so_render_bwd_args &ba, hipStream_t st) {
    if (ba.fwd.map.kind == SO_MAP_UPSCALE) return launch_mk<so_sh_stride(NB), false, SO_MAP_UPSCALE, NB>(ba, st);
    return launch_mk<so_sh_stride(NB), false, SO_MAP_LINEAR, NB>(ba, st);
}

}  // namespace

int so_validate_render(const so_render_args &a);

extern "C" size_t selfocc_render_bwd_ws_bytes(const so_render_bwd_args *args) {
    if (!args) return 0;
    const so_render_args &a = args->fwd;
    if (!rb_in_range(a) || a.n_rays <= 0 || a.n_samples <= 0) return 0;
    if (so_sh_launch(a)) {   // the 64-byte record at every degree
        if (a.n_sem != 0 || a.sh_deg < 0 || a.sh_deg > 2) return 0;
        return a.sh_deg == 0 ? rb_layout<4, 1>(a, rb_chunk(), nullptr, nullptr, nullptr)
                             : (a.sh_deg == 1 ? rb_layout<12, 4>(a, rb_chunk(), nullptr, nullptr, nullptr)
                                              : rb_layout<28, 9>(a, rb_chunk(), nullptr, nullptr, nullptr));
    }
    if (a.n_sem == 1 || a.n_sem > 21 || a.n_sem < 0) return 0;   // not built (so_validate_render)
    switch (a.n_rgb + a.n_sem == 0 ? 0 : (3 + a.n_sem + 3) & ~3) {   // the row width: 64-byte records up to 8 floats, 128-byte above
        case 0: return rb_layout<0>(a, rb_chunk(), nullptr, nullptr, nullptr);
        case 4: return rb_layout<4>(a, rb_chunk(), nullptr, nullptr, nullptr);
        case 8: return rb_layout<8>(a, rb_chunk(), nullptr, nullptr, nullptr);
        default: return rb_layout<24>(a, rb_chunk(), nullptr, nullptr, nullptr);
    }
}

extern "C" int selfocc_render_bwd(const so_render_bwd_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_render_bwd_args &ba = *args;
    const so_render_args &a = ba.fwd;
    if (so_validate_render(a)) return -1;
    SO_REQUIRE(a.n_samples <= 64 * kMaxM, "render_bwd: n_samples must be <= %d", 64 * kMaxM);
    if (a.n_rays == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int nf = a.n_rgb + a.n_sem;
    const bool bf = a.feat_dtype == SO_DTYPE_BF16;
    if (nf == 0) return launch_m<0, false>(ba, st);
    if (so_sh_launch(a)) return a.sh_deg == 0 ? launch_sh<1>(ba, st) : (a.sh_deg == 1 ? launch_sh<4>(ba, st) : launch_sh<9>(ba, st));
    if (nf == 3) {
        SO_REQUIRE(a.feat_stride == 4, "n_rgb=3, n_sem=0 requires feat_stride == 4");
        return bf ? launch_m<4, true>(ba, st) : launch_m<4, false>(ba, st);
    }
    // so_validate_render: n_sem in 2 .. 21, feat_stride = 3 + n_sem rounded up to 4, bfloat16 at 21 classes only
    if (nf == 8) return launch_m<8, false>(ba, st);            // the shipped widths: rows without a pad channel
    if (nf == 24) return bf ? launch_m<24, true>(ba, st) : launch_m<24, false>(ba, st);
    switch (a.feat_stride) {                                   // any other class count: the masked family of its row width
        case 8: return launch_ns<8>(ba, st);
        case 12: return launch_ns<12>(ba, st);
        case 16: return launch_ns<16>(ba, st);
        case 20: return launch_ns<20>(ba, st);
        default: return launch_ns<24>(ba, st);
    }
}
