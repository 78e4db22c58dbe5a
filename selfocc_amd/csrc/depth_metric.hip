// depth_metric.hip — the depth-evaluation metric tail for gfx950, one launch per frame.
//
// Replaces DepthMetric._after_step (utils/metric_util.py:282-349, with cal_depth_metric :247-280) and the
// per-camera evaluate_depth -> compute_depth_errors_torch loop of the novel-depth scripts (metric_util.py:424-444,
// eval_novel_depth.py:176-196).  The reference runs one F.grid_sample, then per camera two boolean-mask indexings
// (a nonzero() host sync each), two torch.median and ~20 small ops per eval type: ~250 launches, 12 syncs per frame.
//
// Shape: ONE workgroup of 1024 threads per camera (6 workgroups at nuscenes size).  The frame is small (6 x 34 720
// points), so the launch is latency-bound, not bandwidth-bound: a block per camera keeps every phase inside one
// workgroup (barriers, no second launch, no inter-block protocol) and uses 16 waves to overlap the gather's loads.
//   1. gather  : bilinear sample of pred at every location (torch's GPU grid_sampler_2d arithmetic, restated below),
//                optional store of the sampled depth; masked (gt, pred) pairs compacted IN ORDER into the workspace
//                (block-wide ballot scan, so every later pass is deterministic);
//   2. median  : radix select (4 passes of 8 bits) on order-preserving u32 keys of the compacted gt and pred,
//                histograms in LDS, the data re-read from L2; no sort;
//   3. metrics : per eval type, the f32 elementwise terms of cal_depth_metric summed in f64 (thread-strided, then a
//                fixed-order block reduction), finalised by thread 0 into the accumulators / the (N, 7) rows.
#include <math.h>
#include "so_device.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kUnroll = 4;
constexpr int kStats = 7;     // abs_rel, sq_rel, sq, log_sq sums; a1, a2, a3 counts

// torch's grid_sampler_2d_kernel<float> (aten/src/ATen/native/cuda/GridSampler.cu{h}), bilinear, border,
// align_corners = True, at the grid value g = loc * 2 - 1 that the reference builds with two elementwise ops:
//   unnormalise ((g + 1) / 2) * (size - 1); clip to [0, size - 1] (max, then min); corner weights from the
//   integer corners converted back to float; out = 0, then += value * weight for the in-bounds corners nw, ne,
//   sw, se in that order.  The ROCm build contracts `out += v * w` into a fused multiply-add (v_fma_f32 from 0,
//   then v_fmac_f32: read from its gfx950 code object), so it is spelled fmaf() here (this file is built with
//   -ffp-contract=off).  After the border clip the coordinate is finite, so torch's safe_downgrade_to_int_range
//   never fires.
SO_DEVFN float grid_sample_border(const float *__restrict__ img, int h, int w, float u, float v) {
    const float gx = (u * 2.0f) - 1.0f, gy = (v * 2.0f) - 1.0f;
    float x = ((gx + 1.0f) / 2.0f) * (float)(w - 1);
    float y = ((gy + 1.0f) / 2.0f) * (float)(h - 1);
    x = fminf((float)(w - 1), fmaxf(x, 0.0f));
    y = fminf((float)(h - 1), fmaxf(y, 0.0f));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float nw = ((float)x1 - x) * ((float)y1 - y);
    const float ne = (x - (float)x0) * ((float)y1 - y);
    const float sw = ((float)x1 - x) * (y - (float)y0);
    const float se = (x - (float)x0) * (y - (float)y0);
    const bool xin0 = x0 >= 0 && x0 < w, xin1 = x1 >= 0 && x1 < w;
    const bool yin0 = y0 >= 0 && y0 < h, yin1 = y1 >= 0 && y1 < h;
    float out = 0.0f;
    if (yin0 && xin0) out = fmaf(img[(size_t)y0 * w + x0], nw, out);
    if (yin0 && xin1) out = fmaf(img[(size_t)y0 * w + x1], ne, out);
    if (yin1 && xin0) out = fmaf(img[(size_t)y1 * w + x0], sw, out);
    if (yin1 && xin1) out = fmaf(img[(size_t)y1 * w + x1], se, out);
    return out;
}

// order-preserving u32 key of a float (negative values: all bits flipped; positive: sign bit set)
SO_DEVFN uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SO_DEVFN float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Stable block-wide compaction slot of `flag`: the rank of this thread among the flagged threads of the block,
// offset by `base` (uniform; advanced by the block's total).  -1 for an unflagged thread.
SO_DEVFN int block_slot(bool flag, int *s_wave, int &base) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(b);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const int c = s_wave[k];
        off += (k < wv) ? c : 0;
        tot += c;
    }
    __syncthreads();      // s_wave is rewritten by the next call
    base += tot;
    return flag ? off + before : -1;
}

SO_DEVFN double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the f32 elementwise terms of cal_depth_metric / compute_depth_errors_torch for one point, added to s[0..6]
SO_DEVFN void add_terms(float gt, float p, double *s) {
    p = (p < 1e-3f) ? 1e-3f : p;          // torch.clamp(p, 1e-3, 80) (NaN passes through)
    p = (p > 80.0f) ? 80.0f : p;
    const float thresh = fmaxf(gt / p, p / gt);
    const float d = gt - p;
    const float dl = logf(gt) - logf(p);
    s[0] += (double)(fabsf(d) / gt);
    s[1] += (double)((d * d) / gt);
    s[2] += (double)(d * d);
    s[3] += (double)(dl * dl);
    s[4] += (thresh < 1.25f) ? 1.0 : 0.0;
    s[5] += (thresh < 1.5625f) ? 1.0 : 0.0;       // 1.25 ** 2, exact in f32
    s[6] += (thresh < 1.953125f) ? 1.0 : 0.0;     // 1.25 ** 3, exact in f32
}

// stats -> (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3); the reference's f32 means of 0 / 1 values are count / m
SO_DEVFN void finalise(const double *s, int m, float *o) {
    if (m == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) o[k] = __builtin_nanf("");
        return;
    }
    const double dm = (double)m;
    o[0] = (float)(s[0] / dm);
    o[1] = (float)(s[1] / dm);
    o[2] = (float)sqrt(s[2] / dm);
    o[3] = (float)sqrt(s[3] / dm);
    o[4] = (float)s[4] / (float)m;
    o[5] = (float)s[5] / (float)m;
    o[6] = (float)s[6] / (float)m;
}

// one (type, camera) entry of the accumulators += this frame's values (the reference's `self.abs_rel[t, cam] += ...`)
SO_DEVFN void add_row(const so_depth_metric_args &a, size_t o, const float *v, float scaling) {
    a.abs_rel[o] += v[0];
    a.sq_rel[o] += v[1];
    a.rmse[o] += v[2];
    a.rmse_log[o] += v[3];
    a.a1[o] += v[4];
    a.a2[o] += v[5];
    a.a3[o] += v[6];
    a.scaling[o] += scaling;
}

__global__ __launch_bounds__(kThreads) void depth_metric_kernel(so_depth_metric_args a) {
    __shared__ int s_wave[kWaves];
    __shared__ uint32_t s_hist[2][256];
    __shared__ uint32_t s_prefix[2], s_rank[2];
    __shared__ double s_red[kWaves][2 * kStats];
    __shared__ double s_tot[2 * kStats];

    const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = a.n;
    const float *__restrict__ img = a.pred + (size_t)cam * a.h * a.w;
    const float2 *__restrict__ loc = reinterpret_cast<const float2 *>(a.loc) + (size_t)cam * n;
    const bool metrics = a.gt != nullptr;
    float *cg = nullptr, *cp = nullptr;
    if (metrics) {
        cg = reinterpret_cast<float *>(a.ws) + (size_t)cam * 2 * n;
        cp = cg + n;
    }

    // ---- 1. gather + ordered compaction of the masked points ----
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += kThreads * kUnroll) {
        float2 l[kUnroll];
        float g[kUnroll], p[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = i0 + u * kThreads + tid;
            const bool live = i < n;
            l[u] = live ? loc[i] : make_float2(0.0f, 0.0f);
            g[u] = (live && metrics) ? a.gt[(size_t)cam * n + i] : 0.0f;
            ok[u] = live && metrics && a.mask[(size_t)cam * n + i] != 0;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) p[u] = grid_sample_border(img, a.h, a.w, l[u].x, l[u].y);
        if (a.sampled) {
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int i = i0 + u * kThreads + tid;
                if (i < n) a.sampled[(size_t)cam * n + i] = p[u];
            }
        }
        if (metrics) {
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int j = block_slot(ok[u], s_wave, m);
                if (j >= 0) {
                    cg[j] = g[u];
                    cp[j] = p[u];
                }
            }
        }
    }
    if (!metrics) return;
    __syncthreads();      // the compacted arrays (global, this block's own writes) are read by every thread below

    // ---- 2. lower medians (element (m - 1) / 2) of the compacted gt and pred: radix select ----
    const bool want_raw = a.raw_row >= 0 || a.errors != nullptr;
    const bool want_med = a.median_row >= 0 || a.medians != nullptr;
    float med_gt = __builtin_nanf(""), med_p = __builtin_nanf("");
    if (want_med && m > 0) {
        if (tid < 2) {
            s_prefix[tid] = 0u;
            s_rank[tid] = (uint32_t)((m - 1) / 2);
        }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t hmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            if (tid < 512) (&s_hist[0][0])[tid] = 0u;
            __syncthreads();
            const uint32_t pg = s_prefix[0], pp = s_prefix[1];
            for (int j = tid; j < m; j += kThreads) {
                const uint32_t kg = f2key(cg[j]), kp = f2key(cp[j]);
                if ((kg & hmask) == pg) atomicAdd(&s_hist[0][(kg >> shift) & 255u], 1u);
                if ((kp & hmask) == pp) atomicAdd(&s_hist[1][(kp >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wv < 2) {     // wave 0: gt, wave 1: pred; lane owns bins 4 lane .. 4 lane + 3
                uint32_t c[4], sum = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    c[q] = s_hist[wv][4 * lane + q];
                    sum += c[q];
                }
                uint32_t incl = sum;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t t = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += t;
                }
                const uint32_t k = s_rank[wv];
                uint32_t cum = incl - sum;
                if (cum <= k && k < incl) {      // exactly one lane holds rank k
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (k < cum + c[q]) {
                            s_prefix[wv] = s_prefix[wv] | ((uint32_t)(4 * lane + q) << shift);
                            s_rank[wv] = k - cum;
                            break;
                        }
                        cum += c[q];
                    }
                }
            }
            __syncthreads();
        }
        med_gt = key2f(s_prefix[0]);
        med_p = key2f(s_prefix[1]);
    }
    const float scale = med_gt / med_p;      // metric_util.py:328-330, f32 as the reference

    // ---- 3. metric sums: [0, kStats) raw, [kStats, 2 kStats) median ----
    double s[2 * kStats];
#pragma unroll
    for (int k = 0; k < 2 * kStats; ++k) s[k] = 0.0;
    for (int j = tid; j < m; j += kThreads) {
        const float g = cg[j], p = cp[j];
        if (want_raw) add_terms(g, p, s);
        if (want_med) add_terms(g, scale * p, s + kStats);
    }
#pragma unroll
    for (int k = 0; k < 2 * kStats; ++k) {
        const double v = wave_sum(s[k]);
        if (lane == 0) s_red[wv][k] = v;
    }
    __syncthreads();
    if (tid < 2 * kStats) {      // fixed order over the waves
        double v = 0.0;
        for (int q = 0; q < kWaves; ++q) v += s_red[q][tid];
        s_tot[tid] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    float raw[7], med[7];
    finalise(s_tot, m, raw);
    finalise(s_tot + kStats, m, med);
    const int N = a.N;
    if (a.errors) {
#pragma unroll
        for (int k = 0; k < 7; ++k) a.errors[(size_t)cam * 7 + k] = raw[k];
    }
    if (a.medians) {
        a.medians[2 * cam] = med_gt;
        a.medians[2 * cam + 1] = med_p;
    }
    if (a.count) {        // accumulators (all or none: host)
        if (a.raw_row >= 0) add_row(a, (size_t)a.raw_row * N + cam, raw, 1.0f);
        if (a.median_row >= 0) add_row(a, (size_t)a.median_row * N + cam, med, scale);
        if (cam == 0) a.count[0] += 1.0f;
    }
}

}  // namespace

extern "C" size_t selfocc_depth_metric_ws_bytes(const so_depth_metric_args *args) {
    if (!args || args->N <= 0 || args->n <= 0 || !args->gt) return 0;
    return (((size_t)args->N * args->n * 2 * sizeof(float)) + 255) & ~(size_t)255;
}

extern "C" int selfocc_depth_metric(const so_depth_metric_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_depth_metric_args &a = *args;
    SO_REQUIRE(a.N > 0 && a.h > 0 && a.w > 0 && a.n >= 0, "depth_metric: bad shape N=%d h=%d w=%d n=%d", a.N, a.h,
               a.w, a.n);
    SO_REQUIRE(a.n < (1 << 24), "depth_metric: n = %d points per camera, limit 2^24 (counts exact in f32)", a.n);
    SO_REQUIRE((long long)a.h * a.w < (1LL << 31), "depth_metric: image of %d x %d too large", a.h, a.w);
    SO_REQUIRE(a.pred && a.loc, "depth_metric: pred / loc is NULL");
    SO_REQUIRE(((uintptr_t)a.loc & 7u) == 0, "depth_metric: loc must be 8-byte aligned (float2 rows)");
    const bool acc = a.abs_rel || a.sq_rel || a.rmse || a.rmse_log || a.a1 || a.a2 || a.a3 || a.scaling || a.count;
    if (acc) {
        SO_REQUIRE(a.abs_rel && a.sq_rel && a.rmse && a.rmse_log && a.a1 && a.a2 && a.a3 && a.scaling && a.count,
                   "depth_metric: the accumulators go together (abs_rel .. a3, scaling, count)");
        SO_REQUIRE(a.n_types >= 1 && a.raw_row >= -1 && a.raw_row < a.n_types && a.median_row >= -1 &&
                       a.median_row < a.n_types && (a.raw_row != a.median_row || a.raw_row < 0),
                   "depth_metric: bad rows raw=%d median=%d of n_types=%d", a.raw_row, a.median_row, a.n_types);
    }
    const bool metrics = acc || a.errors || a.medians;
    SO_REQUIRE(metrics || a.sampled, "depth_metric: no output requested");
    SO_REQUIRE(!metrics || (a.gt && a.mask), "depth_metric: metrics need gt and mask");
    SO_REQUIRE(metrics || (!a.gt && !a.mask), "depth_metric: gt / mask given but no metric output requested");
    if (metrics) {
        const size_t need = selfocc_depth_metric_ws_bytes(&a);
        SO_REQUIRE(need == 0 || (a.ws && a.ws_bytes >= need), "depth_metric: workspace of %llu bytes < %llu needed",
                   (unsigned long long)a.ws_bytes, (unsigned long long)need);
    }
    hipLaunchKernelGGL(depth_metric_kernel, dim3((unsigned)a.N), dim3(kThreads), 0, (hipStream_t)stream, a);
    return so_launch_status();
}
