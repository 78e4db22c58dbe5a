// ssc_metric.hip — the occupancy metric tail of eval_iou_kitti.py (:166-190) for gfx950, one launch per frame.
//
// Replaces, per frame: the threshold and the four crops of pred_occ, torch.flip of the label volume, the
// torch.nonzero + .tolist() of IoU._after_step (utils/metric_util.py:189-199), the 2 x 256 row loops of
// SSCMetrics.add_batch (utils/scenerf_metric.py:69-188: two boolean-mask indexings, i.e. host syncs, per row), the
// max_d / min_d .item() pair and, with --sem, cityscapes2semantickitti + MeanIoU._after_step.
//
// Shape: a streaming reduction (Guideline 12).  A grid sized from the CU count walks the volume with a grid-stride
// loop; each lane takes 4 consecutive voxels along d (16-byte loads of the f32 sdf / label, one d run shares h and w,
// so the flipped label read stays contiguous) when D % 4 == 0 and the pointers are aligned, else 1.
//   binary predicates (IoU seen, completion tp / fp / fn, semantic bins 0 and 1, the MeanIoU non-empty column, bad)
//     : __ballot + __popcll into wave-uniform counters;
//   integer sums (IoU correct / positive of a non-binary prediction): per lane int64, wave reduction at the end;
//   other class bins: u32 LDS atomics;
// then an LDS fold and ONE 64-bit global atomic per nonzero counter per block.  The counts are integers, so the
// result does not depend on the order in which blocks arrive.  d_range: per block max of (d + 1) and (D - d), folded
// with u32 atomicMax into a caller's zeroed scratch; the last block to finish (ticket) writes (min, max) and zeroes the
// scratch again, so a call is one kernel and no memset.
#include "so_device.h"

namespace {

constexpr int kThreads = 256, kMaxBins = 256, kLabelSpan = 256;

// ballot counters of one wave (index into s_cnt)
enum {
    C_SEEN, C_CTP, C_CFP, C_CFN,
    C_TP0, C_FP0, C_FN0, C_TP1, C_FP1, C_FN1,
    C_MSEEN, C_MCORR, C_MPOS, C_BAD, C_N
};

// a label as the reference's comparisons see it: integral (equal to some int32), its value, and its sign
struct Label {
    int v;
    bool integ, pos;
};

SO_DEVFN Label label_f32(float f) {
    Label l;
    l.integ = (f == rintf(f)) && fabsf(f) < 2147483648.0f;   // NaN / inf / fractional: no class
    l.v = l.integ ? (int)f : 0;
    l.pos = f > 0.0f;
    return l;
}

SO_DEVFN Label label_i64(long long x) {
    Label l;
    l.integ = x >= -2147483648LL && x <= 2147483647LL;
    l.v = l.integ ? (int)x : 0;
    l.pos = x > 0;
    return l;
}

SO_DEVFN int clamp_i32(long long x) {
    return x > 2147483647LL ? 2147483647 : (x < -2147483648LL ? (-2147483647 - 1) : (int)x);
}

template <int V>
SO_DEVFN void load_labels(const void *p, int dtype, long long i, Label *t) {
    if (dtype == SO_LBL_F32) {
        const float *q = (const float *)p + i;
        if constexpr (V == 4) {
            const float4 v = *(const float4 *)q;
            t[0] = label_f32(v.x); t[1] = label_f32(v.y); t[2] = label_f32(v.z); t[3] = label_f32(v.w);
        } else {
            t[0] = label_f32(q[0]);
        }
    } else if (dtype == SO_LBL_U8) {
        const uint8_t *q = (const uint8_t *)p + i;
        if constexpr (V == 4) {
            const uint32_t v = *(const uint32_t *)q;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = label_i64((v >> (8 * j)) & 0xffu);
        } else {
            t[0] = label_i64(q[0]);
        }
    } else if (dtype == SO_LBL_I32) {
        const int32_t *q = (const int32_t *)p + i;
        if constexpr (V == 4) {
            const int4 v = *(const int4 *)q;
            t[0] = label_i64(v.x); t[1] = label_i64(v.y); t[2] = label_i64(v.z); t[3] = label_i64(v.w);
        } else {
            t[0] = label_i64(q[0]);
        }
    } else {
        const long long *q = (const long long *)p + i;
        if constexpr (V == 4) {
            const longlong2 a = *(const longlong2 *)q, b = *(const longlong2 *)(q + 2);
            t[0] = label_i64(a.x); t[1] = label_i64(a.y); t[2] = label_i64(b.x); t[3] = label_i64(b.y);
        } else {
            t[0] = label_i64(q[0]);
        }
    }
}

template <int V>
SO_DEVFN void load_ints(const void *p, int dtype, long long i, long long *x) {
    if (dtype == SO_LBL_U8) {
        const uint8_t *q = (const uint8_t *)p + i;
        if constexpr (V == 4) {
            const uint32_t v = *(const uint32_t *)q;
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = (v >> (8 * j)) & 0xffu;
        } else {
            x[0] = q[0];
        }
    } else if (dtype == SO_LBL_I32) {
        const int32_t *q = (const int32_t *)p + i;
        if constexpr (V == 4) {
            const int4 v = *(const int4 *)q;
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = q[0];
        }
    } else {
        const long long *q = (const long long *)p + i;
        if constexpr (V == 4) {
            const longlong2 a = *(const longlong2 *)q, b = *(const longlong2 *)(q + 2);
            x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
        } else {
            x[0] = q[0];
        }
    }
}

template <int V>
SO_DEVFN void load_mask(const uint8_t *m, long long i, bool *out) {
    if (!m) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = true;
        return;
    }
    if constexpr (V == 4) {
        const uint32_t v = *(const uint32_t *)(m + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = ((v >> (8 * j)) & 0xffu) != 0;
    } else {
        out[0] = m[i] != 0;
    }
}

SO_DEVFN unsigned ballot_count(bool b) { return (unsigned)__popcll(__ballot(b)); }

SO_DEVFN long long wave_sum_i64(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

SO_DEVFN int wave_max_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

template <int V>
__global__ __launch_bounds__(kThreads) void ssc_metric_kernel(const so_ssc_metric_args a, long long n) {
    __shared__ unsigned s_sem[3 * kMaxBins];
    __shared__ unsigned s_miou[3 * (kMaxBins + 1)];
    __shared__ int s_map[kLabelSpan];
    __shared__ unsigned s_cnt[C_N];
    __shared__ unsigned long long s_sum[2];
    __shared__ unsigned s_d[2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int nc = a.semantic ? a.n_classes : 0;
    const int nm = a.miou ? a.n_miou : 0;
    for (int k = tid; k < 3 * nc; k += kThreads) s_sem[k] = 0;
    for (int k = tid; k < 3 * (nm + 1); k += kThreads) s_miou[k] = 0;
    if (a.miou)
        for (int k = tid; k < kLabelSpan; k += kThreads) {
            const int c = a.miou_map[k];
            s_map[k] = (c >= 0 && c < nm) ? c : -1;    // a bad map entry never addresses outside s_miou
        }
    if (tid < C_N) s_cnt[tid] = 0;
    if (tid < 2) {
        s_sum[tid] = 0;
        s_d[tid] = 0;
    }
    __syncthreads();

    unsigned cnt[C_N];
#pragma unroll
    for (int k = 0; k < C_N; ++k) cnt[k] = 0;
    long long corr = 0, pos = 0;
    int dmax1 = 0, dmin1 = 0;      // max of (d + 1) and of (D - d) over occupied labels; 0 = none

    const unsigned W = (unsigned)a.W, D = (unsigned)a.D;
    const long long stride = (long long)gridDim.x * kThreads * V;
    for (long long base = (long long)blockIdx.x * kThreads * V; base < n; base += stride) {
        const long long i = base + (long long)tid * V;
        const bool live = i < n;
        const long long ic = live ? i : 0;          // a safe index for the loads of a dead lane
        const unsigned hw = (unsigned)(ic / D), d0 = (unsigned)(ic - (long long)hw * D);
        const unsigned h = hw / W, w = hw - h * W;
        const long long gi = a.flip_gt ? ((long long)h * W + (W - 1 - w)) * D + d0 : ic;

        Label t[V];
        load_labels<V>(a.gt, a.gt_dtype, gi, t);
        long long pv[V];
        if (a.sdf) {
            float s[V];
            if constexpr (V == 4) {
                const float4 v = *(const float4 *)(a.sdf + ic);
                s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
            } else {
                s[0] = a.sdf[ic];
            }
            const bool hw_in = (int)h >= a.crop[0] && (int)h < a.H - a.crop[1] && (int)w >= a.crop[2] &&
                               (int)w < a.W - a.crop[3];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int d = (int)d0 + j;
                const bool in = hw_in && d >= a.crop[4] && d < a.D - a.crop[5];
                pv[j] = (in && s[j] <= a.thresh) ? 1 : 0;     // NaN <= thresh is false
            }
            if (a.occ && live) {
                if constexpr (V == 4) {
                    *(int4 *)(a.occ + ic) = make_int4((int)pv[0], (int)pv[1], (int)pv[2], (int)pv[3]);
                } else {
                    a.occ[ic] = (int)pv[0];
                }
            }
        } else {
            load_ints<V>(a.pred, a.pred_dtype, ic, pv);
        }
        bool m_iou[V], m_ne[V], m_ns[V];
        load_mask<V>(a.iou_mask, ic, m_iou);
        load_mask<V>(a.nonempty, ic, m_ne);
        load_mask<V>(a.nonsurface, ic, m_ns);
        long long sv[V];
        if (a.miou) load_ints<V>(a.sem, SO_LBL_I64, ic, sv);

#pragma unroll
        for (int j = 0; j < V; ++j) {
            const Label tj = t[j];
            const int p = clamp_i32(pv[j]);
            const bool t255 = tj.integ && tj.v == 255;
            if (a.iou) {
                const bool m = live && m_iou[j];
                const bool seen = m && !(tj.integ && (tj.v == a.iou_empty || (a.iou_ignore >= 0 && tj.v == a.iou_ignore)));
                cnt[C_SEEN] += ballot_count(seen);
                corr += seen ? pv[j] : 0;
                pos += m ? pv[j] : 0;
            }
            if (a.d_range && live && !(tj.integ && (tj.v == 0 || tj.v == 255))) {
                const int d = (int)d0 + j;
                dmax1 = max(dmax1, d + 1);
                dmin1 = max(dmin1, a.D - d);
            }
            if (a.completion || a.semantic) {
                // get_score_*: t == 255 -> (t, p) = (0, 0); add_batch masks those voxels out
                const bool sm = live && m_ne[j] && (!t255 || a.ssc_keep255);
                const bool tpos = t255 ? false : tj.pos;
                const int ps = t255 ? 0 : p;
                if (a.completion) {
                    const bool cm = sm && m_ns[j];
                    cnt[C_CTP] += ballot_count(cm && tpos && ps > 0);
                    cnt[C_CFP] += ballot_count(cm && !tpos && ps > 0);
                    cnt[C_CFN] += ballot_count(cm && tpos && !(ps > 0));
                }
                if (a.semantic) {
                    const bool ti = t255 || tj.integ;
                    const int tv = t255 ? 0 : tj.v;
                    const int tc = (ti && tv >= 0 && tv < nc) ? tv : -1;
                    const int pc = (ps >= 0 && ps < nc) ? ps : -1;
                    const bool eq = ti && tv == ps;
                    const int b_tp = (sm && eq) ? tc : -1;
                    const int b_fp = (sm && !eq) ? pc : -1;
                    const int b_fn = (sm && !eq) ? tc : -1;
                    cnt[C_TP0] += ballot_count(b_tp == 0);
                    cnt[C_FP0] += ballot_count(b_fp == 0);
                    cnt[C_FN0] += ballot_count(b_fn == 0);
                    cnt[C_TP1] += ballot_count(b_tp == 1);
                    cnt[C_FP1] += ballot_count(b_fp == 1);
                    cnt[C_FN1] += ballot_count(b_fn == 1);
                    if (b_tp >= 2) atomicAdd(&s_sem[b_tp], 1u);
                    if (b_fp >= 2) atomicAdd(&s_sem[nc + b_fp], 1u);
                    if (b_fn >= 2) atomicAdd(&s_sem[2 * nc + b_fn], 1u);
                }
            }
            if (a.miou) {
                const bool mm = live && !t255;
                long long s = sv[j];
                const bool sok = s >= -(long long)a.n_lut && s < (long long)a.n_lut;
                if (s < 0) s += a.n_lut;
                const int pm = sok ? p * a.lut[s] : 0;
                cnt[C_BAD] += ballot_count(live && !sok);
                const int tk = (tj.integ && tj.v >= 0 && tj.v < kLabelSpan) ? s_map[tj.v] : -1;
                const int pk = (pm >= 0 && pm < kLabelSpan) ? s_map[pm] : -1;
                if (mm && tk >= 0) atomicAdd(&s_miou[tk], 1u);
                if (mm && tk >= 0 && tk == pk) atomicAdd(&s_miou[(nm + 1) + tk], 1u);
                if (mm && pk >= 0) atomicAdd(&s_miou[2 * (nm + 1) + pk], 1u);
                const bool te = !(tj.integ && tj.v == a.miou_empty), pe = pm != a.miou_empty;
                cnt[C_MSEEN] += ballot_count(mm && te);
                cnt[C_MCORR] += ballot_count(mm && te && pe);
                cnt[C_MPOS] += ballot_count(mm && pe);
            }
        }
    }

    // fold: wave -> LDS -> one global atomic per counter per block
    if (a.iou) {
        corr = wave_sum_i64(corr);
        pos = wave_sum_i64(pos);
    }
    if (a.d_range) {
        dmax1 = wave_max_i32(dmax1);
        dmin1 = wave_max_i32(dmin1);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < C_N; ++k)
            if (cnt[k]) atomicAdd(&s_cnt[k], cnt[k]);
        if (corr) atomicAdd(&s_sum[0], (unsigned long long)corr);
        if (pos) atomicAdd(&s_sum[1], (unsigned long long)pos);
        if (dmax1) {
            atomicMax(&s_d[0], (unsigned)dmax1);
            atomicMax(&s_d[1], (unsigned)dmin1);
        }
    }
    __syncthreads();
    for (int k = tid; k < 3 * nc; k += kThreads) {
        const int r = k / nc, c = k - r * nc;
        unsigned v = s_sem[k];
        if (c < 2) v += s_cnt[C_TP0 + 3 * c + r];
        if (v) atomicAdd(&a.semantic[k], (unsigned long long)v);
    }
    for (int k = tid; k < 3 * (nm + 1); k += kThreads) {
        const int r = k / (nm + 1), c = k - r * (nm + 1);
        unsigned v = s_miou[k];
        if (c == nm) v += s_cnt[C_MSEEN + r];
        if (v) atomicAdd(&a.miou[k], (unsigned long long)v);
    }
    if (tid == 0) {
        if (a.iou) {
            if (s_cnt[C_SEEN]) atomicAdd(&a.iou[0], (unsigned long long)s_cnt[C_SEEN]);
            if (s_sum[0]) atomicAdd(&a.iou[1], s_sum[0]);
            if (s_sum[1]) atomicAdd(&a.iou[2], s_sum[1]);
        }
        if (a.completion)
            for (int r = 0; r < 3; ++r)
                if (s_cnt[C_CTP + r]) atomicAdd(&a.completion[r], (unsigned long long)s_cnt[C_CTP + r]);
        if (a.bad && s_cnt[C_BAD]) atomicAdd(a.bad, (unsigned long long)s_cnt[C_BAD]);
        if (a.d_range) {
            if (s_d[0]) {
                atomicMax(&a.ws[0], s_d[0]);
                atomicMax(&a.ws[1], s_d[1]);
            }
            __threadfence();
            const unsigned ticket = atomicAdd(&a.ws[2], 1u);
            if (ticket == gridDim.x - 1) {          // every other block has folded its range
                __threadfence();
                const unsigned mx = atomicExch(&a.ws[0], 0u), mn = atomicExch(&a.ws[1], 0u);
                atomicExch(&a.ws[2], 0u);
                a.d_range[0] = mx ? a.D - (int)mn : -1;
                a.d_range[1] = mx ? (int)mx - 1 : -1;
            }
        }
    }
}

// IoU coordinate form: positive = sum of pred (grid-stride over the volume), correct = sum of pred at the rows
// (grid-stride over the rows), seen += n_coords; rows out of range -> bad
__global__ __launch_bounds__(kThreads) void iou_coords_kernel(const so_ssc_metric_args a, long long n) {
    __shared__ unsigned long long s_sum[3];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 3) s_sum[tid] = 0;
    __syncthreads();
    long long pos = 0, corr = 0, bad = 0;
    const long long step = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + tid; i < n; i += step) {
        long long v;
        load_ints<1>(a.pred, a.pred_dtype, i, &v);
        pos += v;
    }
    const long long dims[3] = {a.H, a.W, a.D};
    for (long long r = (long long)blockIdx.x * kThreads + tid; r < a.n_coords; r += step) {
        long long c[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = a.coords[3 * r + k];
            ok = ok && c[k] >= -dims[k] && c[k] < dims[k];
            c[k] += c[k] < 0 ? dims[k] : 0;
        }
        if (ok) {
            long long v;
            load_ints<1>(a.pred, a.pred_dtype, (c[0] * dims[1] + c[1]) * dims[2] + c[2], &v);
            corr += v;
        } else {
            ++bad;
        }
    }
    pos = wave_sum_i64(pos);
    corr = wave_sum_i64(corr);
    bad = wave_sum_i64(bad);
    if (lane == 0) {
        if (corr) atomicAdd(&s_sum[0], (unsigned long long)corr);
        if (pos) atomicAdd(&s_sum[1], (unsigned long long)pos);
        if (bad) atomicAdd(&s_sum[2], (unsigned long long)bad);
    }
    __syncthreads();
    if (tid == 0) {
        if (blockIdx.x == 0 && a.n_coords) atomicAdd(&a.iou[0], (unsigned long long)a.n_coords);
        if (s_sum[0]) atomicAdd(&a.iou[1], s_sum[0]);
        if (s_sum[1]) atomicAdd(&a.iou[2], s_sum[1]);
        if (s_sum[2]) atomicAdd(a.bad, s_sum[2]);
    }
}

int cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached[dev] = cus;
    }
    return cached[dev];
}

bool aligned(const void *p, size_t b) { return ((uintptr_t)p % b) == 0; }

bool lbl_dtype_ok(int d, bool f32_ok) { return (d == SO_LBL_F32 && f32_ok) || d == SO_LBL_U8 || d == SO_LBL_I32 || d == SO_LBL_I64; }

size_t lbl_size(int d) { return d == SO_LBL_U8 ? 1 : (d == SO_LBL_I64 ? 8 : 4); }

}  // namespace

extern "C" int selfocc_ssc_metric(const so_ssc_metric_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_ssc_metric_args &a = *args;
    SO_REQUIRE(a.H >= 1 && a.W >= 1 && a.D >= 1, "ssc_metric: bad volume %d x %d x %d", a.H, a.W, a.D);
    const long long n = (long long)a.H * a.W * a.D;
    SO_REQUIRE(n < (1LL << 31), "ssc_metric: n = %lld >= 2^31 voxels", n);
    SO_REQUIRE(a.gt != nullptr, "ssc_metric: gt is NULL");
    SO_REQUIRE(lbl_dtype_ok(a.gt_dtype, true), "ssc_metric: bad gt_dtype %d", a.gt_dtype);
    SO_REQUIRE((a.pred == nullptr) != (a.sdf == nullptr), "ssc_metric: exactly one of pred / sdf");
    SO_REQUIRE(a.sdf || lbl_dtype_ok(a.pred_dtype, false), "ssc_metric: bad pred_dtype %d", a.pred_dtype);
    SO_REQUIRE(a.flip_gt == 0 || a.flip_gt == 1, "ssc_metric: flip_gt must be 0 / 1");
    SO_REQUIRE(a.ssc_keep255 == 0 || a.ssc_keep255 == 1, "ssc_metric: ssc_keep255 must be 0 / 1");
    for (int k = 0; k < 6; ++k) SO_REQUIRE(a.crop[k] >= 0, "ssc_metric: negative crop");
    SO_REQUIRE(a.iou || a.completion || a.semantic || a.miou || a.d_range || a.occ, "ssc_metric: no output requested");
    SO_REQUIRE(!a.semantic || (a.n_classes >= 1 && a.n_classes <= kMaxBins),
               "ssc_metric: n_classes = %d outside [1, %d]", a.n_classes, kMaxBins);
    SO_REQUIRE(!a.miou || (a.sem && a.lut && a.miou_map && a.n_lut >= 1 && a.n_miou >= 0 && a.n_miou <= kMaxBins),
               "ssc_metric: miou needs sem, lut (n_lut >= 1), miou_map and 0 <= n_miou <= %d", kMaxBins);
    SO_REQUIRE(!a.d_range || a.ws, "ssc_metric: d_range needs ws");
    SO_REQUIRE(!a.occ || a.sdf, "ssc_metric: occ needs the sdf form");
    const void *p32[] = {a.sdf, a.occ};
    bool vec = a.D % 4 == 0 && aligned(a.gt, 4 * lbl_size(a.gt_dtype)) && aligned(a.sem, 16) &&
               aligned(a.nonempty, 4) && aligned(a.nonsurface, 4) && aligned(a.iou_mask, 4) &&
               aligned(p32[0], 16) && aligned(p32[1], 16) && (a.sdf || aligned(a.pred, 4 * lbl_size(a.pred_dtype)));
    const int V = vec ? 4 : 1;
    long long blocks = (n + (long long)kThreads * V - 1) / ((long long)kThreads * V);
    const long long cap = 4LL * cu_count();
    if (blocks > cap) blocks = cap;
    if (vec)
        hipLaunchKernelGGL(ssc_metric_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a, n);
    else
        hipLaunchKernelGGL(ssc_metric_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a, n);
    return so_launch_status();
}

extern "C" int selfocc_iou_coords(const so_ssc_metric_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    const so_ssc_metric_args &a = *args;
    SO_REQUIRE(a.H >= 1 && a.W >= 1 && a.D >= 1, "iou_coords: bad volume %d x %d x %d", a.H, a.W, a.D);
    const long long n = (long long)a.H * a.W * a.D;
    SO_REQUIRE(n < (1LL << 31), "iou_coords: n = %lld >= 2^31 voxels", n);
    SO_REQUIRE(a.n_coords >= 0 && a.n_coords < (1LL << 31), "iou_coords: bad n_coords %lld", (long long)a.n_coords);
    SO_REQUIRE(a.pred != nullptr && lbl_dtype_ok(a.pred_dtype, false), "iou_coords: pred is NULL or bad pred_dtype");
    SO_REQUIRE(a.coords != nullptr || a.n_coords == 0, "iou_coords: coords is NULL");
    SO_REQUIRE(a.iou != nullptr && a.bad != nullptr, "iou_coords: iou / bad is NULL");
    const long long work = n > a.n_coords ? n : a.n_coords;
    long long blocks = (work + kThreads - 1) / kThreads;
    const long long cap = 4LL * cu_count();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(iou_coords_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, a, n);
    return so_launch_status();
}
