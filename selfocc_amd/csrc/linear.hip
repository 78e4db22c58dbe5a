// linear.hip — weight and bias gradient of the encoder's tall-skinny projections in ONE pass over dY and X:
//     dW[n][k] = sum_r dY[r][n] X[r][k]        db[n] = sum_r dY[r][n]
// (the Linear layers of TPVFormerLayer / BEVFormerLayer and their attention modules: sampling_offsets,
// attention_weights, value_proj, output_proj, FFN — mmcv Linear under torch autograd in the reference,
// model/encoder/tpvformer/attention/image_cross_attention.py:130-160, cross_view_hybrid_attention.py:35-60).
//
// Shapes: r runs over 66 k - 180 k rows, K = 96 (192) input features, N = 96 .. 2304 outputs.  The vendor GEMM for
// dY^T X with that reduction length runs on a handful of workgroups; round 1 split it into <= 256 batched GEMMs
// + a sum, and took the bias gradient with torch's column reduction: dY is read twice, 56 + 20 + ~10 us per layer
// call, 36 calls per training iteration.  Here the reduction over rows is the K dimension of
// v_mfma_f32_32x32x2_f32 and BOTH operands load from global memory straight in MFMA layout:
//     A[m = n][kk = row pair]: lane (i, half) <- dY[r + half][n0 + i]     (32 consecutive floats of one row)
//     B[kk = row pair][col = k]: lane (i, half) <- X[r + half][k0 + i]
// no LDS, no transposes; the bias gradient is the running sum of the A operand.  A wave keeps NTW x KT 32 x 32
// accumulator tiles (<= 12: 192 registers) for its quarter of the block's rows; the four waves of a block are
// summed through one LDS tile at the end, and the per-block partials by a second tiny kernel in a fixed order
// (deterministic).  f32 MFMA on gfx950 is an exact fmaf chain (no TF32): float32 arithmetic.
//
// Measured (66 049 x 384 x 96, scripts/micro/wgrad_bench.py): 65 us = 70 TFLOP/s, 1.9 TB/s.  Built without the MFMAs
// it takes 35 us (3.6 TB/s), with the loads hoisted out of the loop 45 us (the 1.2 M MFMAs at 64 clk on 1 024 SIMDs
// are 31 us): at 2 waves per SIMD (144 accumulator + 48 prefetch registers) the two overlap only partly.  Tried without
// gain: branch-free clamped loads + ping-pong register buffers + sched_barrier so that the compiler emits counted
// vmcnt waits (74 us: 64-bit address math per load, spills), an XCD-aware block order that lets the n-groups of a row
// chunk share x in one L2 (70 -> 70 us; 96 -> 138 us for N = 432); and (end of round 2) the LDS-staged form — a block
// stages 32 rows of dY / X with coalesced float4 loads (next stage in registers, one barrier per stage) and its four
// waves split the 96 x K output 2 x 2 on v_mfma_f32_16x16x4_f32 (36 accumulator registers, ds_read_b32 operands): correct,
// but 83 / 113 / 202 us where this kernel takes 70 / 95 / 153 us (a barrier per 72 MFMAs per wave and one LDS read per
// operand cost more than the overlap buys) — dropped.
#include "so_device.h"
#include <algorithm>
#include <cstdlib>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Row groups (selfocc_linear_wgrad_grouped): the units of the table (so_device.h) are the chunks, which walk their group's rows
// in steps of rows_per_block — a chunk never straddles a group.
template <bool GRP>
SO_DEVFN void so_wgrad_chunk(const so_group_table &gr, int chunk, long long rows_per_block, long long T, long long &r_blk, long long &r_end) {
    r_blk = (long long)chunk * rows_per_block;
    r_end = T;
    if constexpr (GRP) {
        const auto p = so_group_of(gr, chunk);
        r_blk = p.row_lo + (long long)p.unit * rows_per_block;
        r_end = p.row_hi;
    }
}

constexpr int kRowPairsAhead = 4;      // row pairs loaded per step (all loads of a step are in flight together)

template <int KT, int NTW, bool GRP = false>
__global__ __launch_bounds__(256, 2) void linear_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                              float *__restrict__ part_w /* [chunks][N][K] */,
                                                              float *__restrict__ part_b /* [chunks][N] */,
                                                              long long T, int N, int K, long long rows_per_block, so_group_table gr) {
    constexpr int U = (NTW * KT > 9) ? kRowPairsAhead / 2 : kRowPairsAhead;   // 12 tiles: 192 accumulator registers
    __shared__ float red[NTW * KT * 1024];
    __shared__ float red_b[4][NTW * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, half = lane >> 5;
    const int chunk = blockIdx.x;
    const int n0 = blockIdx.y * (NTW * 32);
    long long r_blk, r_end;
    so_wgrad_chunk<GRP>(gr, chunk, rows_per_block, T, r_blk, r_end);
    const long long rpw = rows_per_block / 4;                         // rows per wave (host: a multiple of 2)
    const long long r0 = r_blk + wave * rpw, r1 = min(r_end, r0 + rpw);

    f32x16 acc[NTW][KT];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][u][v] = 0.0f;
    float bsum[NTW];
    bool ncol[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) { bsum[t] = 0.0f; ncol[t] = n0 + t * 32 + i < N; }

    auto load = [&](long long r, float (&a)[NTW], float (&b)[KT]) {
        const long long rr = r + half;
        const bool ok = rr < r1;
        const float *dyr = dy + rr * N + n0 + i;
        const float *xr = x + rr * K + i;
#pragma unroll
        for (int t = 0; t < NTW; ++t) a[t] = (ok && ncol[t]) ? dyr[t * 32] : 0.0f;
#pragma unroll
        for (int u = 0; u < KT; ++u) b[u] = ok ? xr[u * 32] : 0.0f;
    };
    float a_cur[U][NTW], b_cur[U][KT], a_nxt[U][NTW], b_nxt[U][KT];
#pragma unroll
    for (int s = 0; s < U; ++s) load(r0 + 2 * s, a_cur[s], b_cur[s]);
    for (long long r = r0; r < r1; r += 2 * U) {
#pragma unroll
        for (int s = 0; s < U; ++s) load(r + 2 * (U + s), a_nxt[s], b_nxt[s]);
#pragma unroll
        for (int s = 0; s < U; ++s) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                bsum[t] += a_cur[s][t];
#pragma unroll
                for (int u = 0; u < KT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[s][t], b_cur[s][u], acc[t][u], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < U; ++s) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) a_cur[s][t] = a_nxt[s][t];
#pragma unroll
            for (int u = 0; u < KT; ++u) b_cur[s][u] = b_nxt[s][u];
        }
    }

    // block reduction: waves 1..3 hand their tiles to wave 0 through one LDS tile set, one after the other
#pragma unroll
    for (int t = 0; t < NTW; ++t) bsum[t] += __shfl_xor(bsum[t], 32, 64);
    if (half == 0) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) red_b[wave][t * 32 + i] = bsum[t];
    }
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int u = 0; u < KT; ++u)
#pragma unroll
                    for (int v = 0; v < 16; ++v) red[((t * KT + u) * 16 + v) * 64 + lane] = acc[t][u][v];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int u = 0; u < KT; ++u)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[t][u][v] += red[((t * KT + u) * 16 + v) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    // C layout: col = lane & 31 (k), row = (v & 3) + 8 (v >> 2) + 4 half (n)
    float *pw = part_w + (size_t)chunk * N * K;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = n0 + t * 32 + (v & 3) + 8 * (v >> 2) + 4 * half;
            if (n >= N) continue;
#pragma unroll
            for (int u = 0; u < KT; ++u) pw[(size_t)n * K + u * 32 + i] = acc[t][u][v];
        }
        if (half == 0 && ncol[t])
            part_b[(size_t)chunk * N + n0 + t * 32 + i] =
                (red_b[0][t * 32 + i] + red_b[1][t * 32 + i]) + (red_b[2][t * 32 + i] + red_b[3][t * 32 + i]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same reduction on the bf16 matrix pipe with the exact three-way split of linear_fwd.hip (round 3): every loaded
// float32 of dY and X becomes three bfloat16 (x = x1 + x2 + x3 exactly), six v_mfma_f32_32x32x16_bf16 (the products with
// i + j <= 4, small terms first) replace eight v_mfma_f32_32x32x2_f32 per 16 rows — 2.67 x fewer matrix-pipe cycles at
// float32-level accuracy.  Operand layout of the 16-row step (reduction index = row):
//     A[m = n][k = row]: lane (i, kb) <- dY[r + 8 kb + j][n0 + 32 t + i], j < 8     (per j: 32 consecutive floats of a row)
//     B[k = row][col]:   lane (i, kb) <- X[r + 8 kb + j][32 u + i]
// X's parts are split once per step and shared by the NTW tile rows; dY's parts per tile row.  The bias gradient is the
// float32 running sum of the raw A operand, as before.  Accumulator layout and everything after the loop are the f32
// kernel's.
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));

SO_DEVFN void so_wsplit3(const float (&x)[8], bf16x8w &a1, bf16x8w &a2, bf16x8w &a3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 b1 = (__bf16)x[j];
        const float r1 = x[j] - (float)b1;
        const __bf16 b2 = (__bf16)r1;
        const float r2 = r1 - (float)b2;
        a1[j] = b1; a2[j] = b2; a3[j] = (__bf16)r2;
    }
}

// P = planes per operand: 3 = the exact split; 1 = SO_LINEAR_BF16X1 (LINEAR_BF16), ONE product of the round-to-nearest-even
// bfloat16 of dY and X — one conversion per loaded value instead of the split, one MFMA instead of six, and the bias gradient is
// the float32 running sum of the ROUNDED dY (the mode computes what the default would on the rounded operands).  The 16-row
// walk, the tiles, the block reduction and the stores are P = 3's.  P = 1 also has the K = 128 instances (KT = 4) that P = 3
// leaves to the f32-MFMA kernel: a flagged launch never runs on that one.  Two things are P = 1's own (measured):
// it prefetches the next step wherever <= 6 accumulator tiles leave the registers (with a sixth of the matrix work nothing else
// hides a load: without it the NTW = 2 shapes ran 2 x slower than the default), and K = 192 runs as two blocks of three column
// tiles (grid z) instead of KT = 6, which has no registers for the prefetch.
template <int KT, int NTW, bool GRP = false, int P = 3>
__global__ __launch_bounds__(256, 2) void linear_wgrad_b3_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                 float *__restrict__ part_w, float *__restrict__ part_b,
                                                                 long long T, int N, int K, long long rows_per_block, so_group_table gr) {
    static_assert(P == 3 || P == 1, "planes per operand");
    // P = 1: blockIdx.z selects a block of KT * 32 input columns (K = 192 runs as two halves of three tiles: six tiles and a
    // prefetch do not fit the registers, and without the prefetch the one-product loop only waits for its loads)
    int k0 = 0;
    if constexpr (P == 1) k0 = blockIdx.z * (KT * 32);
    __shared__ float red[NTW * KT * 1024];
    __shared__ float red_b[4][NTW * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, half = lane >> 5;                       // half = k block (rows 8 half .. 8 half + 7 of a step)
    const int chunk = blockIdx.x;
    const int n0 = blockIdx.y * (NTW * 32);
    long long r_blk, r_end;
    so_wgrad_chunk<GRP>(gr, chunk, rows_per_block, T, r_blk, r_end);
    const long long rpw = rows_per_block / 4;
    const long long r0 = r_blk + wave * rpw, r1 = min(r_end, r0 + rpw);

    f32x16 acc[NTW][KT];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][u][v] = 0.0f;
    float bsum[NTW];
    bool ncol[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) { bsum[t] = 0.0f; ncol[t] = n0 + t * 32 + i < N; }

    // the operands of step r + 16 are loaded before the MFMAs of step r (NTW = 1: the registers are there): a wave has
    // 2 - 3 neighbours on its SIMD, not enough to cover the HBM latency of 16 rows by themselves
    // (NTW = 2 with the second operand set: 255 registers, measured 58 -> 74 us).  P = 1 has one plane per operand instead of three and
    // a sixth of the matrix work to hide a load behind: it prefetches wherever <= 6 accumulator tiles leave the registers.
    constexpr bool PF = (NTW == 1 && KT <= 3) || (P == 1 && NTW * KT <= 6 && KT <= 4);
    float a[NTW][8], b[KT][8], an[PF ? NTW : 1][8], bn[PF ? KT : 1][8];
    auto load_step = [&](long long r, float (&da)[NTW][8], float (&db)[KT][8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long rr = r + 8 * half + j;
            const bool ok = rr < r1;
            const float *dyr = dy + rr * N + n0 + i;
            const float *xr = x + rr * K + k0 + i;
#pragma unroll
            for (int t = 0; t < NTW; ++t) da[t][j] = (ok && ncol[t]) ? dyr[t * 32] : 0.0f;
#pragma unroll
            for (int u = 0; u < KT; ++u) db[u][j] = ok ? xr[u * 32] : 0.0f;
        }
    };
    if constexpr (PF) load_step(r0, a, b);
    for (long long r = r0; r < r1; r += 16) {
        if constexpr (PF) {
            if (r + 16 < r1) load_step(r + 16, an, bn);
        } else {
            load_step(r, a, b);
        }
        if constexpr (P == 3) {
            bf16x8w b1[KT], b2[KT], b3[KT];
#pragma unroll
            for (int u = 0; u < KT; ++u) so_wsplit3(b[u], b1[u], b2[u], b3[u]);
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum[t] += a[t][j];
                bf16x8w a1, a2, a3;
                so_wsplit3(a[t], a1, a2, a3);
#pragma unroll
                for (int u = 0; u < KT; ++u) {
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b2[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b1[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2[u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[u], acc[t][u], 0, 0, 0);
                }
            }
        } else {
            bf16x8w b1[KT];
#pragma unroll
            for (int u = 0; u < KT; ++u)
#pragma unroll
                for (int j = 0; j < 8; ++j) b1[u][j] = (__bf16)b[u][j];
#pragma unroll
            for (int t = 0; t < NTW; ++t) {
                bf16x8w a1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a1[j] = (__bf16)a[t][j];
                    bsum[t] += (float)a1[j];
                }
#pragma unroll
                for (int u = 0; u < KT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1[u], acc[t][u], 0, 0, 0);
            }
        }
        if constexpr (PF) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int t = 0; t < NTW; ++t) a[t][j] = an[t][j];
#pragma unroll
                for (int u = 0; u < KT; ++u) b[u][j] = bn[u][j];
            }
        }
    }

    // block reduction and stores: as in linear_wgrad_kernel
#pragma unroll
    for (int t = 0; t < NTW; ++t) bsum[t] += __shfl_xor(bsum[t], 32, 64);
    if (half == 0) {
#pragma unroll
        for (int t = 0; t < NTW; ++t) red_b[wave][t * 32 + i] = bsum[t];
    }
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int u = 0; u < KT; ++u)
#pragma unroll
                    for (int v = 0; v < 16; ++v) red[((t * KT + u) * 16 + v) * 64 + lane] = acc[t][u][v];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int u = 0; u < KT; ++u)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[t][u][v] += red[((t * KT + u) * 16 + v) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    float *pw = part_w + (size_t)chunk * N * K;
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = n0 + t * 32 + (v & 3) + 8 * (v >> 2) + 4 * half;
            if (n >= N) continue;
#pragma unroll
            for (int u = 0; u < KT; ++u) pw[(size_t)n * K + k0 + u * 32 + i] = acc[t][u][v];
        }
        if (half == 0 && ncol[t] && k0 == 0)
            part_b[(size_t)chunk * N + n0 + t * 32 + i] =
                (red_b[0][t * 32 + i] + red_b[1][t * 32 + i]) + (red_b[2][t * 32 + i] + red_b[3][t * 32 + i]);
    }
}

// dW / db = sum over the chunks in a fixed order: wave w of a block adds the chunks c = w (mod 4) of 64 consecutive
// elements (8 loads in flight), the four waves are combined through LDS
__global__ __launch_bounds__(256) void linear_wgrad_reduce_kernel(const float *__restrict__ part_w,
                                                                  const float *__restrict__ part_b,
                                                                  float *__restrict__ dw, float *__restrict__ db, so_group_table gr,
                                                                  int NK, int N) {
    // blockIdx.y = row group: its chunks' partials -> its dw / db (an empty group sums nothing: zeros)
    const auto grp = so_group_of<true>(gr, (int)blockIdx.y);
    const int chunks = grp.units;
    part_w += (size_t)grp.first * NK;
    part_b += (size_t)grp.first * N;
    dw += (size_t)blockIdx.y * NK;
    if (db) db += (size_t)blockIdx.y * N;
    __shared__ float red[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int e = blockIdx.x * 64 + lane;
    const bool is_w = e < NK, is_b = !is_w && e < NK + N && db != nullptr;
    const float *src = is_w ? part_w + e : part_b + (e - NK);
    const size_t stride = is_w ? (size_t)NK : (size_t)N;
    float s = 0.0f;
    if (is_w || is_b) {
        int c = wave;
        for (; c + 28 < chunks; c += 32) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = src[(size_t)(c + 4 * j) * stride];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += t[j];
        }
        for (; c < chunks; c += 4) s += src[(size_t)c * stride];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        const float tot = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (is_w) dw[e] = tot;
        else if (is_b) db[e - NK] = tot;
    }
}

struct WgradPlan {
    int kt, ntw, ngroups, chunks;
    int kz;       // blocks of kt * 32 input columns (grid z): 1, or 2 for the one-product K = 192 plan
    long long rows_per_block;
    bool x1;      // SO_LINEAR_BF16X1: the one-product (P = 1) instance of the bf16 kernel
};

// round 3: the bf16 three-way-split kernels (same results to float32 rounding); SELFOCC_LINEAR_B3=0 keeps the f32-MFMA ones
bool so_wgrad_b3() {
    static const bool on = !(getenv("SELFOCC_LINEAR_B3") && atoi(getenv("SELFOCC_LINEAR_B3")) == 0);
    return on;
}

bool so_wgrad_flags_ok(uint32_t flags) { return !(flags & ~(uint32_t)SO_LINEAR_BF16X1); }

bool so_wgrad_plan(long long T, int N, int K, WgradPlan &p, uint32_t flags = 0) {
    static const int env_chunks = getenv("SELFOCC_WGRAD_CHUNKS") ? atoi(getenv("SELFOCC_WGRAD_CHUNKS")) : 0;     // dev A/B
    // SO_LINEAR_BF16X1: always the bf16 kernel (its P = 1 instance), whatever SELFOCC_LINEAR_B3 says and at K = 128 too — the
    // f32-MFMA kernel never serves a flagged launch.  Its tile rows are the default bf16 plan's; K = 128 takes K = 96's rule.
    // NTW is never above the default plan's for the same shape, so the plan never has more chunks: selfocc_linear_wgrad_workspace
    // is a valid upper bound for a flagged launch (tests/test_linear_bf16_cpu.py sweeps it).
    p.x1 = (flags & SO_LINEAR_BF16X1) != 0;
    p.kz = 1;
    const bool b3 = p.x1 || so_wgrad_b3();
    // tile rows of dY per wave (NTW).  bf16x3 kernels, K = 96: one or two (round 3, scripts/micro/wgrad_bench.py: N <= 96 had
    // 128 blocks = one wave on half of the SIMDs with three; 40 -> 28 us at 66 049 x 96 x 96, 108 -> 84 us at 153 000 x 288 x 96
    // with two); K = 192: one (222 registers; 66 -> 44 us at 78 899 x 96 x 192); K = 128 stays on the f32-MFMA kernel
    if (K == 96) { p.kt = 3; p.ntw = b3 ? ((N <= 96 || T < 16384) ? 1 : 2) : 3; }
    // one-product K = 192: two halves of three column tiles (grid z), one tile row as the default's K = 192 plan has — so the
    // chunks, and with them the workspace, are the default plan's
    else if (K == 192 && p.x1) { p.kt = 3; p.ntw = 1; p.kz = 2; }
    else if (K == 192) { p.kt = 6; p.ntw = b3 ? 1 : 2; }
    else if (K == 32) { p.kt = 1; p.ntw = 4; }
    else if (K == 64) { p.kt = 2; p.ntw = b3 ? 2 : 4; }
    else if (K == 128) { p.kt = 4; p.ntw = p.x1 ? ((N <= 96 || T < 16384) ? 1 : 2) : 3; }
    else return false;
    if (T < 1 || N < 1 || (long long)N * K >= (1LL << 30)) return false;
    const int nt = (N + 31) / 32;
    p.ngroups = (nt + p.ntw - 1) / p.ntw;
    // ~2 blocks per CU, at most 128 partial sums per element; at least 64 rows per block (16 per wave)
    const int target = env_chunks > 0 ? 4 * env_chunks : 512;
    long long chunks = std::max(1LL, std::min((long long)(target / std::max(1, std::min(p.ngroups, target))), (T + 63) / 64));
    chunks = std::min(chunks, env_chunks > 0 ? (long long)env_chunks : 128LL);
    long long rpb = (T + chunks - 1) / chunks;
    rpb = (rpb + 7) / 8 * 8;                          // rows per wave a multiple of 2
    chunks = (T + rpb - 1) / rpb;
    p.chunks = (int)chunks;
    p.rows_per_block = rpb;
    return true;
}

}  // namespace

extern "C" int selfocc_linear_wgrad_supported(int64_t T, int32_t N, int32_t K) {
    WgradPlan p;
    return so_wgrad_plan(T, N, K, p) ? 1 : 0;
}

extern "C" size_t selfocc_linear_wgrad_workspace_flags(int64_t T, int32_t N, int32_t K, uint32_t flags) {
    WgradPlan p;
    if (!so_wgrad_flags_ok(flags) || !so_wgrad_plan(T, N, K, p, flags)) return 0;
    return (size_t)p.chunks * ((size_t)N * K + N) * sizeof(float);
}

extern "C" size_t selfocc_linear_wgrad_workspace(int64_t T, int32_t N, int32_t K) {
    return selfocc_linear_wgrad_workspace_flags(T, N, K, 0);
}

// the chunk table: group g's rows in ceil(rows_g / rows_per_block) chunks of the plan's rows_per_block (none for an empty group)
static so_group_table so_wgrad_groups(const so_row_groups &in, const WgradPlan &p) {
    return so_build_group_table(in, [&](long long rows) { return (rows + p.rows_per_block - 1) / p.rows_per_block; });
}

static int so_wgrad_launch(const float *dy, const float *x, float *dw, float *db, long long T, int N, int K, const WgradPlan &p,
                           const so_group_table &gr, bool grouped, void *workspace, size_t workspace_bytes, void *stream) {
    SO_REQUIRE(dy && x && dw, "linear_wgrad: NULL pointer");
    const int chunks = gr.unit_start[gr.n];
    const size_t need = (size_t)chunks * ((size_t)N * K + N) * sizeof(float);
    SO_REQUIRE(workspace != nullptr && workspace_bytes >= need, "linear_wgrad: workspace too small (%zu bytes, need %zu)",
               workspace_bytes, need);
    float *part_w = (float *)workspace, *part_b = part_w + (size_t)chunks * N * K;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)p.ngroups, (unsigned)p.kz);
    const bool b3 = p.x1 || (so_wgrad_b3() && p.kt != 4);      // default: K = 128 stays on the f32-MFMA kernel
    bool launched = chunks == 0;
    // one (kernel, KT, NTW) of the list below: launched when it is the plan's
    auto pass = [&](auto B3, auto KT, auto NTW) {
        if (launched || p.x1 || b3 != B3 || p.kt != KT || p.ntw != NTW) return;
        launched = true;
        so_with_const<bool, true, false>(grouped, [&](auto GRP) {
            if constexpr (B3)
                hipLaunchKernelGGL((linear_wgrad_b3_kernel<KT, NTW, GRP, 3>), grid, dim3(256), 0, st, dy, x, part_w, part_b, T, N, K,
                                   p.rows_per_block, gr);
            else
                hipLaunchKernelGGL((linear_wgrad_kernel<KT, NTW, GRP>), grid, dim3(256), 0, st, dy, x, part_w, part_b, T, N, K,
                                   p.rows_per_block, gr);
        });
    };
    // ... and of the one-product instances (SO_LINEAR_BF16X1)
    auto pass1 = [&](auto KT, auto NTW) {
        if (launched || !p.x1 || p.kt != KT || p.ntw != NTW) return;
        launched = true;
        so_with_const<bool, true, false>(grouped, [&](auto GRP) {
            hipLaunchKernelGGL((linear_wgrad_b3_kernel<KT, NTW, GRP, 1>), grid, dim3(256), 0, st, dy, x, part_w, part_b, T, N, K,
                               p.rows_per_block, gr);
        });
    };
    // the (KT, NTW) pairs so_wgrad_plan can produce; only these are instantiated (the b3 kernel at 3 x 3 / 4 x 3 / 6 x 2
    // accumulator tiles needs more than 256 registers)
    constexpr std::true_type B3;
    constexpr std::false_type F32;
    pass(B3, so_int<1>{}, so_int<4>{}); pass(B3, so_int<2>{}, so_int<2>{}); pass(B3, so_int<3>{}, so_int<1>{});
    pass(B3, so_int<3>{}, so_int<2>{}); pass(B3, so_int<6>{}, so_int<1>{});
    pass(F32, so_int<1>{}, so_int<4>{}); pass(F32, so_int<2>{}, so_int<4>{}); pass(F32, so_int<3>{}, so_int<3>{});
    pass(F32, so_int<4>{}, so_int<3>{}); pass(F32, so_int<6>{}, so_int<2>{});
    pass1(so_int<1>{}, so_int<4>{}); pass1(so_int<2>{}, so_int<2>{}); pass1(so_int<3>{}, so_int<1>{}); pass1(so_int<3>{}, so_int<2>{});
    pass1(so_int<4>{}, so_int<1>{}); pass1(so_int<4>{}, so_int<2>{});
    SO_REQUIRE(launched, "linear_wgrad: no kernel for the plan's KT = %d, NTW = %d", p.kt, p.ntw);
    const int NK = N * K;
    hipLaunchKernelGGL(linear_wgrad_reduce_kernel, dim3((unsigned)((NK + N + 63) / 64), (unsigned)gr.n), dim3(256), 0, st, part_w,
                       part_b, dw, db, gr, NK, N);
    return so_launch_status();
}

extern "C" int selfocc_linear_wgrad_flags(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                                          void *workspace, size_t workspace_bytes, uint32_t flags, void *stream) {
    WgradPlan p;
    SO_REQUIRE(so_wgrad_flags_ok(flags), "linear_wgrad: unknown flags 0x%x (SO_LINEAR_BF16X1 is the only one)", flags);
    SO_REQUIRE(so_wgrad_plan(T, N, K, p, flags), "linear_wgrad: unsupported shape (T = %lld rows, N = %d, K = %d; K must be 32, 64, "
               "96, 128 or 192)", (long long)T, N, K);
    so_group_table gr = {};
    gr.n = 1;
    gr.unit_start[1] = p.chunks;
    gr.row_start[1] = T;
    return so_wgrad_launch(dy, x, dw, db, T, N, K, p, gr, false, workspace, workspace_bytes, stream);
}

extern "C" int selfocc_linear_wgrad(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N,
                                    int32_t K, void *workspace, size_t workspace_bytes, void *stream) {
    return selfocc_linear_wgrad_flags(dy, x, dw, db, T, N, K, workspace, workspace_bytes, 0, stream);
}

// the plan of the grouped pass: the ungrouped plan of all T rows (kernel choice, rows per chunk), chunks cut per group
static int so_wgrad_grouped_plan(long long T, int N, int K, const so_row_groups &groups, WgradPlan &p, so_group_table &gr,
                                 uint32_t flags) {
    SO_REQUIRE(so_wgrad_flags_ok(flags), "linear_wgrad_grouped: unknown flags 0x%x (SO_LINEAR_BF16X1 is the only one)", flags);
    if (so_check_row_groups(groups, T, "linear_wgrad_grouped") < 0) return -1;
    SO_REQUIRE(so_wgrad_plan(T > 0 ? T : 1, N, K, p, flags), "linear_wgrad_grouped: unsupported shape (T = %lld rows, N = %d, K = %d; "
               "K must be 32, 64, 96, 128 or 192)", T, N, K);
    gr = so_wgrad_groups(groups, p);
    return 0;
}

extern "C" int selfocc_linear_wgrad_grouped_supported(int64_t T, int32_t N, int32_t K, so_row_groups groups) {
    if (so_check_row_groups(groups, T, "linear_wgrad_grouped") < 0) return -1;
    WgradPlan p;
    return so_wgrad_plan(T > 0 ? T : 1, N, K, p) ? 1 : 0;
}

extern "C" size_t selfocc_linear_wgrad_grouped_workspace_flags(int64_t T, int32_t N, int32_t K, so_row_groups groups, uint32_t flags) {
    WgradPlan p;
    so_group_table gr;
    if (so_wgrad_grouped_plan(T, N, K, groups, p, gr, flags) < 0) return 0;
    const size_t chunks = (size_t)std::max(1, gr.unit_start[gr.n]);
    return chunks * ((size_t)N * K + N) * sizeof(float);
}

extern "C" size_t selfocc_linear_wgrad_grouped_workspace(int64_t T, int32_t N, int32_t K, so_row_groups groups) {
    return selfocc_linear_wgrad_grouped_workspace_flags(T, N, K, groups, 0);
}

extern "C" int selfocc_linear_wgrad_grouped_flags(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                                                  so_row_groups groups, void *workspace, size_t workspace_bytes, uint32_t flags,
                                                  void *stream) {
    WgradPlan p;
    so_group_table gr;
    if (so_wgrad_grouped_plan(T, N, K, groups, p, gr, flags) < 0) return -1;
    return so_wgrad_launch(dy, x, dw, db, T, N, K, p, gr, true, workspace, workspace_bytes, stream);
}

extern "C" int selfocc_linear_wgrad_grouped(const float *dy, const float *x, float *dw, float *db, int64_t T, int32_t N, int32_t K,
                                            so_row_groups groups, void *workspace, size_t workspace_bytes, void *stream) {
    return selfocc_linear_wgrad_grouped_flags(dy, x, dw, db, T, N, K, groups, workspace, workspace_bytes, 0, stream);
}

