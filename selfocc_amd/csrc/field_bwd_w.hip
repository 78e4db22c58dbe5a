// field_bwd_w.hip — backward of the fused tri-plane -> volume MLP (training, one hidden layer) on float32 MFMA, generic in the
// width: embed_dims 64, 96 and 128.  At C = 96 it is the route of the heads that field_bwd_b3.hip does not
// take (a feature stride that is no multiple of 4, volumes past 32-bit indexing, SELFOCC_FIELD_BWD_B3=0).
//
// Reference semantics: autograd through  x = hw + zh + wz,  a = Softplus(x),  y = W1 a + b1,  z = Softplus(y),
// out = W2 z + b2  (sdfstudio-fork SDFCustomField; in-repo analogue model/head/nerfacc_head/bev_nerf.py:74-95).
// Nothing of the forward is kept; per 32-voxel tile (a 4 x 4 x 2 patch) the activations are recomputed and
//     y   = a W1^T            (K = C inputs)         dZ  = dOut W2          (K = 32 outputs)      dY = dZ * sigmoid(y)
//     dW2 += dOut^T z         (K = 32 voxels)        dW1 += dY^T a          (K = 32 voxels)
//     dA  = dY W1             (K = C units)          dX  = dA * sigmoid(x)  -> the three plane gradients
// run on v_mfma_f32_32x32x2_f32 (an exact k-ordered fmaf chain: float32 arithmetic).  The plane gradients are scattered with
// one 128-byte row segment per plane row of the tile (g_hw summed along the d-walk first), the weight / bias gradients stay in
// accumulators for all tiles of a wave and are added to global memory once at the end.
//
// A wave owns NCT 32-column tiles — hidden units n in y / dZ / dY / dW2 / the rows of dW1, inputs k in dA / dX — so its
// accumulators are dW1[NCT][C / 32] + dW2[NCT]: 96 registers at C = 64, 192 at C = 96, 160 at C = 128 (the 320 that a wave
// owning all of a 128-wide tile would need do not fit the 512 registers of a lane next to the operands).
//   C = 64:  NCT = 2, one wave per tile, four tiles in flight per block, no block barrier.
//   C = 96:  NCT = 3, one wave per tile, four tiles in flight per block, no block barrier.
//   C = 128: NCT = 2, TWO waves per tile (sub = 0 / 1: columns 0..63 / 64..127), two tiles in flight per block.  The pair shares
//            the tile's two transpose tiles in LDS: each wave computes its half of a (S1) and of dY (S7), the other one reads
//            them as the contraction operand of y (S2), dW1 (S8) and dA (S9).  Three block barriers per tile; no MFMA is
//            issued twice (896 per tile, 448 per wave), only the 32 x 32 upstream gradient is loaded by both waves.
// LDS: W1 as [k][n] with row stride C + 1 (conflict-free as B[k][n] for y AND as B[n][k] for dA), W2 as [o][n], and per
// tile in flight T1 (a) and T2 (z, then dY) of 32 x (C + 4) floats: 94.6 KB at C = 64, 148.5 KB at C = 96, 150.1 KB at C = 128.
#include "field_device.h"
#include <algorithm>

namespace {

constexpr int kFW_WAVES = 4;

// acc[ct] += A B over KS k-steps, the lane's A operands (its A-layout run of an LDS tile row) read 16 steps at a time, one
// chunk ahead of the MFMAs that use it: 32 live operand registers instead of KS
template <int KS, int NCT, class BOp>
SO_DEVFN void fw_chain(f32x16 (&acc)[NCT], const float *arun, BOp &&bop) {
    float cur[16], nxt[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = ((const float4 *)arun)[q];
        cur[4 * q + 0] = t.x; cur[4 * q + 1] = t.y; cur[4 * q + 2] = t.z; cur[4 * q + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < KS / 16; ++c) {
        if (c + 1 < KS / 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 t = ((const float4 *)arun)[4 * (c + 1) + q];
                nxt[4 * q + 0] = t.x; nxt[4 * q + 1] = t.y; nxt[4 * q + 2] = t.z; nxt[4 * q + 3] = t.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j], bop(16 * c + j, ct), acc[ct], 0, 0, 0);
            if (j == 7) __builtin_amdgcn_sched_barrier(0);                // bound the B reads hoisted over the chain
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) cur[j] = nxt[j];
    }
}

constexpr int fw_wpt(int C) { return C == 128 ? 2 : 1; }      // waves per tile
constexpr int fw_tpb(int C) { return kFW_WAVES / fw_wpt(C); }  // tiles in flight per block
constexpr size_t fw_lds_bytes(int C) {
    return ((size_t)C * (C + 1) + 32 * (C + 1) + (size_t)fw_tpb(C) * 2 * 32 * (C + 4)) * sizeof(float);
}

template <int C>
__global__ __launch_bounds__(kFW_WAVES * 64) void field_volume_bwd_w_kernel(FieldBwdArgs a) {
    static_assert(C == 64 || C == 96 || C == 128, "a wave owns two or three 32-column tiles: one or two waves per tile");
    constexpr int KS = C / 2;             // k-steps of a GEMM that contracts C features (2 k per MFMA)
    constexpr int KT = C / 32;            // 32-column tiles of the full width
    constexpr int WPT = fw_wpt(C), TPB = fw_tpb(C);
    constexpr int NCT = KT / WPT;         // 32-column tiles of a wave
    constexpr int RUN = KS / WPT;         // the part of its A-layout run that a lane builds in S1
    constexpr int LD = C + 1, TS = C + 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *w1s = smem;                          // [kk = ks * 2 + half][n], k = half * KS + ks      C x LD
    float *w2k = w1s + C * LD;                  // [oo = os * 2 + ohalf][n], o = ohalf * 16 + os    32 x LD
    float *tiles = w2k + 32 * LD;               // per tile in flight: T1 (a), T2 (z, then dY)     2 x 32 x TS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, half = lane >> 5;
    const int slot = wave / WPT, sub = wave % WPT;
    const int n0 = 32 * NCT * sub;              // the wave's first column
    for (int e = threadIdx.x; e < C * C; e += kFW_WAVES * 64) {
        const int k = e % C, n = e / C;                       // coalesced read of w1 (n, k)
        w1s[((k % KS) * 2 + k / KS) * LD + n] = a.w1[e];
    }
    for (int e = threadIdx.x; e < 32 * C; e += kFW_WAVES * 64) {
        const int n = e % C, o = e / C;
        w2k[((o % 16) * 2 + o / 16) * LD + n] = o < a.out_dim ? a.w2[(size_t)o * C + n] : 0.0f;
    }
    __syncthreads();
    float *T1 = tiles + (size_t)slot * 2 * 32 * TS, *T2 = T1 + 32 * TS;

    f32x16 dW1[NCT][KT], dW2[NCT];
#pragma unroll
    for (int r = 0; r < NCT; ++r) {
#pragma unroll
        for (int v = 0; v < 16; ++v) dW2[r][v] = 0.0f;
#pragma unroll
        for (int c = 0; c < KT; ++c)
#pragma unroll
            for (int v = 0; v < 16; ++v) dW1[r][c][v] = 0.0f;
    }
    float db1[NCT] = {};
    float db2 = 0.0f;                           // output i, the tile rows of parity half (summed where S6 loads dOut^T)
    float bias1[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) bias1[ct] = a.b1[n0 + ct * 32 + i];

    // d-walk (so_tile_range): the 16 hw rows of the slot's current (h, w) column of patches are carried in registers
    float hw_acc[NCT][8];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int q = 0; q < 8; ++q) hw_acc[ct][q] = 0.0f;
    int col_prev = -1;
    auto flush_hw = [&](int col) {
        const int pw_ = col % a.PW, ph_ = col / a.PW;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int hh = 4 * ph_ + (q >> 1), ww = 4 * pw_ + 2 * half + (q & 1);
                if (hh < a.H && ww < a.W && hw_acc[ct][q] != 0.0f)
                    unsafeAtomicAdd(a.g_hw + ((size_t)hh * a.W + ww) * C + n0 + ct * 32 + i, hw_acc[ct][q]);
                hw_acc[ct][q] = 0.0f;
            }
        }
    };
    const int n_slots = gridDim.x * TPB, sid = blockIdx.x * TPB + slot;
    int t_lo, t_hi;
    so_tile_range(a.n_tiles, sid, n_slots, t_lo, t_hi);
    // with two waves per tile the block's slots keep step (block barriers): every slot runs the trip count of the longest
    // one, and a slot that has no tile left only keeps the barriers
    const int n_iter = WPT == 1 ? t_hi - t_lo : (a.n_tiles + n_slots - 1) / n_slots;
    for (int it = 0; it < n_iter; ++it) {
        const int tile = t_lo + it;
        if (WPT > 1 && tile >= t_hi) {     // wave-uniform
            __syncthreads();
            __syncthreads();
            __syncthreads();
            continue;
        }
        if (tile / a.PD != col_prev) {
            if (col_prev >= 0) flush_hw(col_prev);
            col_prev = tile / a.PD;
        }
        int h_b, w_b, d_b;
        so_patch_origin(tile, a.PW, a.PD, h_b, w_b, d_b);
        auto row_voxel = [&](int r, bool &live) {                // linear index of tile row r (64-bit: every volume size)
            return so_patch_voxel<long long, false>(h_b, w_b, d_b, r >> 3, (r >> 1) & 3, r & 1, a.H, a.W, a.D, live);
        };
        // ---- S1: a = Softplus(x): the lane builds RUN columns of row i (of its A-layout run half * KS .. + KS, the part
        //      sub * RUN .. + RUN) -> T1; with two waves per tile the A-layout run is read back once both halves stand ----
        bool mlive;
        const long long m = row_voxel(i, mlive);
        const int h = min(h_b + (i >> 3), a.H - 1), w = min(w_b + ((i >> 1) & 3), a.W - 1), d = min(d_b + (i & 1), a.D - 1);
        const int hwi = h * a.W + w;
        float av[RUN];                                                   // WPT == 1: the lane's whole A-layout run
        {
            const int c0 = half * KS + sub * RUN;
            const float4 *p0 = (const float4 *)(a.hw + (size_t)hwi * C + c0);
            const float4 *p1 = (const float4 *)(a.zh + ((size_t)d * a.H + h) * C + c0);
            const float4 *p2 = (const float4 *)(a.wz + ((size_t)w * a.D + d) * C + c0);
            float4 *t1 = (float4 *)(T1 + i * TS + c0);
#pragma unroll
            for (int q = 0; q < RUN / 4; ++q) {
                const float4 x0 = p0[q], x1 = p1[q], x2 = p2[q];
                float4 s4;
                s4.x = so_softplus((x0.x + x1.x) + x2.x);
                s4.y = so_softplus((x0.y + x1.y) + x2.y);
                s4.z = so_softplus((x0.z + x1.z) + x2.z);
                s4.w = so_softplus((x0.w + x1.w) + x2.w);
                if (WPT == 1) { av[4 * q + 0] = s4.x; av[4 * q + 1] = s4.y; av[4 * q + 2] = s4.z; av[4 * q + 3] = s4.w; }
                t1[q] = s4;
                if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // at most 4 x 3 loads in flight
            }
        }
        if (WPT > 1) __syncthreads();                                     // barrier 1: T1 complete
        __builtin_amdgcn_sched_barrier(0);
        // ---- S2: y = W1 a + b1 (C layout, the wave's NCT x 32 units); z = Softplus(y) -> T2 ----------------------------
        f32x16 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[ct][v] = 0.0f;
        {
            const float *bcol = w1s + half * LD + n0 + i;
            if constexpr (WPT == 1) {                                     // the lane's own S1 registers
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ks], bcol[ks * 2 * LD + ct * 32], acc[ct], 0, 0, 0);
                    if ((ks & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                fw_chain<KS, NCT>(acc, T1 + i * TS + half * KS, [&](int ks, int ct) { return bcol[ks * 2 * LD + ct * 32]; });
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int v = 0; v < 16; ++v) T2[so_crow(v, half) * TS + n0 + ct * 32 + i] = so_softplus(acc[ct][v] + bias1[ct]);
        __builtin_amdgcn_sched_barrier(0);
        // ---- S3: dOut, A layout: lane (row i, half) holds outputs half * 16 .. + 16 ------------------------------
        float dav[16];
#pragma unroll
        for (int os = 0; os < 16; ++os) {
            const int o = half * 16 + os;
            float g = 0.0f;
            if (mlive && o < a.out_dim) {
                if (o == 0) g = a.g_sdf ? a.g_sdf[m] : 0.0f;
                else g = a.g_feat ? a.g_feat[(size_t)m * a.feat_stride + (o - 1)] : 0.0f;
            }
            dav[os] = g;
        }
        // ---- S4 / S5: dZ = dOut W2 ; dY = dZ sigmoid(y) ----------------------------------------------------------
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[ct][v] = 0.0f;
#pragma unroll
        for (int os = 0; os < 16; ++os) {
            const float *brow = w2k + (os * 2 + half) * LD + n0 + i;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(dav[os], brow[ct * 32], acc[ct], 0, 0, 0);
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            float sum = 0.0f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const float z = T2[so_crow(v, half) * TS + n0 + ct * 32 + i];   // this lane's own element (written in S2)
                acc[ct][v] = acc[ct][v] * (1.0f - __expf(-z));                  // sigmoid(y) = 1 - exp(-softplus(y))
                sum += acc[ct][v];
            }
            db1[ct] += sum;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- S6: dW2 += dOut^T z : rows o, the wave's columns n, K = the 32 rows of the tile -------------------
#pragma unroll
        for (int ms = 0; ms < 16; ++ms) {
            bool rlive;
            const long long mr = row_voxel(2 * ms + half, rlive);  // A' operand: dOut[mr][o = i]
            float g = 0.0f;
            if (rlive && i < a.out_dim) {
                if (i == 0) g = a.g_sdf ? a.g_sdf[mr] : 0.0f;
                else g = a.g_feat ? a.g_feat[(size_t)mr * a.feat_stride + (i - 1)] : 0.0f;
            }
            db2 += g;
            const float *zrow = T2 + (2 * ms + half) * TS + n0 + i;   // B' operand: z[mr][n] (the wave's own writes)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
                dW2[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(g, zrow[ct * 32], dW2[ct], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        // ---- S7: dY -> T2 (the wave's columns)      ----------------------------------------------------------------
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int v = 0; v < 16; ++v) T2[so_crow(v, half) * TS + n0 + ct * 32 + i] = acc[ct][v];
        if (WPT > 1) {
            __syncthreads();                                              // barrier 2: T2 = dY complete
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S8: dW1 += dY^T a : rows n (the wave's NCT tiles), columns k (all KT tiles) ----------------------------
#pragma unroll
        for (int ms = 0; ms < 16; ++ms) {
            const float *arow = T1 + (2 * ms + half) * TS + i;
            const float *yrow = T2 + (2 * ms + half) * TS + n0 + i;
            float bv[NCT];
#pragma unroll
            for (int rt = 0; rt < NCT; ++rt) bv[rt] = yrow[rt * 32];
#pragma unroll
            for (int ct = 0; ct < KT; ++ct) {                       // rows n (from dY), columns k (from a):
                const float avv = arow[ct * 32];                    // row-contiguous in g_w1 (n, k)
#pragma unroll
                for (int rt = 0; rt < NCT; ++rt)
                    dW1[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[rt], avv, dW1[rt][ct], 0, 0, 0);
            }
            if ((ms & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S9: dA = dY W1 (the wave's inputs k): A = dY in A layout (all of T2), B[n][k] = w1s read the other way
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[ct][v] = 0.0f;
        {
            int krow[NCT];                                          // w1s row of column k = n0 + ct * 32 + i
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int k = n0 + ct * 32 + i;
                krow[ct] = ((k % KS) * 2 + k / KS) * LD;
            }
            fw_chain<KS, NCT>(acc, T2 + i * TS + half * KS, [&](int ns, int ct) { return w1s[krow[ct] + half * KS + ns]; });
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S10 / S11: dX = dA sigmoid(x) (C layout) -> plane gradients -----------------------------------------
        // C-layout register v of lane (i, half) = tile row r = (v & 3) + 8 (v >> 2) + 4 half = patch voxel
        //   dd = v & 1,   ww = 2 half + ((v >> 1) & 1),   hh = v >> 2
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int k = n0 + ct * 32 + i;
            float dx[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = so_crow(v, half);
                const bool live = so_creg_live(v, half, h_b, w_b, d_b, a.H, a.W, a.D);
                const float ar = T1[r * TS + k];
                dx[v] = live ? acc[ct][v] * (1.0f - __expf(-ar)) : 0.0f;
            }
            // g_hw[h][w] += sum over d: registers v, v ^ 1 (8 rows per lane, the halves hold different w)
#pragma unroll
            for (int q = 0; q < 8; ++q) hw_acc[ct][q] += dx[2 * q] + dx[2 * q + 1];
            // g_wz[w][d] += sum over h: registers v, v + 4, v + 8, v + 12 (4 rows per lane)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ww = w_b + 2 * half + (q >> 1), dd = d_b + (q & 1);
                if (ww < a.W && dd < a.D)
                    unsafeAtomicAdd(a.g_wz + ((size_t)ww * a.D + dd) * C + k, (dx[q] + dx[q + 4]) + (dx[q + 8] + dx[q + 12]));
            }
            // g_zh[d][h] += sum over w: registers v, v ^ 2 and the partner half; half 0 issues d = d_b, half 1 d = d_b + 1
#pragma unroll
            for (int hq = 0; hq < 4; ++hq) {
                const float s0 = dx[4 * hq] + dx[4 * hq + 2], s1 = dx[4 * hq + 1] + dx[4 * hq + 3];     // dd = 0 / 1, this half's two w
                const float t0 = s0 + __shfl_xor(s0, 32, 64), t1 = s1 + __shfl_xor(s1, 32, 64);
                const int hh = h_b + hq, dd = d_b + half;
                if (hh < a.H && dd < a.D) unsafeAtomicAdd(a.g_zh + ((size_t)dd * a.H + hh) * C + k, half ? t1 : t0);
            }
        }
        if (WPT > 1) __syncthreads();                                     // barrier 3: T1 / T2 free for the next tile
        else __builtin_amdgcn_wave_barrier();
    }
    if (col_prev >= 0) flush_hw(col_prev);

    // ---- the wave's weight / bias gradients -> global (once) -------------------------------------------------
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int cr = so_crow(v, half);
#pragma unroll
        for (int ct = 0; ct < KT; ++ct)
#pragma unroll
            for (int rt = 0; rt < NCT; ++rt)            // dW1[n = n0 + rt * 32 + cr][k = ct * 32 + i] -> g_w1 (n, k): 128-byte rows
                unsafeAtomicAdd(a.g_w1 + (size_t)(n0 + rt * 32 + cr) * C + ct * 32 + i, dW1[rt][ct][v]);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)                // dW2[o = cr][n = n0 + ct * 32 + i]
            if (cr < a.out_dim) unsafeAtomicAdd(a.g_w2 + (size_t)cr * C + n0 + ct * 32 + i, dW2[ct][v]);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const float tot = db1[ct] + __shfl_xor(db1[ct], 32, 64);
        if (half == 0) unsafeAtomicAdd(a.g_b1 + n0 + ct * 32 + i, tot);
    }
    if (sub == 0) {                                   // both waves of a tile saw the same dOut
        const float tot = db2 + __shfl_xor(db2, 32, 64);
        if (half == 0 && i < a.out_dim) unsafeAtomicAdd(a.g_b2 + i, tot);
    }
}

}  // namespace

int so_field_volume_bwd_w(const FieldBwdArgs &a, int C, hipStream_t st) {
    so_with_const<int, 64, 96, 128>(C, [&](auto CC) {
        const int blocks = std::min((a.n_tiles + fw_tpb(CC) - 1) / fw_tpb(CC), 256);      // one block per CU (LDS)
        so_launch_lds<field_volume_bwd_w_kernel<CC>>(dim3(blocks), dim3(kFW_WAVES * 64), fw_lds_bytes(CC), 160 * 1024 - 256, st, a);
    });
    return so_launch_status();
}
