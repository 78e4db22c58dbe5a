// camera_se.hip — CameraAwareSE (model/encoder/tpvformer/modules/camera_se_net.py) fused with the encoder's flatten
// (tpvformer_encoder.py:258-277).  Per FPN level the reference multiplies the map by the camera's gate, runs a 1x1
// convolution, then adds the camera and the level embedding on permuted views and concatenates: ten passes over the maps.
// The gate scales INPUT channels and the embeddings add to OUTPUT channels, so both fold into the convolution:
//     Wg[b,n] (C x M) = w * gate[b*N+n][None, :]          bias[n,l] = conv bias + cams_embeds[n] + level_embeds[l]
//     out[n][start_l + p][b][:] = Wg[b,n] x_l[b][n][:][p] + bias[n,l]
// a batched tall-skinny GEMM whose one operand is the map as it lies in memory (channel-major, pixels contiguous) and whose
// output rows are the pixel-major `value` rows the MSDA kernels read: the maps are read once, `value` is written once.
//
// Matrix pipe: v_mfma_f32_16x16x4_f32 (exact f32 fmaf chains).  A block stages its camera's gated weights in
// LDS once ([C][M + 4]: the pad makes both the forward's row-per-lane and the dgrad's row-per-lane-group reads
// conflict-free); the map / gradient operand goes from global memory straight into MFMA layout:
//   forward   D[c][pixel] = Wg (A, LDS) x X (B): a lane loads a float4 ALONG the pixels, its four values feed four
//             different 16-pixel tiles (pixel p0 + 4 m + j -> tile j, column m): 256 contiguous bytes per channel row per
//             16 lanes; the four accumulator registers of a lane are four consecutive output channels: one float4 store.
//   dgrad     D[pixel][k] = G (A) x Wg (B, LDS): a lane loads a float4 of g ALONG the channels and uses its four values in
//             four MFMA steps (the k order of a reduction is free as long as both operands agree); the four accumulator
//             registers are four consecutive pixels of one map channel: one float4 store into the channel-major gradient.
//   wgrad     dWc[b,n] (C x M) = sum_p g (x) x over ALL levels, the ungated map: 512-pixel chunks, each a block that stages
//             (64 pixels x C) of g and (M x 64 pixels) of x in LDS per step and keeps 2 x 2 wave tiles of the product in
//             registers; chunk partials and the chunk's column sums of g go to the workspace, a second kernel adds them in
//             chunk order: a fixed summation order, no float atomics (deterministic).
#include "so_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CS_TILE = 256;        // pixels per block, forward and dgrad (4 waves x 64)
constexpr int CS_CHUNK = 512;       // pixels per block, wgrad
constexpr int CS_MAX_LEVELS = 8;

struct CamSeArgs {
    const float *feat[CS_MAX_LEVELS];   // (B, N, M, hw_l) maps
    float *dfeat[CS_MAX_LEVELS];        // their gradients (NULL: not wanted)
    int hw[CS_MAX_LEVELS], start[CS_MAX_LEVELS];
    int tile0[CS_MAX_LEVELS + 1];       // first tile (CS_TILE pixels) / chunk (CS_CHUNK pixels) of level l
    const float *gate, *w, *bias, *cams, *lvls;
    float *out;                         // forward: (N, S, B, C)
    const float *g;                     // backward: (N, S, B, C)
    float *part_w, *part_c;             // wgrad partials: (B*N * chunks, C, M) and (B*N * chunks, C)
    int L, B, N, C, M, S;
};

__device__ __forceinline__ int cs_level_of(const CamSeArgs &a, int tile) {
    int l = 0;
    for (int k = 1; k < a.L; ++k) l += (tile >= a.tile0[k]);
    return l;
}

// Wg[c][k] = w[c][k] * gate[bn][k] into LDS rows of M + 4 floats
__device__ __forceinline__ void cs_stage_weights(float *wl, const CamSeArgs &a, int bn) {
    const int M = a.M, MP = M + 4;
    const float *gate = a.gate + (size_t)bn * M;
    for (int e = threadIdx.x; e < a.C * M; e += 256) {
        const int c = e / M, k = e - c * M;
        wl[c * MP + k] = a.w[e] * gate[k];
    }
}

// four consecutive pixels of one channel row; `vec`: the row start and p are 16-byte aligned (hw % 4 == 0)
__device__ __forceinline__ f32x4 cs_load_px4(const float *row, int p, int hw, bool vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec) {
        if (p < hw) v = *(const f32x4 *)(row + p);
    } else {
        if (p < hw) v[0] = row[p];
        if (p + 1 < hw) v[1] = row[p + 1];
        if (p + 2 < hw) v[2] = row[p + 2];
        if (p + 3 < hw) v[3] = row[p + 3];
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
template <int CT>   // C = 16 CT
__global__ __launch_bounds__(256) void camera_se_fwd_kernel(CamSeArgs a) {
    extern __shared__ float wl[];      // [C][M + 4]
    const int l = cs_level_of(a, (int)blockIdx.x);
    const int n = blockIdx.y, b = blockIdx.z, bn = b * a.N + n;
    const int M = a.M, MP = M + 4, hw = a.hw[l];
    constexpr int C = 16 * CT;
    cs_stage_weights(wl, a, bn);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int p0 = ((int)blockIdx.x - a.tile0[l]) * CS_TILE + wave * 64;
    if (p0 >= hw) return;
    const bool vec = (hw & 3) == 0;
    const float *x = a.feat[l] + (size_t)bn * M * hw;
    const int pl = p0 + 4 * m;                                   // this lane's pixels pl + j, j = tile

    f32x4 acc[CT][4];
    {
        const float *cb = a.bias, *ce = a.cams + (size_t)n * C, *le = a.lvls + (size_t)l * C;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            f32x4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = ct * 16 + 4 * q + r;
                t[r] = (cb[c] + ce[c]) + le[c];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[ct][j] = t;
        }
    }
    constexpr int U = 4;                                          // k steps in flight (M / 4 is a multiple of 8)
    f32x4 cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = cs_load_px4(x + (size_t)(4 * u + q) * hw, pl, hw, vec);
    for (int kk0 = 0; kk0 < M / 4; kk0 += U) {
        if (kk0 + U < M / 4) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = cs_load_px4(x + (size_t)(4 * (kk0 + U + u) + q) * hw, pl, hw, vec);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *wr = wl + m * MP + 4 * (kk0 + u) + q;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const float av = wr[ct * 16 * MP];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[ct][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, cur[u][j], acc[ct][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = pl + j;
        if (p < hw) {
            float *o = a.out + (((size_t)n * a.S + a.start[l] + p) * a.B + b) * C + 4 * q;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) *(f32x4 *)(o + ct * 16) = acc[ct][j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int MT>   // M = 16 MT
__global__ __launch_bounds__(256) void camera_se_dgrad_kernel(CamSeArgs a) {
    extern __shared__ float wl[];      // [C][M + 4]
    const int l = cs_level_of(a, (int)blockIdx.x);
    if (a.dfeat[l] == nullptr) return;                            // block-uniform
    const int n = blockIdx.y, b = blockIdx.z, bn = b * a.N + n;
    constexpr int M = 16 * MT, MP = M + 4;
    const int C = a.C, hw = a.hw[l];
    cs_stage_weights(wl, a, bn);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int p0 = ((int)blockIdx.x - a.tile0[l]) * CS_TILE + wave * 64;
    if (p0 >= hw) return;
    const size_t prow = (size_t)a.B * C;                          // floats between two pixel rows of g
    const float *g = a.g + (((size_t)n * a.S + a.start[l]) * a.B + b) * C + 4 * q;

    f32x4 acc[MT][4];
#pragma unroll
    for (int kt = 0; kt < MT; ++kt)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[kt][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 cur[4], nxt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + 16 * j + m;                            // tile j = pixels p0 + 16 j .. + 15, row m
        cur[j] = p < hw ? *(const f32x4 *)(g + (size_t)p * prow) : zero;
    }
    for (int cc = 0; cc < C / 16; ++cc) {
        if (cc + 1 < C / 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = p0 + 16 * j + m;
                nxt[j] = p < hw ? *(const f32x4 *)(g + (size_t)p * prow + 16 * (cc + 1)) : zero;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float *wr = wl + (16 * cc + 4 * q + r) * MP + m;    // reduction index of this step: c = 16 cc + 4 q + r
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) {
                const float bv = wr[kt * 16];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[kt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[j][r], bv, acc[kt][j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    // D[row = pixel 4 q + r of tile j][col = channel 16 kt + m]
    float *dx = a.dfeat[l] + (size_t)bn * M * hw;
    const bool vec = (hw & 3) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + 16 * j + 4 * q;
        if (p >= hw) continue;
#pragma unroll
        for (int kt = 0; kt < MT; ++kt) {
            float *o = dx + (size_t)(16 * kt + m) * hw + p;
            if (vec) {
                *(f32x4 *)o = acc[kt][j];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (p + r < hw) o[r] = acc[kt][j][r];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int CT2, int MT2>   // C = 32 CT2, M = 32 MT2: every wave owns CT2 x MT2 tiles of the 2 x 2 split
__global__ __launch_bounds__(256) void camera_se_wgrad_kernel(CamSeArgs a) {
    constexpr int C = 32 * CT2, M = 32 * MT2, GP = C + 16, XP = 68;
    extern __shared__ float sm[];
    float *gs = sm;                    // [64 pixels][C + 16]
    float *xs = sm + 64 * GP;          // [M][68]
    const int chunk = blockIdx.x, l = cs_level_of(a, chunk);
    const int n = blockIdx.y, b = blockIdx.z, bn = b * a.N + n;
    const int hw = a.hw[l];
    const int pc0 = (chunk - a.tile0[l]) * CS_CHUNK, pc1 = min(hw, pc0 + CS_CHUNK);
    const bool vec = (hw & 3) == 0;
    const float *x = a.feat[l] + (size_t)bn * M * hw;
    const size_t prow = (size_t)a.B * C;
    const float *g = a.g + (((size_t)n * a.S + a.start[l]) * a.B + b) * C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int c_base = (wave & 1) * (C / 2), k_base = (wave >> 1) * (M / 2);

    f32x4 acc[CT2][MT2];
#pragma unroll
    for (int ct = 0; ct < CT2; ++ct)
#pragma unroll
        for (int kt = 0; kt < MT2; ++kt) acc[ct][kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float colsum = 0.0f;

    for (int p0 = pc0; p0 < pc1; p0 += 64) {
        for (int e = threadIdx.x; e < 64 * (C / 4); e += 256) {
            const int p = e / (C / 4), c4 = e - p * (C / 4);
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (p0 + p < hw) v = *(const f32x4 *)(g + (size_t)(p0 + p) * prow + 4 * c4);
            *(f32x4 *)(gs + p * GP + 4 * c4) = v;
        }
        for (int e = threadIdx.x; e < M * 16; e += 256) {
            const int k = e >> 4, p4 = e & 15;
            *(f32x4 *)(xs + k * XP + 4 * p4) = cs_load_px4(x + (size_t)k * hw, p0 + 4 * p4, hw, vec);
        }
        __syncthreads();
        if ((int)threadIdx.x < C) {
            float s = 0.0f;
            for (int p = 0; p < 64; ++p) s += gs[p * GP + threadIdx.x];     // rows past the map are zero
            colsum += s;
        }
#pragma unroll 2
        for (int s = 0; s < 16; ++s) {                            // four pixels per MFMA: 4 s + q
            float av[CT2], bv[MT2];
#pragma unroll
            for (int ct = 0; ct < CT2; ++ct) av[ct] = gs[(4 * s + q) * GP + c_base + 16 * ct + m];
#pragma unroll
            for (int kt = 0; kt < MT2; ++kt) bv[kt] = xs[(k_base + 16 * kt + m) * XP + 4 * s + q];
#pragma unroll
            for (int ct = 0; ct < CT2; ++ct)
#pragma unroll
                for (int kt = 0; kt < MT2; ++kt)
                    acc[ct][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[kt], acc[ct][kt], 0, 0, 0);
        }
        __syncthreads();
    }
    const size_t slot = (size_t)bn * a.tile0[a.L] + chunk;
    float *pw = a.part_w + slot * C * M;
#pragma unroll
    for (int ct = 0; ct < CT2; ++ct)
#pragma unroll
        for (int kt = 0; kt < MT2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pw[(size_t)(c_base + 16 * ct + 4 * q + r) * M + k_base + 16 * kt + m] = acc[ct][kt][r];
    if ((int)threadIdx.x < C) a.part_c[slot * C + threadIdx.x] = colsum;
}

// chunk partials -> dWc (B*N, C, M) and colsum (L, N, C), chunks in ascending order (batch outermost for colsum)
__global__ __launch_bounds__(256) void camera_se_reduce_kernel(CamSeArgs a, float *__restrict__ dwc, float *__restrict__ colsum) {
    const int chunks = a.tile0[a.L], CM = a.C * a.M, BN = a.B * a.N;
    if ((int)blockIdx.y < BN) {
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= CM) return;
        const float *p = a.part_w + (size_t)blockIdx.y * chunks * CM + e;
        float s = 0.0f;
        for (int t = 0; t < chunks; ++t) s += p[(size_t)t * CM];
        dwc[(size_t)blockIdx.y * CM + e] = s;
        return;
    }
    for (int e = blockIdx.x * 256 + threadIdx.x; e < a.L * a.N * a.C; e += gridDim.x * 256) {
        const int c = e % a.C, ln = e / a.C, n = ln % a.N, l = ln / a.N;
        float s = 0.0f;
        for (int b = 0; b < a.B; ++b)
            for (int t = a.tile0[l]; t < a.tile0[l + 1]; ++t) s += a.part_c[((size_t)(b * a.N + n) * chunks + t) * a.C + c];
        colsum[e] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
bool cs_shape_ok(int B, int N, int C, int M, int L) {
    // grid.y / grid.z carry the camera and the batch; the reduce kernel's grid.y carries B * N + 1
    if (B < 1 || N < 1 || B >= 65536 || N >= 65536 || (long long)B * N >= 65535 || L < 1 || L > CS_MAX_LEVELS) return false;
    if (C != 32 && C != 64 && C != 96 && C != 128) return false;
    return (M == C || M == 2 * C) && M <= 192;
}

// sizes, level starts and tiles of `per` pixels; false: a bad level or a problem beyond 32-bit indexing
bool cs_plan(CamSeArgs &a, const int32_t *host_hw, int L, int B, int N, int C, int M, int per) {
    long long S = 0, tiles = 0;
    for (int l = 0; l < L; ++l) {
        if (host_hw[l] < 1) return false;
        a.hw[l] = host_hw[l]; a.start[l] = (int)S; a.tile0[l] = (int)tiles;
        S += host_hw[l];
        tiles += (host_hw[l] + per - 1) / per;
        if (S >= (1LL << 31)) return false;
    }
    for (int l = L; l < CS_MAX_LEVELS; ++l) { a.hw[l] = 0; a.start[l] = 0; a.feat[l] = nullptr; a.dfeat[l] = nullptr; }
    a.tile0[L] = (int)tiles;
    if (S * B * N * (C > M ? C : M) >= (1LL << 40) || tiles >= 65536LL * 16) return false;
    a.L = L; a.B = B; a.N = N; a.C = C; a.M = M; a.S = (int)S;
    return true;
}

bool cs_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <typename K>
void cs_allow_lds(K kernel, size_t bytes) {
    if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

extern "C" int selfocc_camera_se_supported(int32_t B, int32_t N, int32_t C, int32_t M, int32_t n_levels) {
    return cs_shape_ok(B, N, C, M, n_levels) ? 1 : 0;
}

extern "C" size_t selfocc_camera_se_flatten_bwd_workspace(const int32_t *host_hw, int32_t n_levels, int32_t B, int32_t N,
                                                          int32_t C, int32_t M) {
    CamSeArgs a;
    if (host_hw == nullptr || !cs_shape_ok(B, N, C, M, n_levels) || !cs_plan(a, host_hw, n_levels, B, N, C, M, CS_CHUNK)) return 0;
    return (size_t)B * N * a.tile0[n_levels] * ((size_t)C * M + C) * sizeof(float);
}

extern "C" int selfocc_camera_se_flatten_fwd(const float *const *feats, const int32_t *host_hw, int32_t n_levels, int32_t B,
                                             int32_t N, int32_t C, int32_t M, const float *gate, const float *w,
                                             const float *bias, const float *cams_embeds, const float *level_embeds, float *out,
                                             void *stream) {
    SO_REQUIRE(cs_shape_ok(B, N, C, M, n_levels), "camera_se_flatten_fwd: unsupported shape (B %d, N %d, C %d, M %d, %d levels; "
               "C in {32, 64, 96, 128}, M = C or 2 C <= 192, 1 .. 8 levels)", B, N, C, M, n_levels);
    SO_REQUIRE(feats && host_hw && gate && w && bias && cams_embeds && level_embeds && out, "camera_se_flatten_fwd: NULL pointer");
    CamSeArgs a = {};
    for (int l = 0; l < n_levels; ++l) {
        SO_REQUIRE(feats[l] != nullptr && host_hw[l] >= 1, "camera_se_flatten_fwd: level %d: NULL map or no pixels", l);
        SO_REQUIRE(cs_aligned16(feats[l]), "camera_se_flatten_fwd: level %d: map not 16-byte aligned", l);
        a.feat[l] = feats[l];
    }
    SO_REQUIRE(cs_aligned16(out), "camera_se_flatten_fwd: out not 16-byte aligned");
    SO_REQUIRE(cs_plan(a, host_hw, n_levels, B, N, C, M, CS_TILE), "camera_se_flatten_fwd: problem too large");
    for (int l = 0; l < n_levels; ++l) a.feat[l] = feats[l];
    a.gate = gate; a.w = w; a.bias = bias; a.cams = cams_embeds; a.lvls = level_embeds; a.out = out;
    const size_t shm = (size_t)C * (M + 4) * sizeof(float);
    const dim3 grid((unsigned)a.tile0[n_levels], (unsigned)N, (unsigned)B);
#define SO_CS_FWD(CT_)                                                                            \
    do {                                                                                          \
        cs_allow_lds(camera_se_fwd_kernel<CT_>, shm);                                             \
        hipLaunchKernelGGL((camera_se_fwd_kernel<CT_>), grid, dim3(256), shm, (hipStream_t)stream, a); \
    } while (0)
    switch (C / 16) {
        case 2: SO_CS_FWD(2); break;
        case 4: SO_CS_FWD(4); break;
        case 6: SO_CS_FWD(6); break;
        default: SO_CS_FWD(8); break;
    }
#undef SO_CS_FWD
    return so_launch_status();
}

extern "C" int selfocc_camera_se_flatten_bwd(const float *g, const float *const *feats, const int32_t *host_hw, int32_t n_levels,
                                             int32_t B, int32_t N, int32_t C, int32_t M, const float *gate, const float *w,
                                             float *const *d_feats, float *dwc, float *colsum, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    SO_REQUIRE(cs_shape_ok(B, N, C, M, n_levels), "camera_se_flatten_bwd: unsupported shape (B %d, N %d, C %d, M %d, %d levels; "
               "C in {32, 64, 96, 128}, M = C or 2 C <= 192, 1 .. 8 levels)", B, N, C, M, n_levels);
    SO_REQUIRE(g && feats && host_hw && gate && w && dwc && colsum, "camera_se_flatten_bwd: NULL pointer");
    SO_REQUIRE(cs_aligned16(g), "camera_se_flatten_bwd: g not 16-byte aligned");
    CamSeArgs a = {};
    bool any_dx = false;
    for (int l = 0; l < n_levels; ++l) {
        SO_REQUIRE(feats[l] != nullptr && host_hw[l] >= 1, "camera_se_flatten_bwd: level %d: NULL map or no pixels", l);
        float *d = d_feats ? d_feats[l] : nullptr;
        SO_REQUIRE(cs_aligned16(feats[l]) && cs_aligned16(d), "camera_se_flatten_bwd: level %d: map or gradient not 16-byte aligned", l);
        any_dx = any_dx || d != nullptr;
    }
    SO_REQUIRE(cs_plan(a, host_hw, n_levels, B, N, C, M, CS_CHUNK), "camera_se_flatten_bwd: problem too large");
    const size_t need = (size_t)B * N * a.tile0[n_levels] * ((size_t)C * M + C) * sizeof(float);
    SO_REQUIRE(workspace != nullptr && cs_aligned16(workspace) && workspace_bytes >= need,
               "camera_se_flatten_bwd: workspace NULL, unaligned or too small (%zu bytes, need %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < n_levels; ++l) { a.feat[l] = feats[l]; a.dfeat[l] = d_feats ? d_feats[l] : nullptr; }
    a.gate = gate; a.w = w; a.g = g;
    a.part_w = (float *)workspace;
    a.part_c = a.part_w + (size_t)B * N * a.tile0[n_levels] * C * M;

    // 1. dWc / colsum: chunk partials, then the fixed-order sum
    {
        const size_t shm = ((size_t)64 * (C + 16) + (size_t)M * 68) * sizeof(float);
        const dim3 grid((unsigned)a.tile0[n_levels], (unsigned)N, (unsigned)B);
#define SO_CS_WGRAD(CT2_, MT2_)                                                                             \
    do {                                                                                                    \
        cs_allow_lds(camera_se_wgrad_kernel<CT2_, MT2_>, shm);                                              \
        hipLaunchKernelGGL((camera_se_wgrad_kernel<CT2_, MT2_>), grid, dim3(256), shm, st, a);              \
    } while (0)
        const bool wide = M == 2 * C;
        switch (C / 32) {
            case 1: if (wide) SO_CS_WGRAD(1, 2); else SO_CS_WGRAD(1, 1); break;
            case 2: if (wide) SO_CS_WGRAD(2, 4); else SO_CS_WGRAD(2, 2); break;
            case 3: if (wide) SO_CS_WGRAD(3, 6); else SO_CS_WGRAD(3, 3); break;
            default: SO_CS_WGRAD(4, 4); break;
        }
#undef SO_CS_WGRAD
        int rc = so_launch_status();
        if (rc != 0) return rc;
        hipLaunchKernelGGL(camera_se_reduce_kernel, dim3((unsigned)((C * M + 255) / 256), (unsigned)(B * N + 1)), dim3(256), 0, st,
                           a, dwc, colsum);
        rc = so_launch_status();
        if (rc != 0) return rc;
    }
    // 2. the map gradients (levels whose pointer is NULL are skipped)
    if (any_dx) {
        CamSeArgs d = a;
        if (!cs_plan(d, host_hw, n_levels, B, N, C, M, CS_TILE)) return -1;      // same sizes: cannot fail after the plan above
        for (int l = 0; l < n_levels; ++l) { d.feat[l] = feats[l]; d.dfeat[l] = d_feats[l]; }
        const size_t shm = (size_t)C * (M + 4) * sizeof(float);
        const dim3 grid((unsigned)d.tile0[n_levels], (unsigned)N, (unsigned)B);
#define SO_CS_DGRAD(MT_)                                                                            \
    do {                                                                                            \
        cs_allow_lds(camera_se_dgrad_kernel<MT_>, shm);                                             \
        hipLaunchKernelGGL((camera_se_dgrad_kernel<MT_>), grid, dim3(256), shm, st, d);             \
    } while (0)
        switch (M / 16) {
            case 2: SO_CS_DGRAD(2); break;
            case 4: SO_CS_DGRAD(4); break;
            case 6: SO_CS_DGRAD(6); break;
            case 8: SO_CS_DGRAD(8); break;
            default: SO_CS_DGRAD(12); break;
        }
#undef SO_CS_DGRAD
        return so_launch_status();
    }
    return 0;
}
