// render_bwd_brick_body.h — the body of rb_brick_kernel / rb_brick_sh_kernel (render_bwd.hip), included once per kernel
// template (no include guard).  The including kernel provides its arguments (RbBin b, g_sdf_vol, g_feat_vol, g_inv_s, H, W, D)
// and the compile-time constants NF, NT, NB; see render_bwd_body.h for why the sharing is textual.
    constexpr int RECF = RbRec<NF, NB>::RECF, NCH = RbRec<NF, NB>::NCH, RW = RbRec<NF, NB>::RW, LPG = RbRec<NF, NB>::LPG;
    constexpr int NG = NT / LPG, U = 4;
    extern __shared__ double tile[];   // [kTileVox][RW]
    if (blockIdx.x == 0 && g_inv_s) {   // the ray kernel's partial sums of d L / d inv_s: one atomic per wave of this block
        float t = 0.0f;
        for (int k = threadIdx.x; k < kInvsSlots; k += NT) t += b.invs_part[k];
        t = so_wave_sum_32to1(t);
        if ((threadIdx.x & 63) == 0) unsafeAtomicAdd(g_inv_s, t);
    }
    if ((int)blockIdx.x >= b.n_items[0]) return;
    const int4 it = b.items[blockIdx.x];
    const int bd = it.x % b.nbd, bw = (it.x / b.nbd) % b.nbw, bh = it.x / (b.nbd * b.nbw);
    const int oh = bh * kBH, ow = bw * kBW, od = bd * kBD;
    for (int k = threadIdx.x; k < kTileVox * RW; k += NT) tile[k] = 0.0;
    __syncthreads();
    const int grp = threadIdx.x / LPG, sub = threadIdx.x % LPG;
    // lanes [0, NCH) of a group: one feature channel each, all 8 corners; lanes [RECF - 8, RECF): ONE corner each of the
    // sdf column (its coefficient has four terms: spreading the corners over the 8 otherwise idle tail lanes keeps the
    // per-corner loop of the feature lanes at one multiply)
    const bool sdf_lane = sub >= LPG - 8;
    const int mk = sub - (LPG - 8), mkd = mk & 1, mkw = (mk >> 1) & 1, mkh = (mk >> 2) & 1;
    const int moff = ((mkh * kTW + mkw) * kTD + mkd) * RW + NCH;
    // Group g walks the CONTIGUOUS slice [y + g * per, ...) of the item, U records at a time.  The records of an item are
    // in ray order (a run of consecutive samples of one ray takes consecutive slots), and consecutive samples of a ray share
    // their cell 2 - 6 times at the shipped step / voxel ratio: the group sums such a run in registers and issues its LDS
    // atomics once per run (the kernel sits on the ds_add_f64 issue rate: ~15 clocks per instruction, 35 M of them per launch
    // before this).  SELFOCC_RB_DBG & 4: no merging (every sample flushes).
    const int per = (it.z - it.y + NG - 1) / NG;
    const int gb = it.y + grp * per, ge = min(it.z, gb + per);
    const bool merge = !(b.dbg & 4);
    int cur = -1;                 // packed cell of the open run
    float acc[8];                 // feature lanes: the run's sum per corner; sdf lanes: acc[0] = the own corner's sum
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
    float sacc_sh = 0.0f;         // NB > 0: a lane can own a channel AND an sdf corner, so the sdf sum has its own register
    float &sacc = *[&]() { if constexpr (NB > 0) return &sacc_sh; else return &acc[0]; }();
    auto flush = [&]() {
        const int h0 = (cur >> 20) - 2, w0 = ((cur >> 10) & 1023) - 2, d0 = (cur & 1023) - 2;
        const int lh = h0 - oh, lw = w0 - ow, ld = d0 - od;
        // a corner counts when it is inside the volume AND inside this brick's tile (the second never fails: the
        // counting pass and the ray kernel derive the cell with the same code; it only keeps a mismatch inside the tile)
        const bool okh[2] = {((unsigned)h0 < (unsigned)H) && ((unsigned)lh < (unsigned)kTH),
                             ((unsigned)(h0 + 1) < (unsigned)H) && ((unsigned)(lh + 1) < (unsigned)kTH)};
        const bool okw[2] = {((unsigned)w0 < (unsigned)W) && ((unsigned)lw < (unsigned)kTW),
                             ((unsigned)(w0 + 1) < (unsigned)W) && ((unsigned)(lw + 1) < (unsigned)kTW)};
        const bool okd[2] = {((unsigned)d0 < (unsigned)D) && ((unsigned)ld < (unsigned)kTD),
                             ((unsigned)(d0 + 1) < (unsigned)D) && ((unsigned)(ld + 1) < (unsigned)kTD)};
        double *t0 = tile + ((lh * kTW + lw) * kTD + ld) * RW;
        if constexpr (NCH > 0) {
            if (sub < NCH) {
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int kd = kk & 1, kw = (kk >> 1) & 1, kh = kk >> 2;
                    if (okd[kd] && okw[kw] && okh[kh] && acc[kk] != 0.0f)
                        __hip_atomic_fetch_add(t0 + ((kh * kTW + kw) * kTD + kd) * RW + sub, (double)acc[kk], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        if (sdf_lane && okd[mkd] && okw[mkw] && okh[mkh] && sacc != 0.0f)
            __hip_atomic_fetch_add(t0 + moff, (double)sacc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
        sacc = 0.0f;
    };
    for (int i0 = gb; i0 < ge; i0 += U) {
        bool ok[U];
        float v[U];
        float4 ta[U], tb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            ok[u] = i < ge;
            if (ok[u]) {
                const float *r = b.rec + (size_t)i * RECF;
                if constexpr (NB > 0) v[u] = (sub < NCH) ? r[sub / NB] * rb_sh_one(sub % NB, r[3], r[4], r[5]) : 0.0f;
                else v[u] = (b.dbg & 16) ? 0.0f : r[sub];
                ta[u] = *(const float4 *)(r + (RECF - 8));
                tb[u] = *(const float4 *)(r + (RECF - 4));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u] || (b.dbg & 1)) continue;
            const int pack = __float_as_int(ta[u].y);
            if (pack != cur || !merge) {
                if (cur >= 0) flush();
                cur = pack;
            }
            const float fh[2] = {1.0f - ta[u].z, ta[u].z}, fw[2] = {1.0f - ta[u].w, ta[u].w}, fd[2] = {1.0f - tb[u].x, tb[u].x};
            if constexpr (NCH > 0) {
                if (sub < NCH) {
                    const float fdfw[2][2] = {{fd[0] * fw[0], fd[0] * fw[1]}, {fd[1] * fw[0], fd[1] * fw[1]}};
#pragma unroll
                    for (int kk = 0; kk < 8; ++kk) acc[kk] = fmaf(fdfw[kk & 1][(kk >> 1) & 1] * fh[kk >> 2], v[u], acc[kk]);
                }
            }
            if (sdf_lane) {
                // d L / d sdf corner = ds W_k + qz dW_k/dd + qx dW_k/dw + qy dW_k/dh
                const float fds = fd[mkd], fws = fw[mkw], fhs = fh[mkh];
                const float Wk = (fds * fws) * fhs;
                const float dWd = (mkd ? 1.0f : -1.0f) * (fws * fhs);
                const float dWw = (mkw ? 1.0f : -1.0f) * (fds * fhs);
                const float dWh = (mkh ? 1.0f : -1.0f) * (fds * fws);
                sacc += fmaf(Wk, ta[u].x, fmaf(dWd, tb[u].w, fmaf(dWw, tb[u].y, dWh * tb[u].z)));
            }
        }
    }
    if (cur >= 0) flush();
    __syncthreads();
    if (b.dbg & 2) return;
    // flush.  Feature rows: RECF lanes per voxel row, consecutive groups = consecutive d (contiguous rows in HBM).
    if constexpr (NCH > 0) {
        if (g_feat_vol) {
            for (int r = grp; r < kTileVox; r += NG) {
                const int rd = r % kTD, rw = (r / kTD) % kTW, rh = r / (kTD * kTW);
                const int h = oh + rh, w = ow + rw, d = od + rd;
                if (h < H && w < W && d < D && sub < NCH) {
                    const float val = (float)tile[r * RW + sub];
                    if (val != 0.0f) unsafeAtomicAdd(g_feat_vol + ((size_t)(h * W + w) * D + d) * NF + sub, val);
                }
            }
        }
    }
    if (g_sdf_vol) {   // the sdf column: consecutive lanes = consecutive d
        for (int r = threadIdx.x; r < kTileVox; r += NT) {
            const int rd = r % kTD, rw = (r / kTD) % kTW, rh = r / (kTD * kTW);
            const int h = oh + rh, w = ow + rw, d = od + rd;
            if (h < H && w < W && d < D) {
                const float val = (float)tile[r * RW + NCH];
                if (val != 0.0f) unsafeAtomicAdd(g_sdf_vol + (size_t)(h * W + w) * D + d, val);
            }
        }
    }
