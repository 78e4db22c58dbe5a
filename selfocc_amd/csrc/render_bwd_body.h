// render_bwd_body.h — the body of the ray kernels of render_bwd.hip, included once per kernel template (no include guard).
// The including kernel provides its by-value arguments `so_render_bwd_args ba`, `RbBin bin` and the compile-time constants
// NF, BF16, M, WPR, BIN, MK, NB, MASKED (SO_SEM_ON, so_device.h: d L / d feature stays an exact 0 in a pad channel, and neither
// scatter adds a zero).  Textual sharing instead of a common device function: the shipped kernels must stay the code
// they are, and a body that takes the arguments by reference compiles to different registers.
    static_assert(WPR == 1 || WPR == 4, "waves per ray");
    constexpr int RECF = RbRec<NF, NB>::RECF, NCH = RbRec<NF, NB>::NCH;
    const so_render_args &a = ba.fwd;
    constexpr int NSEM = (NB == 0 && NF > 4) ? NF - 3 : 0;
    const int nsem = MASKED ? a.n_sem : NSEM;   // the launch's class count (uniform)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray = WPR == 1 ? blockIdx.x * 4 + wave : blockIdx.x;
    const int wstep = WPR == 1 ? 0 : wave;   // position of this wave inside a step group
    __shared__ float xch[4][8];
    // sum of v[0..N) over the waves that share the ray (block-uniform control flow when WPR == 4)
    auto ray_sum = [&](auto &v, auto nconst) {
        constexpr int N = decltype(nconst)::value;
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = so_wave_sum_32to1(v[k]);
        if constexpr (WPR > 1) {
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < N; ++k) xch[wave][k] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] = (xch[0][k] + xch[1][k]) + (xch[2][k] + xch[3][k]);
            __syncthreads();
        }
    };
    // per-wave transpose buffer of the feature-gradient scatter (phase B); odd record stride
    __shared__ __attribute__((aligned(16))) float lds_rec[BIN ? 4 : 4 * 64 * (NF > 0 ? (NF + 9 + (((NF + 9) & 1) ? 0 : 1)) : 9)];
    if (ray >= a.n_rays) return;  // wave-uniform (block-uniform when the waves share a ray)
    const int H = a.map.h.tot_len, W = a.map.w.tot_len, D = a.map.d.tot_len;
    const int S = a.n_samples;
    const RayGeom g = so_ray_of(a, ray);
    float Y[NB > 0 ? NB : 1];
    if constexpr (NB > 0) so_sh_basis<NB>(g.dx, g.dy, g.dz, Y);

    float tn, tf;
    so_collide(a, g, tn, tf);

    // ---- phase A: per-sample forward state -------------------------------------------------
    so_cell cell[M];
    float alpha[M], fj[M], tmid[M], delta[M], Pc[M], Nc[M], sdfv[M], halfv[M];
    bool live[M], cneg[M], unclipped[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int i = (j * WPR + wstep) * 64 + lane;   // a step covers 64 CONSECUTIVE samples (one per lane)
        live[j] = i < S;
        const int ic = live[j] ? i : S - 1;
        const float t0 = so_edge(a, ray, ic, tn, tf), t1 = so_edge(a, ray, ic + 1, tn, tf);
        delta[j] = t1 - t0;
        tmid[j] = (t0 + t1) / 2.0f;
        cell[j] = sample_cell<MK>(a, g, t0, t1);
        float v[8], wk[8];
        so_gather_sdf(a.sdf_vol, H, W, D, cell[j], v);
        sdfv[j] = so_trilerp_sdf(cell[j], v, wk);
        float gx, gy, gz;
        so_trilerp_grad(cell[j], v, gx, gy, gz);
        const float cosv = (g.dx * gx + g.dy * gy) + g.dz * gz;
        cneg[j] = cosv < 0.0f;
        halfv[j] = (fminf(cosv, 0.0f) * delta[j]) * 0.5f;
        Pc[j] = so_sigmoid((sdfv[j] - halfv[j]) * so_inv_s(a));
        Nc[j] = so_sigmoid((sdfv[j] + halfv[j]) * so_inv_s(a));
        const float araw = ((Pc[j] - Nc[j]) + 1e-5f) / (Pc[j] + 1e-5f);
        unclipped[j] = (araw > 0.0f) && (araw < 1.0f);
        alpha[j] = live[j] ? fminf(fmaxf(araw, 0.0f), 1.0f) : 0.0f;
        fj[j] = live[j] ? (1.0f - alpha[j]) + 1e-7f : 1.0f;
    }
    // BIN: the slots of this wave's samples in the brick-ordered record array: one returning atomic per run of lanes
    // with one (brick, shard) counter, issued here so that its latency hides behind phase B's gathers
    int slot_base[M], slot_head[M];
    if constexpr (BIN) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            int key = -1;
            if (live[j]) key = rb_key(bin, cell[j], H, W, D) * kShards + rb_shard((long long)ray * S + ((j * WPR + wstep) * 64 + lane));
            const int run = rb_run(key, lane, slot_head[j]);
            slot_base[j] = 0;
            if (run > 0 && key >= 0) slot_base[j] = atomicAdd(bin.cursor + key, run);
        }
    }
    // transmittance: exclusive prefix product over the samples in ray order = per step an exclusive scan
    // over the lanes (Hillis-Steele on shuffles) times the product of all earlier steps
    float T[M], w[M];
    float acc_l = 0.0f, dsum_l = 0.0f, carry = 1.0f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        float incl = fj[j];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float o = __shfl_up(incl, d, 64);
            if (lane >= d) incl *= o;
        }
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float tot = __shfl(incl, 63, 64);
        float before = carry;                     // product over all earlier steps
        if constexpr (WPR > 1) {
            if (lane == 0) xch[wave][0] = tot;
            __syncthreads();
#pragma unroll
            for (int ww = 0; ww < WPR; ++ww) {
                if (ww < wave) before *= xch[ww][0];
                carry *= xch[ww][0];
            }
            __syncthreads();
        } else {
            carry *= tot;
        }
        T[j] = before * excl;
        w[j] = alpha[j] * T[j];
        acc_l += w[j];
        dsum_l = fmaf(w[j], tmid[j], dsum_l);
    }
    float ad[2] = {acc_l, dsum_l};
    ray_sum(ad, std::integral_constant<int, 2>{});
    const float acc = ad[0], dsum = ad[1];
    const float inv_ae = 1.0f / (acc + 1e-10f);
    const float depth_raw = dsum * inv_ae;
    const float ddn = (a.flags & SO_FLAG_DEPTH_DIV_NORM) ? 1.0f / g.dn : 1.0f;

    // upstream per-ray gradients (wave-uniform)
    const float g_depth = ba.g_depth ? ba.g_depth[ray] * ddn : 0.0f;
    float g_accum = ba.g_acc ? ba.g_acc[ray] : 0.0f;
    float g_rgb[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (NF > 0) {
        if (ba.g_rgb) {
            // rgb_k = clamp(sum_i w_i col_ik + bg_k (1 - acc)): the clamp and the background need the
            // forward value; recompute sum_i w_i col_ik below, so first pass: gather colours
        }
    }

    // ---- phase B: colour / semantics: Gw contributions + feature-volume scatter ---------------
    float Gw[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const size_t so = (size_t)ray * S + ((j * WPR + wstep) * 64 + lane);
        Gw[j] = (ba.g_weights && live[j]) ? ba.g_weights[so] : 0.0f;
        Gw[j] += g_depth * (tmid[j] - depth_raw) * inv_ae;
    }
    if constexpr (NF > 0) {
        float col[M][3];
        float rgb_l[3] = {0.0f, 0.0f, 0.0f};
        // pass 1: ONE gather of the 8 corners' feature rows per sample (round 6: the colours used to be gathered here and the whole
        // rows again in pass 2 — the corner gathers are 475 of the ray kernel's 994 us, profiles/r6_c_render_bwd_gather_bound.txt):
        // interpolated colour (kept: forward rgb for the clamp mask) and, with semantics, the sample's softmax probabilities (kept)
        // (the probabilities wait in lane-private LDS columns [j][k][thread], not in 21 registers: kept live across the ray
        // reduction they pushed the 24-channel kernel from 213 to 256 + 24 registers — one wave per SIMD — or into scratch)
        __shared__ float pk_s[(NSEM > 0 ? NSEM : 1) * M * 256];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            float f3[3] = {0.0f, 0.0f, 0.0f};
            float lg[NSEM > 0 ? NSEM : 1];
#pragma unroll
            for (int k = 0; k < (NSEM > 0 ? NSEM : 1); ++k) lg[k] = 0.0f;
            const float fd[2] = {cell[j].fd0, cell[j].fd1}, fw[2] = {cell[j].fw0, cell[j].fw1}, fh[2] = {cell[j].fh0, cell[j].fh1};
            if constexpr (NB > 0) {   // the forward's fold: f3 = the raw (pre-activation) colour
                float wk[8];
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) wk[kk] = (fd[kk & 1] * fw[(kk >> 1) & 1]) * fh[kk >> 2];
                so_sh_gather<NB>(a.feat_vol, H, W, D, cell[j], wk, Y, f3);
            }
#pragma unroll
            for (int kk = 0; kk < (NB > 0 ? 0 : 8); ++kk) {
                const int h = cell[j].h0 + (kk >> 2), ww = cell[j].w0 + ((kk >> 1) & 1), d = cell[j].d0 + (kk & 1);
                const bool in = (h >= 0) && (h < H) && (ww >= 0) && (ww < W) && (d >= 0) && (d < D);
                const int hc = min(max(h, 0), H - 1), wc = min(max(ww, 0), W - 1), dc = min(max(d, 0), D - 1);
                const float wgt = in ? (fd[kk & 1] * fw[(kk >> 1) & 1]) * fh[kk >> 2] : 0.0f;
                const size_t vox = ((size_t)hc * W + wc) * D + dc;
                if constexpr (NSEM > 0) {
                    float f[NF];
#ifdef SO_RB_NO_GATHER      // A/B build (scripts/build_variant.sh nogather render_bwd.hip -DSO_RB_NO_GATHER; timing only): no corner gathers —
#pragma unroll              // the bound of "keep the forward's interpolated features".  (As a RUN-TIME switch the branch cost the shipped
                    for (int k = 0; k < NF; ++k) f[k] = 0.01f * k;      // kernel 45 %: 1 040 -> 1 502 us.)
#else
                    load_feat<NF, BF16>(a.feat_vol, vox, f);
#endif
#pragma unroll
                    for (int k = 0; k < 3; ++k) f3[k] = fmaf(f[k], wgt, f3[k]);
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) lg[k] = fmaf(f[3 + k], wgt, lg[k]);
                } else {
                    float c3[3];
#ifdef SO_RB_NO_GATHER
                    c3[0] = 0.1f; c3[1] = 0.2f; c3[2] = 0.3f;
#else
                    if constexpr (!BF16) {
                        const float *p = (const float *)a.feat_vol + vox * NF;
                        c3[0] = p[0]; c3[1] = p[1]; c3[2] = p[2];
                    } else {
                        const uint16_t *p = (const uint16_t *)a.feat_vol + vox * NF;
                        c3[0] = so_bf16_to_f32(p[0]); c3[1] = so_bf16_to_f32(p[1]); c3[2] = so_bf16_to_f32(p[2]);
                    }
#endif
#pragma unroll
                    for (int k = 0; k < 3; ++k) f3[k] = fmaf(c3[k], wgt, f3[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if constexpr (NB > 0) {
                    col[j][k] = f3[k];                                // pre-activation
                    rgb_l[k] = fmaf(w[j], so_sh_act(col[j][k], a.sh_act), rgb_l[k]);
                } else {
                    col[j][k] = 0.28209479177387814f * f3[k] + 0.5f;  // pre-relu
                    rgb_l[k] = fmaf(w[j], fmaxf(col[j][k], 0.0f), rgb_l[k]);
                }
            }
            if constexpr (NSEM > 0) {
                float mx = lg[0];
#pragma unroll
                for (int k = 1; k < NSEM; ++k) if (SO_SEM_ON(k)) mx = fmaxf(mx, lg[k]);
                float den = 0.0f;
#pragma unroll
                for (int k = 0; k < NSEM; ++k) {
                    if (SO_SEM_ON(k)) { lg[k] = so_expf(lg[k] - mx); den += lg[k]; }
                    else lg[k] = 0.0f;
                }
                const float iden = 1.0f / den;
#pragma unroll
                for (int k = 0; k < NSEM; ++k) pk_s[(j * NSEM + k) * 256 + threadIdx.x] = lg[k] * iden;
            }
        }
        float bgk[3] = {0.0f, 0.0f, 0.0f};
        ray_sum(rgb_l, std::integral_constant<int, 3>{});
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.bkgd_mode == SO_BKGD_CONST) bgk[k] = a.bkgd[k];
            else if (a.bkgd_mode == SO_BKGD_PER_RAY) bgk[k] = a.bkgd_rays[3 * (size_t)ray + k];
            float r = rgb_l[k];
            if (a.bkgd_mode != SO_BKGD_NONE) r = r + bgk[k] * (1.0f - acc);
            float gk = ba.g_rgb ? ba.g_rgb[3 * (size_t)ray + k] : 0.0f;
            if ((a.flags & SO_FLAG_CLAMP_RGB) && (r < 0.0f || r > 1.0f)) gk = 0.0f;
            g_rgb[k] = gk;
            if (a.bkgd_mode != SO_BKGD_NONE) g_accum -= gk * bgk[k];
        }
        float g_semr[NSEM > 0 ? NSEM : 1];
        if constexpr (NSEM > 0) {
#pragma unroll
            for (int k = 0; k < NSEM; ++k) g_semr[k] = (ba.g_sem && SO_SEM_ON(k)) ? ba.g_sem[(size_t)ray * nsem + k] : 0.0f;
        }
        // pass 2: full feature vector per sample: Gw += g_rgb . col + g_sem . p; scatter d L / d feat.
        // The scatter is TRANSPOSED through LDS: each lane parks {cell, 8 corner weights, d L / d f[NF]}
        // of its sample, then GS = 2^ceil(log2 NF) consecutive lanes own the NF contiguous channels of one
        // sample's corner, so an atomic instruction touches 64 / GS segments of NF * 4 bytes instead of 64
        // scattered dwords (the lane-per-sample form cost 112 ms per nuscenes_occ iteration).
        constexpr int GS = NF <= 4 ? 4 : (NF <= 8 ? 8 : 32);       // lanes per sample in the scatter
        constexpr int REC = NF + 9 + (((NF + 9) & 1) ? 0 : 1);     // odd stride: conflict-free columns
        float *rec = lds_rec + wave * (64 * REC);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            float df[NF];  // d L / d interpolated feature
#pragma unroll
            for (int k = 0; k < NF; ++k) df[k] = 0.0f;
            const float fd[2] = {cell[j].fd0, cell[j].fd1}, fw[2] = {cell[j].fw0, cell[j].fw1}, fh[2] = {cell[j].fh0, cell[j].fh1};
            float g_raw[3] = {0.0f, 0.0f, 0.0f};   // NB > 0: d L / d raw colour
            if (live[j]) {
                if constexpr (NB > 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        Gw[j] = fmaf(g_rgb[k], so_sh_act(col[j][k], a.sh_act), Gw[j]);
                        g_raw[k] = (g_rgb[k] * w[j]) * so_sh_dact(col[j][k], a.sh_act);
                    }
                    if constexpr (!BIN) {
#pragma unroll
                        for (int k = 0; k < 3 * NB; ++k) df[k] = g_raw[k / NB] * Y[k % NB];
                    }
                } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    Gw[j] = fmaf(g_rgb[k], fmaxf(col[j][k], 0.0f), Gw[j]);
                    df[k] = (col[j][k] > 0.0f) ? g_rgb[k] * w[j] * 0.28209479177387814f : 0.0f;
                }
                }
                if constexpr (NSEM > 0) {
                    float pk[NSEM];
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) pk[k] = pk_s[(j * NSEM + k) * 256 + threadIdx.x];
                    float gp = 0.0f;
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) gp = fmaf(g_semr[k], pk[k], gp);
                    Gw[j] += gp;
#pragma unroll
                    for (int k = 0; k < NSEM; ++k) if (SO_SEM_ON(k)) df[3 + k] = w[j] * pk[k] * (g_semr[k] - gp);  // softmax backward
                }
            }
            if constexpr (BIN) {
                const int slot = __shfl(slot_base[j], slot_head[j], 64) + (lane - slot_head[j]);
                if constexpr (NB > 0) {
                    if (live[j]) {
                        float4 *dst = (float4 *)(bin.rec + (size_t)slot * RECF);
                        dst[0] = make_float4(g_raw[0], g_raw[1], g_raw[2], g.dx);
                        dst[1] = make_float4(g.dy, g.dz, 0.0f, 0.0f);
                    }
                } else
                if (live[j] && !(bin.dbg & 8)) {   // the feature part of the sample's record, 16 bytes at a time
                    float4 *dst = (float4 *)(bin.rec + (size_t)slot * RECF);
#pragma unroll
                    for (int q = 0; q < (RECF - 8) / 4; ++q) {
                        float4 t;
                        t.x = (4 * q < NCH) ? df[(4 * q < NCH) ? 4 * q : 0] : 0.0f;
                        t.y = (4 * q + 1 < NCH) ? df[(4 * q + 1 < NCH) ? 4 * q + 1 : 0] : 0.0f;
                        t.z = (4 * q + 2 < NCH) ? df[(4 * q + 2 < NCH) ? 4 * q + 2 : 0] : 0.0f;
                        t.w = (4 * q + 3 < NCH) ? df[(4 * q + 3 < NCH) ? 4 * q + 3 : 0] : 0.0f;
                        dst[q] = t;
                    }
                }
            } else if (ba.g_feat_vol) {   // wave-uniform
                float *mine = rec + lane * REC;
                mine[0] = __int_as_float((cell[j].h0 * W + cell[j].w0) * D + cell[j].d0);
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int h = cell[j].h0 + (kk >> 2), ww = cell[j].w0 + ((kk >> 1) & 1), d = cell[j].d0 + (kk & 1);
                    const bool in = live[j] && (h >= 0) && (h < H) && (ww >= 0) && (ww < W) && (d >= 0) && (d < D);
                    mine[1 + kk] = in ? (fd[kk & 1] * fw[(kk >> 1) & 1]) * fh[kk >> 2] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < NF; ++k) mine[9 + k] = (NF == 4 && k == 3) ? 0.0f : df[k];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int sub = lane % GS, grp = lane / GS;
                // Row grp serves the samples of lanes grp * GS .. + GS - 1, which are CONSECUTIVE on the ray; a
                // run of samples inside one voxel (about two at the shipped step / voxel ratio) shares its 8
                // corners, so the row sums the run's contributions and issues one set of atomics for it.
                // (The rows of one instruction are GS samples apart: different voxels, no shared L2 line.)
                for (int t = 0; t < GS; ++t) {
                    const float *r = rec + (grp * GS + t) * REC;
                    const int base = __float_as_int(r[0]);
                    if (t > 0 && __float_as_int(r[-REC]) == base) continue;   // inside a run: already added
                    float val[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                    int tt = t;
                    const float *rr = r;
                    do {
                        const float dfc = (sub < NF) ? rr[9 + sub] : 0.0f;
#pragma unroll
                        for (int kk = 0; kk < 8; ++kk) val[kk] = fmaf(rr[1 + kk], dfc, val[kk]);
                        ++tt;
                        rr += REC;
                    } while (tt < GS && __float_as_int(rr[0]) == base);
                    if (sub < NF) {
#pragma unroll
                        for (int kk = 0; kk < 8; ++kk) {
                            if (val[kk] != 0.0f) {
                                const int vox = base + ((kk >> 2) * W + ((kk >> 1) & 1)) * D + (kk & 1);
                                unsafeAtomicAdd(ba.g_feat_vol + (size_t)vox * NF + sub, val[kk]);
                            }
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
#pragma unroll
    for (int j = 0; j < M; ++j) Gw[j] += g_accum;

    // ---- phase C: reverse affine scan  E_i = Gw_{i+1} alpha_{i+1} + f_{i+1} E_{i+1} -----------
    // Each sample is the affine map x -> Gw_i alpha_i + f_i x; E_i is the composition of the maps of all
    // later samples applied to 0.  Per step (last step first): inclusive suffix composition over the lanes,
    // then E of lane l = (maps of lanes l+1 .. 63 of this step)(E after the step).
    float Ev[M];
    float E_end = 0.0f;   // E after the last sample of the current step
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
        float SA = Gw[j] * alpha[j], SB = fj[j];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float oa = __shfl_down(SA, d, 64), ob = __shfl_down(SB, d, 64);
            if (lane + d < 64) { SA = fmaf(SB, oa, SA); SB = SB * ob; }
        }
        const float na = __shfl_down(SA, 1, 64), nb = __shfl_down(SB, 1, 64);
        const float wa = __shfl(SA, 0, 64), wb = __shfl(SB, 0, 64);   // the whole step as one map
        float E_mine = E_end;                     // E after the last sample of THIS wave's step
        if constexpr (WPR > 1) {
            if (lane == 0) { xch[wave][0] = wa; xch[wave][1] = wb; }
            __syncthreads();
#pragma unroll
            for (int ww = WPR - 1; ww >= 0; --ww) {   // later steps are applied first
                if (ww > wave) E_mine = fmaf(xch[ww][1], E_mine, xch[ww][0]);
                E_end = fmaf(xch[ww][1], E_end, xch[ww][0]);
            }
            __syncthreads();
        } else {
            E_end = fmaf(wb, E_end, wa);
        }
        Ev[j] = (lane == 63) ? E_mine : fmaf(nb, E_mine, na);
    }

    float dinv_s_l = 0.0f;
    // SDF-volume records: {cell, 8 corner coefficients} per lane, in this wave's own slab of lds_rec (the same
    // slab as its feature records: with one wave per ray the waves of a block are not in step)
    float *srec = lds_rec + wave * (64 * (NF > 0 ? (NF + 9 + (((NF + 9) & 1) ? 0 : 1)) : 9));
#pragma unroll
    for (int j = M - 1; j >= 0; --j) {
        float dalpha = T[j] * (Gw[j] - Ev[j]);
        float coefs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float r_ds = 0.0f, r_qx = 0.0f, r_qy = 0.0f, r_qz = 0.0f;   // BIN: the record's sdf coefficients
        if (live[j]) {
            if (!unclipped[j]) dalpha = 0.0f;
            const float pe = Pc[j] + 1e-5f;
            const float dP = dalpha * (Nc[j] / (pe * pe));
            const float dN = -dalpha / pe;
            const float da = dP * Pc[j] * (1.0f - Pc[j]);
            const float db = dN * Nc[j] * (1.0f - Nc[j]);
            const size_t so = (size_t)ray * S + ((j * WPR + wstep) * 64 + lane);
            float ds = (da + db) * so_inv_s(a);
            const float dh = (db - da) * so_inv_s(a);
            dinv_s_l += da * (sdfv[j] - halfv[j]) + db * (sdfv[j] + halfv[j]);
            const float dc = cneg[j] ? dh * (delta[j] * 0.5f) : 0.0f;
            float dgx = dc * g.dx, dgy = dc * g.dy, dgz = dc * g.dz;
            if (ba.g_sdf) ds += ba.g_sdf[so];
            if (ba.g_grad) { dgx += ba.g_grad[3 * so]; dgy += ba.g_grad[3 * so + 1]; dgz += ba.g_grad[3 * so + 2]; }
            if (BIN && ba.g_sdf_vol) {
                r_ds = ds; r_qx = dgx * cell[j].sw; r_qy = dgy * cell[j].sh; r_qz = dgz * cell[j].sd;
            }
            if (!BIN && ba.g_sdf_vol) {
                // sdf = sum_k W_k v_k ; grad_axis = slope_axis * sum_k dW_k/d axis * v_k
                const so_cell &c = cell[j];
                const float fd[2] = {c.fd0, c.fd1}, fw[2] = {c.fw0, c.fw1}, fh[2] = {c.fh0, c.fh1};
                const float qx = dgx * c.sw, qy = dgy * c.sh, qz = dgz * c.sd;  // metre x<->w, y<->h, z<->d
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int kd = kk & 1, kw = (kk >> 1) & 1, kh = kk >> 2;
                    const int h = c.h0 + kh, ww = c.w0 + kw, d = c.d0 + kd;
                    const bool in = (h >= 0) && (h < H) && (ww >= 0) && (ww < W) && (d >= 0) && (d < D);
                    const float Wk = (fd[kd] * fw[kw]) * fh[kh];
                    const float dWd = (kd ? 1.0f : -1.0f) * (fw[kw] * fh[kh]);
                    const float dWw = (kw ? 1.0f : -1.0f) * (fd[kd] * fh[kh]);
                    const float dWh = (kh ? 1.0f : -1.0f) * (fd[kd] * fw[kw]);
                    coefs[kk] = in ? fmaf(Wk, ds, fmaf(dWd, qz, fmaf(dWw, qx, dWh * qy))) : 0.0f;
                }
            }
        }
        if constexpr (BIN) {
            const so_cell &c = cell[j];
            const int slot = __shfl(slot_base[j], slot_head[j], 64) + (lane - slot_head[j]);
            if (live[j]) {
                // so_locate does not clamp: a sample outside the box (a ray that misses it, near_plane past the exit, an
                // aabb larger than the mapping) has h0 <= -2 or h0 >= H.  The clamp keeps such an index OUTSIDE the volume
                // (-2 and 1021 >= tot_len fail every corner test of rb_brick_kernel), as the atomic path's `in` test does.
                const int pack = ((min(max(c.h0, -2), 1021) + 2) << 20) | ((min(max(c.w0, -2), 1021) + 2) << 10) |
                                 (min(max(c.d0, -2), 1021) + 2);
                float4 *dst = (float4 *)(bin.rec + (size_t)slot * RECF + (RECF - 8));
                dst[0] = make_float4(r_ds, __int_as_float(pack), c.fh1, c.fw1);
                dst[1] = make_float4(c.fd1, r_qx, r_qy, r_qz);
            }
        } else if (ba.g_sdf_vol) {   // wave-uniform
            // Scalar per-lane atomics would be one 64-byte fabric write each (8 per sample: as much traffic as
            // the whole feature scatter).  Instead 8-lane rows (one corner per lane) walk the samples in ray
            // order and add the coefficients of a run of samples inside one voxel before one atomic per corner.
            float *mine = srec + lane * 9;
            mine[0] = __int_as_float((cell[j].h0 * W + cell[j].w0) * D + cell[j].d0);
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) mine[1 + kk] = coefs[kk];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int sub = lane & 7, grp = lane >> 3;
            const int voff = ((sub >> 2) * W + ((sub >> 1) & 1)) * D + (sub & 1);
            for (int t = 0; t < 8; ++t) {
                const float *r = srec + (grp * 8 + t) * 9;
                const int base = __float_as_int(r[0]);
                if (t > 0 && __float_as_int(r[-9]) == base) continue;   // inside a run: already added
                float val = 0.0f;
                int tt = t;
                const float *rr = r;
                do {
                    val += rr[1 + sub];
                    ++tt;
                    rr += 9;
                } while (tt < 8 && __float_as_int(rr[0]) == base);
                // a coefficient is non-zero only for a corner inside the volume, so base + voff is a valid voxel
                if (val != 0.0f) unsafeAtomicAdd(ba.g_sdf_vol + (base + voff), val);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (ba.g_inv_s) {
        const float t = so_wave_sum_32to1(dinv_s_l);
        // BIN: kInvsSlots partial sums (rb_brick_kernel's first block adds them up) instead of one atomic per wave on ONE word
        if (lane == 0) unsafeAtomicAdd(BIN ? bin.invs_part + (blockIdx.x & (kInvsSlots - 1)) : ba.g_inv_s, t);
    }
