// render_upsample.hip — NeuS hierarchical up-sampling (selfocc_render_upsample): the coarse-to-fine sampler that places new
// samples where the SDF crosses zero.  A declared restatement of upstream sdfstudio's NeuSSampler + nerfstudio's PDFSampler
// (the fork that implements it for the reference is not on disk).  The definition, per ray:
//
//   inputs: the collider's tnear / tfar (so_collide); S0 = n_samples, M = n_importance, K = n_steps, m = M / K (integer
//           division); base_variance; one number r_k in [0, 1) per step (0.5 when no u_rand is given).
//   state:  normalised edges b[0..n], non-decreasing, with n samples.  Start: n = S0 and b[j] = so_edge_unit(j), i.e. what
//           so_edge computes before its last line.  Metric position of an edge, everywhere: t = b * tfar + (1 - b) * tnear.
//   for step k = 0 .. K - 1, with s = base_variance * 2^k:
//     1. f_i = trilinear SDF at o + d * t_i, i = 0 .. n - 1, through the mapping, with the arithmetic of field_query; always
//        the sample start, whatever sample_pos says
//     2. for i = 0 .. n - 2:  delta_i = t_{i+1} - t_i;  mid = (f_i + f_{i+1}) * 0.5;  cos_i = (f_{i+1} - f_i) / (delta_i + 1e-5);
//        c_i = clip(min(cos_{i-1}, cos_i), -1e3, 0), with cos_{-1} = 0;  e- = mid - c_i delta_i * 0.5,  e+ = mid + c_i delta_i * 0.5;
//        alpha_i = (sigmoid(e- s) - sigmoid(e+ s) + 1e-5) / (sigmoid(e- s) + 1e-5)
//     3. w_i = alpha_i prod_{j<i} (1 - alpha_j + 1e-7) for i <= n - 2;  w_{n-1} = 0
//     4. w_i += 1e-5;  W = sum w;  pad = max(0, 1e-5 - W);  w_i += pad / n;  W += pad;
//        cdf_0 = 0,  cdf_{i+1} = min(1, cdf_i + w_i / W)
//     5. u_j = lin_j + r_k / (m + 1), for j = 0 .. m;  lin = torch.linspace(0, 1 - 1 / (m + 1), m + 1) in float32;
//        idx = number of cdf entries <= u_j (searchsorted(..., side='right'));  lo = clamp(idx - 1, 0, n),  hi = clamp(idx, 0, n);
//        q = (u_j - cdf_lo) / (cdf_hi - cdf_lo), 0 when the denominator is 0, clipped to [0, 1];  p_j = b_lo + q (b_hi - b_lo)
//     6. the new edge list is sort(b[0..n-1] U p[0..m-1]) followed by max(b[n], p[m]);  n <- n + m
//   result: S_tot = S0 + K m samples and S_tot + 1 edges, which the march composites with the learned inv_s (SO_JITTER_EDGES).
//
// One wave per ray, four rays per block.  The ray's edges, SDF values, cdf and new points live in LDS (S_tot + 1 floats each per wave).
// In the scans lane l owns the ceil(n / 64) consecutive samples from l * ceil(n / 64) on; the transmittance product and the
// cdf sum are a lane-local chain plus a 6-step wave scan, in DOUBLE: the float32 terms of the cdf (>= ~1e-5 of a total of ~1)
// add exactly in 53 bits, so the cdf is non-decreasing whatever the association, as the inverse-CDF search needs.  A new
// point's SDF is looked up when the point is made and travels with it through the merge, so only m lookups per step are new
// work.  The merge is by rank, no sort network: a new point goes to (old starts <= it) + (new points before it), an old start
// to its index + (new points below it); the new-point part counts instead of assuming p sorted, because
// fl(b_lo + fl(q * fl(b_hi - b_lo))) may exceed b_hi by an ulp.  No atomics: the same inputs give the same bits.
#include "ray_device.h"

namespace {

constexpr int kUpMaxSamples = 256;   // S_tot limit: what render_train / render_bwd take
constexpr int kUpMaxSteps = 8;
constexpr int kUpWaves = 4;          // rays per block

// Per wave, seven rows of `row` floats in dynamic LDS, row = S_tot + 1 rounded up to 4 (the launch knows S_tot): the edges and
// the SDF at the sample starts, each twice (ping-pong over the steps), the cdf, the step's new points p[0..m] and their SDF.
// 3.7 KB per wave at S_tot = 128, so that registers, not LDS, bound the occupancy.
constexpr int kUpRows = 7;
SO_DEVFN int so_upsample_row(int s_tot) { return (s_tot + 4) & ~3; }
static inline int so_upsample_row_host(int s_tot) { return (s_tot + 4) & ~3; }

template <int MK>
SO_DEVFN float so_upsample_sdf(const so_render_args &a, const RayGeom &g, float b, float tnear, float tfar) {
    const float t = so_edge_metric(b, tnear, tfar);
    const float px = g.ox + g.dx * t, py = g.oy + g.dy * t, pz = g.oz + g.dz * t;
    const so_cell cell = so_locate_k<MK>(a.map, px, py, pz);
    float v[8], wk[8];
    so_gather_sdf(a.sdf_vol, a.map.h.tot_len, a.map.w.tot_len, a.map.d.tot_len, cell, v);
    return so_trilerp_sdf(cell, v, wk);
}

// number of entries of the non-decreasing x[0..len-1] that are <= v
SO_DEVFN int so_count_le(const float *x, int len, float v) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

SO_DEVFN double so_shfl_up_f64(double v, int d) {
    const long long bits = __double_as_longlong(v);
    const int lo = __shfl_up((int)(bits & 0xffffffffLL), d, 64), hi = __shfl_up((int)(bits >> 32), d, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// m = new samples per step (>= 1 when n_steps > 0), s_tot = n_samples + n_steps * m <= kUpMaxSamples (host-checked)
template <int MK>
__global__ __launch_bounds__(64 * kUpWaves) void render_upsample_kernel(so_render_args a, int m, int n_steps, float base_variance,
                                                                        const float *__restrict__ u_rand, float *__restrict__ edges,
                                                                        int s_tot) {
    extern __shared__ float so_upsample_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ray_of_wave = blockIdx.x * kUpWaves + wave;
    const bool live = ray_of_wave < a.n_rays;
    const int ray = live ? ray_of_wave : a.n_rays - 1;   // a wave past the end redoes the last ray (the barriers stay uniform) and stores nothing
    const int row = so_upsample_row(s_tot);
    float *const rows = so_upsample_smem + wave * (kUpRows * row);
    float *const l_cdf = rows + 4 * row, *const l_p = rows + 5 * row, *const l_pf = rows + 6 * row;
    const RayGeom g = so_ray_of(a, ray);
    float tnear, tfar;
    so_collide(a, g, tnear, tfar);

    int n = a.n_samples, cur = 0;
    for (int j = lane; j <= n; j += 64) rows[j] = so_edge_unit(a, ray, j);
    __syncthreads();
    if (n_steps > 0)
        for (int i = lane; i < n; i += 64) rows[2 * row + i] = so_upsample_sdf<MK>(a, g, rows[i], tnear, tfar);
    __syncthreads();

    for (int k = 0; k < n_steps; ++k) {
        const float s = base_variance * (float)(1 << k);
        const float *b = rows + cur * row, *f = rows + (2 + cur) * row;
        float *bn = rows + (cur ^ 1) * row, *fn = rows + (2 + (cur ^ 1)) * row;
        const int P = (n + 63) >> 6;            // samples per lane, 1 .. 4

        // ---- 2. alphas of the lane's samples, and the lane's own transmittance chain ----
        float al[4];
        double tr[4], run = 1.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * P + q;
            al[q] = 0.0f;
            double fstep = 1.0;
            if (q < P && i < n - 1) {
                const float f0 = f[i], f1 = f[i + 1];
                const float t0 = so_edge_metric(b[i], tnear, tfar), t1 = so_edge_metric(b[i + 1], tnear, tfar);
                const float delta = t1 - t0;
                const float mid = (f0 + f1) * 0.5f;
                const float cosv = (f1 - f0) / (delta + 1e-5f);
                float cprev = 0.0f;
                if (i > 0) cprev = (f0 - f[i - 1]) / ((t0 - so_edge_metric(b[i - 1], tnear, tfar)) + 1e-5f);
                const float c = fminf(fmaxf(fminf(cprev, cosv), -1e3f), 0.0f);
                const float half = (c * delta) * 0.5f;
                const float prev_cdf = so_sigmoid((mid - half) * s);
                const float next_cdf = so_sigmoid((mid + half) * s);
                al[q] = ((prev_cdf - next_cdf) + 1e-5f) / (prev_cdf + 1e-5f);
                fstep = (double)((1.0f - al[q]) + 1e-7f);
            }
            tr[q] = run;                         // product over the lane's samples before this one
            run = run * fstep;
        }
        // ---- 3. exclusive wave scan of the lanes' products ----
        double incl = run;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = so_shfl_up_f64(incl, d);
            if (lane >= d) incl = incl * up;
        }
        double before = so_shfl_up_f64(incl, 1);
        if (lane == 0) before = 1.0;
        // ---- 4. weights -> pdf -> cdf ----
        float w[4];
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * P + q;
            const bool in = q < P && i < n;
            w[q] = in ? al[q] * (float)(before * tr[q]) + 1e-5f : 0.0f;      // al = 0 at i = n - 1: w_{n-1} = 0 (+ 1e-5)
            sum = sum + (double)w[q];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const long long bits = __double_as_longlong(sum);
            const int lo = __shfl_xor((int)(bits & 0xffffffffLL), d, 64), hi = __shfl_xor((int)(bits >> 32), d, 64);
            sum = sum + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
        }
        float W = (float)sum;
        const float pad = fmaxf(0.0f, 1e-5f - W);
        const float pad_each = pad / (float)n;
        W = W + pad;
        double part[4], lsum = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * P + q;
            const bool in = q < P && i < n;
            lsum = lsum + (in ? (double)((w[q] + pad_each) / W) : 0.0);
            part[q] = lsum;
        }
        double sincl = lsum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = so_shfl_up_f64(sincl, d);
            if (lane >= d) sincl = sincl + up;
        }
        double sbefore = so_shfl_up_f64(sincl, 1);
        if (lane == 0) { sbefore = 0.0; l_cdf[0] = 0.0f; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * P + q;
            if (q < P && i < n) l_cdf[i + 1] = fminf(1.0f, (float)(sbefore + part[q]));
        }
        __syncthreads();

        // ---- 5. the new points p[0..m] (and the SDF of p[0..m-1], unless this is the last step) ----
        const float r = u_rand ? u_rand[(size_t)k * a.n_rays + ray] : 0.5f;
        const float lin_end = 1.0f - 1.0f / (float)(m + 1);
        const float lin_step = lin_end / (float)m;
        const float shift = r / (float)(m + 1);
        for (int j = lane; j <= m; j += 64) {
            const float lin = (j < (m + 1) / 2) ? lin_step * (float)j : lin_end - lin_step * (float)(m - j);
            const float u = lin + shift;
            const int idx = so_count_le(l_cdf, n + 1, u);
            const int lo = min(max(idx - 1, 0), n), hi = min(max(idx, 0), n);
            const float c0 = l_cdf[lo], den = l_cdf[hi] - c0;
            float q = den == 0.0f ? 0.0f : (u - c0) / den;
            q = fminf(fmaxf(q, 0.0f), 1.0f);
            const float b0 = b[lo];
            const float pj = b0 + q * (b[hi] - b0);
            l_p[j] = pj;
            if (j < m && k + 1 < n_steps) l_pf[j] = so_upsample_sdf<MK>(a, g, pj, tnear, tfar);
        }
        __syncthreads();

        // ---- 6. merge by rank: keys (value, old before new, index) ----
        for (int j = lane; j < m; j += 64) {
            const float pj = l_p[j];
            int rank = so_count_le(b, n, pj);
            for (int jj = 0; jj < m; ++jj) {
                const float o = l_p[jj];
                rank += (o < pj || (o == pj && jj < j)) ? 1 : 0;
            }
            bn[rank] = pj;                       // rank <= n + m - 1 <= S_tot - 1 < row
            if (k + 1 < n_steps) fn[rank] = l_pf[j];
        }
        for (int i = lane; i < n; i += 64) {
            const float bi = b[i];
            int rank = i;
            for (int jj = 0; jj < m; ++jj) rank += (l_p[jj] < bi) ? 1 : 0;
            bn[rank] = bi;
            fn[rank] = f[i];
        }
        if (lane == 0) bn[n + m] = fmaxf(b[n], l_p[m]);
        __syncthreads();
        n += m;
        cur ^= 1;
    }

    if (live)
        for (int j = lane; j <= n; j += 64) edges[(size_t)ray * (s_tot + 1) + j] = rows[cur * row + j];
}

}  // namespace

extern "C" int selfocc_render_upsample(const so_render_upsample_args *args, void *stream) {
    SO_REQUIRE(args != nullptr, "args is NULL");
    SO_REQUIRE(args->edges != nullptr, "render_upsample: edges is NULL");
    so_render_args a = so_geometry_only(args->fwd);
    a.inv_s_dev = nullptr;                               // inv_s is ignored too: the sampler has its own variance
    SO_REQUIRE(a.n_samples >= 1, "render_upsample: n_samples must be >= 1 (got %d)", (int)a.n_samples);
    SO_REQUIRE(a.n_rays >= 0, "render_upsample: n_rays must be >= 0 (got %d)", (int)a.n_rays);
    SO_REQUIRE(a.jitter_mode != SO_JITTER_EDGES, "render_upsample: the sampler starts from the uniform bins (jitter_mode 0, 1 or 2), "
               "not from SO_JITTER_EDGES");
    SO_REQUIRE(args->n_importance >= 0, "render_upsample: n_importance must be >= 0 (got %d)", (int)args->n_importance);
    SO_REQUIRE(args->n_steps >= 0, "render_upsample: n_steps must be >= 0 (got %d)", (int)args->n_steps);
    SO_REQUIRE(args->n_steps <= kUpMaxSteps, "render_upsample: n_steps must be <= %d (got %d)", kUpMaxSteps, (int)args->n_steps);
    const int m = args->n_steps > 0 ? args->n_importance / args->n_steps : 0;
    const int n_steps = m >= 1 ? args->n_steps : 0;
    const long long s_tot = (long long)a.n_samples + (long long)n_steps * m;
    SO_REQUIRE(s_tot <= kUpMaxSamples, "render_upsample: n_samples + n_steps * (n_importance / n_steps) = %lld samples, must be <= %d",
               s_tot, kUpMaxSamples);
    SO_REQUIRE(args->base_variance > 0.0f && __builtin_isfinite(args->base_variance),
               "render_upsample: base_variance must be positive and finite (got %g)", (double)args->base_variance);
    if (so_validate_render(a)) return -1;
    if (a.n_rays == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((a.n_rays + kUpWaves - 1) / kUpWaves)), block(64 * kUpWaves);
    const size_t lds = (size_t)kUpWaves * kUpRows * so_upsample_row_host((int)s_tot) * sizeof(float);      // <= 29 120 bytes
    if (a.map.kind == SO_MAP_UPSCALE)
        hipLaunchKernelGGL(render_upsample_kernel<SO_MAP_UPSCALE>, grid, block, lds, st, a, m, n_steps, args->base_variance,
                           args->u_rand, args->edges, (int)s_tot);
    else
        hipLaunchKernelGGL(render_upsample_kernel<SO_MAP_LINEAR>, grid, block, lds, st, a, m, n_steps, args->base_variance,
                           args->u_rand, args->edges, (int)s_tot);
    return so_launch_status();
}
