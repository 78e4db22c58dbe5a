// field_grad.hip — the SDF gradient d sdf / d metre at arbitrary metre positions (selfocc_field_grad) and its backward
// with respect to the SDF volume (selfocc_field_grad_bwd), for gfx950.  DESIGN.md section 3.25.
//
// Until now the metric gradient existed only inside the render kernels, at ray samples.  Two definitions are served:
//   * ANALYTIC: the gradient the render kernels define for a sample at that position.  Nothing is restated: the cell is
//     so_locate_k's (linear, two-segment and linear_upscale mappings; the canonical cell at a voxel face), the corners are
//     so_gather_sdf's (zero padding), the value is so_trilerp_sdf's and the gradient so_trilerp_grad's (so_device.h) — the
//     calls render_train.hip makes for a sample, in its order, so the bits are those of its per-sample `grad` and `sdf`;
//   * NUMERICAL: central differences (sdfstudio's use_numerical_gradients / numerical_gradients_delta): for each axis k,
//     p+- = x with x_k +- delta in float32, s+- = the value selfocc_field_query returns at p+- (same locate, gather, sum and
//     padding), grad_k = (0.5f * (s+ - s-)) / delta in that association.  Six locates per point, no intermediate tensor.
// Both are linear in the SDF volume, so the backward is the transposed scatter (float atomics into a zero-initialised
// g_sdf_vol: selfocc_field_query_bwd's contract).  There is no gradient with respect to the positions.
//
// Lanes.  Pure gather / scatter, a few dozen flops per point.  Analytic: a lane per point (four 8-byte loads forward, eight
// atomics backward).  Numerical: a TEAM of 8 adjacent lanes per point — lane 0 the point itself, lanes 1 .. 6 the taps
// +x -x +y -y +z -z, lane 7 idle — so a lane does ONE locate, and 262 144 points make 32 768 waves, not 4 096 waves of six
// dependent locates each; forward the team's lanes 0 .. 2 fetch their axis' two tap values with one shuffle each and store
// the 12 contiguous bytes of the point's gradient; backward a team whose seven cells are one cell sums its corner
// contributions across the lanes first and adds one corner per lane (8 atomics per point instead of 56).
#include "so_device.h"

int so_validate_mapping(const so_mapping &m);      // render_fwd.hip

namespace {

constexpr int kTeam = 8;     // numerical mode: lanes per point

// the value selfocc_field_query returns for a point: its call sequence (occ.hip, field_query_kernel)
template <int MK>
SO_DEVFN float fg_sdf_at(const so_field_grad_args &a, int H, int W, int D, float x, float y, float z) {
    const so_cell c = so_locate_k<MK>(a.q.map, x, y, z);
    float v[8], wk[8];
    so_gather_sdf(a.q.sdf_vol, H, W, D, c, v);
    return so_trilerp_sdf(c, v, wk);
}

// c_k * w_k added to the in-range corners of a cell; wk = (fd * fw) * fh as so_trilerp_sdf forms it
SO_DEVFN void fg_scatter_value(float *__restrict__ g_sdf_vol, int H, int W, int D, const so_cell &c, float coef) {
    const float fd[2] = {c.fd0, c.fd1}, fw[2] = {c.fw0, c.fw1}, fh[2] = {c.fh0, c.fh1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int h = c.h0 + (k >> 2), w = c.w0 + ((k >> 1) & 1), d = c.d0 + (k & 1);
        if (h < 0 || h >= H || w < 0 || w >= W || d < 0 || d >= D) continue;   // zero padding: no gradient
        const float wk = (fd[k & 1] * fw[(k >> 1) & 1]) * fh[k >> 2];
        atomicAdd(g_sdf_vol + ((size_t)h * W + w) * D + d, coef * wk);
    }
}

// the tap of team lane j (1 .. 6) of a numerical point: axis (j - 1) / 2, +delta for odd j, -delta for even j
SO_DEVFN void fg_tap(int j, float delta, float &x, float &y, float &z) {
    const float s = (j & 1) ? delta : -delta;
    if (j == 1 || j == 2) x = x + s;
    if (j == 3 || j == 4) y = y + s;
    if (j == 5 || j == 6) z = z + s;
}

template <int MK>
__global__ __launch_bounds__(256) void field_grad_analytic_kernel(so_field_grad_args a) {
    const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gt >= a.q.n) return;
    const size_t i = (size_t)gt;
    const int H = a.q.map.h.tot_len, W = a.q.map.w.tot_len, D = a.q.map.d.tot_len;
    const so_cell c = so_locate_k<MK>(a.q.map, a.q.xyz[3 * i], a.q.xyz[3 * i + 1], a.q.xyz[3 * i + 2]);
    float v[8], wk[8], gx, gy, gz;
    so_gather_sdf(a.q.sdf_vol, H, W, D, c, v);
    const float s = so_trilerp_sdf(c, v, wk);
    so_trilerp_grad(c, v, gx, gy, gz);
    if (a.q.sdf) a.q.sdf[i] = s;
    a.grad[3 * i] = gx; a.grad[3 * i + 1] = gy; a.grad[3 * i + 2] = gz;
}

template <int MK>
__global__ __launch_bounds__(256) void field_grad_numerical_kernel(so_field_grad_args a) {
    const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pt = gt / kTeam;
    const int j = (int)(gt - pt * kTeam);
    const bool live = pt < a.q.n;
    const size_t i = live ? (size_t)pt : (size_t)a.q.n - 1;      // dead teams shadow the last point (the shuffles need every lane)
    const int H = a.q.map.h.tot_len, W = a.q.map.w.tot_len, D = a.q.map.d.tot_len;
    float x = a.q.xyz[3 * i], y = a.q.xyz[3 * i + 1], z = a.q.xyz[3 * i + 2];
    fg_tap(j, a.delta, x, y, z);
    const float s = fg_sdf_at<MK>(a, H, W, D, x, y, z);
    // lane j < 3 of the team: axis j, taps at team lanes 2 j + 1 (+) and 2 j + 2 (-)
    const int lane = (int)(threadIdx.x & 63), base = lane - j, ax = j < 3 ? j : 0;
    const float sp = __shfl(s, base + 2 * ax + 1, 64);
    const float sm = __shfl(s, base + 2 * ax + 2, 64);
    if (!live) return;
    if (j == 0 && a.q.sdf) a.q.sdf[i] = s;
    if (j < 3) a.grad[3 * i + j] = (0.5f * (sp - sm)) / a.delta;
}

template <int MK>
__global__ __launch_bounds__(256) void field_grad_analytic_bwd_kernel(so_field_grad_args a, const float *__restrict__ g_sdf,
                                                                      const float *__restrict__ g_grad,
                                                                      float *__restrict__ g_sdf_vol) {
    const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gt >= a.q.n) return;
    const size_t i = (size_t)gt;
    const int H = a.q.map.h.tot_len, W = a.q.map.w.tot_len, D = a.q.map.d.tot_len;
    const so_cell c = so_locate_k<MK>(a.q.map, a.q.xyz[3 * i], a.q.xyz[3 * i + 1], a.q.xyz[3 * i + 2]);
    const float fd[2] = {c.fd0, c.fd1}, fw[2] = {c.fw0, c.fw1}, fh[2] = {c.fh0, c.fh1};
    const float gs = g_sdf ? g_sdf[i] : 0.0f;
    // upstream of the GRID gradient: so_trilerp_grad multiplies the grid sums by the slopes last (x <-> w, y <-> h, z <-> d)
    const float uw = g_grad ? g_grad[3 * i] * c.sw : 0.0f;
    const float uh = g_grad ? g_grad[3 * i + 1] * c.sh : 0.0f;
    const float ud = g_grad ? g_grad[3 * i + 2] * c.sd : 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int kd = k & 1, kw = (k >> 1) & 1, kh = k >> 2;
        const int h = c.h0 + kh, w = c.w0 + kw, d = c.d0 + kd;
        if (h < 0 || h >= H || w < 0 || w >= W || d < 0 || d >= D) continue;   // zero padding: no gradient
        // the coefficients of v_k in so_trilerp_sdf and so_trilerp_grad
        const float cs = (fd[kd] * fw[kw]) * fh[kh];
        const float cd = fw[kw] * fh[kh], cw = fd[kd] * fh[kh], ch = fd[kd] * fw[kw];
        float t = gs * cs;
        t = kd ? t + ud * cd : t - ud * cd;
        t = kw ? t + uw * cw : t - uw * cw;
        t = kh ? t + uh * ch : t - uh * ch;
        atomicAdd(g_sdf_vol + ((size_t)h * W + w) * D + d, t);
    }
}

// One lane per (point, tap), as forward.  When all the team's cells are one cell — with delta well below a voxel, most points —
// the team's 7 x 8 corner contributions are summed across its lanes first (three butterfly steps per corner) and lane k adds
// corner k: 8 atomics per point, one per lane, instead of 56 of which seven at a time hit one address.  A team whose taps
// cross a face scatters lane by lane.  (Float atomics land in any order in either case.)
template <int MK>
__global__ __launch_bounds__(256) void field_grad_numerical_bwd_kernel(so_field_grad_args a, const float *__restrict__ g_sdf,
                                                                       const float *__restrict__ g_grad,
                                                                       float *__restrict__ g_sdf_vol) {
    const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long pt = gt / kTeam;
    const int j = (int)(gt - pt * kTeam);
    const bool live = pt < a.q.n;
    const size_t i = live ? (size_t)pt : (size_t)a.q.n - 1;      // dead teams shadow the last point (the shuffles need every lane)
    const int H = a.q.map.h.tot_len, W = a.q.map.w.tot_len, D = a.q.map.d.tot_len;
    float x = a.q.xyz[3 * i], y = a.q.xyz[3 * i + 1], z = a.q.xyz[3 * i + 2];
    fg_tap(j, a.delta, x, y, z);
    // this lane's upstream: g_sdf at the point itself, +-(0.5 g_k) / delta at a tap (d grad_k / d s+ = 0.5 / delta = - d grad_k / d s-)
    const bool has = live && (j == 0 ? g_sdf != nullptr : (j < 7 && g_grad != nullptr));
    float coef = 0.0f;
    if (has) {
        if (j == 0) {
            coef = g_sdf[i];
        } else {
            const float half = (0.5f * g_grad[3 * i + ((j - 1) >> 1)]) / a.delta;
            coef = (j & 1) ? half : -half;
        }
    }
    const so_cell c = so_locate_k<MK>(a.q.map, x, y, z);
    const int base = (int)(threadIdx.x & 63) - j;                // the team's lane 0 (teams are aligned: 256 % kTeam == 0)
    const bool same = c.h0 == __shfl(c.h0, base, 64) && c.w0 == __shfl(c.w0, base, 64) && c.d0 == __shfl(c.d0, base, 64);
    const unsigned long long agree = __ballot(same);
    if (((agree >> base) & 0xffull) == 0xffull) {                // the whole team, its idle lane included (it sits on the point)
        const float fd[2] = {c.fd0, c.fd1}, fw[2] = {c.fw0, c.fw1}, fh[2] = {c.fh0, c.fh1};
        float mine = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float t = coef * ((fd[k & 1] * fw[(k >> 1) & 1]) * fh[k >> 2]);
#pragma unroll
            for (int m = 1; m < kTeam; m <<= 1) t += __shfl_xor(t, m, 64);
            if (j == k) mine = t;
        }
        const int h = c.h0 + (j >> 2), w = c.w0 + ((j >> 1) & 1), d = c.d0 + (j & 1);
        if (live && h >= 0 && h < H && w >= 0 && w < W && d >= 0 && d < D)      // zero padding: no gradient
            atomicAdd(g_sdf_vol + ((size_t)h * W + w) * D + d, mine);
    } else if (has) {
        fg_scatter_value(g_sdf_vol, H, W, D, c, coef);
    }
}

// the checks both entries share; 1: nothing to do (n == 0)
int fg_validate(const so_field_grad_args *args, const char *who) {
    SO_REQUIRE(args != nullptr, "%s: args is NULL", who);
    const so_field_grad_args &a = *args;
    if (so_validate_mapping(a.q.map)) return -1;
    SO_REQUIRE(a.q.n >= 0, "%s: n must be >= 0 (got %d)", who, (int)a.q.n);
    SO_REQUIRE(a.mode == SO_GRAD_ANALYTIC || a.mode == SO_GRAD_NUMERICAL, "%s: unknown mode %d (0 = analytic, 1 = numerical)", who,
               (int)a.mode);
    SO_REQUIRE(a.mode != SO_GRAD_NUMERICAL || (a.delta > 0.0f && __builtin_isfinite(a.delta)),
               "%s: numerical mode needs a finite delta > 0 metres (got %g)", who, (double)a.delta);
    if (a.q.n == 0) return 1;
    SO_REQUIRE(a.q.xyz != nullptr, "%s: xyz is NULL", who);
    SO_REQUIRE(a.q.sdf_vol != nullptr, "%s: sdf_vol is NULL", who);
    return 0;
}

unsigned fg_blocks(const so_field_grad_args &a) {
    const long long threads = (long long)a.q.n * (a.mode == SO_GRAD_NUMERICAL ? kTeam : 1);      // n < 2^31: < 2^26 blocks
    return (unsigned)((threads + 255) / 256);
}

}  // namespace

extern "C" int selfocc_field_grad(const so_field_grad_args *args, void *stream) {
    const int rc = fg_validate(args, "field_grad");
    if (rc) return rc < 0 ? rc : 0;
    const so_field_grad_args &a = *args;
    SO_REQUIRE(a.grad != nullptr, "field_grad: grad is NULL");
    const bool up = a.q.map.kind == SO_MAP_UPSCALE;
    const dim3 grid(fg_blocks(a)), block(256);
    if (a.mode == SO_GRAD_NUMERICAL)
        hipLaunchKernelGGL((up ? field_grad_numerical_kernel<SO_MAP_UPSCALE> : field_grad_numerical_kernel<SO_MAP_LINEAR>), grid,
                           block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((up ? field_grad_analytic_kernel<SO_MAP_UPSCALE> : field_grad_analytic_kernel<SO_MAP_LINEAR>), grid,
                           block, 0, (hipStream_t)stream, a);
    return so_launch_status();
}

extern "C" int selfocc_field_grad_bwd(const so_field_grad_args *args, const float *g_sdf, const float *g_grad,
                                      float *g_sdf_vol, void *stream) {
    const int rc = fg_validate(args, "field_grad_bwd");
    if (rc) return rc < 0 ? rc : 0;
    const so_field_grad_args &a = *args;
    if (!g_sdf && !g_grad) return 0;
    SO_REQUIRE(g_sdf_vol != nullptr, "field_grad_bwd: g_sdf_vol is NULL");
    const bool up = a.q.map.kind == SO_MAP_UPSCALE;
    const dim3 grid(fg_blocks(a)), block(256);
    if (a.mode == SO_GRAD_NUMERICAL)
        hipLaunchKernelGGL((up ? field_grad_numerical_bwd_kernel<SO_MAP_UPSCALE> : field_grad_numerical_bwd_kernel<SO_MAP_LINEAR>),
                           grid, block, 0, (hipStream_t)stream, a, g_sdf, g_grad, g_sdf_vol);
    else
        hipLaunchKernelGGL((up ? field_grad_analytic_bwd_kernel<SO_MAP_UPSCALE> : field_grad_analytic_bwd_kernel<SO_MAP_LINEAR>),
                           grid, block, 0, (hipStream_t)stream, a, g_sdf, g_grad, g_sdf_vol);
    return so_launch_status();
}
