"""Host side of the fused SDF ray-march renderer (selfocc_render_fwd / _bwd).

This is the operator-level surface the head (selfocc_amd/model/head) builds on; it
replaces what the reference obtains from the sdfstudio fork's
``NeuSCustomModel.__call__(RayBundle)`` (model/head/neus_head/neus_head.py:353,394,531).
Tensors are only device-memory handles here: the arithmetic is in csrc/render_*.hip.
"""
import dataclasses
import os
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import abi, sh
from ._lib import lib, check, ptr, current_stream


@dataclass
class SDFVolume:
    """The pre-computed field volume in the layout the kernels read.

    sdf  : (H, W, D) float32
    feat : (H, W, D, F) float32 / bfloat16 or None; channels = raw colour (3) then
           semantic logits (n_sem = 2 .. 21), then pad: F == 3 + n_sem rounded up to a multiple of 4.
    sh_deg / sh_act : view-dependent colour (selfocc_amd/sh.py).  With sh_deg > 0 the colour channels are the
           3 * (sh_deg + 1)^2 spherical-harmonics coefficients, colour-major, F = 12 / 28 for degree 1 / 2 (float32,
           n_sem == 0); n_rgb stays 3, the number of colour outputs.
    The reference materialises (1, 1 + color_dims, H, W, D) instead
    (nerfacc_head/bev_nerf.py:74-95); ``from_reference_layout`` converts.
    """
    mapping: object            # GridMeterMapping / LinearMapping / NonLinearMapping (has to_abi())
    sdf: torch.Tensor
    feat: Optional[torch.Tensor] = None
    n_rgb: int = 0
    n_sem: int = 0
    sh_deg: int = 0
    sh_act: str = 'relu'

    @staticmethod
    def feat_width(n_rgb, n_sem, sh_deg=0):
        if n_rgb + n_sem == 0:
            return 0
        if sh_deg > 0:
            assert n_rgb == 3 and n_sem == 0, "sh_deg > 0 is built without semantic channels"
            return sh.feat_stride(sh_deg)
        # rows are [r, g, b, logit_0 .. logit_{n_sem - 1}, pad]: 3 + n_sem rounded up to 4 floats (4 without semantics; 8 / 24 for
        # 5 / 21 classes have no pad).  The render kernels never read a pad channel and leave its gradient zero.
        return (n_rgb + n_sem + 3) & ~3

    @property
    def n_colour(self):
        """colour channels stored per voxel: 3 * (sh_deg + 1)^2 coefficients when colour is rendered"""
        return sh.n_coef(self.sh_deg) if self.n_rgb else 0

    @classmethod
    def from_reference_layout(cls, mapping, density_color, n_rgb=0, n_sem=0, feat_dtype=torch.float32, sh_deg=0, sh_act='relu'):
        """density_color: (1, 1 + n_colour + n_sem, H, W, D) as in the reference (n_colour = 3 * (sh_deg + 1)^2 or 0)."""
        sh.check(sh_deg, sh_act)
        assert density_color.dim() == 5 and density_color.shape[0] == 1
        n_col = sh.n_coef(sh_deg) if n_rgb else 0
        assert density_color.shape[1] == 1 + n_col + n_sem
        sdf = density_color[0, 0].contiguous().float()
        feat = None
        if n_col + n_sem > 0:
            F = cls.feat_width(n_rgb, n_sem, sh_deg)
            H, W, D = sdf.shape
            feat = torch.zeros(H, W, D, F, dtype=feat_dtype, device=sdf.device)
            feat[..., :n_col + n_sem] = density_color[0, 1:].permute(1, 2, 3, 0).to(feat_dtype)
        return cls(mapping, sdf, feat, n_rgb, n_sem, sh_deg, sh_act)

    def to_reference_layout(self):
        ch = [self.sdf[None]]
        if self.feat is not None:
            ch.append(self.feat[..., :self.n_colour + self.n_sem].float().permute(3, 0, 1, 2))
        return torch.cat(ch, 0)[None]

    def with_tensors(self, sdf, feat):
        """the same field description (mapping, channel meaning) over other tensors"""
        return SDFVolume(self.mapping, sdf, feat, self.n_rgb, self.n_sem, self.sh_deg, self.sh_act)

    def detached(self):
        return self.with_tensors(self.sdf.detach(), None if self.feat is None else self.feat.detach())

    def cpu(self):
        return self.with_tensors(self.sdf.cpu(), None if self.feat is None else self.feat.cpu())

    def to(self, device):
        return self.with_tensors(self.sdf.to(device), None if self.feat is None else self.feat.to(device))


@dataclass
class RaySet:
    """Either explicit rays (RayBundle-like) or a per-camera pixel lattice from which
    the kernel generates origin / direction itself (RaySampler + Img2LiDAR fused)."""
    origins: Optional[torch.Tensor] = None    # (N, 3)
    dirs: Optional[torch.Tensor] = None       # (N, 3) unit
    dir_norm: Optional[torch.Tensor] = None   # (N,)
    img2lidar: Optional[torch.Tensor] = None  # (n_cams, 4, 4) float32
    nx: int = 0
    ny: int = 0
    sx: float = 1.0
    sy: float = 1.0
    ox: float = 0.0
    oy: float = 0.0

    @property
    def pixel_grid(self):
        return self.img2lidar is not None

    @property
    def n_rays(self):
        if self.pixel_grid:
            return self.img2lidar.shape[0] * self.nx * self.ny
        return self.origins.shape[0]

    @property
    def device(self):
        return (self.img2lidar if self.pixel_grid else self.origins).device

    def cpu(self):
        c = lambda t: None if t is None else t.cpu()
        return RaySet(c(self.origins), c(self.dirs), c(self.dir_norm), c(self.img2lidar),
                      self.nx, self.ny, self.sx, self.sy, self.ox, self.oy)


@dataclass
class RenderConfig:
    aabb: tuple                       # (xmin, ymin, zmin, xmax, ymax, zmax)
    n_samples: int = 128
    inv_s: float = 20.0
    inv_s_dev: object = None          # optional 1-element float32 DEVICE tensor: the kernels read inv_s from it (no host copy)
    near_plane: float = 0.0
    sample_pos: int = abi.SAMPLE_AT_START
    jitter_mode: int = abi.JITTER_NONE
    bkgd_mode: int = abi.BKGD_NONE
    bkgd: tuple = (0.0, 0.0, 0.0)
    depth_div_norm: bool = True
    clamp_rgb: bool = False
    exact: bool = False               # canonical IEEE op order (bit-exact with the oracle), slower
    brick: bool = True                # fast path: re-pack the SDF volume into 16-byte corner records per launch
    skip: bool = True                 # fast path + brick: composite saturated free-space samples without interpolating
    face_safe: bool = True            # fast path: canonical cell selection within a few ulp of a voxel face (skip marcher on
                                      # the cfg2 frame, MI355X: 7.2 % slower at inv_s 20, 3.5 % at 200)
    ahead: bool = True                # SDF-only per-ray launches with brick + skip: code-ahead skip marcher (A/B)
    ray_per_lane: bool = False        # ignored since ABI 30 (was: per-sample launches through ray-per-lane kernels, an A/B switch)
    bwd_scatter: str = 'auto'         # backward: 'binned' = brick-binned LDS scatter of the volume gradients (needs a scratch
                                      # of ~(record + 8) bytes per sample), 'atomic' = per-sample row atomics, 'auto' = binned
                                      # from 2^19 samples per launch — measured cross-over 0.4 - 0.5 M samples at 25 channels, scripts/time_render_bwd_sizes.py
                                      # (SELFOCC_RB_SCATTER overrides 'auto')


def _c(t, dtype=torch.float32):
    assert t.dtype == dtype and t.is_contiguous(), f"need contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}"
    return t


def marshal_render_args(vol: SDFVolume, rays: RaySet, cfg: RenderConfig, *, per_sample=False,
                        want_grad_samples=False, t_rand=None, bkgd_rays=None, outputs=None, inputs_only=False):
    """Fill an ``so_render_args`` for tensors living on ONE device (CUDA for the HIP
    library; the test oracle feeds CPU tensors through the same marshalling).
    Returns (args, outputs_dict, keepalive).  ``inputs_only``: allocate no output (the callers whose entry point
    ignores the outputs of the struct: render_median_depth)."""
    dev = vol.sdf.device
    a = abi.SoRenderArgs()
    a.map = vol.mapping.to_abi()
    H, W, D = a.map.h.tot_len, a.map.w.tot_len, a.map.d.tot_len
    assert tuple(vol.sdf.shape) == (H, W, D), f"sdf volume {tuple(vol.sdf.shape)} != mapping {(H, W, D)}"
    a.sdf_vol = ptr(_c(vol.sdf))
    a.n_rgb, a.n_sem = vol.n_rgb, vol.n_sem
    sh.check(vol.sh_deg, vol.sh_act)
    a.sh_deg, a.sh_act = vol.sh_deg, abi.SH_SIGMOID if vol.sh_act == 'sigmoid' else abi.SH_RELU
    if vol.feat is not None:
        assert vol.feat.is_contiguous() and vol.feat.shape[:3] == (H, W, D)
        assert vol.feat.dtype in (torch.float32, torch.bfloat16)
        a.feat_vol = ptr(vol.feat)
        a.feat_dtype = abi.DTYPE_F32 if vol.feat.dtype == torch.float32 else abi.DTYPE_BF16
        a.feat_stride = vol.feat.shape[3]
    N = rays.n_rays
    a.n_rays = N
    keep = [vol, rays, t_rand, bkgd_rays]
    if rays.pixel_grid:
        a.ray_mode = abi.RAYS_PIXEL_GRID
        a.img2lidar = ptr(_c(rays.img2lidar))
        a.n_cams, a.nx, a.ny = rays.img2lidar.shape[0], rays.nx, rays.ny
        a.sx, a.sy, a.ox, a.oy = rays.sx, rays.sy, rays.ox, rays.oy
    else:
        a.ray_mode = abi.RAYS_EXPLICIT
        a.origins, a.dirs = ptr(_c(rays.origins)), ptr(_c(rays.dirs))
        a.dir_norm = ptr(None if rays.dir_norm is None else _c(rays.dir_norm))
    for i in range(6):
        a.aabb[i] = float(cfg.aabb[i])
    a.near_plane = cfg.near_plane
    a.n_samples = S = cfg.n_samples
    a.sample_pos = cfg.sample_pos
    a.jitter_mode = cfg.jitter_mode
    if cfg.jitter_mode != abi.JITTER_NONE:
        exp = (N,) if cfg.jitter_mode == abi.JITTER_SINGLE else (N, S + 1)       # JITTER_EDGES: the (N, S + 1) edges themselves
        assert t_rand is not None and tuple(t_rand.shape) == exp, f"t_rand must be {exp}"
        a.t_rand = ptr(_c(t_rand))
    a.inv_s = float(cfg.inv_s)
    if cfg.inv_s_dev is not None:
        t = cfg.inv_s_dev
        assert t.dtype == torch.float32 and t.numel() == 1 and t.device == dev, "inv_s_dev: one float32 on the volume's device"
        a.inv_s_dev = ptr(t)
        keep.append(t)
    a.bkgd_mode = cfg.bkgd_mode
    for i in range(3):
        a.bkgd[i] = float(cfg.bkgd[i])
    if cfg.bkgd_mode == abi.BKGD_PER_RAY:
        assert bkgd_rays is not None and tuple(bkgd_rays.shape) == (N, 3)
        a.bkgd_rays = ptr(_c(bkgd_rays))
    a.flags = (abi.FLAG_DEPTH_DIV_NORM if cfg.depth_div_norm else 0) | (abi.FLAG_CLAMP_RGB if cfg.clamp_rgb else 0) | \
        (abi.FLAG_EXACT if cfg.exact else 0) | (0 if cfg.skip else abi.FLAG_NO_SKIP) | \
        (0 if cfg.face_safe else abi.FLAG_NO_FACE_SAFE) | (0 if cfg.ahead else abi.FLAG_NO_AHEAD) | \
        (abi.FLAG_RAY_PER_LANE if cfg.ray_per_lane else 0)

    f32 = dict(dtype=torch.float32, device=dev)
    out = outputs if outputs is not None else {}
    if inputs_only:
        return a, out, keep
    def alloc(name, *shape):
        if name not in out:
            out[name] = torch.empty(*shape, **f32)
        return ptr(out[name])
    a.depth, a.acc = alloc('depth', N), alloc('acc', N)
    a.max_depth, a.nears, a.fars = alloc('max_depth', N), alloc('nears', N), alloc('fars', N)
    if vol.n_rgb == 3:
        a.rgb = alloc('rgb', N, 3)
    if vol.n_sem > 0:
        a.sem = alloc('sem', N, vol.n_sem)
    if per_sample:
        a.weights, a.ts, a.deltas = alloc('weights', N, S), alloc('ts', N, S), alloc('deltas', N, S)
        if want_grad_samples:
            a.sdf, a.grad = alloc('sdf', N, S), alloc('grad', N, S, 3)
    keep.append(out)
    return a, out, keep


def _with_edges(cfg, edges, t_rand, n_rays):
    """``edges=`` of the render calls: (N, S + 1) normalised, non-decreasing edges per ray (``upsample_edges``) replace the
    uniform bins.  They set the mode and the sample count and travel in the ``t_rand`` slot; they are constants (upstream
    samples them under no_grad)."""
    if edges is None:
        return cfg, t_rand
    assert t_rand is None, "edges= replaces the uniform bins: t_rand does not apply (the jitter is in the edges)"
    assert edges.dim() == 2 and edges.shape[0] == n_rays and edges.shape[1] >= 2, \
        f"edges must be (n_rays = {n_rays}, n_samples + 1), got {tuple(edges.shape)}"
    return dataclasses.replace(cfg, n_samples=edges.shape[1] - 1, jitter_mode=abi.JITTER_EDGES), edges.detach()


_GEOMETRY_FIELDS = ('aabb', 'n_samples', 'inv_s', 'inv_s_dev', 'near_plane', 'sample_pos', 'jitter_mode')


def _geometry_args(vol, rays, cfg, *, t_rand, edges=None, what, fields=_GEOMETRY_FIELDS):
    """The ``so_render_args`` of a geometry-only entry point (csrc/ray_device.h: so_geometry_only): the SDF volume alone
    (``vol.feat`` is not looked at), the rays, and of ``cfg`` only ``fields``, the sampling fields and inv_s; its background,
    colour and march switches do not apply.  No output is allocated and no tensor is copied: every pointer is into the
    storage of one of the caller's own arguments, which keep it alive.  Returns (args, n_rays, device)."""
    if not vol.sdf.is_cuda:
        raise RuntimeError(f"selfocc_amd.{what} needs CUDA(HIP) tensors: there is no CPU fallback")
    cfg, t_rand = _with_edges(cfg, edges, t_rand, rays.n_rays)
    geo = RenderConfig(**{f: getattr(cfg, f) for f in fields})
    a, _out, _keep = marshal_render_args(SDFVolume(vol.mapping, vol.sdf), rays, geo, t_rand=t_rand, inputs_only=True)
    return a, rays.n_rays, vol.sdf.device


def render_rays(vol: SDFVolume, rays: RaySet, cfg: RenderConfig, *, per_sample=False,
                want_grad_samples=False, t_rand=None, bkgd_rays=None, outputs=None, edges=None):
    """Forward render on the GPU (no autograd).  Returns a dict of per-ray tensors
    (depth, acc, rgb, sem, max_depth, nears, fars) and, with ``per_sample``, the
    (N, S) tensors weights / ts / deltas (/ sdf / grad).  ``edges``: see ``_with_edges`` (S = edges.shape[1] - 1)."""
    if not vol.sdf.is_cuda:
        raise RuntimeError("selfocc_amd.render_rays needs CUDA(HIP) tensors: there is no CPU fallback")
    cfg, t_rand = _with_edges(cfg, edges, t_rand, rays.n_rays)
    a, out, _keep = marshal_render_args(vol, rays, cfg, per_sample=per_sample,
                                        want_grad_samples=want_grad_samples, t_rand=t_rand,
                                        bkgd_rays=bkgd_rays, outputs=outputs)
    # the re-pack only pays off for large ray batches; the 'linear_upscale' mapping takes the canonical route, which reads no brick
    if cfg.brick and not cfg.exact and a.map.kind == abi.MAP_LINEAR and rays.n_rays * cfg.n_samples >= 16 * vol.sdf.numel():
        a.sdf_brick = ptr(_brick_workspace(vol.sdf))
    check(lib().selfocc_render_fwd(a, current_stream(vol.sdf.device)), "selfocc_render_fwd")
    return out


def render_median_depth(vol: SDFVolume, rays: RaySet, cfg: RenderConfig, *, t_rand=None, want_index=False, edges=None):
    """Median depth of every ray in ONE launch (selfocc_render_median, csrc/render_median.hip): nerfstudio's
    DepthRenderer(method="median"), the ``ms_depths_median`` of eval_depth.py.  Equal, bit for bit, to
    ``median_depth_reference`` applied to the ``weights`` / ``ts`` of ``render_rays(vol, rays, cfg, per_sample=True)``,
    without materialising them: a ray stops marching at the first sample whose running weight sum reaches 0.5.
    Reads the SDF volume only (``vol.feat`` is not looked at) and marches in the canonical order whatever ``cfg.exact``.
    Returns {'median_depth': (N,) float32[, 'median_index': (N,) int32]}."""
    ma = abi.SoRenderMedianArgs()
    ma.fwd, N, dev = _geometry_args(vol, rays, cfg, t_rand=t_rand, edges=edges, what="render_median_depth")
    out = {'median_depth': torch.empty(N, dtype=torch.float32, device=dev)}
    if want_index:
        out['median_index'] = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:          # nothing to launch (and an empty tensor has no address to pass)
        return out
    ma.median_depth = ptr(out['median_depth'])
    if want_index:
        ma.median_index = ptr(out['median_index'])
    check(lib().selfocc_render_median(ma, current_stream(dev)), "selfocc_render_median")
    return out


def median_depth_reference(weights, ts):
    """The definition of the median depth, on CPU tensors or arrays of shape (..., S):
        c_0 = w_0, c_i = c_{i-1} + w_i  in float32, in sample order;   j = the first i with c_i >= 0.5, S - 1 if none
    Returns (median_depth = ts[..., j] float32, median_index = j int32), as tensors when ``weights`` is one.
    Sequential float32 on purpose: torch.cumsum on the CPU accumulates float32 in double."""
    import numpy as np
    as_tensor = isinstance(weights, torch.Tensor)
    host = lambda t: (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    if as_tensor and weights.is_cuda:
        raise RuntimeError("median_depth_reference is the CPU definition: pass CPU tensors or arrays")
    w, t = host(weights).astype(np.float32, copy=False), host(ts).astype(np.float32, copy=False)
    assert w.shape == t.shape and w.ndim >= 1 and w.shape[-1] >= 1, f"weights {w.shape} / ts {t.shape}: need equal (..., S >= 1)"
    S = w.shape[-1]
    c = np.add.accumulate(w, axis=-1, dtype=np.float32)
    hit = c >= np.float32(0.5)                                  # a NaN sum never compares true
    j = np.where(hit.any(-1), hit.argmax(-1), S - 1).astype(np.int32)
    depth = np.take_along_axis(t, j[..., None].astype(np.int64), -1)[..., 0]
    if as_tensor:
        return torch.from_numpy(np.ascontiguousarray(depth)), torch.from_numpy(np.ascontiguousarray(j))
    return depth, j


def render_normal_vis(vol: SDFVolume, rays: RaySet, cfg: RenderConfig, *, t_rand=None, edges=None):
    """Rendered surface normal of every ray in ONE launch (selfocc_render_normal, csrc/render_normal.hip): sdfstudio's
    ``normal_vis``, the ``vis_normal`` of the reference's render dicts.  Equal, bit for bit, to ``normal_vis_reference``
    applied to the ``weights`` / ``grad`` of ``render_rays(vol, rays, cfg, per_sample=True, want_grad_samples=True)``,
    without materialising them.  Reads the SDF volume only (``vol.feat`` is not looked at), marches every sample in the
    canonical order whatever ``cfg.exact``, and never reads anything back to the host (``cfg.inv_s_dev`` is honoured).
    Returns (N, 3) float32; a ray that misses the box by more than a cell (zero gradients) gives (0.5, 0.5, 0.5)."""
    na = abi.SoRenderNormalArgs()
    na.fwd, N, dev = _geometry_args(vol, rays, cfg, t_rand=t_rand, edges=edges, what="render_normal_vis")
    out = torch.empty(N, 3, dtype=torch.float32, device=dev)
    if N == 0:          # nothing to launch (and an empty tensor has no address to pass)
        return out
    na.normal_vis = ptr(out)
    check(lib().selfocc_render_normal(na, current_stream(dev)), "selfocc_render_normal")
    return out


def normal_vis_reference(weights, grad):
    """The definition of the rendered normal, on CPU tensors or arrays: ``weights`` (n, S),
    ``grad`` (n, S, 3), every step one float32 operation, the sum in sample order:
        r_i = sqrt((gx*gx + gy*gy) + gz*gz);  d_i = max(r_i, 1e-12);  n_i = g_i / d_i
        N = 0;  N = N + w_i * n_i  for i = 0 .. S - 1;   normal_vis = (N + 1) / 2
    Returns (n, 3) float32, a tensor when ``weights`` is one.  A plain loop over the samples on purpose: a library sum adds in
    another order.  numpy float32 on purpose: its square root and division are the correctly rounded ones, as the kernel's
    are; torch.sqrt on the CPU is not on every build."""
    import numpy as np
    as_tensor = isinstance(weights, torch.Tensor)
    host = lambda t: (t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    if as_tensor and (weights.is_cuda or grad.is_cuda):
        raise RuntimeError("normal_vis_reference is the CPU definition: pass CPU tensors or arrays")
    w, g = host(weights).astype(np.float32, copy=False), host(grad).astype(np.float32, copy=False)
    assert w.ndim == 2 and g.shape == (*w.shape, 3) and w.shape[1] >= 1, \
        f"weights {w.shape} / grad {g.shape}: need (n, S >= 1) / (n, S, 3)"
    gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
    r = np.sqrt((gx * gx + gy * gy) + gz * gz)
    d = np.fmax(r, np.float32(1e-12))[..., None]              # fmaxf: a NaN norm gives the clamp
    n = g / d
    N = np.zeros((w.shape[0], 3), dtype=np.float32)
    for i in range(w.shape[1]):
        N = N + w[:, i, None] * n[:, i]
    out = (N + np.float32(1.0)) / np.float32(2.0)
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out)) if as_tensor else out


UPSAMPLE_MAX_SAMPLES, UPSAMPLE_MAX_STEPS = 256, 8


def upsample_plan(n_samples, n_importance, n_steps):
    """(m, K, S_tot) of NeuS up-sampling: m = n_importance // n_steps new samples in each of K steps, K = 0 (nothing runs,
    S_tot = n_samples) unless n_importance > 0, n_steps > 0 and m >= 1.  Refuses, by name, what the kernels do not take."""
    if n_importance < 0 or n_steps < 0:
        raise ValueError(f"num_samples_importance = {n_importance} / num_up_sample_steps = {n_steps} must be >= 0")
    if n_steps > UPSAMPLE_MAX_STEPS:
        raise ValueError(f"num_up_sample_steps = {n_steps} is not built (built: <= {UPSAMPLE_MAX_STEPS})")
    m = n_importance // n_steps if n_steps > 0 else 0
    K = n_steps if m >= 1 else 0
    s_tot = n_samples + K * m
    if K > 0 and s_tot > UPSAMPLE_MAX_SAMPLES:
        raise ValueError(f"num_samples + num_up_sample_steps * (num_samples_importance // num_up_sample_steps) = {s_tot} samples "
                         f"is not built (built: <= {UPSAMPLE_MAX_SAMPLES}, what the per-sample forward and the backward take)")
    return m, K, s_tot


def upsample_edges(vol: SDFVolume, rays: RaySet, cfg: RenderConfig, n_importance, n_steps, base_variance, t_rand=None, u_rand=None):
    """NeuS hierarchical up-sampling in ONE launch (selfocc_render_upsample, csrc/render_upsample.hip; the definition is in
    that file's header and in DESIGN.md section 3.20): from the ``cfg.n_samples`` uniform (or jittered: ``cfg.jitter_mode`` /
    ``t_rand``) bins, ``n_steps`` rounds that each place ``n_importance // n_steps`` new samples by the inverse CDF of
    fixed-variance NeuS weights (``base_variance * 2^k``).  ``u_rand`` (n_steps, N) uniform [0, 1) or None (0.5).
    Returns the (N, S_tot + 1) normalised edges for the ``edges=`` argument of the render calls; with nothing to add
    (``upsample_plan``: K = 0) they are the start edges.  Reads the SDF volume only; no gradient."""
    m, K, s_tot = upsample_plan(cfg.n_samples, int(n_importance), int(n_steps))
    if s_tot > UPSAMPLE_MAX_SAMPLES:
        raise ValueError(f"n_samples = {s_tot} is not built for upsample_edges (built: <= {UPSAMPLE_MAX_SAMPLES})")
    assert cfg.jitter_mode != abi.JITTER_EDGES, "upsample_edges starts from the uniform bins"
    ua = abi.SoRenderUpsampleArgs()
    # the sampler has its own variance and always looks up the sample start: neither inv_s nor sample_pos
    ua.fwd, N, dev = _geometry_args(vol, rays, cfg, t_rand=t_rand, what="upsample_edges",
                                    fields=('aabb', 'n_samples', 'near_plane', 'jitter_mode'))
    edges = torch.empty(N, s_tot + 1, dtype=torch.float32, device=dev)
    if N == 0:
        return edges
    ua.n_importance, ua.n_steps, ua.base_variance = int(n_importance), int(n_steps), float(base_variance)
    if u_rand is not None and K > 0:
        assert tuple(u_rand.shape) == (int(n_steps), N), f"u_rand must be {(int(n_steps), N)}"
        ua.u_rand = ptr(_c(u_rand))
    ua.edges = ptr(edges)
    check(lib().selfocc_render_upsample(ua, current_stream(dev)), "selfocc_render_upsample")
    return edges


def uniform_edges_reference(n_samples, jitter_mode=abi.JITTER_NONE, t_rand=None, n_rays=1):
    """(n_rays, n_samples + 1) float32: the normalised edges the kernels start from (so_edge before its last line), operation
    for operation: torch.linspace(0, 1, n + 1) in its symmetric-halves form, then the optional stratified jitter."""
    n = int(n_samples)
    j = torch.arange(n + 1)
    step = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    upper = (1.0 - step.double() * (n - j).double()).float()          # fmaf(-step, n - j, 1): the product is exact in float64
    b = torch.where(j < (n + 1) // 2, step * j.float(), upper)
    if jitter_mode != abi.JITTER_NONE:
        tr = t_rand.float().cpu()
        tr = tr[:, None] if jitter_mode == abi.JITTER_SINGLE else tr
        lo = torch.cat([b[:1], (b[1:] + b[:-1]) / 2.0])
        hi = torch.cat([(b[1:] + b[:-1]) / 2.0, b[-1:]])
        return (lo[None] + (hi - lo)[None] * tr).contiguous()
    return b[None].repeat(n_rays, 1)


def neus_upsample_reference(sdf_at, origins, dirs, nears, fars, n_samples, n_importance, n_steps, base_variance, *,
                            jitter_mode=abi.JITTER_NONE, t_rand=None, u_rand=None, dtype=torch.float32):
    """The definition of NeuS up-sampling on CPU tensors, in ``dtype`` (float32, or float64 on
    request).  ``sdf_at``: callable (n, 3) positions in ``dtype`` -> (n,) SDF, the lookup of the field.  origins / dirs (N, 3),
    nears / fars (N,): the rays and what the box collider gives them.  The start edges are part of the inputs: float32
    (``uniform_edges_reference``) whatever ``dtype``.  Returns (N, S_tot + 1) normalised edges in ``dtype``."""
    N = origins.shape[0]
    m, K, _ = upsample_plan(int(n_samples), int(n_importance), int(n_steps))
    b = uniform_edges_reference(n_samples, jitter_mode, t_rand, N).to(dtype)
    o, d = origins.cpu().to(dtype), dirs.cpu().to(dtype)
    tn, tf = nears.cpu().to(dtype)[:, None], fars.cpu().to(dtype)[:, None]
    n = int(n_samples)
    for k in range(K):
        s = float(base_variance) * 2.0 ** k
        t = b * tf + (1 - b) * tn                                                      # (N, n + 1)
        f = sdf_at((o[:, None, :] + d[:, None, :] * t[:, :n, None]).reshape(-1, 3)).reshape(N, n).to(dtype)
        delta = t[:, 1:n] - t[:, :n - 1]                                               # i = 0 .. n - 2
        mid = (f[:, :-1] + f[:, 1:]) * 0.5
        cos = (f[:, 1:] - f[:, :-1]) / (delta + 1e-5)
        prev = torch.cat([torch.zeros(N, 1, dtype=dtype), cos[:, :-1]], 1)[:, :n - 1]       # cos_{i-1}, cos_{-1} = 0
        c = torch.minimum(prev, cos).clamp(-1e3, 0.0)
        half = c * delta * 0.5
        pc, nc = torch.sigmoid((mid - half) * s), torch.sigmoid((mid + half) * s)
        alpha = (pc - nc + 1e-5) / (pc + 1e-5)
        trans = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dtype), 1.0 - alpha + 1e-7], 1), 1)[:, :-1]
        w = torch.cat([alpha * trans, torch.zeros(N, 1, dtype=dtype)], 1) + 1e-5       # (N, n)
        W = w.sum(-1, keepdim=True)
        pad = torch.relu(1e-5 - W)
        w, W = w + pad / n, W + pad
        cdf = torch.cat([torch.zeros(N, 1, dtype=dtype), torch.cumsum(w / W, -1).clamp(max=1.0)], 1).contiguous()   # (N, n + 1)
        lin = torch.linspace(0.0, 1.0 - 1.0 / (m + 1), m + 1, dtype=torch.float32).to(dtype)
        r = torch.full((N,), 0.5, dtype=dtype) if u_rand is None else u_rand[k].cpu().to(dtype)
        u = (lin[None] + r[:, None] / (m + 1)).contiguous()                            # (N, m + 1)
        idx = torch.searchsorted(cdf, u, right=True)
        lo, hi = (idx - 1).clamp(0, n), idx.clamp(0, n)
        c_lo, c_hi = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
        den = c_hi - c_lo
        q = torch.where(den == 0, torch.zeros_like(den), (u - c_lo) / torch.where(den == 0, torch.ones_like(den), den)).clamp(0.0, 1.0)
        b_lo, b_hi = torch.gather(b, 1, lo), torch.gather(b, 1, hi)
        p = b_lo + q * (b_hi - b_lo)
        b = torch.cat([torch.sort(torch.cat([b[:, :n], p[:, :m]], 1), -1).values, torch.maximum(b[:, n:], p[:, m:])], 1)
        n += m
    return b


_BRICK_WS = {}


def _brick_workspace(sdf):
    """Per (device, stream, shape) scratch for the 16-byte corner records of the SDF volume ([H][W][D][4] f32) followed
    by one skip-code byte per cell; rewritten by every launch on the launch stream, so it is never stale and two
    streams never share one."""
    key = (sdf.device, torch.cuda.current_stream(sdf.device).cuda_stream, tuple(sdf.shape))
    ws = _BRICK_WS.get(key)
    if ws is None:
        n = sdf.numel()
        ws = _BRICK_WS[key] = torch.empty((n * 17 + 15) // 16 * 16, dtype=torch.uint8, device=sdf.device)
    return ws


def _scatter_workspace(device, nbytes):
    """Scratch of the binned backward scatter (~(record + 8) bytes per sample: 0.95 GB at the nuscenes_occ training shape,
    28 800 rays x 256 samples x 128-byte records).  Taken from torch's caching allocator for the duration of ONE backward
    call — stream-ordered, returned to the pool when the call ends, so that the forward pass of the next iteration can
    reuse the memory (until round 4 it was a grow-only, process-lifetime buffer per (device, stream): +0.95 GB of peak)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class _RenderFunction(torch.autograd.Function):
    """Differentiable wrt the SDF volume, the feature volume and inv_s (a 0-dim / 1-elem
    tensor).  Ray geometry carries no gradient — the reference's rays come from constant
    camera matrices (model/head/nerfacc_head/img2lidar.py:36-69)."""

    @staticmethod
    def forward(ctx, sdf_vol, feat_vol, inv_s, mapping, n_rgb, n_sem, rays, cfg, t_rand, bkgd_rays, want_grad_samples,
                sh_deg=0, sh_act='relu'):
        vol = SDFVolume(mapping, sdf_vol, feat_vol, n_rgb, n_sem, sh_deg, sh_act)
        # the kernels read inv_s from the device tensor itself: no read-back, no stream sync, nothing to go stale
        cfg_run = RenderConfig(**{**cfg.__dict__, 'inv_s_dev': inv_s.detach().reshape(1).float().contiguous()})
        out = render_rays(vol, rays, cfg_run, per_sample=True, want_grad_samples=want_grad_samples,
                          t_rand=t_rand, bkgd_rays=bkgd_rays)
        # tensor inputs go through save_for_backward (version-counter checks, saved-tensor hooks); the ray set and
        # the config are plain python state
        ctx.has = (feat_vol is not None, t_rand is not None, bkgd_rays is not None)
        ctx.save_for_backward(*[t for t in (sdf_vol, feat_vol, t_rand, bkgd_rays, cfg_run.inv_s_dev) if t is not None])
        ctx.meta = (mapping, n_rgb, n_sem, sh_deg, sh_act)
        ctx.rays, ctx.cfg = rays, RenderConfig(**{**cfg_run.__dict__, 'inv_s_dev': None})
        ctx.inv_s_shape = inv_s.shape
        ctx.keys = ['depth', 'acc'] + (['rgb'] if n_rgb else []) + (['sem'] if n_sem else []) + ['weights'] + \
            (['sdf', 'grad'] if want_grad_samples else [])
        ctx.nondiff_keys = ['ts', 'deltas', 'max_depth', 'nears', 'fars']
        nd = tuple(out[k] for k in ctx.nondiff_keys)
        ctx.mark_non_differentiable(*nd)
        return tuple(out[k] for k in ctx.keys) + nd

    @staticmethod
    def backward(ctx, *grads):
        saved = list(ctx.saved_tensors)
        sdf_vol = saved.pop(0)
        feat_vol = saved.pop(0) if ctx.has[0] else None
        t_rand = saved.pop(0) if ctx.has[1] else None
        bkgd_rays = saved.pop(0) if ctx.has[2] else None
        inv_s_dev = saved.pop(0)
        vol = SDFVolume(ctx.meta[0], sdf_vol, feat_vol, *ctx.meta[1:])
        rays, cfg = ctx.rays, RenderConfig(**{**ctx.cfg.__dict__, 'inv_s_dev': inv_s_dev})
        gmap = {k: g for k, g in zip(ctx.keys, grads)}
        a, _out, _keep = marshal_render_args(vol, rays, cfg, per_sample=False, t_rand=t_rand,
                                             bkgd_rays=bkgd_rays, outputs={})
        ba = abi.SoRenderBwdArgs()
        ba.fwd = a
        hold = []
        def gp(name):
            g = gmap.get(name)
            if g is None:
                return None
            g = g.contiguous().float()
            hold.append(g)
            return ptr(g)
        ba.g_depth, ba.g_acc, ba.g_rgb, ba.g_sem = gp('depth'), gp('acc'), gp('rgb'), gp('sem')
        ba.g_weights, ba.g_sdf, ba.g_grad = gp('weights'), gp('sdf'), gp('grad')
        g_sdf_vol = torch.zeros_like(vol.sdf)
        ba.g_sdf_vol = ptr(g_sdf_vol)
        g_feat = None
        if vol.feat is not None and ctx.needs_input_grad[1]:
            g_feat = torch.zeros(vol.feat.shape, dtype=torch.float32, device=vol.feat.device)
            ba.g_feat_vol = ptr(g_feat)
        g_inv_s = torch.zeros(1, device=vol.sdf.device)
        ba.g_inv_s = ptr(g_inv_s)
        mode = cfg.bwd_scatter if cfg.bwd_scatter != 'auto' else os.environ.get('SELFOCC_RB_SCATTER', 'auto')
        if mode == 'binned' or (mode == 'auto' and rays.n_rays * cfg.n_samples >= (1 << 19)):
            need = int(lib().selfocc_render_bwd_ws_bytes(ba))
            if need > 0:
                ws = _scatter_workspace(vol.sdf.device, need)
                ba.scatter_ws, ba.scatter_ws_bytes = ptr(ws), ws.numel()
                hold.append(ws)
            elif mode == 'binned':
                raise RuntimeError("bwd_scatter='binned': the volume / launch is outside the binned scatter's range")
        check(lib().selfocc_render_bwd(ba, current_stream(vol.sdf.device)), "selfocc_render_bwd")
        if g_feat is not None and vol.feat.dtype != torch.float32:
            g_feat = g_feat.to(vol.feat.dtype)
        return (g_sdf_vol, g_feat, g_inv_s.reshape(ctx.inv_s_shape), None, None, None, None, None, None, None, None, None, None)


def render_rays_autograd(vol: SDFVolume, inv_s: torch.Tensor, rays: RaySet, cfg: RenderConfig, *,
                         want_grad_samples=True, t_rand=None, bkgd_rays=None, edges=None):
    """Training-time render: returns the same dict as ``render_rays(per_sample=True)`` with
    depth / acc / rgb / sem / weights / sdf / grad attached to the autograd graph of
    ``vol.sdf``, ``vol.feat`` and ``inv_s``.  ``edges``: see ``_with_edges``; they carry no gradient."""
    cfg, t_rand = _with_edges(cfg, edges, t_rand, rays.n_rays)
    res = _RenderFunction.apply(vol.sdf, vol.feat, inv_s, vol.mapping, vol.n_rgb, vol.n_sem, rays, cfg,
                                t_rand, bkgd_rays, want_grad_samples, vol.sh_deg, vol.sh_act)
    keys = ['depth', 'acc'] + (['rgb'] if vol.n_rgb else []) + (['sem'] if vol.n_sem else []) + ['weights'] + \
        (['sdf', 'grad'] if want_grad_samples else []) + ['ts', 'deltas', 'max_depth', 'nears', 'fars']
    return dict(zip(keys, res))
