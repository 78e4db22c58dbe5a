"""Shared by tests/test_render_bwd_cases_cpu.py and tests/test_render_bwd_sharp_gpu.py: the case table that reaches every
instantiation of render_bwd_kernel / render_fwd_samples_kernel (row type x lane shape (M, WPR) x scatter x mapping kind), the
float64 reference of a case with the mask of its non-comparable rays, and the metrics.

Why a mask.  The trilinear SDF gradient is piece-wise constant per cell, -relu(-cos) and the relu colour have kinks: a sample
within float32 rounding of one of them legitimately falls on either side in two correct evaluations, and everything behind it
on the ray differs.  The kernel marches ALL rays; the upstream gradients are zeroed on the rays that are not comparable, as
decided from the float64 reference alone:
  * any sample within MARGIN voxels of a voxel face (the reference's own positions: starts or mid-points, jitter applied),
  * any sample with |d . grad| < 1e-4,
  * any sample whose relu colour argument is within 1e-4 of 0 (no case here sets clamp_rgb),
and `depth`'s upstream where acc <= 0.05 (a ratio of two rounding-noise sums).  Nothing else is left out.

MARGIN is a few float32 ulps of the largest grid coordinate: 2e-5 voxel for cfg1 (coordinates <= 32, ulp 1.9e-6 .. 3.8e-6),
1e-4 for the upscale scene (coordinates <= 320, ulp 3.1e-5; positions reach 80 m, ulp 7.6e-6 m = 1.9e-5 of a 0.4 m cell).  The CPU
test checks that the float32 and the float64 port put every kept sample into the same cell.  The reference takes the mapping slope
in float64 over SLOPE_EPS metres, below MARGIN on the finest cell (0.4 m: 8e-6 m / 4e-5 m), so it is exact for every kept sample.
"""
import collections
import math

import torch

from oracle import torch_port as tp
from selfocc_amd import abi, sh, synthetic as sy
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume
from nsem_cases import volume as masked_volume
from sh_compose import compose64
from test_render_bwd_gpu import TRAIN_SHAPE_TOL

MARGIN = {'linear': 2e-5, 'linear_upscale': 1e-4}
SLOPE_EPS = 1e-6
FWD_TOL = 1e-4                      # forward outputs: max |got - ref| <= 1e-4 max |ref|, the project's strict rule
C0 = 0.28209479177387814
JITTERS = (abi.JITTER_NONE, abi.JITTER_SINGLE, abi.JITTER_PER_BIN)
MAX_SAMPLES = 100_000               # rays of a case are thinned to about this many samples (float64 autograd stays ~1 s)

Row = collections.namedtuple('Row', 'name n_rgb n_sem sh_deg sh_act bf16', defaults=(0, 0, 0, 'relu', False))
Case = collections.namedtuple('Case', 'sweep row S jitter sample_pos scatter mapping')

SDF, RGB, SEM21 = Row('sdf'), Row('rgb', 3), Row('sem21', 3, 21)
SH2, SH2S = Row('sh2relu', 3, 0, 2, 'relu'), Row('sh2sigmoid', 3, 0, 2, 'sigmoid')
BF4, BF24 = Row('bf16rgb', 3, 0, bf16=True), Row('bf16sem21', 3, 21, bf16=True)
# every row type of so_with_row (csrc/render_row.h): SDF only, 4, unmasked 8 / 24, masked 8 / 8 / 12 (pad) / 12 (full) / 16 / 20 /
# 24, spherical harmonics 4 / 12 / 28 with both activations, bfloat16 4 / 24
ROWS = [SDF, RGB, Row('sem5', 3, 5), SEM21] + [Row(f'sem{n}', 3, n) for n in (2, 4, 6, 9, 13, 14, 20)] + \
    [Row('sh0sigmoid', 3, 0, 0, 'sigmoid'), Row('sh1relu', 3, 0, 1, 'relu'), Row('sh1sigmoid', 3, 0, 1, 'sigmoid'), SH2, SH2S, BF4, BF24]
SEAM_S = (1, 63, 64, 65, 128, 129, 256, 257, 512)      # the edges of the four (M, WPR) instances and of kMaxM
SEAM_BINNED = (64, 65, 129, 257, 512)


def lane_shape(S):
    """(M, WPR) of launch_ray (csrc/render_bwd.hip) for n_samples = S"""
    m = (S + 63) // 64
    return (1, 1) if m <= 1 else (2, 1) if m == 2 else (1, 4) if m <= 4 else (2, 4)


def row_label(row):
    """the so_row instantiation a Row reaches"""
    if row.n_rgb + row.n_sem == 0:
        return 'so_row<0>'
    if row.sh_deg > 0 or row.sh_act == 'sigmoid':
        return f'so_sh_row<{sh.n_basis(row.sh_deg)}>'
    nf = SDFVolume.feat_width(row.n_rgb, row.n_sem)
    masked = row.n_sem not in (0, 5, 21)
    return f"so_row<{nf}{', bf16' if row.bf16 else ''}{', masked' if masked else ''}>"


def _cases():
    out = []
    for ri, row in enumerate((SDF, RGB, SEM21)):
        for i, S in enumerate(SEAM_S):
            for scatter in ('atomic', 'binned') if S in SEAM_BINNED else ('atomic',):
                out.append(Case('seam', row, S, JITTERS[(i + ri) % 3], (i + ri) % 2, scatter, 'linear'))
    for ri, row in enumerate(ROWS):
        for si, S in enumerate((100, 300)):
            for scatter in ('atomic', 'binned'):
                out.append(Case('row', row, S, JITTERS[(ri + si) % 3], ri % 2, scatter, 'linear'))
    for ri, row in enumerate((SDF, RGB, SEM21, SH2S, BF4)):
        for si, S in enumerate((48, 257)):
            for scatter in ('atomic', 'binned'):
                out.append(Case('upscale', row, S, JITTERS[(ri + si) % 3], (ri + si) % 2, scatter, 'linear_upscale'))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.sweep}-{c.row.name}-S{c.S}-{c.scatter}"


def ref_key(c):
    """what the reference of a case depends on: everything but the scatter"""
    return c._replace(scatter='')


def ref_id(c):
    return f"{c.sweep}-{c.row.name}-S{c.S}"


REF_CASES = list(dict.fromkeys(ref_key(c) for c in CASES))


# Where float32 itself is above a fifth of a bound: the float32 port's error for that very case (tests/test_render_bwd_cases_cpu.py::
# test_yardstick, rounded up), written down instead of a wider bound or a dropped case.  The bounds stay what they are for these too
# (the kernels meet them, profiles/render_bwd_sharp_parity.jsonl); what these pairs lack is the factor 5 between float32's own error
# and the bound.  Two causes, both in the number format and not in the case:
#  * `weights` at S >= 257 on cfg1: the error of a weight is that of the SDF difference between neighbouring samples, ~1e-6 absolute
#    (grid coordinates <= 32 carry 2e-6 .. 4e-6 voxel of float32 rounding) whatever S, while max |weights| falls with the bin
#    (0.03 at S = 512): 2.1e-5 .. 3.0e-5 relative, a factor 3.4 .. 5 below the bound;
#  * the upscale scene: grid coordinates reach 320 and positions 80 m, 8 x the rounding of cfg1 per voxel; everything that hangs on
#    the cell fraction (grad -> cos -> weights, the scatter weights) is a factor 3 .. 5 below its bound, `weights` 1.1 .. 3.3.
FLOAT32_ABOVE_A_FIFTH = {
    'seam-sdf-S257': dict(fwd_weights=3.1e-05),
    'seam-rgb-S512': dict(fwd_weights=2.2e-05),
    'seam-sem21-S512': dict(fwd_weights=2.6e-05),
    'row-sem21-S300': dict(fwd_weights=3.1e-05),
    'row-sem4-S300': dict(fwd_weights=2.1e-05),
    'row-sem14-S300': dict(fwd_weights=3.1e-05),
    'row-sh0sigmoid-S300': dict(fwd_weights=2.1e-05),
    'row-sh2sigmoid-S300': dict(fwd_weights=3.1e-05),
    'row-bf16sem21-S300': dict(fwd_weights=2.1e-05),
    'upscale-sdf-S48': dict(sdf_l2=2.3e-05, fwd_weights=6.6e-05),
    'upscale-sdf-S257': dict(fwd_weights=9.4e-05),
    'upscale-rgb-S48': dict(sdf_l2=2.5e-05, sdf_max=4.1e-05, feat_l2=2.2e-05, feat_max=3.3e-05, fwd_weights=3.2e-05, fwd_grad=2.3e-05, fwd_rgb=2.2e-05),
    'upscale-rgb-S257': dict(feat_l2=1.6e-05, fwd_weights=4.5e-05, fwd_grad=2.1e-05),
    'upscale-sem21-S48': dict(sdf_l2=2.1e-05, sdf_max=3.3e-05, feat_l2=2.2e-05, feat_max=4.6e-05, fwd_weights=3.2e-05, fwd_sem=3.1e-05),
    'upscale-sem21-S257': dict(fwd_weights=7.3e-05),
    'upscale-sh2sigmoid-S48': dict(sdf_max=3.7e-05, feat_l2=2.2e-05, feat_max=3.6e-05, fwd_weights=8.3e-05),
    'upscale-sh2sigmoid-S257': dict(sdf_max=3.7e-05, fwd_weights=7.5e-05),
    'upscale-bf16rgb-S48': dict(sdf_l2=2.7e-05, sdf_max=4.0e-05, fwd_weights=6.0e-05, fwd_rgb=2.5e-05),
    'upscale-bf16rgb-S257': dict(fwd_weights=5.0e-05),
}


def bounds(case):
    """per metric.  Backward: TRAIN_SHAPE_TOL of tests/test_render_bwd_gpu.py; forward outputs: FWD_TOL.  bfloat16 storage: g_sdf
    and inv_s keep theirs; the feature gradient comes back ROUNDED to bfloat16 (8 significant bits: <= 2^-9 relative per element,
    so <= 2^-9 in rel-L2, on top of the float32 bound; element-wise 2^-9 of the element, allowed 2^-8 of the largest)."""
    b = dict(TRAIN_SHAPE_TOL)
    b.update({'fwd_' + k: FWD_TOL for k in ('depth', 'acc', 'weights', 'sdf', 'grad', 'rgb', 'sem')})
    if case.row.bf16:
        b['feat_l2'], b['feat_max'] = 2.0 ** -9 + 7e-5, 2.0 ** -8
    return b


# ------------------------------------------------------------------------------------------------------------------------------
# inputs of a case
# ------------------------------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple('Inputs', 'case vol ex cfg t_rand bk G n_ch')


# "If a case cannot meet the cap or the yardstick, change its rays or seed": the seed of the random draws (jitter, background,
# upstream gradients; the candidate rays of the upscale scene) is 3 and cfg1's volume seed 11 unless listed here.  d L / d inv_s is
# ONE number, a cancelling sum over every sample: with some draws the float32 port itself is off by more than a fifth of 1e-3.
DRAW_SEED = {'seam-sdf-S129': 4, 'seam-rgb-S128': 4, 'seam-sem21-S257': 5, 'row-rgb-S100': 5, 'row-sem2-S300': 5, 'row-sem6-S300': 4,
             'row-sem9-S100': 4, 'row-sh1sigmoid-S100': 5,        # inv_s of the float32 port 3.0e-4 .. 3.0e-3 off with seed 3
             'upscale-sdf-S257': 5, 'upscale-rgb-S257': 10, 'upscale-sem21-S48': 5}   # inv_s 2.2e-4 .. 1.5e-3; 0.80 of the rays kept
VOL_SEED = {'seam-rgb-S1': 13}                                     # 0.29 of the kept rays accumulate > 0.05 in volume 11


def _thin(ex, n):
    step = max(1, math.ceil(ex.n_rays / n))
    idx = torch.arange(0, ex.n_rays, step)
    return RaySet(origins=ex.origins[idx].contiguous(), dirs=ex.dirs[idx].contiguous(), dir_norm=ex.dir_norm[idx].contiguous())


def make_inputs(case, draw_seed=None, vol_seed=None):
    row, S = case.row, case.S
    draw_seed = DRAW_SEED.get(ref_id(case), 3) if draw_seed is None else draw_seed
    vol_seed = VOL_SEED.get(ref_id(case), 11) if vol_seed is None else vol_seed
    dt = torch.bfloat16 if row.bf16 else torch.float32
    bkgd = abi.BKGD_PER_RAY if row.n_rgb else abi.BKGD_NONE
    if case.mapping == 'linear_upscale':
        import test_mapping_upscale_gpu as up
        m = GridMeterMapping(**up.HEAD_UPSCALE)
        if row.sh_deg > 0 or row.sh_act == 'sigmoid':
            sdf = up._volume(m, 0, 0, seed=1).sdf
            feat = torch.zeros(*sdf.shape, sh.feat_stride(row.sh_deg))
            feat[..., :sh.n_coef(row.sh_deg)] = torch.randn(*sdf.shape, sh.n_coef(row.sh_deg), generator=torch.Generator().manual_seed(2))
            vol = SDFVolume(m, sdf, feat, 3, 0, row.sh_deg, row.sh_act)
        else:
            vol = up._volume(m, row.n_rgb, row.n_sem, dt, seed=1)
        # the whole volume; under per-bin jitter a box that ends in free space (before the wall at 65 m, below the ceiling at 7 m):
        # in the closed scene no ray reaches its last bin with transmittance left, and the last random value would go unchecked
        aabb = (-60.0, -60.0, -4.0, 60.0, 60.0, 6.0) if case.jitter == abi.JITTER_PER_BIN else up.AABB
        cfg = RenderConfig(aabb=aabb, n_samples=S, inv_s=12.0, sample_pos=case.sample_pos, jitter_mode=case.jitter, bkgd_mode=bkgd)
        ex = up._candidate_rays(max(256, min(1000, MAX_SAMPLES // S)), seed=S + draw_seed - 3)
        up._coverage(m, ex, cfg)
    else:
        if row.sh_deg > 0 or row.sh_act == 'sigmoid':
            vol = sy.make_volume("cfg1", n_rgb=3, sh_deg=row.sh_deg, sh_act=row.sh_act, seed=vol_seed, noise=0.02)
        elif row.n_sem not in (0, 5, 21):
            vol = masked_volume("cfg1", row.n_sem, seed=vol_seed, noise=0.02)              # 64.0 in the pad channels
        else:
            vol = sy.make_volume("cfg1", n_rgb=row.n_rgb, n_sem=row.n_sem, feat_dtype=dt, seed=vol_seed, noise=0.02)
        cfg = sy.make_render_config("cfg1", inv_s=12.0, sample_pos=case.sample_pos, jitter_mode=case.jitter, bkgd_mode=bkgd)
        cfg.n_samples = S
        ex = _thin(sy.explicit_rays(sy.make_rays("cfg1", seed=11)), max(256, min(1000, MAX_SAMPLES // S)))
        # off the lattice: from cfg1's camera (grid d = 1.5) the un-jittered sample i of S = 3 k lies ON the face d = 2 for every
        # ray that leaves through the top (i = k: 60 % of the rays at S = 300)
        ex.origins += torch.tensor([0.031, -0.017, 0.073])
    N = ex.n_rays
    g = torch.Generator().manual_seed(draw_seed)
    t_rand = None if case.jitter == abi.JITTER_NONE else \
        torch.rand(*((N,) if case.jitter == abi.JITTER_SINGLE else (N, S + 1)), generator=g)
    bk = torch.rand(N, 3, generator=g) if row.n_rgb else None
    G = dict(depth=torch.randn(N, generator=g), acc=torch.randn(N, generator=g), weights=torch.randn(N, S, generator=g),
             sdf=0.1 * torch.randn(N, S, generator=g), grad=0.1 * torch.randn(N, S, 3, generator=g))
    if row.n_rgb:
        G['rgb'] = torch.randn(N, 3, generator=g)
    if row.n_sem:
        G['sem'] = torch.randn(N, row.n_sem, generator=g)
    n_ch = (sh.n_coef(row.sh_deg) if row.n_rgb else 0) + row.n_sem
    return Inputs(case, vol, ex, cfg, t_rand, bk, G, n_ch)


# ------------------------------------------------------------------------------------------------------------------------------
# the port of a case in a working dtype: forward, then d (sum_k out_k . G_k) / d (sdf volume, feature volume, inv_s)
# ------------------------------------------------------------------------------------------------------------------------------
def port_forward(inp, dtype=torch.float64, t_rand=None, drop_corner=None):
    """-> (outputs attached to the graph, leaves).  The bfloat16 rows: the port on the bfloat16-ROUNDED features."""
    vol, ex, cfg, row = inp.vol, inp.ex, inp.cfg, inp.case.row
    t_rand = inp.t_rand if t_rand is None else t_rand
    inv_s = torch.tensor(cfg.inv_s, dtype=dtype, requires_grad=True)
    kw = dict(slope_eps=SLOPE_EPS, slope_f64=True, drop_corner=drop_corner)
    if row.sh_deg > 0 or row.sh_act == 'sigmoid':
        sdf, feat = vol.sdf.to(dtype).requires_grad_(True), vol.feat.to(dtype).requires_grad_(True)
        out = compose64(vol.mapping, sdf, feat, row.sh_deg, row.sh_act, ex, cfg, inv_s, t_rand, inp.bk, **kw)
        return out, (sdf, feat, inv_s)
    v = vol.to_reference_layout()[0].to(dtype).requires_grad_(True)                  # (C, H, W, D)
    out = tp.render_port_differentiable(vol.mapping, v, row.n_rgb, row.n_sem, ex.origins.to(dtype), ex.dirs.to(dtype),
                                        ex.dir_norm.to(dtype), cfg, inv_s, None if t_rand is None else t_rand.to(dtype),
                                        None if inp.bk is None else inp.bk.to(dtype), **kw)
    return out, (v, inv_s)


def port_grads(inp, out, leaves, G):
    """-> dict g_sdf (H, W, D), g_feat (H, W, D, n_ch) or None, g_inv_s; float64"""
    dt = leaves[0].dtype
    g = torch.autograd.grad(sum((out[k] * G[k].to(dt)).sum() for k in G), leaves, retain_graph=True)
    if len(leaves) == 3:
        return dict(g_sdf=g[0].double(), g_feat=g[1][..., :inp.n_ch].double(), g_inv_s=g[2].double())
    return dict(g_sdf=g[0][0].double(), g_feat=g[0][1:].permute(1, 2, 3, 0).double() if inp.n_ch else None, g_inv_s=g[1].double())


def sample_positions(inp, out, dtype=torch.float64):
    """the positions the port sampled at: starts or mid-points of its own (jittered) bins"""
    at = out['starts'].detach() if inp.cfg.sample_pos == 0 else (out['starts'].detach() + out['ends'].detach()) / 2
    return inp.ex.origins.to(dtype)[:, None, :] + inp.ex.dirs.to(dtype)[:, None, :] * at[..., None]


def keep_mask(inp, out):
    """rays that keep their upstream gradients, from the float64 reference's outputs alone"""
    assert not inp.cfg.clamp_rgb
    gc = inp.vol.mapping.meter2grid(sample_positions(inp, out))
    fr = gc - torch.floor(gc)
    keep = torch.minimum(fr, 1 - fr).amin(dim=(1, 2)) > MARGIN[inp.case.mapping]
    cos = (inp.ex.dirs.double()[:, None, :] * out['grad'].detach()).sum(-1)
    keep &= (cos.abs() > 1e-4).all(dim=1)
    if inp.case.row.n_rgb and inp.case.row.sh_act == 'relu':
        raw = out['raw'].detach()
        arg = raw + 0.5 if inp.case.row.sh_deg > 0 else C0 * raw + 0.5               # relu(raw + 0.5) / sh0_color
        keep &= (arg.abs() > 1e-4).all(dim=(1, 2))
    return keep


def masked_upstream(inp, out, keep):
    G = {k: v * keep.reshape(-1, *([1] * (v.dim() - 1))).to(v.dtype) for k, v in inp.G.items()}
    G['depth'] = G['depth'] * (out['acc'].detach() > 0.05).float()
    return G


Reference = collections.namedtuple('Reference', 'inp out leaves keep G grads')
_LAST = {}


def reference(case):
    """float64 reference of a case (shared by the atomic and the binned case, and by the tests of one case): computed once, never
    modified.  Only the latest one is held: the tests run grouped by reference."""
    key = ref_key(case)
    if key not in _LAST:
        _LAST.clear()
        inp = make_inputs(case)
        out, leaves = port_forward(inp)
        keep = keep_mask(inp, out)
        G = masked_upstream(inp, out, keep)
        _LAST[key] = Reference(inp, out, leaves, keep, G, port_grads(inp, out, leaves, G))
    return _LAST[key]


# ------------------------------------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def grad_metrics(got, ref):
    """the keys of TRAIN_SHAPE_TOL; got / ref: dicts of port_grads (float64)"""
    m = dict(sdf_l2=_rel_l2(got['g_sdf'], ref['g_sdf']),
             sdf_max=((got['g_sdf'] - ref['g_sdf']).abs().max() / ref['g_sdf'].abs().max()).item(),
             inv_s_rel=(abs(got['g_inv_s'].item() - ref['g_inv_s'].item()) / abs(ref['g_inv_s'].item())))
    if ref['g_feat'] is not None:
        m['feat_l2'] = _rel_l2(got['g_feat'], ref['g_feat'])
        m['feat_max'] = ((got['g_feat'] - ref['g_feat']).abs().max() / ref['g_feat'].abs().max()).item()
    return m


def forward_metrics(got, r):
    """per output: max |got - ref| / max |ref| over the kept rays (`depth`: kept rays with acc > 0.05); got: float64 on the CPU"""
    m = {}
    for k in r.G:
        ref = r.out[k].detach().double()
        sel = r.keep & (r.out['acc'].detach() > 0.05) if k == 'depth' else r.keep
        m['fwd_' + k] = ((got[k].double()[sel] - ref[sel]).abs().max() / ref[sel].abs().max()).item()
    return m
