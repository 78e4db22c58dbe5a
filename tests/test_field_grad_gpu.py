"""GPU: the SDF gradient at arbitrary points (selfocc_field_grad / selfocc_field_grad_bwd, csrc/field_grad.hip; DESIGN.md
section 3.25) and the head's uniform eikonal points (NeuSHead(use_uniform_gradient=True)).

  1. analytic mode equals, bit for bit, the per-sample `grad` / `sdf` the render writes for a sample at that position
     (one-sample explicit rays whose origins are the points), under the linear, two-segment and linear_upscale mappings;
  2. `sdf` equals field_query's value bit for bit, points outside the volume included;
  3. numerical mode equals (0.5 * (s+ - s-)) / delta formed in float32 torch from the entry's own `sdf` at the six shifted points;
  4. both modes against the float64 port, under the tolerance of the per-sample `grad` (tests/test_render_sh_gpu.py);
  5. the backward against float64 autograd, under the d/d sdf_vol bound of tests/test_render_bwd_gpu.py;
  6. the head: eik_grad's rows, EikonalLoss on them, gradients at the tri-planes, no host synchronisation.

Scenes: cfg1 of selfocc_amd/synthetic.py (32 x 32 x 4, 'linear') and the synthetic scene of tests/test_mapping_upscale_gpu.py
under NeuSHead's default 'linear_upscale' mapping and under the two-segment 'linear' mapping of the same extent.
Measured maxima are appended to parity_out/field_grad_parity.jsonl."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from selfocc_amd import abi, occ, synthetic as sy
from selfocc_amd._lib import check, current_stream, lib, ptr
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.occ import field_grad, field_grad_autograd, field_query
from selfocc_amd.render import RaySet, RenderConfig, SDFVolume, render_rays
import test_mapping_upscale_gpu as up

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "field_grad_parity.jsonl")
KINDS = ("linear", "twoseg", "upscale")
VOXEL = {"linear": 12.8 / 31, "twoseg": 0.4, "upscale": 0.4}        # metres per (inner) voxel along x / y


def _log(**row):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(row) + "\n")


@functools.lru_cache(maxsize=None)
def _scene(kind):
    """(volume on the host, volume on the device, box); built once and never written to"""
    if kind == "linear":
        vol, aabb = sy.make_volume("cfg1", seed=3), sy.CONFIGS["cfg1"]["aabb"]
    else:
        m = GridMeterMapping(**(up.HEAD_UPSCALE if kind == "upscale" else up.LINEAR["twoseg"]))
        vol, aabb = up._volume(m, 0, 0, seed=5), up.AABB
    return vol, vol.to(D0), tuple(aabb)


def _points(kind, n, seed, outside=False):
    """n float32 points: a quarter exactly on lattice nodes, a quarter on a cell face (one integer grid coordinate), the rest
    uniform; strictly inside the box — or, ``outside``, the uniform ones from a box 40 % larger along every axis"""
    vol, _, aabb = _scene(kind)
    m = vol.mapping
    g = torch.Generator().manual_seed(seed)
    H, W, D = vol.sdf.shape
    lo, hi = torch.tensor(aabb[:3], dtype=torch.float64), torch.tensor(aabb[3:], dtype=torch.float64)
    k = (n + 3) // 4
    gi = torch.stack([torch.randint(1, s - 1, (2 * k,), generator=g) for s in (H, W, D)], -1).double()
    gi[k:] += torch.rand(k, 3, generator=g, dtype=torch.float64) * 0.98 + 0.01
    gi[k:, 0] = torch.where(torch.arange(k) % 3 == 0, gi[k:, 0].floor(), gi[k:, 0])
    gi[k:, 1] = torch.where(torch.arange(k) % 3 == 1, gi[k:, 1].floor(), gi[k:, 1])
    gi[k:, 2] = torch.where(torch.arange(k) % 3 == 2, gi[k:, 2].floor(), gi[k:, 2])
    gi = torch.minimum(gi, torch.tensor([H - 2.0, W - 2.0, D - 2.0], dtype=torch.float64))
    special = m.grid2meter(gi).float()
    u = torch.rand(n, 3, generator=g, dtype=torch.float64)
    uni = (lo - 0.2 * (hi - lo) + u * 1.4 * (hi - lo)) if outside else (lo + (0.001 + 0.998 * u) * (hi - lo))
    pts = torch.cat([special, uni.float()])[torch.randperm(2 * k + n, generator=g)[:n]] if n > 1 else special[:1]
    if not outside:
        assert ((pts > lo.float()) & (pts < hi.float())).all()
    return pts.contiguous()


def _off_faces(kind, pts, margin):
    """the points at least ``margin`` voxels off every voxel face (float64)"""
    g = _scene(kind)[0].mapping.meter2grid(pts.double())
    fr = g - torch.floor(g)
    return pts[torch.minimum(fr, 1 - fr).amin(1) >= margin].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# 1. analytic mode == the render's per-sample gradient, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("kind", KINDS)
def test_analytic_gradient_is_the_render_sample_gradient_bit_for_bit(hip, kind, n):
    _, vol, aabb = _scene(kind)
    pts = _points(kind, n, seed=n).to(D0)
    g = torch.Generator().manual_seed(7)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = (d / d.norm(dim=-1, keepdim=True)).float().contiguous().to(D0)
    cfg = RenderConfig(aabb=aabb, n_samples=1, near_plane=0.0, sample_pos=abi.SAMPLE_AT_START, jitter_mode=abi.JITTER_NONE)
    ref = render_rays(vol, RaySet(origins=pts, dirs=d, dir_norm=None), cfg, per_sample=True, want_grad_samples=True)
    assert torch.count_nonzero(ref['nears']) == 0               # the box entry is behind the origin: sample 0 starts at t = 0
    got = field_grad(vol, pts)
    assert got['grad'].shape == (n, 3) and got['sdf'].shape == (n,)
    assert torch.equal(got['grad'], ref['grad'][:, 0]) and torch.equal(got['sdf'], ref['sdf'][:, 0])
    assert torch.isfinite(got['grad']).all() and got['grad'].abs().max() > 0
    # without the value, and under autograd: the same bits
    assert torch.equal(field_grad(vol, pts, want_sdf=False)['grad'], got['grad'])
    sdf_p = vol.sdf.clone().requires_grad_(True)
    qa = field_grad_autograd(SDFVolume(vol.mapping, sdf_p, None, 0, 0), pts)
    assert qa['grad'].requires_grad and torch.equal(qa['grad'].detach(), got['grad']) and torch.equal(qa['sdf'].detach(), got['sdf'])


# ---------------------------------------------------------------------------------------------------------------------
# 2. sdf == field_query, inside and outside the volume, both modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_sdf_is_the_field_query_value_bit_for_bit(hip, kind):
    _, vol, aabb = _scene(kind)
    pts = torch.cat([_points(kind, 700, seed=11), _points(kind, 1300, seed=12, outside=True)]).to(D0)
    want = field_query(vol, pts)['sdf']
    assert (want == 0).any() and (want != 0).sum() > 900            # some points are more than a cell outside, half are inside
    assert torch.equal(field_grad(vol, pts)['sdf'], want)
    assert torch.equal(field_grad(vol, pts, mode='numerical', delta=0.01)['sdf'], want)
    assert torch.equal(field_grad(vol, pts, mode='numerical', delta=VOXEL[kind])['sdf'], want)
    assert 'sdf' not in field_grad(vol, pts, mode='numerical', delta=0.01, want_sdf=False)
    empty = field_grad(vol, pts[:0])
    assert empty['grad'].shape == (0, 3) and empty['sdf'].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 3. numerical mode, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _taps(pts, delta32):
    """the six shifted point sets, formed in float32 on the points' device: [(+x, -x), (+y, -y), (+z, -z)]"""
    out = []
    for k in range(3):
        p, q = pts.clone(), pts.clone()
        p[:, k] = pts[:, k] + delta32
        q[:, k] = pts[:, k] - delta32
        out.append((p, q))
    return out


@pytest.mark.parametrize("delta", ["1cm", "voxel"])
@pytest.mark.parametrize("kind", KINDS)
def test_numerical_gradient_is_the_central_difference_of_the_entrys_own_sdf(hip, kind, delta):
    _, vol, aabb = _scene(kind)
    delta = 0.01 if delta == "1cm" else VOXEL[kind]
    d32 = torch.tensor(delta, dtype=torch.float32, device=D0)        # a device tensor: torch divides by it (a host scalar is
    lo, hi = torch.tensor(aabb[:3]), torch.tensor(aabb[3:])          # folded into a multiplication by its reciprocal)
    near = _points(kind, 400, seed=21)
    # ... of which 300 are pushed to within delta of a face of the volume, inside or outside it
    g = torch.Generator().manual_seed(22)
    ax = torch.randint(0, 3, (300,), generator=g)
    face = torch.where(torch.rand(300, generator=g) < 0.5, lo[ax], hi[ax])
    near[torch.arange(300), ax] = face + (torch.rand(300, generator=g) * 2 - 1) * float(delta)
    pts = torch.cat([near, _points(kind, 600, seed=23), _points(kind, 200, seed=24, outside=True)]).to(D0).contiguous()
    got = field_grad(vol, pts, mode='numerical', delta=delta)
    want = torch.stack([(0.5 * (field_grad(vol, p)['sdf'] - field_grad(vol, q)['sdf'])) / d32 for p, q in _taps(pts, d32)], -1)
    assert torch.equal(got['grad'], want)
    assert torch.isfinite(want).all() and (want.abs().amax(1) > 0).sum() > 900
    for n in (1, 7, 8, 9, 63, 65):                                   # teams of 8 lanes: sizes around a team, a wave, a block
        assert torch.equal(field_grad(vol, pts[:n].contiguous(), mode='numerical', delta=delta, want_sdf=False)['grad'], want[:n]), n
    if delta == 0.01:
        cells = [torch.floor(vol.mapping.meter2grid(t.cpu().double())) for pq in _taps(pts, d32) for t in pq]
        # the uniform points' taps mostly share a cell; the node and face points (half of `near` and of the inside set) straddle
        assert sum((cells[2 * k] == cells[2 * k + 1]).all(1).float().mean() for k in range(3)) / 3 > 0.4
    else:
        cells = [torch.floor(vol.mapping.meter2grid(t.cpu().double())) for t in _taps(pts, d32)[0]]
        assert (cells[0] != cells[1]).any(1).float().mean() > 0.5             # the taps cross cells (the outer cells are wider)


# ---------------------------------------------------------------------------------------------------------------------
# 4. both modes against float64
# ---------------------------------------------------------------------------------------------------------------------
def _port64(kind, vol64, xyz64):
    """float64 (values (n), metre gradient (n, 3)) of oracle.torch_port.trilinear_explicit, slope in float64"""
    vals, grad = tp.trilinear_explicit(_scene(kind)[0].mapping.mapping, vol64[None], xyz64, slope_f64=True)
    return vals[:, 0], grad


def _numerical64(kind, vol64, pts, delta):
    """central differences in float64 at the taps the entry defines: x_k +- delta formed in float32"""
    d32 = torch.tensor(delta, dtype=torch.float32)
    cols = []
    for p, q in _taps(pts, d32):
        cols.append(0.5 * (_port64(kind, vol64, p.double())[0] - _port64(kind, vol64, q.double())[0]) / d32.double())
    return torch.stack(cols, -1)


# The tolerance of the per-sample `grad` in tests/test_render_sh_gpu.py / test_mapping_upscale_gpu.py: rtol 2e-3, atol 2e-4.
# Numerical mode divides the float32 rounding of two SDF values by 2 delta, so a case is listed where that stays below the
# tolerance by the formats alone: a grid coordinate g carries ~ulp(g) of rounding, i.e. ulp(g) x (metres per voxel) of SDF:
# 2e-6 x 0.41 m on the 32-cell grid (over 0.02 m: 4e-5), 3e-5 x 0.4 m on the 321-cell grids (over 0.02 m: 6e-4 — beyond the
# tolerance whatever the kernel does — over 0.8 m: 1.5e-5).  So: 1 cm on cfg1 only, one voxel everywhere.
FP64_CASES = [(k, 'analytic', None) for k in KINDS] + [('linear', 'numerical', 0.01)] + [(k, 'numerical', VOXEL[k]) for k in KINDS]


@pytest.mark.parametrize("kind,mode,delta", FP64_CASES, ids=[f"{k}-{m}-{d}" for k, m, d in FP64_CASES])
def test_gradient_vs_float64_port(hip, kind, mode, delta):
    vol_h, vol, _ = _scene(kind)
    # the analytic gradient is discontinuous across voxel faces: the points keep 4e-3 voxel off them, as the render tests do
    pts = _off_faces(kind, torch.cat([_points(kind, 1500, seed=31), _points(kind, 500, seed=32, outside=True)]), 4e-3)
    assert pts.shape[0] >= 1200, pts.shape
    vol64 = vol_h.sdf.double()
    got = field_grad(vol, pts.to(D0), mode=mode, delta=delta)
    want_sdf, want = _port64(kind, vol64, pts.double())
    if mode == 'numerical':
        want = _numerical64(kind, vol64, pts, delta)
    err = (got['grad'].cpu().double() - want).abs()
    e_sdf = (got['sdf'].cpu().double() - want_sdf).abs().max().item()
    worst = (err / (2e-4 + 2e-3 * want.abs())).max().item()
    print(f"\n[field_grad vs float64] {kind} {mode} delta {delta}: n {pts.shape[0]} max |grad err| {err.max().item():.3e} "
          f"(max |grad| {want.abs().max().item():.3f}) worst err / tolerance {worst:.3f}; max |sdf err| {e_sdf:.3e}")
    _log(test="gradient_vs_float64_port", kind=kind, mode=mode, delta=delta, n=int(pts.shape[0]), max_abs_err=err.max().item(),
         max_abs_grad=want.abs().max().item(), worst_err_over_tolerance=worst, max_abs_sdf_err=e_sdf)
    assert want.abs().max() > 0.5
    assert torch.allclose(got['grad'].cpu().double(), want, rtol=2e-3, atol=2e-4)
    assert torch.allclose(got['sdf'].cpu().double(), want_sdf, rtol=2e-3, atol=2e-4)


# ---------------------------------------------------------------------------------------------------------------------
# 5. backward against float64 autograd
# ---------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bwd_points(kind):
    """off-face points inside and outside the volume, 150 of them three times over (repeated points accumulate)"""
    pts = _off_faces(kind, torch.cat([_points(kind, 900, seed=41), _points(kind, 300, seed=42, outside=True)]), 4e-3)
    return torch.cat([pts, pts[:150], pts[:150]]).contiguous()


def _entry_bwd(vol, pts, mode, delta, g_sdf, g_grad):
    """selfocc_field_grad_bwd itself, so that either upstream can be NULL (autograd hands zeros, never None)"""
    a = occ._grad_args(vol.mapping, vol.sdf, pts, mode, delta)
    out = torch.zeros_like(vol.sdf)
    check(lib().selfocc_field_grad_bwd(a, ptr(g_sdf), ptr(g_grad), ptr(out), current_stream(pts.device)), "selfocc_field_grad_bwd")
    return out


BWD_CASES = [(k, 'analytic', None) for k in KINDS] + [('linear', 'numerical', 0.01), ('linear', 'numerical', VOXEL['linear']),
                                                       ('upscale', 'numerical', 0.01), ('twoseg', 'numerical', VOXEL['twoseg'])]


@pytest.mark.parametrize("kind,mode,delta", BWD_CASES, ids=[f"{k}-{m}-{d}" for k, m, d in BWD_CASES])
def test_backward_vs_float64_autograd(hip, kind, mode, delta):
    vol_h, vol, _ = _scene(kind)
    pts = _bwd_points(kind)
    n = pts.shape[0]
    gen = torch.Generator().manual_seed(5)
    gs, gg = torch.randn(n, generator=gen), torch.randn(n, 3, generator=gen)

    vol64 = vol_h.sdf.double().requires_grad_(True)
    want_sdf, want_grad = _port64(kind, vol64, pts.double())
    if mode == 'numerical':
        want_grad = _numerical64(kind, vol64, pts, delta)
    r_s, = torch.autograd.grad((want_sdf * gs.double()).sum(), vol64, retain_graph=True)
    r_g, = torch.autograd.grad((want_grad * gg.double()).sum(), vol64)
    assert r_s.abs().max() > 0 and r_g.abs().max() > 0

    # through autograd, both upstreams at once
    sdf_p = vol.sdf.clone().requires_grad_(True)
    q = field_grad_autograd(SDFVolume(vol.mapping, sdf_p, None, 0, 0), pts.to(D0), mode=mode, delta=delta)
    ((q['sdf'] * gs.to(D0)).sum() + (q['grad'] * gg.to(D0)).sum()).backward()
    e_both = _rel_l2(sdf_p.grad.cpu().double(), r_s + r_g)
    # the entry with either upstream alone (the other NULL), and with none / zeros
    p, s, g3 = pts.to(D0), gs.to(D0), gg.to(D0)
    e_g = _rel_l2(_entry_bwd(vol, p, mode, delta, None, g3).cpu().double(), r_g)
    e_s = _rel_l2(_entry_bwd(vol, p, mode, delta, s, None).cpu().double(), r_s)
    print(f"\n[field_grad bwd vs float64] {kind} {mode} delta {delta}: n {n} rel L2 both {e_both:.3e} g_grad alone {e_g:.3e} "
          f"g_sdf alone {e_s:.3e}")
    _log(test="backward_vs_float64_autograd", kind=kind, mode=mode, delta=delta, n=n, rel_l2_both=e_both, rel_l2_g_grad=e_g,
         rel_l2_g_sdf=e_s)
    assert e_both < 2e-3, f"d/d sdf_vol rel L2 {e_both:.3e}"
    assert e_g < 2e-3, f"d/d sdf_vol (g_grad alone) rel L2 {e_g:.3e}"
    assert e_s < 2e-3, f"d/d sdf_vol (g_sdf alone) rel L2 {e_s:.3e}"
    assert (sdf_p.grad.cpu().double() - (r_s + r_g)).abs().max() < 2e-2 * (r_s + r_g).abs().max()
    assert torch.count_nonzero(_entry_bwd(vol, p, mode, delta, None, None)) == 0
    assert torch.count_nonzero(_entry_bwd(vol, p, mode, delta, torch.zeros_like(s), torch.zeros_like(g3))) == 0
    # repeated points accumulate: the 150 points given three times weigh three times
    first = _entry_bwd(vol, p[:150].contiguous(), mode, delta, s[:150].contiguous(), g3[:150].contiguous())
    thrice = _entry_bwd(vol, torch.cat([p[:150]] * 3).contiguous(), mode, delta, torch.cat([s[:150]] * 3).contiguous(),
                        torch.cat([g3[:150]] * 3).contiguous())
    assert _rel_l2(thrice.double(), 3 * first.double()) < 1e-6
    # positions carry no gradient
    xyz = pts.to(D0).requires_grad_(True)
    assert not field_grad_autograd(vol, xyz, mode=mode, delta=delta)['grad'].requires_grad


def test_field_gradient_method_follows_forward_sdfnetwork(hip):
    """SDFField.gradient: attached to the volume exactly when forward_sdfnetwork is; numerical = the operator's numerical mode"""
    from test_head_gpu import make_head, make_inputs
    head = make_head(color_dims=0, return_sem=False, render_bkgd='white', return_second_grad=False)
    rep, _, _ = make_inputs()
    field = head.model.field
    pts = _points("linear", 300, seed=51).to(D0)
    vol = field.pre_compute_density_color(rep)
    assert vol.sdf.requires_grad
    g, s = field.gradient(pts), field.forward_sdfnetwork(pts)
    assert g.requires_grad and s.requires_grad and g.shape == (300, 3)
    plain = SDFVolume(vol.mapping, vol.sdf.detach(), None, 0, 0)
    assert torch.equal(g.detach(), field_grad(plain, pts)['grad'])
    assert torch.equal(field.gradient(pts, numerical=True, delta=0.05).detach(), field_grad(plain, pts, 'numerical', 0.05)['grad'])
    with torch.no_grad():
        assert not field.gradient(pts).requires_grad and not field.forward_sdfnetwork(pts).requires_grad
        assert torch.equal(field.gradient(pts), g.detach())
    with pytest.raises(ValueError, match="delta"):
        field.gradient(pts, numerical=True)
    with pytest.raises(ValueError, match="delta"):
        field.gradient(pts, delta=0.01)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the head
# ---------------------------------------------------------------------------------------------------------------------
N_UNI, RAYS, S, CAMS = 500, 60, 32, 2


def _forward(head, seed=1):
    from test_head_gpu import make_inputs
    os.environ['eval'] = 'false'
    rep, metas, imgs = make_inputs()
    torch.manual_seed(seed)
    np.random.seed(0)
    return head(rep, metas, global_iter=0), rep


def _same(a, b, key):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and torch.equal(a, b), key
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y, key)
    else:
        assert a is b or a == b, key


@pytest.mark.parametrize("delta", [None, 0.05])
def test_head_eik_grad_is_the_ray_samples_then_the_uniform_points(hip, delta):
    from test_head_gpu import make_head
    kw = dict(return_uniform_sdf=True, return_sample_sdf=True)
    off, _ = _forward(make_head(**kw).train())
    head = make_head(use_uniform_gradient=True, nbr_gradient_points=N_UNI, sample_gradient=True, uniform_gradient_delta=delta, **kw).train()
    on, rep = _forward(head)
    n_ray = CAMS * RAYS * S
    assert off['eik_grad'].shape == (n_ray, 3) and on['eik_grad'].shape == (n_ray + N_UNI, 3)
    assert torch.equal(on['eik_grad'][:n_ray], off['eik_grad'])
    assert set(on) == set(off)
    for k in off:                       # every other output: the knob moves no random stream (uniform_sdf draws its shift too)
        if k != 'eik_grad':
            _same(on[k], off[k], k)
    # the uniform rows: the field's gradient at points of the box, finite and not all alike
    uni = on['eik_grad'][n_ray:]
    assert torch.isfinite(uni).all() and uni.abs().amax(1).gt(0).float().mean() > 0.9 and uni.std(0).min() > 0
    # the draw is torch.rand in roi_aabb, after every other draw of the call: replayed here from the generator's state
    torch.manual_seed(1)
    np.random.seed(0)
    from test_head_gpu import make_inputs
    rep2, metas, _ = make_inputs()
    on2 = head(rep2, metas, global_iter=0)
    assert torch.equal(on2['eik_grad'], on['eik_grad'])

    # EikonalLoss takes the concatenated tensor through its HIP path
    from selfocc_amd.loss.simple import EikonalLoss
    eg = on['eik_grad']
    loss = EikonalLoss(weight=1.0).eikonal(eg)
    ref = ((eg.detach().double().norm(2, dim=-1) - 1) ** 2).mean()
    assert loss.dtype == torch.float32 and abs(loss.double().item() - ref.item()) <= 2e-6 * abs(ref.item())
    # ... of the uniform rows alone, the backward reaches the tri-planes
    (((uni.norm(2, dim=-1) - 1) ** 2).mean()).backward(retain_graph=True)
    for r in rep:
        assert r.grad is not None and torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0
        r.grad = None
    loss.backward()
    for r in rep:
        assert r.grad is not None and torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0


def test_head_uniform_points_alone_when_sample_gradient_is_off(hip):
    from test_head_gpu import make_head
    head = make_head(use_uniform_gradient=True, nbr_gradient_points=N_UNI, sample_gradient=False).train()
    asked = []
    import selfocc_amd.model.head.neus_head as nh
    real = nh.render_rays_autograd
    nh.render_rays_autograd = lambda *a, **k: (asked.append(k.get('want_grad_samples')), real(*a, **k))[1]
    try:
        on, rep = _forward(head)
    finally:
        nh.render_rays_autograd = real
    assert asked == [False]                                  # the render is not asked for per-sample gradients
    assert on['eik_grad'].shape == (N_UNI, 3) and on['eik_grad'].requires_grad
    # the rows are gradients of THIS volume: a loss on them reaches the planes
    ((on['eik_grad'].norm(2, dim=-1) - 1) ** 2).mean().backward()
    for r in rep:
        assert r.grad is not None and torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0
    # without autograd the knob does nothing: the ray-sample gradients, as ever
    with torch.no_grad():
        quiet, _ = _forward(head)
    assert quiet['eik_grad'].shape == (CAMS * RAYS * S, 3)


def test_head_knob_off_ignores_the_companion_knobs(hip):
    """use_uniform_gradient=False: every key and value of forward() is what it is without the three other knobs"""
    from test_head_gpu import make_head
    base, _ = _forward(make_head(sample_gradient=False, return_uniform_sdf=True).train())
    assert set(base) == {'ms_depths', 'ms_colors', 'ms_accs', 'ms_fars', 'ms_rays', 'origin', 'direction', 'direction_norm',
                         'ray_indices', 'weights', 'ts', 'deltas', 'eik_grad', 'uniform_sdf', 'ms_max_depths', 'second_grad', 'sem'}
    assert base['eik_grad'].shape == (CAMS * RAYS * S, 3)
    for kw in (dict(sample_gradient=True), dict(sample_gradient=True, nbr_gradient_points=9, uniform_gradient_delta=0.01, calculate_online=True)):
        other, _ = _forward(make_head(return_uniform_sdf=True, **kw).train())
        assert set(other) == set(base)
        for k in base:
            _same(other[k], base[k], k)


def test_head_training_step_with_uniform_points_never_synchronises(hip):
    from test_head_gpu import make_head, make_inputs
    from test_head_sh_gpu import no_sync
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    os.environ['eval'] = 'false'
    loss_fn = OPENOCC_LOSS.build(dict(type='MultiLoss', loss_cfgs=[dict(type='EikonalLoss', weight=0.1),
                                                                   dict(type='SecondGradLoss', weight=0.01)]))
    for delta in (None, 0.05):
        head = make_head(use_uniform_gradient=True, nbr_gradient_points=N_UNI, sample_gradient=True, uniform_gradient_delta=delta,
                         ray_sample_mode='fixed', render_bkgd='white').train()
        rep, metas, _ = make_inputs()
        total, _ = loss_fn(dict(head(rep, metas, global_iter=0), metas=metas))      # warm-up: constants are uploaded once
        total.backward()
        for r in rep:
            r.grad = None
        with no_sync():
            out = head(rep, metas, global_iter=1)
            total, parts = loss_fn(dict(out, metas=metas))
            total.backward()
        assert out['eik_grad'].shape == (CAMS * RAYS * S + N_UNI, 3)
        assert torch.isfinite(total).all() and float(parts['EikonalLoss']) > 0
        for r in rep:
            assert r.grad is not None and torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0
