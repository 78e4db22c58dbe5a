"""GPU: NeuS hierarchical up-sampling (selfocc_render_upsample) and explicit edges in the march
(SO_JITTER_EDGES), from the kernel up to the head.

Scenes, rays and the comparison rule: tests/upsample_cases.py.  The sampler is compared with the float64 host reference by
the SHARE of edges that are off by more than TAU = 1e-6: at most 3 x p32, the share of the float32 host reference itself,
measured in the same test (tests/test_upsample_cpu.py lists p32 per case).  Every case prints its shares and appends them to
upsample_parity.jsonl.
"""
import dataclasses
import json
import os

import pytest
import torch

from oracle.torch_port import sh0_color, trilinear_explicit
from selfocc_amd import abi
from selfocc_amd.occ import field_query
from selfocc_amd.render import (RaySet, RenderConfig, median_depth_reference, render_median_depth, render_rays,
                                render_rays_autograd, uniform_edges_reference, upsample_edges)
import render_bwd_cases as rc
import upsample_cases as uc
from test_render_bwd_gpu import LOG as TRAIN_SHAPE_LOG, TRAIN_SHAPE_TOL

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(TRAIN_SHAPE_LOG), "upsample_parity.jsonl")
INV_S = 20.0


def _dev(rays):
    c = lambda t: None if t is None else t.to(D0)
    return dataclasses.replace(rays, origins=c(rays.origins), dirs=c(rays.dirs), dir_norm=c(rays.dir_norm), img2lidar=c(rays.img2lidar))


def _log(rec):
    print("\n" + json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


class Scene:
    """one volume kind: the volume, the two ray sets on the host (the lattice also as the explicit rays the kernels make of it)
    and on the device, and the collider's nears / fars AS A KERNEL WRITES THEM (render_rays), once"""

    def __init__(self, kind):
        self.kind = kind
        self.vol, self.aabb = uc.make_volume(kind)
        self.vol_dev = self.vol.to(D0)
        lattice = uc.make_pixel_rays(kind)
        self.host = [uc.make_explicit_rays(kind), uc.lattice_as_explicit(lattice)]
        self.dev = [_dev(self.host[0]), _dev(lattice)]
        self.cfg = RenderConfig(aabb=self.aabb, n_samples=8, inv_s=INV_S, exact=True)
        self.nf = []
        for r in self.dev:
            o = render_rays(self.vol_dev, r, self.cfg)
            self.nf.append((o['nears'].cpu(), o['fars'].cpu()))


_SCENES = {}


def scene(kind):
    if kind not in _SCENES:
        _SCENES[kind] = Scene(kind)
    return _SCENES[kind]


def _sampling(s, i, size, jitter, with_u):
    """(cfg, t_rand, u_rand) of ray set i, draws on the host"""
    t_rand, u_rand = uc.draws(s.host[i].n_rays, size[0], size[2], jitter, with_u)
    return dataclasses.replace(s.cfg, n_samples=size[0], jitter_mode=jitter), t_rand, u_rand


def _launch(s, i, size, jitter=abi.JITTER_NONE, with_u=False, rays=None):
    cfg, t_rand, u_rand = _sampling(s, i, size, jitter, with_u)
    up = lambda t: None if t is None else t.to(D0)
    return upsample_edges(s.vol_dev, s.dev[i] if rays is None else rays, cfg, size[1], size[2], uc.BASE_VARIANCE,
                          t_rand=up(t_rand), u_rand=up(u_rand))


# ---- 1. the sampler against the float64 reference ------------------------------------------------------------------
def test_the_collider_and_the_lattice_rays_are_what_the_reference_is_given(hip):
    """the reference runs on explicit rays and on nears / fars: they must be the kernel's own, bit for bit"""
    for kind in uc.MAPPINGS:
        s = scene(kind)
        for i in range(2):
            n, f = uc.collide(s.host[i], s.aabb)
            assert torch.equal(n, s.nf[i][0]) and torch.equal(f, s.nf[i][1]), (kind, i)
        as_explicit = _launch(s, 1, (16, 16, 4), abi.JITTER_SINGLE, True, rays=_dev(s.host[1]))
        assert torch.equal(as_explicit, _launch(s, 1, (16, 16, 4), abi.JITTER_SINGLE, True)), kind
        assert int(((s.nf[0][1] - s.nf[0][0]) < 1e-5).sum()) >= uc.N_MISS        # rays that miss the box are in the scene


@pytest.mark.parametrize("jitter,with_u", [(abi.JITTER_NONE, False), (abi.JITTER_SINGLE, True)], ids=["plain", "jitter_u"])
@pytest.mark.parametrize("size", uc.SIZES[:4], ids=lambda z: "S%d_M%d_K%d" % z)
@pytest.mark.parametrize("kind", list(uc.MAPPINGS))
def test_sampler_vs_the_float64_reference(hip, kind, size, jitter, with_u):
    s = scene(kind)
    S0, M, K = size
    s_tot = S0 + K * (M // K)
    got, r64, r32, rpert = [], [], [], []
    for i in range(2):
        cfg, t_rand, u_rand = _sampling(s, i, size, jitter, with_u)
        e = _launch(s, i, size, jitter, with_u).cpu()
        assert e.shape == (s.host[i].n_rays, s_tot + 1) and e.dtype == torch.float32 and torch.isfinite(e).all()
        assert (e[:, 1:] >= e[:, :-1]).all(), "edges must be non-decreasing (rays that miss the box included)"
        start = uniform_edges_reference(S0, jitter, t_rand, e.shape[0])
        assert torch.equal(e[:, 0], start[:, 0]) and torch.equal(e[:, -1], start[:, -1]), "the first and the last edge are exact"
        got.append(e)
        ref = lambda dtype, bv=uc.BASE_VARIANCE: uc.reference(s.vol, s.host[i], *s.nf[i], size, dtype, jitter, t_rand, u_rand, bv)
        r64.append(ref(torch.float64))
        r32.append(ref(torch.float32))
        rpert.append(ref(torch.float32, uc.BASE_VARIANCE * uc.PERTURB))
    got, r64, r32, rpert = (torch.cat(x) for x in (got, r64, r32, rpert))
    share, worst = uc.share_off(got, r64)
    p32, worst32 = uc.share_off(r32, r64)
    pert, _ = uc.share_off(rpert, r64)
    _log(dict(test="sampler", kind=kind, size=list(size), jitter=jitter, u_rand=with_u, rays=got.shape[0], share=share,
              p32=p32, cap=uc.FACTOR * p32, worst=worst, worst32=worst32, perturbed=pert))
    assert pert > uc.FACTOR * p32, "the inputs must give the rule its margin: base_variance x 1.001 has to fail it"
    assert share <= uc.FACTOR * p32, (share, p32)


@pytest.mark.parametrize("jitter", [abi.JITTER_NONE, abi.JITTER_SINGLE, abi.JITTER_PER_BIN], ids=["plain", "single", "per_bin"])
def test_nothing_to_add_gives_the_start_edges(hip, jitter):
    """(64, 3, 4): m = 0, no step runs"""
    s = scene('linear')
    for i in range(2):
        cfg, t_rand, _ = _sampling(s, i, (64, 3, 4), jitter, False)
        e = _launch(s, i, (64, 3, 4), jitter).cpu()
        assert torch.equal(e, uniform_edges_reference(64, jitter, t_rand, s.host[i].n_rays))
        if jitter == abi.JITTER_NONE:
            assert torch.equal(e, uc.uniform_edges(64, s.host[i].n_rays))


# ---- 2. determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64, 4), (200, 56, 4)], ids=lambda z: "S%d_M%d_K%d" % z)
def test_two_launches_give_identical_bits(hip, size):
    for kind in uc.MAPPINGS:
        s = scene(kind)
        for i in range(2):
            a, b = _launch(s, i, size, abi.JITTER_SINGLE, True), _launch(s, i, size, abi.JITTER_SINGLE, True)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_sizes_are_refused_by_name(hip):
    s = scene('linear')
    cfg = dataclasses.replace(s.cfg, n_samples=201)
    with pytest.raises(ValueError, match="257"):
        upsample_edges(s.vol_dev, s.dev[0], cfg, 56, 4, 64.0)
    with pytest.raises(ValueError, match="num_up_sample_steps = 9"):
        upsample_edges(s.vol_dev, s.dev[0], s.cfg, 18, 9, 64.0)
    with pytest.raises(RuntimeError, match="base_variance"):
        upsample_edges(s.vol_dev, s.dev[0], s.cfg, 16, 4, 0.0)


# ---- 3. plumbing: uniform edges are the JITTER_NONE launch, bit for bit ------------------------------------------------
PER_RAY = ('depth', 'acc', 'rgb', 'sem', 'max_depth', 'nears', 'fars')
PER_SAMPLE = ('weights', 'ts', 'deltas', 'sdf', 'grad')


@pytest.mark.parametrize("S", [5, 64, 129, 256])
@pytest.mark.parametrize("kind", list(uc.MAPPINGS))
def test_uniform_edges_reproduce_the_plain_exact_launch(hip, kind, S):
    s = scene(kind)
    vol = uc.make_volume(kind, n_feat=8)[0].to(D0)
    for i in range(2):
        rays, N = s.dev[i], s.host[i].n_rays
        cfg = dataclasses.replace(s.cfg, n_samples=S, exact=True, sample_pos=abi.SAMPLE_AT_MID if S == 129 else abi.SAMPLE_AT_START)
        wrong = dataclasses.replace(cfg, n_samples=7, jitter_mode=abi.JITTER_SINGLE)     # edges= must override both fields
        edges = uc.uniform_edges(S, N).to(D0)                                            # torch.linspace
        for per_sample in (False, True):
            want = render_rays(vol, rays, cfg, per_sample=per_sample, want_grad_samples=per_sample)
            got = render_rays(vol, rays, wrong, per_sample=per_sample, want_grad_samples=per_sample, edges=edges)
            keys = PER_RAY + (PER_SAMPLE if per_sample else ())
            assert set(got) == set(want) == set(keys)
            for k in keys:
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (kind, i, S, per_sample, k)
        m_want = render_median_depth(vol, rays, cfg, want_index=True)
        m_got = render_median_depth(vol, rays, wrong, want_index=True, edges=edges)
        assert torch.equal(m_got['median_index'], m_want['median_index']) and torch.equal(m_got['median_depth'], m_want['median_depth'])


# ---- 4. non-uniform edges from the sampler ---------------------------------------------------------------------------
def _ulp_apart(a, b):
    """largest distance in units of the last place between two float32 tensors of one sign pattern"""
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("size", [(64, 64, 4), (5, 6, 3)], ids=lambda z: "S%d_M%d_K%d" % z)
@pytest.mark.parametrize("kind", list(uc.MAPPINGS))
def test_the_march_composites_the_samplers_edges(hip, kind, size):
    s = scene(kind)
    vol = uc.make_volume(kind, n_feat=8)[0].to(D0)
    i = 0                                                                     # explicit rays: the positions are known on the host
    rays_h, (nears, fars) = s.host[i], s.nf[i]
    edges = _launch(s, i, size, abi.JITTER_SINGLE, True)
    S = edges.shape[1] - 1
    out = {k: v.cpu() for k, v in render_rays(vol, s.dev[i], s.cfg, per_sample=True, want_grad_samples=True, edges=edges).items()}
    assert out['weights'].shape == (rays_h.n_rays, S)
    b = edges.cpu()
    t = b * fars[:, None] + (1.0 - b) * nears[:, None]                        # so_edge's last line, float32
    dn = rays_h.dir_norm[:, None]
    assert _ulp_apart(out['ts'], ((t[:, :-1] + t[:, 1:]) / 2.0) / dn) <= 1
    assert _ulp_apart(out['deltas'], (t[:, 1:] - t[:, :-1]) / dn) <= 1
    pos = rays_h.origins[:, None, :] + rays_h.dirs[:, None, :] * t[:, :-1, None]
    q = field_query(s.vol_dev, pos.reshape(-1, 3).to(D0))['sdf'].cpu().reshape(-1, S)
    assert torch.equal(out['sdf'], q), "sdf at the samples is field_query at the sample starts"
    # the float64 composite of the kernel's own sdf / grad / deltas
    sdf, grad, delta = out['sdf'].double(), out['grad'].double(), (out['deltas'] * dn).double()
    cos = (rays_h.dirs.double()[:, None, :] * grad).sum(-1).clamp(max=0.0)
    prev, nxt = torch.sigmoid((sdf - cos * delta * 0.5) * INV_S), torch.sigmoid((sdf + cos * delta * 0.5) * INV_S)
    alpha = ((prev - nxt + 1e-5) / (prev + 1e-5)).clip(0.0, 1.0)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-7], 1), 1)[:, :-1]
    ref = alpha * trans
    d = (out['weights'].double() - ref).abs()
    assert (d <= 1e-4 + 2e-3 * ref).double().mean() > 0.9995 and d.max() < 5e-3, (d.max(), kind, size)
    assert ref.sum(-1).max() > 0.5, "some rays must hit a surface"
    med = render_median_depth(vol, s.dev[i], s.cfg, edges=edges, want_index=True)
    want_d, want_j = median_depth_reference(out['weights'], out['ts'])
    assert torch.equal(med['median_index'].cpu(), want_j) and torch.equal(med['median_depth'].cpu(), want_d)


# ---- 5. backward ----------------------------------------------------------------------------------------------------
def _port(vol, rays, nears, fars, edges, inv_s, dtype=torch.float64):
    """compact float64 port of the render with the edges as constants -> (outputs, leaves (volume (C, H, W, D), inv_s))"""
    v = vol.to_reference_layout()[0].to(dtype).requires_grad_(True)
    inv = torch.tensor(inv_s, dtype=dtype, requires_grad=True)
    o, d, dn = rays.origins.to(dtype), rays.dirs.to(dtype), rays.dir_norm.to(dtype)
    b = edges.to(dtype)
    t = b * fars.to(dtype)[:, None] + (1 - b) * nears.to(dtype)[:, None]
    starts, ends = t[:, :-1], t[:, 1:]
    S = starts.shape[1]
    deltas, mids = ends - starts, (starts + ends) / 2
    pos = o[:, None, :] + d[:, None, :] * starts[..., None]
    h, grad = trilinear_explicit(vol.mapping, v, pos.reshape(-1, 3), rc.SLOPE_EPS, True)
    sdf, grad = h[:, 0].reshape(-1, S), grad.reshape(-1, S, 3)
    cos = -torch.relu(-(d[:, None, :] * grad).sum(-1))
    prev, nxt = torch.sigmoid((sdf - cos * deltas * 0.5) * inv), torch.sigmoid((sdf + cos * deltas * 0.5) * inv)
    alpha = ((prev - nxt + 1e-5) / (prev + 1e-5)).clip(0.0, 1.0)
    w = alpha * torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-7], 1), 1)[:, :-1]
    acc = w.sum(-1)
    out = dict(depth=(w * mids).sum(-1) / (acc + 1e-10) / dn, acc=acc, weights=w, sdf=sdf, grad=grad, starts=starts, ends=ends,
               raw=h[:, 1:4].reshape(-1, S, 3), rgb=(w[..., None] * sh0_color(h[:, 1:4]).reshape(-1, S, 3)).sum(-2))
    if vol.n_sem:
        out['sem'] = (w[..., None] * torch.softmax(h[:, 4:4 + vol.n_sem], -1).reshape(-1, S, vol.n_sem)).sum(-2)
    return out, (v, inv)


def _keep(vol, rays, out):
    """rays that keep their upstream gradients (tests/render_bwd_cases.py keep_mask): no sample within a few float32 ulps of a
    voxel face, of cos = 0 or of the relu colour's kink, decided from the float64 port alone"""
    pos = rays.origins.double()[:, None, :] + rays.dirs.double()[:, None, :] * out['starts'].detach()[..., None]
    gc = vol.mapping.meter2grid(pos)
    fr = gc - torch.floor(gc)
    keep = torch.minimum(fr, 1 - fr).amin(dim=(1, 2)) > rc.MARGIN['linear']
    keep &= ((rays.dirs.double()[:, None, :] * out['grad'].detach()).sum(-1).abs() > 1e-4).all(dim=1)
    return keep & ((rc.C0 * out['raw'].detach() + 0.5).abs() > 1e-4).all(dim=(1, 2))


def _device_grads(vol, rays, cfg, G, edges):
    v = vol.to(D0)
    sdf_p, feat_p = v.sdf.clone().requires_grad_(True), v.feat.clone().requires_grad_(True)
    inv_s = torch.tensor([cfg.inv_s], device=D0, requires_grad=True)
    out = render_rays_autograd(v.with_tensors(sdf_p, feat_p), inv_s, rays, cfg, want_grad_samples=True, edges=edges)
    sum((out[k] * G[k].to(D0)).sum() for k in G).backward()
    n_ch = vol.n_rgb + vol.n_sem
    return dict(g_sdf=sdf_p.grad.cpu().double(), g_inv_s=inv_s.grad.cpu().double()[0], g_feat=feat_p.grad.cpu().double()[..., :n_ch]), out


_BWD_REF = {}


def _bwd_reference(kind, n_feat):
    """float64 reference of the backward case: edges from the sampler ((16, 16, 4), jittered), computed once"""
    key = (kind, n_feat)
    if key not in _BWD_REF:
        s = scene(kind)
        vol = uc.make_volume(kind, n_feat=n_feat)[0]
        rays, (nears, fars) = s.host[0], s.nf[0]
        edges = _launch(s, 0, (16, 16, 4), abi.JITTER_SINGLE, True)
        out, leaves = _port(vol, rays, nears, fars, edges.cpu(), INV_S)
        keep = _keep(vol, rays, out)
        g = torch.Generator().manual_seed(3)
        N, S = rays.n_rays, edges.shape[1] - 1
        G = dict(depth=torch.randn(N, generator=g), acc=torch.randn(N, generator=g), weights=torch.randn(N, S, generator=g),
                 sdf=0.1 * torch.randn(N, S, generator=g), grad=0.1 * torch.randn(N, S, 3, generator=g), rgb=torch.randn(N, 3, generator=g))
        if vol.n_sem:
            G['sem'] = torch.randn(N, vol.n_sem, generator=g)
        G = {k: v * keep.reshape(-1, *([1] * (v.dim() - 1))).to(v.dtype) for k, v in G.items()}
        G['depth'] = G['depth'] * (out['acc'].detach() > 0.05).float()
        gr = torch.autograd.grad(sum((out[k] * G[k].double()).sum() for k in G), leaves)
        grads = dict(g_sdf=gr[0][0].double(), g_feat=gr[0][1:].permute(1, 2, 3, 0).double(), g_inv_s=gr[1].double())
        _BWD_REF[key] = (vol, edges, G, grads, float(keep.float().mean()))
    return _BWD_REF[key]


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
@pytest.mark.parametrize("n_feat", [4, 8], ids=["C4", "C8"])
def test_backward_through_the_samplers_edges_vs_float64_autograd(hip, n_feat, scatter):
    s = scene('linear')
    vol, edges, G, ref, kept = _bwd_reference('linear', n_feat)
    assert kept > 0.5 and edges.shape[1] == 33
    cfg = dataclasses.replace(s.cfg, inv_s=INV_S, bwd_scatter=scatter)
    got, out = _device_grads(vol, s.dev[0], cfg, G, edges)
    m = rc.grad_metrics(got, ref)
    _log(dict(test="backward", n_feat=n_feat, scatter=scatter, rays_with_upstream=kept, **m))
    assert not out['ts'].requires_grad and out['weights'].shape == (s.host[0].n_rays, 32)
    for k, val in m.items():
        assert val <= TRAIN_SHAPE_TOL[k], (k, val, TRAIN_SHAPE_TOL[k])


@pytest.mark.parametrize("scatter", ["atomic", "binned"])
def test_backward_with_uniform_edges_is_the_plain_exact_backward(hip, scatter):
    s = scene('linear')
    vol, _edges, G32, _ref, _ = _bwd_reference('linear', 8)
    N = s.host[0].n_rays
    cfg = dataclasses.replace(s.cfg, n_samples=32, inv_s=INV_S, bwd_scatter=scatter, exact=True)
    plain, _ = _device_grads(vol, s.dev[0], cfg, G32, None)
    with_edges, _ = _device_grads(vol, s.dev[0], cfg, G32, uc.uniform_edges(32, N).to(D0))
    m = rc.grad_metrics(with_edges, plain)
    for k, val in m.items():
        assert val <= TRAIN_SHAPE_TOL[k], (k, val)
    assert plain['g_sdf'].abs().max() > 0 and plain['g_feat'].abs().max() > 0


# ---- 6. the head -----------------------------------------------------------------------------------------------------
def _head(**kw):
    from test_head_gpu import make_head
    # 8 x 10 rays on 64 x 64 pixels: row stride 8, exact in float32, so that a row-block chunk makes the rows of the frame
    return make_head(render_bkgd='white', num_samples=16, num_samples_importance=16, num_up_sample_steps=4, base_variance=16,
                     ray_number=[8, 10], return_sample_sdf=True, **kw)


def test_head_trains_one_step_on_the_importance_samples(hip):
    from test_head_gpu import make_inputs
    os.environ['eval'] = 'false'
    head = _head(return_median_depth=True).train()
    assert head.total_samples == 32
    rep, metas, _ = make_inputs()
    import numpy as np
    np.random.seed(0)
    torch.manual_seed(1)
    out = head(rep, metas, global_iter=0)
    R, S, N = 80, 32, 2
    for k in ('weights', 'ts', 'deltas', 'ray_indices', 'sample_sdf'):
        assert len(out[k]) == N and all(t.shape == (R * S,) for t in out[k]), k
    assert out['eik_grad'].shape == (N * R * S, 3)
    assert torch.equal(out['ray_indices'][0], torch.arange(R, device=D0).repeat_interleave(S))
    for cam in range(N):
        w, ts = out['weights'][cam].detach().cpu().reshape(R, S), out['ts'][cam].detach().cpu().reshape(R, S)
        assert (ts[:, 1:] >= ts[:, :-1]).all()
        assert torch.equal(out['ms_depths_median'][0][0, cam].cpu(), median_depth_reference(w, ts)[0]), cam
    loss = out['ms_depths'][0].sum() + out['ms_colors'][0].sum() + sum(w.sum() for w in out['weights']) + (out['eik_grad'] ** 2).sum()
    loss.backward()
    for t in rep:
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0


def test_head_render_is_the_operator_level_call_chunked(hip):
    from test_head_gpu import make_inputs
    os.environ['eval'] = 'true'
    try:
        rep, metas, _ = make_inputs()
        head = _head(return_median_depth=True).eval()
        with torch.no_grad():
            head.prepare(rep, metas)
            vol = head.model.field.volume.detached()
            rays, _pix, num_cams, num_rays = head._rays(metas, D0)
            cfg = head._render_cfg(False)
            cfg.inv_s_dev = head.model.field.inv_s_device()
            edges = upsample_edges(vol, rays, cfg, 16, 4, 16.0)
            assert edges.shape == (num_cams * num_rays, 33)
            assert not torch.equal(edges, uc.uniform_edges(32, edges.shape[0]).to(D0)), "the field must move some samples"
            want = render_rays(vol, rays, cfg, edges=edges)
            want_med = render_median_depth(vol, rays, cfg, edges=edges)['median_depth']
            head.up_edge_bytes = edges.numel() * 4 // 3               # three chunks of rows
            n_chunks = -(-(rays.n_rays * 33 * 4) // head.up_edge_bytes)
            assert n_chunks >= 2
            got = head.render(metas)
            shp = (1, num_cams, num_rays)
            assert torch.equal(got['ms_depths'][0], want['depth'].reshape(shp))
            assert torch.equal(got['ms_accs'][0], want['acc'].reshape(shp))
            assert torch.equal(got['ms_colors'][0], want['rgb'].reshape(*shp, 3))
            assert torch.equal(got['ms_max_depths'][0], want['max_depth'].reshape(shp))
            assert torch.equal(got['sem'][0], want['sem'].reshape(*shp, -1))
            assert torch.equal(got['ms_depths_median'][0], want_med.reshape(shp))
            per = render_rays(vol, rays, cfg, edges=edges, per_sample=True)
            assert torch.equal(want_med.cpu(), median_depth_reference(per['weights'].cpu(), per['ts'].cpu())[0])
            normal = head.render(metas, vis_normal=True)['vis_normal'][0]
            assert normal.shape == (*shp, 3) and torch.isfinite(normal).all()
    finally:
        os.environ['eval'] = 'false'
