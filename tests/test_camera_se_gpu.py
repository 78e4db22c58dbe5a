"""GPU: the fused CameraAwareSE flatten (csrc/camera_se.hip behind CameraAwareSE.flatten) against
  * the fixture the real reference class produced (tests/golden/make_golden_camera_se.py), both widths, both modes;
  * the module's torch route on the same device and a float64 torch evaluation (CPU), at the shipped nuScenes shape, a KITTI
    shape, batch 2, one 1x1 level, eight levels, C = M = 128, non-contiguous maps, spare level-embedding rows;
  * inside TPVFormerEncoder: forward planes anchored to the fixture's reference-generated module outputs, gradients between
    the fused and the torch route;
plus the fallback for unsupported shapes, autocast, sync-freedom on a new frame and run-to-run determinism.

Bounds: per tensor, relative to its scale (max |ref|): max(2e-5, 10 x spread), the spread being the float32-vs-float64
difference of the REFERENCE computation on that tensor (stored in the fixture, or measured here between the float32 torch route
and the float64 evaluation) — never the fused route's own error.  Measured values are appended to
parity_out/camera_se_parity.jsonl."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import camera_se_cases as cases
import test_camera_se_cpu as tc
from selfocc_amd.model.encoder import CameraAwareSE, camera_se

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
TOL = 2e-5
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "camera_se_parity.jsonl")


def log(**rec):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(rec) + "\n")


def fused_only(monkeypatch):
    """make the torch composition raise: what runs after this is the fused route or nothing"""
    def boom(*a, **k):
        raise AssertionError("the torch composition ran where the fused route was meant to")
    monkeypatch.setattr(CameraAwareSE, '_compose', boom)


def flatten_route(cams, lvls, levels):
    """route for tc.run_module: the encoder's value, cut back into per-level (B, N, C, h, w) maps so that the fixture's upstream
    gradients and output names apply; the embeddings are subtracted again in float64-exact fashion by feeding zeros"""
    def route(mod, maps, metas):
        val = mod.flatten(maps, metas, cams, lvls)                  # (N, S, B, C)
        outs, s0 = [], 0
        for h, w in levels:
            outs.append(val[:, s0:s0 + h * w].permute(2, 0, 3, 1).reshape(val.shape[2], val.shape[0], val.shape[3], h, w))
            s0 += h * w
        return outs
    return route


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('name', ['c96m96', 'c96m192', 'enc32'])
def test_fused_route_reproduces_the_fixture(hip, monkeypatch, name, mode):
    """zero embeddings: value IS the module's output, flattened; every output, gradient and buffer against the reference's"""
    z = cases.load_fixture()
    inp, mod = tc.build_case(name, mode == 'train', D0)
    tc.check_seeds(z, name, mod, inp)
    C, L = inp['C'], len(inp['levels'])
    cams, lvls = torch.zeros(inp['N'], C, device=D0), torch.zeros(L, C, device=D0)
    fused_only(monkeypatch)
    got = tc.run_module(mod, [m.to(D0) for m in inp['maps']], [u.to(D0) for u in inp['ups']], inp['metas'],
                        flatten_route(cams, lvls, inp['levels']))
    assert {f'{name}.{mode}.{k}' for k in got} == {k for k in z if k.startswith(f'{name}.{mode}.') and '.spread.' not in k}
    tc.compare_to_fixture(z, f'{name}.{mode}', got,
                          report=lambda key, err, bnd: log(test='fixture', tensor=key, err=err, bound=bnd))


# ---- fused vs torch route vs float64 ------------------------------------------------------------------------------------------
NUSC = ((96, 200), (48, 100), (24, 50), (12, 25))
KITTI = ((44, 152), (22, 76), (11, 38), (6, 19))
PARITY = {
    # name: (B, N, C, M, levels, modes, non-contiguous maps)
    'nuscenes': (1, 6, 96, 96, NUSC, ('train', 'eval'), False),
    'kitti': (1, 1, 96, 96, KITTI, ('eval',), False),           # training-mode BatchNorm1d refuses a single row, in the reference as here
    'wide': (1, 6, 96, 192, ((24, 50), (12, 25)), ('train', 'eval'), False),
    'batch2': (2, 3, 32, 32, ((13, 17), (5, 5)), ('train', 'eval'), False),
    'one_pixel': (1, 2, 32, 32, ((1, 1),), ('train',), False),
    'eight_levels': (1, 2, 32, 64, ((9, 31), (16, 16), (7, 5), (3, 3), (2, 2), (1, 3), (1, 2), (1, 1)), ('train',), False),
    'c128': (1, 2, 128, 128, ((20, 33), (7, 9)), ('train',), False),
    'noncontiguous': (1, 3, 64, 64, ((12, 25), (6, 19)), ('train',), True),
}


def _problem(B, N, C, M, levels, noncontig, seed=77):
    g = torch.Generator().manual_seed(seed)
    if noncontig:
        maps = [torch.randn(B, N, C, w, h, generator=g).transpose(3, 4) for h, w in levels]
    else:
        maps = [torch.randn(B, N, C, h, w, generator=g) for h, w in levels]
    S = sum(h * w for h, w in levels)
    return dict(maps=maps, gv=torch.randn(N, S, B, C, generator=g), cams=torch.randn(N, C, generator=g),
                lvls=torch.randn(len(levels) + 1, C, generator=g), metas=cases.make_metas(seed, B, N))


def _run_flatten(mod, p, device, dtype, method):
    mod = copy.deepcopy(mod).to(device=device, dtype=dtype)
    maps = [m.to(device=device, dtype=dtype).requires_grad_(True) for m in p['maps']]
    cams = p['cams'].to(device=device, dtype=dtype).requires_grad_(True)
    lvls = p['lvls'].to(device=device, dtype=dtype).requires_grad_(True)
    val = getattr(mod, method)(maps, p['metas'], cams, lvls)
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad((val * p['gv'].to(device=device, dtype=dtype)).sum(), maps + [cams, lvls] + list(params.values()))
    res = {'value': val.detach()}
    res.update({f'grad.map.{l}': grads[l] for l in range(len(maps))})
    res['grad.cams_embeds'], res['grad.level_embeds'] = grads[len(maps)], grads[len(maps) + 1]
    res.update({f'grad.{n}': g for n, g in zip(params, grads[len(maps) + 2:])})
    return {k: v.detach().double().cpu() for k, v in res.items()}


@pytest.mark.parametrize('case', list(PARITY))
def test_fused_vs_torch_route_vs_float64(hip, monkeypatch, case):
    B, N, C, M, levels, modes, noncontig = PARITY[case]
    for mode in modes:
        p = _problem(B, N, C, M, levels, noncontig)
        mod = cases.seed_module(CameraAwareSE(C, M, C), 4242).train(mode == 'train')
        f64 = _run_flatten(mod, p, 'cpu', torch.float64, 'flatten_torch')
        t32 = _run_flatten(mod, p, D0, torch.float32, 'flatten_torch')
        with monkeypatch.context() as mp:
            fused_only(mp)
            fus = _run_flatten(mod, p, D0, torch.float32, 'flatten')
        L = len(levels)
        assert float(fus['grad.level_embeds'][L].abs().max()) == 0.0            # the spare row's gradient stays exactly zero
        for k, ref in f64.items():
            scale = float(ref.abs().max())
            if k == 'grad.reduce_conv.0.bias' and mode == 'train':               # mathematically zero (see the fixture's generator)
                scale = float(f64['grad.reduce_conv.0.weight'].abs().max())
            if scale == 0.0:
                assert float(fus[k].abs().max()) == 0.0, k
                continue
            spread = float((t32[k] - ref).abs().max()) / scale
            e64 = float((fus[k] - ref).abs().max()) / scale
            e32 = float((fus[k] - t32[k]).abs().max()) / scale
            bnd = max(TOL, 10.0 * spread)
            log(test='parity', case=case, mode=mode, tensor=k, fused_vs_f64=e64, fused_vs_torch=e32, torch_vs_f64=spread, bound=bnd)
            print(f'{case}.{mode}.{k}: fused-f64 {e64:.3g}  fused-torch {e32:.3g}  torch-f64 {spread:.3g}  bound {bnd:.3g}')
            assert e64 <= bnd and e32 <= bnd, (case, mode, k, e64, e32, spread)


def _fold(gate, w, bias, cams, lvls, maps):
    """the contract in plain torch ops, any dtype / device"""
    B, N = maps[0].shape[:2]
    flat = []
    for l, x in enumerate(maps):
        y = torch.einsum('ck,ikp->ipc', w, x.flatten(0, 1).flatten(2) * gate[:, :, None]).unflatten(0, (B, N)) + bias     # (B, N, p, C)
        flat.append((y + cams[None, :, None, :]) + lvls[l])
    return torch.cat(flat, 2).permute(1, 2, 0, 3)                              # (N, S, B, C)


@pytest.mark.parametrize('N,C,M,levels', [(1, 96, 96, KITTI), (1, 32, 32, ((1, 1),)), (1, 96, 192, ((6, 19), (3, 10)))])
def test_kernels_driven_directly_with_a_given_gate_single_camera(hip, N, C, M, levels):
    """forward and backward at N = 1 (KITTI), where the module's training-mode BatchNorm1d cannot run"""
    g = torch.Generator().manual_seed(3)
    B = 1
    t = dict(gate=torch.sigmoid(torch.randn(B * N, M, generator=g)), w=torch.randn(C, M, generator=g) / M ** 0.5,
             bias=torch.randn(C, generator=g), cams=torch.randn(N, C, generator=g), lvls=torch.randn(len(levels), C, generator=g))
    maps = [torch.randn(B, N, M, h, w, generator=g) for h, w in levels]
    gv = torch.randn(N, sum(h * w for h, w in levels), B, C, generator=g)

    def run(device, dtype, fused):
        a = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in t.items()}
        xs = [m.to(device=device, dtype=dtype).requires_grad_(True) for m in maps]
        if fused:
            val = camera_se._CameraSeFlatten.apply(a['gate'], a['w'].reshape(C, M, 1, 1), a['bias'], a['cams'], a['lvls'], *xs)
        else:
            val = _fold(a['gate'], a['w'], a['bias'], a['cams'], a['lvls'], xs)
        grads = torch.autograd.grad((val * gv.to(device=device, dtype=dtype)).sum(), list(a.values()) + xs)
        names = ['grad.' + k for k in a] + [f'grad.map.{l}' for l in range(len(xs))]
        return {'value': val.detach().double().cpu(), **{n: gr.double().cpu() for n, gr in zip(names, grads)}}
    f64, t32, fus = run('cpu', torch.float64, False), run(D0, torch.float32, False), run(D0, torch.float32, True)
    for k, ref in f64.items():
        scale = float(ref.abs().max())
        spread, err = float((t32[k] - ref).abs().max()) / scale, float((fus[k] - ref).abs().max()) / scale
        log(test='direct', N=N, C=C, M=M, tensor=k, fused_vs_f64=err, torch_vs_f64=spread)
        assert err <= max(TOL, 10.0 * spread), (k, err, spread)


def test_a_map_without_requires_grad_gets_no_gradient_and_the_others_do_not_change(hip, monkeypatch):
    fused_only(monkeypatch)
    B, N, C, M, levels = 1, 3, 32, 32, ((8, 8), (4, 4), (2, 3))
    p = _problem(B, N, C, M, levels, False)
    mod = cases.seed_module(CameraAwareSE(C, M, C), 4242).to(D0).eval()
    cams, lvls, gv = p['cams'].to(D0), p['lvls'].to(D0), p['gv'].to(D0)

    def grads(frozen):
        maps = [m.to(D0).requires_grad_(l != frozen) for l, m in enumerate(p['maps'])]
        (mod.flatten(maps, p['metas'], cams, lvls) * gv).sum().backward()
        out = [m.grad for m in maps] + [q.grad.clone() for q in mod.parameters()]
        mod.zero_grad()
        return out
    full, part = grads(None), grads(1)
    assert part[1] is None
    assert all(torch.equal(a, b) for i, (a, b) in enumerate(zip(full, part)) if i != 1)


def test_backward_is_deterministic(hip, monkeypatch):
    fused_only(monkeypatch)
    B, N, C, M, levels = 1, 6, 96, 96, ((48, 100), (24, 50), (12, 25))
    p = _problem(B, N, C, M, levels, False)
    mod = cases.seed_module(CameraAwareSE(C, M, C), 4242).train()
    a, b = _run_flatten(mod, p, D0, torch.float32, 'flatten'), _run_flatten(mod, p, D0, torch.float32, 'flatten')
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_unsupported_shape_takes_the_torch_composition(hip):
    B, N, C, M, levels = 1, 2, 40, 40, ((5, 7), (2, 2))
    p = _problem(B, N, C, M, levels, False)
    mod = cases.seed_module(CameraAwareSE(C, M, C), 4242).train()
    assert hip.selfocc_camera_se_supported(B, N, C, M, len(levels)) == 0
    a, b = _run_flatten(mod, p, D0, torch.float32, 'flatten'), _run_flatten(mod, p, D0, torch.float32, 'flatten_torch')
    f64 = _run_flatten(mod, p, 'cpu', torch.float64, 'flatten_torch')
    for k, ref in f64.items():       # the same torch ops in both; two executions of vendor kernels need not agree to the bit
        scale = float(ref.abs().max())
        if scale == 0.0:
            assert float(a[k].abs().max()) == 0.0, k
            continue
        bnd = max(TOL, 10.0 * float((b[k] - ref).abs().max()) / scale)
        assert float((a[k] - b[k]).abs().max()) / scale <= bnd and float((a[k] - ref).abs().max()) / scale <= bnd, k


# ---- inside the encoder --------------------------------------------------------------------------------------------------------
def _encoders(num_cams, **kw):
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    cfg = tc._enc_cfg(**kw)
    cfg['num_cams'] = num_cams
    for layer in cfg['transformerlayers']:
        layer['attn_cfgs'][1]['num_cams'] = num_cams
    torch.manual_seed(1)
    aware = MODELS.build(copy.deepcopy(dict(cfg, camera_aware=True))).to(D0)
    aware.init_weights()
    plain = MODELS.build(copy.deepcopy(cfg)).to(D0)
    plain.load_state_dict({k: v for k, v in aware.state_dict().items() if not k.startswith('camera_se_net.')}, strict=True)
    lifter = MODELS.build(dict(type='TPVQueryLifter', tpv_h=32, tpv_w=32, tpv_z=4, dim=32)).to(D0)
    return aware, plain, lifter


def _geometry_metas(n_cams, seed=0):
    import test_head_gpu as th
    _, metas, _ = th.make_inputs(n_cams=n_cams, seed=seed)
    m = np.array(metas[0]['img2lidar'], dtype=np.float64)
    m[:, :3, 3] += 0.01 * (seed + 1)
    return {'lidar2img': np.stack([np.linalg.inv(x) for x in m]), 'img_shape': (64, 64)}


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_encoder_planes_match_the_plain_encoder_fed_the_reference_outputs(hip, monkeypatch, mode):
    z = cases.load_fixture()
    inp = cases.case_inputs('enc32')
    aware, plain, lifter = _encoders(3)
    cases.seed_module(aware.camera_se_net, inp['seed'])
    tc.check_seeds(z, 'enc32', aware.camera_se_net, inp)
    for m in (aware, plain, lifter):
        m.train(mode == 'train')
    meta = dict(_geometry_metas(3), intrinsic=list(z['enc32.metas.intrinsic'][0]), cam2ego=list(z['enc32.metas.cam2ego'][0]))
    maps = [torch.from_numpy(z[f'enc32.maps.{l}']).to(D0) for l in range(2)]
    ref_outs = [torch.from_numpy(z[f'enc32.{mode}.out.{l}']).to(D0) for l in range(2)]
    rep = lifter(maps)['representation']
    gw = [torch.randn(r.shape, generator=torch.Generator().manual_seed(i)).to(D0) for i, r in enumerate(rep)]

    def run(enc, feats, hip_route=True):
        enc = copy.deepcopy(enc)                        # training-mode BatchNorm1d updates its buffers: every run starts equal
        feats = [f.clone().requires_grad_(True) for f in feats]
        with monkeypatch.context() as mp:
            if enc.camera_aware and hip_route:
                fused_only(mp)
            if not hip_route:
                mp.setattr(camera_se, 'CAMERA_SE_HIP', False)
            if enc.camera_aware:                           # keep d loss / d value: the upstream gradient the module sees here
                inner = enc.camera_se_net.flatten

                def flatten(*a, **k):
                    val = inner(*a, **k)
                    val.register_hook(lambda g: upstream.__setitem__(hip_route, g.detach().clone()))
                    return val
                mp.setattr(enc.camera_se_net, 'flatten', flatten)
            planes = enc([r.detach() for r in rep], ms_img_feats=feats, metas=[meta])['representation']
        sum((pl * g).sum() for pl, g in zip(planes, gw)).backward()
        grads = {f'map.{l}': f.grad for l, f in enumerate(feats)}
        grads.update({n: q.grad for n, q in enc.named_parameters()
                      if q.grad is not None and (n.startswith('camera_se_net.') or n in ('cams_embeds', 'level_embeds'))})
        return [pl.detach() for pl in planes], grads
    upstream = {}
    planes_ref, _ = run(plain, ref_outs)
    planes_fused, g_fused = run(aware, maps)
    planes_torch, g_torch = run(aware, maps, hip_route=False)
    for i, (a, b) in enumerate(zip(planes_fused, planes_ref)):
        err = float((a - b).abs().max()) / float(b.abs().max())
        log(test='encoder', mode=mode, tensor=f'plane.{i}', err=err, bound=TOL)
        assert err <= TOL, (i, err)
    assert set(g_fused) == set(g_torch) and 'camera_se_net.context_conv.weight' in g_fused and 'cams_embeds' in g_fused
    # the reference computation's own float32 noise UNDER THIS upstream gradient: the module's torch route in float32 against a
    # float64 run, both fed the d loss / d value the torch-route encoder produced (N = 3 rows of training-mode BatchNorm1d:
    # the conditioning depends on the upstream, so the fixture's spreads, taken under another loss, do not transfer)
    prob = dict(maps=[m.cpu() for m in maps], gv=upstream[False].cpu(), cams=aware.cams_embeds.detach().cpu(),
                lvls=aware.level_embeds.detach().cpu(), metas=[meta])
    m32 = _run_flatten(aware.camera_se_net, prob, D0, torch.float32, 'flatten_torch')
    m64 = _run_flatten(aware.camera_se_net, prob, 'cpu', torch.float64, 'flatten_torch')
    names = {'cams_embeds': 'grad.cams_embeds', 'level_embeds': 'grad.level_embeds', 'map.0': 'grad.map.0', 'map.1': 'grad.map.1'}
    for k, ref in g_torch.items():
        mk = names.get(k, 'grad.' + k[len('camera_se_net.'):])
        spread = float((m32[mk] - m64[mk]).abs().max()) / float(m64[mk].abs().max())
        bnd = max(TOL, 10.0 * spread)
        err = float((g_fused[k] - ref).abs().max()) / float(ref.abs().max())
        log(test='encoder', mode=mode, tensor='grad.' + k, err=err, bound=bnd)
        assert err <= bnd, (k, err, bnd)


def _aware_frame(seed, n_cams=2):
    g = torch.Generator().manual_seed(seed)
    meta = dict(_geometry_metas(n_cams, seed), **cases.make_metas(100 + seed, 1, n_cams)[0])     # every frame: its own calibration
    feats = [torch.randn(1, n_cams, 32, 8, 8, generator=g).to(D0), torch.randn(1, n_cams, 32, 4, 4, generator=g).to(D0)]
    return [meta], feats


def test_eval_frame_and_training_step_are_sync_free_on_a_new_frame(hip, monkeypatch):
    """Only the lifter and the camera-aware ENCODER are under the sync check here (forward, and a backward from a plain
    mean-square of the planes): the new frame's calibration misses the content cache and is uploaded.  Head and MultiLoss are
    held sync-free by test_sync_free_gpu.py and do not depend on the encoder option."""
    from test_sync_free_gpu import no_sync
    fused_only(monkeypatch)
    aware, _, lifter = _encoders(2)

    def frame(metas, feats, train):
        feats = [f.requires_grad_(train) for f in feats]
        planes = aware(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
        if train:
            sum(pl.square().mean() for pl in planes).backward()
        return planes
    for train in (False, True):
        for m in (aware, lifter):
            m.train(train)
        with torch.set_grad_enabled(train):
            frame(*_aware_frame(0), train)               # warm-up: workspaces, constant tensors
            new = _aware_frame(1)                        # a NEW frame's intrinsics: no cache hit on the contents
            with no_sync():
                planes = frame(*new, train)
        assert all(torch.isfinite(pl).all() for pl in planes)
        if train:
            assert torch.isfinite(aware.camera_se_net.context_mlp.fc1.weight.grad).all()
            assert float(aware.camera_se_net.context_conv.weight.grad.abs().max()) > 0.0


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_training_step_under_autocast_with_camera_aware(hip, dtype):
    """the pattern of test_encoder_glue_gpu.test_training_step_under_autocast: a whole training step (lifter, camera-aware encoder,
    head, losses) under torch.autocast runs, every gradient is finite, the loss stays close to the float32 step's"""
    import test_sync_free_gpu as S

    def step(amp):
        torch.manual_seed(0); np.random.seed(0)
        th, lifter, _, head, loss_fn = S._stages(train=True)
        enc, _, _ = _encoders(2)
        enc.train()
        for m in (lifter, enc, head):
            for mod in m.modules():
                if isinstance(mod, nn.Dropout):
                    mod.p = 0.0
        metas, feats, imgs = S._frame(th, 0)
        metas[0].update(cases.make_metas(5, 1, 2)[0])
        with torch.autocast("cuda", dtype=dtype, enabled=amp):
            rep = enc(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
            out = head(rep, metas, global_iter=7)
            total, _ = loss_fn(dict(out, metas=metas, **imgs))
        total.backward()
        params = [p for m in (lifter, enc, head) for p in m.parameters()]
        assert torch.isfinite(total).all() and all(p.grad is None or torch.isfinite(p.grad).all() for p in params)
        assert enc.camera_se_net.context_conv.weight.grad is not None and enc.camera_se_net.bn.weight.grad is not None
        return float(total.detach())
    ref, amp = step(False), step(True)
    assert abs(amp - ref) <= 0.05 * abs(ref) + 1e-3, (amp, ref)
