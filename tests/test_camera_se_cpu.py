"""CPU: CameraAwareSE (selfocc_amd/model/encoder/camera_se.py) against the fixture the real reference class produced
(tests/golden/make_golden_camera_se.py): state-dict compatibility, the torch route's outputs / gradients / buffers, the
folded formulas the HIP kernels implement (in float64 against autograd through the composition), and the host-side
argument checks of the new C entry points.

Bounds: per tensor, relative to its scale (max |ref|): max(2e-5, 10 x spread.<name>), the spread being the reference's own
float32-vs-float64 difference on that tensor, stored in the fixture."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import camera_se_cases as cases
from selfocc_amd import abi
from selfocc_amd.model.encoder import CameraAwareSE

CFG = json.load(open(os.path.join(cases.GOLDEN, 'camera_se_cfg.json')))
TOL = 2e-5


def bound(z, key):
    key = key.replace('.out.', '.spread.out.').replace('.grad.', '.spread.grad.').replace('.buf.', '.spread.buf.')
    return max(TOL, 10.0 * float(np.asarray(z[key]).reshape(-1)[0]))


def compare_to_fixture(z, prefix, got, report=None):
    """every element of every tensor of `got` (name -> tensor) against the fixture's `<prefix>.<name>`"""
    for name, t in got.items():
        key = f'{prefix}.{name}'
        ref = torch.from_numpy(z[key])
        if name.endswith('num_batches_tracked'):
            assert int(t) == int(ref), key
            continue
        scale = float(ref.abs().max())
        if name == 'grad.reduce_conv.0.bias' and '.train' in prefix:     # mathematically zero: a bias in front of a BatchNorm
            scale = float(np.abs(z[f'{prefix}.grad.reduce_conv.0.weight']).max())
        err = float((t.detach().cpu().float() - ref).abs().max()) / scale
        if report is not None:
            report(key, err, bound(z, key))
        print(f'{key}: {err:.3g} (bound {bound(z, key):.3g})')
        assert err <= bound(z, key), (key, err, bound(z, key))


def run_module(mod, maps, ups, metas, route):
    """outputs, all gradients and (training mode) buffers of one call; `route` maps (module, maps, metas) -> output list"""
    maps = [m.clone().requires_grad_(True) for m in maps]
    outs = route(mod, maps, metas)
    loss = sum((o * u).sum() for o, u in zip(outs, ups))
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(loss, maps + list(params.values()))
    res = {f'out.{l}': o for l, o in enumerate(outs)}
    res.update({f'grad.map.{l}': grads[l] for l in range(len(maps))})
    res.update({f'grad.{n}': g for n, g in zip(params, grads[len(maps):])})
    if mod.training:
        res.update({f'buf.{n}': b.detach().clone() for n, b in mod.named_buffers()})
    return res


def build_case(name, train, device='cpu'):
    inp = cases.case_inputs(name)
    mod = cases.seed_module(CameraAwareSE(inp['C'], inp['M'], inp['C']), inp['seed']).train(train)
    return inp, mod.to(device)


def check_seeds(z, name, mod, inp):
    for k, v in cases.checks(mod, inp).items():
        assert np.allclose(v, z[f'{name}.{k}'], rtol=1e-9), f"seeded {k} of {name} differ from the generator's (torch RNG changed?)"


@pytest.mark.parametrize('name', ['c96m96', 'c96m192'])
def test_reference_state_dict_loads_strictly(name):
    c = CFG[name]
    mod = CameraAwareSE(c['in_channels'], c['mid_channels'], c['out_channels'])
    sd = {k: torch.zeros(s, dtype=torch.int64 if k.endswith('num_batches_tracked') else torch.float32) for k, s in c['state_dict'].items()}
    assert set(sd) == set(mod.state_dict())
    assert {k: list(v.shape) for k, v in mod.state_dict().items()} == c['state_dict']
    mod.load_state_dict(sd, strict=True)
    assert ('reduce_conv.0.weight' in sd) == (c['in_channels'] != c['mid_channels'])


def test_init_weight_opens_the_gate():
    mod = CameraAwareSE(32, 32, 32)
    mod.init_weight()
    assert float(mod.context_mlp.fc2.weight.detach().abs().max()) == 0.0 and bool((mod.context_mlp.fc2.bias == 10.0).all())


def _enc_cfg(**kw):
    from selfocc_amd import synthetic as sy
    dim = 32
    layer = dict(type='TPVFormerLayer',
                 attn_cfgs=[dict(type='CrossViewHybridAttention', embed_dims=dim, num_heads=2, num_levels=3,
                                 num_points=4, dropout=0.0, batch_first=True),
                            dict(type='TPVCrossAttention', embed_dims=dim, num_cams=3, dropout=0.0, batch_first=True,
                                 num_heads=2, num_levels=2, num_points=[3, 3, 2])],
                 feedforward_channels=2 * dim, ffn_dropout=0.0,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    return dict(type='TPVFormerEncoder', mapping_args=sy.CONFIGS["cfg1"]["mapping"], embed_dims=dim, num_cams=3, num_feature_levels=2,
                positional_encoding=dict(type='TPVPositionalEncoding', num_freqs=[3] * 3, embed_dims=dim,
                                         tot_range=[0.0, 0.0, -1.0, 12.8, 12.8, 2.0]),
                num_points_cross=[3, 3, 2], num_points_self=[4] * 3, transformerlayers=[layer, layer], num_layers=2, **kw)


def test_encoder_builds_with_camera_aware_and_bev_encoder_still_rejects_it():
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    enc = MODELS.build(_enc_cfg(camera_aware=True))
    keys = [k for k in enc.state_dict() if k.startswith('camera_se_net.')]
    assert 'camera_se_net.context_conv.weight' in keys and 'camera_se_net.bn.running_mean' in keys
    assert not any(k.startswith('camera_se_net.reduce_conv') for k in keys)
    assert enc.camera_se_net.context_conv.weight.shape == (32, 32, 1, 1)
    wide = MODELS.build(_enc_cfg(camera_aware=True, camera_aware_mid_channels=64))
    assert wide.camera_se_net.context_conv.weight.shape == (32, 64, 1, 1)
    assert wide.camera_se_net.reduce_conv[0].weight.shape == (64, 32, 3, 3)
    plain = MODELS.build(_enc_cfg())
    assert not any('camera_se_net' in k for k in plain.state_dict())
    # init_weights: the matrices get the encoder's xavier_uniform_; CameraAwareSE.init_weight() is NOT called (as in the reference)
    enc.init_weights()
    assert float(enc.camera_se_net.context_mlp.fc2.weight.detach().abs().max()) > 0.0
    assert float(enc.camera_se_net.context_mlp.fc2.bias.detach().abs().max()) < 5.0
    with pytest.raises(NotImplementedError, match='row_shard'):
        MODELS.build(_enc_cfg(camera_aware=True, row_shard=True))
    bev = dict(type='BEVFormerEncoder', mapping_args=_enc_cfg()['mapping_args'], embed_dims=32, num_cams=3, num_feature_levels=2,
               positional_encoding=dict(type='BEVPositionalEncoding', num_freqs=3, embed_dims=32, tot_range=[0.0, 0.0, -1.0, 12.8, 12.8, 2.0]),
               transformerlayers=[], num_layers=0, camera_aware=True)
    with pytest.raises(TypeError, match='camera_aware'):
        MODELS.build(bev)


@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('name', ['c96m96', 'c96m192', 'enc32'])
def test_torch_route_reproduces_the_fixture_on_cpu(name, mode):
    z = cases.load_fixture()
    inp, mod = build_case(name, mode == 'train')
    check_seeds(z, name, mod, inp)
    got = run_module(mod, inp['maps'], inp['ups'], inp['metas'], lambda m, maps, metas: m(maps, metas))
    assert {f'{name}.{mode}.{k}' for k in got} == {k for k in z if k.startswith(f'{name}.{mode}.') and '.spread.' not in k}
    compare_to_fixture(z, f'{name}.{mode}', got)


def test_flatten_on_cpu_is_the_reference_composition():
    """flatten() off the GPU: forward() + the encoder's two broadcast adds and cat, exactly"""
    inp, mod = build_case('enc32', False)
    g = torch.Generator().manual_seed(5)
    cams, lvls = torch.randn(inp['N'], 32, generator=g), torch.randn(3, 32, generator=g)
    val = mod.flatten(inp['maps'], inp['metas'], cams, lvls)
    outs = mod(inp['maps'], inp['metas'])
    ref = torch.cat([(o.flatten(3).permute(1, 0, 3, 2) + cams[:, None, None, :]) + lvls[None, None, l:l + 1, :] for l, o in enumerate(outs)], 2)
    assert val.shape == (inp['N'], 80, 1, 32) and torch.equal(val, ref.permute(0, 2, 1, 3))


def test_intrinsic_3x3_and_missing_keys():
    inp, mod = build_case('enc32', False)
    m3 = [{'intrinsic': [k[:3, :3] for k in inp['metas'][0]['intrinsic']], 'cam2ego': inp['metas'][0]['cam2ego']}]
    a, b = mod(inp['maps'], inp['metas']), mod(inp['maps'], m3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for key in ('intrinsic', 'cam2ego'):
        bad = [{k: v for k, v in inp['metas'][0].items() if k != key}]
        with pytest.raises(KeyError, match=key):
            mod(inp['maps'], bad)


@pytest.mark.parametrize('B,N,C,M,levels', [(1, 6, 96, 96, ((4, 7), (2, 3), (1, 2))), (2, 3, 32, 64, ((3, 5), (1, 1)))])
def test_folded_formulas_equal_autograd_through_the_composition(B, N, C, M, levels):
    """Section "the fold" of DESIGN 3.13 in float64: value = Wg x + bias and the five gradient formulas against autograd
    through gate multiply -> 1x1 convolution -> broadcast adds -> cat.  This is the contract the kernels are held to."""
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xs = [r(B, N, M, h, w).requires_grad_(True) for h, w in levels]
    gate = torch.sigmoid(r(B * N, M)).requires_grad_(True)
    w, bias = r(C, M, 1, 1).requires_grad_(True), r(C).requires_grad_(True)
    cams, lvls = r(N, C).requires_grad_(True), r(len(levels) + 1, C).requires_grad_(True)
    flat = []
    for l, x in enumerate(xs):
        y = torch.nn.functional.conv2d(x.flatten(0, 1) * gate[:, :, None, None], w, bias).unflatten(0, (B, N))
        flat.append((y.flatten(3).permute(1, 0, 3, 2) + cams[:, None, None, :]) + lvls[None, None, l:l + 1, :])
    value = torch.cat(flat, 2).permute(0, 2, 1, 3)                       # (N, S, B, C)
    gv = r(*value.shape)
    auto = torch.autograd.grad((value * gv).sum(), xs + [gate, w, bias, cams, lvls])

    W = w.detach()[:, :, 0, 0]
    Wg = W[None] * gate.detach()[:, None, :]                              # (B*N, C, M)
    dwc = torch.zeros(B * N, C, M, dtype=torch.float64)
    colsum = torch.zeros(len(levels), N, C, dtype=torch.float64)
    s0 = 0
    for l, x in enumerate(xs):
        hw = x.shape[3] * x.shape[4]
        xl = x.detach().reshape(B * N, M, hw)
        fold = torch.einsum('ick,ikp->ipc', Wg, xl).reshape(B, N, hw, C) + (bias.detach() + cams.detach()[:, None, :] + lvls.detach()[l])[None]
        assert torch.allclose(fold.permute(1, 2, 0, 3), value.detach()[:, s0:s0 + hw], rtol=0, atol=1e-12)
        gl = gv[:, s0:s0 + hw].permute(2, 0, 1, 3).reshape(B * N, hw, C)      # (b n, p, c)
        dx = torch.einsum('ick,ipc->ikp', Wg, gl).reshape(x.shape)
        assert torch.allclose(dx, auto[l], rtol=0, atol=1e-12)
        dwc += torch.einsum('ipc,ikp->ick', gl, xl)
        colsum[l] = gv[:, s0:s0 + hw].sum((1, 2))
        s0 += hw
    L = len(levels)
    a_gate, a_w, a_bias, a_cams, a_lvls = auto[L:]
    assert torch.allclose((dwc * W[None]).sum(1), a_gate, rtol=0, atol=1e-11)
    assert torch.allclose((dwc * gate.detach()[:, None, :]).sum(0), a_w[:, :, 0, 0], rtol=0, atol=1e-11)
    assert torch.allclose(colsum.sum((0, 1)), a_bias, rtol=0, atol=1e-11)
    assert torch.allclose(colsum.sum(0), a_cams, rtol=0, atol=1e-11)
    assert torch.allclose(colsum.sum(1), a_lvls[:L], rtol=0, atol=1e-11) and float(a_lvls[L].abs().max()) == 0.0


def test_supported_query_answers_for_the_listed_shapes():
    from selfocc_amd._lib import lib
    sup = lib().selfocc_camera_se_supported
    for B, N, Cc, M, L in [(1, 6, 96, 96, 4), (1, 6, 96, 192, 4), (1, 6, 128, 128, 4), (1, 3, 32, 32, 2), (1, 1, 96, 96, 4),
                           (2, 6, 96, 96, 1), (1, 6, 96, 96, 8), (1, 6, 64, 128, 3)]:
        assert sup(B, N, Cc, M, L) == 1, (B, N, Cc, M, L)
    for B, N, Cc, M, L in [(1, 6, 40, 40, 4), (1, 6, 96, 128, 4), (1, 6, 128, 256, 4), (1, 6, 96, 96, 9), (1, 6, 96, 96, 0),
                           (0, 6, 96, 96, 4), (1, 0, 96, 96, 4), (1, 6, 256, 256, 4)]:
        assert sup(B, N, Cc, M, L) == 0, (B, N, Cc, M, L)


def test_c_entry_points_reject_bad_arguments_as_pure_host_logic():
    """every rejection happens before any HIP call: rc < 0 and a key word in selfocc_last_error(); no GPU here"""
    from selfocc_amd._lib import lib
    l = lib()
    fake = C.create_string_buffer(256 + 16)
    base = (C.addressof(fake) + 15) & ~15                  # never dereferenced: every call below fails its checks first
    L = 2
    hw = (C.c_int32 * L)(12, 5)
    ptrs = (C.c_void_p * L)(base, base + 16)
    dptrs = (C.c_void_p * L)(base + 32, None)
    ws_bytes = l.selfocc_camera_se_flatten_bwd_workspace(hw, L, 1, 6, 96, 96)
    assert ws_bytes == 6 * 2 * (96 * 96 + 96) * 4          # one 512-pixel chunk per level and camera
    assert l.selfocc_camera_se_flatten_bwd_workspace(hw, L, 1, 6, 40, 40) == 0
    assert l.selfocc_camera_se_flatten_bwd_workspace(None, L, 1, 6, 96, 96) == 0

    def fwd(**kw):
        a = dict(feats=ptrs, hw=hw, L=L, B=1, N=6, C=96, M=96, gate=base, w=base, bias=base, cams=base, lvls=base, out=base)
        a.update(kw)
        rc = l.selfocc_camera_se_flatten_fwd(a['feats'], a['hw'], a['L'], a['B'], a['N'], a['C'], a['M'], a['gate'], a['w'], a['bias'],
                                             a['cams'], a['lvls'], a['out'], None)
        return rc, l.selfocc_last_error()

    def bwd(**kw):
        a = dict(g=base, feats=ptrs, hw=hw, L=L, B=1, N=6, C=96, M=96, gate=base, w=base, d=dptrs, dwc=base, colsum=base, ws=base,
                 ws_bytes=ws_bytes)
        a.update(kw)
        rc = l.selfocc_camera_se_flatten_bwd(a['g'], a['feats'], a['hw'], a['L'], a['B'], a['N'], a['C'], a['M'], a['gate'], a['w'],
                                             a['d'], a['dwc'], a['colsum'], a['ws'], a['ws_bytes'], None)
        return rc, l.selfocc_last_error()

    for call, kw, word in [
        (fwd, dict(C=40, M=40), b'unsupported shape'), (fwd, dict(M=128), b'unsupported shape'), (fwd, dict(L=9), b'unsupported shape'),
        (fwd, dict(N=0), b'unsupported shape'), (fwd, dict(gate=None), b'NULL'), (fwd, dict(out=None), b'NULL'), (fwd, dict(feats=None), b'NULL'),
        (fwd, dict(feats=(C.c_void_p * L)(base, None)), b'level 1'), (fwd, dict(hw=(C.c_int32 * L)(12, 0)), b'level 1'),
        (fwd, dict(feats=(C.c_void_p * L)(base + 4, base)), b'aligned'), (fwd, dict(out=base + 8), b'aligned'),
        (bwd, dict(C=128, M=96), b'unsupported shape'), (bwd, dict(g=None), b'NULL'), (bwd, dict(dwc=None), b'NULL'),
        (bwd, dict(colsum=None), b'NULL'), (bwd, dict(g=base + 4), b'aligned'),
        (bwd, dict(d=(C.c_void_p * L)(base + 4, None)), b'aligned'), (bwd, dict(ws=None), b'workspace'),
        (bwd, dict(ws_bytes=ws_bytes - 4), b'workspace'), (bwd, dict(hw=(C.c_int32 * L)(0, 5)), b'level 0'),
    ]:
        rc, err = call(**kw)
        assert rc < 0 and word in err, (call.__name__, kw, rc, err)
    assert abi.ABI_VERSION == 35 and l.selfocc_abi_version() == 35       # only new entry points: no version bump
