"""GPU: TPVPositionLifter against the REAL reference class (tests/golden/pos_lifter.npz) — outputs and parameter gradients
with the bounds tests/test_golden_gpu.py uses for encoder modules — and its inference form: the planes as views of ONE
cached concatenated tensor that the encoder's first step takes without a copy."""
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
D0 = torch.device("cuda:0")
GOLD = np.load(os.path.join(G, "pos_lifter.npz"))
CFG = json.load(open(os.path.join(G, "pos_lifter_cfg.json")))
PLANES = ('hw', 'zh', 'wz')


def build(name):
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    m = MODELS.build(copy.deepcopy(CFG['lifters'][name]))
    pre = f'{name}.sd.'
    m.load_state_dict({k[len(pre):]: torch.tensor(GOLD[k]) for k in GOLD.files if k.startswith(pre)}, strict=True)
    return m.to(D0)


@pytest.mark.parametrize("name", ['linear', 'linear_upscale'])
@pytest.mark.parametrize("min_rows", [None, 1], ids=['linear', 'tall'])
def test_outputs_and_gradients_vs_reference_class(hip, name, min_rows, monkeypatch):
    """min_rows=1: the row-split tall-Linear path the shipped plane sizes take, on the fixture's small planes"""
    from selfocc_amd.model.bricks import TallLinear
    if min_rows is not None:
        monkeypatch.setattr(TallLinear, 'min_rows', min_rows)
    m = build(name).train()
    bs = CFG['bs']
    outs = m([torch.zeros(bs, 1, device=D0)])['representation']
    loss = 0.
    for p, o in zip(PLANES, outs):
        ref = torch.tensor(GOLD[f'{name}.out.{p}'])
        assert o.shape == ref.shape
        assert torch.allclose(o.detach().cpu(), ref, rtol=1e-4, atol=1e-4), (p, (o.detach().cpu() - ref).abs().max())
        loss = loss + (o * torch.tensor(GOLD[f'{name}.G.{p}']).to(D0)).sum()
    loss.backward()
    for k, prm in m.named_parameters():
        ref = torch.tensor(GOLD[f'{name}.grad.{k}'])
        err = (prm.grad.cpu() - ref).abs().max()
        assert err <= 1e-4 * ref.abs().max(), (k, err.item(), ref.abs().max().item())
    # inference, bs = 1: the same planes
    with torch.no_grad():
        rep = m.eval()([torch.zeros(1, 1, device=D0)])['representation']
    for p, o in zip(PLANES, rep):
        ref = torch.tensor(GOLD[f'{name}.out.{p}'])[:1]
        assert torch.allclose(o.cpu(), ref, rtol=1e-4, atol=1e-4), p


def test_inference_planes_feed_the_encoder_as_one_cached_tensor(hip):
    from selfocc_amd.registry import MODELS
    from selfocc_amd.model.encoder.tpvformer import _Planes
    enc_np = np.load(os.path.join(G, "encoder.npz"))
    cfg = json.load(open(os.path.join(G, "encoder_cfg.json")))
    assert cfg['encoder']['mapping_args'] == CFG['lifters']['linear']['mapping_args']
    enc = MODELS.build(dict(type='TPVFormerEncoder', **copy.deepcopy(cfg['encoder'])))
    enc.load_state_dict({k[4:]: torch.tensor(v) for k, v in enc_np.items() if k.startswith('enc.')}, strict=True)
    enc = enc.to(D0).eval()
    lifter = build('linear').eval()
    query = MODELS.build(dict(type='TPVQueryLifter', **cfg['lifter'])).to(D0).eval()
    feats = [torch.tensor(enc_np['feat0']).to(D0), torch.tensor(enc_np['feat1']).to(D0)]
    metas = [dict(lidar2img=enc_np['lidar2img'], img_shape=tuple(cfg['img_shape']))]
    sizes = [cfg['lifter']['tpv_h'] * cfg['lifter']['tpv_w'], cfg['lifter']['tpv_z'] * cfg['lifter']['tpv_h'],
             cfg['lifter']['tpv_w'] * cfg['lifter']['tpv_z']]
    with torch.no_grad():
        rep = lifter(feats)['representation']
        assert isinstance(rep, _Planes) and rep.cat.shape == (1, sum(sizes), 32) and rep.cat.is_contiguous()
        assert [p.shape[1] for p in rep] == sizes
        assert all(p.untyped_storage().data_ptr() == rep.cat.untyped_storage().data_ptr() for p in rep)
        again = lifter(feats)['representation']
        assert again.cat is rep.cat                                        # the Linears did not run again
        # the same values as learned queries: the encoder cannot tell the two lifters apart
        for prm, p in zip((query.tpv_hw, query.tpv_zh, query.tpv_wz), rep):
            prm.copy_(p)
        out_pos = enc(rep, ms_img_feats=feats, metas=metas)['representation']
        out_qry = enc(query(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
        assert len(out_pos) == 3 and all(torch.equal(a, b) for a, b in zip(out_pos, out_qry))
        assert torch.equal(lifter(feats)['representation'].cat, rep.cat)   # the encoder did not write into the cached tensor
        # an in-place parameter update rebuilds the cached tensor
        old = rep.cat.clone()
        lifter.position_layer_zh.bias.add_(0.5)
        new = lifter(feats)['representation']
        assert new.cat is not rep.cat
        assert torch.equal(new[0], old[:, :sizes[0]]) and torch.equal(new[2], old[:, sizes[0] + sizes[1]:])
        assert torch.allclose(new[1], old[:, sizes[0]:sizes[0] + sizes[1]] + 0.5, rtol=1e-6, atol=1e-6)
    # under autograd (training) the planes are plain expanded tensors that carry the graph
    rep = lifter.train()(feats)['representation']
    assert not isinstance(rep, _Planes) and all(p.requires_grad for p in rep)
