"""CPU: TPVPositionLifter (model/lifter/tpv_pos_lifter.py) as a registry module against the REAL reference class
(tests/golden/pos_lifter.npz, make_golden_pos_lifter.py): construction from the stored cfg, a strict load of the reference's
state dict, the constant Fourier-feature buffers, and outputs / parameter gradients where the module runs on the CPU."""
import copy
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
GOLD = np.load(os.path.join(G, "pos_lifter.npz"))
CFG = json.load(open(os.path.join(G, "pos_lifter_cfg.json")))
PLANES = ('hw', 'zh', 'wz')


def build(name):
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    m = MODELS.build(copy.deepcopy(CFG['lifters'][name]))
    pre = f'{name}.sd.'
    m.load_state_dict({k[len(pre):]: torch.tensor(GOLD[k]) for k in GOLD.files if k.startswith(pre)}, strict=True)
    return m


@pytest.mark.parametrize("name", ['linear', 'linear_upscale'])
def test_registry_build_state_dict_and_buffers(name):
    from selfocc_amd.model.bricks import TallLinear
    from selfocc_amd.model.lifter import TPVPositionLifter
    m = build(name)
    assert type(m) is TPVPositionLifter
    cfg = CFG['lifters'][name]
    # nn.Linear's keys, nothing else: the feature buffers are non-persistent, as in the reference
    assert sorted(m.state_dict()) == sorted(f'position_layer_{p}.{w}' for p in PLANES for w in ('weight', 'bias'))
    for i, p in enumerate(PLANES):
        lin = getattr(m, f'position_layer_{p}')
        assert type(lin) is TallLinear and lin.weight.shape == (cfg['embed_dims'], 4 * cfg['num_freqs'][i])
        buf = m.get_buffer(f'{p}_freq_feat')
        ref = torch.tensor(GOLD[f'{name}.buf.{p}_freq_feat'])
        assert buf.shape == ref.shape
        assert torch.allclose(buf, ref, atol=1e-6), (p, (buf - ref).abs().max())
    assert dict(m.named_buffers()).keys() == {f'{p}_freq_feat' for p in PLANES}


@pytest.mark.parametrize("name", ['linear', 'linear_upscale'])
def test_outputs_and_gradients_on_cpu(name):
    m = build(name)
    bs = CFG['bs']
    outs = m([torch.zeros(bs, 1)])['representation']
    assert len(outs) == 3
    loss = 0.
    for p, o in zip(PLANES, outs):
        ref = torch.tensor(GOLD[f'{name}.out.{p}'])
        assert o.shape == ref.shape and o.shape[0] == bs
        assert torch.allclose(o, ref, rtol=1e-4, atol=1e-4), (p, (o - ref).abs().max())
        loss = loss + (o * torch.tensor(GOLD[f'{name}.G.{p}'])).sum()
    loss.backward()
    for k, prm in m.named_parameters():
        ref = torch.tensor(GOLD[f'{name}.grad.{k}'])
        assert (prm.grad - ref).abs().max() <= 1e-4 * ref.abs().max(), k
    # an expanded view of one (N, C) plane, not bs copies
    assert all(o.stride(0) == 0 for o in outs)


def test_feature_order_is_coord_freq_sincos():
    """freqs = pi * 2^(k - 1), k = 0 .. F-1; per row [coord][freq][sin, cos] of the metres normalised by tot_range"""
    m = build('linear')
    cfg = CFG['lifters']['linear']
    r, F = cfg['tot_range'], cfg['num_freqs'][1]
    # plane zh: cell (z, h) -> metres (y of h, z of z), normalised by the y and z ranges
    from selfocc_amd.mapping import GridMeterMapping
    mp = GridMeterMapping(**cfg['mapping_args'])
    z, h = 2, 5
    met = mp.grid2meter(torch.tensor([[float(h), 0.0, float(z)]]))[0]
    n = [(met[1].item() - r[1]) / (r[4] - r[1]), (met[2].item() - r[2]) / (r[5] - r[2])]
    row = m.zh_freq_feat[z * mp.size_h + h]
    want = [fn(torch.tensor(c * np.pi * 2.0 ** (k - 1), dtype=torch.float32)) for c in n for k in range(F)
            for fn in (torch.sin, torch.cos)]
    assert torch.allclose(row, torch.stack(want), atol=1e-5)


def test_shim_model_lifter_exposes_the_class(tmp_path):
    ref = tmp_path / "SelfOcc"
    for sub in ("backbone", "neck", "segmentor", "lifter"):
        (ref / "model" / sub).mkdir(parents=True)
        (ref / "model" / sub / "__init__.py").write_text(
            "raise RuntimeError('reference lifter imported')\n" if sub == "lifter" else "")
    (ref / "model" / "__init__.py").write_text("raise RuntimeError('the reference model/__init__.py ran')\n")
    (ref / "stub.py").write_text(textwrap.dedent("""
        import model
        from model.lifter import TPVPositionLifter
        import selfocc_amd.registry as R
        assert R.MODELS.get('TPVPositionLifter') is TPVPositionLifter
        assert TPVPositionLifter.__module__ == 'selfocc_amd.model.lifter'
        print('SHIM-OK')
        """))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "shim"))
    r = subprocess.run([sys.executable, "stub.py"], cwd=ref, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SHIM-OK" in r.stdout, r.stdout + r.stderr
