"""The width-generic float32-MFMA backward of csrc/field_bwd_w.hip (selfocc_field_volume_bwd at embed_dims 64 and 128, and at
96 with SELFOCC_FIELD_BWD_B3=0, the route of the 96-wide heads the bf16 x 3 kernel does not take) against float64 torch
autograd of test_field_gpu.reference (which calls no selfocc kernel).

Shapes are the smallest at which each mechanism of the kernel can go wrong: one voxel; patches ragged in all three axes;
whole patches with one d-patch per column; a stride that is not a multiple of four floats; the full output range; no feature
gradient; and grids with one tile more than the launch has tile slots, so that a slot walks several tiles and the hw rows of
a column of d-patches are flushed by several slots.  A slot is one wave at C = 64 and 96 (256 blocks x 4 = 1 024 slots, 1 025
tiles at 20 x 20 x 82) and a PAIR of waves at C = 128 (512 slots, 513 tiles at 12 x 36 x 38, where the last slots of a block idle
through the block barriers of the others).

Pass rule (the project's rule for this op, tests/test_field_gpu.py): allclose(rtol=1e-3, atol=1e-4 max|g64|) per tensor, no
element left out.  Per tensor rel-L2 and max|g - g64| / max|g64| go to parity_out/field_widths_parity.jsonl; the logs of the
first two MI355X sessions are profiles/field_widths_parity.jsonl, and MEASURED holds their values: the second, sharp
assertion is 10 x the measured value (the convention of tests/test_field_full_size_gpu.py: the margin is for the run-to-run
order of the atomics).

At C = 96 the cases run with SELFOCC_FIELD_BWD_DBG=1 as well: only the bf16 x 3 kernel honours that switch (it drops the zh / wz
plane-gradient atomics), so zh / wz gradients that pass name the float32 kernel as the one that ran."""
import functools
import json
import os

import pytest
import torch
import torch.nn as nn

from selfocc_amd._lib import lib, ptr, current_stream
from selfocc_amd.field import FieldVolumeFunction
from test_field_gpu import reference

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "field_widths_parity.jsonl")
GRADS = ("hw", "zh", "wz", "w1", "b1", "w2", "b2")
WIDTHS = (64, 96, 128)           # 96: the float32 route, by SELFOCC_FIELD_BWD_B3=0 (run_case)
GENERIC = (64, 128)              # the widths whose every backward is this kernel

# (H, W, D, out_dim, F)
CASES = {
    "1x1x1": (1, 1, 1, 1, 0),
    "5x3x3_F24": (5, 3, 3, 25, 24),             # ragged in all three axes
    "8x8x2_F4": (8, 8, 2, 4, 4),                # whole patches, PD = 1
    "9x7x25_F24": (9, 7, 25, 25, 24),
    "5x6x31_F0": (5, 6, 31, 1, 0),              # g_feat absent
    "4x5x11_out20_F19": (4, 5, 11, 20, 19),     # a stride that is not a multiple of 4
    "6x5x4_out32_F31": (6, 5, 4, 32, 31),       # the full output range
    "20x20x82_F24": (20, 20, 82, 25, 24),       # 1 025 tiles: the 1 024 slots of C = 64 / 96, plus one
    "12x36x38_F24": (12, 36, 38, 25, 24),       # 513 tiles: the 512 slots of C = 128, plus one
}
BITE = ("20x20x82_F24", "9x7x25_F24")

# (rel-L2, max|g - g64| / max|g64|) per (C, case) and tensor, measured on MI355X: the larger of the two sessions logged in
# profiles/field_widths_parity.jsonl, rounded up to two digits.  Everything sits at 1e-7 .. 1e-6 (float32 arithmetic end to
# end); b2 is a sum of the upstream gradient over all voxels (ONE number where out_dim = 1) and moves with the order of the
# atomics (5.9e-7 and 1.6e-6 in the two sessions at C = 128, 5 x 6 x 31); at one voxel it is the upstream gradient itself.
MEASURED = {
    (64, "1x1x1"): dict(hw=(1.3e-07, 2.2e-07), zh=(1.3e-07, 2.2e-07), wz=(1.3e-07, 2.2e-07), w1=(7.8e-08, 7.2e-08), b1=(6.4e-08, 8.4e-08), w2=(2.6e-07, 3.9e-07), b2=(0.0e+00, 0.0e+00), sdf=(2.8e-07, 2.8e-07)),
    (64, "5x3x3_F24"): dict(hw=(2.2e-07, 3.1e-07), zh=(2.3e-07, 3.3e-07), wz=(2.3e-07, 3.3e-07), w1=(1.8e-07, 2.7e-07), b1=(1.4e-07, 1.6e-07), w2=(1.9e-07, 2.6e-07), b2=(6.5e-08, 8.6e-08), sdf=(2.3e-07, 4.2e-07), feat=(2.3e-07, 2.5e-07)),
    (64, "8x8x2_F4"): dict(hw=(2.0e-07, 3.1e-07), zh=(2.0e-07, 2.4e-07), wz=(2.1e-07, 2.8e-07), w1=(2.0e-07, 1.7e-07), b1=(2.1e-07, 2.1e-07), w2=(2.9e-07, 2.3e-07), b2=(8.2e-08, 1.2e-07), sdf=(2.6e-07, 5.0e-07), feat=(2.4e-07, 2.5e-07)),
    (64, "9x7x25_F24"): dict(hw=(2.3e-07, 1.6e-07), zh=(2.2e-07, 2.4e-07), wz=(2.2e-07, 2.0e-07), w1=(2.6e-07, 5.3e-07), b1=(2.2e-07, 2.3e-07), w2=(2.6e-07, 3.5e-07), b2=(1.7e-07, 2.5e-07), sdf=(2.2e-07, 3.4e-07), feat=(2.2e-07, 3.5e-07)),
    (64, "5x6x31_F0"): dict(hw=(2.1e-07, 2.5e-07), zh=(2.0e-07, 2.2e-07), wz=(2.0e-07, 2.2e-07), w1=(2.4e-07, 1.8e-07), b1=(2.4e-07, 2.8e-07), w2=(4.4e-07, 6.1e-07), b2=(4.2e-07, 4.2e-07), sdf=(2.7e-07, 3.6e-07)),
    (64, "4x5x11_out20_F19"): dict(hw=(2.1e-07, 2.5e-07), zh=(2.0e-07, 2.5e-07), wz=(2.1e-07, 2.6e-07), w1=(1.8e-07, 1.6e-07), b1=(1.5e-07, 1.3e-07), w2=(2.0e-07, 1.9e-07), b2=(8.5e-08, 1.3e-07), sdf=(1.9e-07, 4.1e-07), feat=(2.3e-07, 3.0e-07)),
    (64, "6x5x4_out32_F31"): dict(hw=(2.2e-07, 2.4e-07), zh=(2.2e-07, 1.8e-07), wz=(2.1e-07, 2.8e-07), w1=(1.8e-07, 1.4e-07), b1=(1.6e-07, 1.1e-07), w2=(2.4e-07, 4.2e-07), b2=(1.2e-07, 1.5e-07), sdf=(3.7e-07, 3.9e-07), feat=(2.4e-07, 3.1e-07)),
    (64, "20x20x82_F24"): dict(hw=(2.5e-07, 2.9e-07), zh=(2.2e-07, 2.4e-07), wz=(2.3e-07, 2.2e-07), w1=(6.3e-07, 1.1e-06), b1=(7.1e-07, 1.1e-06), w2=(6.5e-07, 8.8e-07), b2=(5.7e-07, 6.6e-07), sdf=(3.3e-07, 4.9e-07), feat=(2.6e-07, 3.5e-07)),
    (64, "12x36x38_F24"): dict(hw=(2.3e-07, 2.5e-07), zh=(2.3e-07, 2.6e-07), wz=(2.2e-07, 2.1e-07), w1=(4.6e-07, 7.7e-07), b1=(4.6e-07, 5.4e-07), w2=(4.7e-07, 5.8e-07), b2=(4.3e-07, 6.2e-07), sdf=(3.4e-07, 6.5e-07), feat=(2.6e-07, 5.2e-07)),
    (96, "1x1x1"): dict(hw=(2.7e-07, 3.5e-07), zh=(2.7e-07, 3.5e-07), wz=(2.7e-07, 3.5e-07), w1=(1.7e-07, 4.3e-07), b1=(1.6e-07, 4.5e-07), w2=(2.2e-07, 2.2e-07), b2=(0.0e+00, 0.0e+00), sdf=(2.3e-08, 2.3e-08)),
    (96, "5x3x3_F24"): dict(hw=(2.3e-07, 2.7e-07), zh=(2.2e-07, 2.6e-07), wz=(2.4e-07, 2.3e-07), w1=(1.7e-07, 2.5e-07), b1=(1.3e-07, 1.8e-07), w2=(2.2e-07, 2.0e-07), b2=(7.8e-08, 1.2e-07), sdf=(3.0e-07, 3.3e-07), feat=(2.5e-07, 2.5e-07)),
    (96, "8x8x2_F4"): dict(hw=(2.5e-07, 2.8e-07), zh=(2.7e-07, 2.7e-07), wz=(2.3e-07, 1.8e-07), w1=(2.3e-07, 4.0e-07), b1=(1.9e-07, 2.3e-07), w2=(3.4e-07, 3.7e-07), b2=(2.4e-07, 1.9e-07), sdf=(2.5e-07, 3.6e-07), feat=(2.6e-07, 3.2e-07)),
    (96, "9x7x25_F24"): dict(hw=(2.5e-07, 2.3e-07), zh=(2.5e-07, 2.6e-07), wz=(2.4e-07, 2.9e-07), w1=(2.5e-07, 3.8e-07), b1=(2.3e-07, 4.3e-07), w2=(2.7e-07, 3.3e-07), b2=(1.7e-07, 1.7e-07), sdf=(2.8e-07, 5.9e-07), feat=(2.4e-07, 3.5e-07)),
    (96, "5x6x31_F0"): dict(hw=(2.4e-07, 2.5e-07), zh=(2.0e-07, 2.6e-07), wz=(2.1e-07, 2.4e-07), w1=(2.4e-07, 3.8e-07), b1=(2.6e-07, 2.8e-07), w2=(3.6e-07, 4.7e-07), b2=(1.4e-07, 1.4e-07), sdf=(3.8e-07, 8.1e-07)),
    (96, "4x5x11_out20_F19"): dict(hw=(2.5e-07, 2.8e-07), zh=(2.4e-07, 3.4e-07), wz=(2.4e-07, 2.5e-07), w1=(2.3e-07, 3.5e-07), b1=(2.0e-07, 2.3e-07), w2=(2.3e-07, 3.0e-07), b2=(7.6e-08, 1.2e-07), sdf=(2.1e-07, 2.2e-07), feat=(2.3e-07, 3.3e-07)),
    (96, "6x5x4_out32_F31"): dict(hw=(2.5e-07, 3.0e-07), zh=(2.4e-07, 2.4e-07), wz=(2.6e-07, 2.2e-07), w1=(2.2e-07, 2.7e-07), b1=(2.2e-07, 2.3e-07), w2=(2.5e-07, 3.2e-07), b2=(8.7e-08, 1.1e-07), sdf=(2.8e-07, 1.7e-07), feat=(2.5e-07, 4.8e-07)),
    (96, "20x20x82_F24"): dict(hw=(2.7e-07, 3.5e-07), zh=(2.4e-07, 2.7e-07), wz=(2.4e-07, 2.2e-07), w1=(6.0e-07, 9.9e-07), b1=(6.0e-07, 7.0e-07), w2=(6.5e-07, 9.7e-07), b2=(5.0e-07, 6.0e-07), sdf=(3.1e-07, 5.1e-07), feat=(2.3e-07, 3.9e-07)),
    (96, "12x36x38_F24"): dict(hw=(2.5e-07, 3.0e-07), zh=(2.5e-07, 2.7e-07), wz=(2.4e-07, 2.7e-07), w1=(4.5e-07, 9.2e-07), b1=(4.3e-07, 5.3e-07), w2=(5.1e-07, 8.4e-07), b2=(4.7e-07, 5.8e-07), sdf=(3.1e-07, 4.7e-07), feat=(2.3e-07, 3.5e-07)),
    (128, "1x1x1"): dict(hw=(2.2e-07, 2.8e-07), zh=(2.2e-07, 2.8e-07), wz=(2.2e-07, 2.8e-07), w1=(1.1e-07, 1.4e-07), b1=(8.4e-08, 1.2e-07), w2=(2.7e-07, 3.7e-07), b2=(0.0e+00, 0.0e+00), sdf=(1.7e-06, 1.7e-06)),
    (128, "5x3x3_F24"): dict(hw=(2.7e-07, 2.5e-07), zh=(2.7e-07, 3.5e-07), wz=(2.5e-07, 2.8e-07), w1=(2.0e-07, 1.9e-07), b1=(1.6e-07, 1.5e-07), w2=(2.7e-07, 3.3e-07), b2=(6.0e-08, 7.2e-08), sdf=(2.7e-07, 3.8e-07), feat=(3.4e-07, 3.8e-07)),
    (128, "8x8x2_F4"): dict(hw=(2.6e-07, 3.1e-07), zh=(2.6e-07, 1.7e-07), wz=(2.6e-07, 3.0e-07), w1=(1.9e-07, 3.2e-07), b1=(1.5e-07, 1.3e-07), w2=(2.5e-07, 2.7e-07), b2=(3.2e-08, 2.6e-08), sdf=(4.0e-07, 4.8e-07), feat=(3.9e-07, 4.7e-07)),
    (128, "9x7x25_F24"): dict(hw=(2.7e-07, 2.5e-07), zh=(2.7e-07, 3.1e-07), wz=(2.7e-07, 3.0e-07), w1=(2.5e-07, 3.0e-07), b1=(2.5e-07, 2.4e-07), w2=(3.0e-07, 3.6e-07), b2=(2.2e-07, 3.1e-07), sdf=(4.4e-07, 5.5e-07), feat=(3.0e-07, 4.3e-07)),
    (128, "5x6x31_F0"): dict(hw=(2.7e-07, 3.2e-07), zh=(2.7e-07, 2.6e-07), wz=(2.6e-07, 2.4e-07), w1=(2.4e-07, 1.8e-07), b1=(3.0e-07, 2.6e-07), w2=(3.8e-07, 5.9e-07), b2=(1.6e-06, 1.6e-06), sdf=(3.5e-07, 4.9e-07)),
    (128, "4x5x11_out20_F19"): dict(hw=(2.7e-07, 3.2e-07), zh=(2.6e-07, 2.5e-07), wz=(2.7e-07, 2.3e-07), w1=(2.2e-07, 2.4e-07), b1=(2.0e-07, 1.6e-07), w2=(2.8e-07, 3.5e-07), b2=(1.4e-07, 2.1e-07), sdf=(2.4e-07, 3.5e-07), feat=(3.2e-07, 3.8e-07)),
    (128, "6x5x4_out32_F31"): dict(hw=(3.0e-07, 2.7e-07), zh=(2.9e-07, 2.6e-07), wz=(2.9e-07, 3.1e-07), w1=(2.1e-07, 3.2e-07), b1=(1.8e-07, 2.1e-07), w2=(2.4e-07, 1.9e-07), b2=(8.6e-08, 1.2e-07), sdf=(3.5e-07, 3.9e-07), feat=(3.3e-07, 2.8e-07)),
    (128, "20x20x82_F24"): dict(hw=(2.8e-07, 3.0e-07), zh=(2.7e-07, 2.9e-07), wz=(2.7e-07, 2.7e-07), w1=(4.9e-07, 6.9e-07), b1=(5.4e-07, 8.7e-07), w2=(5.3e-07, 6.5e-07), b2=(5.4e-07, 6.7e-07), sdf=(2.4e-07, 4.8e-07), feat=(3.0e-07, 6.5e-07)),
    (128, "12x36x38_F24"): dict(hw=(2.9e-07, 2.8e-07), zh=(2.9e-07, 3.3e-07), wz=(2.8e-07, 2.9e-07), w1=(4.6e-07, 8.8e-07), b1=(4.6e-07, 5.4e-07), w2=(5.0e-07, 6.8e-07), b2=(3.4e-07, 3.2e-07), sdf=(2.8e-07, 4.6e-07), feat=(3.2e-07, 4.3e-07)),
}


def n_tiles(H, W, D):
    return -(-H // 4) * -(-W // 4) * -(-D // 2)


def err(got, ref):
    d = got.double() - ref
    return ((d.norm() / ref.norm().clamp_min(1e-300)).item(), (d.abs().max() / ref.abs().max().clamp_min(1e-300)).item())


def passes(got, ref):
    """the pass rule of this op"""
    return torch.allclose(got.double(), ref, rtol=1e-3, atol=1e-4 * ref.abs().max().item())


def make_inputs(C, name):
    H, W, D, out_dim, F = CASES[name]
    g = torch.Generator().manual_seed(H * 100 + W * 10 + D + C)
    hw, zh, wz = (torch.randn(n, C, generator=g) * 1.2 for n in (H * W, D * H, W * D))
    hw[0, :8] = torch.tensor([-30.0, -12.0, -4.0, -1.0, 0.0, 6.0, 19.0, 25.0])     # every Softplus regime
    l1, l2 = nn.Linear(C, C), nn.Linear(C, out_dim)
    for l in (l1, l2):
        nn.init.normal_(l.weight, std=0.3, generator=g)
        nn.init.normal_(l.bias, std=0.5, generator=g)
    gs = torch.randn(H, W, D, generator=g)
    gf = torch.randn(H, W, D, F, generator=g) if F else None
    return (hw, zh, wz), (l1, l2), gs, gf


def reference64(planes, lins, size, out_dim, gs, gf):
    """float64 autograd of test_field_gpu.reference on the CPU: (out, the seven gradients)"""
    leaves = [t.detach().double().requires_grad_(True) for t in planes]
    l64 = [nn.Linear(l.in_features, l.out_features).double() for l in lins]
    for a, b in zip(l64, lins):
        a.load_state_dict({k: v.double() for k, v in b.state_dict().items()})
    out = reference(*leaves, size, l64)
    up = torch.zeros_like(out)
    up[..., 0] = gs.double()
    if gf is not None and out_dim > 1:
        up[..., 1:] = gf[..., :out_dim - 1].double()
    out.backward(up)
    return out.detach(), [t.grad for t in leaves] + [l64[0].weight.grad, l64[0].bias.grad, l64[1].weight.grad, l64[1].bias.grad]


@functools.lru_cache(maxsize=None)
def run_case(C, name):
    """One case, once: inputs, the float64 reference and the kernel's results (shared by the tests; nothing mutates them).
    The switches that select the kernel are part of what is cached: they are set here, around the launch."""
    H, W, D, out_dim, F = CASES[name]
    planes, lins, gs, gf = make_inputs(C, name)
    out64, g64 = reference64(planes, lins, (H, W, D), out_dim, gs, gf)
    dev = [t.detach().clone().to(D0).requires_grad_(True)
           for t in (*planes, lins[0].weight, lins[0].bias, lins[1].weight, lins[1].bias)]
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("SELFOCC_FIELD_BWD_B3", raising=False)
        mp.delenv("SELFOCC_FIELD_BWD_DBG", raising=False)
        if C == 96:
            mp.setenv("SELFOCC_FIELD_BWD_B3", "0")
            mp.setenv("SELFOCC_FIELD_BWD_DBG", "1")       # the float32 kernel ignores it; the b3 kernel would leave zh / wz zero
        sdf, feat = FieldVolumeFunction.apply(*dev, (H, W, D), F)
        torch.autograd.backward([sdf, feat] if F else [sdf], [gs.to(D0), gf.to(D0)] if F else [gs.to(D0)])
        got = [t.grad.cpu() for t in dev]
    return dict(planes=planes, lins=lins, gs=gs, gf=gf, out64=out64, g64=g64, got=got, sdf=sdf.detach().cpu(),
                feat=feat.detach().cpu() if F else None)


def log_record(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("C", WIDTHS)
def test_backward_vs_float64_autograd(hip, C, name):
    """All seven gradients and the forward outputs of FieldVolumeFunction against float64 autograd."""
    H, W, D, out_dim, F = CASES[name]
    r = run_case(C, name)
    errs = {n: err(a, b) for n, a, b in zip(GRADS, r["got"], r["g64"])}
    errs["sdf"] = err(r["sdf"], r["out64"][..., 0])
    if F and out_dim > 1:
        errs["feat"] = err(r["feat"][..., :out_dim - 1], r["out64"][..., 1:])
    slots = 512 if C == 128 else 1024
    log_record(dict(C=C, case=name, size=[H, W, D], out_dim=out_dim, F=F, tiles=n_tiles(H, W, D), slots=slots, err=errs))
    print(C, name, errs)
    # forward outputs: the rule of test_field_volume_vs_torch
    scale = r["out64"].abs().max().item()
    assert torch.allclose(r["sdf"].double(), r["out64"][..., 0], rtol=1e-4, atol=1e-5 * scale)
    if F:
        assert r["feat"].shape == (H, W, D, F)
        assert torch.allclose(r["feat"][..., :out_dim - 1].double(), r["out64"][..., 1:], rtol=1e-4, atol=1e-5 * scale)
        assert torch.all(r["feat"][..., out_dim - 1:] == 0)
    for n, a, b in zip(GRADS, r["got"], r["g64"]):
        assert a.shape == b.shape
        assert passes(a, b), (C, name, n, errs[n])
    if C == 96:                               # the float32 kernel ran: SELFOCC_FIELD_BWD_DBG=1 took no zh / wz gradient away
        assert r["got"][1].abs().max() > 0 and r["got"][2].abs().max() > 0
    assert set(errs) == set(MEASURED[(C, name)])
    for n, e in errs.items():                 # the sharp bound: 10 x the measured value
        m = MEASURED[(C, name)][n]
        assert e[0] <= 10 * m[0] and e[1] <= 10 * m[1], (C, name, n, e, m)


@pytest.mark.parametrize("name", BITE)
@pytest.mark.parametrize("C", WIDTHS)
def test_bounds_catch_a_dropped_patch(hip, C, name):
    """The reference recomputed with the upstream gradient of ONE 4 x 4 x 2 patch zeroed: what a kernel that dropped that tile
    would be compared with.  The pass rule must reject the kernel's result against it, for the three plane gradients at least."""
    H, W, D, out_dim, F = CASES[name]
    r = run_case(C, name)
    hb, wb, db = 4 * (H // 8), 4 * (W // 8), 2 * (D // 4)
    gs2, gf2 = r["gs"].clone(), r["gf"].clone()
    gs2[hb:hb + 4, wb:wb + 4, db:db + 2] = 0
    gf2[hb:hb + 4, wb:wb + 4, db:db + 2] = 0
    _, g64p = reference64(r["planes"], r["lins"], (H, W, D), out_dim, gs2, gf2)
    for n, a, b in list(zip(GRADS, r["got"], g64p))[:3]:
        assert not passes(a, b), (C, name, n, err(a, b))
        e, m = err(a, b), MEASURED[(C, name)][n]          # and the sharp bound, by a wide margin
        assert e[0] > 100 * m[0] and e[1] > 100 * m[1], (C, name, n, e, m)


def _abi_call(C, H, W, D, out_dim, fill=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(D0)
    hw, zh, wz = rn(H * W, C), rn(D * H, C), rn(W * D, C)
    w1, b1, w2 = rn(C, C) * 0.3, rn(C) * 0.5, rn(out_dim, C) * 0.3
    gs = rn(H, W, D)
    grads = [torch.full_like(t, fill) for t in (hw, zh, wz, w1, b1, w2)] + [torch.full((out_dim,), fill, device=D0)]
    rc = lib().selfocc_field_volume_bwd(ptr(hw), ptr(zh), ptr(wz), H, W, D, C, ptr(w1), ptr(b1), ptr(w2), out_dim, ptr(gs), None,
                                        0, *(ptr(t) for t in grads), current_stream(D0))
    torch.cuda.synchronize()
    return rc, grads


@pytest.mark.parametrize("C", GENERIC)
def test_c_abi_without_feature_gradient(hip, C):
    """g_feat = NULL, out_dim = 4: the output layer's feature rows receive exactly nothing, the SDF row something."""
    rc, g = _abi_call(C, 6, 7, 5, 4)
    assert rc == 0, lib().selfocc_last_error().decode()
    assert torch.all(g[5][1:] == 0) and torch.all(g[6][1:] == 0)
    assert g[5][0].abs().min() > 0 and g[6][0] != 0
    for t in g[:5]:
        assert torch.isfinite(t).all() and t.abs().max() > 0


@pytest.mark.parametrize("C", (80, 256))
def test_c_abi_refuses_other_widths(hip, C):
    rc, g = _abi_call(C, 3, 3, 3, 4, fill=7.0)
    assert rc < 0
    assert "64, 96 or 128" in lib().selfocc_last_error().decode()
    for t in g:
        assert torch.all(t == 7.0)            # no gradient buffer was touched


@pytest.mark.parametrize("C", GENERIC)
def test_through_the_field(hip, C):
    """SDFField at the 32 x 32 x 12 mapping of test_sdffield_fused_equals_unfused: under grad it takes FieldVolumeFunction,
    its gradients equal the op-by-op route's, and inference is unchanged."""
    from selfocc_amd.model.head.neus_head import SDFField
    mapping_args = dict(nonlinear_mode='linear', h_size=[32, 0], h_range=[40.0, 0], h_half=False, w_size=[32, 0],
                        w_range=[40.0, 0], w_half=False, d_size=[12, 0], d_range=[-1.0, 5.4, 5.4])
    torch.manual_seed(3)
    f = SDFField(mapping_args, embed_dims=C, color_dims=24, density_layers=2, sh_deg=0, tpv=True, return_sem=True).to(D0)
    H, W, D = f.size_h, f.size_w, f.size_d
    rep = [torch.randn(1, H * W, C, device=D0), torch.randn(1, D * H, C, device=D0), torch.randn(1, W * D, C, device=D0)]
    with torch.no_grad():
        fused = f.pre_compute_density_color(rep)
        f.fused_volume = False
        plain = f.pre_compute_density_color(rep)
    assert fused.sdf.shape == plain.sdf.shape and fused.feat.shape == plain.feat.shape
    assert torch.allclose(fused.sdf, plain.sdf, rtol=1e-4, atol=1e-5)
    assert torch.allclose(fused.feat, plain.feat, rtol=1e-4, atol=1e-5)
    grads = {}
    for fused in (True, False):
        f.fused_volume = fused
        f.zero_grad()
        reps = [r.clone().requires_grad_(True) for r in rep]
        vol = f.pre_compute_density_color(reps)
        assert vol.sdf.requires_grad
        assert (type(vol.sdf.grad_fn).__name__ == 'FieldVolumeFunctionBackward') == fused
        (vol.sdf.square().mean() + vol.feat.square().mean()).backward()
        grads[fused] = [r.grad.clone() for r in reps] + [p.grad.clone() for p in f.density_net.parameters()]
    f.fused_volume = True
    for a, b in zip(grads[True], grads[False]):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-4 * b.abs().max().item())


def test_a_128_wide_head_trains(hip, monkeypatch):
    """NeuSHead(embed_dims=128) at the small shapes of test_render_nsem_gpu: one forward + backward through the fused field."""
    import numpy as np
    import test_render_nsem_gpu as nsem
    from selfocc_amd.registry import OPENOCC_LOSS
    monkeypatch.setattr(nsem, "C", 128)              # _head's embed_dims and _inputs' plane width
    monkeypatch.setenv('eval', 'false')
    head = nsem._head(color_dims=23, return_sem=True).train()
    f = head.model.field
    assert f.embed_dims == 128 and f.fused_volume
    rep, metas, imgs = nsem._inputs(20)
    assert rep[0].shape[-1] == 128
    np.random.seed(0)
    out = head(rep, metas, global_iter=0)
    assert type(f.volume.sdf.grad_fn).__name__ == 'FieldVolumeFunctionBackward'
    loss_fn = OPENOCC_LOSS.build(dict(type='MultiLoss', loss_cfgs=[
        dict(type='SemCELossMS', weight=1.0, img_size=[64, 64], ray_resize=[6, 10],
             input_dict={'sem': 'sem', 'metas': 'metas', 'ms_rays': 'ms_rays'}),
        dict(type='RGBLossMS', weight=0.1, img_size=[64, 64], no_ssim=False, ray_resize=[6, 10],
             input_dict={'ms_colors': 'ms_colors', 'ms_rays': 'ms_rays', 'gt_imgs': 'curr_imgs'})]))
    total, _ = loss_fn(dict(out, metas=metas, curr_imgs=imgs))
    assert torch.isfinite(total)
    total.backward()
    for p in f.density_net.parameters():
        assert torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    for r in rep:
        assert torch.isfinite(r.grad).all() and r.grad.abs().sum() > 0
