"""GPU: the fused field MLP at the two widths a spherical-harmonics head asks of it — (out_dim, feature stride) = (13, 12) for
degree 1 and (28, 28) for degree 2 — at 257 x 257 x 25 voxels, C = 96, two Linears, through FieldVolumeFunction and field_volume,
against float64 autograd.  Inputs, reference, error measure and kernel identification are those of
tests/test_field_full_size_gpu.py (imported).  Both strides are multiples of 4 floats: the dispatch takes the b3 backward.

Bounds follow that file's rule — 10 x the per-tensor (rel-L2, max / max) errors measured on MI355X (MEASURED, log line kept
under parity_out/) — and none exceeds the largest bound that file holds for the same tensor over its SHIPPED cases."""
import math
import time

import pytest
import torch

from selfocc_amd.field import field_volume, field_volume_supported, field_volume_train_supported
import test_field_full_size_gpu as ff
from test_field_full_size_gpu import make_inputs, reference64, kernel_backward, err

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
H, W, D = 257, 257, 25
CASES = {"sh_deg1": (13, 12), "sh_deg2": (28, 28)}

# (rel-L2, max |g - g64| / max |g64|) measured on MI355X, the largest of two sessions x the normal and the DBG launch where the DBG launch leaves
# the gradient alone (parity_out/field_full_size_parity.jsonl, cases sh_deg1 / sh_deg2)
MEASURED = {
    "sh_deg1": dict(hw=(2.3e-7, 2.8e-7), zh=(3.7e-7, 3.0e-7), wz=(3.7e-7, 3.9e-7), w1=(4.3e-6, 4.1e-6), b1=(9.7e-6, 9.2e-6),
                    w2=(1.3e-6, 1.6e-6), b2=(8.7e-7, 1.4e-6), sdf=(1.5e-7, 4.5e-7), feat=(1.9e-7, 3.9e-7)),
    "sh_deg2": dict(hw=(2.5e-7, 5.6e-7), zh=(3.6e-7, 4.4e-7), wz=(3.6e-7, 4.5e-7), w1=(6.2e-6, 3.5e-6), b1=(8.0e-6, 5.2e-6),
                    w2=(2.1e-6, 1.9e-6), b2=(8.7e-7, 1.5e-6), sdf=(5.0e-7, 1.5e-6), feat=(2.4e-7, 6.2e-7)),
}
TENSORS = ff.GRADS + ("sdf", "feat")
CEILING = {t: tuple(10 * max(ff.MEASURED[c.name][t][k] for c in ff.SHIPPED if t in ff.MEASURED[c.name]) for k in (0, 1)) for t in TENSORS}


def _bounds(name):
    return {t: tuple(min(10 * MEASURED[name][t][k], CEILING[t][k]) for k in (0, 1)) for t in TENSORS}


@pytest.mark.parametrize("name", list(CASES))
def test_field_mlp_at_sh_widths_vs_float64(hip, monkeypatch, name):
    t0 = time.time()
    out_dim, F = CASES[name]
    assert field_volume_supported(96, 2, out_dim, F) and field_volume_train_supported(96, 2, out_dim, F, torch.float32)
    monkeypatch.delenv("SELFOCC_FIELD_BWD_DBG", raising=False)
    size = (H, W, D)
    planes, lins, gs, gf = make_inputs(H, W, D, 96, 2, out_dim, F, seed=H * 7919 + W * 131 + D * 17 + out_dim + F)
    out64, g64, shares = reference64(planes, lins, size, gs, gf)
    for br in ("identity", "series", "log"):
        assert shares[br] > 0.01, shares
    sdf, feat, got = kernel_backward(planes, lins, size, F, gs, gf)
    errs = {n: err(a, r) for n, a, r in zip(ff.GRADS, got, g64)}
    errs.update(ff.forward_errors(sdf, feat, out64, F))              # also: the pad channels of the feature volume are zero
    if F > out_dim - 1:
        assert feat[..., out_dim - 1:].abs().max().item() == 0.0     # channel 27 of the degree-2 volume
    bnd = _bounds(name)

    # the kernel that ran: only the b3 kernel honours SELFOCC_FIELD_BWD_DBG=1 (no zh / wz plane-gradient atomics)
    monkeypatch.setenv("SELFOCC_FIELD_BWD_DBG", "1")
    _, _, got_dbg = kernel_backward(planes, lins, size, F, gs, gf)
    monkeypatch.delenv("SELFOCC_FIELD_BWD_DBG")
    ran = "b3" if (got_dbg[1].abs().max().item() == 0 and got_dbg[2].abs().max().item() == 0) else "f32"
    errs_dbg = {n: err(a, r) for n, a, r in zip(ff.GRADS, got_dbg, g64)}
    del got_dbg

    # reference-side control: the upstream gradient of one 4 x 4 x 2 patch zeroed / doubled must leave the bounds by >= 10 x
    hb, wb, db = 4 * (H // 8), 4 * (W // 8), 2 * (D // 4)
    ctl = {}
    for factor in (0.0, 2.0):
        gs2, gf2 = gs.clone(), gf.clone()
        gs2[hb:hb + 4, wb:wb + 4, db:db + 2] *= factor
        gf2[hb:hb + 4, wb:wb + 4, db:db + 2] *= factor
        _, g64p, _ = reference64(planes, lins, size, gs2, gf2)
        ctl[f"x{factor:g}"] = {n: [e / b if b > 0 else math.inf for e, b in zip(err(a, r), bnd[n])] for n, a, r in zip(ff.GRADS, got, g64p)}
        del g64p

    fv_sdf, fv_feat = field_volume(*planes, size, ff.nn_linears(lins, 96), F)
    same = bool(torch.equal(fv_sdf, sdf) and torch.equal(fv_feat, feat))
    rec = dict(case=name, kernel=ran, size=list(size), out_dim=out_dim, F=F, shares=shares, err=errs, bound=bnd, err_dbg=errs_dbg,
               control=ctl, field_volume_equals_function_forward=same, wall_s=round(time.time() - t0, 2))
    ff.log_record(rec)
    print(f"\n[field {name}] kernel {ran} err " + ", ".join(f"{n}=({e[0]:.2e}, {e[1]:.2e})" for n, e in errs.items()))
    print(f"[field {name}] dbg " + ", ".join(f"{n}=({e[0]:.2e}, {e[1]:.2e})" for n, e in errs_dbg.items()))

    assert ran == "b3", rec
    assert same
    for n, e in errs.items():
        assert e[0] <= bnd[n][0] and e[1] <= bnd[n][1], (name, n, e, bnd[n])
    for n in ff.GRADS:
        if n in ("zh", "wz"):
            assert errs_dbg[n][0] >= 10 * bnd[n][0] and errs_dbg[n][1] >= 10 * bnd[n][1], (name, n, errs_dbg[n], bnd[n])
        else:
            assert errs_dbg[n][0] <= bnd[n][0] and errs_dbg[n][1] <= bnd[n][1], (name, n, errs_dbg[n], bnd[n])
    for k, c in ctl.items():
        for n in ff.GRADS:
            assert min(c[n]) >= 10, (name, k, n, c[n])
    ff.bf16_equals_f32_rounded_once(planes, lins, size, F, fv_feat)
