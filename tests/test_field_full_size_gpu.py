"""The fused field MLP (selfocc_field_volume_fwd / selfocc_field_volume_bwd) against float64 autograd at the volume sizes the
TPV configs train at, and at the work-distribution and dispatch edges of its kernels.

At these sizes every wave walks many tiles.  The backward (at most 256 blocks x 4 waves) gives each wave a contiguous range of
4 x 4 x 2 tiles, d-patches fastest, carries the hw-plane sums of the current (h, w) column across its d-patches, flushes them
when the column changes and when the range ends (ranges start and end mid-column: most hw rows receive flushes from two
waves), and keeps dW1 / dW2 / db1 / db2 over its whole range.  The forward's persistent waves grid-stride over 32-voxel tiles.
tests/test_field_gpu.py stops where every wave runs at most one tile.

The reference is the formula of test_field_gpu.reference (x = hw + zh + wz, then [Softplus, Linear] x n) under torch autograd
in float64 on the GPU, over h-slabs whose gradients accumulate in the float64 leaves (~1 GB instead of ~10 GB); it calls no
selfocc kernel.  Errors are per tensor: rel-L2 and max |g - g64| / max |g64|, never relative to an element's own value (both
backward kernels form sigmoid as 1 - exp(-softplus), accurate only to an ulp of 1 where x << 0).  Measured values go to
parity_out/field_full_size_parity.jsonl; every bound is 10 x the value measured on MI355X (MEASURED).  Each backward case
also shows that its bounds catch a wrong tile (the reference recomputed with the upstream gradient of one 4 x 4 x 2 patch
zeroed and doubled) and names the kernel that ran: SELFOCC_FIELD_BWD_DBG=1 (read at every launch) makes the b3 kernel skip the
zh / wz plane-gradient atomics, which those bounds must flag while the other five gradients still pass; the float32 kernel
ignores the switch."""
import json
import math
import os
import time
from collections import namedtuple

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from selfocc_amd._lib import lib, check, ptr, current_stream
from selfocc_amd.field import FieldVolumeFunction, field_volume

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "field_full_size_parity.jsonl")
GRADS = ("hw", "zh", "wz", "w1", "b1", "w2", "b2")
SERIES_BELOW = math.log(0.05)      # the kernels' Softplus: log1p series where exp(x) < 0.05, log(1 + e) up to 20, x above
BWD_WAVES = 256 * 4                # the backward kernels' grid: at most 256 blocks of 4 waves

# kernel: the backward the dispatch in field.hip takes (b3 unless the feature rows are not a multiple of 4 floats);
# abi: through selfocc_field_volume_bwd directly, g_feat = NULL
Case = namedtuple("Case", "name H W D out_dim F kernel abi", defaults=(False,))
SHIPPED = [
    Case("nuscenes_occ", 257, 257, 25, 25, 24, "b3"),
    Case("nuscenes_depth", 257, 257, 31, 1, 0, "b3"),
    Case("kitti", 257, 257, 33, 4, 4, "b3"),
    Case("kitti_h129", 129, 257, 33, 4, 4, "b3"),            # non-square: an h / w mix-up in the plane gradients shows
    Case("rgb3_sem16", 257, 257, 25, 20, 19, "f32"),         # 3 colours + 16 classes: F = 19, the float32-MFMA kernel
]
EDGES = [
    Case("20x20x82_F24", 20, 20, 82, 25, 24, "b3"),          # 1 025 tiles; columns of 41 tiles flushed by many waves
    Case("20x20x82_F19", 20, 20, 82, 20, 19, "f32"),
    Case("257x257x2_F24", 257, 257, 2, 25, 24, "b3"),        # PD = 1: every tile is its own column
    Case("257x257x2_F19", 257, 257, 2, 20, 19, "f32"),
    Case("257x257x1", 257, 257, 1, 4, 4, "b3"),              # ragged in d in every tile
    Case("257x6x25", 257, 6, 25, 25, 24, "b3"),              # ragged in w, ranges crossing columns
    Case("out32_F0", 52, 60, 21, 32, 0, "b3"),               # fb_w2_row's full range, SDF at o' = 31
    Case("out32_F31", 52, 60, 21, 32, 31, "f32"),
    Case("abi_out4_F0", 52, 60, 21, 4, 0, "b3", True),       # feature rows of dW2 / db2 exactly zero
]
FwdCase = namedtuple("FwdCase", "name H W D C n_linear out_dim F")
FWD_GENERIC = [                                              # field_volume_kernel, ~1 M voxels: several tiles per wave
    FwdCase("C64", 101, 103, 100, 64, 2, 25, 24),
    FwdCase("C128", 101, 103, 100, 128, 2, 1, 0),
    FwdCase("C96_one_linear", 101, 103, 100, 96, 1, 20, 19),
]

# Errors measured on MI355X (parity_out/field_full_size_parity.jsonl), per case and tensor: (rel-L2, max |g - g64| / max |g64|),
# the largest of two sessions x (the normal launch, and the DBG launch for the gradients it leaves alone).  Every bound is 10 x
# the measured value.  The plane gradients and the forward outputs sit at 2e-7 .. 1.4e-6 everywhere; b2 is a sum of the upstream
# gradient over all voxels (one number when out_dim = 1 or F = 0) and varies with the order of the atomics.  The weight gradients
# of the b3 kernel grow with the voxel count (b1 rel-L2 1.3e-6 at 33 k voxels, 9e-6 at 1.65 M, 2e-5 at 2.2 M) where the float32
# kernel's stay below 1e-6: its errors have one sign (err_sign in the log: -1.0 for w1 and b1, -0.3 .. -0.7 for the planes;
# about 0 for the float32 kernel), so the sums over all voxels collect them.
MEASURED = {
    "nuscenes_occ": dict(hw=(2.2e-7, 3.9e-7), zh=(3.4e-7, 4.4e-7), wz=(3.3e-7, 3.2e-7), w1=(7.0e-6, 4.2e-6), b1=(9.0e-6, 4.7e-6),
                         w2=(2.2e-6, 1.8e-6), b2=(8.0e-7, 8.6e-7), sdf=(1.7e-7, 4.7e-7), feat=(1.8e-7, 4.5e-7)),
    "nuscenes_depth": dict(hw=(2.4e-7, 3.7e-7), zh=(3.9e-7, 3.7e-7), wz=(3.8e-7, 3.4e-7), w1=(1.4e-5, 9.2e-6), b1=(2.0e-5, 2.0e-5),
                           w2=(4.4e-6, 7.6e-6), b2=(9.3e-7, 9.3e-7), sdf=(1.8e-7, 5.7e-7)),
    "kitti": dict(hw=(2.3e-7, 3.7e-7), zh=(3.5e-7, 4.2e-7), wz=(3.5e-7, 3.0e-7), w1=(1.2e-5, 6.7e-6), b1=(2.1e-5, 1.2e-5),
                  w2=(3.1e-6, 2.2e-6), b2=(1.6e-6, 1.6e-6), sdf=(2.1e-7, 6.2e-7), feat=(2.1e-7, 5.8e-7)),
    "kitti_h129": dict(hw=(2.5e-7, 3.4e-7), zh=(3.9e-7, 4.3e-7), wz=(3.1e-7, 2.5e-7), w1=(4.5e-6, 4.1e-6), b1=(1.2e-5, 1.3e-5),
                       w2=(1.1e-6, 1.4e-6), b2=(8.8e-7, 1.0e-6), sdf=(1.9e-7, 6.5e-7), feat=(2.5e-7, 6.3e-7)),
    "rgb3_sem16": dict(hw=(2.6e-7, 4.2e-7), zh=(2.9e-7, 3.2e-7), wz=(2.9e-7, 3.6e-7), w1=(1.0e-6, 1.5e-6), b1=(7.1e-7, 8.1e-7),
                       w2=(1.0e-6, 2.0e-6), b2=(6.1e-7, 6.3e-7), sdf=(2.3e-7, 7.7e-7), feat=(2.3e-7, 5.6e-7)),
    "20x20x82_F24": dict(hw=(2.7e-7, 4.2e-7), zh=(2.2e-7, 2.0e-7), wz=(2.2e-7, 2.3e-7), w1=(7.5e-7, 1.2e-6), b1=(1.3e-6, 8.7e-7),
                         w2=(5.5e-7, 7.0e-7), b2=(6.9e-7, 1.1e-6), sdf=(3.6e-7, 7.9e-7), feat=(2.1e-7, 4.6e-7)),
    "20x20x82_F19": dict(hw=(2.7e-7, 4.7e-7), zh=(2.4e-7, 2.5e-7), wz=(2.4e-7, 2.8e-7), w1=(7.1e-7, 1.0e-6), b1=(6.3e-7, 8.8e-7),
                         w2=(6.1e-7, 7.1e-7), b2=(8.4e-7, 1.4e-6), sdf=(4.5e-7, 1.0e-6), feat=(1.8e-7, 4.0e-7)),
    "257x257x2_F24": dict(hw=(2.2e-7, 6.8e-7), zh=(3.5e-7, 6.3e-7), wz=(3.5e-7, 3.9e-7), w1=(1.5e-6, 1.7e-6), b1=(3.5e-6, 4.4e-6),
                          w2=(6.5e-7, 1.0e-6), b2=(6.0e-7, 7.7e-7), sdf=(2.2e-7, 5.7e-7), feat=(2.1e-7, 5.0e-7)),
    "257x257x2_F19": dict(hw=(2.6e-7, 1.4e-6), zh=(3.0e-7, 5.4e-7), wz=(3.0e-7, 4.4e-7), w1=(8.7e-7, 1.8e-6), b1=(6.2e-7, 7.8e-7),
                          w2=(6.9e-7, 1.0e-6), b2=(7.9e-7, 1.1e-6), sdf=(5.1e-7, 1.4e-6), feat=(2.0e-7, 4.4e-7)),
    "257x257x1": dict(hw=(2.1e-7, 5.5e-7), zh=(3.6e-7, 3.4e-7), wz=(3.7e-7, 2.5e-7), w1=(1.7e-6, 2.8e-6), b1=(2.3e-6, 2.2e-6),
                      w2=(8.2e-7, 1.3e-6), b2=(6.8e-7, 6.2e-7), sdf=(1.8e-7, 5.0e-7), feat=(2.0e-7, 5.1e-7)),
    "257x6x25": dict(hw=(2.3e-7, 3.4e-7), zh=(2.2e-7, 4.7e-7), wz=(3.5e-7, 3.8e-7), w1=(1.2e-6, 1.5e-6), b1=(1.3e-6, 1.0e-6),
                     w2=(6.6e-7, 1.3e-6), b2=(8.9e-7, 1.1e-6), sdf=(3.3e-7, 7.3e-7), feat=(1.9e-7, 5.3e-7)),
    "out32_F0": dict(hw=(2.2e-7, 2.0e-7), zh=(2.6e-7, 1.7e-7), wz=(2.5e-7, 1.6e-7), w1=(1.4e-6, 1.6e-6), b1=(4.5e-6, 4.4e-6),
                     w2=(4.6e-7, 7.5e-7), b2=(2.9e-7, 2.9e-7), sdf=(2.3e-7, 5.3e-7)),
    "out32_F31": dict(hw=(2.6e-7, 5.6e-7), zh=(2.7e-7, 6.7e-7), wz=(2.7e-7, 2.8e-7), w1=(7.8e-7, 1.8e-6), b1=(6.1e-7, 8.5e-7),
                      w2=(7.3e-7, 1.0e-6), b2=(7.4e-7, 9.7e-7), sdf=(2.5e-7, 6.3e-7), feat=(1.9e-7, 5.4e-7)),
    "abi_out4_F0": dict(hw=(2.2e-7, 2.3e-7), zh=(2.5e-7, 1.8e-7), wz=(2.4e-7, 2.3e-7), w1=(2.5e-6, 2.4e-6), b1=(2.8e-6, 3.8e-6),
                        w2=(1.0e-6, 1.5e-6), b2=(1.5e-6, 1.5e-6)),
    "C64": dict(sdf=(4.7e-7, 1.7e-6), feat=(2.1e-7, 4.6e-7)),
    "C128": dict(sdf=(5.6e-7, 1.5e-6)),
    "C96_one_linear": dict(sdf=(1.7e-7, 4.4e-7), feat=(1.9e-7, 7.3e-7)),
}


def bounds(name, tensors):
    return {t: tuple(10 * v for v in MEASURED[name][t]) for t in tensors}


def n_tiles(H, W, D):
    return -(-H // 4) * -(-W // 4) * -(-D // 2)


def make_inputs(H, W, D, C, n_linear, out_dim, F, seed):
    """Planes randn x 1.2, weights N(0, 0.3), biases N(0, 0.5), random-signed upstream gradients on sdf and on every feature
    channel (padding included).  Three bands of hw rows — runs of the flattened (h, w) index, 1.5 % of it each, starting mid-row —
    move x into each Softplus branch: +25 (identity), -25 (series) and -3 (across the series / log switch)."""
    g = torch.Generator(device=D0).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=D0)
    hw, zh, wz = rn(H * W, C) * 1.2, rn(D * H, C) * 1.2, rn(W * D, C) * 1.2
    n = max(1, round(0.015 * H * W))
    for frac, shift in ((0.15, 25.0), (0.3, -25.0), (0.8, -3.0)):      # clear of the centre, where the control patch sits
        r0 = int(frac * H * W)
        hw[r0:r0 + n] += shift
    lins = [(rn(out_dim if k == n_linear - 1 else C, C) * 0.3, rn(out_dim if k == n_linear - 1 else C) * 0.5)
            for k in range(n_linear)]
    gs = rn(H, W, D)
    gf = rn(H, W, D, F) if F else None
    return (hw, zh, wz), lins, gs, gf


def reference64(planes, lins, size, gs=None, gf=None, slab=16):
    """float64 torch autograd of the field over h-slabs of `slab` rows; the leaves' .grad accumulate across the slabs.
    Returns (out (H, W, D, out_dim), [grads of hw, zh, wz, then weight, bias per Linear] or None, branch shares of x)."""
    H, W, D = size
    C = planes[0].shape[-1]
    dd = torch.float64
    want_grad = gs is not None
    leaves = [t.detach().to(dd).requires_grad_(want_grad) for t in planes]
    lin64 = [tuple(t.detach().to(dd).requires_grad_(want_grad) for t in wb) for wb in lins]
    out_dim = lin64[-1][0].shape[0]
    hw4 = leaves[0].reshape(H, W, 1, C)
    zh4 = leaves[1].reshape(D, H, 1, C).permute(1, 2, 0, 3)
    wz4 = leaves[2].reshape(W, D, 1, C).permute(2, 0, 1, 3)
    out = torch.empty(H, W, D, out_dim, dtype=dd, device=D0)
    n_id = torch.zeros((), dtype=torch.long, device=D0)
    n_ser = torch.zeros((), dtype=torch.long, device=D0)
    with torch.set_grad_enabled(want_grad):
        for h0 in range(0, H, slab):
            h1 = min(H, h0 + slab)
            x = hw4[h0:h1] + zh4[h0:h1] + wz4
            with torch.no_grad():
                n_id += (x > 20).sum()
                n_ser += (x < SERIES_BELOW).sum()
            y = x
            for w, b in lin64:
                y = Fn.linear(Fn.softplus(y), w, b)
            out[h0:h1] = y.detach()
            if want_grad:
                gy = torch.zeros_like(y)
                gy[..., 0] = gs[h0:h1]
                if gf is not None and out_dim > 1:
                    gy[..., 1:] = gf[h0:h1, ..., :out_dim - 1]
                y.backward(gy)
    grads = [t.grad for t in leaves] + [t.grad for wb in lin64 for t in wb] if want_grad else None
    total = H * W * D * C
    n_id, n_ser = n_id.item(), n_ser.item()
    shares = dict(identity=n_id / total, series=n_ser / total, log=(total - n_id - n_ser) / total)
    return out, grads, shares


def kernel_backward(planes, lins, size, F, gs, gf, abi=False):
    """FieldVolumeFunction forward + backward with the upstream gradients (gs, gf); or, abi=True, selfocc_field_volume_bwd
    called directly with g_feat = NULL.  Returns (sdf, feat, the seven gradients)."""
    H, W, D = size
    (w1, b1), (w2, b2) = lins
    if abi:
        out_dim = w2.shape[0]
        g = [torch.zeros_like(t) for t in (*planes, w1, b1, w2, b2)]
        check(lib().selfocc_field_volume_bwd(ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), H, W, D, 96, ptr(w1), ptr(b1),
                                             ptr(w2), out_dim, ptr(gs), None, 0, *(ptr(t) for t in g), current_stream(D0)),
              "selfocc_field_volume_bwd")
        return None, None, g
    dev = [t.detach().clone().requires_grad_(True) for t in (*planes, w1, b1, w2, b2)]
    sdf, feat = FieldVolumeFunction.apply(*dev, size, F)
    torch.autograd.backward([sdf, feat] if F else [sdf], [gs, gf] if F else [gs])
    return sdf.detach(), (feat.detach() if F else None), [t.grad for t in dev]


def err(got, ref):
    """(rel-L2, max |got - ref| / max |ref|) of one tensor."""
    d = got.double() - ref
    return ((d.norm() / ref.norm().clamp_min(1e-300)).item(), (d.abs().max() / ref.abs().max().clamp_min(1e-300)).item())


def sign_of_error(got, ref):
    """sum(got - ref) / sum |got - ref|: near 0 for rounding noise, near +-1 for an error of one sign."""
    d = got.double() - ref
    return (d.sum() / d.abs().sum().clamp_min(1e-300)).item()


def forward_errors(sdf, feat, out, F):
    out_dim = out.shape[-1]
    e = dict(sdf=err(sdf, out[..., 0]))
    if F:
        assert feat.shape[-1] == F
        if out_dim > 1:
            e["feat"] = err(feat[..., :out_dim - 1], out[..., 1:])
        assert torch.all(feat[..., out_dim - 1:] == 0)           # padding channels of the feature volume
    else:
        assert feat is None
    return e


def bf16_equals_f32_rounded_once(planes, lins, size, F, feat32):
    """field_volume with a bfloat16 feature volume == its float32 feature volume rounded once."""
    if not F:
        return
    _, fb = field_volume(*planes, size, nn_linears(lins, planes[0].shape[-1]), F, torch.bfloat16)
    assert fb.dtype == torch.bfloat16
    assert torch.equal(fb, feat32.to(torch.bfloat16))


def log_record(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def nn_linears(lins, C):
    mods = []
    for w, b in lins:
        m = nn.Linear(C, w.shape[0]).to(D0)
        with torch.no_grad():
            m.weight.copy_(w)
            m.bias.copy_(b)
        mods.append(m)
    return mods


@pytest.mark.parametrize("case", SHIPPED + EDGES, ids=lambda c: c.name)
def test_field_backward_vs_float64_at_size(hip, monkeypatch, case):
    """All seven gradients and the forward outputs against float64 autograd; both bound controls; the kernel that ran."""
    t0 = time.time()
    monkeypatch.delenv("SELFOCC_FIELD_BWD_DBG", raising=False)
    H, W, D, out_dim, F = case.H, case.W, case.D, case.out_dim, case.F
    size = (H, W, D)
    tiles = n_tiles(H, W, D)
    assert tiles > BWD_WAVES                                   # some wave walks more than one tile in every case
    if case in SHIPPED:
        assert tiles >= 8 * BWD_WAVES                          # ~54 to ~70 tiles per wave at the shipped sizes
    planes, lins, gs, gf = make_inputs(H, W, D, 96, 2, out_dim, F, seed=H * 7919 + W * 131 + D * 17 + out_dim + F)
    out64, g64, shares = reference64(planes, lins, size, gs, gf)
    for br in ("identity", "series", "log"):
        assert shares[br] > 0.01, shares

    sdf, feat, got = kernel_backward(planes, lins, size, F, gs, gf, case.abi)
    errs = {n: err(a, r) for n, a, r in zip(GRADS, got, g64)}
    err_sign = {n: sign_of_error(a, r) for n, a, r in zip(GRADS, got, g64)}
    if not case.abi:
        errs.update(forward_errors(sdf, feat, out64, F))
    bnd = bounds(case.name, errs)

    # the kernel that ran: only the b3 kernel honours SELFOCC_FIELD_BWD_DBG=1 (no zh / wz plane-gradient atomics)
    monkeypatch.setenv("SELFOCC_FIELD_BWD_DBG", "1")
    _, _, got_dbg = kernel_backward(planes, lins, size, F, gs, gf, case.abi)
    monkeypatch.delenv("SELFOCC_FIELD_BWD_DBG")
    ran = "b3" if (got_dbg[1].abs().max().item() == 0 and got_dbg[2].abs().max().item() == 0) else "f32"
    errs_dbg = {n: err(a, r) for n, a, r in zip(GRADS, got_dbg, g64)}
    del got_dbg

    # reference-side control: the float64 gradients with the upstream gradient of one 4 x 4 x 2 patch zeroed / doubled, vs
    # the kernel's gradients (what a kernel that dropped / repeated that tile would be measured at), in units of the bounds
    hb, wb, db = 4 * (H // 8), 4 * (W // 8), 2 * (D // 4)
    ctl = {}
    for factor in (0.0, 2.0):
        gs2 = gs.clone()
        gs2[hb:hb + 4, wb:wb + 4, db:db + 2] *= factor
        gf2 = None
        if gf is not None:
            gf2 = gf.clone()
            gf2[hb:hb + 4, wb:wb + 4, db:db + 2] *= factor
        _, g64p, _ = reference64(planes, lins, size, gs2, gf2)
        ctl[f"x{factor:g}"] = {n: [e / b if b > 0 else math.inf for e, b in zip(err(a, r), bnd[n])]
                               for n, a, r in zip(GRADS, got, g64p)}
        del g64p

    rec = dict(case=case.name, kernel=ran, size=list(size), out_dim=out_dim, F=F, abi=case.abi, tiles=tiles,
               tiles_per_wave=tiles / min(BWD_WAVES, 4 * -(-tiles // 4)), patch=[hb, wb, db], shares=shares, err=errs,
               bound=bnd, err_sign=err_sign, err_dbg=errs_dbg, control=ctl)
    if not case.abi:
        fv_sdf, fv_feat = field_volume(*planes, size, nn_linears(lins, 96), F)
        rec["field_volume_equals_function_forward"] = bool(torch.equal(fv_sdf, sdf) and (F == 0 or torch.equal(fv_feat, feat)))
    rec["wall_s"] = round(time.time() - t0, 2)
    log_record(rec)

    assert ran == case.kernel, rec
    for n, e in errs.items():
        assert e[0] <= bnd[n][0] and e[1] <= bnd[n][1], (case.name, n, e, bnd[n])
    for n in GRADS:
        if ran == "b3" and n in ("zh", "wz"):
            assert errs_dbg[n][0] >= 10 * bnd[n][0] and errs_dbg[n][1] >= 10 * bnd[n][1], (case.name, n, errs_dbg[n], bnd[n])
        else:
            assert errs_dbg[n][0] <= bnd[n][0] and errs_dbg[n][1] <= bnd[n][1], (case.name, n, errs_dbg[n], bnd[n])
    for k, c in ctl.items():
        for n in GRADS:
            assert min(c[n]) >= 10, (case.name, k, n, c[n])
    if case.abi:
        # g_feat = NULL: the output's feature rows get no gradient at all
        assert torch.all(got[5][1:] == 0) and torch.all(got[6][1:] == 0)
    else:
        assert rec["field_volume_equals_function_forward"]
        bf16_equals_f32_rounded_once(planes, lins, size, F, fv_feat)


@pytest.mark.parametrize("case", FWD_GENERIC, ids=lambda c: c.name)
def test_field_volume_generic_kernel_vs_float64_at_size(hip, case):
    """field_volume_kernel (C = 64 / 128, or one Linear) at ~1 M voxels: its persistent blocks run several tiles per wave."""
    t0 = time.time()
    H, W, D = case.H, case.W, case.D
    size = (H, W, D)
    planes, lins, _, _ = make_inputs(H, W, D, case.C, case.n_linear, case.out_dim, case.F, seed=case.C * 31 + case.n_linear)
    out64, _, shares = reference64(planes, lins, size)
    for br in ("identity", "series", "log"):
        assert shares[br] > 0.01, shares
    sdf, feat = field_volume(*planes, size, nn_linears(lins, case.C), case.F)
    errs = forward_errors(sdf, feat, out64, case.F)
    bnd = bounds(case.name, errs)
    log_record(dict(case=case.name, kernel="field_volume_kernel", size=list(size), C=case.C, n_linear=case.n_linear,
                    out_dim=case.out_dim, F=case.F, fwd_tiles=-(-H * W * D // 32), shares=shares, err=errs, bound=bnd,
                    wall_s=round(time.time() - t0, 2)))
    for n, e in errs.items():
        assert e[0] <= bnd[n][0] and e[1] <= bnd[n][1], (case.name, n, e, bnd[n])
    bf16_equals_f32_rounded_once(planes, lins, size, case.F, feat)
