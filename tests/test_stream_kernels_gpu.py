"""GPU: the small streaming kernels of every training iteration, at the caps, tails and launch branches no other test reaches.

selfocc_flatten_feats (csrc/geometry.hip)
    dynamic LDS is C * 65 * 4 bytes; from C = 190 it exceeds the 48 KiB a launch gets without asking, and the launcher raises the
    kernel's limit first.  C = 189 / 190 straddle that branch, 192 / 256 (the usual TPVFormer width) / 512 (the widest the entry
    accepts: 133 120 bytes of the CU's 160 KiB) run it.  The maps have 1, 63, 64 and 65 pixels: a one-pixel tile, a ragged tile,
    a full tile and a full tile followed by one pixel.
selfocc_eikonal_fwd / _bwd (csrc/losses.hip)
    the grid is capped at 2048 blocks of 256 threads x 4 rows = 2 097 152 rows.  2 097 152 is the largest uncapped launch,
    2 097 153 the first capped one (one thread walks a fifth row), 7 372 800 the shipped size (14 - 15 rows per thread, 2048
    float32 partials added on the Python side).  The reference is the formula in float64.
selfocc_point_sampling (csrc/geometry.hip)
    points ON the decision boundaries: depth at eps = 1e-5 and its float32 neighbours, image coordinates exactly 0, -0, 1, the
    float32 below 1 and the smallest positive float32, with matrices that keep the projection exact."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")


# ---- flatten_feats -------------------------------------------------------------------------------------------------------

MAPS = [(1, 1), (7, 9), (8, 8), (5, 13)]            # 1, 63, 64, 65 pixels


def _feats(B, N, C, shapes, seed, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, C, h, w, generator=g).to(D0).requires_grad_(requires_grad) for h, w in shapes]


def _embeds(N, L, C, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(N, C, generator=g).to(D0), torch.randn(L, C, generator=g).to(D0)


@pytest.mark.parametrize("C", [1, 3, 189, 190, 192, 256, 512])
def test_flatten_feats_every_lds_size_is_the_torch_formula_bit_for_bit(hip, C):
    from selfocc_amd.model.encoder import tpvformer as T
    B, N = 2, 3
    feats = _feats(B, N, C, MAPS, C)
    cams, lvls = _embeds(N, len(MAPS), C, C)
    with torch.no_grad():
        got = T._flatten_feats(cams, lvls, feats)
        want = T._flatten_feats_torch(cams, lvls, feats)
        torch.cuda.synchronize()
    assert got.shape == want.shape == (N, 1 + 63 + 64 + 65, B, C)
    assert got.is_contiguous() and torch.equal(got, want)


def test_flatten_feats_wide_entry_launches_directly(hip):
    """the C entry itself at the widest width it accepts, and its named refusal one past it: no width is accepted and then fails"""
    import ctypes as C
    from selfocc_amd._lib import lib, ptr, current_stream
    from selfocc_amd.model.encoder import tpvformer as T

    def call(width):
        feats = _feats(1, 1, width, [(5, 13)], 7)
        cams, lvls = _embeds(1, 1, width, 7)
        out = torch.full((1, 65, 1, width), float('nan'), device=D0)
        rc = lib().selfocc_flatten_feats((C.c_void_p * 1)(feats[0].data_ptr()), (C.c_int32 * 1)(65), 1, 1, 1, width, ptr(cams),
                                         ptr(lvls), ptr(out), current_stream(D0))
        torch.cuda.synchronize()
        return rc, out, T._flatten_feats_torch(cams, lvls, feats)
    rc, out, want = call(512)
    assert rc == 0 and torch.equal(out, want)
    rc, out, _ = call(513)
    assert rc != 0 and b"bad sizes" in lib().selfocc_last_error() and torch.isnan(out).all()
    # past the entry's limit _flatten_feats is the torch formula
    feats = _feats(1, 2, 513, [(3, 3)], 9)
    cams, lvls = _embeds(2, 1, 513, 9)
    assert torch.equal(T._flatten_feats(cams, lvls, feats), T._flatten_feats_torch(cams, lvls, feats))


def test_flatten_feats_eight_levels_wide(hip):
    from selfocc_amd.model.encoder import tpvformer as T
    B, N, C = 2, 3, 256
    shapes = MAPS + MAPS[::-1]
    feats = _feats(B, N, C, shapes, 8)
    cams, lvls = _embeds(N, 9, C, 8)
    with torch.no_grad():
        got, want = T._flatten_feats(cams, lvls, feats), T._flatten_feats_torch(cams, lvls, feats)
    assert got.shape == (N, 2 * 193, B, C) and torch.equal(got, want)


def test_flatten_feats_backward_at_256_channels(hip):
    from selfocc_amd.model.encoder import tpvformer as T
    B, N, C = 2, 3, 256
    cams, lvls = _embeds(N, len(MAPS) + 1, C, 2)             # one level more than maps: its gradient row stays zero
    cams.requires_grad_(True); lvls.requires_grad_(True)
    fa, fb = _feats(B, N, C, MAPS, 2, True), _feats(B, N, C, MAPS, 2, True)
    ya = T._FlattenFeats.apply(cams, lvls, *fa)
    g = torch.randn(ya.shape, generator=torch.Generator().manual_seed(3)).to(D0)
    ga = torch.autograd.grad(ya, [cams, lvls] + fa, g)
    yb = T._flatten_feats_torch(cams, lvls, fb)
    gb = torch.autograd.grad(yb, [cams, lvls] + fb, g)
    assert torch.equal(ya, yb)
    for a, b in zip(ga, gb):
        assert a.shape == b.shape
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * b.abs().max().item())
    assert torch.all(ga[1][len(MAPS)] == 0)


# ---- eikonal -------------------------------------------------------------------------------------------------------------

EIK_CAP = 2048 * 256 * 4
# Relative error of the loss value against float64 on these inputs, measured on an MI355X (the test prints them); half a
# float32 ulp of the value 0.306 is 4.9e-8, so both are the correctly rounded float32 or its neighbour:
#   n            HIP (float32 partials)    torch's float32 formula
#   2 097 152    8.5e-9                    1.06e-7
#   2 097 153    3.7e-8                    3.7e-8
#   7 372 800    1.5e-8                    1.5e-8
# The bound stays at 2e-6 with float32 partials; the worst gradient element used 0.75 of its bound.
EIK_ROWS = [EIK_CAP, EIK_CAP + 1, 7372800]
ZERO_ROWS = [0, 255, 256, 1000003]                   # all-zero rows: no direction, zero gradient
TINY_ROWS = [1, 257, 1000004, -1]                    # magnitude 1e-25: the float32 squared norm underflows to 0
SUBNORMAL_ROW = 77                                   # magnitude 1e-20: the float32 squared norm is subnormal


@pytest.mark.parametrize("n", EIK_ROWS)
def test_eikonal_vs_float64_past_the_block_cap(hip, n):
    """value: rtol 2e-6 against the float64 formula; gradient: rtol 1e-5, atol 1e-7 / n per element against float64 autograd.
    A row of magnitude 1e-25 has a direction like any other (gradient -2 scale g / ||g||); only an all-zero row has none."""
    from selfocc_amd.loss.simple import EikonalLoss
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 3, generator=g) * 0.7 + 0.3
    x[ZERO_ROWS] = 0.0
    x[TINY_ROWS] = torch.tensor([[1e-25, -1e-25, 1e-25], [1e-25, 0.0, 0.0], [-3e-25, 1e-25, 2e-25], [0.0, 0.0, -1e-25]])
    x[SUBNORMAL_ROW] = torch.tensor([1e-20, 2e-20, -1e-20])
    x = x.to(D0)
    assert torch.all((x[TINY_ROWS] ** 2).sum(-1) == 0) and torch.all(x[TINY_ROWS].abs().sum(-1) > 0)
    a = x.clone().requires_grad_(True)
    eik = EikonalLoss()
    la = eik.eikonal(a)
    (la * 0.37).backward()
    b = x.double().requires_grad_(True)
    lb = ((b.norm(2, dim=-1) - 1) ** 2).mean()
    (lb * 0.37).backward()
    lt = ((x.norm(2, dim=-1) - 1) ** 2).mean()
    err_hip = abs(la.double().item() - lb.item()) / abs(lb.item())
    err_torch = abs(lt.double().item() - lb.item()) / abs(lb.item())
    gerr = (a.grad.double() - b.grad).abs()
    gbound = 1e-7 / n + 1e-5 * b.grad.abs()
    print(f"eikonal n {n}: value {lb.item():.12g}; relative error HIP {err_hip:.3e}, torch float32 {err_torch:.3e}; "
          f"gradient: worst error / bound {(gerr / gbound).max().item():.3f}")
    assert la.dtype == torch.float32 and err_hip <= 2e-6
    assert torch.all(gerr <= gbound), f"{int((gerr > gbound).sum())} elements, first rows {torch.nonzero(gerr > gbound)[:8, 0].tolist()}"
    assert torch.all(a.grad[ZERO_ROWS] == 0)
    assert torch.all(a.grad[TINY_ROWS].abs().sum(-1) > 0.3 / n)           # unit direction x 2 x 0.37 / n
    with torch.no_grad():
        assert torch.equal(eik.eikonal(x), eik.eikonal(x)) and torch.equal(eik.eikonal(x), la.detach())
    a2 = x.clone().requires_grad_(True)
    (eik.eikonal(a2) * 0.37).backward()
    assert torch.equal(a2.grad.view(torch.int32), a.grad.view(torch.int32))


# ---- point_sampling ------------------------------------------------------------------------------------------------------

def _boundary_points():
    """(B = 2, D = 3, Q, 3) reference points whose projections sit on the kernel's decisions, and their metas"""
    f = np.float32
    eps = f(1e-5)
    zs = [eps, np.nextafter(eps, f(0)), np.nextafter(eps, f(1)), f(0), f(-1), f(1)]
    below_one = f(1) - f(2.0 ** -24)
    # u = x / z / 8 and v = y / z / 4: 0, -0, 1, the float32 below 1, the smallest subnormal (quotient rounds to 0), 0.5,
    # and the ratio whose image coordinate is the smallest positive float32
    xr = [f(0), f(-0.0), f(8), f(8) * below_one, f(2.0 ** -149), f(4), f(2.0 ** -146)]
    yr = [f(0), f(-0.0), f(4), f(4) * below_one, f(2.0 ** -149), f(2), f(2.0 ** -147)]
    pts = [(a * z, b * z, z) for z, a, b in itertools.product(zs, xr, yr)]
    D = 3
    inside = (f(4), f(2), f(1))
    while len(pts) % D or len(pts) % 256 == 0:
        pts.append(inside)
    p = torch.tensor(np.asarray(pts, dtype=np.float32))                     # (n, 3)
    assert p.shape[0] == 294 and p.shape[0] % 256 != 0
    Q = p.shape[0] // D
    ref = torch.stack([p.view(Q, D, 3).permute(1, 0, 2), p.flip(0).view(Q, D, 3).permute(1, 0, 2)])     # (2, D, Q, 3)
    l2i = np.stack([np.eye(4, dtype=np.float32), np.diag(np.asarray([2, 2, 1, 1], dtype=np.float32))])  # identity; pure scale
    return ref.contiguous(), l2i


@pytest.mark.parametrize("focal", [False, True])
def test_point_sampling_on_the_decision_boundaries(hip, focal):
    from selfocc_amd.model.encoder.utils import point_sampling
    ref, l2i = _boundary_points()
    meta = {'lidar2img': l2i, 'img_shape': (4, 8)}
    if focal:
        meta.update(focal_ratios_x=[1.5, 0.75], focal_ratios_y=[0.5, 1.25])
    metas = [dict(meta), dict(meta)]
    c_cpu, m_cpu = point_sampling(ref.clone(), metas)
    assert c_cpu.shape == (2, 2, 98, 3, 2) and m_cpu.shape == (2, 2, 98, 3) and m_cpu.dtype == torch.bool
    # the boundary set decides both ways, for each camera: it can tell > from >= and < from <=
    for n in range(2):
        assert m_cpu[n].any() and not m_cpu[n].all()
    flat_pts = ref[0].permute(1, 0, 2).reshape(-1, 3)
    flat_m = m_cpu[0, 0].reshape(-1)
    at_eps = flat_pts[:, 2] == np.float32(1e-5)
    above_eps = flat_pts[:, 2] == np.nextafter(np.float32(1e-5), np.float32(1))
    assert not flat_m[at_eps].any() and flat_m[above_eps].any()            # c2 > eps is strict
    c_gpu, m_gpu = point_sampling(ref.to(D0), metas)
    torch.cuda.synchronize()
    assert c_gpu.is_cuda and c_gpu.shape == c_cpu.shape and m_gpu.dtype == torch.bool
    assert torch.equal(m_gpu.cpu(), m_cpu)
    bad = torch.nonzero((c_gpu.cpu() != c_cpu).flatten(0, -2).any(-1)).flatten()[:6].tolist()
    assert torch.equal(c_gpu.cpu(), c_cpu), f"cam differs at flat (n, b, q, d) indices {bad}"
    assert torch.equal(m_gpu._so_visible.cpu(), m_cpu.any(-1))
