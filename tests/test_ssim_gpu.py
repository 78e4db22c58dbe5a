"""GPU parity: selfocc_ssim_fwd / _bwd (one launch per direction) vs the torch op chain of the reference's SSIM
(loss/reproj_loss_mono_multi_new_combine.py:26-66) in float64, on inputs addressed through non-trivial strides.

The yardstick of every bound is the same torch chain in float32 on the CPU against float64 on the same inputs, computed
in the test: the kernel may be 4 x as far (floors: 2e-6 forward, 2e-6 of max |grad| backward).  Each check appends its
measured pairs (kernel, float32 chain) to parity_out/loss_kernels_parity.jsonl.

Measured on MI355X (float32 chain in brackets): correlated pairs forward 1.1e-5 (1.1e-5), gradients 7.7e-6 (7.4e-6) of
max |grad|, no window within 1e-5 of a clamp edge; low-contrast bright pair 2.2e-4 (2.2e-4) forward, 2.2e-4 (2.1e-4)
gradients; x ~ y forward 3.9e-6 (3.9e-6).  The kernel is never above 1.5 x the chain.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from selfocc_amd.loss.reproj import SSIM

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "loss_kernels_parity.jsonl")


def ssim_ref(x, y):
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    x, y = F.pad(x, (1, 1, 1, 1), mode='reflect'), F.pad(y, (1, 1, 1, 1), mode='reflect')
    pool = lambda t: F.avg_pool2d(t, 3, 1)
    mu_x, mu_y = pool(x), pool(y)
    sigma_x = pool(x ** 2) - mu_x ** 2
    sigma_y = pool(y ** 2) - mu_y ** 2
    sigma_xy = pool(x * y) - mu_x * mu_y
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


# ---- layouts: the logical (N, C, H, W) tensor as a view of a larger one (the rest holds other values) ----
def lay_contiguous(t):
    return t.to(D0)


def lay_channel_last(t):
    return t.permute(0, 2, 3, 1).contiguous().to(D0).permute(0, 3, 1, 2)


def lay_rows_skipped(t):
    """big[:, :, ::2, 1:-1]: H stride 2 (W + 2), W stride 1, a storage offset"""
    N, C, H, W = t.shape
    big = torch.full((N, C, 2 * H, W + 2), 7.0)
    big[:, :, ::2, 1:-1] = t
    return big.to(D0)[:, :, ::2, 1:-1]


def lay_channel_last_padded(t):
    """channel-last with a wider row: W stride C, H stride (W + 3) C, a storage offset"""
    N, C, H, W = t.shape
    big = torch.full((N, H, W + 3, C), -3.0)
    big[:, :, 2:-1, :] = t.permute(0, 2, 3, 1)
    return big.to(D0)[:, :, 2:-1, :].permute(0, 3, 1, 2)


def lay_cols_skipped(t):
    """big[..., ::2]: W stride 2"""
    N, C, H, W = t.shape
    big = torch.full((N, C, H, 2 * W), 5.0)
    big[..., ::2] = t
    return big.to(D0)[..., ::2]


def _chain(x, y, go, dtype):
    xr, yr = x.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
    out = ssim_ref(xr, yr)
    out.backward(go.to(dtype))
    return out.detach(), xr.grad, yr.grad


def _kernel(xv, yv, go, need_x=True, need_y=True):
    xd, yd = xv.detach().requires_grad_(need_x), yv.detach().requires_grad_(need_y)
    assert xd.stride() == xv.stride() and yd.stride() == yv.stride()
    out = SSIM()(xd, yd)
    out.backward(go.to(D0))
    return out.detach().cpu(), (xd.grad.cpu() if need_x else None), (yd.grad.cpu() if need_y else None)


def _log(m):
    print("\n[ssim vs float64] (kernel, float32 chain)", m)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(m) + "\n")
    except OSError:
        pass


def check_ssim(name, x, y, go, lay_x, lay_y, no_window_dropped=True, grads=True):
    """x, y, go: float32 CPU (N, C, H, W).  Windows whose float64 value lies within 1e-5 of a clamp edge take no part in
    the gradient comparison (their upstream gradient is zeroed for the kernel, the float32 chain and float64 alike): a
    float32 value may fall on the other side of the edge, where the gradient is cut."""
    ref = ssim_ref(x.double(), y.double())
    edge = (ref < 1e-5) | (ref > 1 - 1e-5)
    if no_window_dropped:
        assert not edge.any(), (name, int(edge.sum()))
    go = go.masked_fill(edge, 0.0)
    r_out, r_gx, r_gy = _chain(x, y, go, torch.float64)
    p_out, p_gx, p_gy = _chain(x, y, go, torch.float32)
    xv, yv = lay_x(x), lay_y(y)
    assert torch.equal(xv.cpu(), x) and torch.equal(yv.cpu(), y)
    h_out, h_gx, h_gy = _kernel(xv, yv, go)
    assert h_out.shape == r_out.shape
    m = dict(kernel="ssim", case=name, shape=list(x.shape), x_strides=list(xv.stride()), y_strides=list(yv.stride()),
             windows_dropped=int(edge.sum()),
             fwd=((h_out.double() - r_out).abs().max().item(), (p_out.double() - r_out).abs().max().item()))
    assert torch.isfinite(h_gx).all() and torch.isfinite(h_gy).all()
    if grads:
        for key, hg, pg, rg in (("gx", h_gx, p_gx, r_gx), ("gy", h_gy, p_gy, r_gy)):
            scale = rg.abs().max().item()
            assert scale > 0
            m[key] = ((hg.double() - rg).abs().max().item() / scale, (pg.double() - rg).abs().max().item() / scale)
    _log(m)
    assert m["fwd"][0] <= max(4 * m["fwd"][1], 2e-6), m
    if grads:
        for key in ("gx", "gy"):
            assert m[key][0] <= max(4 * m[key][1], 2e-6), (key, m)
    # only one input needs a gradient (the loss call sites: the target is data; g_x = NULL or g_y = NULL in the kernel):
    # bit-equal to the same side of the two-sided call
    _, gx_only, none_y = _kernel(xv, yv, go, True, False)
    _, none_x, gy_only = _kernel(xv, yv, go, False, True)
    assert none_x is None and none_y is None
    assert torch.equal(gx_only, h_gx) and torch.equal(gy_only, h_gy), name
    return m


def correlated_pair(N, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, C, H, W, generator=g)
    y = (x + 0.3 * torch.randn(N, C, H, W, generator=g)).clamp(0, 1)      # correlated: SSIM inside (0, 1)
    go = torch.randn(N, C, H, W, generator=g) * (torch.rand(N, C, H, W, generator=g) > 0.3)   # ~30 % exact zeros
    return x, y, go


@pytest.mark.parametrize("N,H,W,channel_last", [(1, 48, 100, True), (6, 48, 100, True), (2, 7, 5, False), (1, 2, 2, False),
                                                (1, 3, 3, True)])
def test_ssim_fwd_bwd_vs_float64(hip, N, H, W, channel_last):
    g = torch.Generator().manual_seed(N * 100 + H + W)
    base_x = torch.rand(N, H, W, 3, generator=g)
    base_y = (base_x + 0.3 * torch.randn(N, H, W, 3, generator=g)).clamp(0, 1)   # correlated: SSIM inside (0, 1) mostly
    base_y[0, 0, 0] = 1.0 - base_x[0, 0, 0]                                       # and some clamped windows
    go = torch.randn(N, 3, H, W, generator=g)
    view = (lambda t: t.permute(0, 3, 1, 2)) if channel_last else (lambda t: t.permute(0, 3, 1, 2).contiguous())
    xr, yr = base_x.double().requires_grad_(True), base_y.double().requires_grad_(True)
    ref = ssim_ref(view(xr), view(yr))
    d = torch.device("cuda:0")
    xd, yd = base_x.to(d).requires_grad_(True), base_y.to(d).requires_grad_(True)
    out = SSIM()(view(xd), view(yd))
    assert out.shape == ref.shape
    assert torch.allclose(out.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=2e-5)
    # forward and both gradients under the yardstick rule (windows within 1e-5 of a clamp edge may flip their mask: left out)
    lay = lay_channel_last if channel_last else lay_contiguous
    x, y = base_x.permute(0, 3, 1, 2).contiguous(), base_y.permute(0, 3, 1, 2).contiguous()
    check_ssim(f"base_N{N}_{H}x{W}", x, y, go, lay, lay, no_window_dropped=False)


# x and y always in different layouts, none with H / W strides (W, 1)
SHAPES = [((2, 1, 2, 9), lay_rows_skipped, lay_channel_last_padded),
          ((2, 4, 9, 2), lay_cols_skipped, lay_rows_skipped),
          ((1, 3, 3, 64), lay_channel_last_padded, lay_cols_skipped),
          ((3, 3, 7, 5), lay_rows_skipped, lay_cols_skipped),
          ((6, 3, 48, 100), lay_channel_last_padded, lay_rows_skipped)]


@pytest.mark.parametrize("shape,lay_x,lay_y", SHAPES, ids=["x".join(map(str, s[0])) for s in SHAPES])
def test_ssim_strided_shapes_vs_float64(hip, shape, lay_x, lay_y):
    """C = 1, 3, 4; H = 2 and W = 2 (every row / column is a reflected one); upstream gradient with exact zeros (the
    backward's g == 0 shortcut); both gradients, x only, y only."""
    x, y, go = correlated_pair(*shape, seed=sum(shape))
    assert 0.2 < (go == 0).float().mean() < 0.4 or go.numel() < 64
    check_ssim("strided", x, y, go, lay_x, lay_y, no_window_dropped=True)


@pytest.mark.parametrize("shape,lay_x,lay_y", [SHAPES[3], SHAPES[4]], ids=["3x3x7x5", "6x3x48x100"])
def test_ssim_low_contrast_bright_pair(hip, shape, lay_x, lay_y):
    """0.8 + 0.01 rand: sxx / 9 - mu^2 cancels six digits; the float32 chain loses them too (its own error is the yardstick)"""
    g = torch.Generator().manual_seed(7)
    x, y = 0.8 + 0.01 * torch.rand(*shape, generator=g), 0.8 + 0.01 * torch.rand(*shape, generator=g)
    go = torch.randn(*shape, generator=g)
    check_ssim("low_contrast", x, y, go, lay_x, lay_y, no_window_dropped=False)


def test_ssim_x_close_to_y(hip):
    """every window at the clamp edge (value ~1e-5): the forward under the yardstick rule, the gradients finite"""
    shape, lay_x, lay_y = SHAPES[3]
    g = torch.Generator().manual_seed(11)
    x = torch.rand(*shape, generator=g)
    y = (x + 1e-4 * torch.randn(*shape, generator=g)).clamp(0, 1)
    go = torch.randn(*shape, generator=g)
    ref = ssim_ref(x.double(), y.double())
    assert ref.max() < 1e-3
    p_out = ssim_ref(x, y)
    h_out, h_gx, h_gy = _kernel(lay_x(x), lay_y(y), go)
    m = dict(kernel="ssim", case="x_close_to_y", shape=list(shape),
             fwd=((h_out.double() - ref).abs().max().item(), (p_out.double() - ref).abs().max().item()))
    _log(m)
    assert m["fwd"][0] <= max(4 * m["fwd"][1], 2e-6), m
    assert torch.isfinite(h_gx).all() and torch.isfinite(h_gy).all()
