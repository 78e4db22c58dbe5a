"""GPU parity of the fused reprojection sampling (selfocc_reproj_fwd/_bwd) vs the torch-op port of the reference loss
lines, run in float64 on the float32-rounded inputs (forward + autograd gradient wrt the weights).

The yardstick of every bound is the float32 port on the CPU against that same float64 reference, computed in the test:
the kernel may be 4 x as far (another float32 summation order of the same formula: a wave shuffle tree and fmaf against
index_add), never compared with a constant scaled by the global gradient maximum.  Each case appends its measured pairs
(kernel, float32 port) to parity_out/loss_kernels_parity.jsonl.

The gradient is judged per ray on the ray's own scale, e_r = max_s |g - ref| / max_s |ref|.  A ray's gradient is a
difference, g_s = sc_s (a_s - abar) / wtot, and on some rays it is nothing but the rounding residue of that difference:
a ray with one live sample (all of S = 1) has gradient zero in exact arithmetic (the weights are renormalised), and the
near == far rays put every sample on one pixel, so a_s - abar is ~1e-5 of a_s.  The float32 a_s carry ~1e-5 of relative
error (the forward figures), so a row below ILL = 1e-2 of T_r = max_s sc_s (|a_s| + |abar|) / wtot is >= 1e-3 noise on
its own scale in ANY float32 evaluation, ten times the error of an ordinary ray; measured on the CPU, the float32 port
has e_r 0.1 .. 1e11 on exactly these rays and <= 1.4e-4 on all others (T_r / max_s |ref| is 2.7 in the median, 13 at
the 99th percentile and >= 4e3 on the degenerate rays).  Those ill-conditioned rays are judged apart, on the scale of
the float32 error itself: T'_r, which is T_r with a_s replaced by |g_l1| diff_s + |g_rgb| . comb_s.  On that scale every
ray follows one error law (port: 1e-6 .. 3e-5 on ordinary and degenerate rays alike), so their yardstick is the port's
maximum over every ray of the case, not over the 3 - 15 ill-conditioned ones alone.  Every other ray keeps e_r.  Rows
with T_r == 0 (every sample masked, or no upstream gradient) must be exactly zero.

Measured on MI355X (worst case over the 14 cases of this file; float32 port in brackets): l1 9.2e-6 (9.0e-6),
rgb_combine 3.0e-5 (3.0e-5); e_r 1.35e-4 (1.35e-4), l1 term alone 1.41e-4 (1.41e-4), rgb_combine term alone 1.34e-4 (1.34e-4),
the kernel never above 1.03 x the port in any case; ill-conditioned rays 1.8e-5 of T'_r (port, all rays: 3.1e-5); rays
left out as undecided: 0 - 8 of 301.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import torch_port as tp
from selfocc_amd.reproj import ReprojSampleFunction

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "loss_kernels_parity.jsonl")


def make_case(R=300, S=64, Hi=96, Wi=200, seed=0, with_deltas=False, img_hw=None, outside=0.0, edge=0.0):
    """img_hw: size of the previous / next images when it differs from the (Hi, Wi) the pixels are normalised by.
    outside: share of the rays (one block) whose pixel lies far left of the image: no sample projects into either frame.
    edge: share of the rays (one block) within a few pixels of the left image border, where the two opposite yaws push
    the projection out of one frame and not the other."""
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    f = 0.8 * Wi
    K = np.array([[f, 0, Wi / 2, 0], [0, f, Hi / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    def motion(yaw_deg, tx, tz):
        y = math.radians(yaw_deg)
        Rm = np.array([[math.cos(y), 0, math.sin(y), tx], [0, 1, 0, 0.02], [-math.sin(y), 0, math.cos(y), tz], [0, 0, 0, 1]])
        return torch.tensor(K @ Rm @ np.linalg.inv(K), dtype=torch.float32)
    T_prev, T_next = motion(2.0, 0.3, -0.6), motion(-2.5, -0.2, 0.7)
    ih, iw = (Hi, Wi) if img_hw is None else img_hw
    img_prev, img_next = torch.rand(3, ih, iw, generator=g), torch.rand(3, ih, iw, generator=g)
    pix = torch.stack([torch.rand(R, generator=g) * Wi, torch.rand(R, generator=g) * Hi], -1)
    n_out, n_edge = int(outside * R), int(edge * R)
    if n_out:
        pix[R // 10: R // 10 + n_out, 0] = -Wi * (1.0 + torch.rand(n_out, generator=g))
    if n_edge:
        pix[R // 10 + n_out: R // 10 + n_out + n_edge, 0] = 0.5 + 4.0 * torch.rand(n_edge, generator=g)
    curr_rgb = torch.rand(R, 3, generator=g)
    near = torch.rand(R, 1, generator=g) * 0.5
    far = 2.0 + torch.rand(R, 1, generator=g) * 40.0
    far[: R // 20] = near[: R // 20] + 1e-6        # degenerate rays (near == far)
    edges = near + (far - near) * torch.linspace(0, 1, S + 1)[None]
    ts = ((edges[:, :-1] + edges[:, 1:]) / 2).contiguous()
    deltas = (edges[:, 1:] - edges[:, :-1]).contiguous() if with_deltas else None
    weights = torch.softmax(torch.randn(R, S, generator=g) * 3, -1) * torch.rand(R, 1, generator=g)
    if R >= 5:
        weights[R // 2: R // 2 + 5] = 0.0           # rays with no weight at all
    return weights, ts, deltas, pix, curr_rgb, T_prev, T_next, img_prev, img_next, float(Hi), float(Wi)


def _frame_state(T, pix, ts, img_h, img_w):
    """float64, per sample of one transform: (mask as float64 decides it, undecided).  A mask comparison (p2 > 0,
    0 < px < img_w, 0 < py < img_h) within float32 rounding of its threshold may fall either way: delta_i bounds the
    float32 error of row i of the transform (4e-6 of the sum of the magnitudes of its four terms), e_x / e_y carry it
    through the perspective divide."""
    T = T.double()
    t = ts.double()
    x, y = pix[:, :1].double() * t, pix[:, 1:2].double() * t
    p, dl = [], []
    for i in range(3):
        terms = (T[i, 0] * x, T[i, 1] * y, T[i, 2] * t, T[i, 3].expand_as(t))
        p.append(terms[0] + terms[1] + terms[2] + terms[3])
        dl.append(4e-6 * (terms[0].abs() + terms[1].abs() + terms[2].abs() + terms[3].abs()))
    den = p[2].clamp_min(1e-5)
    px, py = p[0] / den, p[1] / den
    ex = (dl[0] + px.abs() * dl[2]) / den + 4e-6 * px.abs()
    ey = (dl[1] + py.abs() * dl[2]) / den + 4e-6 * py.abs()
    und = (p[2].abs() <= dl[2]) | (px.abs() <= ex) | ((px - img_w).abs() <= ex) | (py.abs() <= ey) | ((py - img_h).abs() <= ey)
    und &= ~(p[2] < -dl[2])
    mask = (p[2] > 0) & (px > 0) & (px < img_w) & (py > 0) & (py < img_h)
    return mask, und


def _kept_rays(case):
    """rays without an undecided sample under either transform, and the two float64 masks"""
    _, ts, _, pix, _, T_prev, T_next, _, _, img_h, img_w = case
    mp, up = _frame_state(T_prev, pix, ts, img_h, img_w)
    mn, un = _frame_state(T_next, pix, ts, img_h, img_w)
    return ~(up | un).any(dim=1), mp, mn


def _port_run(case, dtype, g1, g2):
    """the port in ``dtype``: l1, rgb_combine, any_valid and the gradients wrt the weights of the l1 term alone
    (upstream g1) and of the rgb_combine term alone (g2); their sum is the gradient of both."""
    c = [t.to(dtype) if torch.is_tensor(t) else t for t in case]
    w = c[0].clone().requires_grad_(True)
    l1, comb, anyv = tp.reproj_sample_port(w, *c[1:])
    ga, = torch.autograd.grad((l1 * g1.to(dtype)).sum(), w, retain_graph=True)
    gb, = torch.autograd.grad((comb * g2.to(dtype)).sum(), w)
    return l1.detach(), comb.detach(), anyv, ga, gb


def _term_scale(case, g1, g2):
    """The gradient of a ray is a difference: g_s = sc_s (a_s - abar) / wtot with a_s = g_l1 diff_s + g_rgb . comb_s,
    abar its weighted mean, sc_s the sample's 1 / delta (0 when masked) and wtot the clamped weight sum.  Returns, per
    term selection (both, l1 alone, rgb_combine alone), that formula in float64, T_r = max_s sc_s (|a_s| + |abar|) /
    wtot, the size of the two terms whose difference the row is, and T'_r, the same with a_s replaced by
    |g_l1| diff_s + |g_rgb| . comb_s (no cancellation left inside a_s either: the scale of the row's float32 error).  a_s comes from the port itself, called with every
    sample as a ray of its own (one sample of weight 1: l1 = diff_s, rgb_combine = comb_s, any_valid = its mask)."""
    w, ts, deltas, pix, cur = [None if t is None else t.double() for t in case[:5]]
    R, S = w.shape
    rest = [t.double() if torch.is_tensor(t) else t for t in case[5:]]
    d_s, c_s, any_s = tp.reproj_sample_port(torch.ones(R * S, 1, dtype=torch.float64), ts.reshape(-1, 1), None,
                                            pix.repeat_interleave(S, 0), cur.repeat_interleave(S, 0), *rest)
    sc = any_s.reshape(R, S)
    if deltas is not None:
        sc = sc * torch.where(deltas < tp.EPS32, torch.zeros_like(deltas), 1.0 / deltas.clamp_min(tp.EPS32))
    weff = w * sc
    wraw = weff.sum(dim=1)
    wtot = wraw.clamp_min(tp.EPS32)
    a1 = g1.double()[:, None] * d_s.reshape(R, S)
    a2 = (g2.double()[:, None, :] * c_s.reshape(R, S, 3)).sum(dim=-1)
    m1 = g1.double().abs()[:, None] * d_s.reshape(R, S)
    m2 = (g2.double().abs()[:, None, :] * c_s.reshape(R, S, 3)).sum(dim=-1)
    out = []
    for a, mag in ((a1 + a2, m1 + m2), (a1, m1), (a2, m2)):
        live = wraw > tp.EPS32          # below the clamp the denominator is a constant: no abar term
        abar = torch.where(live, (weff * a).sum(dim=1) / wtot, torch.zeros_like(wtot))
        mbar = torch.where(live, (weff * mag).sum(dim=1) / wtot, torch.zeros_like(wtot))
        out.append((sc * (a - abar[:, None]) / wtot[:, None], (sc * (a.abs() + abar.abs()[:, None])).amax(dim=1) / wtot,
                    (sc * (mag + mbar[:, None])).amax(dim=1) / wtot))
    return out


ILL = 1e-2     # a row smaller than this share of T_r is an ill-conditioned difference (module docstring)


def _ray_err(g, ref, keep, T, Tm):
    """Per kept ray -> (worst e_r = max_s |g - ref| / max_s |ref| over the well-conditioned rays,
    worst max_s |g - ref| / T'_r over the ill-conditioned ones (max_s |ref| < ILL * T_r), the same over every live ray,
    the kept rays with T_r == 0: every sample masked or without upstream gradient, zero by construction)"""
    g, ref = g.double(), ref.double()
    top, err = ref.abs().amax(dim=1), (g - ref).abs().amax(dim=1)
    live = keep & (T > 0)
    well, ill = live & (top >= ILL * T), live & (top < ILL * T)
    worst = lambda e: e.max().item() if e.numel() else 0.0
    return worst(err[well] / top[well]), worst(err[ill] / Tm[ill]), worst(err[live] / Tm[live]), keep & (T == 0)


def _kernel(case, g1=None, g2=None):
    dev = [None if t is None else (t.to(D0) if torch.is_tensor(t) else t) for t in case]
    wd = dev[0].clone().requires_grad_(True)
    l1, comb, anyv = ReprojSampleFunction.apply(wd, *dev[1:])
    grad = None
    if g1 is not None:
        grad, = torch.autograd.grad((l1 * g1.to(D0)).sum() + (comb * g2.to(D0)).sum(), wd)
        grad = grad.cpu()
    return l1.detach().cpu(), comb.detach().cpu(), anyv.cpu(), grad


def check_case(name, case, max_dropped=0.03):
    """forward, backward (both terms, l1 alone, rgb_combine alone) and run-to-run identity of one case against float64;
    returns the float64 masks for the caller's own asserts"""
    R, S = case[0].shape
    g = torch.Generator().manual_seed(1)
    g1, g2 = torch.randn(R, generator=g), torch.randn(R, 3, generator=g)
    keep, mp, mn = _kept_rays(case)
    assert (~keep).float().mean().item() <= max_dropped, f"{name}: {(~keep).sum().item()} of {R} rays undecided"
    r_l1, r_comb, r_any, r_ga, r_gb = _port_run(case, torch.float64, g1, g2)
    p_l1, p_comb, p_any, p_ga, p_gb = _port_run(case, torch.float32, g1, g2)
    h_l1, h_comb, h_any, h_g = _kernel(case, g1, g2)
    zero1, zero3 = torch.zeros_like(g1), torch.zeros_like(g2)
    h_ga, h_gb = _kernel(case, g1, zero3)[3], _kernel(case, zero1, g2)[3]
    again = _kernel(case, g1, g2)
    for a, b in zip((h_l1, h_comb, h_any, h_g), again):
        assert torch.equal(a, b), f"{name}: two identical calls differ"

    assert torch.equal(h_any[keep].double(), r_any[keep]), name
    assert torch.equal(r_any.bool(), (mp | mn).any(dim=1)), name      # the rule's float64 masks are the port's
    m = dict(case=name, R=R, S=S, deltas=case[2] is not None, img=list(case[7].shape[1:]), dropped=int((~keep).sum()),
             l1=((h_l1.double() - r_l1).abs()[keep].max().item(), (p_l1.double() - r_l1).abs()[keep].max().item()),
             rgb_combine=((h_comb.double() - r_comb).abs()[keep].max().item(),
                          (p_comb.double() - r_comb).abs()[keep].max().item()))
    zero_rows = {}
    scales = _term_scale(case, g1, g2)
    for (key, hg, pg, rg), (formula, T, Tm) in zip((("grad", h_g, p_ga + p_gb, r_ga + r_gb), ("grad_l1_only", h_ga, p_ga, r_ga),
                                                ("grad_rgb_only", h_gb, p_gb, r_gb)), scales):
        # the float64 autograd gradient is the formula T_r is taken from, to float64 rounding
        assert ((formula - rg).abs().amax(dim=1) <= 1e-9 * T).all(), (name, key)
        eh, eh_ill, _, zr = _ray_err(hg, rg, keep, T, Tm)
        ep, _, ep_all, _ = _ray_err(pg, rg, keep, T, Tm)
        m[key], m[key + "_ill"] = (eh, ep), (eh_ill, ep_all)
        zero_rows[key] = (hg, zr)
        assert rg[zr].abs().max().item() == 0 if zr.any() else True
    m["ill_conditioned_rays"] = int((keep & (scales[0][1] > 0) & ((r_ga + r_gb).abs().amax(dim=1) < ILL * scales[0][1])).sum())
    print("\n[reproj vs float64] (kernel, float32 port)", m)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(m) + "\n")
    except OSError:
        pass
    for key in ("l1", "rgb_combine"):
        assert m[key][0] <= max(4 * m[key][1], 1e-6), (key, m)
    for key in ("grad", "grad_l1_only", "grad_rgb_only"):
        hg, zr = zero_rows[key]
        assert hg[zr].abs().max().item() == 0 if zr.any() else True, (key, m)   # zero by construction: exactly zero
        assert m[key][0] <= max(4 * m[key][1], 1e-5), (key, m)
        assert m[key + "_ill"][0] <= max(4 * m[key + "_ill"][1], 1e-5), (key, m)
    assert torch.isfinite(h_g).all()
    return mp, mn, r_any, keep


@pytest.mark.parametrize("S,with_deltas", [(64, False), (32, True), (256, False), (100, True)])
def test_reproj_fwd_bwd_vs_port(hip, S, with_deltas):
    case = make_case(S=S, seed=S, with_deltas=with_deltas)
    w = case[0].clone().requires_grad_(True)
    l1, comb, anyv = tp.reproj_sample_port(w, *case[1:])

    dev = [None if t is None else (t.to(D0) if torch.is_tensor(t) else t) for t in case]
    hl1, hcomb, hany = ReprojSampleFunction.apply(*dev)
    assert torch.equal(hany.cpu(), anyv)
    assert torch.allclose(hl1.cpu(), l1.detach(), rtol=1e-4, atol=1e-6)
    assert torch.allclose(hcomb.cpu(), comb.detach(), rtol=1e-4, atol=1e-6)
    assert 0.2 < anyv.mean() <= 1.0
    # values and the per-ray gradient against float64, on each ray's own scale
    check_case(f"S{S}", case)


# S: M = 1 (1, 63), 2 (65), 4 with a quarter of the wave dead (129, 192), 8 (257, 300, 512); deltas on every second one;
# R = 301 leaves one ray in the last block of 4; three cases sample 50 x 77 images through pixels normalised by 96 x 200
CASES = [
    ("S1", dict(R=301, S=1)),
    ("S63_d_img", dict(R=301, S=63, with_deltas=True, img_hw=(50, 77))),
    ("S65_next_behind", dict(R=301, S=65)),
    ("S129_d_outside", dict(R=301, S=129, with_deltas=True, outside=0.3, edge=0.25)),
    ("S192_img", dict(R=301, S=192, img_hw=(50, 77))),
    ("S257_d_img", dict(R=301, S=257, with_deltas=True, img_hw=(50, 77))),
    ("S300", dict(R=301, S=300)),
    ("S512_d", dict(R=301, S=512, with_deltas=True)),
    ("R1_S64", dict(R=1, S=64)),
    ("R5_S100_d", dict(R=5, S=100, with_deltas=True)),
]


def build_case(name, kw):
    case = list(make_case(seed=1000 + kw["S"], **kw))
    if name == "S65_next_behind":
        # what ReprojLossMonoMultiNew passes for a missing frame: every sample has at most one valid frame
        case[6] = torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0]))
    return tuple(case)


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_reproj_vs_float64(hip, name, kw):
    case = build_case(name, kw)
    mp, mn, r_any, keep = check_case(name, case)
    one = (mp ^ mn).double().mean().item()
    if name == "S65_next_behind":
        assert not mn.any() and mp.any()
    if name == "S129_d_outside":
        dead = 1.0 - r_any.mean().item()
        assert 0.05 <= dead <= 0.60, dead         # the block of rays outside both images is there, and is not everything
        assert one >= 0.10, one                   # samples with exactly one valid frame


def test_reproj_all_invalid_and_empty(hip):
    case = list(make_case(R=40, S=16))
    case[5] = torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0]))      # projects behind both cameras
    case[6] = torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0]))
    dev = [None if t is None else (t.to(D0) if torch.is_tensor(t) else t) for t in case]
    l1, comb, anyv = ReprojSampleFunction.apply(*dev)
    assert anyv.sum() == 0 and l1.abs().max() == 0 and comb.abs().max() == 0
    empty = [None if t is None else (t[:0].to(D0) if (torch.is_tensor(t) and t.shape[0] == 40) else (t.to(D0) if torch.is_tensor(t) else t)) for t in case]
    l1, comb, anyv = ReprojSampleFunction.apply(*empty)
    assert l1.numel() == 0
