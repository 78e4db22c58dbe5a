"""GPU: the reprojection sampling on channel-last images of any channel count (selfocc_reproj_c_fwd / _bwd: csrc/reproj.hip's one
kernel with its channel-last tap fetch) and the ``dims`` knob of the two reprojection losses.

1. The kernel against float64, by the rule of tests/test_reproj_gpu.py (its module docstring states it in full): the
   reference is the torch-op port of the reference lines in float64 on the float32-rounded inputs (tests/reproj_dims_port.py:
   oracle.torch_port.reproj_sample_port is fixed at 3 channels), the yardstick of every bound is the float32 port on the CPU
   against that reference, computed here, and the kernel may be 4 x as far.  Gradients are judged per ray on the ray's own
   scale, ill-conditioned rows on T'_r; rays with a mask comparison inside float32 rounding are left out, at most 5 % of them.
   The geometry is that file's ``make_case``; only the images and the current values are drawn anew with C channels.
   Measured pairs (kernel, float32 port) go to parity_out/reproj_dims_parity.jsonl.
2. ``wnorm`` / ``any_valid`` bit for bit those of selfocc_reproj_fwd on the same geometry.
3. C = 3 through the channel-last entries against the planar entries: one kernel body with two tap fetches, so l1, combine
   and any_valid agree in every bit and the gradient in every value, at every samples-per-lane instance.
4. Pad channels filled with NaN change no bit of any output.
5. Two runs of one launch are bit-identical (inside every case of 1).
6. The one Python body of ReprojSampleFunction / ReprojSampleCFunction: a planar call equals the raw C entry, and a wrong
   shape is a ValueError before any launch.
7. The loss classes against tests/golden/reproj_dims.npz (the reference's own classes with dims = 1, 5, 16), with the bounds of
   test_golden_gpu.py::test_reproj_losses_vs_reference_class.
8. One dims = 16 forward + backward of each class under torch.cuda.set_sync_debug_mode("error").

Measured on MI355X (worst case over the nine cases of 1 and the two of 3; float32 port in brackets; profiles/
reproj_dims_parity.jsonl): l1 1.21e-5 (1.20e-5), combine 1.56e-5 (1.56e-5); e_r 2.63e-4 (2.64e-4), l1 term alone 1.35e-4
(1.37e-4), combine term alone 2.68e-4 (2.69e-4), the kernel never above 1.21 x the port on a figure above its floor;
ill-conditioned rays 3.2e-6 of T'_r (port, all rays: 1.4e-5); rays left out as undecided: 0 - 11 of 301.  On the four 3-channel
cases of 3 the channel-last entry equals the planar one in every bit.
"""
import json
import os

import numpy as np
import pytest
import torch

import reproj_dims_port as port
from test_reproj_gpu import ILL, _kept_rays, _ray_err, make_case
from selfocc_amd import abi
from selfocc_amd._lib import check, current_stream, ptr
from selfocc_amd.reproj import ChannelLastImage, ReprojSampleCFunction, ReprojSampleFunction

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "parity_out", "reproj_dims_parity.jsonl")
G = os.path.join(ROOT, "tests", "golden")
INVALID = torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0]))       # maps every point behind the camera


def make_case_c(C, seed, **kw):
    """make_case's geometry and weights; curr (R, C) and the two images (C, ih, iw) drawn with C channels"""
    case = list(make_case(seed=seed, **kw))
    g = torch.Generator().manual_seed(seed + 7)
    R = case[0].shape[0]
    ih, iw = case[7].shape[1:]
    case[4] = torch.rand(R, C, generator=g)
    case[7], case[8] = torch.rand(C, ih, iw, generator=g), torch.rand(C, ih, iw, generator=g)
    return case


def to_dev(case):
    return [None if t is None else (t.to(D0) if torch.is_tensor(t) else t) for t in case]


def _port_run(case, dtype, g1, g2):
    c = [t.to(dtype) if torch.is_tensor(t) else t for t in case]
    w = c[0].clone().requires_grad_(True)
    l1, comb, anyv = port.reproj_sample_port_c(w, *c[1:])
    ga, = torch.autograd.grad((l1 * g1.to(dtype)).sum(), w, retain_graph=True)
    gb, = torch.autograd.grad((comb * g2.to(dtype)).sum(), w)
    return l1.detach(), comb.detach(), anyv, ga, gb


def _term_scale(case, g1, g2):
    """test_reproj_gpu._term_scale at C channels: per term selection (both, l1 alone, combine alone) the float64 formula
    g_s = sc_s (a_s - abar) / wtot, T_r and T'_r"""
    w, ts, deltas, pix, cur = [None if t is None else t.double() for t in case[:5]]
    R, S = w.shape
    C = cur.shape[1]
    rest = [t.double() if torch.is_tensor(t) else t for t in case[5:]]
    d_s, c_s, any_s = port.reproj_sample_port_c(torch.ones(R * S, 1, dtype=torch.float64), ts.reshape(-1, 1), None,
                                                pix.repeat_interleave(S, 0), cur.repeat_interleave(S, 0), *rest)
    sc = any_s.reshape(R, S)
    if deltas is not None:
        sc = sc * torch.where(deltas < port.EPS32, torch.zeros_like(deltas), 1.0 / deltas.clamp_min(port.EPS32))
    weff = w * sc
    wraw = weff.sum(dim=1)
    wtot = wraw.clamp_min(port.EPS32)
    a1 = g1.double()[:, None] * d_s.reshape(R, S)
    a2 = (g2.double()[:, None, :] * c_s.reshape(R, S, C)).sum(dim=-1)
    m1 = g1.double().abs()[:, None] * d_s.reshape(R, S)
    m2 = (g2.double().abs()[:, None, :] * c_s.reshape(R, S, C)).sum(dim=-1)
    out = []
    for a, mag in ((a1 + a2, m1 + m2), (a1, m1), (a2, m2)):
        live = wraw > port.EPS32
        abar = torch.where(live, (weff * a).sum(dim=1) / wtot, torch.zeros_like(wtot))
        mbar = torch.where(live, (weff * mag).sum(dim=1) / wtot, torch.zeros_like(wtot))
        out.append((sc * (a - abar[:, None]) / wtot[:, None], (sc * (a.abs() + abar.abs()[:, None])).amax(dim=1) / wtot,
                    (sc * (mag + mbar[:, None])).amax(dim=1) / wtot))
    return out


def _kernel(case, g1=None, g2=None, fn=ReprojSampleCFunction):
    dev = to_dev(case)
    wd = dev[0].clone().requires_grad_(True)
    l1, comb, anyv = fn.apply(wd, *dev[1:])
    grad = None
    if g1 is not None:
        grad, = torch.autograd.grad((l1 * g1.to(D0)).sum() + (comb * g2.to(D0)).sum(), wd)
        grad = grad.cpu()
    return l1.detach().cpu(), comb.detach().cpu(), anyv.cpu(), grad


def check_case(name, case, max_dropped=0.05):
    """test_reproj_gpu.check_case for the channel-generic entry; returns what the C = 3 comparison needs as well"""
    R, S = case[0].shape
    C = case[4].shape[1]
    g = torch.Generator().manual_seed(1)
    g1, g2 = torch.randn(R, generator=g), torch.randn(R, C, generator=g)
    keep, mp, mn = _kept_rays(case)
    assert (~keep).float().mean().item() <= max_dropped, f"{name}: {(~keep).sum().item()} of {R} rays undecided"
    r_l1, r_comb, r_any, r_ga, r_gb = _port_run(case, torch.float64, g1, g2)
    p_l1, p_comb, p_any, p_ga, p_gb = _port_run(case, torch.float32, g1, g2)
    h_l1, h_comb, h_any, h_g = _kernel(case, g1, g2)
    zero1, zeroc = torch.zeros_like(g1), torch.zeros_like(g2)
    h_ga, h_gb = _kernel(case, g1, zeroc)[3], _kernel(case, zero1, g2)[3]
    again = _kernel(case, g1, g2)
    for a, b in zip((h_l1, h_comb, h_any, h_g), again):
        assert torch.equal(a, b), f"{name}: two identical calls differ"

    assert torch.equal(h_any[keep].double(), r_any[keep]), name
    assert torch.equal(r_any.bool(), (mp | mn).any(dim=1)), name      # the rule's float64 masks are the port's
    m = dict(case=name, R=R, S=S, C=C, deltas=case[2] is not None, img=list(case[7].shape[1:]), dropped=int((~keep).sum()),
             l1=((h_l1.double() - r_l1).abs()[keep].max().item(), (p_l1.double() - r_l1).abs()[keep].max().item()),
             combine=((h_comb.double() - r_comb).abs()[keep].max().item(),
                      (p_comb.double() - r_comb).abs()[keep].max().item()))
    zero_rows, yard = {}, {}
    scales = _term_scale(case, g1, g2)
    for (key, hg, pg, rg), (formula, T, Tm) in zip((("grad", h_g, p_ga + p_gb, r_ga + r_gb), ("grad_l1_only", h_ga, p_ga, r_ga),
                                                    ("grad_combine_only", h_gb, p_gb, r_gb)), scales):
        assert ((formula - rg).abs().amax(dim=1) <= 1e-9 * T).all(), (name, key)
        eh, eh_ill, _, zr = _ray_err(hg, rg, keep, T, Tm)
        ep, _, ep_all, _ = _ray_err(pg, rg, keep, T, Tm)
        m[key], m[key + "_ill"] = (eh, ep), (eh_ill, ep_all)
        zero_rows[key] = (hg, zr)
        yard[key] = (rg, T, Tm)
        assert rg[zr].abs().max().item() == 0 if zr.any() else True
    m["ill_conditioned_rays"] = int((keep & (scales[0][1] > 0) & ((r_ga + r_gb).abs().amax(dim=1) < ILL * scales[0][1])).sum())
    print("\n[reproj_c vs float64] (kernel, float32 port)", m)
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(m) + "\n")
    except OSError:
        pass
    for key in ("l1", "combine"):
        assert m[key][0] <= max(4 * m[key][1], 1e-6), (key, m)
    for key in ("grad", "grad_l1_only", "grad_combine_only"):
        hg, zr = zero_rows[key]
        assert hg[zr].abs().max().item() == 0 if zr.any() else True, (key, m)   # zero by construction: exactly zero
        assert m[key][0] <= max(4 * m[key][1], 1e-5), (key, m)
        assert m[key + "_ill"][0] <= max(4 * m[key + "_ill"][1], 1e-5), (key, m)
    assert torch.isfinite(h_g).all() and torch.isfinite(h_l1).all() and torch.isfinite(h_comb).all()
    return dict(m=m, keep=keep, mp=mp, mn=mn, r_any=r_any, g1=g1, g2=g2, out=(h_l1, h_comb, h_any, h_g), yard=yard["grad"])


# C: one channel, the 3 of the specialised kernel, an exact group, a ragged tail, many groups, many groups with a ragged tail.
# S: every samples-per-lane instance with ragged lane tails: M = 1 (1, 12, 64), 2 (65), 4 (130: a quarter of the wave dead),
# 8 (512).  R = 301 leaves one ray in the last block of 4; R = 1 and 5 are blocks not full of rays.  `img`: the images have
# another resolution than the (96, 200) the pixels are normalised by.  The near == far rays (R // 20) and the five zero-weight
# rays are make_case's.  The float64 reference of a case costs R * S * C elements, so the largest C goes with R = 5 at S = 512.
CASES = [
    ("C1_S1", dict(C=1, R=301, S=1)),
    ("C3_S12_d", dict(C=3, R=301, S=12, with_deltas=True)),
    ("C4_S64_img_next_behind", dict(C=4, R=301, S=64, img_hw=(50, 77))),
    ("C5_S65_d_outside", dict(C=5, R=301, S=65, with_deltas=True, outside=0.3, edge=0.25)),
    ("C16_S130_d_img", dict(C=16, R=301, S=130, with_deltas=True, img_hw=(50, 77))),
    ("C5_S512", dict(C=5, R=301, S=512)),
    ("C99_S65_img", dict(C=99, R=301, S=65, img_hw=(24, 50))),
    # the default seed (2000 + S + C) puts one of these five rays on a mask threshold (20 % undecided, geometry alone): 2613
    ("C99_S512_d_R5", dict(C=99, R=5, S=512, with_deltas=True, seed=2613)),
    ("C16_S64_R1", dict(C=16, R=1, S=64)),
]


def build_case(name, kw):
    kw = dict(kw)
    C = kw.pop("C")
    case = make_case_c(C, kw.pop("seed", 2000 + kw["S"] + C), **kw)
    if name == "C4_S64_img_next_behind":
        case[6] = INVALID.clone()         # what ReprojLossMonoMultiNew passes for a missing frame
    return case


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_reproj_c_vs_float64(hip, name, kw):
    case = build_case(name, kw)
    r = check_case(name, case)
    if name == "C4_S64_img_next_behind":
        assert not r["mn"].any() and r["mp"].any()
    if name == "C5_S65_d_outside":
        dead = 1.0 - r["r_any"].mean().item()
        assert 0.05 <= dead <= 0.60, dead                             # the block of rays outside both images is there
        assert (r["mp"] ^ r["mn"]).double().mean().item() >= 0.10     # samples with exactly one valid frame


def _raw_fwd(hip, case, generic, full=False):
    """one forward through the C entry itself, with `wnorm`: -> wnorm (R, S), any_valid (R); full: l1 (R), combine (R, C) too"""
    w, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next, img_h, img_w = to_dev(case)
    R, S = w.shape
    C = curr.shape[1]
    a = abi.SoReprojCArgs() if generic else abi.SoReprojArgs()
    if generic:
        stride = (C + 3) // 4 * 4
        cl = lambda img: torch.cat([img.permute(1, 2, 0), img.new_zeros(*img.shape[1:], stride - C)], -1).contiguous()
        img_prev, img_next = cl(img_prev), cl(img_next)
        a.Hi, a.Wi, a.img_stride = img_prev.shape
        a.C, a.curr = C, ptr(curr)
    else:
        a.Hi, a.Wi = img_prev.shape[1:]
        a.curr_rgb = ptr(curr)
    a.weights, a.ts, a.deltas, a.pix = ptr(w), ptr(ts), ptr(deltas), ptr(pix)
    a.T_prev, a.T_next, a.img_prev, a.img_next = ptr(T_prev), ptr(T_next), ptr(img_prev), ptr(img_next)
    a.R, a.S, a.img_h, a.img_w = R, S, img_h, img_w
    wnorm, anyv, l1 = torch.full((R, S), -1.0, device=D0), torch.empty(R, device=D0), torch.empty(R, device=D0)
    comb = torch.empty(R, C, device=D0)
    a.wnorm, a.any_valid, a.l1 = ptr(wnorm), ptr(anyv), ptr(l1)
    if generic:
        a.combine = ptr(comb)
        check(hip.selfocc_reproj_c_fwd(a, current_stream(D0)), "selfocc_reproj_c_fwd")
    else:
        a.rgb_combine = ptr(comb)
        check(hip.selfocc_reproj_fwd(a, current_stream(D0)), "selfocc_reproj_fwd")
    return (wnorm.cpu(), anyv.cpu()) + ((l1.cpu(), comb.cpu()) if full else ())


@pytest.mark.parametrize("C", [1, 5, 99])
def test_wnorm_and_any_valid_are_the_three_channel_entry_s_bits(hip, C):
    """the channel-free part comes from the shared reproj_device.h: same bits at every C, every samples-per-lane instance"""
    for S, kw in ((12, dict()), (65, dict(with_deltas=True, outside=0.3, edge=0.25)), (130, dict(img_hw=(50, 77))),
                  (512, dict(with_deltas=True))):
        geo = make_case(R=61, S=S, seed=3000 + S, **kw)
        ref_w, ref_any = _raw_fwd(hip, geo, generic=False)
        case = make_case_c(C, 3000 + S, R=61, S=S, **kw)
        for a, b in zip(case[:4] + case[5:7], list(geo[:4]) + list(geo[5:7])):
            assert (a is None and b is None) or torch.equal(a, b)         # the same geometry and weights
        got_w, got_any = _raw_fwd(hip, case, generic=True)
        assert torch.equal(got_w, ref_w) and torch.equal(got_any, ref_any), (C, S)
        assert (ref_w != -1.0).all() and ref_any.sum() > 0, (C, S)       # every element written; the case is not empty


def test_three_channels_new_entry_against_old_entry(hip):
    """the same 3-channel case through both pairs of entries: within the yardstick either is held to against float64 (4 x the
    float32 port's error), and, both being one kernel body that differs in the tap fetch alone, equal: l1, combine and any_valid
    in every bit, the gradient in every value (the sign of an exact zero is free).  S: M = 2 and 4 on whole images, M = 1 and 8
    on a small image with masked rays and samples."""
    small = dict(R=61, img_hw=(24, 50), with_deltas=True, outside=0.2, edge=0.2)
    for name, kw in (("S100_d", dict(R=301, S=100, with_deltas=True)), ("S256_img", dict(R=301, S=256, img_hw=(50, 77))),
                     ("S12_d_small", dict(S=12, **small)), ("S512_d_small", dict(S=512, **small))):
        case = list(make_case(seed=4000 + kw["S"], **kw))
        r = check_case("C3_both_" + name, case)
        n_l1, n_comb, n_any, n_g = r["out"]
        o_l1, o_comb, o_any, o_g = _kernel(case, r["g1"], r["g2"], fn=ReprojSampleFunction)
        keep, m = r["keep"], r["m"]
        assert torch.equal(n_any, o_any)
        d_l1, d_comb = (n_l1 - o_l1).abs()[keep].max().item(), (n_comb - o_comb).abs()[keep].max().item()
        rg, T, Tm = r["yard"]
        e, e_ill, _, _ = _ray_err(n_g, o_g, keep, T, Tm)
        print(f"\n[reproj_c vs reproj, C = 3] {name}: l1 {d_l1:.3e} combine {d_comb:.3e} grad e_r {e:.3e} ill {e_ill:.3e} "
              f"bit-equal {torch.equal(n_l1, o_l1) and torch.equal(n_comb, o_comb) and torch.equal(n_g, o_g)}")
        assert d_l1 <= max(4 * m["l1"][1], 1e-6) and d_comb <= max(4 * m["combine"][1], 1e-6), (d_l1, d_comb, m)
        assert e <= max(4 * m["grad"][1], 1e-5) and e_ill <= max(4 * m["grad_ill"][1], 1e-5), (e, e_ill, m)
        assert torch.equal(n_l1, o_l1) and torch.equal(n_comb, o_comb) and torch.equal(n_g, o_g), name


def test_planar_call_is_the_raw_entry_and_checks_its_shapes(hip):
    """ReprojSampleFunction shares its body, the shape checks included, with ReprojSampleCFunction: a valid planar call
    returns what selfocc_reproj_fwd itself returns, a wrong ``curr`` or transform is refused before any launch (either
    would be read out of bounds)"""
    case = list(make_case(R=61, S=65, seed=6065, img_hw=(24, 50)))
    dev = to_dev(case)
    l1, comb, anyv = ReprojSampleFunction.apply(*dev)
    _, r_any, r_l1, r_comb = _raw_fwd(hip, case, generic=False, full=True)
    assert torch.equal(l1.cpu(), r_l1) and torch.equal(comb.cpu(), r_comb) and torch.equal(anyv.cpu(), r_any)
    assert r_any.sum() > 0 and r_l1.abs().max() > 0
    for i, bad in ((4, dev[4][:, :2]), (4, dev[4][:-1]), (5, dev[5][:3]), (6, dev[6][:, :3])):
        args = list(dev)
        args[i] = bad
        with pytest.raises(ValueError):
            ReprojSampleFunction.apply(*args)


@pytest.mark.parametrize("C", [1, 5, 99])
def test_nan_in_the_pad_channels_reaches_no_output(hip, C):
    case = make_case_c(C, 5000 + C, R=61, S=65, with_deltas=True, img_hw=(24, 50), outside=0.2, edge=0.2)
    dev = to_dev(case)
    stride = (C + 3) // 4 * 4
    assert stride > C
    g = torch.Generator().manual_seed(2)
    g1, g2 = torch.randn(61, generator=g).to(D0), torch.randn(61, C, generator=g).to(D0)

    def run(pad):
        imgs = []
        for img in dev[7:9]:
            data = torch.full((*img.shape[1:], stride), pad, device=D0)
            data[..., :C] = img.permute(1, 2, 0)
            imgs.append(ChannelLastImage(data, C))
        wd = dev[0].clone().requires_grad_(True)
        l1, comb, anyv = ReprojSampleCFunction.apply(wd, *dev[1:7], *imgs, *dev[9:])
        grad, = torch.autograd.grad((l1 * g1).sum() + (comb * g2).sum(), wd)
        return l1.detach().cpu(), comb.detach().cpu(), anyv.cpu(), grad.cpu()

    zero, nan = run(0.0), run(float("nan"))
    for a, b in zip(zero, nan):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    assert zero[0].abs().max() > 0 and zero[3].abs().max() > 0


VARIANTS = [
    ('combine_ssim', 'ReprojLossMonoMultiNewCombine', dict(ray_resize=[6, 10]), False),
    ('combine_nossim_deltas', 'ReprojLossMonoMultiNewCombine', dict(no_ssim=True), True),
    ('combine_noautomask', 'ReprojLossMonoMultiNewCombine', dict(ray_resize=[6, 10], no_automask=True), False),
    ('mono_ssim', 'ReprojLossMonoMultiNew', dict(ray_resize=[6, 10]), False),
    ('mono_nossim_deltas', 'ReprojLossMonoMultiNew', dict(no_ssim=True), True)]


def _loss_and_inputs(los, C, cls, kw, use_d):
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    R, S, Hi, Wi, rh, rw = los['dims'].tolist()
    keys = dict(curr_imgs='curr_imgs', prev_imgs='prev_imgs', next_imgs='next_imgs', ray_indices='ray_indices',
                weights='weights', ts='ts', metas='metas', ms_rays='ms_rays')
    if use_d:
        keys['deltas'] = 'deltas'
    lossf = OPENOCC_LOSS.build(dict(type=cls, weight=1.0, input_dict=keys, img_size=[Hi, Wi], dims=C, **kw))
    t = lambda a: torch.tensor(a).to(D0)
    w = [t(los['weights'][c]).requires_grad_(True) for c in range(2)]
    inp = dict(curr_imgs=t(los[f'c{C}.curr']), prev_imgs=t(los[f'c{C}.prev']), next_imgs=t(los[f'c{C}.next']),
               ray_indices=[torch.arange(R, device=D0).unsqueeze(-1).repeat(1, S).flatten()] * 2, weights=w,
               ts=[t(los['ts'][c]) for c in range(2)], deltas=[t(los['deltas'][c]) for c in range(2)],
               metas=[dict(img2prevImg=los['img2prevImg'], img2nextImg=los['img2nextImg'])], ms_rays=t(los['rays']))
    return lossf, inp, w


@pytest.mark.parametrize("C", [1, 5, 16])
@pytest.mark.parametrize("name,cls,kw,use_d", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_losses_with_dims_vs_reference_class(hip, C, name, cls, kw, use_d):
    """loss value and d loss / d weights of the reference's own classes with dims = C on (1, 2, C, h, w) feature maps whose
    resolution differs from img_size (tests/golden/make_golden_reproj_dims.py)"""
    los = np.load(os.path.join(G, "reproj_dims.npz"))
    assert los[f'c{C}.{name}.gap'] > 1e-4 and los[f'c{C}.curr'].shape[2] == C
    lossf, inp, w = _loss_and_inputs(los, C, cls, kw, use_d)
    val = lossf(inp)
    val.backward()
    assert torch.allclose(val.detach().cpu(), torch.tensor(los[f'c{C}.{name}.loss']), rtol=2e-5, atol=1e-7), \
        (val.item(), los[f'c{C}.{name}.loss'])
    gw = torch.stack([x.grad.cpu() for x in w])
    ref = torch.tensor(los[f'c{C}.{name}.gw'])
    assert torch.allclose(gw, ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())
    assert ((gw - ref).norm() / ref.norm()) < 1e-3


@pytest.mark.parametrize("name,cls,kw,use_d", [VARIANTS[0], VARIANTS[3]], ids=["combine", "mono"])
def test_dims_16_step_does_not_synchronise(hip, name, cls, kw, use_d):
    los = np.load(os.path.join(G, "reproj_dims.npz"))
    lossf, inp, w = _loss_and_inputs(los, 16, cls, kw, use_d)
    lossf(inp).backward()                     # first call: lazy initialisation may synchronise
    for x in w:
        x.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        val = lossf(inp)
        val.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(val).item() and all(torch.isfinite(x.grad).all().item() for x in w)
