"""GPU: ReprojLossMonoMultiNew(sdf_loss=True) against the REAL reference class (tests/golden/sdf_loss.npz, written by
make_golden_sdf_loss.py, which asserts and stores the margins that keep every arg-max / arg-min of the fixture away from a
tie), and the head's ``sample_sdf`` output through MultiLoss into the SDF volume's gradient.

Bounds: the loss and d / d weights as tests/test_golden_gpu.py holds the same class without the term (rtol 2e-5 / atol 1e-7;
rtol 2e-3, atol 2e-3 of the maximum).  d / d sample_sdf has exactly the reference's support — one entry per ray a temporal
frame wins, at that frame's pick — and its values are sign(sdf) * weight / (count * cameras): rtol 1e-5."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
D0 = torch.device("cuda:0")
KEYS = dict(curr_imgs='curr_imgs', prev_imgs='prev_imgs', next_imgs='next_imgs', ray_indices='ray_indices',
            weights='weights', ts='ts', metas='metas', ms_rays='ms_rays')
VARIANTS = [('ssim', dict(ray_resize=[6, 10]), False), ('nossim_deltas', dict(no_ssim=True), True),
            ('noautomask', dict(ray_resize=[6, 10], no_automask=True), False)]


def _build(Hi, Wi, use_d, sample_sdfs, **kw):
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    keys = dict(KEYS)
    if use_d:
        keys['deltas'] = 'deltas'
    if sample_sdfs:
        keys['sample_sdfs'] = 'sample_sdfs'
    return OPENOCC_LOSS.build(dict(type='ReprojLossMonoMultiNew', weight=1.0, input_dict=keys, img_size=[Hi, Wi], **kw))


def _inputs(gold):
    R, S = gold['dims'].tolist()[:2]
    t = lambda a: torch.tensor(a).to(D0)
    w = [t(gold['weights'][c]).requires_grad_(True) for c in range(2)]
    s = [t(gold['sample_sdf'][c]).requires_grad_(True) for c in range(2)]
    inp = dict(curr_imgs=t(gold['curr']), prev_imgs=t(gold['prev']), next_imgs=t(gold['next']),
               ray_indices=[torch.arange(R, device=D0).unsqueeze(-1).repeat(1, S).flatten()] * 2, weights=w,
               ts=[t(gold['ts'][c]) for c in range(2)], deltas=[t(gold['deltas'][c]) for c in range(2)],
               metas=[dict(img2prevImg=gold['img2prevImg'], img2nextImg=gold['img2nextImg'])], ms_rays=t(gold['rays']),
               sample_sdfs=s)
    return inp, w, s


@pytest.mark.parametrize("name,kw,use_d", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_sdf_loss_vs_reference_class(hip, name, kw, use_d):
    gold = np.load(os.path.join(G, "sdf_loss.npz"))
    R, S, Hi, Wi = gold['dims'].tolist()[:4]
    # the fixture is away from every tie (the generator asserted it; the file carries the figures)
    weight_gap, border_px, cand_gap, masked_prev, masked_next = gold[f'{name}.margins'].tolist()
    assert weight_gap > 1e-3 and border_px > 1e-3 and cand_gap > 1e-4
    assert masked_prev >= 12 and masked_next == 0          # fully masked rays in every previous frame: the pick-is-0 branch
    lossf = _build(Hi, Wi, use_d, True, sdf_loss=True, sdf_loss_weight=0.1, **kw)
    inp, w, s = _inputs(gold)
    val = lossf(inp)
    val.backward()
    ref_loss = torch.tensor(gold[f'{name}.loss'])
    print(f"\n[sdf_loss {name}] loss {val.item():.8f} reference {ref_loss.item():.8f}")
    assert torch.allclose(val.detach().cpu(), ref_loss, rtol=2e-5, atol=1e-7), (val.item(), ref_loss.item())
    gw, ref = torch.stack([x.grad.cpu() for x in w]), torch.tensor(gold[f'{name}.gw'])
    assert torch.allclose(gw, ref, rtol=2e-3, atol=2e-3 * ref.abs().max().item())
    gs, ref = torch.stack([x.grad.cpu() for x in s]), torch.tensor(gold[f'{name}.gsdf'])
    assert int((ref != 0).sum()) in (54, 55, 120)
    assert torch.equal(gs != 0, ref != 0), ((gs != 0).sum().item(), (ref != 0).sum().item())
    on = ref != 0
    assert torch.allclose(gs[on], ref[on], rtol=1e-5, atol=0.0), ((gs[on] - ref[on]).abs() / ref[on].abs()).max()


@pytest.mark.parametrize("name,kw,use_d", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_sdf_loss_off_changes_nothing(hip, name, kw, use_d):
    """sdf_loss=False with sample_sdfs handed in == the class without any of it, bit for bit (value and gradient)"""
    gold = np.load(os.path.join(G, "sdf_loss.npz"))
    Hi, Wi = gold['dims'].tolist()[2:4]
    res = []
    for sample_sdfs, extra in ((True, dict(sdf_loss=False, sdf_loss_weight=0.1)), (False, {})):
        lossf = _build(Hi, Wi, use_d, sample_sdfs, **extra, **kw)
        inp, w, s = _inputs(gold)
        val = lossf(inp)
        val.backward()
        assert all(x.grad is None for x in s)
        res.append((val.detach().cpu(), torch.stack([x.grad.cpu() for x in w])))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    # and the term, when on, adds weight * mean over cameras of a non-negative quantity
    on = _build(Hi, Wi, use_d, True, sdf_loss=True, sdf_loss_weight=0.1, **kw)
    assert on(_inputs(gold)[0]).item() > res[0][0].item()


def test_head_sample_sdf_through_multiloss_reaches_the_sdf_volume(hip):
    """NeuSHead(return_sample_sdf=True) -> MultiLoss(ReprojLossMonoMultiNew(sdf_loss=True)) with the default input_dict,
    without a host synchronisation; d loss / d (SDF volume) is finite and is not the gradient of the run with weight 0"""
    import test_head_gpu as th
    from selfocc_amd.registry import OPENOCC_LOSS
    os.environ['eval'] = 'false'
    head = th.make_head(return_sample_sdf=True).train()

    def loss_fn(weight):
        return OPENOCC_LOSS.build(dict(type='MultiLoss', loss_cfgs=[
            dict(type='ReprojLossMonoMultiNew', weight=1.0, img_size=[64, 64], ray_resize=[6, 10], sdf_loss=True,
                 sdf_loss_weight=weight)]))
    on, off = loss_fn(0.1), loss_fn(0.0)

    def step(rep, metas, imgs):
        out = head(rep, metas, global_iter=0)
        assert len(out['sample_sdf']) == 2 and out['sample_sdf'][0].shape == out['weights'][0].shape
        vol = head.model.field.volume.sdf
        inputs = dict(out, metas=metas, **imgs)
        tot_on, parts = on(inputs)
        g_on, = torch.autograd.grad(tot_on, vol, retain_graph=True)
        g_off, = torch.autograd.grad(off(inputs)[0], vol)
        return tot_on, g_on, g_off
    np.random.seed(0)
    step(*th.make_inputs(seed=0))              # warm-up: workspaces, constant tensors
    new = th.make_inputs(seed=1)               # the data loader's side
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tot, g_on, g_off = step(*new)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(tot) and torch.isfinite(g_on).all() and torch.isfinite(g_off).all()
    assert g_on.abs().sum() > 0 and not torch.equal(g_on, g_off)
