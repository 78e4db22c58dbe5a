"""GPU: the median depth in one launch (selfocc_render_median).

The oracle of every case is `median_depth_reference` applied to the `weights` / `ts` that `render_rays(per_sample=True)` —
the sample-parallel kernel every earlier version ships, not the kernel under test — returns for the same inputs.  Index and
depth must be EQUAL on every ray: no tolerance, no ray left out.  Before a case looks at the kernel it asserts, on the
oracle's indices alone, that the scene makes the comparison mean something (median_cases.scene_is_sharp).
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

from selfocc_amd import abi
from selfocc_amd.render import SDFVolume, render_rays, render_median_depth, median_depth_reference
import median_cases as mc

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")


def _dev(rays):
    c = lambda t: None if t is None else t.to(D0)
    return dataclasses.replace(rays, origins=c(rays.origins), dirs=c(rays.dirs), dir_norm=c(rays.dir_norm), img2lidar=c(rays.img2lidar))


def _oracle(vol, rays, cfg, t_rand):
    o = render_rays(vol, rays, cfg, per_sample=True, t_rand=t_rand)
    w, ts = o['weights'].cpu(), o['ts'].cpu()
    depth, index = median_depth_reference(w, ts)
    return depth, index, w


def _assert_equal(got, depth, index, label):
    gj, gd = got['median_index'].cpu(), got['median_depth'].cpu()
    assert gj.dtype == torch.int32 and gd.dtype == torch.float32 and gj.shape == index.shape and gd.shape == depth.shape
    wrong = (gj != index).nonzero().flatten().tolist()
    assert not wrong, f"{label}: median_index differs on {len(wrong)} of {index.numel()} rays, first {wrong[:5]}: " \
                      f"got {gj[wrong[:5]].tolist()} want {index[wrong[:5]].tolist()}"
    # bit for bit (a NaN depth would still have to be the same NaN)
    assert torch.equal(gd.view(torch.int32), depth.view(torch.int32)), f"{label}: median_depth differs"


@pytest.mark.parametrize("pixel", [True, False], ids=["pixgrid", "explicit"])
@pytest.mark.parametrize("name", list(mc.CASES))
def test_median_equals_the_reference_on_per_sample_weights(hip, name, pixel):
    kind, rays, cfg, t_rand = mc.case(name, pixel)
    assert rays.n_rays == (mc.N_CAMS * mc.NX * mc.NY if pixel else mc.N_EXPLICIT) and rays.n_rays % 64 != 0
    vol = mc.make_volume(kind)[0].to(D0)
    rays, t_rand = _dev(rays), None if t_rand is None else t_rand.to(D0)
    depth, index, w = _oracle(vol, rays, cfg, t_rand)
    assert mc.scene_is_sharp(index.numpy(), w.numpy()) == [], mc.scene_stats(index.numpy(), w.numpy())
    got = render_median_depth(vol, rays, cfg, t_rand=t_rand, want_index=True)
    _assert_equal(got, depth, index, f"{name} {'pixgrid' if pixel else 'explicit'}")
    only = render_median_depth(vol, rays, cfg, t_rand=t_rand)
    assert set(only) == {'median_depth'} and torch.equal(only['median_depth'], got['median_depth'])


def test_inv_s_comes_from_the_device_copy(hip):
    kind, rays, cfg, _ = mc.case('base', True)
    vol, rays = mc.make_volume(kind)[0].to(D0), _dev(rays)
    want = render_median_depth(vol, rays, dataclasses.replace(cfg, inv_s=200.0), want_index=True)
    cfg_dev = dataclasses.replace(cfg, inv_s=1.0, inv_s_dev=torch.tensor([200.0], device=D0))       # the host value must lose
    depth, index, w = _oracle(vol, rays, cfg_dev, None)
    assert mc.scene_is_sharp(index.numpy(), w.numpy()) == []
    got = render_median_depth(vol, rays, cfg_dev, want_index=True)
    _assert_equal(got, depth, index, "inv_s_dev")
    assert torch.equal(got['median_index'], want['median_index']) and torch.equal(got['median_depth'], want['median_depth'])
    soft = render_median_depth(vol, rays, dataclasses.replace(cfg, inv_s=1.0), want_index=True)
    assert not torch.equal(soft['median_index'], got['median_index'])          # ... and inv_s matters on this scene


@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_feature_volumes_are_ignored(hip, feat_dtype):
    """geometry only: a volume that carries 24 feature channels gives what the bare SDF volume gives"""
    kind, rays, cfg, _ = mc.case('base', False)
    rays = _dev(rays)
    bare = mc.make_volume(kind)[0].to(D0)
    full = mc.make_volume(kind, n_feat=24, feat_dtype=feat_dtype)[0].to(D0)
    assert full.feat.shape[-1] == 24 and full.n_sem == 21 and torch.equal(full.sdf, bare.sdf)
    depth, index, w = _oracle(full, rays, cfg, None)                   # the oracle marches the full volume
    assert mc.scene_is_sharp(index.numpy(), w.numpy()) == []
    got = render_median_depth(full, rays, cfg, want_index=True)
    _assert_equal(got, depth, index, f"24 channels {feat_dtype}")
    ref = render_median_depth(bare, rays, cfg, want_index=True)
    assert torch.equal(got['median_index'], ref['median_index']) and torch.equal(got['median_depth'], ref['median_depth'])


def test_no_rays_is_no_launch(hip):
    kind, rays, cfg, _ = mc.case('base', False)
    vol = mc.make_volume(kind)[0].to(D0)
    none = dataclasses.replace(_dev(rays), origins=torch.zeros(0, 3, device=D0), dirs=torch.zeros(0, 3, device=D0),
                               dir_norm=torch.zeros(0, device=D0))
    out = render_median_depth(vol, none, cfg, want_index=True)
    assert out['median_depth'].shape == (0,) and out['median_index'].shape == (0,)


# ---- the head -----------------------------------------------------------------------------------------------------
RENDER_KEYS = {'ms_depths', 'ms_colors', 'vis_normal', 'ms_accs', 'ms_rays', 'ms_max_depths', 'sem'}
FORWARD_KEYS = {'ms_depths', 'ms_colors', 'ms_accs', 'ms_fars', 'ms_rays', 'origin', 'direction', 'direction_norm', 'ray_indices',
                'weights', 'ts', 'deltas', 'eik_grad', 'uniform_sdf', 'ms_max_depths', 'second_grad', 'sem'}


def _head(**kw):
    from test_head_gpu import make_head
    return make_head(render_bkgd='white', **kw)


def _direct(head, metas):
    """the head's own rays and configuration through the operator-level call"""
    vol = head.model.field.volume.detached()
    rays, _pix, num_cams, num_rays = head._rays(metas, vol.sdf.device)
    cfg = head._render_cfg(False)
    cfg.inv_s_dev = head.model.field.inv_s_device()
    return render_median_depth(vol, rays, cfg)['median_depth'].reshape(1, num_cams, num_rays)


def test_head_render_adds_the_key_only_on_request(hip):
    from test_head_gpu import make_inputs
    os.environ['eval'] = 'true'
    try:
        rep, metas, _ = make_inputs()
        on, off = _head(return_median_depth=True).eval(), _head().eval()
        assert off.return_median_depth is False
        with torch.no_grad():
            for h in (on, off):
                h.prepare(rep, metas)
            out_on, out_off = on.render(metas), off.render(metas)
            assert set(out_off) == RENDER_KEYS and set(out_on) == RENDER_KEYS | {'ms_depths_median'}
            med = out_on['ms_depths_median']
            assert isinstance(med, list) and len(med) == 1 and med[0].shape == (1, 2, 60) == out_on['ms_depths'][0].shape
            assert torch.equal(med[0], _direct(on, metas))
            # the existing per-ray outputs do not notice the extra launch
            for k in RENDER_KEYS:
                a, b = out_on[k], out_off[k]
                assert torch.equal(a[0], b[0]) if isinstance(a, list) else torch.equal(a, b), k
            # one call can override the head's default, either way
            assert set(on.render(metas, median_depth=False)) == RENDER_KEYS
            once = off.render(metas, median_depth=True)
            assert set(once) == RENDER_KEYS | {'ms_depths_median'} and torch.equal(once['ms_depths_median'][0], med[0])
            # a crossing inside the frame: the median is a depth along the ray, between the near and the far plane
            assert torch.isfinite(med[0]).all() and (med[0] >= 0).all() and med[0].max() > 0
    finally:
        os.environ['eval'] = 'false'


@pytest.mark.parametrize("two_split", [False, True], ids=["one_set", "two_split"])
def test_head_forward_adds_the_key_from_its_own_samples(hip, two_split):
    """training mode: the jitter is drawn inside forward(); the median must come from that very draw, i.e. be the
    reference applied to the per-sample weights / ts the same call returns.  two_split slices it like ms_max_depths."""
    from test_head_gpu import make_inputs
    os.environ['eval'] = 'false'
    kw = dict(trans_kw=['img2lidar', 'temImg2lidar'], two_split=True) if two_split else {}
    rep, metas, _ = make_inputs()
    n_out = 2                                     # cameras in the per-ray maps: both of one set, or the first set of two
    for flag in (True, False):
        head = _head(return_median_depth=flag, **kw).train()
        np.random.seed(0)
        torch.manual_seed(1)
        out = head(rep, metas, global_iter=0)
        if not flag:
            assert set(out) == FORWARD_KEYS
            continue
        assert set(out) == FORWARD_KEYS | {'ms_depths_median'}
        med = out['ms_depths_median'][0]
        assert med.shape == out['ms_max_depths'][0].shape == (1, n_out, 60) and not med.requires_grad
        assert len(out['weights']) == n_out
        for cam in range(n_out):
            w, ts = out['weights'][cam].detach().cpu().reshape(60, 32), out['ts'][cam].detach().cpu().reshape(60, 32)
            want, _ = median_depth_reference(w, ts)
            assert torch.equal(med[0, cam].cpu(), want), cam


def test_head_with_a_random_background_and_colour(hip):
    """the builder's default head (render_bkgd='random', colour + 5 classes), as every shipped config has it: the median is
    geometry only, so the per-ray background of the render beside it is none of its business"""
    from test_head_gpu import make_head, make_inputs
    rep, metas, _ = make_inputs()
    head = make_head(return_median_depth=True)
    assert head.render_bkgd == 'random' and head._render_cfg(True).bkgd_mode == abi.BKGD_PER_RAY
    os.environ['eval'] = 'false'
    np.random.seed(0)
    out = head.train()(rep, metas, global_iter=0)
    assert out['ms_colors'][0].shape == (1, 2, 60, 3) and out['ms_depths_median'][0].shape == (1, 2, 60)
    for cam in range(2):
        w, ts = out['weights'][cam].detach().cpu().reshape(60, 32), out['ts'][cam].detach().cpu().reshape(60, 32)
        assert torch.equal(out['ms_depths_median'][0][0, cam].cpu(), median_depth_reference(w, ts)[0]), cam
    os.environ['eval'] = 'true'
    try:
        head.eval()
        with torch.no_grad():
            head.prepare(rep, metas)
            got = head.render(metas)
            assert got['ms_colors'][0].shape == (1, 2, 60, 3) and torch.equal(got['ms_depths_median'][0], _direct(head, metas))
            assert torch.equal(head.render(metas, median_depth=True)['ms_depths_median'][0], got['ms_depths_median'][0])
    finally:
        os.environ['eval'] = 'false'


def test_the_call_ignores_background_and_march_switches(hip):
    kind, rays, cfg, _ = mc.case('base', True)
    vol, rays = mc.make_volume(kind)[0].to(D0), _dev(rays)
    want = render_median_depth(vol, rays, cfg, want_index=True)
    odd = dataclasses.replace(cfg, bkgd_mode=abi.BKGD_PER_RAY, clamp_rgb=True, exact=True, brick=False, skip=False, face_safe=False,
                              ahead=False, depth_div_norm=False)
    got = render_median_depth(vol, rays, odd, want_index=True)
    assert torch.equal(got['median_index'], want['median_index']) and torch.equal(got['median_depth'], want['median_depth'])
