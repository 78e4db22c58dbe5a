"""GPU: the occupancy metric tail (selfocc_amd/ssc_metric.py, csrc/ssc_metric.hip) against the reference's own IoU,
SSCMetrics and MeanIoU buffers (tests/golden/ssc_metric.npz) and against the drop-in classes fed by the torch-composed
script steps; one launch per call and no host synchronisation."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
KITTI_SHAPES = [(256, 256, 32), (64, 48, 16), (40, 36, 10), (24, 20, 8)]
SSC = ('completion_tp', 'completion_fp', 'completion_fn', 'tps', 'fps', 'fns')
TOTALS = ('total_seen', 'total_correct', 'total_positive')


def gold():
    return np.load(os.path.join(HERE, "golden", "ssc_metric.npz"))


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def sdf_of(q):
    q = torch.from_numpy(q).to(D0)
    return torch.where(q == -128, torch.tensor(float('nan'), device=D0), q.float() * 0.25)


def unpack(bits, shape):
    return torch.from_numpy(np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)).to(D0)


def eq(got, ref, msg=''):
    ref = torch.as_tensor(np.asarray(ref))
    assert torch.equal(got.detach().cpu().reshape(ref.shape).to(ref.dtype), ref), (msg, got, ref)


def metrics():
    from selfocc_amd import IoU, MeanIoU, SSCMetrics
    iou, ssc = IoU(), SSCMetrics(2)
    iou.reset()
    miou = MeanIoU(list(range(1, 20)), 0, [str(c) for c in range(1, 20)], True, 0)
    miou.reset()
    return iou, ssc, miou


def script_steps(sdf, gt, sem, iou, ssc, miou):
    """eval_iou_kitti.py:166-190 composed with torch ops, fed to the drop-in classes (the reference's call sequence)"""
    from selfocc_amd import cityscapes2semantickitti
    D = sdf.shape[2]
    pred_occ = (sdf <= 0.0).to(torch.int)
    gt_occ_raw = torch.flip(gt, [1])
    gt_occ = gt_occ_raw.clone()
    gt_occ[gt_occ == 255] = 0
    gt_occ = torch.nonzero(gt_occ)
    pred_occ[..., D - 4:] = 0
    pred_occ[-6:, ...] = 0
    pred_occ[:, :6, :] = 0
    pred_occ[:, -6:, :] = 0
    iou._after_step(pred_occ, gt_occ)
    ssc.add_batch(pred_occ, gt_occ_raw.clone())
    miou._after_step(pred_occ * cityscapes2semantickitti(sem), gt_occ_raw, gt_occ_raw != 255)
    return pred_occ


def check_kitti(G, k, iou, ssc, miou):
    for name in TOTALS:
        eq(getattr(iou, name), G[f'after{k}.iou.{name}'], (k, 'iou', name))
        eq(getattr(miou, name), G[f'after{k}.miou.{name}'], (k, 'miou', name))
    for name in SSC:
        eq(getattr(ssc, name), G[f'after{k}.ssc.{name}'], (k, 'ssc', name))


def check_epoch(G, iou, ssc, miou):
    assert iou._after_epoch() == G['kitti.iou_epoch']
    for key, v in ssc.get_stats().items():
        eq(torch.as_tensor(v).float(), G[f'kitti.stats.{key}'], key)
    got = miou._after_epoch()
    np.testing.assert_allclose(got, G['kitti.miou_epoch'], rtol=1e-6)


def test_drop_in_classes_match_the_reference_buffers_frame_by_frame(hip):
    G = gold()
    iou, ssc, miou = metrics()
    for k in range(len(KITTI_SHAPES)):
        gt = torch.from_numpy(G[f'f{k}.gt'].astype(np.float32)).to(D0)
        sem = torch.from_numpy(G[f'f{k}.sem'].astype(np.int64)).to(D0)
        pred = script_steps(sdf_of(G[f'f{k}.sdf_q']), gt, sem, iou, ssc, miou)
        eq(pred.bool(), unpack(G[f'f{k}.occ'], pred.shape).cpu(), k)
        check_kitti(G, k, iou, ssc, miou)
    check_epoch(G, iou, ssc, miou)


def test_kitti_occ_metrics_matches_the_reference_buffers_and_d_range(hip):
    from selfocc_amd import kitti_occ_metrics
    G = gold()
    iou, ssc, miou = metrics()
    for k, shape in enumerate(KITTI_SHAPES):
        gt = G[f'f{k}.gt'].astype(np.float32)          # numpy, before the flip, as read_semantic_kitti returns it
        sem = torch.from_numpy(G[f'f{k}.sem'].astype(np.int64)).to(D0)
        out = kitti_occ_metrics(sdf_of(G[f'f{k}.sdf_q']), gt, iou=iou, ssc=ssc, miou=miou, sem=sem, want_occ=True)
        eq(out['d_range'], G[f'f{k}.d_range'], k)
        eq(out['occ'].bool(), unpack(G[f'f{k}.occ'], shape).cpu(), k)
        check_kitti(G, k, iou, ssc, miou)
    check_epoch(G, iou, ssc, miou)


def test_ssc20_masks_and_direct_scores_match_the_reference(hip):
    from selfocc_amd import SSCMetrics
    G = gold()
    s20 = SSCMetrics(20)
    for k in range(2):
        pred = torch.from_numpy(G[f's{k}.pred'].astype(np.int64)).to(D0)
        gt = torch.from_numpy(G[f's{k}.gt'].astype(np.float32)).to(D0)
        ne, ns = unpack(G[f's{k}.nonempty'], gt.shape), unpack(G[f's{k}.nonsurface'], gt.shape)
        s20.add_batch(pred, gt, ne, ns)
        for name in SSC:
            eq(getattr(s20, name), G[f's{k}.after.{name}'], (k, name))
    for key, v in s20.get_stats().items():
        eq(torch.as_tensor(v).float(), G[f'ssc20.stats.{key}'], key)
    pred = torch.from_numpy(G['s0.pred'].astype(np.int64)).to(D0)
    gt = torch.from_numpy(G['s0.gt'].astype(np.float32)).to(D0)
    tp, fp, fn = s20.get_score_completion(pred, gt)
    assert tp.dtype == torch.int64 and tp.dim() == 0
    eq(torch.stack([tp, fp, fn]), G['direct.completion'])
    r = s20.get_score_semantic_and_completion(pred, gt)
    assert r[0].dtype == torch.int32 and tuple(r[0].shape) == (20,)
    eq(torch.stack(r), G['direct.semantic'])


def test_iou_coordinate_and_occ3d_forms_match_the_reference(hip):
    from selfocc_amd import IoU
    G = gold()
    ic = IoU()
    ic.reset()
    for k in range(2):
        outputs = torch.from_numpy(G[f'c{k}.outputs'].astype(np.int64)).to(D0)
        ic._after_step(outputs, torch.from_numpy(G[f'c{k}.coords']).to(D0))
        for name in TOTALS:
            eq(getattr(ic, name), G[f'c{k}.after.{name}'], (k, name))
    assert ic._after_epoch() == G['coords.epoch']
    plain, masked = IoU(use_mask=False), IoU(use_mask=True)
    plain.reset()
    masked.reset()
    shape = (200, 200, 16)
    for k in range(2):
        sems = G[f'o{k}.semantics']
        mask = np.unpackbits(G[f'o{k}.mask'], count=int(np.prod(shape))).reshape(shape).astype(bool)
        outputs = unpack(G[f'o{k}.outputs'], shape).to(torch.int64)
        for m in (plain, masked):
            m._after_step(outputs, {'semantics': sems, 'mask_camera': mask}, occ3d=True)
        for tag, m in (('plain', plain), ('masked', masked)):
            for name in TOTALS:
                eq(getattr(m, name), G[f'o{k}.{tag}.{name}'], (k, tag, name))
    assert plain._after_epoch() == G['occ3d.plain.epoch']
    assert masked._after_epoch() == G['occ3d.masked.epoch']
    assert tuple(plain.xyz.shape) == (200, 200, 16, 3) and 'xyz' not in plain.state_dict()


def random_frame(seed):
    g = torch.Generator(device=D0).manual_seed(seed)
    shape = (256, 256, 32)
    sdf = torch.randn(shape, generator=g, device=D0)
    sdf[torch.rand(shape, generator=g, device=D0) < 0.01] = 0.0
    sdf[torch.rand(shape, generator=g, device=D0) < 0.01] = float('nan')
    gt = torch.randint(0, 20, shape, generator=g, device=D0).float()
    gt[torch.rand(shape, generator=g, device=D0) < 0.2] = 255
    gt[torch.rand(shape, generator=g, device=D0) < 0.4] = 0
    sem = torch.randint(0, 19, shape, generator=g, device=D0)
    return sdf, gt, sem


def state(iou, ssc, miou):
    return [iou.counts.clone(), ssc._counts.clone(), miou.counts.clone()]


def test_full_size_fused_call_equals_the_script_steps_and_is_sync_free_with_one_kernel(hip):
    from selfocc_amd import kitti_occ_metrics
    sdf, gt, sem = random_frame(7)
    ref = metrics()
    script_steps(sdf, gt, sem, *ref)
    got = metrics()
    kitti_occ_metrics(sdf, gt, iou=got[0], ssc=got[1], miou=got[2], sem=sem)        # warm-up: tables, scratch
    got = metrics()
    torch.cuda.synchronize()
    with no_sync():
        out = kitti_occ_metrics(sdf, gt, iou=got[0], ssc=got[1], miou=got[2], sem=sem)
    for a, b in zip(state(*got), state(*ref)):
        assert torch.equal(a, b)
    occ = torch.nonzero(((torch.flip(gt, [1]) != 0) & (torch.flip(gt, [1]) != 255)))[:, 2]
    assert out['d_range'].tolist() == [occ.min().item(), occ.max().item()]
    with no_sync():
        got[0]._after_step(sdf.new_zeros(sdf.shape, dtype=torch.int32), gt)
        got[1].add_batch(sdf.new_zeros(sdf.shape, dtype=torch.int32), gt)
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        kitti_occ_metrics(sdf, gt, iou=got[0], ssc=got[1], miou=got[2], sem=sem)
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    names = [e.name for e in kernels]
    assert len(kernels) == 1 and 'ssc_metric_kernel' in names[0], names


def test_every_gt_and_pred_dtype_gives_identical_counts(hip):
    from selfocc_amd import IoU, SSCMetrics
    sdf, gt, sem = random_frame(11)
    pred = (sdf <= 0).to(torch.int32)
    cut = (gt[:, :, :30].contiguous(), pred[:, :, :30].contiguous())      # D % 4 != 0: one voxel per lane
    for g_, p_ in ((gt, pred), cut):
        results = []
        for gd in (torch.float32, torch.uint8, torch.int32, torch.int64):
            for pd in (torch.bool, torch.uint8, torch.int32, torch.int64):
                iou, ssc = IoU(), SSCMetrics(20)
                iou.reset()
                iou._after_step(p_.to(pd), g_.to(gd))
                ssc.add_batch(p_.to(pd), g_.to(gd))
                results.append(torch.cat([iou.counts, ssc._counts]))
        assert all(torch.equal(r, results[0]) for r in results[1:])


def test_nan_sdf_all_255_frames_and_reset(hip):
    from selfocc_amd import kitti_occ_metrics
    shape = (64, 48, 16)
    iou, ssc, miou = metrics()
    sdf = torch.full(shape, float('nan'), device=D0)
    gt = torch.randint(1, 20, shape, device=D0).float()
    sem = torch.zeros(shape, dtype=torch.int64, device=D0)
    out = kitti_occ_metrics(sdf, gt, iou=iou, ssc=ssc, miou=miou, sem=sem, want_occ=True)
    assert not out['occ'].any() and iou.counts[1:].sum().item() == 0 and iou.counts[0].item() == gt.numel()
    assert ssc._counts[0].item() == 0 and ssc._counts[1].item() == 0 and ssc._counts[2].item() == gt.numel()
    iou.reset()
    ssc.reset()
    miou.reset()
    sdf = torch.full(shape, -1.0, device=D0)
    out = kitti_occ_metrics(sdf, torch.full(shape, 255.0, device=D0), iou=iou, ssc=ssc, miou=miou, sem=sem)
    assert out['d_range'].tolist() == [-1, -1]
    assert iou.counts[0].item() == 0 and iou.counts[2].item() == out_pos(shape)
    assert not ssc._counts.any() and not miou.counts.any()
    assert iou._after_epoch() == 100.0             # nothing seen: the reference appends 1
    st = ssc.get_stats()
    assert st['precision'] == 0 and st['recall'] == 0 and st['iou'] == 0
    assert torch.equal(st['iou_ssc'].cpu(), torch.zeros(2))
    iou.reset()
    ssc.reset()
    assert not iou.counts.any() and not ssc._counts.any() and not iou.bad.any()


def out_pos(shape):
    H, W, D = shape
    return (H - 6) * (W - 12) * (D - 4)


def test_out_of_range_coordinates_make_after_epoch_raise(hip):
    from selfocc_amd import IoU
    iou = IoU()
    iou.reset()
    outputs = torch.ones(8, 6, 4, dtype=torch.int32, device=D0)
    coords = torch.tensor([[0, 0, 0], [7, 5, 3], [-1, -1, -1], [8, 0, 0], [0, -7, 0], [0, 0, 1 << 40]],
                          dtype=torch.int64, device=D0)
    iou._after_step(outputs, coords)
    assert iou.counts.tolist() == [6, 3, 192] and iou.bad.item() == 3
    with pytest.raises(IndexError):
        iou._after_epoch()
