#!/usr/bin/env python
"""Generate tests/golden/ssc_metric.npz by running the REAL reference IoU, MeanIoU, cityscapes2semantickitti
(utils/metric_util.py) and SSCMetrics (utils/scenerf_metric.py), loaded by file path from the read-only reference tree
with the stand-ins of make_golden.install_stubs, on seeded synthetic frames, on CPU.  In this process only,
``Tensor.cuda`` is the identity and ``dist.barrier`` / ``dist.all_reduce`` are no-ops.

Cases (every buffer is recorded after every frame):
  kitti  : eval_iou_kitti.py:166-190 restated line by line (threshold, flip, the four crops, nonzero, IoU, SSCMetrics(2),
           --sem MeanIoU through the cityscapes table) on a 256 x 256 x 32 frame, a 64 x 48 x 16 and a 40 x 36 x 10 frame
           (D % 4 != 0) and a 24 x 20 x 8 frame without an occupied voxel (the reference's max_d raises there: no
           d_range is recorded for it).  The crop is d >= D - 4, the last 6 h, the first and last 6 w (the script's at
           D = 32).  Labels 0-19 in blocks with 255 regions; sdf on a 0.25 grid with NaN and sdf == thresh = 0 exactly;
           occupied voxels on the crop borders.
  ssc20  : SSCMetrics(20), predictions 0-21, labels 0-21 and 255, both masks; two frames.
  direct : get_score_completion / get_score_semantic_and_completion of SSCMetrics(20) with nonempty=None.
  coords : IoU in the coordinate form, with duplicated rows.
  occ3d  : IoU._after_step(..., occ3d=True) on 200 x 200 x 16 Occ3D dicts, with and without use_mask; two frames.
Then the values of IoU._after_epoch, SSCMetrics.get_stats and MeanIoU._after_epoch.  Every total stays below 2^24, so
the reference's float32 buffers are exact.

Storage: sdf as int8 quarter units (-128 = NaN), labels u8, sem int8, binary volumes np.packbits.

Run:  python tests/golden/make_golden_ssc_metric.py        (needs the reference tree; ~20 s)
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402

KITTI_SHAPES = [(256, 256, 32), (64, 48, 16), (40, 36, 10), (24, 20, 8)]
NAN_Q = -128


def blocks(rng, shape, bs, values, p):
    """a volume of `values` drawn with probabilities p on (bs)-blocks"""
    n = [-(-s // b) for s, b in zip(shape, bs)]
    v = rng.choice(values, size=n, p=p)
    for ax, b in enumerate(bs):
        v = np.repeat(v, b, axis=ax)
    return v[:shape[0], :shape[1], :shape[2]]


def sprinkle(rng, vol, frac, values):
    m = rng.random(vol.shape) < frac
    vol = vol.copy()
    vol[m] = rng.choice(values, size=int(m.sum()))
    return vol


def kitti_frame(rng, shape, empty=False):
    H, W, D = shape
    q = blocks(rng, shape, (8, 8, 4), np.array([-8, -1, 0, 1, 8], np.int8), [0.25, 0.15, 0.1, 0.15, 0.35])
    q = sprinkle(rng, q, 0.02, np.array([-4, 0, 4, NAN_Q], np.int8))
    q[:, :, D - 5:D - 3] = 0                       # sdf == thresh on both sides of the d crop border
    q[H - 7:H - 5] = -4                            # occupied on the h crop border
    q[:, 5:7] = -4
    q[:, W - 7:W - 5] = -4                         # and on the two w borders
    lab = blocks(rng, shape, (8, 4, 4), np.arange(21, dtype=np.uint8) % 20,
                 np.r_[0.4, np.full(19, 0.6 / 20), 0.6 / 20])
    lab = np.where(blocks(rng, shape, (16, 16, 8), np.array([0, 1], np.uint8), [0.85, 0.15]) == 1, 255, lab)
    lab = sprinkle(rng, lab, 0.01, np.r_[np.arange(20), 255].astype(np.uint8))
    if empty:
        lab = np.where(lab == 255, 255, 0).astype(np.uint8)
    sem = blocks(rng, shape, (4, 4, 4), np.arange(19, dtype=np.int8), None)
    return q.astype(np.int8), lab.astype(np.uint8), sem.astype(np.int8)


def sdf_of(q):
    return np.where(q == NAN_Q, np.float32(np.nan), q.astype(np.float32) * np.float32(0.25)).astype(np.float32)


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *rel.split('/')))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    assert os.path.isdir(REF), f"{REF} not found: golden vectors can only be regenerated where the reference is mounted"
    install_stubs()
    torch.Tensor.cuda = lambda self, *a, **k: self          # this process only: the reference's .cuda() calls
    dist.barrier = lambda *a, **k: None
    dist.all_reduce = lambda *a, **k: None
    mu = load('ref_metric_util', 'utils/metric_util.py')
    sm = load('ref_scenerf_metric', 'utils/scenerf_metric.py')
    rng = np.random.default_rng(20241015)
    out = {}

    # ---- kitti: the script's tail ------------------------------------------------------------------------------
    iou, ssc = mu.IoU(), sm.SSCMetrics(2)
    iou.reset()
    miou = mu.MeanIoU(list(range(1, 20)), 0, [str(c) for c in range(1, 20)], True, 0)
    miou.reset()
    for k, shape in enumerate(KITTI_SHAPES):
        q, lab, sem_np = kitti_frame(rng, shape, empty=(k == 3))
        out[f'f{k}.sdf_q'], out[f'f{k}.gt'], out[f'f{k}.sem'] = q, lab, sem_np
        D = shape[2]
        pred_occ = (torch.from_numpy(sdf_of(q)) <= 0.0).to(torch.int)
        gt_occ_raw = torch.flip(torch.from_numpy(lab.astype(np.float32)), [1])
        gt_occ = gt_occ_raw.clone()
        gt_occ[gt_occ == 255] = 0
        gt_occ = torch.nonzero(gt_occ)
        if gt_occ.shape[0]:
            out[f'f{k}.d_range'] = np.array([int(gt_occ[:, 2].min()), int(gt_occ[:, 2].max())], np.int32)
        else:
            out[f'f{k}.d_range'] = np.array([-1, -1], np.int32)     # declared deviation: the reference raises
        pred_occ[..., D - 4:] = 0
        pred_occ[-6:, ...] = 0
        pred_occ[:, :6, :] = 0
        pred_occ[:, -6:, :] = 0
        out[f'f{k}.occ'] = np.packbits(pred_occ.numpy().astype(bool))
        iou._after_step(pred_occ, gt_occ)
        ssc.add_batch(pred_occ, gt_occ_raw.clone())
        sem = mu.cityscapes2semantickitti(torch.from_numpy(sem_np.astype(np.int64)))
        miou._after_step(pred_occ * sem, gt_occ_raw, gt_occ_raw != 255)
        for name in ('total_seen', 'total_correct', 'total_positive'):
            out[f'after{k}.iou.{name}'] = getattr(iou, name).clone().numpy()
            out[f'after{k}.miou.{name}'] = getattr(miou, name).clone().numpy()
        for name in ('completion_tp', 'completion_fp', 'completion_fn', 'tps', 'fps', 'fns'):
            out[f'after{k}.ssc.{name}'] = getattr(ssc, name).clone().numpy()
    out['kitti.iou_epoch'] = np.float64(iou._after_epoch())
    for key, v in ssc.get_stats().items():
        out[f'kitti.stats.{key}'] = np.asarray(v, dtype=np.float32)
    out['kitti.miou_epoch'] = np.array(miou._after_epoch(), np.float64)
    out['lut.cityscapes2semantickitti'] = mu.cityscapes2semantickitti(torch.arange(19)).numpy()
    out['lut.openseed2nuscenes'] = mu.openseed2nuscenes(torch.arange(21)).numpy()

    # ---- ssc20: multi-class predictions, both masks; then direct get_score_* ------------------------------------
    s20 = sm.SSCMetrics(20)
    for k, shape in enumerate([(48, 40, 16), (30, 26, 6)]):
        vals = np.r_[np.arange(22), 255].astype(np.uint8)
        p_lab = np.r_[np.full(22, 0.9 / 22), 0.1]
        gt = sprinkle(rng, blocks(rng, shape, (4, 4, 2), vals, p_lab), 0.05, vals)
        pred = np.where(rng.random(shape) < 0.6, np.where(gt == 255, 0, gt),
                        blocks(rng, shape, (2, 2, 2), np.arange(22, dtype=np.uint8), None)).astype(np.uint8)
        ne, ns = rng.random(shape) < 0.8, rng.random(shape) < 0.7
        out[f's{k}.pred'], out[f's{k}.gt'] = pred, gt
        out[f's{k}.nonempty'], out[f's{k}.nonsurface'] = np.packbits(ne), np.packbits(ns)
        s20.add_batch(torch.from_numpy(pred.astype(np.int64)), torch.from_numpy(gt.astype(np.float32)),
                      torch.from_numpy(ne), torch.from_numpy(ns))
        for name in ('completion_tp', 'completion_fp', 'completion_fn', 'tps', 'fps', 'fns'):
            out[f's{k}.after.{name}'] = getattr(s20, name).clone().numpy()
    for key, v in s20.get_stats().items():
        out[f'ssc20.stats.{key}'] = np.asarray(v, dtype=np.float32)
    pred_d, gt_d = out['s0.pred'], out['s0.gt']
    tp, fp, fn = s20.get_score_completion(torch.from_numpy(pred_d.astype(np.int64)),
                                          torch.from_numpy(gt_d.astype(np.float32)))
    out['direct.completion'] = np.array([int(tp), int(fp), int(fn)], np.int64)
    r = s20.get_score_semantic_and_completion(torch.from_numpy(pred_d.astype(np.int64)),
                                              torch.from_numpy(gt_d.astype(np.float32)))
    out['direct.semantic'] = torch.stack(r).numpy()

    # ---- coords: the drop-in coordinate form, with duplicated rows ---------------------------------------------
    ic = mu.IoU()
    ic.reset()
    for k, shape in enumerate([(32, 24, 8), (16, 16, 4)]):
        outputs = blocks(rng, shape, (2, 2, 2), np.array([0, 1, 2], np.int8), [0.5, 0.4, 0.1])
        idx = rng.integers(0, np.prod(shape), size=np.prod(shape) // 5)
        idx = np.r_[idx, idx[:50], idx[:10]]                          # duplicates counted as often as they occur
        coords = np.stack(np.unravel_index(idx, shape), 1).astype(np.int64)
        out[f'c{k}.outputs'], out[f'c{k}.coords'] = outputs, coords
        ic._after_step(torch.from_numpy(outputs.astype(np.int64)), torch.from_numpy(coords))
        for name in ('total_seen', 'total_correct', 'total_positive'):
            out[f'c{k}.after.{name}'] = getattr(ic, name).clone().numpy()
    out['coords.epoch'] = np.float64(ic._after_epoch())

    # ---- occ3d: the Occ3D dict form, with and without use_mask -------------------------------------------------
    shape = (200, 200, 16)
    plain, masked = mu.IoU(use_mask=False), mu.IoU(use_mask=True)
    plain.reset()
    masked.reset()
    for k in range(2):
        sems = blocks(rng, shape, (4, 4, 2), np.arange(18, dtype=np.uint8), np.r_[np.full(17, 0.3 / 17), 0.7])
        mask = blocks(rng, shape, (8, 8, 4), np.array([False, True]), [0.3, 0.7])
        outputs = blocks(rng, shape, (2, 2, 2), np.array([0, 1], np.uint8), [0.7, 0.3])
        out[f'o{k}.semantics'], out[f'o{k}.mask'] = sems, np.packbits(mask)
        out[f'o{k}.outputs'] = np.packbits(outputs.astype(bool))
        for m in (plain, masked):
            m._after_step(torch.from_numpy(outputs.astype(np.int64)), {'semantics': sems, 'mask_camera': mask},
                          occ3d=True)
        for tag, m in (('plain', plain), ('masked', masked)):
            for name in ('total_seen', 'total_correct', 'total_positive'):
                out[f'o{k}.{tag}.{name}'] = getattr(m, name).clone().numpy()
    out['occ3d.plain.epoch'] = np.float64(plain._after_epoch())
    out['occ3d.masked.epoch'] = np.float64(masked._after_epoch())

    for k, v in out.items():
        if v.dtype == np.float32 and v.ndim and k.split('.')[-1].startswith(('total', 'completion', 'tps', 'fps', 'fns')):
            assert float(np.abs(v).max(initial=0)) < 2 ** 24, k
    path = os.path.join(HERE, 'ssc_metric.npz')
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, keys={len(out)}")


if __name__ == '__main__':
    main()
