"""Host side of the occupancy metric tail of eval_iou_kitti.py (:166-190): IoU (utils/metric_util.py:168-233),
SSCMetrics (utils/scenerf_metric.py:43-188), the two class LUTs (metric_util.py:9-64) and ``kitti_occ_metrics``, the
whole per-frame tail after ``forward_occ`` in one launch.  The counting is csrc/ssc_metric.hip; nothing in
``IoU._after_step``, ``SSCMetrics.add_batch`` or ``kitti_occ_metrics`` synchronises the host: the reference's
``torch.nonzero`` / ``.tolist()`` / per-row boolean-mask indexing and ``max_d.item()`` are gone, the totals stay on
the device until ``_after_epoch`` / ``get_stats``.

Declared deviations (README "Deviations"):
  * the counts are exact int64 (``total_*``, ``completion_*``, ``tps`` / ``fps`` / ``fns`` are float32 views of them);
    the reference's float32 buffers round once a total passes 2^24;
  * ``get_stats`` / ``_after_epoch`` all-reduce only when torch.distributed is initialised (the reference needs a
    process group);
  * a frame without an occupied ground-truth voxel gives ``d_range = (-1, -1)`` (the reference's ``.max()`` raises).
"""
import logging

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import abi
from ._lib import lib, check, ptr, current_stream, upload
from .occ import OPENSEED2NUSCENES

logger = logging.getLogger('selfocc')

CITYSCAPES2SEMANTICKITTI = [9, 11, 13, 13, 14, 18, 19, 19, 15, 17, 0, 6, 7, 1, 4, 5, 5, 3, 2]
# pred_occ[..., 28:], [-6:, ...], [:, :6, :], [:, -6:, :] = 0 (eval_iou_kitti.py:181-185) at 256 x 256 x 32, as
# {lo_h, hi_h, lo_w, hi_w, lo_d, hi_d}: index i_k outside [lo_k, n_k - hi_k) is not occupied
KITTI_CROP = (0, 6, 6, 6, 0, 4)

_DTYPES = {torch.float32: abi.LBL_F32, torch.uint8: abi.LBL_U8, torch.bool: abi.LBL_U8, torch.int32: abi.LBL_I32,
           torch.int64: abi.LBL_I64}
_INT_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.int64)
_TABLES = {}     # (values, device, dtype) -> device tensor: uploaded once, not once per call
_WS = {}         # (device, stream) -> the self-resetting d_range scratch of selfocc_ssc_metric


def _need_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")


def _table(values, device, dtype):
    key = (tuple(int(v) for v in values), str(device), dtype)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = upload(np.asarray(key[0], dtype=np.int64), device, dtype)
    return t


def _lut_apply(values, sem):
    shape = sem.shape
    return _table(values, sem.device, sem.dtype)[sem.flatten()].reshape(*shape)


def cityscapes2semantickitti(sem):
    """Drop-in for utils/metric_util.py:9-32; the table is uploaded once per device and dtype."""
    return _lut_apply(CITYSCAPES2SEMANTICKITTI, sem)


def openseed2nuscenes(sem):
    """Drop-in for utils/metric_util.py:34-64; the table is uploaded once per device and dtype."""
    return _lut_apply(OPENSEED2NUSCENES, sem)


def _ws(device):
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    t = _WS.get(key)
    if t is None:      # zero once (a copy, not a kernel); every call leaves it zero again
        t = _WS[key] = upload(np.zeros(4, dtype=np.int32), device, torch.int32)
    return t


def _labels(t, what, int_only=False):
    """contiguous tensor + its SO_LBL_* code; bool is read as its bytes"""
    _need_cuda(t, what)
    if t.dtype not in _DTYPES or (int_only and t.dtype not in _INT_DTYPES):
        ok = _INT_DTYPES if int_only else tuple(_DTYPES)
        raise TypeError(f"{what}: dtype {t.dtype} not supported ({', '.join(map(str, ok))})")
    code = _DTYPES[t.dtype]
    t = t.contiguous()
    return (t.view(torch.uint8) if t.dtype == torch.bool else t), code


def _mask(m, n, what):
    if m is None:
        return None
    _need_cuda(m, what)
    if m.numel() != n:
        raise ValueError(f"{what} has {m.numel()} elements, the volume {n}")
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    if m.dtype == torch.uint8:
        return m.contiguous()
    return (m == 1).contiguous().view(torch.uint8)     # the reference selects ``mask == 1``


def _args(shape, pred=None, gt=None):
    a = abi.SoSscMetricArgs()
    a.H, a.W, a.D = shape
    a.iou_ignore = -1
    keep = []
    if pred is not None:
        p, a.pred_dtype = _labels(pred, "prediction", int_only=True)
        a.pred = ptr(p)
        keep.append(p)
    if gt is not None:
        g, a.gt_dtype = _labels(gt, "label")
        a.gt = ptr(g)
        keep.append(g)
    return a, keep


def _flat(n):
    if n >= 2 ** 31:
        raise ValueError(f"{n} voxels: the metric kernels take fewer than 2^31")
    return (1, 1, n)


def _launch(a, device, what='selfocc_ssc_metric'):
    fn = lib().selfocc_iou_coords if what == 'selfocc_iou_coords' else lib().selfocc_ssc_metric
    check(fn(a, current_stream(device)), what)


def _same_numel(x, y, what):
    if x.numel() != y.numel():
        raise ValueError(f"{what}: prediction has {x.numel()} elements, label {y.numel()}")


class IoU(nn.Module):
    """Same constructor, attributes and methods as the reference's IoU (utils/metric_util.py:168-233).
    ``_after_step`` also takes a dense label volume of the outputs' shape (occupied = label not in {0, 255}, what the
    script's ``nonzero`` of the 255-cleared labels lists).  One launch per step, no host synchronisation."""

    def __init__(self, use_mask=False):
        super().__init__()
        self.class_indices = [0]
        self.num_classes = 1
        self.label_str = ['occupied']
        self.use_mask = use_mask
        xx = torch.linspace(-40.0, 40.0, 200)
        yy = torch.linspace(-40.0, 40.0, 200)
        zz = torch.linspace(-1.0, 5.4, 16)
        xyz = torch.stack([
            xx[:, None, None].expand(-1, 200, 16),
            yy[None, :, None].expand(200, -1, 16),
            zz[None, None, :].expand(200, 200, -1)
        ], dim=-1)
        self.register_buffer('xyz', xyz, persistent=False)

    def reset(self):
        dev = torch.device("cuda", torch.cuda.current_device())
        self.counts = torch.zeros(3, dtype=torch.int64, device=dev)      # seen, correct, positive
        self.bad = torch.zeros(1, dtype=torch.int64, device=dev)         # out-of-range rows / sem indices

    @property
    def total_seen(self):
        return self.counts[0:1].float()

    @property
    def total_correct(self):
        return self.counts[1:2].float()

    @property
    def total_positive(self):
        return self.counts[2:3].float()

    def _after_step(self, outputs, targets, occ3d=False):
        if occ3d:
            self._after_step_occ3d(outputs, targets)
            return
        _need_cuda(outputs, "IoU")
        if torch.is_tensor(targets) and targets.shape == outputs.shape:
            if outputs.numel() == 0:
                return
            a, keep = _args(_flat(outputs.numel()), outputs, targets)
            a.iou_empty, a.iou_ignore = 0, 255
            a.iou = ptr(self.counts)
            _launch(a, outputs.device)
            return
        _need_cuda(targets, "IoU coordinates")
        if outputs.dim() != 3 or targets.dim() != 2 or targets.shape[1] != 3:
            raise ValueError(f"IoU: outputs (H, W, D) with targets (N, 3) coordinates or a label volume of the same "
                             f"shape, got {tuple(outputs.shape)} and {tuple(targets.shape)}")
        if outputs.numel() >= 2 ** 31 or targets.shape[0] >= 2 ** 31:
            raise ValueError("IoU: fewer than 2^31 voxels and rows")
        a, keep = _args(tuple(outputs.shape), outputs)
        coords = targets.to(torch.int64).contiguous()
        a.coords, a.n_coords = ptr(coords), coords.shape[0]
        a.iou, a.bad = ptr(self.counts), ptr(self.bad)
        _launch(a, outputs.device, 'selfocc_iou_coords')

    def _after_step_occ3d(self, outputs, targets):
        _need_cuda(outputs, "IoU")
        dev = outputs.device
        label = upload(targets['semantics'], dev)
        _same_numel(outputs, label, "IoU occ3d")
        if label.numel() == 0:
            return
        a, keep = _args(_flat(outputs.numel()), outputs, label)
        a.iou_empty, a.iou_ignore = 17, -1
        if self.use_mask:
            mask = _mask(upload(targets['mask_camera'], dev).bool(), label.numel(), "mask_camera")
            a.iou_mask = ptr(mask)
            keep.append(mask)
        a.iou = ptr(self.counts)
        _launch(a, dev)

    def _after_epoch(self):
        if dist.is_initialized():
            dist.all_reduce(self.counts)      # RCCL; integer sums are exact
            dist.all_reduce(self.bad)
        bad = int(self.bad.item())
        if bad:
            raise IndexError(f"IoU: {bad} coordinate rows (or sem indices) out of range since the last reset()")
        seen, correct, positive = self.counts.cpu().float().split(1)      # the reference's float32 arithmetic
        ious = []
        for i in range(self.num_classes):
            if seen[i] == 0:
                ious.append(1)
            else:
                ious.append((correct[i] / (seen[i] + positive[i] - correct[i])).item())
        miou = np.mean(ious)
        logger.info('Validation per class iou:')
        for iou, label_str in zip(ious, self.label_str):
            logger.info('%s : %.2f%%' % (label_str, iou * 100))
        logger.info(f'Final iou: {miou * 100}')
        return miou * 100


class SSCMetrics:
    """Same constructor, attributes and methods as the reference's SSCMetrics (utils/scenerf_metric.py:43-188).
    ``add_batch`` is one launch without a host synchronisation; the counts are exact int64 on the device."""

    def __init__(self, n_classes):
        self.n_classes = n_classes
        self.reset()

    def hist_info(self, n_cl, pred, gt):
        """(n_cl, n_cl) confusion histogram (rows: gt) of the labels in [0, n_cl), their correct and labelled counts"""
        assert pred.shape == gt.shape
        k = (gt >= 0) & (gt < n_cl)
        g, p = gt[k].astype(np.int64), pred[k].astype(np.int64)
        hist = np.zeros((n_cl, n_cl), dtype=np.int64)
        np.add.at(hist, (g, p), 1)
        return hist, int(np.count_nonzero(p == g)), int(np.count_nonzero(k))

    @staticmethod
    def compute_score(hist, correct, labeled):
        """per-class IoU, its mean with and without class 0, and the pixel accuracy of a confusion histogram"""
        tp = np.diag(hist)
        with np.errstate(divide='ignore', invalid='ignore'):
            iu = tp / (hist.sum(1) + hist.sum(0) - tp)
        mean_iu = np.nanmean(iu)
        mean_iu_no_back = np.nanmean(iu[1:])
        pixel_acc = correct / labeled if labeled != 0 else 0
        return iu, mean_iu, mean_iu_no_back, pixel_acc

    def reset(self):
        dev = torch.device("cuda", torch.cuda.current_device())
        self._counts = torch.zeros(3 + 3 * self.n_classes, dtype=torch.int64, device=dev)

    @property
    def completion_tp(self):
        return self._counts[0:1].float()

    @property
    def completion_fp(self):
        return self._counts[1:2].float()

    @property
    def completion_fn(self):
        return self._counts[2:3].float()

    @property
    def tps(self):
        return self._counts[3:3 + self.n_classes].float()

    @property
    def fps(self):
        return self._counts[3 + self.n_classes:3 + 2 * self.n_classes].float()

    @property
    def fns(self):
        return self._counts[3 + 2 * self.n_classes:].float()

    def _count(self, y_pred, y_true, nonempty, nonsurface, completion, semantic, keep255):
        _need_cuda(y_pred, "SSCMetrics")
        _same_numel(y_pred, y_true, "SSCMetrics")
        n = y_true.numel()
        if n == 0:
            return
        a, keep = _args(_flat(n), y_pred, y_true)
        ne, ns = _mask(nonempty, n, "nonempty"), _mask(nonsurface, n, "nonsurface")
        a.nonempty, a.nonsurface = ptr(ne), ptr(ns)
        a.n_classes, a.ssc_keep255 = self.n_classes, int(keep255)
        a.completion, a.semantic = ptr(completion), ptr(semantic)
        _launch(a, y_pred.device)

    def add_batch(self, y_pred, y_true, nonempty=None, nonsurface=None):
        c = self._counts
        self._count(y_pred, y_true, nonempty, nonsurface, c[0:3], c[3:], keep255=False)

    def get_score_completion(self, predict, target, nonempty=None):
        """(tp, fp, fn) 0-d int64 tensors of (target > 0, predict > 0); target == 255 counts as (0, 0)"""
        out = torch.zeros(3, dtype=torch.int64, device=predict.device)
        self._count(predict, target, nonempty, None, out, None, keep255=True)
        return out[0], out[1], out[2]

    def get_score_semantic_and_completion(self, predict, target, nonempty=None):
        """(tp, fp, fn) int32 (n_classes,) tensors; target == 255 counts as (0, 0)"""
        out = torch.zeros(3 * self.n_classes, dtype=torch.int64, device=predict.device)
        self._count(predict, target, nonempty, None, None, out, keep255=True)
        out = out.to(torch.int32).view(3, self.n_classes)
        return out[0], out[1], out[2]

    def get_stats(self):
        if dist.is_initialized():
            dist.all_reduce(self._counts)     # RCCL; integer sums are exact
        dev = self._counts.device
        c = self._counts.cpu().float()        # the reference's float32 arithmetic on the exact counts
        C = self.n_classes
        tp, fp, fn = c[0:1], c[1:2], c[2:3]
        if tp != 0:
            precision = (tp / (tp + fp)).to(dev)
            recall = (tp / (tp + fn)).to(dev)
            iou = (tp / (tp + fp + fn)).to(dev)
        else:
            precision, recall, iou = 0, 0, 0
        tps, fps, fns = c[3:3 + C], c[3 + C:3 + 2 * C], c[3 + 2 * C:]
        iou_ssc = tps / (tps + fps + fns + 1e-5)
        return {
            "precision": precision,
            "recall": recall,
            "iou": iou,
            "iou_ssc": iou_ssc.to(dev),
            "iou_ssc_mean": torch.mean(iou_ssc[1:]).to(dev),
        }


def _miou_map(miou, device):
    cls = list(miou.class_indices)
    if len(set(cls)) != len(cls) or any(not 0 <= c < 256 for c in cls):
        raise ValueError(f"kitti_occ_metrics: MeanIoU class_indices must be distinct and in [0, 256), got {cls}")
    m = [-1] * 256
    for k, c in enumerate(cls):
        m[c] = k
    return _table(m, device, torch.int32)


def kitti_occ_metrics(sdf, gt_label, *, iou=None, ssc=None, miou=None, sem=None, thresh=0.0, crop=KITTI_CROP,
                      flip_gt=True, lut=CITYSCAPES2SEMANTICKITTI, want_occ=False):
    """eval_iou_kitti.py:166-190 after ``forward_occ`` in one launch, without a host synchronisation:
        pred_occ = (sdf <= thresh) with the crops; gt = flip(gt_label, [1]) (flip_gt);
        iou._after_step(pred_occ, nonzero(gt with 255 -> 0)); ssc.add_batch(pred_occ, gt);
        miou._after_step(pred_occ * lut[sem], gt, gt != 255)       (miou a MeanIoU, needs sem);
    sdf (H, W, D) float32; gt_label (H, W, D) float32 / uint8 / int32 / int64 tensor or numpy array (uploaded
    without a sync) as read_semantic_kitti returns it.  Returns {'d_range': (min_d, max_d) int32 device tensor over
    the occupied labels, (-1, -1) for none} and 'occ' (int32 pred_occ) with want_occ.  A sem index outside lut counts
    into iou.bad (IoU._after_epoch raises)."""
    _need_cuda(sdf, "kitti_occ_metrics (sdf)")
    dev = sdf.device
    if sdf.dim() != 3 or sdf.dtype != torch.float32 or sdf.numel() == 0:
        raise ValueError(f"sdf must be a non-empty (H, W, D) float32 volume, got {tuple(sdf.shape)} {sdf.dtype}")
    if isinstance(gt_label, np.ndarray):
        gt_label = upload(gt_label, dev)
    if tuple(gt_label.shape) != tuple(sdf.shape):
        raise ValueError(f"gt_label {tuple(gt_label.shape)} must have the sdf's shape {tuple(sdf.shape)}")
    a, keep = _args(tuple(sdf.shape), None, gt_label)
    s = sdf.contiguous()
    keep.append(s)
    a.sdf, a.thresh = ptr(s), float(thresh)
    for k in range(6):
        a.crop[k] = int(crop[k])
    a.flip_gt = int(bool(flip_gt))
    out = {'d_range': torch.empty(2, dtype=torch.int32, device=dev)}
    a.d_range, a.ws = ptr(out['d_range']), ptr(_ws(dev))
    if want_occ:
        out['occ'] = torch.empty(sdf.shape, dtype=torch.int32, device=dev)
        a.occ = ptr(out['occ'])
    if iou is not None:
        a.iou_empty, a.iou_ignore = 0, 255
        a.iou, a.bad = ptr(iou.counts), ptr(iou.bad)
    if ssc is not None:
        a.n_classes = ssc.n_classes
        a.completion, a.semantic = ptr(ssc._counts[0:3]), ptr(ssc._counts[3:])
    if miou is not None:
        if sem is None:
            raise ValueError("kitti_occ_metrics: miou needs sem")
        _need_cuda(sem, "kitti_occ_metrics (sem)")
        if sem.numel() != sdf.numel():
            raise ValueError(f"sem has {sem.numel()} elements, the volume {sdf.numel()}")
        sem_t = sem.to(torch.int64).contiguous()
        lut_t = lut.to(device=dev, dtype=torch.int32) if torch.is_tensor(lut) else _table(lut, dev, torch.int32)
        map_t = _miou_map(miou, dev)
        keep += [sem_t, lut_t, map_t]
        a.sem, a.lut, a.n_lut, a.miou_map = ptr(sem_t), ptr(lut_t), lut_t.numel(), ptr(map_t)
        a.n_miou, a.miou_empty = miou.num_classes, int(miou.empty_label)
        a.miou = ptr(miou.counts)
    _launch(a, dev)
    return out
