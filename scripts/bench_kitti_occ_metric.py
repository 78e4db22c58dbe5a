"""The occupancy metric tail of eval_iou_kitti.py (:166-190) at SemanticKITTI size (256 x 256 x 32):
selfocc_amd.kitti_occ_metrics (one HIP launch, no host sync) against a torch restatement of the reference's tail on the
GPU (threshold, flip, crops, nonzero, IoU._after_step with its .tolist() gather, SSCMetrics.add_batch with its 256-row
boolean-mask loops, max_d / min_d .item(); with --sem also cityscapes2semantickitti with its per-call table upload and
MeanIoU._after_step with its per-class .item() loop), restated from utils/metric_util.py and utils/scenerf_metric.py.

Median over --iters calls (cyclic GC collected before and held off) of the wall time of one frame's tail including the
drain of the stream, and of the device time of our launch (events).  Prints one JSON line.  Launch counts: run under
`rocprofv3 --kernel-trace --stats` with `--path ours|ref` and divide the dispatches by --warm + --iters.
    python scripts/bench_kitti_occ_metric.py [--iters 50] [--path both|ours|ref] [--sem]"""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--path", default="both", choices=["both", "ours", "ref"])
ap.add_argument("--sem", action="store_true")
args = ap.parse_args()
d = torch.device("cuda:0")
CITY = [9, 11, 13, 13, 14, 18, 19, 19, 15, 17, 0, 6, 7, 1, 4, 5, 5, 3, 2]


class RefIoU:
    def __init__(self):
        self.total_seen, self.total_correct, self.total_positive = (torch.zeros(1, device=d) for _ in range(3))

    def _after_step(self, outputs, targets):
        seen = targets.shape[0]
        correct = outputs[tuple(targets.transpose(0, 1).tolist())].sum()
        self.total_seen[0] += seen
        self.total_correct[0] += correct
        self.total_positive[0] += outputs.sum()


class RefSSC:
    def __init__(self, n):
        self.n = n
        self.ctp, self.cfp, self.cfn = (torch.zeros(1, device=d) for _ in range(3))
        self.tps, self.fps, self.fns = (torch.zeros(n, device=d) for _ in range(3))

    @staticmethod
    def completion(predict, target, nonempty):
        predict, target = predict.clone(), target.clone()
        predict[target == 255] = 0
        target[target == 255] = 0
        bs = predict.shape[0]
        target, predict = target.reshape(bs, -1), predict.reshape(bs, -1)
        b_pred, b_true = torch.zeros(predict.shape, device=d), torch.zeros(target.shape, device=d)
        b_pred[predict > 0] = 1
        b_true[target > 0] = 1
        tp_sum = fp_sum = fn_sum = 0
        for i in range(bs):
            m = nonempty[i, :].reshape(-1) == 1
            y_true, y_pred = b_true[i, :][m], b_pred[i, :][m]
            tp_sum += torch.logical_and(y_true == 1, y_pred == 1).sum()
            fp_sum += torch.logical_and(y_true != 1, y_pred == 1).sum()
            fn_sum += torch.logical_and(y_true == 1, y_pred != 1).sum()
        return tp_sum, fp_sum, fn_sum

    def semantic(self, predict, target, nonempty):
        predict, target = predict.clone(), target.clone()
        bs = predict.shape[0]
        predict[target == 255] = 0
        target[target == 255] = 0
        target, predict = target.reshape(bs, -1), predict.reshape(bs, -1)
        tp_sum, fp_sum, fn_sum = (torch.zeros(self.n, dtype=torch.int32, device=d) for _ in range(3))
        for i in range(bs):
            y_true, y_pred = target[i, :], predict[i, :]
            m = torch.logical_and(nonempty[i, :].reshape(-1) == 1, y_true != 255)
            y_pred, y_true = y_pred[m], y_true[m]
            for j in range(self.n):
                tp_sum[j] += torch.logical_and(y_true == j, y_pred == j).sum()
                fp_sum[j] += torch.logical_and(y_true != j, y_pred == j).sum()
                fn_sum[j] += torch.logical_and(y_true == j, y_pred != j).sum()
        return tp_sum, fp_sum, fn_sum

    def add_batch(self, y_pred, y_true):
        mask = y_true != 255
        tp, fp, fn = self.completion(y_pred, y_true, mask)
        self.ctp += tp
        self.cfp += fp
        self.cfn += fn
        tp, fp, fn = self.semantic(y_pred, y_true, mask)
        self.tps += tp
        self.fps += fp
        self.fns += fn


class RefMeanIoU:
    def __init__(self):
        self.cls = list(range(1, 20))
        self.total_seen, self.total_correct, self.total_positive = (torch.zeros(20, device=d) for _ in range(3))

    def _after_step(self, outputs, targets, mask):
        outputs, targets = outputs[mask], targets[mask]
        for i, c in enumerate(self.cls):
            self.total_seen[i] += torch.sum(targets == c).item()
            self.total_correct[i] += torch.sum((targets == c) & (outputs == c)).item()
            self.total_positive[i] += torch.sum(outputs == c).item()
        self.total_seen[-1] += torch.sum(targets != 0).item()
        self.total_correct[-1] += torch.sum((targets != 0) & (outputs != 0)).item()
        self.total_positive[-1] += torch.sum(outputs != 0).item()


def ref_tail(sdf, gt_np, sem, m):
    iou, ssc, miou = m
    pred_occ = (sdf <= 0.0).to(torch.int)
    gt_occ_raw = torch.flip(torch.from_numpy(gt_np).cuda(), [1])
    gt_occ = gt_occ_raw.clone()
    gt_occ[gt_occ == 255] = 0
    gt_occ = torch.nonzero(gt_occ)
    max_d, min_d = gt_occ[:, 2].max(), gt_occ[:, 2].min()
    pred_occ[..., 28:] = 0
    pred_occ[-6:, ...] = 0
    pred_occ[:, :6, :] = 0
    pred_occ[:, -6:, :] = 0
    iou._after_step(pred_occ, gt_occ)
    ssc.add_batch(pred_occ, gt_occ_raw.clone())
    if args.sem:
        lut = torch.tensor(CITY, dtype=sem.dtype, device=sem.device)       # the reference's per-call table
        miou._after_step(pred_occ * lut[sem.flatten()].reshape(sem.shape), gt_occ_raw, gt_occ_raw != 255)
    return max_d.item(), min_d.item()


def our_tail(sdf, gt_np, sem, m):
    from selfocc_amd import kitti_occ_metrics
    iou, ssc, miou = m
    gt = torch.from_numpy(gt_np).cuda()                                    # the script's own label upload
    return kitti_occ_metrics(sdf, gt, iou=iou, ssc=ssc, miou=miou if args.sem else None, sem=sem)


def median_wall(fn, *a):
    for _ in range(args.warm):
        fn(*a)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    ts = []
    try:
        for _ in range(args.iters):
            t0 = time.perf_counter()
            fn(*a)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    finally:
        gc.enable()
    return float(np.median(ts))


def main():
    g = torch.Generator(device=d).manual_seed(0)
    shape = (256, 256, 32)
    sdf = torch.randn(shape, generator=g, device=d)
    rng = np.random.default_rng(0)
    gt_np = rng.integers(0, 20, shape).astype(np.float32)
    gt_np[rng.random(shape) < 0.6] = 0
    gt_np[rng.random(shape) < 0.1] = 255
    sem = torch.randint(0, 19, shape, generator=g, device=d)
    res = dict(shape=list(shape), sem=args.sem, iters=args.iters)
    if args.path in ("both", "ref"):
        res['ref_ms'] = median_wall(ref_tail, sdf, gt_np, sem, (RefIoU(), RefSSC(2), RefMeanIoU()))
    if args.path in ("both", "ours"):
        from selfocc_amd import IoU, MeanIoU, SSCMetrics
        iou, ssc = IoU(), SSCMetrics(2)
        iou.reset()
        miou = MeanIoU(list(range(1, 20)), 0, [str(c) for c in range(1, 20)], True, 0)
        miou.reset()
        m = (iou, ssc, miou)
        res['ours_ms'] = median_wall(our_tail, sdf, gt_np, sem, m)
        gt = torch.from_numpy(gt_np).cuda()
        from selfocc_amd import kitti_occ_metrics
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        dev = []
        for _ in range(args.iters):
            ev[0].record()
            kitti_occ_metrics(sdf, gt, iou=iou, ssc=ssc, miou=miou if args.sem else None, sem=sem)
            ev[1].record()
            ev[1].synchronize()
            dev.append(ev[0].elapsed_time(ev[1]))
        res['ours_launch_ms'] = float(np.median(dev))
        res['ours_call_only_ms'] = median_wall(
            lambda: kitti_occ_metrics(sdf, gt, iou=iou, ssc=ssc, miou=miou if args.sem else None, sem=sem))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
