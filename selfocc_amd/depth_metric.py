"""Host side of the depth-evaluation metric tail: DepthMetric (utils/metric_util.py:282-397) and the per-camera
``evaluate_depth`` -> ``compute_depth_errors_torch`` rows of the novel-depth scripts (metric_util.py:424-444,
eval_novel_depth.py:176-196).  One HIP launch per call (csrc/depth_metric.hip), no host synchronisation: the
reference's per-camera boolean-mask indexing (a ``nonzero()`` sync each) and ``torch.median`` calls are gone, the
totals stay on the device until ``_after_epoch``.

Declared deviation: a camera with no valid point gives NaN for its entries (its 'raw' scaling still counts 1, as in
the reference); the reference gives NaN for 'raw' too but raises inside ``torch.median`` for 'median' — raising would
need a host sync."""
import logging

import torch
import torch.distributed as dist
import torch.nn as nn

from . import abi
from ._lib import lib, check, ptr, current_stream

logger = logging.getLogger('selfocc')

METRICS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3')
EVAL_TYPES = ('raw', 'median')


def _need_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")


def _launch(depth_pred, depth_loc, depth_gt=None, depth_mask=None, *, acc=None, rows=(-1, -1), n_types=0,
            errors=None, sampled=None, medians=None):
    """Fill the ABI struct and launch selfocc_depth_metric on the current stream (no sync)."""
    for t, what in ((depth_pred, 'depth_pred'), (depth_loc, 'depth_loc'), (depth_gt, 'depth_gt'),
                    (depth_mask, 'depth_mask')):
        if t is not None:
            _need_cuda(t, f"DepthMetric ({what})")
    if depth_loc.dim() != 3 or depth_loc.shape[2] != 2:
        raise ValueError(f"depth_loc must be (N, n, 2), got {tuple(depth_loc.shape)}")
    N, n = depth_loc.shape[0], depth_loc.shape[1]
    if depth_pred.dim() != 3 or depth_pred.shape[0] != N:
        raise ValueError(f"depth_pred must be (N, h, w) with N = {N}, got {tuple(depth_pred.shape)}")
    pred = depth_pred.contiguous().float()
    loc = depth_loc.contiguous().float()
    a = abi.SoDepthMetricArgs()
    a.pred, a.loc = ptr(pred), ptr(loc)
    a.N, a.h, a.w, a.n = N, pred.shape[1], pred.shape[2], n
    a.n_types, a.raw_row, a.median_row = n_types, rows[0], rows[1]
    keep = [pred, loc]
    if depth_gt is not None:
        if tuple(depth_gt.shape) != (N, n) or tuple(depth_mask.shape) != (N, n):
            raise ValueError(f"depth_gt / depth_mask must be (N, n) = {(N, n)}, got "
                             f"{tuple(depth_gt.shape)} / {tuple(depth_mask.shape)}")
        if depth_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"depth_mask must be bool or uint8, got {depth_mask.dtype}")
        gt = depth_gt.contiguous().float()
        mask = depth_mask.contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)        # same bytes (0 / 1), no launch
        a.gt, a.mask = ptr(gt), ptr(mask)
        keep += [gt, mask]
    if acc is not None:
        for name in METRICS + ('scaling', 'count'):
            setattr(a, name, ptr(acc[name]))
    a.errors, a.sampled, a.medians = ptr(errors), ptr(sampled), ptr(medians)
    ws_bytes = lib().selfocc_depth_metric_ws_bytes(a)
    if ws_bytes:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pred.device)     # torch's caching allocator
        a.ws, a.ws_bytes = ptr(ws), ws_bytes
        keep.append(ws)
    check(lib().selfocc_depth_metric(a, current_stream(pred.device)), "selfocc_depth_metric")
    return keep


def sample_depth(depth_pred, depth_loc):
    """(N, n) = F.grid_sample(depth_pred (N, h, w)[:, None], depth_loc (N, n, 2)[:, None] * 2 - 1, 'bilinear',
    padding_mode='border', align_corners=True), bit-identical to torch's GPU kernel."""
    out = torch.empty(depth_loc.shape[0], depth_loc.shape[1], device=depth_loc.device)
    _launch(depth_pred, depth_loc, sampled=out)
    return out


def masked_medians(depth_pred, depth_loc, depth_gt, depth_mask):
    """(N, 2): per camera torch.median of depth_gt[mask] and of the sampled depth_pred[mask] (the lower median);
    NaN for a camera without a valid point."""
    out = torch.empty(depth_loc.shape[0], 2, device=depth_loc.device)
    _launch(depth_pred, depth_loc, depth_gt, depth_mask, medians=out)
    return out


def depth_errors(depth_pred, depth_loc, depth_gt, depth_mask):
    """(N, 7) rows (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3): ``compute_depth_errors_torch`` of each camera's
    masked gt against the sampled prediction — the drop-in for the per-camera ``evaluate_depth`` loop of
    eval_novel_depth.py:176-196 (``torch.stack`` of its rows).  depth_pred (N, h, w) or (N, 1, h, w)."""
    if depth_pred.dim() == 4:
        depth_pred = depth_pred.flatten(0, 1)
    out = torch.empty(depth_loc.shape[0], 7, device=depth_loc.device)
    _launch(depth_pred, depth_loc, depth_gt, depth_mask, errors=out)
    return out


class DepthMetric(nn.Module):
    """Same constructor, buffers (names, shapes, state_dict) and methods as the reference's DepthMetric
    (utils/metric_util.py:282-397); ``_after_step`` is one HIP launch without a host sync."""

    def __init__(self, camera_names=['front'], eval_types=['raw', 'median']):
        super().__init__()
        for t in eval_types:
            if t not in EVAL_TYPES:
                raise NotImplementedError(f"eval type {t!r}")
        if len(set(eval_types)) != len(eval_types):
            raise ValueError(f"repeated eval type in {eval_types}")
        self.num_cams = len(camera_names)
        self.camera_names = camera_names
        self.num_types = len(eval_types)
        self.eval_types = eval_types
        for name in METRICS:
            self.register_buffer(name, torch.zeros(self.num_types, self.num_cams))
        self.register_buffer('count', torch.zeros(1))
        self.register_buffer('scaling', torch.zeros(self.num_types, self.num_cams))

    def _reset(self):
        for name in METRICS + ('count', 'scaling'):
            getattr(self, name).zero_()

    def _rows(self):
        return tuple(self.eval_types.index(t) if t in self.eval_types else -1 for t in EVAL_TYPES)

    def _after_step(self, depth_loc, depth_gt, depth_mask, depth_pred):
        # depth_loc: N, n, 2; depth_gt: N, n; depth_mask: N, n (bool / uint8); depth_pred: N, h, w
        num_cams = depth_gt.shape[0]
        if num_cams != self.num_cams:
            raise ValueError(f"{num_cams} cameras in the frame, DepthMetric was built for {self.num_cams}")
        acc = {name: getattr(self, name) for name in METRICS + ('count', 'scaling')}
        for name, t in acc.items():
            _need_cuda(t, f"DepthMetric buffer {name} (call .cuda() on the module)")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError(f"DepthMetric buffer {name} must be contiguous float32")
        _launch(depth_pred, depth_loc, depth_gt, depth_mask, acc=acc, rows=self._rows(), n_types=self.num_types)

    def _after_epoch(self):
        if dist.is_initialized():
            dist.barrier()
            for name in ('count',) + METRICS + ('scaling',):
                dist.all_reduce(getattr(self, name))
            dist.barrier()
        count = self.count
        avg = {name: getattr(self, name) / count for name in METRICS + ('scaling',)}
        if not dist.is_initialized() or dist.get_rank() == 0:
            host = {k: v.cpu() for k, v in avg.items()}
            logger.info(f'Averaging over {count.item()} samples.')
            for type_idx, type_ in enumerate(self.eval_types):
                logger.info("{} evaluation:".format(type_))
                logger.info(("{:>12} | " * 9).format("cam_name", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2",
                                                     "a3", "scale"))
                for cam, cam_name in enumerate(self.camera_names):
                    logger.info((f"{cam_name:>12} | " + "&{: 12.3f}  " * 8).format(
                        *(float(host[k][type_idx, cam]) for k in METRICS + ('scaling',))) + "\\\\")
                logger.info(("{:>12} | " + "&{: 12.3f}  " * 8).format(
                    "All", *(float(host[k][type_idx].mean()) for k in METRICS + ('scaling',))) + "\\\\")
        return {t: {k: v[i].cpu() for k, v in avg.items()} for i, t in enumerate(self.eval_types)}
