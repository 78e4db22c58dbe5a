"""GPU: the depth-evaluation metric tail (selfocc_amd/depth_metric.py, csrc/depth_metric.hip) against torch's GPU
F.grid_sample / torch.median, the reference's own DepthMetric buffers (tests/golden/depth_metric.npz) and a torch
restatement of the reference loop; one launch per call and no host synchronisation."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'a1', 'a2', 'a3')


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def grid_sample(pred, loc):
    return F.grid_sample(pred.unsqueeze(1), loc.unsqueeze(1) * 2 - 1, mode='bilinear', padding_mode='border',
                         align_corners=True).reshape(loc.shape[0], loc.shape[1])


def cal_depth_metric(gt, p):
    """utils/metric_util.py:247-280 restated in torch (f32)"""
    p = torch.clamp(p, 1e-3, 80)
    th = torch.maximum(gt / p, p / gt)
    return torch.stack([(torch.abs(gt - p) / gt).mean(), (((gt - p) ** 2) / gt).mean(), ((gt - p) ** 2).mean() ** .5,
                        ((torch.log(gt) - torch.log(p)) ** 2).mean() ** .5, (th < 1.25).float().mean(),
                        (th < 1.25 ** 2).float().mean(), (th < 1.25 ** 3).float().mean()])


def reference_step(pred, loc, gt, mask):
    """the reference's per-camera loop (metric_util.py:311-349): rows (2 types, N, 8 = 7 metrics + scaling)"""
    p = grid_sample(pred, loc)
    out = torch.zeros(2, gt.shape[0], 8, dtype=torch.float32, device=gt.device)
    for c in range(gt.shape[0]):
        g, q = gt[c][mask[c]], p[c][mask[c]]
        out[0, c, :7], out[0, c, 7] = cal_depth_metric(g, q), 1.0
        scale = torch.median(g) / torch.median(q)
        out[1, c, :7], out[1, c, 7] = cal_depth_metric(g, scale * q), scale
    return out


def nuscenes_frame(seed):
    g = torch.Generator(device=D0).manual_seed(seed)
    N, h, w, n = 6, 450, 800, 34720
    pred = torch.rand(N, h, w, generator=g, device=D0) * 60 + 0.5
    loc = torch.rand(N, n, 2, generator=g, device=D0) * 1.1 - 0.05
    gt = torch.rand(N, n, generator=g, device=D0) * 60 + 0.5
    mask = torch.rand(N, n, generator=g, device=D0) < 0.15
    return pred, loc, gt, mask


def buffers(m):
    return torch.stack([getattr(m, k) for k in METRICS + ('scaling',)], -1)     # (types, N, 8)


def test_gather_is_bit_identical_to_torch_grid_sample(hip):
    from selfocc_amd.depth_metric import sample_depth
    g = torch.Generator(device=D0).manual_seed(1)
    for (N, h, w, n) in [(6, 45, 80, 3000), (2, 450, 800, 34720), (3, 7, 1, 500), (1, 1, 9, 300), (2, 33, 17, 1)]:
        pred = torch.randn(N, h, w, generator=g, device=D0) * 30
        loc = torch.rand(N, n, 2, generator=g, device=D0) * 1.4 - 0.2
        edges = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.5, 0.0], [0.0, 0.5], [1.0, 0.5],
                              [0.5, 1.0], [-3.0, 0.25], [7.0, 2.0], [1.0 - 2 ** -24, 2 ** -30], [-0.0, 1.0 + 2 ** -23]],
                             device=D0)
        k = min(n, len(edges))
        loc[:, :k] = edges[:k]
        torch.testing.assert_close(sample_depth(pred, loc), grid_sample(pred, loc), rtol=0, atol=0)


def test_medians_are_bit_identical_to_torch_median(hip):
    from selfocc_amd.depth_metric import masked_medians, sample_depth
    g = torch.Generator(device=D0).manual_seed(2)
    N, h, w, n = 6, 40, 64, 4001
    pred = torch.rand(N, h, w, generator=g, device=D0) * 40 + 0.1
    pred[2] = torch.floor(pred[2] / 10) * 10 + 1        # tied samples
    pred[4] = 7.25                                      # all samples equal
    pred[5] -= 20                                       # negative values: the key order across the sign
    loc = torch.rand(N, n, 2, generator=g, device=D0)
    gt = torch.rand(N, n, generator=g, device=D0) * 50 - 5
    gt[2] = torch.floor(gt[2] / 8) * 8                  # tied gt
    gt[4] = 3.5                                         # all equal
    mask = torch.rand(N, n, generator=g, device=D0) < 0.3
    mask[0] = False
    mask[0, :7] = True                                  # odd count
    mask[1] = False
    mask[1, 100:1100] = True                            # even count
    mask[3] = False
    mask[3, 4000] = True                                # one element
    got = masked_medians(pred, loc, gt, mask)
    p = sample_depth(pred, loc)
    for c in range(N):
        exp = torch.stack([torch.median(gt[c][mask[c]]), torch.median(p[c][mask[c]])])
        torch.testing.assert_close(got[c], exp, rtol=0, atol=0)


def test_three_steps_match_the_reference_buffers(hip):
    from selfocc_amd import DepthMetric, depth_errors
    G = np.load(os.path.join(HERE, "golden", "depth_metric.npz"))
    m = DepthMetric(camera_names=[f'cam{i}' for i in range(6)], eval_types=['raw', 'median']).cuda()
    for k in range(3):
        pred, loc, gt, mask = (torch.from_numpy(G[f'f{k}.{s}']).to(D0) for s in ('pred', 'loc', 'gt', 'mask'))
        m._after_step(loc, gt, mask, pred)
        torch.testing.assert_close(depth_errors(pred, loc, gt, mask).cpu(), torch.from_numpy(G[f'f{k}.errors']),
                                   rtol=1e-5, atol=1e-6)
    for name in ('abs_rel', 'sq_rel', 'rmse', 'rmse_log', 'scaling'):
        torch.testing.assert_close(getattr(m, name).cpu(), torch.from_numpy(G[name]), rtol=1e-5, atol=1e-6,
                                   msg=name)
    for name in ('a1', 'a2', 'a3', 'count'):
        assert torch.equal(getattr(m, name).cpu(), torch.from_numpy(G[name])), name


def test_nuscenes_frame_is_sync_free_and_matches_torch(hip):
    from selfocc_amd import DepthMetric, depth_errors
    m = DepthMetric(camera_names=[f'cam{i}' for i in range(6)]).cuda()
    m._after_step(*[nuscenes_frame(0)[i] for i in (1, 2, 3, 0)])       # warm-up (library load, allocator)
    depth_errors(*nuscenes_frame(0))
    m._reset()
    pred, loc, gt, mask = nuscenes_frame(1)
    with no_sync():
        m._after_step(loc, gt, mask, pred)
        rows = depth_errors(pred, loc, gt, mask.to(torch.uint8))
    ref = reference_step(pred, loc, gt, mask)
    torch.testing.assert_close(buffers(m), ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rows, ref[0, :, :7], rtol=1e-5, atol=1e-6)
    assert m.count.item() == 1


def test_camera_without_valid_point_gives_nan_for_that_camera_only(hip):
    from selfocc_amd import DepthMetric, depth_errors
    pred, loc, gt, mask = nuscenes_frame(3)
    full = DepthMetric(camera_names=[f'cam{i}' for i in range(6)]).cuda()
    full._after_step(loc, gt, mask, pred)
    empty = mask.clone()
    empty[2] = False
    m = DepthMetric(camera_names=[f'cam{i}' for i in range(6)]).cuda()
    m._after_step(loc, gt, empty, pred)
    rows = depth_errors(pred, loc, gt, empty)
    b, bf = buffers(m), buffers(full)
    others = [0, 1, 3, 4, 5]
    assert torch.equal(b[:, others], bf[:, others])
    assert torch.isnan(b[:, 2, :7]).all() and torch.isnan(b[1, 2, 7])
    assert b[0, 2, 7].item() == 1.0                      # 'raw' scaling counts 1, as in the reference
    assert torch.isnan(rows[2]).all() and not torch.isnan(rows[others]).any()
    assert m.count.item() == 1


def test_raw_only_skips_the_median_and_reset_zeroes(hip):
    from selfocc_amd import DepthMetric
    pred, loc, gt, mask = nuscenes_frame(4)
    both = DepthMetric(camera_names=[f'cam{i}' for i in range(6)], eval_types=['raw', 'median']).cuda()
    raw = DepthMetric(camera_names=[f'cam{i}' for i in range(6)], eval_types=['raw']).cuda()
    med_first = DepthMetric(camera_names=[f'cam{i}' for i in range(6)], eval_types=['median', 'raw']).cuda()
    for mod in (both, raw, med_first):
        mod._after_step(loc, gt, mask, pred)
    assert tuple(raw.abs_rel.shape) == (1, 6)
    assert torch.equal(buffers(raw)[0], buffers(both)[0])
    assert torch.equal(buffers(med_first), buffers(both).flip(0))
    both._reset()
    for k in METRICS + ('scaling', 'count'):
        assert not getattr(both, k).any(), k
