"""The torch-op form of the reference's per-sample reprojection lines (loss/reproj_loss_mono_multi_new_combine.py:108-201) for
one camera on images of ANY channel count: ``oracle.torch_port.reproj_sample_port`` with its 3 replaced by C = curr.shape[1]
(that port is fixed at three channels).  float32 inputs: the reference's arithmetic; float64 inputs: the same function (the two
eps clamps stay at float32's finfo), the high-precision reference of tests/test_reproj_dims_gpu.py.  It runs on the device of
its inputs: on the GPU it is the torch-op yardstick that scripts/bench_reproj_dims.py times.  Not a test module."""
import torch
import torch.nn.functional as F

EPS32 = torch.finfo(torch.float32).eps


def reproj_sample_port_c(weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next, img_h, img_w):
    """weights, ts, deltas (R, S); pix (R, 2); curr (R, C); T_* (4, 4); img_* (C, Hi, Wi) -> l1 (R), combine (R, C), any_valid (R)"""
    R, S = weights.shape
    C = curr.shape[1]
    dev = weights.device
    ray_idx = torch.arange(R, device=dev).unsqueeze(-1).repeat(1, S).flatten()
    weight, t = weights.flatten(), ts.flatten()
    rays = pix[ray_idx]
    if deltas is not None:
        delta = deltas.flatten().detach()
        weight = weight.clone()
        weight[delta < EPS32] = 0.
        weight = weight / delta.clamp_min(EPS32)
    pixel_coords = torch.ones((1, 1, len(rays), 4), dtype=weights.dtype, device=dev)
    pixel_coords[..., :2] = rays.reshape(1, 1, -1, 2)
    pixel_coords[..., :3] *= t.reshape(1, 1, -1, 1)
    pixel_coords = pixel_coords.unsqueeze(-1)

    def cal_pixel(trans, coords):
        pixel = torch.matmul(trans.reshape(1, 1, 1, 4, 4), coords).squeeze(-1)
        mask = pixel[..., 2] > 0
        pixel = pixel[..., :2] / torch.maximum(torch.ones_like(pixel[..., :1]) * 1e-5, pixel[..., 2:3])
        mask = mask & (pixel[..., 0] > 0) & (pixel[..., 0] < img_w) & (pixel[..., 1] > 0) & (pixel[..., 1] < img_h)
        return pixel, mask

    def sample_pixel(pixel, img):
        pixel = pixel.clone()
        pixel[..., 0] /= img_w
        pixel[..., 1] /= img_h
        pixel = 2 * pixel - 1
        val = F.grid_sample(img[None], pixel, mode='bilinear', padding_mode='border', align_corners=True)
        return val.reshape(1, 1, C, val.shape[-1]).permute(0, 1, 3, 2)

    pixel_prev, prev_mask = cal_pixel(T_prev, pixel_coords)
    pixel_next, next_mask = cal_pixel(T_next, pixel_coords)
    val_prev = sample_pixel(pixel_prev, img_prev)
    val_next = sample_pixel(pixel_next, img_next)
    curr_ = curr[ray_idx].reshape(1, 1, -1, C)
    diff_prev = torch.mean(torch.abs(curr_ - val_prev), dim=-1)
    diff_next = torch.mean(torch.abs(curr_ - val_next), dim=-1)
    diff_prev[~prev_mask] = 0.
    diff_next[~next_mask] = 0.
    cnt = prev_mask.to(torch.float) + next_mask.to(torch.float)
    general_mask = cnt > 0
    cnt = torch.clamp(cnt, 1.0).to(weights.dtype)
    diff = (diff_prev + diff_next) / cnt
    weight = weight.clone()
    weight[~general_mask.flatten()] = 0.
    weight_sum = torch.zeros(R, dtype=weight.dtype, device=dev)
    weight_sum.index_add_(-1, ray_idx, weight)
    weight_sum = weight_sum.clamp_min(EPS32)
    weight = weight / torch.gather(weight_sum, -1, ray_idx)
    l1 = torch.zeros(R, dtype=diff.dtype, device=dev)
    l1 = l1.index_add(-1, ray_idx, weight * diff.flatten())
    val_prev = val_prev * prev_mask[..., None]
    val_next = val_next * next_mask[..., None]
    comb_ = (val_prev + val_next) / cnt.unsqueeze(-1)
    comb = torch.zeros(R, C, dtype=comb_.dtype, device=dev).index_add(0, ray_idx, comb_.reshape(-1, C) * weight.unsqueeze(-1))
    ray_filter = torch.zeros(R, dtype=weight.dtype, device=dev).index_add(0, ray_idx, general_mask.flatten().to(weight.dtype))
    return l1, comb, (ray_filter > 0).to(weights.dtype)
