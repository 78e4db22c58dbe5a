"""CameraAwareSE of the TPV encoder  <- model/encoder/tpvformer/modules/camera_se_net.py, call site tpvformer_encoder.py:60-67, 258-259.

A squeeze-and-excitation gate computed from the cameras' calibration (4 intrinsic + 12 cam2ego numbers per camera ->
BatchNorm1d -> two-layer MLP -> sigmoid) scales the channels of every FPN map, then a 1x1 convolution mixes them.  Parameter
and buffer names are the reference's, so its state dicts load with strict=True.

Two routes:
  forward(ms_img_feats, metas)                         the reference's list of (B, N, C, h, w) maps, torch ops
  flatten(ms_img_feats, metas, cams_embeds, level_embeds)
      the encoder's `value` (N, sum hw, B, C) directly.  The gate multiplies input channels and the embeddings add to
      output channels, so both fold into the 1x1 convolution: one HIP launch reads the maps once and writes `value`
      once (csrc/camera_se.hip); the backward is two products over the same data.  The gate itself (B*N x M numbers)
      and the folds of its gradient stay torch ops.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..._lib import upload

# env SELFOCC_CAMERA_SE_HIP=0: always the torch composition (kernel A/B runs)
CAMERA_SE_HIP = os.environ.get('SELFOCC_CAMERA_SE_HIP', '1') == '1'

_CAM_CACHE = {}


def _camera_numbers(metas, like):
    """(B*N, 16) float32 on like.device: K00, K11, K02, K12 of metas[b]['intrinsic'][n] (3x3 or 4x4), then the 12 entries
    of metas[b]['cam2ego'][n][:3, :].  Uploaded without a stream sync and kept per frame, keyed on the contents."""
    rows = []
    for b, meta in enumerate(metas):
        for key in ('intrinsic', 'cam2ego'):
            if key not in meta:
                raise KeyError(f"camera_aware=True reads metas[{b}]['{key}'] (per camera: 'intrinsic' 3x3 or 4x4, 'cam2ego' "
                               f"4x4); this frame's metas carry {sorted(k for k in meta if isinstance(k, str))}")
        K = np.asarray([np.asarray(k, dtype=np.float64) for k in meta['intrinsic']])
        E = np.asarray([np.asarray(e, dtype=np.float64) for e in meta['cam2ego']])
        if K.ndim != 3 or K.shape[1] < 3 or K.shape[2] < 3 or E.ndim != 3 or E.shape[0] != K.shape[0] or E.shape[1] < 3 or E.shape[2] != 4:
            raise ValueError(f"metas[{b}]: 'intrinsic' {K.shape} must be (N, 3|4, 3|4) and 'cam2ego' {E.shape} (N, 4, 4)")
        rows.append(np.concatenate([np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], -1), E[:, :3, :].reshape(len(E), 12)], -1))
    arr = np.ascontiguousarray(np.stack(rows).astype(np.float32))              # (B, N, 16)
    ck = (arr.shape, arr.tobytes(), str(like.device))
    hit = _CAM_CACHE.get(ck)
    if hit is None:
        hit = upload(arr.reshape(-1, 16), like.device, torch.float32)
        _CAM_CACHE.clear()                                                    # one frame at a time
        _CAM_CACHE[ck] = hit
    return hit, arr.shape[0], arr.shape[1]


class _Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, out_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(F.relu(self.fc1(x)))


def _aligned(t):
    """contiguous float32 storage on a 16-byte boundary (the kernels load and store 16 bytes at a time)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def fused_supported(feats, gate, weight, cams_embeds, level_embeds):
    f0 = feats[0]
    if not (CAMERA_SE_HIP and f0.is_cuda and not torch.is_autocast_enabled() and 1 <= len(feats) <= 8):
        return False
    if not all(f.dtype == torch.float32 and f.dim() == 5 and f.shape[:3] == f0.shape[:3] and f.shape[3] * f.shape[4] >= 1 for f in feats):
        return False
    if not all(t.dtype == torch.float32 and t.device == f0.device for t in (gate, weight, cams_embeds, level_embeds)):
        return False
    B, N, M = f0.shape[:3]
    Cc = weight.shape[0]
    if cams_embeds.shape != (N, Cc) or level_embeds.shape[0] < len(feats) or level_embeds.shape[1] != Cc:
        return False
    from ..._lib import lib
    return lib().selfocc_camera_se_supported(B, N, Cc, M, len(feats)) == 1


class _CameraSeFlatten(torch.autograd.Function):
    """value = fold(gate, context_conv, embeddings) applied to the maps: selfocc_camera_se_flatten_fwd / _bwd."""

    @staticmethod
    def forward(ctx, gate, weight, bias, cams_embeds, level_embeds, *feats):
        from ..._lib import lib, check, ptr, current_stream
        f0 = feats[0]
        B, N, M = f0.shape[:3]
        Cc = weight.shape[0]
        xs = [_aligned(f.detach()) for f in feats]
        hw = [f.shape[3] * f.shape[4] for f in xs]
        gate_c, w_c = gate.detach().contiguous(), weight.detach().reshape(Cc, M).contiguous()
        out = f0.new_empty(N, sum(hw), B, Cc)
        check(lib().selfocc_camera_se_flatten_fwd(_ptr_array(xs), (C.c_int32 * len(hw))(*hw), len(xs), B, N, Cc, M, ptr(gate_c),
                                                  ptr(w_c), ptr(bias.detach().contiguous()), ptr(cams_embeds.detach().contiguous()),
                                                  ptr(level_embeds.detach().contiguous()), ptr(out), current_stream(f0.device)),
              "selfocc_camera_se_flatten_fwd")
        ctx.save_for_backward(gate_c, w_c, *xs)
        ctx.shapes = [tuple(f.shape) for f in feats]
        ctx.n_level_rows = level_embeds.shape[0]
        ctx.w_shape = tuple(weight.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from ..._lib import lib, check, ptr, current_stream
        gate, w, *xs = ctx.saved_tensors
        B, N, M = ctx.shapes[0][:3]
        Cc, L = w.shape[0], len(xs)
        g = _aligned(g.float())
        hw_l = [s[3] * s[4] for s in ctx.shapes]
        hw = (C.c_int32 * L)(*hw_l)
        dxs = [torch.empty(s, device=g.device, dtype=torch.float32) if ctx.needs_input_grad[5 + i] else None
               for i, s in enumerate(ctx.shapes)]
        dwc = torch.empty(B * N, Cc, M, device=g.device, dtype=torch.float32)
        colsum = torch.empty(L, N, Cc, device=g.device, dtype=torch.float32)
        ws_bytes = lib().selfocc_camera_se_flatten_bwd_workspace(hw, L, B, N, Cc, M)
        ws = torch.empty(ws_bytes, device=g.device, dtype=torch.uint8)
        check(lib().selfocc_camera_se_flatten_bwd(ptr(g), _ptr_array(xs), hw, L, B, N, Cc, M, ptr(gate), ptr(w), _ptr_array(dxs),
                                                  ptr(dwc), ptr(colsum), ptr(ws), ws_bytes, current_stream(g.device)),
              "selfocc_camera_se_flatten_bwd")
        need = ctx.needs_input_grad
        g_gate = (dwc * w).sum(1) if need[0] else None                              # (B*N, M)
        g_w = (dwc * gate[:, None, :]).sum(0).reshape(ctx.w_shape) if need[1] else None
        g_bias = colsum.sum((0, 1)) if need[2] else None
        g_cam = colsum.sum(0) if need[3] else None
        g_lvl = None
        if need[4]:
            g_lvl = colsum.new_zeros(ctx.n_level_rows, Cc)        # rows beyond the maps handed in keep a zero gradient
            g_lvl[:L] = colsum.sum(1)
        return (g_gate, g_w, g_bias, g_cam, g_lvl, *dxs)


class CameraAwareSE(nn.Module):
    def __init__(self, in_channels=96, mid_channels=192, out_channles=96):
        super().__init__()
        self.in_channels, self.mid_channels, self.out_channels = in_channels, mid_channels, out_channles
        self.bn = nn.BatchNorm1d(16)
        self.context_mlp = _Mlp(16, mid_channels, mid_channels)
        self.context_conv = nn.Conv2d(mid_channels, out_channles, kernel_size=1)
        if in_channels == mid_channels:
            self.reduce_conv = nn.Identity()
        else:
            self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, kernel_size=3, padding=1),
                                             nn.BatchNorm2d(mid_channels), nn.ReLU(inplace=True))

    def init_weight(self):
        """The gate starts (almost) open: sigmoid(10) for every camera and channel."""
        nn.init.zeros_(self.context_mlp.fc2.weight)
        nn.init.constant_(self.context_mlp.fc2.bias, 10.0)

    def gate(self, metas, like):
        """(B*N, M) gate of this frame's cameras, and (B, N)."""
        nums, B, N = _camera_numbers(metas, like)
        return torch.sigmoid(self.context_mlp(self.bn(nums.to(like.dtype)))), B, N

    def _reduced(self, ms_img_feats):
        return [self.reduce_conv(f.flatten(0, 1)).unflatten(0, f.shape[:2]) for f in ms_img_feats]

    def _compose(self, feats, gate, B, N):
        outs = []
        for x in feats:
            y = self.context_conv(x.flatten(0, 1) * gate[:, :, None, None].to(x.dtype))
            outs.append(y.unflatten(0, (B, N)))
        return outs

    def forward(self, ms_img_feats, metas):
        gate, B, N = self.gate(metas, ms_img_feats[0])
        return self._compose(self._reduced(ms_img_feats), gate, B, N)

    def flatten_torch(self, ms_img_feats, metas, cams_embeds, level_embeds):
        """The reference's composition: forward(), then the encoder's flatten in torch ops."""
        from .tpvformer import _flatten_feats_torch
        return _flatten_feats_torch(cams_embeds, level_embeds, self.forward(ms_img_feats, metas))

    def flatten(self, ms_img_feats, metas, cams_embeds, level_embeds):
        """The encoder's `value` (N, sum hw, B, C): value[n, start_l + p, b] = context_conv(gate * x_l)[b, n, :, p] +
        cams_embeds[n] + level_embeds[l].  One fused HIP pass on the shapes selfocc_camera_se_supported covers (float32,
        GPU, no autocast); the torch composition everywhere else."""
        f0 = ms_img_feats[0]
        if not (CAMERA_SE_HIP and f0.is_cuda and not torch.is_autocast_enabled()):
            return self.flatten_torch(ms_img_feats, metas, cams_embeds, level_embeds)
        gate, B, N = self.gate(metas, f0)                  # once: a training-mode BatchNorm1d updates its buffers here
        feats = self._reduced(ms_img_feats)
        w, b = self.context_conv.weight, self.context_conv.bias
        if not fused_supported(feats, gate, w, cams_embeds, level_embeds):
            from .tpvformer import _flatten_feats_torch
            return _flatten_feats_torch(cams_embeds, level_embeds, self._compose(feats, gate, B, N))
        return _CameraSeFlatten.apply(gate, w, b, cams_embeds, level_embeds, *feats)
