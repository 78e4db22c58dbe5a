"""Host side of the fused reprojection sampling (selfocc_reproj_fwd / _bwd): the
per-sample part of ReprojLossMonoMultiNewCombine.reproj_loss
(loss/reproj_loss_mono_multi_new_combine.py:108-201) for one camera, and of the arg-max pick of the mono loss's
``sdf_loss`` term (selfocc_reproj_pick_fwd / _bwd; loss/reproj_loss_mono_multi_new.py:265-270).  Images of a channel
count other than 3 (the losses' ``dims`` knob) go through selfocc_reproj_c_fwd / _bwd on channel-last images."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import abi
from ._lib import lib, check, ptr, current_stream


def _args(weights, ts, deltas, pix, curr_rgb, T_prev, T_next, img_prev, img_next, img_h, img_w):
    R, S = weights.shape
    a = abi.SoReprojArgs()
    a.weights, a.ts = ptr(weights), ptr(ts)
    a.deltas = ptr(deltas)
    a.pix, a.curr_rgb = ptr(pix), ptr(curr_rgb)
    a.T_prev, a.T_next = ptr(T_prev), ptr(T_next)
    a.img_prev, a.img_next = ptr(img_prev), ptr(img_next)
    a.R, a.S = R, S
    a.Hi, a.Wi = img_prev.shape[-2], img_prev.shape[-1]
    a.img_h, a.img_w = float(img_h), float(img_w)
    return a


class ReprojSampleFunction(Function):
    """(weights (R,S), ts (R,S), deltas (R,S)|None, pix (R,2), curr_rgb (R,3), T_prev (4,4),
    T_next (4,4), img_prev (3,Hi,Wi), img_next (3,Hi,Wi), img_h, img_w)
       -> l1 (R), rgb_combine (R,3), any_valid (R).   Differentiable wrt ``weights`` only
    (ts / pixels / matrices / images are constants of the loss in the reference too)."""

    @staticmethod
    def forward(ctx, weights, ts, deltas, pix, curr_rgb, T_prev, T_next, img_prev, img_next, img_h, img_w):
        if not weights.is_cuda:
            raise RuntimeError("ReprojSampleFunction needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")
        f = lambda t: None if t is None else t.detach().contiguous().float()
        tens = [f(t) for t in (weights, ts, deltas, pix, curr_rgb, T_prev, T_next, img_prev, img_next)]
        a = _args(*tens, img_h, img_w)
        R = tens[0].shape[0]
        dev = weights.device
        l1 = torch.empty(R, device=dev)
        comb = torch.empty(R, 3, device=dev)
        anyv = torch.empty(R, device=dev)
        a.l1, a.rgb_combine, a.any_valid = ptr(l1), ptr(comb), ptr(anyv)
        check(lib().selfocc_reproj_fwd(a, current_stream(dev)), "selfocc_reproj_fwd")
        # saved through autograd (version-counter checks, saved-tensor hooks): an in-place change of `weights`
        # between forward and backward is an error, not a silent mismatch
        ctx.has_deltas = tens[2] is not None
        ctx.save_for_backward(*[t for t in tens if t is not None])
        ctx.hw = (img_h, img_w)
        ctx.mark_non_differentiable(anyv)
        return l1, comb, anyv

    @staticmethod
    @once_differentiable
    def backward(ctx, g_l1, g_comb, _g_any):
        tens = list(ctx.saved_tensors)
        if not ctx.has_deltas:
            tens.insert(2, None)
        a = _args(*tens, *ctx.hw)
        g_l1 = g_l1.contiguous().float()
        g_comb = g_comb.contiguous().float()
        g_w = torch.zeros_like(tens[0])
        check(lib().selfocc_reproj_bwd(a, ptr(g_l1), ptr(g_comb), ptr(g_w), current_stream(g_w.device)),
              "selfocc_reproj_bwd")
        return (g_w,) + (None,) * 10


class ChannelLastImage:
    """One image for selfocc_reproj_c_*: ``data`` (Hi, Wi, stride) float32 contiguous, of which the first ``C`` channels of
    a pixel count and the rest is padding (stride % 4 == 0)."""

    def __init__(self, data, C):
        if data.dim() != 3 or data.dtype != torch.float32 or not data.is_contiguous() or data.shape[2] % 4 or not \
                1 <= C <= data.shape[2]:
            raise ValueError(f"ChannelLastImage: need a contiguous float32 (Hi, Wi, stride) tensor with stride % 4 == 0 and "
                             f"1 <= C <= stride, got {tuple(data.shape)} {data.dtype}, C = {C}")
        self.data, self.C = data, C


def channel_last(img):
    """(C, Hi, Wi) image of any strides -> ChannelLastImage with the pixel stride padded to a multiple of 4, in ONE copy.
    The padding stays uninitialised: the kernel's contract is that no output depends on it."""
    if isinstance(img, ChannelLastImage):
        return img
    C, Hi, Wi = img.shape
    data = torch.empty(Hi, Wi, (C + 3) // 4 * 4, device=img.device, dtype=torch.float32)
    data[..., :C].copy_(img.detach().permute(1, 2, 0))
    return ChannelLastImage(data, C)


def _args_c(weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next, C, img_h, img_w):
    a = abi.SoReprojCArgs()
    a.weights, a.ts, a.deltas = ptr(weights), ptr(ts), ptr(deltas)
    a.pix, a.curr = ptr(pix), ptr(curr)
    a.T_prev, a.T_next = ptr(T_prev), ptr(T_next)
    a.img_prev, a.img_next = ptr(img_prev), ptr(img_next)
    a.R, a.S = weights.shape
    a.Hi, a.Wi, a.img_stride = img_prev.shape
    a.C = C
    a.img_h, a.img_w = float(img_h), float(img_w)
    return a


class ReprojSampleCFunction(Function):
    """ReprojSampleFunction on images of C channels (selfocc_reproj_c_fwd / _bwd):
    (weights (R,S), ts (R,S), deltas (R,S)|None, pix (R,2), curr (R,C), T_prev (4,4), T_next (4,4), img_prev, img_next,
    img_h, img_w) -> l1 (R), combine (R,C), any_valid (R).  ``img_prev`` / ``img_next`` are ChannelLastImage (convert an
    image once with ``channel_last`` where it is sampled more than once) or tensors with (C, Hi, Wi) semantics of any layout,
    converted here.  Differentiable wrt ``weights`` only."""

    @staticmethod
    def forward(ctx, weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next, img_h, img_w):
        if not weights.is_cuda:
            raise RuntimeError("ReprojSampleCFunction needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")
        f = lambda t: None if t is None else t.detach().contiguous().float()
        weights, ts, deltas, pix, curr, T_prev, T_next = (f(t) for t in (weights, ts, deltas, pix, curr, T_prev, T_next))
        img_prev, img_next = channel_last(img_prev), channel_last(img_next)
        R, S = weights.shape
        C = img_prev.C
        if img_next.C != C or img_next.data.shape != img_prev.data.shape:
            raise ValueError(f"reproj_c: img_prev {tuple(img_prev.data.shape)} (C = {C}) and img_next "
                             f"{tuple(img_next.data.shape)} (C = {img_next.C}) differ")
        if curr.shape != (R, C) or pix.shape != (R, 2) or ts.shape != (R, S) or (deltas is not None and deltas.shape != (R, S)):
            raise ValueError(f"reproj_c: need curr (R, C) = {(R, C)}, pix (R, 2) and ts / deltas of the shape of weights "
                             f"{(R, S)}; got curr {tuple(curr.shape)}, pix {tuple(pix.shape)}, ts {tuple(ts.shape)}")
        if T_prev.numel() != 16 or T_next.numel() != 16:
            raise ValueError("reproj_c: the transforms must be (4, 4)")
        tens = [weights, ts, deltas, pix, curr, T_prev, T_next, img_prev.data, img_next.data]
        a = _args_c(*tens, C, img_h, img_w)
        dev = weights.device
        l1 = torch.empty(R, device=dev)
        comb = torch.empty(R, C, device=dev)
        anyv = torch.empty(R, device=dev)
        a.l1, a.combine, a.any_valid = ptr(l1), ptr(comb), ptr(anyv)
        check(lib().selfocc_reproj_c_fwd(a, current_stream(dev)), "selfocc_reproj_c_fwd")
        # saved through autograd, like ReprojSampleFunction: an in-place change of `weights` before backward is an error
        ctx.has_deltas = deltas is not None
        ctx.save_for_backward(*[t for t in tens if t is not None])
        ctx.chw = (C, img_h, img_w)
        ctx.mark_non_differentiable(anyv)
        return l1, comb, anyv

    @staticmethod
    @once_differentiable
    def backward(ctx, g_l1, g_comb, _g_any):
        tens = list(ctx.saved_tensors)
        if not ctx.has_deltas:
            tens.insert(2, None)
        a = _args_c(*tens, *ctx.chw)
        g_l1 = g_l1.contiguous().float()
        g_comb = g_comb.contiguous().float()
        g_w = torch.zeros_like(tens[0])
        check(lib().selfocc_reproj_c_bwd(a, ptr(g_l1), ptr(g_comb), ptr(g_w), current_stream(g_w.device)),
              "selfocc_reproj_c_bwd")
        return (g_w,) + (None,) * 10


class ReprojPickFunction(Function):
    """(values (R,S), weights (R,S), ts (R,S), deltas (R,S)|None, pix (R,2), T_prev (4,4), T_next (4,4), img_h, img_w)
       -> pick_value (R,2), pick_index (R,2) int32: per ray and frame (0 = prev, 1 = next) the sample with the largest
    masked, renormalised weight (the smallest index among equal maxima; 0 on a fully masked ray) and ``values`` there.
    ONE launch serves both frames.  Differentiable wrt ``values`` only: an arg-max hands no gradient to the weights
    (the reference's ``argmax`` + ``gather`` does not either)."""

    @staticmethod
    def forward(ctx, values, weights, ts, deltas, pix, T_prev, T_next, img_h, img_w):
        if not values.is_cuda:
            raise RuntimeError("ReprojPickFunction needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")
        f = lambda t: None if t is None else t.detach().contiguous().float()
        values, weights, ts, deltas, pix, T_prev, T_next = (f(t) for t in (values, weights, ts, deltas, pix, T_prev, T_next))
        R, S = weights.shape
        if values.shape != (R, S) or ts.shape != (R, S) or (deltas is not None and deltas.shape != (R, S)):
            raise ValueError(f"reproj_pick: values / ts / deltas must have the shape of weights {(R, S)}")
        if pix.shape != (R, 2) or T_prev.numel() != 16 or T_next.numel() != 16:
            raise ValueError("reproj_pick: pix must be (R, 2) and the transforms (4, 4)")
        dev = values.device
        a = abi.SoReprojPickArgs()
        a.weights, a.ts, a.deltas, a.values = ptr(weights), ptr(ts), ptr(deltas), ptr(values)
        a.pix, a.T_prev, a.T_next = ptr(pix), ptr(T_prev), ptr(T_next)
        a.R, a.S = R, S
        a.img_h, a.img_w = float(img_h), float(img_w)
        index = torch.empty(R, 2, device=dev, dtype=torch.int32)
        value = torch.empty(R, 2, device=dev, dtype=torch.float32)
        a.pick_index, a.pick_value = ptr(index), ptr(value)
        if R > 0:       # an empty tensor has no address, and the entry refuses NULL inputs whatever R is
            check(lib().selfocc_reproj_pick_fwd(a, current_stream(dev)), "selfocc_reproj_pick_fwd")
        ctx.save_for_backward(index)
        ctx.S = S
        ctx.mark_non_differentiable(index)
        return value, index

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_index):
        index, = ctx.saved_tensors
        g_value = g_value.contiguous().float()
        g = torch.empty(index.shape[0], ctx.S, device=index.device, dtype=torch.float32)    # every element is written
        if index.shape[0] > 0:
            check(lib().selfocc_reproj_pick_bwd(ptr(index), ptr(g_value), ptr(g), index.shape[0], ctx.S,
                                                current_stream(g.device)), "selfocc_reproj_pick_bwd")
        return (g,) + (None,) * 8


def reproj_pick(values, weights, ts, deltas, pix, T_prev, T_next, img_h, img_w):
    """-> (pick_value (R, 2) float32, pick_index (R, 2) int32); see ReprojPickFunction."""
    return ReprojPickFunction.apply(values, weights, ts, deltas, pix, T_prev, T_next, img_h, img_w)
