"""Host side of the fused reprojection sampling: the per-sample part of ReprojLossMonoMultiNewCombine.reproj_loss
(loss/reproj_loss_mono_multi_new_combine.py:108-201) for one camera, and of the arg-max pick of the mono loss's
``sdf_loss`` term (selfocc_reproj_pick_fwd / _bwd; loss/reproj_loss_mono_multi_new.py:265-270).  The sampling is one kernel
and, here, one Function body with two image forms: planar 3-channel images through selfocc_reproj_fwd / _bwd, channel-last
images of any channel count (the losses' ``dims`` knob) through selfocc_reproj_c_fwd / _bwd."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import abi
from ._lib import lib, check, ptr, current_stream


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


def _args(tens, C, img_h, img_w):
    """tens = [weights, ts, deltas | None, pix, curr, T_prev, T_next, img_prev, img_next] -> the struct of the image form:
    so_reproj_args for planar (3, Hi, Wi) images (C is None), so_reproj_c_args for channel-last (Hi, Wi, stride) ones"""
    weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next = tens
    a = abi.SoReprojArgs() if C is None else abi.SoReprojCArgs()
    a.weights, a.ts, a.deltas, a.pix = ptr(weights), ptr(ts), ptr(deltas), ptr(pix)
    a.T_prev, a.T_next = ptr(T_prev), ptr(T_next)
    a.img_prev, a.img_next = ptr(img_prev), ptr(img_next)
    a.R, a.S = weights.shape
    if C is None:
        a.curr_rgb = ptr(curr)
        a.Hi, a.Wi = img_prev.shape[1:]
    else:
        a.curr, a.C = ptr(curr), C
        a.Hi, a.Wi, a.img_stride = img_prev.shape
    a.img_h, a.img_w = float(img_h), float(img_w)
    return a


class _ReprojSample(Function):
    """The one body of ReprojSampleFunction / ReprojSampleCFunction.  A subclass names its entries (``who``), says whether
    its images are planar and turns an image argument into the float32 tensor whose address the entry gets, and C."""

    @classmethod
    def forward(cls, ctx, weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next, img_h, img_w):
        if not weights.is_cuda:
            raise RuntimeError(f"{cls.__name__} needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")
        f = lambda t: None if t is None else t.detach().contiguous().float()
        weights, ts, deltas, pix, curr, T_prev, T_next = (f(t) for t in (weights, ts, deltas, pix, curr, T_prev, T_next))
        (img_prev, C), (img_next, C_next) = cls._image(img_prev), cls._image(img_next)
        R, S = weights.shape
        who = cls.who
        if C_next != C or img_next.shape != img_prev.shape:
            raise ValueError(f"{who}: img_prev {tuple(img_prev.shape)} (C = {C}) and img_next {tuple(img_next.shape)} "
                             f"(C = {C_next}) differ")
        if curr.shape != (R, C) or pix.shape != (R, 2) or ts.shape != (R, S) or (deltas is not None and deltas.shape != (R, S)):
            raise ValueError(f"{who}: need curr (R, C) = {(R, C)}, pix (R, 2) and ts / deltas of the shape of weights "
                             f"{(R, S)}; got curr {tuple(curr.shape)}, pix {tuple(pix.shape)}, ts {tuple(ts.shape)}")
        if T_prev.numel() != 16 or T_next.numel() != 16:
            raise ValueError(f"{who}: the transforms must be (4, 4)")
        tens = [weights, ts, deltas, pix, curr, T_prev, T_next, img_prev, img_next]
        ctx.form = (None if cls.planar else C, img_h, img_w)
        a = _args(tens, *ctx.form)
        dev = weights.device
        l1 = torch.empty(R, device=dev)
        comb = torch.empty(R, C, device=dev)
        anyv = torch.empty(R, device=dev)
        a.l1, a.any_valid = ptr(l1), ptr(anyv)
        if cls.planar:
            a.rgb_combine = ptr(comb)
        else:
            a.combine = ptr(comb)
        check(getattr(lib(), f"selfocc_{who}_fwd")(a, current_stream(dev)), f"selfocc_{who}_fwd")
        # saved through autograd (version-counter checks, saved-tensor hooks): an in-place change of `weights`
        # between forward and backward is an error, not a silent mismatch
        ctx.has_deltas = deltas is not None
        ctx.save_for_backward(*[t for t in tens if t is not None])
        ctx.mark_non_differentiable(anyv)
        return l1, comb, anyv

    @classmethod
    @once_differentiable
    def backward(cls, ctx, g_l1, g_comb, _g_any):
        tens = list(ctx.saved_tensors)
        if not ctx.has_deltas:
            tens.insert(2, None)
        a = _args(tens, *ctx.form)
        g_l1 = g_l1.contiguous().float()
        g_comb = g_comb.contiguous().float()
        g_w = torch.zeros_like(tens[0])
        check(getattr(lib(), f"selfocc_{cls.who}_bwd")(a, ptr(g_l1), ptr(g_comb), ptr(g_w), current_stream(g_w.device)),
              f"selfocc_{cls.who}_bwd")
        return (g_w,) + (None,) * 10


class ReprojSampleFunction(_ReprojSample):
    """(weights (R,S), ts (R,S), deltas (R,S)|None, pix (R,2), curr_rgb (R,3), T_prev (4,4),
    T_next (4,4), img_prev (3,Hi,Wi), img_next (3,Hi,Wi), img_h, img_w)
       -> l1 (R), rgb_combine (R,3), any_valid (R), through selfocc_reproj_fwd / _bwd on the planar images as they are.
    Differentiable wrt ``weights`` only (ts / pixels / matrices / images are constants of the loss in the reference too)."""
    who, planar = "reproj", True

    @staticmethod
    def _image(img):
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"reproj: need planar (3, Hi, Wi) images, got {tuple(img.shape)}")
        return img.detach().contiguous().float(), 3


class ReprojSampleCFunction(_ReprojSample):
    """ReprojSampleFunction on images of C channels (selfocc_reproj_c_fwd / _bwd):
    (weights (R,S), ts (R,S), deltas (R,S)|None, pix (R,2), curr (R,C), T_prev (4,4), T_next (4,4), img_prev, img_next,
    img_h, img_w) -> l1 (R), combine (R,C), any_valid (R).  ``img_prev`` / ``img_next`` are ChannelLastImage (convert an
    image once with ``channel_last`` where it is sampled more than once) or tensors with (C, Hi, Wi) semantics of any layout,
    converted here.  Differentiable wrt ``weights`` only."""
    who, planar = "reproj_c", False

    @staticmethod
    def _image(img):
        img = channel_last(img)
        return img.data, img.C


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
