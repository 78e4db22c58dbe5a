"""Small building blocks the reference takes from mmengine / mmcv (absent here): BaseModule,
ModuleList, init helpers, FFN, norm builder and the mmcv MultiScaleDeformableAttention base
class whose parameters / state-dict keys CrossViewHybridAttention inherits
(model/encoder/tpvformer/attention/cross_view_hybrid_attention.py:12)."""
import math
import os
import warnings

import torch
import torch.nn as nn

from ..registry import MODELS
from ..dropout import dropout_add
from .._lib import lib, check, ptr, current_stream
from ..linear import (linear_wgrad, wgrad_supported, linear_fwd, linear_fwd_supported, linear_fwd_heads, linear_dgrad, dgrad_supported,
                      linear_fwd_heads_supported, row_groups, linear_fwd_grouped, linear_fwd_grouped_supported, linear_dgrad_grouped,
                      linear_dgrad_grouped_supported, linear_wgrad_grouped, linear_wgrad_grouped_supported)
from ..msda import (MultiScaleDeformableAttnFunction, msda_fused_inference, MSDAFusedFunction,
                    msda_fused_supported, msda_fused_kernels_built, ValueGradSink)


class BaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg
        self._is_init = False

    def init_weights(self):
        for m in self.children():
            if hasattr(m, 'init_weights'):
                m.init_weights()
        self._is_init = True


ModuleList = nn.ModuleList


def xavier_init(module, gain=1, bias=0, distribution='normal'):
    if getattr(module, 'weight', None) is not None:
        (nn.init.xavier_uniform_ if distribution == 'uniform' else nn.init.xavier_normal_)(module.weight, gain=gain)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


def constant_init(module, val, bias=0):
    if getattr(module, 'weight', None) is not None:
        nn.init.constant_(module.weight, val)
    if getattr(module, 'bias', None) is not None:
        nn.init.constant_(module.bias, bias)


GROUPED_LN_CALLS = [0]             # forward calls served by the grouped LayerNorm kernel (tests read this)


def _aligned(t):
    """`t` contiguous with a 16-byte-aligned data pointer (the LayerNorm kernels move float4s and their C entries refuse anything
    else): itself where it already is, else a copy in a fresh allocation — a contiguous view keeps its storage offset
    (``buf[1:1 + n]``, a slice of a ``cat`` / ``split`` buffer whose rows are no multiple of four floats)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _LayerNormFunction(torch.autograd.Function):
    """LayerNorm over the channel dimension (csrc/layernorm.hip).  ``sizes`` None: one (weight, bias), selfocc_layernorm_fwd /
    _bwd.  ``sizes`` = host integers (no upload, no synchronisation): one (weight, bias) pair per row group — the planes of a
    MultiPlaneNorm, concatenated — through selfocc_layernorm_fwd_grouped / _bwd_grouped, one launch for all groups in each
    direction.  ``wb`` = (weight_1, bias_1, weight_2, bias_2, ...)."""

    @staticmethod
    def forward(ctx, x, sizes, eps, *wb):
        C = x.shape[-1]
        x2 = _aligned(x.reshape(-1, C).float())
        rows = x2.shape[0]
        assert sizes is None or sum(sizes) == rows, (sizes, rows)
        y = torch.empty_like(x2)
        need = any(ctx.needs_input_grad)
        mean = torch.empty(rows, device=x.device) if need else None
        rstd = torch.empty(rows, device=x.device) if need else None
        w, b = _aligned(stack_rows(wb[0::2]).float()), _aligned(stack_rows(wb[1::2]).float())      # (G * C,) = [G][C]
        args = (ptr(x2), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, C, float(eps))
        if sizes is None:
            check(lib().selfocc_layernorm_fwd(*args, current_stream(x.device)), "selfocc_layernorm_fwd")
        else:
            check(lib().selfocc_layernorm_fwd_grouped(*args, row_groups(sizes), current_stream(x.device)),
                  "selfocc_layernorm_fwd_grouped")
            GROUPED_LN_CALLS[0] += 1
        if need:
            # the parameters themselves, not the stacked view: autograd's version check catches in-place updates before backward
            ctx.save_for_backward(x2, mean, rstd, *wb[0::2])
        ctx.shape, ctx.sizes = x.shape, sizes
        return y.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x2, mean, rstd, *ws = ctx.saved_tensors
        rows, C = x2.shape
        G = len(ws)
        w = _aligned(stack_rows(ws).float())
        dy2 = _aligned(dy.reshape(rows, C).float())
        dx = torch.empty_like(x2)
        dg, db = x2.new_empty(G, C), x2.new_empty(G, C)
        groups = () if ctx.sizes is None else (row_groups(ctx.sizes),)
        entry, workspace = ((lib().selfocc_layernorm_bwd, lib().selfocc_layernorm_bwd_workspace) if ctx.sizes is None else
                            (lib().selfocc_layernorm_bwd_grouped, lib().selfocc_layernorm_bwd_grouped_workspace))
        nbytes = int(workspace(rows, C, *groups))
        wsp = torch.empty(nbytes, dtype=torch.uint8, device=x2.device)
        check(entry(ptr(x2), ptr(w), ptr(mean), ptr(rstd), ptr(dy2), ptr(dx), ptr(dg), ptr(db), rows, C, *groups, ptr(wsp), nbytes,
                    current_stream(x2.device)), "selfocc_layernorm_bwd" if ctx.sizes is None else "selfocc_layernorm_bwd_grouped")
        return (dx.view(ctx.shape), None, None, *[t for g in range(G) for t in (dg[g], db[g])])


class FastLayerNorm(nn.LayerNorm):
    """nn.LayerNorm (same parameters / state-dict keys) whose CUDA float32 forward / backward run the streaming HIP
    kernels of csrc/layernorm.hip; anything else (CPU tensors in the host-side tests, exotic widths) is nn.LayerNorm."""

    def forward(self, x):
        C = x.shape[-1]
        if (x.is_cuda and x.dtype == torch.float32 and self.elementwise_affine and self.bias is not None
                and len(self.normalized_shape) == 1 and C % 4 == 0 and 4 <= C <= 128 and not torch.is_autocast_enabled()):
            return _LayerNormFunction.apply(x, None, self.eps, self.weight, self.bias)
        return super().forward(x)


def build_norm_layer(cfg, num_features):
    typ = cfg.get('type', 'LN')
    if typ == 'MultiPlaneNorm':     # the registered module, built as mmcv does: layer(num_features, **the other keys)
        return 'mpn', MultiPlaneNorm(num_features, **{k: v for k, v in cfg.items() if k != 'type'})
    if typ != 'LN':
        raise NotImplementedError(f"norm {typ}: only LN is used on the SelfOcc hot path")
    return 'ln', FastLayerNorm(num_features, eps=cfg.get('eps', 1e-5))


def build_activation_layer(cfg):
    typ = cfg.get('type', 'ReLU')
    if typ == 'ReLU':
        return nn.ReLU(inplace=cfg.get('inplace', False))
    if typ == 'GELU':
        return nn.GELU()
    raise NotImplementedError(typ)


# weight / bias gradients of _TallLinear through selfocc_linear_wgrad (False: batched GEMMs + torch reductions, A/B)
FUSED_WGRAD = True
# input gradient of the tall Linears on the bf16x3 kernel (csrc/linear_fwd.hip, selfocc_linear_dgrad) instead of the vendor GEMM
FUSED_DGRAD = os.environ.get('SELFOCC_LINEAR_DGRAD', '1') == '1'
DGRAD_MIN_ROWS = 32768      # below: too few 32-row tiles for 1 024 SIMDs, the vendor GEMM splits the reduction
# forward of the tall projections (and, in inference, the residual add / LayerNorm that follow them) through
# selfocc_linear_fwd (csrc/linear_fwd.hip); False: torch.addmm + separate elementwise kernels (A/B)
FUSED_LINEAR_FWD = os.environ.get('SELFOCC_FUSED_LINEAR', '1') == '1'
LINEAR_FWD_MIN_ROWS = 1024
# True: every tall-Linear pass that takes the HIP route (forward, input gradient, weight / bias gradient; ungrouped, head-major
# and grouped) computes ONE bf16 product of the round-to-nearest-even bfloat16 of its two operands instead of the exact
# three-way split — float32 accumulation, bias / residual / LayerNorm and outputs (C ABI: SO_LINEAR_BF16X1; csrc/linear_fwd.hip,
# csrc/linear.hip).  A sixth of the MFMAs and no split arithmetic for about three digits (2^-9 relative per operand), so it is
# opt-in like VALUE_BF16 below: the default reproduces the reference to 1e-4.  It changes supported HIP launches only — a
# projection that stays on torch (few rows, an unsupported K, CPU, autocast) stays what it is.  env SELFOCC_LINEAR_BF16=1 sets it;
# read at call time.  An autograd Function records the mode at forward time and its backward runs in that mode.
LINEAR_BF16 = os.environ.get('SELFOCC_LINEAR_BF16', '0') == '1'
LINEAR_BF16_CALLS = [0]            # tall-Linear launches made in the one-product mode (tests read this)


def _bf16(mode=None):
    """The mode keyword of ONE tall-Linear launch — from the switch, or from the mode a Function recorded at forward time: nothing
    when it is off (the call is the one it always was), ``bf16=True`` when it is on, counted in LINEAR_BF16_CALLS."""
    on = LINEAR_BF16 if mode is None else bool(mode)
    if not on:
        return {}
    LINEAR_BF16_CALLS[0] += 1
    return {'bf16': True}


# inference: value_proj writes the head-major layout the MSDA kernels gather fastest from (selfocc_linear_fwd_heads: no
# transposing copy) when the attention has 6 heads x 16 channels (every shipped config)
HEAD_MAJOR_PROJ = os.environ.get('SELFOCC_HEAD_MAJOR_PROJ', '1') == '1'


HEAD_MAJOR_PROJ_TRAIN = os.environ.get('SELFOCC_HEAD_MAJOR_PROJ_TRAIN', '1') == '1'


def value_proj_head_major(lins, value2d, nv, num_heads):
    """The head-major (B, 6, nv, 16) projections of (B * nv, K) rows through the G nn.Linear(K, 96) ``lins``, ONE
    selfocc_linear_fwd_heads launch with their weights stacked, or None when the shape / mode does not qualify (the caller
    then projects pixel-major as the reference does).  Under autograd: the tuple of the G outputs of one _TallLinearHeads
    node, each tagged ``_so_grad_sink = (ValueGradSink, g)`` for the g-th attention's MSDA Function; else the
    (G, B, 6, nv, 16) tensor.  Either way ``[g]`` is group g's value — under autograd the Function's own output, not a
    select (select's backward is a zero fill + a copy)."""
    K = value2d.shape[1]
    if not (HEAD_MAJOR_PROJ and FUSED_LINEAR_FWD and not torch.is_autocast_enabled() and value2d.is_cuda
            and value2d.dtype == torch.float32 and num_heads == 6):
        return None
    if any(tuple(l.weight.shape) != (96, K) or l.weight.dtype != torch.float32 or (l.bias is None and len(lins) > 1)
           for l in lins):
        return None
    rows = value2d.shape[0]
    if rows < LINEAR_FWD_MIN_ROWS or not linear_fwd_heads_supported(rows, 96 * len(lins), K, nv):
        return None
    wb = [t for l in lins for t in (l.weight, l.bias)]
    if torch.is_grad_enabled() and (value2d.requires_grad or any(l.weight.requires_grad for l in lins)):
        if not HEAD_MAJOR_PROJ_TRAIN:
            return None
        sink = ValueGradSink(len(lins)) if VALUE_GRAD_SINK else None
        outs = _TallLinearHeads.apply(value2d, nv, sink, *wb)
        if sink is not None:
            for g, o in enumerate(outs):
                o._so_grad_sink = (sink, g)
        return outs
    return linear_fwd_heads(value2d, stack_rows(wb[0::2]), stack_rows(wb[1::2]), nv, **_bf16())


# training: the MSDA backward writes grad_value pixel-major straight into the row-major gradient of the (stacked) value
# projection (msda.ValueGradSink, ABI 32 g_value_stride) instead of head-major + one transposing copy per attention
VALUE_GRAD_SINK = os.environ.get('SELFOCC_VALUE_GRAD_SINK', '1') == '1'


# training: the three TPV planes' value projections of the same image features as ONE projection / ONE backward
# (_TallLinearHeads with G = 3): the 59 MB input is read once per layer instead of three times in each direction, one input
# gradient instead of three + two accumulations (env SELFOCC_MERGED_VALUE_PROJ_TRAIN=0: per plane, as round 2)
MERGED_VALUE_PROJ_TRAIN = os.environ.get('SELFOCC_MERGED_VALUE_PROJ_TRAIN', '1') == '1'


def _linear_fwd_ok(x2d, weight):
    return (x2d.is_cuda and x2d.dtype == torch.float32 and weight.dtype == torch.float32
            and x2d.shape[0] >= LINEAR_FWD_MIN_ROWS and linear_fwd_supported(x2d.shape[0], weight.shape[0], x2d.shape[1]))


def _tall_fwd(x, w, b, relu=False, bf16=None):
    """relu?(x W^T + b) for (T, K) rows: one selfocc_linear_fwd launch when the shape qualifies, else torch.addmm.
    ``bf16``: the mode of the launch (None: the LINEAR_BF16 switch)"""
    if FUSED_LINEAR_FWD and _linear_fwd_ok(x, w):
        return linear_fwd(x, w, b, relu=relu, **_bf16(bf16))
    y = torch.addmm(b, x, w.t()) if b is not None else x @ w.t()
    return torch.relu(y) if relu else y


def fused_linear(lin, x, relu=False, residual=None, norm=None, out=None):
    """Inference form of ``norm(relu(lin(x)) + residual)`` (each part optional) for (..., K) activations: ONE
    selfocc_linear_fwd launch when the shape qualifies (CUDA float32, >= LINEAR_FWD_MIN_ROWS rows, K in 32 / 64 / 96 /
    128 / 192, LayerNorm width <= 96), else the separate torch / HIP steps in the reference's order (mmcv FFN:
    ``identity + layers(x)``; image_cross_attention.py:136 ``dropout(slots) + residual``; then the layer's `norm`).
    ``out``: optional (..., N) destination with unit column stride (a slice of a larger buffer)."""
    N, K = lin.weight.shape
    lead = x.shape[:-1]
    rows = x.numel() // max(K, 1)
    x2 = x.reshape(rows, K)
    ln_ok = norm is None or (isinstance(norm, nn.LayerNorm) and norm.elementwise_affine and norm.bias is not None
                             and tuple(norm.normalized_shape) == (N,) and N <= 96)
    if (FUSED_LINEAR_FWD and not torch.is_grad_enabled() and ln_ok and _linear_fwd_ok(x2, lin.weight)
            and not torch.is_autocast_enabled()):
        r2 = residual.reshape(rows, N) if residual is not None else None
        o2 = None
        if out is not None and out.stride(-1) == 1:
            o2 = out.view(rows, N) if out.is_contiguous() else (out[0] if out.dim() == 3 and out.shape[0] == 1 else None)
        ln = (norm.weight, norm.bias, norm.eps) if norm is not None else None
        y = linear_fwd(x2, lin.weight, lin.bias, relu=relu, residual=r2, ln=ln, out=o2, **_bf16())
        if o2 is not None:
            return out
        y = y.view(*lead, N)
        if out is not None:
            out.copy_(y)
            return out
        return y
    y = lin(x)
    if relu:
        y = torch.relu(y)
    if residual is not None:
        y = y + residual
    if norm is not None:
        y = norm(y)
    if out is not None:
        out.copy_(y)
        return out
    return y


def _dgrad(dy, weight, sizes=None, bf16=False):
    """dx = dy W — per row group with ``sizes`` (weight [G][N][K]) — on the HIP route where FUSED_DGRAD and the support query
    allow it (``bf16``: in the one-product mode), else matmul"""
    N, K = dy.shape[1], weight.shape[-1]
    hip = FUSED_DGRAD and dy.is_cuda and dy.dtype == torch.float32
    if sizes is None:
        if hip and dy.shape[0] >= DGRAD_MIN_ROWS and dgrad_supported(dy.shape[0], N, K):
            return linear_dgrad(dy, weight, **_bf16(bf16))
        return dy @ weight
    if hip and linear_dgrad_grouped_supported(sizes, N, K):
        return linear_dgrad_grouped(dy, weight, sizes, **_bf16(bf16))
    return torch.cat([d @ w for d, w in zip(torch.split(dy, sizes), weight.view(len(sizes), N, K))])


def _tall_linear_backward(x, weight, dy, has_bias, need_dx=True, y=None, sizes=None, bf16=False):
    """(dx, dW, db) of y = relu?(x W^T + b) for a row-major dy (shared by _TallLinear, _TallLinearHeads and _GroupedTallLinear).
    ``y``: the saved output of a ReLU epilogue, which masks dy.  ``sizes``: one weight per row group (weight [G][N][K]) through
    the grouped kernels -> dW (G, N, K), db (G, N); MultiPlaneFFN.forward_cat has asked their support queries.  ``bf16``: the
    mode the Function recorded at forward time — the HIP passes then run in the one-product mode (LINEAR_BF16)."""
    dy = dy.contiguous().to(x.dtype)
    if y is not None:
        dy = torch.ops.aten.threshold_backward(dy, y, 0)
    T = x.shape[0]
    if sizes is not None or (FUSED_WGRAD and dy.is_cuda and dy.dtype == torch.float32 and T > 0
                             and wgrad_supported(T, dy.shape[1], x.shape[1])):
        # one MFMA pass over dy and x for dW and db (csrc/linear.hip) instead of batched GEMMs + two reductions
        dw, db = (linear_wgrad(dy, x, has_bias, **_bf16(bf16)) if sizes is None else
                  linear_wgrad_grouped(dy, x, sizes, has_bias, **_bf16(bf16)))
        return (_dgrad(dy, weight, sizes, bf16) if need_dx else None), dw, db
    G = max(1, min(256, T // 2048))  # ~2 k+ rows per batched GEMM: enough workgroups, small partial-sum tensor
    R = T // G                       # rows per batched GEMM
    Tp = R * G
    dw = dy.new_zeros(dy.shape[1], x.shape[1])
    db = dy.new_zeros(dy.shape[1])
    if R > 0:
        dyb = dy[:Tp].view(G, R, dy.shape[1])
        dw = torch.bmm(dyb.transpose(1, 2), x[:Tp].view(G, R, x.shape[1]))
        dw = dw[0] if G == 1 else dw.sum(0)
        # bias gradient in two stages as well: torch's column reduction of a (1.65 M, N) matrix has only
        # N outputs to parallelise over (~200 GB/s, 3.1 ms per call in profiles/r1_h_train_iteration.txt;
        # rocBLAS gemv against a ones vector is worse: 16 ms); (G, R, N).sum(1) has G * N
        db = dyb.sum(1).sum(0) if T > 300000 else None
    if db is None:
        db = dy.sum(0)               # moderate row counts: one column reduction is fine
    elif Tp < T:
        db = db + dy[Tp:].sum(0)
    if Tp < T:
        dw = dw + dy[Tp:].t() @ x[Tp:]
    return (_dgrad(dy, weight, None, bf16) if need_dx else None), dw, (db if has_bias else None)


def stacked_view(params):
    """ONE contiguous tensor that IS the row-concatenation of the leaf parameters ``params`` — their storages are made to
    alias consecutive row blocks of it — so that a stacked projection costs no ``torch.cat`` per call (the round-6 training
    iteration launched ~40 five-microsecond cats for the merged sampling_offsets | attention_weights and value projections).
    The parameters stay separate ``nn.Parameter`` objects with their own names, gradients, version counters and optimiser
    state; in-place updates (optimisers, ``load_state_dict``) keep the aliasing, a ``module.to(...)`` / ``.data =``
    assignment breaks it and the next call re-establishes it.  Each parameter belongs to ONE stack, always in the same order:
    two different groupings would re-alias (one cat each) on every call.  None when a tensor is not a leaf parameter
    (``functional_call`` views under row sharding, autocast casts, ...) or is an inference tensor: the caller then cats."""
    p0 = params[0]
    if any((not isinstance(p, nn.Parameter)) or (not p.is_leaf) or p.is_inference() or p.dtype != p0.dtype
           or p.device != p0.device or p.shape[1:] != p0.shape[1:] for p in params):
        return None
    rows = sum(p.shape[0] for p in params)
    st, off, aliased = p0.untyped_storage(), p0.storage_offset(), True
    for p in params:
        if p.untyped_storage().data_ptr() != st.data_ptr() or p.storage_offset() != off or not p.is_contiguous():
            aliased = False
            break
        off += p.numel()
    if aliased:
        return torch.as_strided(p0.data, (rows, *p0.shape[1:]), p0.data.stride(), p0.storage_offset())
    # never an inference tensor, even when the first call comes under torch.inference_mode(): the parameters re-pointed at
    # it would be inference tensors too, and unusable for training from then on
    with torch.inference_mode(False), torch.no_grad():
        buf = torch.cat([p.data for p in params], 0)
        o = 0
        for p in params:
            p.data = buf[o:o + p.shape[0]]
            o += p.shape[0]
    return buf


def stack_rows(ts):
    """The row-concatenation of ``ts``: the tensor itself (or None) for one, else the parameters' shared buffer
    (stacked_view) or a torch.cat."""
    if len(ts) == 1:
        return ts[0]
    st = stacked_view(ts)
    return st if st is not None else torch.cat(ts, 0)


def _split_rows(dw, db, sizes):
    """(dW_1, db_1, dW_2, db_2, ...): the per-Linear row blocks of a stacked projection's weight / bias gradients"""
    if len(sizes) == 1:
        return dw, db
    return [t for g in zip(dw.split(sizes), db.split(sizes)) for t in g]


class _TallLinear(torch.autograd.Function):
    """y = relu?(x [W_1; ...; W_G]^T + [b_1; ...; b_G]): G >= 1 Linears of the SAME rows (T, K) as ONE projection with
    their weights stacked, output row-major (T, N_1 + ... + N_G); the bias is optional when G = 1.

    For x with millions of rows and a handful of output features: the vendor GEMM picked for the weight gradient
    dW = dy^T x of such a shape (25 x 1.65 M x 96 at the shipped nuscenes_occ sizes) runs on 2 workgroups — 23 ms per
    call, 4 calls per iteration in the round-1 profile; _tall_linear_backward splits the reduction over rows instead.
    G = 2 is the `sampling_offsets` | `attention_weights` pair of every deformable attention (image_cross_attention.py:296-312
    and cross_view_hybrid_attention.py:78-90 read the same `query` twice): one read of x and one launch forward, and —
    because the MSDA backward writes the gradient of the merged row (ABI 32 ``ol_stride``) — ONE input-gradient pass, ONE
    weight-gradient pass and no gradient add in backward.  ``relu`` is the FFN's first layer: the ReLU runs in the
    projection's epilogue and backward masks dy with the saved output (nn.ReLU(inplace=True) on the view returned here
    costs autograd a CopySlices: four extra 60 MB copies and a fill per layer)."""

    # under torch.autocast (the reference's env amp=true) the op takes float32 inputs like the HIP ops around it; mixed precision
    # on these projections is the LINEAR_BF16 switch (SELFOCC_LINEAR_BF16=1: one bf16 product, float32 accumulation), which is
    # independent of autocast.  The mode is recorded here, and backward runs in it whatever the switch says by then.
    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, relu, *wb):
        w, b = stack_rows(wb[0::2]), stack_rows(wb[1::2])
        ctx.bf16 = LINEAR_BF16
        y = _tall_fwd(x, w, b, relu, ctx.bf16)
        # the parameters themselves, not the stacked view: autograd's version check catches in-place updates before backward
        ctx.save_for_backward(x, y if relu else None, *wb[0::2])
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, dy):
        x, y, *ws = ctx.saved_tensors
        dx, dw, db = _tall_linear_backward(x, stack_rows(ws), dy, ctx.has_bias, ctx.needs_input_grad[0], y, bf16=ctx.bf16)
        return (dx, None, *_split_rows(dw, db, [w.shape[0] for w in ws]))


class _TallLinearHeads(torch.autograd.Function):
    """G >= 1 value projections nn.Linear(K, 96) of the SAME rows (one attention's value_proj, or the TPV planes' of one
    layer) with HEAD-MAJOR results: forward = one selfocc_linear_fwd_heads launch with the stacked (G * 96, K) weight, one
    (B, 6, nv, 16) tensor per group — the layout the MSDA kernels gather fastest from, forward and backward point kernels
    alike; backward = one weight-gradient and one input-gradient pass over the row-major (rows, G * 96) gradient, which the
    MSDA backward wrote in place (msda.ValueGradSink) or which is assembled with one transposing copy per group."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, nv, sink, *wb):
        w, b = stack_rows(wb[0::2]), stack_rows(wb[1::2])
        ctx.save_for_backward(x, *wb[0::2])
        ctx.has_bias, ctx.sink = b is not None, sink
        ctx.bf16 = LINEAR_BF16                                     # backward runs in the mode of the forward
        return tuple(linear_fwd_heads(x, w, b, nv, **_bf16(ctx.bf16)).unbind(0))

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, *gys):
        x, *ws = ctx.saved_tensors
        G = len(ws)
        B, H, nv, d = next(g for g in gys if g is not None).shape
        # the G attentions' MSDA backward wrote their grad_value pixel-major into ONE row-major buffer (msda.ValueGradSink):
        # the gys are views of it — no transposing copies
        dy2 = ctx.sink.rows(list(gys)) if ctx.sink is not None else None
        if dy2 is None:
            dy = x.new_empty(B, nv, G, H, d)                       # (b, pix, g, h, c): row-major (rows, G * 96)
            for g, gy in enumerate(gys):
                if gy is None:
                    dy[:, :, g].zero_()
                else:
                    dy[:, :, g].copy_(gy.permute(0, 2, 1, 3))      # one transposing copy per group
            dy2 = dy.view(B * nv, G * H * d)
        dx, dw, db = _tall_linear_backward(x, stack_rows(ws), dy2, ctx.has_bias, ctx.needs_input_grad[0], bf16=ctx.bf16)
        return (dx, None, None, *_split_rows(dw, db, [w.shape[0] for w in ws]))


# sampling_offsets | attention_weights as one projection (env SELFOCC_MERGED_OFF_LOGITS=0: two Linears, as until round 5)
MERGED_OFF_LOGITS = os.environ.get('SELFOCC_MERGED_OFF_LOGITS', '1') == '1'
MERGED_OFF_LOGITS_CALLS = [0]      # calls served by the merged projection (tests read this)


def merged_off_logits(module, x2d):
    """(T, 3 * heads * L * P) rows [heads*L*P*2 raw offsets | heads*L*P logits] = the module's `sampling_offsets` and
    `attention_weights` Linears of the rows ``x2d`` (T, K) in ONE projection, or None when the module / input does not qualify
    (the caller then runs the two Linears).  Same parameters, same state-dict keys; under autograd the result carries one
    backward for both (``_TallLinear`` with G = 2).  The kernels read the offsets as float2 and want an even row stride: an
    odd heads * L * P does not qualify."""
    so, aw = module.sampling_offsets, module.attention_weights
    if not (MERGED_OFF_LOGITS and x2d.is_cuda and x2d.dtype == torch.float32 and not torch.is_autocast_enabled()
            and so.bias is not None and aw.bias is not None and so.weight.dtype == torch.float32
            and so.weight.shape[0] == 2 * aw.weight.shape[0] and aw.weight.shape[0] % 2 == 0
            and x2d.shape[0] >= LINEAR_FWD_MIN_ROWS):
        return None
    MERGED_OFF_LOGITS_CALLS[0] += 1
    wb = (so.weight, so.bias, aw.weight, aw.bias)      # the only stack these parameters are in (stacked_view)
    if torch.is_grad_enabled() and (x2d.requires_grad or so.weight.requires_grad or aw.weight.requires_grad):
        return _TallLinear.apply(x2d, False, *wb)
    return _tall_fwd(x2d, stack_rows(wb[0::2]), stack_rows(wb[1::2]))


class TallLinear(nn.Linear):
    """nn.Linear (same parameters / state-dict keys) whose training forward goes through ``_TallLinear``
    when the input has many rows: the encoder's projections see 66 k - 153 k rows x 96 features, and the
    vendor GEMM chosen for their weight gradients (K = rows, 96 x 96 .. 96 x 2304 outputs) runs on a
    handful of workgroups (MT32x32x256: 0.3 ms x 32 calls per nuscenes_occ iteration)."""
    min_rows = 4096

    def forward(self, x):
        rows = x.numel() // max(x.shape[-1], 1)
        if torch.is_grad_enabled() and rows >= self.min_rows and (x.requires_grad or self.weight.requires_grad):
            y = _TallLinear.apply(x.reshape(rows, x.shape[-1]), False, self.weight, self.bias)
            return y.view(*x.shape[:-1], self.weight.shape[0])
        if not torch.is_grad_enabled() and FUSED_LINEAR_FWD and x.is_cuda and not torch.is_autocast_enabled():
            x2 = x.reshape(rows, x.shape[-1])
            if _linear_fwd_ok(x2, self.weight):
                return linear_fwd(x2, self.weight, self.bias, **_bf16()).view(*x.shape[:-1], self.weight.shape[0])
        return super().forward(x)


@MODELS.register_module()
class FFN(BaseModule):
    """mmcv.cnn.bricks.transformer.FFN: Linear -> act -> drop (x num_fcs-1) -> Linear -> drop,
    returns identity + out."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2,
                 act_cfg=dict(type='ReLU', inplace=True), ffn_drop=0., dropout_layer=None,
                 add_identity=True, init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        assert num_fcs >= 2
        self.embed_dims, self.feedforward_channels, self.num_fcs = embed_dims, feedforward_channels, num_fcs
        layers, in_ch = [], embed_dims
        for _ in range(num_fcs - 1):
            layers.append(nn.Sequential(TallLinear(in_ch, feedforward_channels), build_activation_layer(act_cfg),
                                        nn.Dropout(ffn_drop)))
            in_ch = feedforward_channels
        layers.append(TallLinear(feedforward_channels, embed_dims))
        layers.append(nn.Dropout(ffn_drop))
        self.layers = nn.Sequential(*layers)
        self.dropout_layer = nn.Identity()
        self.add_identity = add_identity

    def forward(self, x, identity=None, post_norm=None):
        """``post_norm``: the layer's next `norm` module, applied to the result (TPVFormerLayer hands it over so that
        inference runs Linear + ReLU and Linear + identity + LayerNorm as two launches)."""
        if (not torch.is_grad_enabled() and self.num_fcs == 2 and self.add_identity and x.is_cuda
                and isinstance(self.layers[0][1], nn.ReLU) and isinstance(self.dropout_layer, nn.Identity)
                and not (self.training and (self.layers[0][2].p > 0 or self.layers[2].p > 0))):
            h = fused_linear(self.layers[0][0], x, relu=True)
            return fused_linear(self.layers[1], h, residual=x if identity is None else identity, norm=post_norm)
        out = self._forward_plain(x, identity)
        return post_norm(out) if post_norm is not None else out

    def _forward_plain(self, x, identity=None):
        lin0 = self.layers[0][0]
        rows = x.numel() // max(x.shape[-1], 1)
        if (FUSED_FFN_RELU and self.num_fcs == 2 and torch.is_grad_enabled() and x.is_cuda and isinstance(lin0, TallLinear)
                and isinstance(self.layers[0][1], nn.ReLU) and rows >= lin0.min_rows
                and (x.requires_grad or lin0.weight.requires_grad)):
            h = _TallLinear.apply(x.reshape(rows, x.shape[-1]), True, lin0.weight, lin0.bias)
            h = self.layers[0][2](h.view(*x.shape[:-1], lin0.weight.shape[0]))
            out = self.layers[1](h)
            if FUSED_DROPOUT_ADD and self.add_identity and isinstance(self.dropout_layer, nn.Identity):
                # the last Dropout and the residual add as one pass (csrc/dropout.hip)
                drop = self.layers[2]
                return dropout_add(out, x if identity is None else identity, drop.p, drop.training)
            out = self.layers[2](out)
        else:
            out = self.layers(x)
        if not self.add_identity:
            return self.dropout_layer(out)
        if identity is None:
            identity = x
        return identity + self.dropout_layer(out)


# MultiPlaneNorm on the concatenated planes as ONE selfocc_layernorm_*_grouped launch per direction (csrc/layernorm.hip);
# env SELFOCC_GROUPED_LN=0: one FastLayerNorm call per plane + a cat (A/B)
GROUPED_LN = os.environ.get('SELFOCC_GROUPED_LN', '1') == '1'

# MultiPlaneFFN on the concatenated planes through the grouped tall-Linear kernels (selfocc_linear_{fwd,dgrad,wgrad}_grouped): one
# launch per Linear and direction for the three planes; env SELFOCC_GROUPED_FFN=0: one FFN call per plane (A/B)
GROUPED_FFN = os.environ.get('SELFOCC_GROUPED_FFN', '1') == '1'
GROUPED_FFN_CALLS = [0]            # FFN steps served by the grouped kernels (tests read this)


class _GroupedTallLinear(torch.autograd.Function):
    """y = relu?(x W_g^T + b_g) for the rows of group g (``sizes``: host integers), G Linears of the SAME shape with their
    weights stacked ([G][N][K], the parameters aliased by stacked_view): forward, input gradient and weight / bias gradient
    are ONE launch each for all groups.  ``wb`` = (weight_1, bias_1, weight_2, bias_2, ...)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, x, sizes, relu, *wb):
        w, b = stack_rows(wb[0::2]), stack_rows(wb[1::2])
        ctx.bf16 = LINEAR_BF16                                     # backward runs in the mode of the forward
        y = linear_fwd_grouped(x, sizes, w, b, relu=relu, **_bf16(ctx.bf16))
        # the parameters themselves, not the stacked view: autograd's version check catches in-place updates before backward
        ctx.save_for_backward(x, y if relu else None, *wb[0::2])
        ctx.sizes = list(sizes)
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, dy):
        x, y, *ws = ctx.saved_tensors
        dx, dw, db = _tall_linear_backward(x, stack_rows(ws), dy, True, ctx.needs_input_grad[0], y, ctx.sizes, ctx.bf16)
        return (dx, None, None, *[t for g in range(len(ws)) for t in (dw[g], db[g])])


@MODELS.register_module()
class MultiPlaneNorm(BaseModule):
    """model/encoder/tpvformer/modules/split_norm.py: one norm layer per TPV plane (hw, zh, wz) — same constructor, same
    parameters ``norms.P.{weight,bias}``; ``forward`` takes and returns the planes.  ``forward_cat`` is the same function of
    the planes' concatenation (what TPVFormerLayer keeps): on the GPU one grouped LayerNorm launch per direction."""

    def __init__(self, embed_dims=64, norm_cfg=dict(type='LN'), init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        self.embed_dim = embed_dims
        self.norm_cfg = norm_cfg
        if norm_cfg.get('type', 'LN') != 'LN':
            raise NotImplementedError(f"MultiPlaneNorm of {norm_cfg.get('type')}: only LN is used on the SelfOcc hot path")
        self.norms = nn.ModuleList([build_norm_layer(self.norm_cfg, self.embed_dim)[1] for _ in range(3)])

    def _grouped_ok(self, x):
        C = x.shape[-1]
        n0 = self.norms[0]
        return (GROUPED_LN and x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()
                and C % 4 == 0 and 4 <= C <= 128
                and all(isinstance(n, FastLayerNorm) and n.elementwise_affine and n.bias is not None
                        and tuple(n.normalized_shape) == (C,) and n.eps == n0.eps and n.weight.dtype == torch.float32
                        for n in self.norms))

    def forward_cat(self, x, sizes):
        """(B, sum sizes, C) concatenated planes -> the same shape, plane p normalised by ``norms[p]``"""
        assert len(sizes) == len(self.norms) and sum(sizes) == x.shape[1], (sizes, tuple(x.shape))
        if x.shape[0] == 1 and self._grouped_ok(x):
            wb = [t for n in self.norms for t in (n.weight, n.bias)]
            return _LayerNormFunction.apply(x, list(sizes), self.norms[0].eps, *wb)
        return torch.cat([n(p) for n, p in zip(self.norms, torch.split(x, list(sizes), 1))], 1)

    def forward(self, tpv):
        tpv = list(tpv)
        if len(tpv) == len(self.norms) and tpv[0].dim() == 3 and tpv[0].shape[0] == 1 and self._grouped_ok(tpv[0]):
            sizes = [p.shape[1] for p in tpv]
            return list(torch.split(self.forward_cat(torch.cat(tpv, 1), sizes), sizes, 1))
        return [self.norms[i](plane) for i, plane in enumerate(tpv)]


@MODELS.register_module()
class MultiPlaneFFN(BaseModule):
    """model/encoder/tpvformer/modules/split_fpn.py: one FFN per TPV plane — same constructor, same parameters
    ``ffns.P.layers...``; ``forward`` takes and returns the planes, each through the FFN above.  ``forward_cat`` is the same
    function of the planes' concatenation (what TPVFormerLayer keeps) on the grouped tall-Linear kernels."""

    def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0.,
                 act_cfg=dict(type='ReLU', inplace=True), init_cfg=None):
        super().__init__(init_cfg)
        self.ffn_cfg = dict(type='FFN', embed_dims=embed_dims, feedforward_channels=feedforward_channels, num_fcs=num_fcs,
                            ffn_drop=ffn_drop, act_cfg=act_cfg)
        self.embed_dims = embed_dims
        self.ffns = nn.ModuleList([MODELS.build(dict(self.ffn_cfg)) for _ in range(3)])

    def forward_cat(self, x, sizes, identity=None, post_norm=None):
        """The same function of the planes' concatenation (1, sum sizes, C) — what TPVFormerLayer keeps — through the grouped
        tall-Linear kernels, or None where they do not cover the case (the caller then runs the per-plane composition):
        training = Linear + ReLU, Linear (one _GroupedTallLinear node each), torch dropout on the hidden rows, dropout_add for
        the last dropout + identity; inference = Linear + ReLU, then Linear + identity + the per-plane LayerNorm of ``post_norm``
        in the epilogue: two launches for all planes."""
        f0 = self.ffns[0]
        if not (GROUPED_FFN and FUSED_LINEAR_FWD and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == 1
                and not torch.is_autocast_enabled() and len(sizes) == len(self.ffns) and sum(sizes) == x.shape[1]
                and x.shape[1] >= LINEAR_FWD_MIN_ROWS
                and all(f.num_fcs == 2 and f.add_identity and isinstance(f.layers[0][1], nn.ReLU)
                        and isinstance(f.dropout_layer, nn.Identity) and f.layers[0][0].weight.dtype == torch.float32
                        and f.layers[0][0].bias is not None and f.layers[1].bias is not None for f in self.ffns)):
            return None
        C, FF = f0.embed_dims, f0.feedforward_channels
        if not (x.shape[2] == C and linear_fwd_grouped_supported(sizes, FF, C) and linear_fwd_grouped_supported(sizes, C, FF)):
            return None
        norms = None
        if post_norm is not None:
            norms = list(post_norm.norms)
            if not (C <= 96 and post_norm._grouped_ok(x)):
                return None
        lin0 = [f.layers[0][0] for f in self.ffns]
        lin1 = [f.layers[1] for f in self.ffns]
        wb0 = [t for l in lin0 for t in (l.weight, l.bias)]          # the only stacks these parameters are in (stacked_view)
        wb1 = [t for l in lin1 for t in (l.weight, l.bias)]
        x2 = x.reshape(x.shape[1], C)
        idt = x2 if identity is None else identity.reshape(x.shape[1], C)
        drop0, drop1 = f0.layers[0][2], f0.layers[2]
        sizes = list(sizes)
        if torch.is_grad_enabled() and (x.requires_grad or lin0[0].weight.requires_grad):
            if not (linear_wgrad_grouped_supported(sizes, FF, C) and linear_wgrad_grouped_supported(sizes, C, FF)):
                return None
            GROUPED_FFN_CALLS[0] += 1
            h = drop0(_GroupedTallLinear.apply(x2, sizes, True, *wb0))
            out = _GroupedTallLinear.apply(h, sizes, False, *wb1)
            if FUSED_DROPOUT_ADD:
                out = dropout_add(out, idt, drop1.p, drop1.training)
            else:
                out = idt + drop1(out)
            out = out.view(x.shape)
            return post_norm.forward_cat(out, sizes) if post_norm is not None else out
        if torch.is_grad_enabled() or (self.training and (drop0.p > 0 or drop1.p > 0)):
            return None
        GROUPED_FFN_CALLS[0] += 1
        h = linear_fwd_grouped(x2, sizes, stack_rows(wb0[0::2]), stack_rows(wb0[1::2]), relu=True, **_bf16())
        ln = None
        if norms is not None:
            ln = (stack_rows([n.weight for n in norms]), stack_rows([n.bias for n in norms]), norms[0].eps)
        return linear_fwd_grouped(h, sizes, stack_rows(wb1[0::2]), stack_rows(wb1[1::2]), residual=idt, ln=ln,
                                  **_bf16()).view(x.shape)

    def forward(self, tpv, identity=None, post_norm=None):
        """``post_norm``: the layer's next MultiPlaneNorm; plane p's result then goes through ``post_norm.norms[p]``"""
        if identity is None:
            identity = [None] * 3
        norms = [None] * 3 if post_norm is None else list(post_norm.norms)
        return [self.ffns[i](plane, identity[i], post_norm=norms[i]) for i, plane in enumerate(tpv)]


# training: the FFN's Linear + ReLU as one autograd node (_TallLinear with relu); env SELFOCC_FUSED_FFN_RELU=0: nn.Sequential
FUSED_FFN_RELU = os.environ.get('SELFOCC_FUSED_FFN_RELU', '1') == '1'
# training: `identity + dropout(x)` at the end of every attention / FFN block as one HIP pass per direction with a
# counter-based mask (selfocc_amd/dropout.py); env SELFOCC_FUSED_DROPOUT=0: torch's dropout + add
FUSED_DROPOUT_ADD = os.environ.get('SELFOCC_FUSED_DROPOUT', '1') == '1'
# training path of deformable_sampling: fused prologue + MSDA in both directions (msda.MSDAFusedFunction)
FUSED_TRAINING = True
# True: the projected `value` of the deformable attentions is STORED as bfloat16 for the gathers (forward and backward
# point kernels); arithmetic and gradients stay float32.  Halves the corner segments the L1-bound gathers move
# (BASELINE configs[1]: "bf16"); deviates from the reference's float32 MSDA by the bf16 rounding of value (~2^-9
# relative), so it is opt-in: the default reproduces the reference to 1e-4.  env SELFOCC_VALUE_BF16=1 sets it.
VALUE_BF16 = os.environ.get('SELFOCC_VALUE_BF16', '0') == '1'


def deformable_sampling(module, query, value, reference_points, spatial_shapes, level_start_index,
                        per_level_reference, key_padding_mask=None):
    """Shared body of the three deformable attentions: value_proj, offset / weight linears,
    softmax, sampling locations, MSDA (HIP).  ``per_level_reference``: reference points
    carry their own (level, point) dims (CrossViewHybridAttention,
    cross_view_hybrid_attention.py:96-99) instead of one anchor per point
    (BEVDeformableAttention, bevformer/attention/image_cross_attention.py:323-328)."""
    bs, num_query, _ = query.shape
    _, num_value, _ = value.shape
    host_shapes = getattr(spatial_shapes, '_so_host', None)
    if host_shapes is not None:      # no device read-back (a stream sync per call) when the caller knows the shapes
        assert sum(host_shapes[0::2][i] * host_shapes[1::2][i] for i in range(len(host_shapes) // 2)) == num_value
    else:
        assert int((spatial_shapes[:, 0] * spatial_shapes[:, 1]).sum()) == num_value
    LP0 = module.num_levels * module.num_points
    v_hm = None
    if (key_padding_mask is None and LP0 <= 256 and module.value_proj.weight.shape[0] == 96
            and (not torch.is_grad_enabled() or FUSED_TRAINING)):
        # the projection itself writes (bs, heads, nv, d)
        v_hm = value_proj_head_major([module.value_proj], value.reshape(bs * num_value, -1), num_value, module.num_heads)
        v_hm = v_hm[0] if v_hm is not None else None
    if v_hm is None:
        value = module.value_proj(value)
        if key_padding_mask is not None:
            value = value.masked_fill(key_padding_mask[..., None], 0.0)
        value = value.view(bs, num_value, module.num_heads, -1)
    if reference_points.shape[-1] != 2:
        raise ValueError('Last dim of reference_points must be 2 on the SelfOcc path, '
                         f'got {reference_points.shape[-1]}')
    LP = module.num_levels * module.num_points
    d_head = module.value_proj.weight.shape[0] // module.num_heads
    use_bf16 = VALUE_BF16 and d_head == 16          # the bfloat16 gathers are built for 16 channels per head only
    kind = {'level': 0, 'point': 1, 'level_point': 2}[per_level_reference]
    fused_inf = not torch.is_grad_enabled() and LP <= 256 and msda_fused_kernels_built(d_head)
    fused_train = False
    if not fused_inf and FUSED_TRAINING and value.is_cuda and LP <= 256:
        host = getattr(spatial_shapes, '_so_host', None)
        if host is None:
            host = [int(v) for v in spatial_shapes.reshape(-1).tolist()]
        fused_train = msda_fused_supported(host, bs, num_query, module.num_heads, d_head, module.num_levels, module.num_points)
    # sampling_offsets | attention_weights: ONE projection with the stacked weight for the fused kernels (they read — and
    # in backward write — the merged row in place), the two Linears of the reference otherwise
    ol = merged_off_logits(module, query.reshape(bs * num_query, -1)) if (fused_inf or fused_train) else None
    if ol is not None:
        ol, off, logits, mlp = ol.view(bs, num_query, -1), None, None, (module.num_levels, module.num_points)
    else:
        mlp = None
        off = module.sampling_offsets(query).view(bs, num_query, module.num_heads, module.num_levels, module.num_points, 2)
    if fused_inf:
        # inference: softmax + sampling-location prologue fused into the HIP kernel (no loc / weight tensors)
        if ol is None:
            logits = module.attention_weights(query).view(bs, num_query, module.num_heads, LP)
        hm = v_hm is not None
        if hm:
            value = v_hm
        if use_bf16:
            value = value.to(torch.bfloat16)
        return msda_fused_inference(value, spatial_shapes, level_start_index, reference_points, kind,
                                    ol if ol is not None else off, logits, hm, mlp)
    if fused_train:
        # training: the same fusion in both directions (no loc / weight tensors, no softmax / normalise kernels)
        if ol is None:
            logits = module.attention_weights(query).view(bs, num_query, module.num_heads, LP)
        hm = v_hm is not None
        if hm:
            value = v_hm
        return MSDAFusedFunction.apply(value, spatial_shapes, level_start_index, reference_points, kind,
                                       ol if ol is not None else off, logits, host, hm, use_bf16, mlp,
                                       getattr(v_hm, '_so_grad_sink', None))
    if v_hm is not None:      # (the unfused fallback below wants the mmcv layout)
        value = v_hm.permute(0, 2, 1, 3).contiguous()
    aw = module.attention_weights(query).view(bs, num_query, module.num_heads,
                                              module.num_levels * module.num_points).softmax(-1)
    aw = aw.view(bs, num_query, module.num_heads, module.num_levels, module.num_points)
    normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
    if per_level_reference == 'level_point':      # (bs, nq, L, P, 2)
        ref = reference_points[:, :, None, :, :, :]
    elif per_level_reference == 'point':          # (bs, nq, P, 2): one anchor per point, all levels
        ref = reference_points[:, :, None, None, :, :]
    else:                                         # (bs, nq, L, 2): mmcv base class
        ref = reference_points[:, :, None, :, None, :]
    loc = ref + off / normalizer[None, None, None, :, None, :]
    return MultiScaleDeformableAttnFunction.apply(value, spatial_shapes, level_start_index, loc, aw,
                                                  module.im2col_step)


@MODELS.register_module()
class MultiScaleDeformableAttention(BaseModule):
    """mmcv.ops.multi_scale_deform_attn.MultiScaleDeformableAttention (mmcv==2.0.1): same
    constructor, parameters (sampling_offsets, attention_weights, value_proj, output_proj) and
    forward contract; used as self-attention by config/nuscenes/nuscenes_occ_bev.py:222."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64,
                 dropout=0.1, batch_first=False, norm_cfg=None, init_cfg=None, value_proj_ratio=1.0):
        super().__init__(init_cfg)
        if embed_dims % num_heads != 0:
            raise ValueError(f'embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}')
        dim_per_head = embed_dims // num_heads
        if dim_per_head & (dim_per_head - 1):
            warnings.warn("the HIP MSDA kernels need a power-of-two dim per head: 8, 16 or 32 for the fused / camera-loop ops, "
                          "4 on the plain op only")
        self.norm_cfg, self.batch_first = norm_cfg, batch_first
        self.dropout = nn.Dropout(dropout)
        self.im2col_step, self.embed_dims = im2col_step, embed_dims
        self.num_levels, self.num_heads, self.num_points = num_levels, num_heads, num_points
        self.sampling_offsets = TallLinear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = TallLinear(embed_dims, num_heads * num_levels * num_points)
        value_proj_size = int(embed_dims * value_proj_ratio)
        self.value_proj = TallLinear(embed_dims, value_proj_size)
        self.output_proj = TallLinear(value_proj_size, embed_dims)
        self.init_weights()

    _scale_points = True  # mmcv scales the i-th point's offset bias by (i + 1)

    def init_weights(self):
        constant_init(self.sampling_offsets, 0.)
        thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
        grid_init = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid_init = (grid_init / grid_init.abs().max(-1, keepdim=True)[0]).view(
            self.num_heads, 1, 1, 2).repeat(1, self.num_levels, self.num_points, 1)
        if self._scale_points:
            for i in range(self.num_points):
                grid_init[:, :, i, :] *= i + 1
        self.sampling_offsets.bias.data = grid_init.view(-1).to(self.sampling_offsets.bias.device)
        constant_init(self.attention_weights, val=0., bias=0.)
        xavier_init(self.value_proj, distribution='uniform', bias=0.)
        if hasattr(self, 'output_proj'):
            xavier_init(self.output_proj, distribution='uniform', bias=0.)
        self._is_init = True

    _reference_kind = 'level'

    def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                reference_points=None, spatial_shapes=None, level_start_index=None, **kwargs):
        if value is None:
            value = query
        if identity is None:
            identity = query
        if query_pos is not None:
            query = query + query_pos
        if not self.batch_first:
            query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
        output = deformable_sampling(self, query, value, reference_points, spatial_shapes, level_start_index,
                                     self._reference_kind, key_padding_mask)
        post_norm = kwargs.get('post_norm')
        if not torch.is_grad_enabled() and not self.training and self.batch_first and output.is_cuda:
            return fused_linear(self.output_proj, output, residual=identity, norm=post_norm)
        output = self.output_proj(output)
        if not self.batch_first:
            output = output.permute(1, 0, 2)
        if FUSED_DROPOUT_ADD:
            output = dropout_add(output, identity, self.dropout.p, self.dropout.training)
        else:
            output = self.dropout(output) + identity
        return post_norm(output) if post_norm is not None else output
