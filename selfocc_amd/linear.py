"""Host side of the tall-Linear kernels (csrc/linear_fwd.hip, csrc/linear.hip): forward, input gradient, and weight / bias
gradient of a Linear with very many rows, each in one pass — ungrouped, or with one weight per row group (``sizes``).
Used by model.bricks (the encoder's projections, the field MLP, the per-plane FFNs).

``bf16=True`` on any pass is the C ABI's SO_LINEAR_BF16X1 (include/selfocc_hip.h): ONE bf16 product of the round-to-nearest-even
bfloat16 of the two operands, float32 accumulation and outputs, the default's epilogue — about three digits for a sixth of the
matrix work (and a third of the LDS / workspace footprint).  Off by default; model.bricks.LINEAR_BF16 is the switch of the encoder.  The support queries answer the same in
both modes (a flagged launch always has a one-product kernel), so their ``bf16`` keyword changes nothing."""
import torch

from ._lib import lib, check, ptr, current_stream
from .abi import LINEAR_RELU, LINEAR_BF16X1, SoRowGroups


def _need_cuda(t, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who} needs CUDA(HIP) tensors: selfocc_amd has no CPU fallback")


# ---- row groups (so_row_groups: the TPV planes of a MultiPlaneFFN / MultiPlaneNorm, concatenated) ----
_ROW_GROUPS = {}


def row_groups(sizes):
    """the by-value so_row_groups of these group sizes (host constants: no upload, no synchronisation; built once per tuple)"""
    key = tuple(int(n) for n in sizes)
    hit = _ROW_GROUPS.get(key)
    if hit is None:
        hit = _ROW_GROUPS[key] = SoRowGroups.from_sizes(key)
    return hit


def _grouped_supported(query, sizes, n_out, n_in):
    return 1 <= len(sizes) <= 8 and query(int(sum(sizes)), int(n_out), int(n_in), row_groups(sizes)) == 1


# ---- weight / bias gradient ----
def wgrad_supported(rows, n_out, n_in, bf16=False):
    return lib().selfocc_linear_wgrad_supported(int(rows), int(n_out), int(n_in)) == 1


def linear_wgrad_grouped_supported(sizes, n_out, n_in, bf16=False):
    return _grouped_supported(lib().selfocc_linear_wgrad_grouped_supported, sizes, n_out, n_in)


def _linear_wgrad(dy, x, with_bias, sizes=None, bf16=False):
    who = "linear_wgrad" if sizes is None else "linear_wgrad_grouped"
    _need_cuda(dy, who)
    T, N = dy.shape
    K = x.shape[1]
    assert x.shape[0] == T and dy.dtype == torch.float32 and x.dtype == torch.float32
    assert sizes is None or sum(sizes) == T
    dy, x = dy.contiguous(), x.contiguous()
    lead = () if sizes is None else (len(sizes),)
    dw = torch.empty(*lead, N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(*lead, N, device=dy.device, dtype=torch.float32) if with_bias else None
    groups = () if sizes is None else (row_groups(sizes),)
    name = "selfocc_" + who + ("_flags" if bf16 else "")
    flags = (LINEAR_BF16X1,) if bf16 else ()      # the default mode stays on the entries without `flags`
    entry, workspace = getattr(lib(), name), getattr(lib(), "selfocc_" + who + "_workspace" + ("_flags" if bf16 else ""))
    nbytes = int(workspace(T, N, K, *groups, *flags))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    check(entry(ptr(dy), ptr(x), ptr(dw), ptr(db), T, N, K, *groups, ptr(ws), nbytes, *flags, current_stream(dy.device)), name)
    return dw, db


def linear_wgrad(dy, x, with_bias=True, bf16=False):
    """dy (T, N), x (T, K) float32 CUDA(HIP) contiguous -> (dw (N, K), db (N) | None).  ``bf16``: dw = bf16(dy)^T bf16(x) and db =
    the column sums of bf16(dy) (the one-product mode)."""
    return _linear_wgrad(dy, x, with_bias, None, bf16)


def linear_wgrad_grouped(dy, x, sizes, with_bias=True, bf16=False):
    """dy (T, N), x (T, K) -> (dw (G, N, K), db (G, N) | None): group g's gradients from its rows; ONE pass + a per-group reduction"""
    return _linear_wgrad(dy, x, with_bias, sizes, bf16)


# ---- input gradient ----
def dgrad_supported(rows, n_out, n_in, bf16=False):
    return lib().selfocc_linear_dgrad_supported(int(rows), int(n_out), int(n_in)) == 1


def linear_dgrad_grouped_supported(sizes, n_out, n_in, bf16=False):
    return _grouped_supported(lib().selfocc_linear_dgrad_grouped_supported, sizes, n_out, n_in)


def _linear_dgrad(dy, weight, sizes=None, bf16=False):
    who = "linear_dgrad" if sizes is None else "linear_dgrad_grouped"
    _need_cuda(dy, who)
    T, N = dy.shape
    K = weight.shape[-1]
    G = 1 if sizes is None else len(sizes)
    assert weight.numel() == G * N * K and dy.dtype == torch.float32 and weight.dtype == torch.float32
    assert sizes is None or sum(sizes) == T
    dy, weight = dy.contiguous(), weight.contiguous()
    dx = torch.empty(T, K, device=dy.device, dtype=torch.float32)
    groups = () if sizes is None else (row_groups(sizes),)
    name = "selfocc_" + who + ("_flags" if bf16 else "")
    flags = (LINEAR_BF16X1,) if bf16 else ()      # the default mode stays on the entries without `flags`
    entry, workspace = getattr(lib(), name), getattr(lib(), "selfocc_" + who + "_workspace" + ("_flags" if bf16 else ""))
    nbytes = int(workspace(N, K, *groups, *flags))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    check(entry(ptr(dy), ptr(weight), ptr(dx), T, N, K, *groups, ptr(ws), nbytes, *flags, current_stream(dy.device)), name)
    return dx


def linear_dgrad(dy, weight, bf16=False):
    """dx (T, K) = dy (T, N) @ weight (N, K), float32 CUDA(HIP) (csrc/linear_fwd.hip, linear_dgrad_b3_kernel).
    ``bf16``: dx = bf16(dy) @ bf16(weight) (the one-product mode)."""
    return _linear_dgrad(dy, weight, None, bf16)


def linear_dgrad_grouped(dy, weight, sizes, bf16=False):
    """dx (T, K): the rows of group g are dy_g (T_g, N) @ weight[g] (N, K); weight (G, N, K); ONE launch (+ the split of W)"""
    return _linear_dgrad(dy, weight, sizes, bf16)


# ---- forward ----
def linear_fwd_supported(rows, n_out, n_in, bf16=False):
    return lib().selfocc_linear_fwd_supported(int(rows), int(n_out), int(n_in)) == 1


def linear_fwd_grouped_supported(sizes, n_out, n_in, bf16=False):
    return _grouped_supported(lib().selfocc_linear_fwd_grouped_supported, sizes, n_out, n_in)


def _linear_fwd(x, weight, bias, relu, residual, ln, out, want_stats, sizes=None, shared_w=False, bf16=False):
    """the argument handling of linear_fwd (``sizes`` None) and linear_fwd_grouped, and the one call that differs"""
    who = "linear_fwd" if sizes is None else "linear_fwd_grouped"
    _need_cuda(x, who)
    T, K = x.shape
    G = 1 if sizes is None else len(sizes)
    assert x.dtype == torch.float32 and weight.dtype == torch.float32 and (sizes is None or sum(sizes) == T)
    x, weight = x.contiguous(), weight.contiguous()
    w_stride = 0 if sizes is None or shared_w else weight.numel() // G      # floats between two groups' weights: N * K
    N = (w_stride or weight.numel()) // K
    assert weight.shape[-1] == K and weight.numel() == (G if w_stride else 1) * N * K
    if bias is not None:
        bias = bias.contiguous()
        assert bias.numel() == (G if w_stride else 1) * N
    if out is None:
        out = torch.empty(T, N, device=x.device, dtype=torch.float32)
    assert out.shape == (T, N) and out.stride(1) == 1 and out.dtype == torch.float32
    ldr = 0
    if residual is not None:
        assert residual.shape == (T, N) and residual.dtype == torch.float32
        if residual.stride(1) != 1:
            residual = residual.contiguous()
        ldr = residual.stride(0) if T > 1 else N
    g = b = y_pre = mean = rstd = None
    eps, ln_stride = 0.0, 0
    if ln is not None:
        g, b, eps = ln
        g, b = g.contiguous(), b.contiguous()
        assert g.numel() == b.numel() and g.numel() in (N, G * N)
        ln_stride = N if g.numel() == G * N and G > 1 else 0      # (G = 1: either way the one set)
        if want_stats:
            y_pre = torch.empty(T, N, device=x.device, dtype=torch.float32)
            mean = torch.empty(T, device=x.device, dtype=torch.float32)
            rstd = torch.empty(T, device=x.device, dtype=torch.float32)
    elif want_stats:
        raise ValueError("want_stats needs ln")
    ldy = out.stride(0) if T > 1 else N
    args = (ptr(x), ptr(weight), ptr(bias), ptr(residual), int(ldr), ptr(g), ptr(b), float(eps), ptr(out), int(ldy), ptr(y_pre),
            ptr(mean), ptr(rstd), T, N, K, (LINEAR_RELU if relu else 0) | (LINEAR_BF16X1 if bf16 else 0))
    if sizes is None:
        check(lib().selfocc_linear_fwd(*args, current_stream(x.device)), "selfocc_linear_fwd")
    else:
        check(lib().selfocc_linear_fwd_grouped(*args, row_groups(sizes), w_stride, ln_stride, current_stream(x.device)),
              "selfocc_linear_fwd_grouped")
    return (out, y_pre, mean, rstd) if want_stats else out


def linear_fwd(x, weight, bias=None, relu=False, residual=None, ln=None, out=None, want_stats=False, bf16=False):
    """y = LN?(relu?(x W^T + b) + residual) in one MFMA-f32 pass (csrc/linear_fwd.hip).

    x (T, K), weight (N, K), bias (N) | None, residual (T, N) | None (row stride free, unit column stride),
    ln = (gamma (N), beta (N), eps) | None, out (T, N) | None (row stride free: a column / row slice of a larger buffer).
    -> y, or (y, y_pre, mean, rstd) with ``want_stats`` (the LayerNorm input and statistics selfocc_layernorm_bwd needs).
    ``bf16``: the product is bf16(x) bf16(W)^T (the one-product mode); bias, residual, gamma, beta and the output stay float32."""
    return _linear_fwd(x, weight, bias, relu, residual, ln, out, want_stats, bf16=bf16)


def linear_fwd_grouped(x, sizes, weight, bias=None, relu=False, residual=None, ln=None, want_stats=False, shared_w=False,
                       bf16=False):
    """y = LN?(relu?(x W_g^T + b_g) + residual) for the rows of group g, ONE launch (selfocc_linear_fwd_grouped).

    x (T, K) with T = sum(sizes); weight [G][N][K] (any shape with that layout: (G, N, K), (G * N, K)) with bias [G][N] | None —
    or, with ``shared_w``, (N, K) / (N) shared by the groups;
    residual (T, N) | None; ln = (gamma, beta, eps) with gamma / beta (G, N) per group or (N) shared.
    -> y (T, N), or (y, y_pre, mean, rstd) with ``want_stats``."""
    return _linear_fwd(x, weight, bias, relu, residual, ln, None, want_stats, sizes, shared_w, bf16)


def linear_fwd_heads_supported(rows, n_out, n_in, nv, bf16=False):
    return (n_out >= 96 and n_out % 96 == 0 and nv >= 16 and rows % nv == 0 and rows * n_out < 2 ** 31
            and linear_fwd_supported(rows, n_out, n_in))


def linear_fwd_heads(x, weight, bias, nv, relu=False, bf16=False):
    """value_proj with a head-major result (csrc/linear_fwd.hip, selfocc_linear_fwd_heads): x (B * nv, K), weight
    (G * 96, K) -> (G, B, 6, nv, 16) float32 — per group the (bs, heads, nv, d) tensor the fused / camera-loop MSDA ops
    take with ``head_major=True``."""
    _need_cuda(x, "linear_fwd_heads")
    T, K = x.shape
    N = weight.shape[0]
    assert weight.shape[1] == K and x.dtype == torch.float32 and weight.dtype == torch.float32
    x, weight = x.contiguous(), weight.contiguous()
    if bias is not None:
        bias = bias.contiguous()
    y = torch.empty(N // 96 if N % 96 == 0 else 0, T // nv if nv else 0, 6, nv, 16, device=x.device, dtype=torch.float32)
    check(lib().selfocc_linear_fwd_heads(ptr(x), ptr(weight), ptr(bias), ptr(y), T, N, K, int(nv),
                                         (LINEAR_RELU if relu else 0) | (LINEAR_BF16X1 if bf16 else 0), current_stream(x.device)),
          "selfocc_linear_fwd_heads")
    return y
