"""Inputs on which the tall-Linear kernels (csrc/linear_fwd.hip, csrc/linear.hip) must be BIT-EXACT, the case lists of
tests/test_linear_exact_gpu.py, a CPU emulation of the six-term bfloat16 scheme and a mirror of the three launch plans.

The method.  Every operand value is an integer multiple of one power of two (the `unit`; 1 except where noted), and per output
element sum_r |x_i||w_j| over the six bf16 terms (plus |bias| + |residual|) stays below 2^24 units.  Then every product and every
partial sum, in ANY order, is an integer below 2^24: float32 accumulation is exact, and so is the three-way bfloat16 split as long
as the three dropped terms (x2 w3, x3 w2, x3 w3) vanish.  The kernel's result must EQUAL the float64 product; a mismatch is an
integer at a known (row, column), whose size names the plane or the reduction index that went wrong.

A product is out[d][s] = sum_r dense[d][r] * sparse[s][r]:
    forward   y  = x W^T      dense = x  (T, K),  sparse = W    (N, K)
    dgrad     dx = dy W       dense = dy (T, N),  sparse = W^T  (K, N)
    wgrad     dW = dy^T x     dense = x^T (K, T), sparse = dy^T (N, T)      (out is dW^T)

    family  dense                     sparse (per row)                  non-zero terms
    A       integers |m| < 2^20       <= 8 non-zeros, +-1               d1 s1, d2 s1, d3 s1
    B       {-1, 0, +1}               <= 8 non-zeros, |m| < 2^20        d1 s1, d1 s2, d1 s3
    C       integers |m| < 2^11       <= 4 non-zeros, |m| < 2^11        d1 s1, d2 s1, d1 s2, d2 s2
    D       (wgrad only) x non-zero integers |m| <= min(1022, (2^24 - 1) / T), dy dense +-1: every row decides every output

The non-zeros of sparse row s sit at ((s nnz + j) stride) mod R with stride coprime to R, close to R / nnz: a row's entries spread
over all k-steps, and the rows of a case together visit min(R, rows * nnz) DIFFERENT reduction indices — all of them wherever the
case has enough rows.  The LayerNorm cases scale the big operand by 2^-20 (2^-11 each in family C): powers of two change nothing
about exactness, and y_pre is O(1), so that mean / rstd / y can be held to the float64 tolerances of tests/test_linear_gpu.py
(a float32 `mean` of 1e5-sized rows cannot be within 1e-5 of anything)."""
import functools
import math

import torch

FAMILIES = ('A', 'B', 'C')
LIMIT = float(2 ** 24)
# the six products of the kernels, in the order they are accumulated (dense plane, sparse plane); small terms first
TERMS = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))
FAMILY_TERMS = {'A': {(1, 1), (2, 1), (3, 1)}, 'B': {(1, 1), (1, 2), (1, 3)}, 'C': {(1, 1), (2, 1), (1, 2), (2, 2)},
                'D': {(1, 1), (2, 1)}}


# ---- generators ----------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(hash_key(key))


def hash_key(key):
    h = 1469598103934665603
    for v in key:
        for ch in str(v):
            h = ((h ^ ord(ch)) * 1099511628211) % (1 << 61)
    return h


def _ints(g, shape, bound, nonzero=False):
    """uniform integers in [-(bound - 1), bound - 1] as float64 (without 0 if `nonzero`)"""
    if nonzero:
        m = torch.randint(1, bound, shape, generator=g, dtype=torch.int64)
        s = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
        return (m * s).double()
    return torch.randint(-(bound - 1), bound, shape, generator=g, dtype=torch.int64).double()


def sparse_stride(R, nnz):
    s = R // nnz + 1
    while math.gcd(s, R) != 1:
        s += 1
    return s


def sparse_positions(rows, R, nnz):
    """(rows, min(nnz, R)) reduction indices, distinct within a row; consecutive rows continue the same walk over Z_R"""
    nnz = min(nnz, R)
    idx = torch.arange(rows, dtype=torch.int64)[:, None] * nnz + torch.arange(nnz, dtype=torch.int64)[None, :]
    return (idx * sparse_stride(R, nnz)) % R


def make_pair(family, D, S, R, seed, forced=(), log2_unit=0):
    """dense (D, R), sparse (S, R) float32 CPU tensors, `want` (D, S) float64 and the sparse positions (S, nnz).
    forced: reduction indices written over the first entries of the sparse rows, one each, in turn (wgrad: the rows at the edges
    of the launch plan's blocks)."""
    g = _gen('pair', family, D, S, R, seed)
    nnz = 4 if family == 'C' else 8
    pos = sparse_positions(S, R, nnz)
    if forced:
        f = torch.tensor(list(forced), dtype=torch.int64)
        pos[:, 0] = f[torch.arange(S) % len(f)]
    if family == 'A':
        dense = _ints(g, (D, R), 2 ** 20)
        vals = _ints(g, pos.shape, 2, nonzero=True)
        ud, us = log2_unit, 0
    elif family == 'B':
        dense = _ints(g, (D, R), 2)
        vals = _ints(g, pos.shape, 2 ** 20, nonzero=True)
        ud, us = 0, log2_unit
    elif family == 'C':
        dense = _ints(g, (D, R), 2 ** 11)
        vals = _ints(g, pos.shape, 2 ** 11, nonzero=True)
        ud, us = log2_unit // 2, log2_unit - log2_unit // 2
    else:
        raise ValueError(family)
    sparse = torch.zeros(S, R, dtype=torch.float64)
    sparse.scatter_(1, pos, vals)              # a forced index that repeats one of the row's own just overwrites it
    dense, sparse = dense * 2.0 ** ud, sparse * 2.0 ** us
    want = dense @ sparse.t()
    return dense.float(), sparse.float(), want, pos


def make_wdense(T, N, K, seed):
    """family D: dy (T, N) in {-1, +1}, x (T, K) non-zero integers -> dense = x^T (K, T), sparse = dy^T (N, T), want (K, N)"""
    g = _gen('wdense', T, N, K, seed)
    bound = min(1022, (2 ** 24 - 1) // T)
    x = _ints(g, (T, K), bound + 1, nonzero=True)
    dy = _ints(g, (T, N), 2, nonzero=True)
    return x.t().contiguous().float(), dy.t().contiguous().float(), x.t() @ dy


def small_ints(shape, bound, seed, log2_unit=0):
    """bias / residual: integers |m| < bound in the case's unit, float32"""
    return (_ints(_gen('small', tuple(shape), bound, seed), shape, bound) * 2.0 ** log2_unit).float()


# ---- CPU emulation of the kernels' arithmetic ---------------------------------------------------------------------------------
def split3(t):
    """float32 -> three float32 tensors holding bfloat16 values (round to nearest even), as so_split3 in the kernels"""
    b1 = t.bfloat16().float()
    r1 = t - b1
    b2 = r1.bfloat16().float()
    b3 = (r1 - b2).bfloat16().float()
    return b1, b2, b3


def emulate_b3(dense, sparse, seed=0, drop=None, shift3=None, omit=None):
    """The six-term scheme in float32: k-steps of 32 in a shuffled order, the terms of a step in the kernels' order, every
    partial sum rounded to float32.  Faults for the negative controls: drop = a (dense plane, sparse plane) term left out;
    shift3 = 'dense' | 'sparse': that operand's third plane moved by one reduction index; omit = one reduction index skipped."""
    R = dense.shape[1]
    Rp = (R + 31) // 32 * 32
    if Rp != R:
        dense = torch.nn.functional.pad(dense, (0, Rp - R))
        sparse = torch.nn.functional.pad(sparse, (0, Rp - R))
    if omit is not None:
        dense = dense.clone()
        dense[:, omit] = 0.0
    d, s = list(split3(dense)), list(split3(sparse))
    if shift3 == 'dense':
        d[2] = torch.roll(d[2], 1, 1)
    elif shift3 == 'sparse':
        s[2] = torch.roll(s[2], 1, 1)
    acc = torch.zeros(dense.shape[0], sparse.shape[0], dtype=torch.float32)
    order = torch.randperm(Rp // 32, generator=_gen('order', seed, Rp)).tolist()
    for ks in order:
        sl = slice(32 * ks, 32 * ks + 32)
        for (i, j) in TERMS:
            if (i, j) == drop:
                continue
            acc = acc + d[i - 1][:, sl] @ s[j - 1][:, sl].t()
    return acc


def contract(dense, sparse, extra=None, log2_unit=0):
    """What the exactness argument needs, measured on the data: (all values integers in the unit, the largest
    sum_r sum_terms |d_i||s_j| (+ |extra|) per output in units, exact split, the set of non-zero terms, dropped terms zero)."""
    d, s = split3(dense), split3(sparse)
    exact = torch.equal(d[0] + d[1] + d[2], dense) and torch.equal(s[0] + s[1] + s[2], sparse)
    live = {(i, j) for i in (1, 2, 3) for j in (1, 2, 3) if bool(d[i - 1].any()) and bool(s[j - 1].any())}
    mass = sum(d[i - 1].abs().double() @ s[j - 1].abs().double().t() for (i, j) in TERMS)
    if extra is not None:
        mass = mass + extra.double()
    scale = 2.0 ** -log2_unit
    ints = all(bool(torch.equal((t.double() * scale).round(), t.double() * scale)) for t in (dense, sparse))
    return dict(ints=ints, mass=float(mass.max()) * scale, exact=exact, live=live,
                dropped_zero=not (live - set(TERMS)))


# ---- mirror of the launch plans (written from the launchers in csrc/linear_fwd.hip and csrc/linear.hip) ----------------------------
def fwd_plan(T, N, K, ln=False, b3_env=True):
    """One dict per launch of selfocc_linear_fwd: the main launch over the full 96-column blocks, then the tail launch."""
    assert K in (32, 64, 96, 128, 192) and T >= 1 and N >= 1 and (not ln or N <= 96)
    ncb_full = N // 96
    tail_cols = N - 96 * ncb_full
    tail_nt = (tail_cols + 31) // 32
    out = []
    for p in range(2):
        nt = 3 if p == 0 else tail_nt
        ncb = ncb_full if p == 0 else 1
        col0 = 0 if p == 0 else 96 * ncb_full
        if (p == 0 and ncb_full == 0) or (p == 1 and tail_nt == 0):
            continue
        cols = min(N - col0, 96 * ncb)
        d = dict(nt=nt, ncb=ncb, col0=col0, ln=ln, full_cols=(cols - 96 * (ncb - 1)) >= 32 * nt)
        if b3_env and K == 192 and T >= 16384:
            nwt = (T + 15) // 16
            groups = min(max(1, 256 // ncb), (nwt + 7) // 8)
            d.update(route='b3_k192', ks=6, waves=8, h=1, groups=groups, nwt=nwt,
                     lds=3 * nt * 32 * (K + 8) * 2, inst=('b3', 6, ln, nt, 8, 1))
        elif b3_env and K <= 128 and (T >= 16384 or N >= 384):
            lds = 3 * nt * 32 * (K + 8) * 2
            per_cu = max(1, min(2, (160 * 1024) // (lds + 512)))
            h = 1 if N <= 192 else 2
            nwt = (T + 16 * h - 1) // (16 * h)
            groups = min(max(1, 256 * per_cu // ncb), (nwt + 3) // 4)
            d.update(route='b3', ks=K // 32, waves=4, h=h, groups=groups, nwt=nwt, lds=lds, inst=('b3', K // 32, ln, nt, 4, h))
        else:
            lds = nt * 32 * (K + 4) * 4
            per_cu = max(1, min(2, (160 * 1024) // (lds + 512)))
            nwt = (T + 15) // 16
            groups = min(max(1, 256 * per_cu // ncb), (nwt + 3) // 4)
            d.update(route='f32', kq=K // 4, waves=4, h=1, groups=groups, nwt=nwt, lds=lds, inst=('f32', K // 4, ln, nt, 4))
        d['second_tile'] = d['waves'] * d['groups'] < d['nwt']         # some wave walks on to a second tile (x prefetch live)
        out.append(d)
    return out


def wgrad_plan(T, N, K, b3_env=True):
    """so_wgrad_plan + the kernel selfocc_linear_wgrad launches for it"""
    if K == 96:
        kt, ntw = 3, ((1 if (N <= 96 or T < 16384) else 2) if b3_env else 3)
    elif K == 192:
        kt, ntw = 6, (1 if b3_env else 2)
    elif K == 32:
        kt, ntw = 1, 4
    elif K == 64:
        kt, ntw = 2, (2 if b3_env else 4)
    elif K == 128:
        kt, ntw = 4, 3
    else:
        raise ValueError(K)
    nt = (N + 31) // 32
    ngroups = (nt + ntw - 1) // ntw
    chunks = max(1, min(512 // max(1, min(ngroups, 512)), (T + 63) // 64))
    chunks = min(chunks, 128)
    rpb = (T + chunks - 1) // chunks
    rpb = (rpb + 7) // 8 * 8
    chunks = (T + rpb - 1) // rpb
    kernel = 'f32' if (K == 128 or not b3_env) else 'b3'
    return dict(kt=kt, ntw=ntw, ngroups=ngroups, chunks=chunks, rows_per_block=rpb, nt=nt, inst=(kernel, kt, ntw),
                workspace=chunks * (N * K + N) * 4)


def dgrad_plan(T, N, K):
    assert N >= 8 and N % 8 == 0 and N <= 4096 and K in (96, 192, 288, 384)
    npad = (N + 95) // 96 * 96
    ncb = K // 96
    nwt = (T + 31) // 32
    groups = min(max(1, 512 // ncb), (nwt + 3) // 4)
    return dict(npad=npad, nchunks=npad // 96, ncb=ncb, groups=groups, nwt=nwt, presplit=npad != 96,
                second_tile=4 * groups < nwt, workspace=3 * K * npad * 2, inst=('dgrad', 'presplit' if npad != 96 else 'inkernel', ncb))


def wgrad_forced_rows(T, N, K, b3_env=True):
    """row 0, row T - 1 and the first and last row of a block in the middle of the plan"""
    p = wgrad_plan(T, N, K, b3_env)
    blk = p['chunks'] // 2
    rows = {0, T - 1, min(T - 1, blk * p['rows_per_block']), min(T, (blk + 1) * p['rows_per_block']) - 1}
    return sorted(rows)


# ---- the case lists of tests/test_linear_exact_gpu.py ---------------------------------------------------------------------------
KS4 = (32, 64, 96, 128)
# (T, N, K, ln)
FWD_B3_H2 = [(70, N, K, False) for K in KS4 for N in (384, 404, 424, 454)] + [(16401, 404, K, False) for K in KS4]
FWD_B3_H1 = ([(16401, N, K, False) for K in KS4 for N in (96, 192, 116, 20, 40, 70)]
             + [(16401, N, K, True) for K in KS4 for N in (96, 70, 40, 20)]
             + [(32801, 96, 96, False), (32801, 96, 96, True)])
FWD_B3_K192 = [(16401, N, 192, False) for N in (96, 116, 136, 40, 20)] + [(16401, N, 192, True) for N in (96, 70, 40, 20)]
FWD_F32 = ([(T, N, K, False) for K in KS4 + (192,) for T in (70, 1) for N in (96, 116, 136, 20)]
           + [(T, N, K, True) for K in KS4 + (192,) for T in (70, 1) for N in (96, 40, 20)])
FWD_CASES = FWD_B3_H2 + FWD_B3_H1 + FWD_B3_K192 + FWD_F32
# one N % 4 == 0 shape per route for the epilogue variants (strided out / residual, aligned and offset by 7 floats; ReLU; no bias)
FWD_VARIANTS = {'b3_h2': (70, 404, 96), 'b3_h1': (16401, 116, 64), 'b3_k192': (16401, 116, 192), 'f32': (70, 116, 128)}
# (B, nv, G, K) of linear_fwd_heads
HEADS_CASES = [(B, nv, G, K) for K in (96, 192) for (B, nv, G) in ((3, 5467, 1), (3, 5467, 4), (3, 17, 1), (2, 35, 2))]
# (T, N, K) of wgrad
WGRAD_CASES = [(70, 96, 96), (1000, 216, 96), (16401, 70, 96), (16401, 216, 96), (16401, 400, 96), (1000, 96, 192), (16401, 40, 192),
               (1000, 33, 32), (1000, 160, 32), (1003, 33, 32), (1000, 70, 64), (1003, 70, 64), (1000, 33, 128), (70, 96, 128),
               (1, 5, 96), (1, 33, 32), (1, 33, 64), (1, 33, 128), (1, 33, 192)]
# (T, N = reduced, K) of dgrad
DGRAD_CASES = ([(T, N, K) for K in (96, 192, 288, 384) for N in (8, 40, 96, 104, 200, 392) for T in (1, 70)]
               + [(16401, 96, 384), (16401, 200, 384), (65601, 104, 96)])
# SELFOCC_LINEAR_B3=0 (child process): shapes the default sends to the bf16 kernels
CHILD_FWD = [(70, 404, 32), (70, 404, 64), (70, 404, 96), (70, 404, 128), (16401, 116, 192)]
CHILD_WGRAD = [(1000, 160, 32), (1000, 70, 64), (1000, 216, 96), (1000, 96, 192)]

# every instantiation the lists above must reach (tests/test_linear_cases_cpu.py compares the sets)
FWD_INSTANCES = ({('b3', ks, False, nt, 4, 2) for ks in (1, 2, 3, 4) for nt in (1, 2, 3)}
                 | {('b3', ks, ln, nt, 4, 1) for ks in (1, 2, 3, 4) for ln in (False, True) for nt in (1, 2, 3)}
                 | {('b3', 6, ln, nt, 8, 1) for ln in (False, True) for nt in (1, 2, 3)}
                 | {('f32', kq, ln, nt, 4) for kq in (8, 16, 24, 32, 48) for ln in (False, True) for nt in (1, 2, 3)})
WGRAD_INSTANCES = {('b3', 1, 4), ('b3', 2, 2), ('b3', 3, 1), ('b3', 3, 2), ('f32', 4, 3), ('b3', 6, 1)}
WGRAD_CHILD_INSTANCES = {('f32', 1, 4), ('f32', 2, 4), ('f32', 3, 3), ('f32', 6, 2)}
DGRAD_INSTANCES = {('dgrad', s, ncb) for s in ('inkernel', 'presplit') for ncb in (1, 2, 3, 4)}

LN_LOG2_UNIT = -20


@functools.lru_cache(maxsize=4)
def fwd_case(family, T, N, K, ln=False):
    """x (T, K), w (N, K), bias (N), residual (T, N), want = x w^T in float64, positions, log2 of the unit"""
    u = LN_LOG2_UNIT if ln else 0
    x, w, want, pos = make_pair(family, T, N, K, seed=1, log2_unit=u)       # bias / residual live in the product's unit
    bias = small_ints((N,), 2 ** 19 if ln else 1000, seed=(T, N, K, 'b'), log2_unit=u)
    res = small_ints((T, N), 2 ** 19 if ln else 1000, seed=(T, N, K, 'r'), log2_unit=u)
    return dict(x=x, w=w, bias=bias, res=res, want=want, pos=pos, log2_unit=u)


@functools.lru_cache(maxsize=4)
def dgrad_case(family, T, N, K):
    """dy (T, N), w (N, K), want = dy w in float64"""
    dy, wt, want, pos = make_pair(family, T, K, N, seed=2)
    return dict(dy=dy, w=wt.t().contiguous(), want=want, pos=pos, dense=dy, sparse=wt)


@functools.lru_cache(maxsize=4)
def wgrad_case(family, T, N, K, b3_env=True):
    """dy (T, N), x (T, K), want_w = dy^T x (N, K) and want_b = colsum(dy) in float64; family 'D' is the dense one"""
    if family == 'D':
        xt, dyt, want = make_wdense(T, N, K, seed=3)
        pos, forced = None, []
    else:
        forced = wgrad_forced_rows(T, N, K, b3_env)
        xt, dyt, want, pos = make_pair(family, K, N, T, seed=3, forced=forced)
    return dict(dy=dyt.t().contiguous(), x=xt.t().contiguous(), want_w=want.t().contiguous(), want_b=dyt.double().sum(1), pos=pos,
                forced=forced, dense=xt, sparse=dyt)
