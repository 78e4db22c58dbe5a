"""Inputs, case lists and launch-plan mirrors for the one-product bfloat16 mode of the tall-Linear kernels (SO_LINEAR_BF16X1 /
bricks.LINEAR_BF16): the helper of tests/test_linear_bf16_cpu.py and tests/test_linear_bf16_gpu.py.

The contract of the mode (include/selfocc_hip.h): a flagged pass computes what the default computes on bf16_rne(a), bf16_rne(b).
The method is that of tests/linear_cases.py with ONE plane.  Every operand value is an integer (times one power of two, the unit),
and per output element sum_r |a^_r||b^_r| + |bias| + |residual| stays below 2^24 units — then every product of the ROUNDED operands
and every partial sum, in any order, is an integer below 2^24, float32 accumulation is exact, and the kernel must EQUAL the float64
product of `t.bfloat16().double()`.  A product is out[d][s] = sum_r dense[d][r] * sparse[s][r], as in linear_cases.py.

    family  dense                   sparse (per row)                         what it decides
    R       integers |m| < 2^10     <= 8 non-zeros, |m| < 2^10 (mass <= 2^23)  the rounding is done, and is round-to-nearest-even:
                                                                             TIES below are written into both operands of every case
    E       integers 1 <= |m| <= 15 dense, 1 <= |m| <= 15 (bf16-exact)       every reduction index of every output
            wgrad: x |m| <= 15, dy dense +-1, T <= 16 401 (mass <= 16 401 * 15)

TIES: 257 and 259 lie exactly between two bfloat16 (256 | 258 | 260), 514 and 518 between (512 | 516 | 520); 513 and 771 are plain
roundings.  RNE gives 256, 260, 512, 520, 512, 772; truncation 256, 258, 512, 516, 512, 768; round-half-away 258, 260, 516, 520, 512,
772 — each wrong rule moves an integer at a known position."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_cases as lc  # noqa: E402
from linear_cases import _ints, sparse_positions, hash_key, small_ints  # noqa: E402,F401

LIMIT = float(2 ** 24)
TIES = (257, 259, 514, 518, 513, 771)
LN_LOG2_UNIT = lc.LN_LOG2_UNIT
FAMILIES = ('R', 'E')


def _gen(*key):
    return torch.Generator().manual_seed(hash_key(('bf16',) + key))


def rne(t):
    """the float64 values of the round-to-nearest-even bfloat16 of a float32 tensor"""
    return t.float().bfloat16().double()


def trunc_bf16(t):
    """bfloat16 by truncation (the wrong rule of the CPU negative control)"""
    return (t.float().view(torch.int32) & ~0xFFFF).view(torch.float32).double()


def half_away_bf16(t):
    """bfloat16 by round-half-away-from-zero (the other wrong rule)"""
    return ((t.float().view(torch.int32) + 0x8000) & ~0xFFFF).view(torch.float32).double()


def make_pair(family, D, S, R, seed, forced=(), log2_unit=0):
    """dense (D, R), sparse (S, R) float32, want = rne(dense) rne(sparse)^T and plain = dense sparse^T in float64, positions.
    forced: reduction indices written over the first entry of the sparse rows in turn (wgrad: the rows at the plan's block edges)."""
    g = _gen('pair', family, D, S, R, seed)
    if family == 'R':
        dense = _ints(g, (D, R), 2 ** 10)
        pos = sparse_positions(S, R, 8)
        if forced:
            f = torch.tensor(list(forced), dtype=torch.int64)
            pos[:, 0] = f[torch.arange(S) % len(f)]
        vals = _ints(g, pos.shape, 2 ** 10, nonzero=True)
        # the ties: dense[d][(d + i) % R] = +-TIES[i] (every row, a diagonal band: every reduction index where D >= R), and the
        # first entry of sparse row s is +-TIES[s % 6]
        ties = torch.tensor(TIES, dtype=torch.float64)
        for i in range(min(len(TIES), R)):
            rows = torch.arange(D)
            dense[rows, (rows + i) % R] = ties[i] * (1 - 2 * (rows % 2)).double()
        srow = torch.arange(S)
        vals[:, 0] = ties[srow % len(TIES)] * (1 - 2 * ((srow // len(TIES)) % 2)).double()
        sparse = torch.zeros(S, R, dtype=torch.float64)
        sparse.scatter_(1, pos, vals)
    elif family == 'E':
        dense, sparse, pos = _ints(g, (D, R), 16, nonzero=True), _ints(g, (S, R), 16, nonzero=True), None
    else:
        raise ValueError(family)
    dense = (dense * 2.0 ** log2_unit).float()
    sparse = sparse.float()
    return dense, sparse, rne(dense) @ rne(sparse).t(), dense.double() @ sparse.double().t(), pos


def contract(family, dense, sparse, extra=None, log2_unit=0):
    """measured on the data: integers in the unit; the largest sum_r |d^||s^| (+ extra) per output, in units; whether the rounding
    changes a value of each operand"""
    scale = 2.0 ** -log2_unit
    ints = all(bool(torch.equal((t.double() * scale).round(), t.double() * scale)) for t in (dense, sparse))
    mass = rne(dense).abs() @ rne(sparse).abs().t()
    if extra is not None:
        mass = mass + extra.double()
    return dict(ints=ints, mass=float(mass.max()) * scale, rounds_dense=not torch.equal(rne(dense), dense.double()),
                rounds_sparse=not torch.equal(rne(sparse), sparse.double()))


# ---- mirrors of the flagged launch plans (written from so_linear_fwd_launch / so_wgrad_plan / so_linear_dgrad_launch) ----------------
def fwd_plan(T, N, K, ln=False, grp=False):
    """one dict per launch of a flagged selfocc_linear_fwd: always linear_fwd_b3_kernel<K / 32, LN, NT, WAVES, H, GRP, 1>
    (``grp``: the launch of selfocc_linear_fwd_grouped, T = all groups' rows; the instance tuple ends with GRP)"""
    assert K in (32, 64, 96, 128, 192) and T >= 1 and N >= 1 and (not ln or N <= 96)
    ncb_full = N // 96
    tail_nt = (N - 96 * ncb_full + 31) // 32
    out = []
    for p in range(2):
        nt = 3 if p == 0 else tail_nt
        ncb = ncb_full if p == 0 else 1
        if (p == 0 and ncb_full == 0) or (p == 1 and tail_nt == 0):
            continue
        k192 = K == 192
        half = k192 or N <= 192
        waves, h = (8 if k192 else 4), (1 if half else 2)
        nwt = (T + 16 * h - 1) // (16 * h)
        groups = min(max(1, 256 * (1 if k192 else 2) // ncb), (nwt + waves - 1) // waves)
        out.append(dict(nt=nt, ncb=ncb, ln=ln, waves=waves, h=h, groups=groups, nwt=nwt, lds=nt * 32 * (K + 8) * 2,
                        second_tile=waves * groups < nwt, inst=('x1', K // 32, ln, nt, waves, h, grp)))
    return out


def wgrad_plan(T, N, K, grp=False):
    """so_wgrad_plan with SO_LINEAR_BF16X1: always linear_wgrad_b3_kernel<KT, NTW, GRP, 1>, K = 128 included (``grp``: the plan of
    all T rows that selfocc_linear_wgrad_grouped cuts into per-group chunks; the instance tuple is (KT, NTW, grid z, GRP))"""
    two = not (N <= 96 or T < 16384)
    # K = 192 runs as two halves of three column tiles (grid z = 2: six tiles leave no registers for the prefetch), one tile row
    # like the default's K = 192 plan
    kt, ntw = {96: (3, 2 if two else 1), 192: (3, 1), 32: (1, 4), 64: (2, 2), 128: (4, 2 if two else 1)}[K]
    nt = (N + 31) // 32
    ngroups = (nt + ntw - 1) // ntw
    chunks = min(max(1, min(512 // max(1, min(ngroups, 512)), (T + 63) // 64)), 128)
    rpb = ((T + chunks - 1) // chunks + 7) // 8 * 8
    chunks = (T + rpb - 1) // rpb
    return dict(kt=kt, ntw=ntw, ngroups=ngroups, chunks=chunks, rows_per_block=rpb, inst=('x1', kt, ntw, 2 if K == 192 else 1, grp),
                workspace=chunks * (N * K + N) * 4)


def dgrad_plan(T, N, K, grp=False):
    p = lc.dgrad_plan(T, N, K)
    return dict(p, workspace=p['workspace'] // 3, inst=('x1',) + p['inst'][1:] + (grp,))


def wgrad_forced_rows(T, N, K):
    p = wgrad_plan(T, N, K)
    blk = p['chunks'] // 2
    return sorted({0, T - 1, min(T - 1, blk * p['rows_per_block']), min(T, (blk + 1) * p['rows_per_block']) - 1})


# ---- case lists ------------------------------------------------------------------------------------------------------------------
KS5 = (32, 64, 96, 128, 192)
# (T, N, K, ln): the smallest shapes at which each path can go wrong — one row and 70 rows (a partial 16 / 32-row tile after full
# ones), a tail of 20 columns alone, a full block, a block + tail, four blocks + tail on 32-row tiles; N = 40 / 424 add the
# two-tile tail (NT = 2) on 16- and 32-row tiles
FWD_SHORT = ([(T, N, K, False) for K in KS5 for T in (1, 70) for N in (20, 96, 116, 404)]
             + [(70, N, K, False) for K in KS5 for N in (40, 424)]
             + [(T, N, K, True) for K in KS5 for T in (1, 70) for N in (20, 96)] + [(70, 40, K, True) for K in KS5])
# long-T shapes per tile variant.  A wave walks on to a second tile, with the x prefetch live, once there are more tiles than the
# grid has waves (2 048): at 16 401 rows that holds for the 32-row tiles of four column blocks only (129 tiles per column block
# on 128 row blocks), so the 16-row variants come again at 32 801 rows (2 051 tiles)
FWD_LONG = [(16401, 404, 96, False), (16401, 116, 64, False), (16401, 116, 192, False), (16401, 96, 96, True),
            (32801, 116, 64, False), (32801, 116, 192, False), (32801, 96, 96, True)]
FWD_CASES = FWD_SHORT + FWD_LONG
FWD_VARIANTS = {'h2': (70, 404, 96), 'h1': (16401, 116, 64), 'k192': (16401, 116, 192)}
HEADS_CASES = [(B, nv, G, K) for K in (96, 192) for (B, nv, G) in ((3, 17, 1), (2, 35, 2), (3, 5467, 4))]
DGRAD_CASES = [(T, N, K) for K in (96, 192, 288, 384) for N in (8, 96, 104, 392) for T in (1, 70)] + [(16401, 200, 384)]
WGRAD_CASES = ([(70, 96, 96), (1000, 216, 96), (16401, 216, 96), (1000, 96, 192), (1000, 33, 32), (1003, 70, 64), (16401, 104, 128), (16401, 216, 192)]
               + [(1, 33, K) for K in KS5])
# grouped forms: an empty group in front, in the middle and at the end; a group of one row
GROUP_SIZES = [(0, 70, 1, 33), (16401, 0, 70)]
# (sizes, N, K): the two tables at N = K = 96 (with shared weights and the per-group LayerNorm), then the other grouped instance
# families — K = 192 (eight-wave forward, two-half wgrad, two-column-block dgrad), 32-row forward tiles with a tail (N > 192),
# a pre-rounded dgrad plane over three column blocks, the wgrad's KT = 4 with two tile rows and KT = 1 / 2
GROUPED_CASES = ([(s, 96, 96) for s in GROUP_SIZES]
                 + [((0, 70, 1, 33), 96, 192), ((0, 70, 1, 33), 404, 64), ((0, 70, 1, 33), 104, 288), ((16401, 0, 70), 104, 128),
                    ((0, 70, 1, 33), 40, 32)])


def grouped_passes(N, K):
    """which grouped passes a (N, K) case runs: forward and wgrad at K in 32 .. 192; the dgrad where its shape rule allows (K inputs
    in 96 .. 384 by 96, N % 8 == 0)"""
    return dict(fwd=K in KS5, dgrad=(K % 96 == 0 and 96 <= K <= 384 and N % 8 == 0), wgrad=K in KS5)

FWD_INSTANCES = ({('x1', ks, ln, nt, 4, 1) for ks in (1, 2, 3, 4) for ln in (False, True) for nt in (1, 2, 3)}
                 | {('x1', ks, False, nt, 4, 2) for ks in (1, 2, 3, 4) for nt in (1, 2, 3)}
                 | {('x1', 6, ln, nt, 8, 1) for ln in (False, True) for nt in (1, 2, 3)})
FWD_INSTANCES = {i + (False,) for i in FWD_INSTANCES}
# (KT, NTW, grid z, GRP)
WGRAD_INSTANCES = {('x1', 1, 4, 1, False), ('x1', 2, 2, 1, False), ('x1', 3, 1, 1, False), ('x1', 3, 2, 1, False), ('x1', 4, 1, 1, False),
                   ('x1', 4, 2, 1, False), ('x1', 3, 1, 2, False)}
DGRAD_INSTANCES = {('x1', s, ncb, False) for s in ('inkernel', 'presplit') for ncb in (1, 2, 3, 4)}
# the grouped (GRP = true) instantiations GROUPED_CASES must reach: each tile family of the forward (four waves x 16 rows with and
# without LayerNorm, four waves x 32 rows with a tail, eight waves), both dgrad forms, and the wgrad's plain, two-half and KT = 4 forms
GROUPED_FWD_INSTANCES = {('x1', 3, False, 3, 4, 1, True), ('x1', 3, True, 3, 4, 1, True), ('x1', 6, False, 3, 8, 1, True),
                         ('x1', 6, True, 3, 8, 1, True), ('x1', 2, False, 3, 4, 2, True), ('x1', 2, False, 1, 4, 2, True),
                         ('x1', 1, False, 2, 4, 1, True), ('x1', 4, False, 3, 4, 1, True), ('x1', 4, False, 1, 4, 1, True),
                         ('x1', 1, True, 2, 4, 1, True)}
GROUPED_WGRAD_INSTANCES = {('x1', 3, 1, 1, True), ('x1', 3, 1, 2, True), ('x1', 2, 2, 1, True), ('x1', 4, 2, 1, True), ('x1', 1, 4, 1, True)}
GROUPED_DGRAD_INSTANCES = {('x1', 'inkernel', 1, True), ('x1', 'inkernel', 2, True), ('x1', 'presplit', 3, True)}


@functools.lru_cache(maxsize=4)
def fwd_case(family, T, N, K, ln=False):
    """x (T, K), w (N, K), bias (N), residual (T, N); want = x^ w^^T, plain = x w^T in float64; log2 of the unit"""
    u = LN_LOG2_UNIT if ln else 0
    x, w, want, plain, pos = make_pair(family, T, N, K, seed=1, log2_unit=u)
    bias = small_ints((N,), 1000, seed=(T, N, K, 'b'), log2_unit=u)
    res = small_ints((T, N), 1000, seed=(T, N, K, 'r'), log2_unit=u)
    return dict(x=x, w=w, bias=bias, res=res, want=want, plain=plain, pos=pos, log2_unit=u)


@functools.lru_cache(maxsize=4)
def dgrad_case(family, T, N, K):
    """dy (T, N), w (N, K); want = dy^ w^, plain = dy w"""
    dy, wt, want, plain, pos = make_pair(family, T, K, N, seed=2)
    return dict(dy=dy, w=wt.t().contiguous(), want=want, plain=plain, dense=dy, sparse=wt)


@functools.lru_cache(maxsize=4)
def wgrad_case(family, T, N, K):
    """dy (T, N), x (T, K); want_w = dy^^T x^ (N, K), want_b = colsum(dy^), and the unrounded pair plain_w / plain_b"""
    if family == 'E':
        g = _gen('wdense', T, N, K)
        xt, dyt = _ints(g, (K, T), 16, nonzero=True).float(), _ints(g, (N, T), 2, nonzero=True).float()
        want, plain = rne(xt) @ rne(dyt).t(), xt.double() @ dyt.double().t()
    else:
        xt, dyt, want, plain, _ = make_pair(family, K, N, T, seed=3, forced=wgrad_forced_rows(T, N, K))
    return dict(dy=dyt.t().contiguous(), x=xt.t().contiguous(), want_w=want.t().contiguous(), plain_w=plain.t().contiguous(),
                want_b=rne(dyt).sum(1), plain_b=dyt.double().sum(1), dense=xt, sparse=dyt)


def grouped_dy(family, res):
    """dy (T, N) of the grouped wgrad cases from the signs of the case's residual: +-1 on every row (family E: |x| <= 15, mass <=
    15 T) or on every 16th row (family R: |x^| <= 2^10, mass <= 2^10 ceil(T / 16) < 2^21)"""
    dy = torch.sign(res) + (res == 0).float()
    if family == 'R':
        dy = dy * (torch.arange(res.shape[0]) % 16 == 0).float()[:, None]
    return dy


def sum_bound(a, b, R, extra=None):
    """|err| <= (R + 2) 2^-24 sum |terms| per element, the terms being the R exact products a^_r b^_r and, with ``extra``, the
    magnitudes added in the epilogue (|bias|, |residual|): float32 summation in ANY order rounds at most once per partial sum, relative
    2^-24, and every partial sum is bounded by the sum of magnitudes — R roundings in the accumulation, at most two in the epilogue"""
    mass = rne(a).abs() @ rne(b).abs().t()
    if extra is not None:
        mass = mass + extra.double()
    return (R + 2) * 2.0 ** -24 * mass


@functools.lru_cache(maxsize=2)
def grouped_case(family, sizes, N, K, ln=False):
    """one grouped case: x (T, K), residual (T, N), per-group weights ws (G, N, K) and biases bs (G, N); dy (T, N) dense for the
    grouped dgrad (reduction over N); dy_w (T, N) = grouped_dy for the grouped wgrad (reduction over a group's rows).  ``ln``: x,
    biases and residual in the 2^-20 unit."""
    T, G = sum(sizes), len(sizes)
    u = LN_LOG2_UNIT if ln else 0
    x, w0, _, _, _ = make_pair(family, T, N, K, seed=1, log2_unit=u)
    ws = torch.stack([w0] + [make_pair(family, 1, N, K, seed=10 + g)[1] for g in range(1, G)])
    bs = torch.stack([small_ints((N,), 1000, seed=('gb', g, N), log2_unit=u) for g in range(G)])
    res = small_ints((T, N), 1000, seed=(T, N, K, 'gr'), log2_unit=u)
    dy = make_pair(family, T, 1, N, seed=20)[0]
    return dict(x=x, ws=ws, bs=bs, res=res, dy=dy, dy_w=grouped_dy(family, res))
