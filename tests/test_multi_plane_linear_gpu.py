"""GPU: the grouped tall-Linear passes behind MultiPlaneFFN — selfocc_linear_fwd_grouped / _dgrad_grouped / _wgrad_grouped
(csrc/linear_fwd.hip, csrc/linear.hip): one launch over the concatenated planes, each row served with the weights of the group
it lies in.

Exactness by the method of tests/linear_cases.py: integer-valued operands for which any accumulation order is exact, every
group drawn from its OWN seed — a row served with another group's weights, or a chunk that straddles a group, is an integer
error at a known place; the result must EQUAL the float64 product per group.  Row splits put the group boundaries inside, at and
next to the 16- / 32-row tiles and the wgrad chunks; empty groups give dw = db = 0 exactly; backward passes are run twice and
must be bit-identical; one group must equal the ungrouped entry bit for bit.  Epilogues (bias, ReLU, residual, LayerNorm with
per-group gamma / beta, grouped and shared W) against float64 at the bounds of tests/test_linear_gpu.py."""
import pytest
import torch

import linear_cases as lc

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
SPLITS = [(1, 1, 1), (16, 16, 16), (17, 15, 33), (31, 0, 64), (0, 5, 0), (257, 63, 65), (2065, 201, 201), (40,),
          (16400, 37, 70)]       # the last: above the 16 384 rows at which the forward takes its bf16 x 3 kernels
SHAPES = [(192, 96), (96, 192), (64, 32)]          # (N, K): the FFN's two Linears at 96 / 192, and a narrow one
IDS = dict(ids=lambda s: 'x'.join(map(str, s)))


def _rows(sizes):
    return [(g, n) for g, n in enumerate(sizes) if n > 0]


def _fwd_inputs(family, sizes, N, K):
    T = sum(sizes)
    x, want = torch.zeros(T, K), torch.zeros(T, N, dtype=torch.float64)
    w, bias = torch.zeros(len(sizes), N, K), torch.zeros(len(sizes), N)
    o = 0
    for g, n in enumerate(sizes):
        # (an empty group still gets weights: nothing may read them)
        xg, wg, wantg, _ = lc.make_pair(family, max(n, 1), N, K, seed=('fwd', g))
        w[g], bias[g] = wg, lc.small_ints((N,), 1000, seed=('b', g, N, K))
        if n:
            x[o:o + n], want[o:o + n] = xg[:n], wantg[:n] + bias[g].double()
        o += n
    res = lc.small_ints((T, N), 1000, seed=('r', T, N, K))
    return x, w, bias, res, want


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("sizes", SPLITS, **IDS)
def test_grouped_forward_is_exact(hip, sizes, N, K, family):
    from selfocc_amd.linear import linear_fwd_grouped, linear_fwd_grouped_supported
    assert linear_fwd_grouped_supported(sizes, N, K)
    x, w, bias, res, want = _fwd_inputs(family, sizes, N, K)
    xd, wd, bd, rd = x.to(D0), w.to(D0), bias.to(D0), res.to(D0)
    y = linear_fwd_grouped(xd, sizes, wd, bd)
    assert torch.equal(y.cpu().double(), want), (y.cpu().double() - want).abs().max().item()
    y = linear_fwd_grouped(xd, sizes, wd, bd, relu=True, residual=rd)        # ReLU before the residual, as FFN does
    assert torch.equal(y.cpu().double(), want.clamp_min(0) + res.double())
    y = linear_fwd_grouped(xd, sizes, wd, None, residual=rd)
    o = 0
    for g, n in enumerate(sizes):
        assert torch.equal(y[o:o + n].cpu().double(), want[o:o + n] - bias[g].double() + res[o:o + n].double()), g
        o += n


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("sizes", SPLITS, **IDS)
def test_grouped_dgrad_is_exact_and_deterministic(hip, sizes, N, K, family):
    from selfocc_amd.linear import linear_dgrad_grouped, linear_dgrad_grouped_supported, dgrad_supported
    if not dgrad_supported(max(sum(sizes), 1), N, K):          # K = 32: the route covers 96 / 192 / 288 / 384 input features
        assert not linear_dgrad_grouped_supported(sizes, N, K)
        return
    assert linear_dgrad_grouped_supported(sizes, N, K)
    T = sum(sizes)
    dy, want, w = torch.zeros(T, N), torch.zeros(T, K, dtype=torch.float64), torch.zeros(len(sizes), N, K)
    o = 0
    for g, n in enumerate(sizes):
        dyg, wt, wantg, _ = lc.make_pair(family, max(n, 1), K, N, seed=('dgrad', g))
        w[g] = wt.t()
        if n:
            dy[o:o + n], want[o:o + n] = dyg[:n], wantg[:n]
        o += n
    dx = linear_dgrad_grouped(dy.to(D0), w.to(D0), sizes)
    assert torch.equal(dx.cpu().double(), want), (dx.cpu().double() - want).abs().max().item()
    assert torch.equal(linear_dgrad_grouped(dy.to(D0), w.to(D0), sizes), dx)


@pytest.mark.parametrize("family", lc.FAMILIES + ('D',))
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("sizes", SPLITS, **IDS)
def test_grouped_wgrad_is_exact_and_deterministic(hip, sizes, N, K, family):
    from selfocc_amd.linear import linear_wgrad_grouped, linear_wgrad_grouped_supported
    assert linear_wgrad_grouped_supported(sizes, N, K)
    T, G = sum(sizes), len(sizes)
    dy, x = torch.zeros(T, N), torch.zeros(T, K)
    want_w, want_b = torch.zeros(G, N, K, dtype=torch.float64), torch.zeros(G, N, dtype=torch.float64)
    o = 0
    for g, n in _rows(sizes):
        if family == 'D':      # within its bound on T: |x| <= min(1022, (2^24 - 1) / T_g)
            xt, dyt, want = lc.make_wdense(n, N, K, seed=('wgrad', g))
        else:
            xt, dyt, want, _ = lc.make_pair(family, K, N, n, seed=('wgrad', g))
        o = sum(sizes[:g])
        dy[o:o + n], x[o:o + n] = dyt.t(), xt.t()
        want_w[g], want_b[g] = want.t(), dyt.double().sum(1)
    dw, db = linear_wgrad_grouped(dy.to(D0), x.to(D0), sizes)
    assert torch.equal(dw.cpu().double(), want_w), (dw.cpu().double() - want_w).abs().max().item()
    assert torch.equal(db.cpu().double(), want_b)
    for g, n in enumerate(sizes):
        if n == 0:      # exact zeros, not a left-over of the workspace
            assert torch.equal(dw[g].cpu(), torch.zeros(N, K)) and torch.equal(db[g].cpu(), torch.zeros(N)), g
    dw2, db2 = linear_wgrad_grouped(dy.to(D0), x.to(D0), sizes)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("T,N,K", [(2467, 192, 96), (2467, 96, 192), (20001, 192, 96), (20001, 96, 192), (70, 64, 32), (20001, 64, 32)])
def test_one_group_is_the_ungrouped_entry_bit_for_bit(hip, T, N, K):
    """the same launch plan, blocks, rows per wave and summation order (20 001 rows: the bf16 x 3 routes of the forward)"""
    from selfocc_amd import linear as L
    g = torch.Generator().manual_seed(T + N + K)
    x = torch.randn(T, K, generator=g).to(D0)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(D0)
    b = torch.randn(N, generator=g).to(D0)
    res = torch.randn(T, N, generator=g).to(D0)
    dy = torch.randn(T, N, generator=g).to(D0)
    assert torch.equal(L.linear_fwd_grouped(x, (T,), w, b, relu=True, residual=res), L.linear_fwd(x, w, b, relu=True, residual=res))
    if N <= 96:
        gamma, beta = (1 + 0.1 * torch.randn(N, generator=g)).to(D0), (0.1 * torch.randn(N, generator=g)).to(D0)
        a = L.linear_fwd_grouped(x, (T,), w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True)
        c = L.linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True)
        for p, q in zip(a, c):
            assert torch.equal(p, q)
    dw, db = L.linear_wgrad_grouped(dy, x, (T,))
    dw0, db0 = L.linear_wgrad(dy, x)
    assert torch.equal(dw[0], dw0) and torch.equal(db[0], db0)
    if L.dgrad_supported(T, N, K):
        assert torch.equal(L.linear_dgrad_grouped(dy, w[None], (T,)), L.linear_dgrad(dy, w))


@pytest.mark.parametrize("shared_w", [False, True], ids=['grouped_w', 'shared_w'])
@pytest.mark.parametrize("N,K", [(96, 192), (96, 96), (64, 32)])
@pytest.mark.parametrize("sizes", SPLITS + [(16500, 700, 801)], **IDS)
def test_grouped_layernorm_epilogue_vs_float64(hip, sizes, N, K, shared_w):
    """Linear + bias + residual + LayerNorm with per-group gamma / beta in one launch, with per-group W and with ONE W shared by
    the groups (a shared projection followed by a per-plane norm); the saved statistics; the bounds of
    tests/test_linear_gpu.py::test_linear_fwd_layernorm_epilogue"""
    from selfocc_amd.linear import linear_fwd_grouped
    T, G = sum(sizes), len(sizes)
    g = torch.Generator().manual_seed(T * 3 + N + K)
    x = torch.randn(T, K, generator=g)
    w = torch.randn(1 if shared_w else G, N, K, generator=g) / K ** 0.5
    b = torch.randn(1 if shared_w else G, N, generator=g)
    res = torch.randn(T, N, generator=g)
    gamma = 1 + 0.1 * torch.randn(G, N, generator=g)                  # a wrong group's gamma is an O(0.1) error, its beta O(1)
    beta = 0.1 * torch.randn(G, N, generator=g) - 0.5 * torch.arange(G)[:, None]
    pre, want, o = torch.zeros(T, N, dtype=torch.float64), torch.zeros(T, N, dtype=torch.float64), 0
    for gi, n in enumerate(sizes):
        wi = 0 if shared_w else gi
        pre[o:o + n] = x[o:o + n].double() @ w[wi].double().t() + b[wi].double() + res[o:o + n].double()
        want[o:o + n] = torch.nn.functional.layer_norm(pre[o:o + n], (N,), gamma[gi].double(), beta[gi].double(), 1e-5)
        o += n
    wd, bd = (w[0], b[0]) if shared_w else (w, b)
    y, y_pre, mean, rstd = linear_fwd_grouped(x.to(D0), sizes, wd.to(D0), bd.to(D0), residual=res.to(D0),
                                              ln=(gamma.to(D0), beta.to(D0), 1e-5), want_stats=True, shared_w=shared_w)
    assert (y_pre.cpu().double() - pre).abs().max().item() < 4e-6 * max(1.0, pre.abs().max().item())
    assert (y.cpu().double() - want).abs().max().item() < 2e-5
    assert (mean.cpu().double() - pre.mean(1)).abs().max().item() < 1e-5
    assert (rstd.cpu().double() - 1 / (pre.var(1, unbiased=False) + 1e-5).sqrt()).abs().max().item() < 1e-4
    y2 = linear_fwd_grouped(x.to(D0), sizes, wd.to(D0), bd.to(D0), residual=res.to(D0), ln=(gamma.to(D0), beta.to(D0), 1e-5),
                            shared_w=shared_w)
    assert torch.equal(y, y2)
