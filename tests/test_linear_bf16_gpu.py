"""The one-product bfloat16 mode of the tall-Linear kernels (SO_LINEAR_BF16X1; ``bf16=True`` in selfocc_amd.linear,
bricks.LINEAR_BF16) on every P = 1 instantiation, BIT-EXACT against the float64 product of the ROUNDED operands.

The inputs (tests/linear_bf16_cases.py) are integers whose round-to-nearest-even bfloat16 values give products and partial sums
below 2^24 in any order, so float32 accumulation is exact and the flagged kernel must EQUAL rne(a) rne(b)^T: family R holds ties
and roundings in both operands (truncation or round-half-away give another integer), family E bf16-exact dense operands (every
reduction index decides every output).  tests/test_linear_bf16_cpu.py holds the contract of these inputs and the instantiations
the lists reach.  Negative control in every family-R test: the default mode (flags = 0) must NOT equal the rounded product — it
equals the unrounded one; a library that ignores the flag fails the first assertion of each test.  Only the LayerNorm epilogue's
own outputs carry the float64 tolerances of tests/test_linear_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want):
    g = got.double().cpu()
    if torch.equal(g, want):
        return True
    bad = (g != want).nonzero()
    i = tuple(bad[0].tolist())
    print(f"{len(bad)} of {want.numel()} elements differ; first at {i}: got {g[i].item()!r}, want {want[i].item()!r}, "
          f"largest difference {(g - want).abs().max().item()!r}")
    return False


def ln_params(N, key):
    g = torch.Generator().manual_seed(bc.hash_key(key))
    return (1 + 0.1 * torch.randn(N, generator=g)).cuda(), (0.1 * torch.randn(N, generator=g)).cuda()


def check_ln(y, mean, rstd, pre, gamma, beta):
    """the tolerances of tests/test_linear_gpu.py against float64, from the exact y_pre"""
    N = pre.shape[1]
    ref = torch.nn.functional.layer_norm(pre, (N,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    assert (y.double().cpu() - ref).abs().max().item() < 2e-5
    assert (mean.double().cpu() - pre.mean(1)).abs().max().item() < 1e-5
    assert (rstd.double().cpu() - 1 / (pre.var(1, unbiased=False) + 1e-5).sqrt()).abs().max().item() < 1e-4


# ---- forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,K,ln", bc.FWD_CASES)
def test_fwd_one_product_is_exact(hip, T, N, K, ln):
    """linear_fwd_b3_kernel<K / 32, LN, NT, WAVES, H, false, 1> on both families, flags = 0 as the negative control"""
    from selfocc_amd.linear import linear_fwd, linear_fwd_supported
    assert linear_fwd_supported(T, N, K, bf16=True)
    for fam in bc.FAMILIES:
        c = bc.fwd_case(fam, T, N, K, ln)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want, plain = c['want'] + c['bias'].double(), c['plain'] + c['bias'].double()
        if not ln:
            y = linear_fwd(x, w, b, bf16=True)
            assert same(y, want), (fam, T, N, K)
            assert torch.equal(linear_fwd(x, w, b, bf16=True), y)
            y0 = linear_fwd(x, w, b)
            assert same(y0, plain), (fam, 'default mode')
            assert (fam == 'E') == torch.equal(y0, y)
            continue
        gamma, beta = ln_params(N, (T, N, K, fam))
        res = c['res'].cuda()
        pre = want + c['res'].double()
        y, y_pre, mean, rstd = linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True, bf16=True)
        assert same(y_pre, pre), (fam, T, N, K)
        check_ln(y, mean, rstd, pre, gamma, beta)
        y2, p2, m2, r2 = linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True, bf16=True)
        assert torch.equal(y, y2) and torch.equal(y_pre, p2) and torch.equal(mean, m2) and torch.equal(rstd, r2)
        assert torch.equal(linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), bf16=True), y)
        p0 = linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True)[1]
        assert same(p0, plain + c['res'].double()) and (fam == 'E') == torch.equal(p0, y_pre)


@pytest.mark.parametrize("route", sorted(bc.FWD_VARIANTS))
def test_fwd_one_product_epilogue_variants_are_exact(hip, route):
    """no bias, ReLU, and relu(.) + residual into a column block of a wider buffer from a strided residual: 16-byte aligned row starts
    (the float4 epilogue) and offset by 7 floats (the scalar one).  Nothing outside the block moves."""
    from selfocc_amd.linear import linear_fwd
    T, N, K = bc.FWD_VARIANTS[route]
    for fam in bc.FAMILIES:
        c = bc.fwd_case(fam, T, N, K)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want = c['want'] + c['bias'].double()
        assert same(linear_fwd(x, w, None, bf16=True), c['want'])
        assert same(linear_fwd(x, w, b, relu=True, bf16=True), want.clamp_min(0))
        for off, pad in ((8, 8), (7, 3)):
            wide = torch.zeros(T, N + 40)
            wide[:, off:off + N] = c['res']
            res = wide.cuda()[:, off:off + N]                    # row stride N + 40
            buf = torch.full((T, 2 * N + pad), 7.0).cuda()
            out = buf[:, N:2 * N]
            assert (out.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0) == (off == 8)
            r = linear_fwd(x, w, b, relu=True, residual=res, out=out, bf16=True)
            assert r.data_ptr() == out.data_ptr()
            assert same(out, want.clamp_min(0) + c['res'].double()), (fam, off)
            assert torch.all(buf[:, :N] == 7.0) and torch.all(buf[:, 2 * N:] == 7.0)


@pytest.mark.parametrize("B,nv,G,K", bc.HEADS_CASES)
def test_fwd_heads_one_product_is_exact(hip, B, nv, G, K):
    """selfocc_linear_fwd_heads with the flag: (b, pix, g, h, c) -> (g, b, h, pix, c) of the rounded product"""
    from selfocc_amd.linear import linear_fwd_heads, linear_fwd_heads_supported
    T, N = B * nv, 96 * G
    assert linear_fwd_heads_supported(T, N, K, nv, bf16=True)
    hm = lambda t: t.view(B, nv, G, 6, 16).permute(2, 0, 3, 1, 4).contiguous()      # noqa: E731
    for fam in bc.FAMILIES:
        c = bc.fwd_case(fam, T, N, K)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want = hm(c['want'] + c['bias'].double())
        got = linear_fwd_heads(x, w, b, nv, bf16=True)
        assert got.shape == (G, B, 6, nv, 16) and same(got, want), fam
        assert torch.equal(linear_fwd_heads(x, w, b, nv, bf16=True), got)
        assert same(linear_fwd_heads(x, w, b, nv, relu=True, bf16=True), want.clamp_min(0))
        assert same(linear_fwd_heads(x, w, None, nv, bf16=True), hm(c['want']))
        got0 = linear_fwd_heads(x, w, b, nv)
        assert same(got0, hm(c['plain'] + c['bias'].double())) and (fam == 'E') == torch.equal(got0, got)


# ---- dgrad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,K", bc.DGRAD_CASES)
def test_dgrad_one_product_is_exact(hip, T, N, K):
    """linear_dgrad_b3_kernel<false, 1>: the in-kernel rounding of W (N <= 96) and the one pre-rounded plane, zero-padded last chunk"""
    from selfocc_amd.linear import linear_dgrad, dgrad_supported
    assert dgrad_supported(T, N, K, bf16=True)
    assert hip.selfocc_linear_dgrad_workspace_flags(N, K, 2) == bc.dgrad_plan(T, N, K)['workspace']
    for fam in bc.FAMILIES:
        c = bc.dgrad_case(fam, T, N, K)
        dy, w = c['dy'].cuda(), c['w'].cuda()
        dx = linear_dgrad(dy, w, bf16=True)
        assert same(dx, c['want']), fam
        assert torch.equal(linear_dgrad(dy, w, bf16=True), dx)
        dx0 = linear_dgrad(dy, w)
        assert same(dx0, c['plain']) and (fam == 'E') == torch.equal(dx0, dx)


# ---- wgrad ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,K", bc.WGRAD_CASES)
def test_wgrad_one_product_is_exact(hip, T, N, K):
    """linear_wgrad_b3_kernel<KT, NTW, false, 1>, K = 128 included (the default leaves it to the f32-MFMA kernel; a flagged launch
    has its own instances): dW = dy^^T x^, and db = the column sums of the ROUNDED dy"""
    from selfocc_amd.linear import linear_wgrad, wgrad_supported
    assert wgrad_supported(T, N, K, bf16=True)
    assert hip.selfocc_linear_wgrad_workspace_flags(T, N, K, 2) == bc.wgrad_plan(T, N, K)['workspace']      # the mirror has not drifted
    for fam in bc.FAMILIES:
        c = bc.wgrad_case(fam, T, N, K)
        dy, x = c['dy'].cuda(), c['x'].cuda()
        dw, db = linear_wgrad(dy, x, bf16=True)
        assert same(dw, c['want_w']), fam
        assert same(db, c['want_b']), fam
        dw2, db2 = linear_wgrad(dy, x, bf16=True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        dw3, none = linear_wgrad(dy, x, with_bias=False, bf16=True)
        assert none is None and torch.equal(dw, dw3)
        dw0, db0 = linear_wgrad(dy, x)
        assert same(dw0, c['plain_w']) and same(db0, c['plain_b'])
        assert (fam == 'E') == torch.equal(dw0, dw) and (fam == 'E') == torch.equal(db0, db)


# ---- grouped forms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,N,K", bc.GROUPED_CASES)
def test_grouped_one_product_passes_are_exact(hip, sizes, N, K):
    """selfocc_linear_fwd_grouped (per-group weights, shared weights, per-group LayerNorm where N <= 96), the grouped dgrad and wgrad
    with the flag, on every grouped instance family (bc.GROUPED_*_INSTANCES); empty groups and a group of one row.  Group g's
    result is the ungrouped product of its rows with W_g."""
    from selfocc_amd.linear import linear_fwd_grouped, linear_dgrad_grouped, linear_wgrad_grouped
    T, G = sum(sizes), len(sizes)
    rows = torch.split(torch.arange(T), list(sizes))
    run = bc.grouped_passes(N, K)
    for fam in bc.FAMILIES:
        c = bc.grouped_case(fam, sizes, N, K)
        x, res, ws, bs = c['x'], c['res'], c['ws'], c['bs']
        xg, wg, bg = x.cuda(), ws.cuda(), bs.cuda()
        if run['fwd']:
            want = torch.cat([bc.rne(x[r]) @ bc.rne(ws[g]).t() + bs[g].double() for g, r in enumerate(rows)])
            plain = torch.cat([x[r].double() @ ws[g].double().t() + bs[g].double() for g, r in enumerate(rows)])
            y = linear_fwd_grouped(xg, sizes, wg, bg, bf16=True)
            assert same(y, want), fam
            assert torch.equal(linear_fwd_grouped(xg, sizes, wg, bg, bf16=True), y)
            y0 = linear_fwd_grouped(xg, sizes, wg, bg)
            assert same(y0, plain) and (fam == 'E') == torch.equal(y0, y)
            assert same(linear_fwd_grouped(xg, sizes, wg, bg, relu=True, residual=res.cuda(), bf16=True), want.clamp_min(0) + res.double())
            assert same(linear_fwd_grouped(xg, sizes, wg[0], bg[0], shared_w=True, bf16=True), bc.rne(x) @ bc.rne(ws[0]).t() + bs[0].double())
        if run['dgrad']:
            dy = c['dy']
            dx = linear_dgrad_grouped(dy.cuda(), wg, sizes, bf16=True)
            assert same(dx, torch.cat([bc.rne(dy[r]) @ bc.rne(ws[g]) for g, r in enumerate(rows)])), fam
            assert torch.equal(linear_dgrad_grouped(dy.cuda(), wg, sizes, bf16=True), dx)
        if run['wgrad']:
            dyc = c['dy_w']
            dw, db = linear_wgrad_grouped(dyc.cuda(), xg, sizes, bf16=True)
            wdw = torch.stack([bc.rne(dyc[r]).t() @ bc.rne(x[r]) for r in rows])
            assert same(dw, wdw) and same(db, torch.stack([dyc[r].double().sum(0) for r in rows])), fam
            dw2, db2 = linear_wgrad_grouped(dyc.cuda(), xg, sizes, bf16=True)
            assert torch.equal(dw, dw2) and torch.equal(db, db2)
    if not (run['fwd'] and N <= 96):
        return
    # per-group LayerNorm on a shared projection and on per-group weights (inputs in the 2^-20 unit: y_pre exact and O(1))
    c = bc.grouped_case('R', sizes, N, K, ln=True)
    x, res, bias = c['x'], c['res'], c['bs'][0]
    gam = torch.stack([ln_params(N, ('g', g))[0] for g in range(G)])
    bet = torch.stack([ln_params(N, ('g', g))[1] for g in range(G)])
    for shared in (True, False):
        ws = c['ws'][:1].expand(G, -1, -1).contiguous() if shared else c['ws']
        pre = torch.cat([bc.rne(x[r]) @ bc.rne(ws[g]).t() for g, r in enumerate(rows)]) + bias.double() + res.double()
        w_arg = ws[0].cuda() if shared else ws.cuda()
        b_arg = bias.cuda() if shared else bias[None].expand(G, -1).contiguous().cuda()
        y, y_pre, mean, rstd = linear_fwd_grouped(x.cuda(), sizes, w_arg, b_arg, residual=res.cuda(), ln=(gam, bet, 1e-5),
                                                  want_stats=True, shared_w=shared, bf16=True)
        assert same(y_pre, pre), shared
        for g, r in enumerate(rows):
            if len(r):
                check_ln(y[r], mean[r], rstd[r], pre[r], gam[g], bet[g])


# ---- random data -----------------------------------------------------------------------------------------------------------------
def test_random_data_within_the_summation_bound(hip):
    """one case per pass, N(0, 1) operands with full significands, against the float64 product of the rounded operands:
    |err| <= (R + 2) 2^-24 sum_r |a^_r b^_r| per element (bc.sum_bound: any summation order of exact products)"""
    from selfocc_amd.linear import linear_fwd, linear_dgrad, linear_wgrad
    g = torch.Generator().manual_seed(5)
    T, N, K = 1003, 200, 96
    x, w, b, dy = torch.randn(T, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(T, N, generator=g)
    xr, wr, dyr = bc.rne(x), bc.rne(w), bc.rne(dy)
    y = linear_fwd(x.cuda(), w.cuda(), b.cuda(), bf16=True).double().cpu()
    # the bias is one more term of the sum: (R + 2) 2^-24 (sum_r |x^ w^| + |b|) — R roundings of the accumulation, one of the bias add
    assert bool(((y - (xr @ wr.t() + b.double())).abs() <= bc.sum_bound(x, w, K, b.abs())).all())
    assert not torch.equal(y.float(), linear_fwd(x.cuda(), w.cuda(), b.cuda()).cpu())
    dx = linear_dgrad(dy.cuda(), w.cuda(), bf16=True).double().cpu()
    assert bool(((dx - dyr @ wr).abs() <= bc.sum_bound(dy, w.t(), N)).all())
    dw, db = linear_wgrad(dy.cuda(), x.cuda(), bf16=True)
    assert bool(((dw.double().cpu() - dyr.t() @ xr).abs() <= bc.sum_bound(dy.t(), x.t(), T)).all())
    assert bool(((db.double().cpu() - dyr.sum(0)).abs() <= (T + 2) * 2.0 ** -24 * dyr.abs().sum(0)).all())
    # LayerNorm epilogue: the tolerances of tests/test_linear_gpu.py from the float64 y_pre of the rounded operands
    w2, b2, res = torch.randn(96, K, generator=g) / K ** 0.5, torch.randn(96, generator=g), torch.randn(T, 96, generator=g)
    gamma, beta = ln_params(96, ('rnd',))
    y, y_pre, mean, rstd = linear_fwd(x.cuda(), w2.cuda(), b2.cuda(), residual=res.cuda(), ln=(gamma, beta, 1e-5), want_stats=True, bf16=True)
    pre = xr @ bc.rne(w2).t() + b2.double() + res.double()
    # bias and residual are two more terms: R roundings of the accumulation, one each of the bias and the residual add
    assert bool(((y_pre.double().cpu() - pre).abs() <= bc.sum_bound(x, w2, K, b2.abs()[None, :] + res.abs())).all())
    check_ln(y, mean, rstd, pre, gamma, beta)


# ---- the autograd Functions and the switch -----------------------------------------------------------------------------------------
def _wrap(hip_names):
    """count the calls of the library's tall-Linear entry points by name (restored by the caller)"""
    from selfocc_amd._lib import lib
    l, counts, saved = lib(), {}, {}
    for n in hip_names:
        saved[n] = getattr(l, n)

        def f(*a, _n=n, _f=saved[n]):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a)
        setattr(l, n, f)
    return l, counts, saved


def test_functions_record_the_mode_at_forward_time(hip):
    """_TallLinear, _TallLinearHeads and _GroupedTallLinear with the switch on at forward and flipped OFF before backward still run
    the flagged backward entries; with the switch off nothing is counted and the outputs are torch.equal to a run made before the
    switch was ever touched."""
    from selfocc_amd.model import bricks
    assert bricks.LINEAR_BF16 is False and bricks.LINEAR_BF16_CALLS[0] == 0, "needs a process that has not touched the switch"
    g = torch.Generator().manual_seed(11)
    T, K, nv = 40000, 96, 20000
    sizes = [30000, 0, 10000]

    def params(n_out, G=1):
        return [t for _ in range(G) for t in ((torch.randn(n_out, K, generator=g) / K ** 0.5).cuda().requires_grad_(True),
                                              torch.randn(n_out, generator=g).cuda().requires_grad_(True))]

    x = torch.randn(T, K, generator=g).cuda().requires_grad_(True)
    wb_tall, wb_heads, wb_grp = params(104), params(96, 2), params(96, 3)

    def run(flip):
        outs = []
        for kind in ('tall', 'heads', 'grouped'):
            for p in [x] + wb_tall + wb_heads + wb_grp:
                p.grad = None
            if kind == 'tall':
                y = bricks._TallLinear.apply(x, True, *wb_tall)
            elif kind == 'heads':
                y = torch.cat([o.reshape(-1) for o in bricks._TallLinearHeads.apply(x, nv, None, *wb_heads)])
            else:
                y = bricks._GroupedTallLinear.apply(x, sizes, False, *wb_grp)
            if flip:
                bricks.LINEAR_BF16 = False
            y.square().sum().backward()
            if flip:
                bricks.LINEAR_BF16 = True
            ps = {'tall': wb_tall, 'heads': wb_heads, 'grouped': wb_grp}[kind]
            outs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in ps])
        return outs

    first = run(False)                                   # before the switch was ever touched
    assert bricks.LINEAR_BF16_CALLS[0] == 0
    names = ["selfocc_linear_dgrad", "selfocc_linear_wgrad", "selfocc_linear_dgrad_grouped", "selfocc_linear_wgrad_grouped",
             "selfocc_linear_dgrad_flags", "selfocc_linear_wgrad_flags", "selfocc_linear_dgrad_grouped_flags",
             "selfocc_linear_wgrad_grouped_flags"]
    l, counts, saved = _wrap(names)
    try:
        bricks.LINEAR_BF16 = True
        flagged = run(True)                              # on at forward, off at backward
        assert counts == {"selfocc_linear_dgrad_flags": 2, "selfocc_linear_wgrad_flags": 2, "selfocc_linear_dgrad_grouped_flags": 1,
                          "selfocc_linear_wgrad_grouped_flags": 1}, counts
        assert bricks.LINEAR_BF16_CALLS[0] == 9          # three forwards, three dgrads, three wgrads
        bricks.LINEAR_BF16 = False
        counts.clear()
        again = run(False)
        assert set(counts) == {"selfocc_linear_dgrad", "selfocc_linear_wgrad", "selfocc_linear_dgrad_grouped",
                               "selfocc_linear_wgrad_grouped"}, counts
        assert bricks.LINEAR_BF16_CALLS[0] == 9
    finally:
        bricks.LINEAR_BF16 = False
        bricks.LINEAR_BF16_CALLS[0] = 0
        for n, f in saved.items():
            setattr(l, n, f)
    for a, b, c in zip(first, again, flagged):
        for ta, tb, tc in zip(a, b, c):
            assert torch.equal(ta, tb)                   # the default mode is untouched by the switch's history
            assert torch.equal(ta, tc) == (not bool(ta.any()))      # ... and the flagged run is another computation (but for the
            #                                                         zero gradients of the empty group)
