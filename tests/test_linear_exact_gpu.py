"""The tall-Linear kernels (selfocc_linear_fwd / _fwd_heads / _dgrad in csrc/linear_fwd.hip, selfocc_linear_wgrad in csrc/linear.hip)
on every route of their launchers, BIT-EXACT against float64.

The inputs (tests/linear_cases.py) are integers on which every product and every partial sum, in any order, is an integer below
2^24: float32 accumulation is exact whatever the summation order, the three-way bfloat16 split loses nothing, and the result must
EQUAL the float64 product.  No tolerance: a low plane read from the wrong offset, a dropped term, a row or a reduction index
skipped or taken twice are integer differences at a known (row, column).  tests/test_linear_cases_cpu.py holds the contract of
these inputs, the set of kernel instantiations the case lists reach, and shows on a CPU emulation that such faults break the
comparison.  Only the LayerNorm epilogue's own outputs (y, mean, rstd) carry the float64 tolerances of tests/test_linear_gpu.py,
computed from the exact y_pre."""
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want):
    """bit-exact against the float64 result; on a mismatch the message names the first element and the integer difference"""
    g = got.double().cpu()
    if torch.equal(g, want):
        return True
    bad = (g != want).nonzero()
    i = tuple(bad[0].tolist())
    print(f"{len(bad)} of {want.numel()} elements differ; first at {i}: got {g[i].item()!r}, want {want[i].item()!r}, "
          f"largest difference {(g - want).abs().max().item()!r}")
    return False


# ---- forward ----------------------------------------------------------------------------------------------------------------
def run_fwd(T, N, K, ln):
    from selfocc_amd.linear import linear_fwd, linear_fwd_supported
    assert linear_fwd_supported(T, N, K)
    for fam in lc.FAMILIES:
        c = lc.fwd_case(fam, T, N, K, ln)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want = c['want'] + c['bias'].double()
        if not ln:
            y = linear_fwd(x, w, b)
            assert same(y, want), (fam, T, N, K)
            assert torch.equal(linear_fwd(x, w, b), y)
            continue
        g = torch.Generator().manual_seed(lc.hash_key((T, N, K, fam)))
        gamma = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
        beta = (0.1 * torch.randn(N, generator=g)).cuda()
        res = c['res'].cuda()
        pre = want + c['res'].double()
        y, y_pre, mean, rstd = linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True)
        assert same(y_pre, pre), (fam, T, N, K)
        ref = torch.nn.functional.layer_norm(pre, (N,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
        assert (y.double().cpu() - ref).abs().max().item() < 2e-5
        assert (mean.double().cpu() - pre.mean(1)).abs().max().item() < 1e-5
        assert (rstd.double().cpu() - 1 / (pre.var(1, unbiased=False) + 1e-5).sqrt()).abs().max().item() < 1e-4
        y2, p2, m2, r2 = linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5), want_stats=True)
        assert torch.equal(y, y2) and torch.equal(y_pre, p2) and torch.equal(mean, m2) and torch.equal(rstd, r2)
        assert torch.equal(linear_fwd(x, w, b, residual=res, ln=(gamma, beta, 1e-5)), y)


@pytest.mark.parametrize("T,N,K,ln", lc.FWD_B3_H2)
def test_fwd_b3_32_row_tiles_is_exact(hip, T, N, K, ln):
    """linear_fwd_b3_kernel<K / 32, false, NT, 4, 2>: N >= 384, full blocks plus a tail of 20 / 40 / 70 columns"""
    run_fwd(T, N, K, ln)


@pytest.mark.parametrize("T,N,K,ln", lc.FWD_B3_H1)
def test_fwd_b3_16_row_tiles_is_exact(hip, T, N, K, ln):
    """linear_fwd_b3_kernel<K / 32, LN, NT, 4, 1>: N <= 192 and T >= 16384, with and without the LayerNorm epilogue"""
    run_fwd(T, N, K, ln)


@pytest.mark.parametrize("T,N,K,ln", lc.FWD_B3_K192)
def test_fwd_b3_k192_is_exact(hip, T, N, K, ln):
    """linear_fwd_b3_kernel<6, LN, NT, 8, 1>"""
    run_fwd(T, N, K, ln)


@pytest.mark.parametrize("T,N,K,ln", lc.FWD_F32)
def test_fwd_f32_mfma_is_exact(hip, T, N, K, ln):
    """linear_fwd16_kernel<K / 4, LN, NT, 4>"""
    run_fwd(T, N, K, ln)


@pytest.mark.parametrize("route", sorted(lc.FWD_VARIANTS))
def test_fwd_epilogue_variants_are_exact(hip, route):
    """ReLU, no bias, and relu(.) + residual into a column block of a wider buffer from a strided residual: with 16-byte aligned
    row starts (the float4 epilogue of the b3 kernels) and offset by 7 floats (the scalar one).  Nothing outside the block moves."""
    from selfocc_amd.linear import linear_fwd
    T, N, K = lc.FWD_VARIANTS[route]
    for fam in lc.FAMILIES:
        c = lc.fwd_case(fam, T, N, K)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want = c['want'] + c['bias'].double()
        assert same(linear_fwd(x, w, None), c['want'])
        y = linear_fwd(x, w, b, relu=True)
        assert same(y, want.clamp_min(0)) and torch.equal(linear_fwd(x, w, b, relu=True), y)
        for off, pad in ((8, 8), (7, 3)):
            wide = torch.zeros(T, N + 40)
            wide[:, off:off + N] = c['res']
            res = wide.cuda()[:, off:off + N]                    # row stride N + 40
            buf = torch.full((T, 2 * N + pad), 7.0).cuda()
            out = buf[:, N:2 * N]
            assert (out.data_ptr() % 16 == 0 and res.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0) == (off == 8)
            r = linear_fwd(x, w, b, relu=True, residual=res, out=out)
            assert r.data_ptr() == out.data_ptr()
            assert same(out, want.clamp_min(0) + c['res'].double()), (fam, off)
            assert torch.all(buf[:, :N] == 7.0) and torch.all(buf[:, 2 * N:] == 7.0)
            first = out.clone()
            linear_fwd(x, w, b, relu=True, residual=res, out=out)
            assert torch.equal(out, first)


@pytest.mark.parametrize("B,nv,G,K", lc.HEADS_CASES)
def test_fwd_heads_is_exact(hip, B, nv, G, K):
    """selfocc_linear_fwd_heads against the float64 product transposed on the CPU: (b, pix, g, h, c) -> (g, b, h, pix, c)"""
    from selfocc_amd.linear import linear_fwd_heads, linear_fwd_heads_supported
    T, N = B * nv, 96 * G
    assert linear_fwd_heads_supported(T, N, K, nv)
    for fam in lc.FAMILIES:
        c = lc.fwd_case(fam, T, N, K)
        x, w, b = c['x'].cuda(), c['w'].cuda(), c['bias'].cuda()
        want = (c['want'] + c['bias'].double()).view(B, nv, G, 6, 16).permute(2, 0, 3, 1, 4).contiguous()
        got = linear_fwd_heads(x, w, b, nv)
        assert got.shape == (G, B, 6, nv, 16) and same(got, want), fam
        assert torch.equal(linear_fwd_heads(x, w, b, nv), got)
        assert same(linear_fwd_heads(x, w, b, nv, relu=True), want.clamp_min(0))
        assert same(linear_fwd_heads(x, w, None, nv), want - c['bias'].double().view(G, 1, 6, 1, 16))


# ---- wgrad ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,K", lc.WGRAD_CASES)
def test_wgrad_is_exact(hip, T, N, K):
    """dW and db from sparse dy (families A and C; the rows at the edges of the plan's blocks forced in) and from dense +-1 dy
    against non-zero x (family D: a skipped or doubled row changes every output)."""
    from selfocc_amd.linear import linear_wgrad, wgrad_supported
    assert wgrad_supported(T, N, K)
    plan = lc.wgrad_plan(T, N, K)
    assert hip.selfocc_linear_wgrad_workspace(T, N, K) == plan['workspace']          # the mirror has not drifted
    for fam in ('A', 'C', 'D'):
        c = lc.wgrad_case(fam, T, N, K)
        dy, x = c['dy'].cuda(), c['x'].cuda()
        dw, db = linear_wgrad(dy, x)
        assert same(dw, c['want_w']), (fam, plan)
        assert same(db, c['want_b']), (fam, plan)
        dw2, db2 = linear_wgrad(dy, x)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        dw3, none = linear_wgrad(dy, x, with_bias=False)
        assert none is None and torch.equal(dw, dw3)


# ---- dgrad ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,K", lc.DGRAD_CASES)
def test_dgrad_is_exact(hip, T, N, K):
    """dx = dy W with dy dense and W sparse per output column: the in-kernel split (N <= 96) and the pre-split planes with a
    zero-padded last 96-wide chunk."""
    from selfocc_amd.linear import linear_dgrad, dgrad_supported
    assert dgrad_supported(T, N, K)
    plan = lc.dgrad_plan(T, N, K)
    assert hip.selfocc_linear_dgrad_workspace(N, K) == plan['workspace']
    for fam in lc.FAMILIES:
        c = lc.dgrad_case(fam, T, N, K)
        dy, w = c['dy'].cuda(), c['w'].cuda()
        dx = linear_dgrad(dy, w)
        assert same(dx, c['want']), (fam, plan)
        assert torch.equal(linear_dgrad(dy, w), dx)


# ---- random data on the newly reached routes: the assertion of test_linear_gpu.test_linear_fwd_matches_f64 -------------------------
@pytest.mark.parametrize("T,N,K", [(16401, 116, 32), (70, 454, 64), (16401, 70, 128), (16401, 116, 192), (16401, 136, 192), (16401, 40, 192),
                                   (70, 116, 192), (1, 20, 192)])
def test_fwd_random_data_matches_f64(hip, T, N, K):
    """values with full 24-bit significands: b3 at K = 32, 64, 128, the tails of the K = 192 b3 kernel, f32 MFMA at K = 192"""
    from selfocc_amd.linear import linear_fwd
    g = torch.Generator().manual_seed(T + N + K)
    x = torch.randn(T, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    b = torch.randn(N, generator=g).cuda()
    want = x.double() @ w.double().t() + b.double()
    y = linear_fwd(x, w, b)
    tol = 2e-6 * max(1.0, want.abs().max().item())
    assert (y.double() - want).abs().max().item() < tol
    assert torch.equal(linear_fwd(x, w, b), y)
    assert (linear_fwd(x, w, b, relu=True).double() - want.clamp_min(0)).abs().max().item() < tol


# ---- SELFOCC_LINEAR_B3=0: the f32-MFMA kernels at the shapes the default sends to the bf16 ones -------------------------------------
def test_the_f32_fallback_kernels_are_exact_in_a_child_process(hip):
    """The switch is read once per process, so a fresh child runs the reduced list (tests/linear_exact_child.py) and prints one JSON
    line per case; started once, never retried."""
    env = dict(os.environ, SELFOCC_LINEAR_B3="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "linear_exact_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    want = ({("fwd", fam, *s) for s in lc.CHILD_FWD for fam in lc.FAMILIES}
            | {("wgrad", fam, *s) for s in lc.CHILD_WGRAD for fam in ('A', 'C', 'D')})
    assert {(d["op"], d["family"], *d["shape"]) for d in lines} == want
    for d in lines:
        assert d["b3_env"] == "0" and d["exact"] and d["repeat_identical"], d
