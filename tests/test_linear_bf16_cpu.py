"""CPU: the one-product bfloat16 mode of the tall-Linear kernels (SO_LINEAR_BF16X1 / bricks.LINEAR_BF16) as far as it goes without a
GPU — the new C entry points and their host-side argument checks, the flag constant, the Python keywords and the switch, the
contract of the exact inputs of tests/test_linear_bf16_gpu.py (tests/linear_bf16_cases.py) on every case it runs, the set of P = 1
kernel instantiations those cases reach, and the sharpness of the comparison: rounding by truncation or half-away breaks it."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "selfocc_hip.h")).read()
NEW_SYMBOLS = ["selfocc_linear_dgrad_flags", "selfocc_linear_dgrad_grouped_flags", "selfocc_linear_wgrad_flags",
               "selfocc_linear_wgrad_grouped_flags", "selfocc_linear_dgrad_workspace_flags",
               "selfocc_linear_dgrad_grouped_workspace_flags", "selfocc_linear_wgrad_workspace_flags",
               "selfocc_linear_wgrad_grouped_workspace_flags"]


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_the_flag_constant():
    from selfocc_amd import abi
    from selfocc_amd._lib import lib
    l = lib()
    for name in NEW_SYMBOLS:
        assert name in abi.SYMBOLS and re.search(r"\b%s\s*\(" % name, HEADER), name
        assert getattr(l, name) is not None
    assert abi.LINEAR_BF16X1 == 2 and abi.LINEAR_RELU == 1
    assert re.search(r"SO_LINEAR_BF16X1\s*=\s*2\b", HEADER)
    assert int(re.search(r"#define SELFOCC_ABI_VERSION (\d+)", HEADER).group(1)) == abi.ABI_VERSION == l.selfocc_abi_version()


def test_python_passes_take_the_bf16_keyword():
    from selfocc_amd import linear
    for name in ("linear_fwd", "linear_fwd_grouped", "linear_fwd_heads", "linear_dgrad", "linear_dgrad_grouped", "linear_wgrad",
                 "linear_wgrad_grouped", "linear_fwd_supported", "linear_fwd_grouped_supported", "linear_fwd_heads_supported",
                 "dgrad_supported", "linear_dgrad_grouped_supported", "wgrad_supported", "linear_wgrad_grouped_supported"):
        p = inspect.signature(getattr(linear, name)).parameters
        assert 'bf16' in p and p['bf16'].default is False, name


def _groups(sizes):
    from selfocc_amd.abi import SoRowGroups
    return SoRowGroups.from_sizes(sizes)


def test_argument_checks_of_the_flagged_entries_are_pure_host_logic():
    """an unknown flag bit, a NULL pointer and a short workspace are refused with a named error before any HIP call (no GPU here)"""
    from selfocc_amd._lib import lib
    l = lib()
    fake = C.create_string_buffer(64)      # never dereferenced: every call below fails its checks first
    f = C.addressof(fake)
    T, N, K, X1 = 70, 96, 96, 2
    g = _groups((30, 40))

    def dgrad(flags=X1, dy=f, ws=f, nbytes=None, grouped=False):
        need = l.selfocc_linear_dgrad_grouped_workspace_flags(200, K, g, X1) if grouped else l.selfocc_linear_dgrad_workspace_flags(200, K, X1)
        nbytes = need if nbytes is None else nbytes
        if grouped:
            return l.selfocc_linear_dgrad_grouped_flags(dy, f, f, T, 200, K, g, ws, nbytes, flags, None)
        return l.selfocc_linear_dgrad_flags(dy, f, f, T, 200, K, ws, nbytes, flags, None)

    def wgrad(flags=X1, dy=f, ws=f, nbytes=None, grouped=False):
        need = l.selfocc_linear_wgrad_grouped_workspace_flags(T, N, K, g, X1) if grouped else l.selfocc_linear_wgrad_workspace_flags(T, N, K, X1)
        nbytes = need if nbytes is None else nbytes
        if grouped:
            return l.selfocc_linear_wgrad_grouped_flags(dy, f, f, f, T, N, K, g, ws, nbytes, flags, None)
        return l.selfocc_linear_wgrad_flags(dy, f, f, f, T, N, K, ws, nbytes, flags, None)

    for call in (dgrad, wgrad):
        for grouped in (False, True):
            for kw, word in ((dict(flags=4), b"unknown flags"), (dict(flags=X1 | 1), b"unknown flags"), (dict(flags=0x80000002), b"unknown flags"),
                             (dict(dy=None), b"NULL"), (dict(ws=None), b"workspace" if call is wgrad else b"NULL"),
                             (dict(nbytes=16), b"workspace")):
                rc = call(grouped=grouped, **kw)
                assert rc < 0 and word in l.selfocc_last_error(), (call.__name__, grouped, kw, rc, l.selfocc_last_error())
    # shapes no kernel serves are named too
    assert l.selfocc_linear_dgrad_flags(f, f, f, T, 12, K, f, 1 << 20, X1, None) < 0 and b"unsupported shape" in l.selfocc_last_error()
    assert l.selfocc_linear_wgrad_flags(f, f, f, f, T, N, 80, f, 1 << 20, X1, None) < 0 and b"unsupported shape" in l.selfocc_last_error()
    assert l.selfocc_linear_wgrad_grouped_flags(f, f, f, f, T + 1, N, K, g, f, 1 << 20, X1, None) < 0 and b"row_start" in l.selfocc_last_error()


def test_flagged_workspace_and_support_queries_are_pure_host_logic():
    """one plane of W^T for the dgrad; the wgrad's plan with the flag (K = 128 on the bf16 kernel) never needs more than the default's;
    the support queries answer the same for both modes — a flagged launch always has a one-product kernel"""
    from selfocc_amd._lib import lib
    from selfocc_amd import linear
    l = lib()
    for (T, N, K) in bc.DGRAD_CASES:
        d = l.selfocc_linear_dgrad_workspace(N, K)
        assert l.selfocc_linear_dgrad_workspace_flags(N, K, 0) == d and d % 3 == 0
        assert l.selfocc_linear_dgrad_workspace_flags(N, K, 2) == d // 3 == bc.dgrad_plan(T, N, K)['workspace']
        assert l.selfocc_linear_dgrad_workspace_flags(N, K, 4) == 0
        assert l.selfocc_linear_dgrad_grouped_workspace_flags(N, K, _groups((T, 0, 5)), 2) == 3 * (d // 3)
        assert linear.dgrad_supported(T, N, K, bf16=True) and linear.dgrad_supported(T, N, K)
    # the default query is a valid upper bound for a flagged launch: the flagged plan never has more tile rows per wave than the
    # default's, hence never more chunks — swept over every K, both sides of the T = 16 384 and N = 96 thresholds, and the shapes
    # where a two-tile-row K = 192 plan would have needed up to twice the default's bytes
    sweep = [(T, N, K) for K in bc.KS5 for T in (1, 70, 1003, 16383, 16384, 81983, 178500) for N in (1, 33, 96, 97, 128, 160, 192, 384, 2304)]
    for (T, N, K) in bc.WGRAD_CASES + [(66049, 384, 128), (66049, 2304, 96), (81983, 192, 192), (81983, 384, 192), (81983, 160, 192)] + sweep:
        d = l.selfocc_linear_wgrad_workspace(T, N, K)
        assert l.selfocc_linear_wgrad_workspace_flags(T, N, K, 0) == d
        x1 = l.selfocc_linear_wgrad_workspace_flags(T, N, K, 2)
        assert x1 == bc.wgrad_plan(T, N, K)['workspace'] and 0 < x1 <= d, (T, N, K, x1, d)
        assert l.selfocc_linear_wgrad_workspace_flags(T, N, K, 6) == 0
        for sizes in ((T, 0, 5), (T // 3, T - T // 3), (1,) * 7 + (T,)):
            gx1 = l.selfocc_linear_wgrad_grouped_workspace_flags(sum(sizes), N, K, _groups(sizes), 2)
            assert 0 < gx1 <= l.selfocc_linear_wgrad_grouped_workspace(sum(sizes), N, K, _groups(sizes)), (sizes, N, K)
        assert linear.wgrad_supported(T, N, K, bf16=True) and linear.wgrad_supported(T, N, K)
    assert l.selfocc_linear_wgrad_workspace_flags(70, 96, 80, 2) == 0
    for K in bc.KS5:
        assert linear.linear_fwd_supported(1, 20, K, bf16=True)
        assert linear.linear_fwd_grouped_supported((0, 70, 1, 33), 96, K, bf16=True)


# ---- the switch ----------------------------------------------------------------------------------------------------------------
def test_env_switch_parses():
    """SELFOCC_LINEAR_BF16=1 sets bricks.LINEAR_BF16 (a fresh interpreter: the variable is read at import); anything else leaves it off"""
    from selfocc_amd.model import bricks
    assert bricks.LINEAR_BF16 == (os.environ.get('SELFOCC_LINEAR_BF16', '0') == '1')
    assert bricks.LINEAR_BF16_CALLS == [0] or isinstance(bricks.LINEAR_BF16_CALLS[0], int)
    code = "from selfocc_amd.model import bricks; print('SWITCH', bricks.LINEAR_BF16, bricks.LINEAR_BF16_CALLS)"
    for val, want in (("1", "SWITCH True [0]"), ("0", "SWITCH False [0]"), ("true", "SWITCH False [0]")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SELFOCC_LINEAR_BF16=val),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and want in r.stdout, (val, r.stdout[-500:], r.stderr[-2000:])


def test_switch_changes_hip_launches_only():
    """a projection that stays on torch (CPU tensors here) stays what it is with the switch on, and counts nothing"""
    from selfocc_amd.model import bricks
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2000, 96, generator=g), torch.randn(40, 96, generator=g), torch.randn(40, generator=g)
    before, calls = bricks.LINEAR_BF16, bricks.LINEAR_BF16_CALLS[0]
    try:
        bricks.LINEAR_BF16 = False
        y0 = bricks._tall_fwd(x, w, b, relu=True)
        lin = bricks.TallLinear(96, 40)
        with torch.no_grad():
            z0 = lin(x)
        bricks.LINEAR_BF16 = True
        assert torch.equal(bricks._tall_fwd(x, w, b, relu=True), y0)
        with torch.no_grad():
            assert torch.equal(lin(x), z0) and torch.equal(bricks.fused_linear(lin, x), z0)
        assert bricks.LINEAR_BF16_CALLS[0] == calls
        # the counter counts launches in the mode: the switch, or the mode a Function recorded
        assert bricks._bf16() == {'bf16': True} and bricks._bf16(False) == {} and bricks._bf16(True) == {'bf16': True}
        assert bricks.LINEAR_BF16_CALLS[0] == calls + 2
    finally:
        bricks.LINEAR_BF16 = before
        bricks.LINEAR_BF16_CALLS[0] = calls


# ---- the case lists reach every P = 1 instantiation --------------------------------------------------------------------------------
def test_case_lists_reach_every_one_product_instantiation():
    fwd = {p['inst'] for (T, N, K, ln) in bc.FWD_CASES for p in bc.fwd_plan(T, N, K, ln)}
    assert fwd == bc.FWD_INSTANCES, fwd ^ bc.FWD_INSTANCES
    # a second tile with the prefetch live on each tile variant (4 waves x 32 rows, 4 x 16, 8 x 16), with and without LayerNorm
    walked = {p['inst'][3:6] + (p['inst'][2],) for (T, N, K, ln) in bc.FWD_LONG for p in bc.fwd_plan(T, N, K, ln) if p['second_tile']}
    assert {(3, 4, 2, False), (3, 4, 1, False), (3, 8, 1, False), (3, 4, 1, True)} <= walked, walked
    for (T, N, K) in bc.FWD_VARIANTS.values():
        assert (T, N, K, False) in bc.FWD_CASES and N % 4 == 0
    heads = {p['inst'] for (B, nv, G, K) in bc.HEADS_CASES for p in bc.fwd_plan(B * nv, 96 * G, K)}
    assert heads == {('x1', 3, False, 3, 4, 1, False), ('x1', 3, False, 3, 4, 2, False), ('x1', 6, False, 3, 8, 1, False)}, heads
    assert {bc.wgrad_plan(*c)['inst'] for c in bc.WGRAD_CASES} == bc.WGRAD_INSTANCES
    assert {bc.dgrad_plan(*c)['inst'] for c in bc.DGRAD_CASES} == bc.DGRAD_INSTANCES
    assert any(bc.dgrad_plan(*c)['second_tile'] for c in bc.DGRAD_CASES)
    # the grouped (GRP = true) instantiations: every family named in bc.GROUPED_*_INSTANCES is reached by bc.GROUPED_CASES
    gf, gw, gd = set(), set(), set()
    for sizes, N, K in bc.GROUPED_CASES:
        T, run = sum(sizes), bc.grouped_passes(N, K)
        if run['fwd']:
            gf |= {p['inst'] for ln in ((False, True) if N <= 96 else (False,)) for p in bc.fwd_plan(T, N, K, ln, True)}
        if run['wgrad']:
            gw.add(bc.wgrad_plan(T, N, K, True)['inst'])
        if run['dgrad']:
            gd.add(bc.dgrad_plan(T, N, K, True)['inst'])
    assert gf == bc.GROUPED_FWD_INSTANCES and gw == bc.GROUPED_WGRAD_INSTANCES and gd == bc.GROUPED_DGRAD_INSTANCES, (gf, gw, gd)
    assert {i[4:6] for i in gf} == {(4, 1), (4, 2), (8, 1)} and {i[1] for i in gw} >= {1, 2, 3, 4} and ('x1', 3, 1, 2, True) in gw
    # the flagged dispatch does not look at what the default would run: the same instance family on both sides of the default's
    # T = 16 384 / N = 384 thresholds
    for K in bc.KS5:
        assert [p['inst'] for p in bc.fwd_plan(70, 116, K)] == [p['inst'] for p in bc.fwd_plan(16401, 116, K)]


# ---- the contract of the data, for every case the GPU tests run -----------------------------------------------------------------------
def check(family, dense, sparse, want, plain, extra=None, log2_unit=0):
    c = bc.contract(family, dense, sparse, extra=extra, log2_unit=log2_unit)
    assert c['ints'] and c['mass'] < bc.LIMIT, c
    if family == 'R':
        # never vacuous: the rounding changes both operands and the result — the default mode's product is another integer matrix
        assert c['rounds_dense'] and c['rounds_sparse'], c
        assert not torch.equal(want, plain)
    else:
        assert not c['rounds_dense'] and not c['rounds_sparse'] and torch.equal(want, plain)
        assert bool((dense != 0).all()) and bool((sparse != 0).all())      # every reduction index decides every output
    assert torch.equal((want * 2.0 ** -log2_unit).round(), want * 2.0 ** -log2_unit)


@pytest.mark.parametrize("T,N,K,ln", bc.FWD_CASES)
def test_forward_cases_keep_the_contract(T, N, K, ln):
    for fam in bc.FAMILIES:
        c = bc.fwd_case(fam, T, N, K, ln)
        scale = 2.0 ** -c['log2_unit']
        for t in (c['bias'], c['res']):
            assert torch.equal((t.double() * scale).round(), t.double() * scale) and float(t.abs().max()) * scale < 1000
        check(fam, c['x'], c['w'], c['want'], c['plain'], extra=c['bias'].abs()[None, :] + c['res'].abs(), log2_unit=c['log2_unit'])


@pytest.mark.parametrize("B,nv,G,K", bc.HEADS_CASES)
def test_heads_cases_keep_the_contract(B, nv, G, K):
    for fam in bc.FAMILIES:
        c = bc.fwd_case(fam, B * nv, 96 * G, K)
        check(fam, c['x'], c['w'], c['want'], c['plain'], extra=c['bias'].abs()[None, :].expand(B * nv, -1))


@pytest.mark.parametrize("T,N,K", bc.DGRAD_CASES)
def test_dgrad_cases_keep_the_contract(T, N, K):
    for fam in bc.FAMILIES:
        c = bc.dgrad_case(fam, T, N, K)
        assert torch.equal(c['w'], c['sparse'].t())
        check(fam, c['dense'], c['sparse'], c['want'], c['plain'])


@pytest.mark.parametrize("T,N,K", bc.WGRAD_CASES)
def test_wgrad_cases_keep_the_contract(T, N, K):
    for fam in bc.FAMILIES:
        c = bc.wgrad_case(fam, T, N, K)
        check(fam, c['dense'], c['sparse'], c['want_w'].t(), c['plain_w'].t())
        assert float(bc.rne(c['dy']).abs().sum(0).max()) < bc.LIMIT
        if fam == 'R':
            assert not torch.equal(c['want_b'], c['plain_b'])          # db sums the ROUNDED dy
            hit = (c['dy'] != 0).any(1)
            assert all(bool(hit[r]) for r in bc.wgrad_forced_rows(T, N, K))
        else:
            assert T <= 16401 and bool((c['dy'].abs() == 1).all())


@pytest.mark.parametrize("sizes,N,K", bc.GROUPED_CASES)
def test_grouped_cases_keep_the_contract(sizes, N, K):
    """every product a grouped case takes — each group's weights with all rows (the per-group rows are a subset), the dgrad's dense dy
    over W's rows, the wgrad's +-1 dy over a group's rows — keeps the mass below 2^24, in both units"""
    run = bc.grouped_passes(N, K)
    for fam in bc.FAMILIES:
        for ln in ((False, True) if (fam == 'R' and run['fwd'] and N <= 96) else (False,)):
            c = bc.grouped_case(fam, sizes, N, K, ln)
            u = bc.LN_LOG2_UNIT if ln else 0
            for g in range(len(sizes)):
                extra = c['bs'][g].abs()[None, :] + c['res'].abs()
                k = bc.contract(fam, c['x'], c['ws'][g], extra=extra, log2_unit=u)
                assert k['ints'] and k['mass'] < bc.LIMIT, (fam, g, k)
                assert (fam == 'R') == (k['rounds_dense'] and k['rounds_sparse'])
                if run['dgrad'] and not ln:
                    kd = bc.contract(fam, c['dy'], c['ws'][g].t().contiguous())
                    assert kd['ints'] and kd['mass'] < bc.LIMIT, (fam, g, kd)
            dyw = c['dy_w']
            assert bool((dyw.abs() <= 1).all()) and bool((dyw != 0).any())
            assert float((dyw.abs().t().double() @ bc.rne(c['x']).abs()).max()) * 2.0 ** -u < bc.LIMIT


# ---- sharpness: the two wrong rounding rules break the comparison -----------------------------------------------------------------------
def test_ties_decide_the_rounding_rule():
    t = torch.tensor(bc.TIES, dtype=torch.float32)
    assert bc.rne(t).tolist() == [256, 260, 512, 520, 512, 772]
    assert bc.trunc_bf16(t).tolist() == [256, 258, 512, 516, 512, 768]
    assert bc.half_away_bf16(t).tolist() == [258, 260, 516, 520, 512, 772]
    assert torch.equal(bc.rne(-t), -bc.rne(t))
    for (T, N, K) in ((1, 20, 32), (70, 116, 96)):
        c = bc.fwd_case('R', T, N, K)
        for wrong in (bc.trunc_bf16, bc.half_away_bf16):
            for which in ('x', 'w'):
                a = wrong(c['x']) if which == 'x' else bc.rne(c['x'])
                b = wrong(c['w']) if which == 'w' else bc.rne(c['w'])
                got = a @ b.t()
                assert not torch.equal(got, c['want']), (wrong.__name__, which)
                # ... in EVERY output row when it is the dense operand that is rounded wrongly
                if which == 'x' and wrong is bc.half_away_bf16:
                    assert bool((got != c['want']).any(1).float().mean() > 0.5)
