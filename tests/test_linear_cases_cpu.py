"""CPU: the contract of the exact inputs of tests/test_linear_exact_gpu.py (tests/linear_cases.py), for every case the GPU tests
run; the set of kernel instantiations those cases reach, by the Python mirror of the launch plans; and the sharpness of the exact
comparison — three faults put into the CPU emulation of the six-term bfloat16 scheme must each break it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_cases as lc  # noqa: E402


def check_pair(family, dense, sparse, want, pos, R, extra=None, log2_unit=0, forced=()):
    c = lc.contract(dense, sparse, extra=extra, log2_unit=log2_unit)
    assert c['ints'] and c['exact'] and c['dropped_zero'], c
    assert c['mass'] < lc.LIMIT, c['mass']
    # the planes the family promises are populated — unless the case is too small to hold a value of that many bits
    if dense.numel() >= 64 and sparse.numel() >= 64:
        assert c['live'] == lc.FAMILY_TERMS[family], (family, c['live'])
    else:
        assert c['live'] <= lc.FAMILY_TERMS[family]
    assert torch.equal(lc.emulate_b3(dense, sparse, seed=R).double(), want)
    if pos is not None:
        nz = sparse != 0
        assert int(nz.sum(1).max()) <= pos.shape[1]
        hit = nz.any(0)
        budget = sparse.shape[0] * pos.shape[1]
        if not forced:      # no reduction index is used twice before all are used: every one decides some output where the rows allow
            assert int(hit.sum()) == min(R, budget)
        else:               # a forced row takes the place of one entry per sparse row
            assert int(hit.sum()) >= min(R, budget) - sparse.shape[0]
            assert all(bool(hit[r]) for r in forced)


@pytest.mark.parametrize("T,N,K,ln", lc.FWD_CASES + [(T, N, K, False) for (T, N, K) in lc.FWD_VARIANTS.values()])
def test_forward_cases_keep_the_contract(T, N, K, ln):
    for fam in lc.FAMILIES:
        c = lc.fwd_case(fam, T, N, K, ln)
        scale = 2.0 ** -c['log2_unit']
        extra = (c['bias'].abs()[None, :] + c['res'].abs())
        for t in (c['bias'], c['res']):
            assert torch.equal((t.double() * scale).round(), t.double() * scale)
        check_pair(fam, c['x'], c['w'], c['want'], c['pos'], K, extra=extra, log2_unit=c['log2_unit'])


@pytest.mark.parametrize("B,nv,G,K", lc.HEADS_CASES)
def test_heads_cases_keep_the_contract(B, nv, G, K):
    for fam in lc.FAMILIES:
        c = lc.fwd_case(fam, B * nv, 96 * G, K)
        check_pair(fam, c['x'], c['w'], c['want'], c['pos'], K, extra=c['bias'].abs()[None, :].expand(B * nv, -1))


@pytest.mark.parametrize("T,N,K", lc.DGRAD_CASES)
def test_dgrad_cases_keep_the_contract(T, N, K):
    for fam in lc.FAMILIES:
        c = lc.dgrad_case(fam, T, N, K)
        assert torch.equal(c['w'], c['sparse'].t())
        check_pair(fam, c['dense'], c['sparse'], c['want'], c['pos'], N)


@pytest.mark.parametrize("b3_env,T,N,K", [(True, *s) for s in lc.WGRAD_CASES] + [(False, *s) for s in lc.CHILD_WGRAD])
def test_wgrad_cases_keep_the_contract(b3_env, T, N, K):
    for fam in ('A', 'C'):
        c = lc.wgrad_case(fam, T, N, K, b3_env)
        p = lc.wgrad_plan(T, N, K, b3_env)
        assert set(c['forced']) >= {0, T - 1}
        if p['chunks'] >= 3:      # both edges of a block that is neither the first nor the last
            lo = [r for r in c['forced'] if 0 < r < T - 1]
            assert len(lo) == 2 and lo[0] % p['rows_per_block'] == 0 and lo[1] == lo[0] + p['rows_per_block'] - 1
        check_pair(fam, c['dense'], c['sparse'], c['want_w'].t(), c['pos'], T, forced=c['forced'])
        assert torch.equal(c['want_b'], c['dy'].double().sum(0)) and torch.equal(c['want_b'], c['want_b'].round())
        assert float(c['dy'].abs().sum(0).max()) < lc.LIMIT
    c = lc.wgrad_case('D', T, N, K, b3_env)
    assert bool((c['x'] != 0).all()) and bool((c['dy'].abs() == 1).all())
    assert float(c['x'].abs().max()) <= min(1022, (2 ** 24 - 1) // T)
    check_pair('D', c['dense'], c['sparse'], c['want_w'].t(), None, T)


# ---- which kernels the case lists reach -------------------------------------------------------------------------------------
def test_the_forward_cases_reach_every_instantiation():
    got = {p['inst'] for (T, N, K, ln) in lc.FWD_CASES for p in lc.fwd_plan(T, N, K, ln)}
    assert got == lc.FWD_INSTANCES, (sorted(lc.FWD_INSTANCES - got, key=str), sorted(got - lc.FWD_INSTANCES, key=str))
    # the groups of the issue's route table are what the lists' names say
    assert all(p['route'] == 'b3' and p['h'] == 2 for c in lc.FWD_B3_H2 for p in lc.fwd_plan(*c))
    assert all(p['route'] == 'b3' and p['h'] == 1 for c in lc.FWD_B3_H1 for p in lc.fwd_plan(*c))
    assert all(p['route'] == 'b3_k192' for c in lc.FWD_B3_K192 for p in lc.fwd_plan(*c))
    assert all(p['route'] == 'f32' for c in lc.FWD_F32 for p in lc.fwd_plan(*c))
    # a partial last 32-column tile (N = 70: NT = 3 with 6 columns in the third) with and without LayerNorm, on both bf16 routes
    for K in (32, 64, 96, 128, 192):
        for ln in (False, True):
            if K == 192 and not ln:
                continue
            assert any(T == 16401 and k == K and l == ln and not p['full_cols'] and p['nt'] == 3
                       for (T, N, k, l) in lc.FWD_CASES for p in lc.fwd_plan(T, N, k, l)), (K, ln)
    # a second tile per wave (the x prefetch is live) per K on every route that has large cases
    for K in lc.KS4:
        assert lc.fwd_plan(16401, 404, K)[0]['second_tile'] and not lc.fwd_plan(70, 404, K)[0]['second_tile']
    for ln in (False, True):
        assert lc.fwd_plan(32801, 96, 96, ln)[0]['second_tile'] and not lc.fwd_plan(16401, 96, 96, ln)[0]['second_tile']
    # epilogue variants: one N % 4 == 0 shape per route, with a tail launch
    want = {'b3_h2': ('b3', 2), 'b3_h1': ('b3', 1), 'b3_k192': ('b3_k192', 1), 'f32': ('f32', 1)}
    for name, (T, N, K) in lc.FWD_VARIANTS.items():
        plan = lc.fwd_plan(T, N, K)
        assert N % 4 == 0 and len(plan) == 2 and all((p['route'], p['h']) == want[name] for p in plan)


def test_the_heads_cases_reach_every_route():
    got = {(p['route'], p['h'], K) for (B, nv, G, K) in lc.HEADS_CASES for p in lc.fwd_plan(B * nv, 96 * G, K)}
    assert got == {('b3', 1, 96), ('b3', 2, 96), ('b3_k192', 1, 192), ('f32', 1, 96), ('f32', 1, 192)}
    for (B, nv, G, K) in lc.HEADS_CASES:
        assert nv >= 16 and nv % 16 != 0        # a 16-row tile straddles two batch items


def test_the_wgrad_cases_reach_every_instantiation():
    got = {lc.wgrad_plan(*c)['inst'] for c in lc.WGRAD_CASES}
    assert got == lc.WGRAD_INSTANCES, got
    got = {lc.wgrad_plan(*c, b3_env=False)['inst'] for c in lc.CHILD_WGRAD}
    assert got == lc.WGRAD_CHILD_INSTANCES, got
    plans = [lc.wgrad_plan(*c) for c in lc.WGRAD_CASES]
    assert any(p['nt'] % p['ntw'] != 0 for p in plans if p['kt'] == 1)           # a tile row group that is not full
    assert any(p['chunks'] > 32 for p in plans) and any(p['chunks'] == 1 for p in plans)   # both loops of the reduce kernel
    for K in (32, 64, 96, 128, 192):
        assert any(T % 8 != 0 and T > 1 for (T, N, k) in lc.WGRAD_CASES if k == K), K
        assert any(T == 1 for (T, N, k) in lc.WGRAD_CASES if k == K), K


def test_the_dgrad_cases_reach_every_route():
    got = {lc.dgrad_plan(*c)['inst'] for c in lc.DGRAD_CASES}
    assert got == lc.DGRAD_INSTANCES, got
    assert lc.dgrad_plan(16401, 96, 384)['second_tile'] and lc.dgrad_plan(16401, 200, 384)['second_tile']
    assert lc.dgrad_plan(65601, 104, 96)['second_tile'] and not lc.dgrad_plan(70, 104, 96)['second_tile']
    assert any(lc.dgrad_plan(*c)['npad'] != c[1] and lc.dgrad_plan(*c)['presplit'] for c in lc.DGRAD_CASES)   # zero-padded last chunk


def test_the_child_cases_take_the_f32_kernels_of_shapes_the_default_sends_to_b3():
    for (T, N, K) in lc.CHILD_FWD:
        assert all(p['route'] != 'f32' for p in lc.fwd_plan(T, N, K))
        assert all(p['route'] == 'f32' for p in lc.fwd_plan(T, N, K, b3_env=False))
    assert {K for (_, _, K) in lc.CHILD_FWD} == {32, 64, 96, 128, 192}


# ---- sharpness: faults in the emulation that the exact comparison must see ---------------------------------------------------------
@pytest.mark.parametrize("fam,term", [('A', (1, 1)), ('A', (2, 1)), ('A', (3, 1)), ('B', (1, 2)), ('B', (1, 3)), ('C', (2, 2))])
@pytest.mark.parametrize("R", [32, 64, 96, 128, 192])
def test_a_dropped_term_breaks_the_exact_comparison(fam, term, R):
    dense, sparse, want, _ = lc.make_pair(fam, 70, 116, R, seed=11)
    assert torch.equal(lc.emulate_b3(dense, sparse).double(), want)
    got = lc.emulate_b3(dense, sparse, drop=term).double()
    assert not torch.equal(got, want)
    assert float((got != want).double().mean()) > 0.5          # not a stray element: most outputs see it


@pytest.mark.parametrize("fam,which", [('A', 'dense'), ('B', 'sparse')])
@pytest.mark.parametrize("R", [32, 64, 96, 128, 192])
def test_a_third_plane_one_index_off_breaks_the_exact_comparison(fam, which, R):
    dense, sparse, want, _ = lc.make_pair(fam, 70, 116, R, seed=12)
    assert not torch.equal(lc.emulate_b3(dense, sparse, shift3=which).double(), want)


@pytest.mark.parametrize("T,N,K", [(70, 96, 96), (1003, 33, 32), (16401, 40, 192)])
def test_an_omitted_row_breaks_the_dense_wgrad_comparison(T, N, K):
    c = lc.wgrad_case('D', T, N, K)
    want = c['want_w'].t()
    assert torch.equal(lc.emulate_b3(c['dense'], c['sparse']).double(), want)
    for row in (0, T // 2, T - 1):
        got = lc.emulate_b3(c['dense'], c['sparse'], omit=row).double()
        assert bool((got != want).all())                       # every output misses the row
