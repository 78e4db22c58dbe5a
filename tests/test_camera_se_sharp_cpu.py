"""CPU: what the case table, the bounds and the kernel-order model of tests/camera_se_sharp_cases.py are worth (the GPU side:
tests/test_camera_se_sharp_gpu.py).

* the table holds exactly the (C, M) pairs selfocc_camera_se_supported accepts and the pixel counts on the kernels' edges;
* the exact family is exact: float32 equals float64 bit for bit in four summation orders (torch ascending, reversed, a seeded
  permutation, the kernel-order model) and 8 A < 2^24 everywhere;
* K per tensor is the smallest of 2, 4, 8 for which the kernel-order model is inside K max(e(port32), 1) on every case;
* every indexing defect of the model changes bits of the exact family in every case where it applies;
* every precision defect lands at least 2 x outside the random family's bound, on every raw tensor of every case."""
import numpy as np
import pytest
import torch

import camera_se_sharp_cases as sc

problem = sc.problem


def test_table_holds_every_supported_pair_and_every_edge():
    """the accepted set is read from the library when it is built (no GPU needed: a host function); the rule of cs_shape_ok
    restated otherwise, so that the table is checked on any machine"""
    grid = [(C, M) for C in range(16, 161, 16) for M in (C, 2 * C, 3 * C)]
    try:
        from selfocc_amd._lib import lib
        fn = lib().selfocc_camera_se_supported
        accepted = {(C, M) for C, M in grid if fn(2, 3, C, M, 8) == 1}
    except (OSError, RuntimeError) as e:
        print('library not loadable here, restating cs_shape_ok:', e)
        accepted = {(C, M) for C, M in grid if C in (32, 64, 96, 128) and M in (C, 2 * C) and M <= 192}
    assert accepted == set(sc.PAIRS) and len(sc.PAIRS) == 7
    for s in ('EDGE8', 'CHUNK4'):
        assert {(c.C, c.M) for c in sc.CASES if c.levels == s and (c.B, c.N) == (2, 3)} == set(sc.PAIRS), s
    hw = {s: [h * w for h, w in lv] for s, lv in sc.LEVELS.items()}
    assert hw == {'EDGE8': [1, 2, 3, 63, 64, 65, 255, 257], 'CHUNK4': [256, 511, 512, 513], 'ONE': [1025], 'PIXEL': [1]}
    assert any(s % 4 for s in np.cumsum(hw['EDGE8'])[:-1]) and any(s % 2 for s in np.cumsum(hw['EDGE8'])[:-1])     # odd level starts
    assert {c.levels for c in sc.CASES} == set(sc.LEVELS)
    assert [(c.B, c.N) for c in sc.CASES].count((1, 1)) == 1 and {(c.B, c.N) for c in sc.CASES} == {(2, 3), (1, 1)}
    assert max(sc.case_bytes(c) for c in sc.CASES) < 10e6
    assert len(sc.chunks_of(1025)) == 3 and len(sc.chunks_of(1025, sc.CS_TILE)) == 5 and 1025 % 64 == 1


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_exact_family_is_exact_in_any_order(c):
    inp, ref, A, yard = problem(c, 'exact')
    for k in sc.TENSORS:
        # every term a multiple of 1/8 and 8 A < 2^24; g_gate = sum_c dWc w has integer terms only, and A < 2^24 is what it needs
        # (its A reaches 3e6 at 1 792 pixels and 128 channels: 8 A would not fit, and need not)
        grain = 1.0 if k == 'g_gate' else 0.125
        assert float(sc.flat(A[k]).max()) / grain < 2.0 ** 24, (k, float(sc.flat(A[k]).max()))
        assert np.array_equal(sc.flat(ref[k]) / grain, np.round(sc.flat(ref[k]) / grain)), k
        assert yard[k] == 0.0, (k, yard[k])                                      # ascending: the torch float32 evaluation
    for order in ('reversed', 20261):
        got = sc.evaluate(inp, torch.float32, order=order)
        for k in sc.TENSORS:
            assert sc.bits_differing(got[k], ref[k]) == 0, (order, k)
    got = sc.model(inp)
    for k in sc.TENSORS:
        assert sc.bits_differing(got[k], ref[k]) == 0, ('kernel order', k)


def test_permuted_evaluation_is_the_same_function():
    """the reordered evaluations above compute the same tensors (float64, random family: differences at rounding level only)"""
    inp, ref, A, _ = problem(sc.CASES[0], 'random')
    for order in ('reversed', 20261):
        e = sc.figures(sc.evaluate(inp, torch.float64, order=order), ref, A)
        assert max(e.values()) < 1e-6, e


_MODEL = {}


def model_figures(c):
    if c not in _MODEL:
        inp, ref, A, yard = problem(c, 'random')
        _MODEL[c] = sc.figures(sc.model(inp), ref, A)
    return _MODEL[c]


def test_K_is_the_smallest_that_admits_the_kernel_order_model():
    worst = {k: 0.0 for k in sc.TENSORS}          # model / max(yardstick, 1)
    port = {k: 0.0 for k in sc.TENSORS}
    for c in sc.CASES:
        yard, e = problem(c, 'random')[3], model_figures(c)
        for k in sc.TENSORS:
            worst[k] = max(worst[k], e[k] / max(yard[k], 1.0))
            port[k] = max(port[k], yard[k])
    for k in sc.TENSORS:
        smallest = next((K for K in (2, 4, 8) if worst[k] <= K), None)
        print(f'{k}: K {smallest}  model / bound {worst[k] / sc.K[k]:.3f}  worst e(port32) {port[k]:.2f}')
        assert smallest == sc.K[k], (k, worst[k], sc.K[k])


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
@pytest.mark.parametrize("defect", sc.INDEX_DEFECTS)
def test_indexing_defect_changes_bits_of_the_exact_family(defect, c):
    if not sc.applies(defect, c):
        inp = problem(c, 'exact')[0]
        if defect in ('gate_row', 'cams_next', 'lvl_neighbour', 'drop_last_pixel'):      # then it changes nothing at all
            assert sc.bits_differing(sc.model_fwd(inp, defect), sc.model_fwd(inp)) == 0
        return
    inp, ref = problem(c, 'exact')[:2]
    hit = {'gate_row': ('out', 'dx'), 'drop_last_step': ('dWc', 'colsum'), 'colsum_row_past': ('colsum',)}.get(defect, ('out',))
    got = sc.model(inp, defect, hit)
    for k in hit:
        assert sc.bits_differing(got[k], ref[k]) > 0, (defect, k)
    if defect == 'colsum_row_past':               # the map operand of that row is zero: dWc does not move
        assert sc.bits_differing(sc.model(inp, defect, ('dWc',))['dWc'], ref['dWc']) == 0


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
@pytest.mark.parametrize("defect", sc.PRECISION_DEFECTS)
def test_precision_defect_is_twice_outside_every_raw_bound(defect, c):
    inp, ref, A, yard = problem(c, 'random')
    b = sc.bounds(yard)
    e = sc.figures(sc.model(inp, defect, sc.RAW), ref, A)
    print(defect, sc.case_id(c), {k: round(e[k] / b[k], 1) for k in sc.RAW})
    for k in sc.RAW:
        assert e[k] >= 2.0 * b[k], (defect, k, e[k], b[k])


def test_fma_rounds_once_where_it_matters():
    x = np.float32(1 + 2.0 ** -12)                # x x = 1 + 2^-11 + 2^-24: the product alone rounds the last term away
    assert float(sc.fma(x, x, np.float32(-1.0))) == 2.0 ** -11 + 2.0 ** -24
    assert float(np.float32(x * x) - np.float32(1.0)) == 2.0 ** -11
    assert sc._bf16(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1.0])).tolist() == [1.0, 1 + 2.0 ** -6, 1.0]      # ties to even
    assert sc._mant10(np.float32([1 + 2.0 ** -10 + 2.0 ** -11])).tolist() == [1 + 2.0 ** -10]
