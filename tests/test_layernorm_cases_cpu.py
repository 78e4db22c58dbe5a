"""CPU: what the case table, the host model and the bounds of tests/layernorm_cases.py are worth (the GPU side:
tests/test_layernorm_sharp_gpu.py).

* the host model — the kernels of csrc/layernorm.hip restated in numpy float32 — is within every bound of every case, at most half
  way to the bounds of the two ill-conditioned families (K is twice its worst ratio to the float32 port);
* every defect that can be switched on in the model is at least a factor 2 outside the bound of some tensor, in the case that
  exists for it; the float64 reference scaled by 1.001 fails the plain family at every width, tensor by tensor;
* the inputs are what the table says they are (no cancellation in the parameter gradients, exact partial sums in constant rows);
* the table reaches all 32 widths, block counts 1, 8, 9, 64, 65 and 2 048 and 1, 2 and 3 trips of the row loop."""
import math

import numpy as np
import pytest

import layernorm_cases as lc


def _first(**kw):
    for c in lc.CASES:
        if all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError(kw)


def _worst_excess(c, defect):
    """the largest figure / bound over the tensors of a case with a defect switched on, and the constant-row failures"""
    recs, bad = lc.check_case(c, lambda p: lc.host_model(p, defect))
    return max((fig / b if b > 0 else (math.inf if fig > 0 else 0.0)) for _g, _k, fig, b, _p in recs), bad


def test_host_model_is_within_every_bound():
    worst = {fam: dict.fromkeys(lc.TENSORS, 0.0) for fam in lc.FAMILIES}
    for c in lc.CASES:
        recs, bad = lc.check_case(c, lc.host_model)
        assert not bad, (lc.case_id(c), bad)
        for gi, k, fig, b, pf in recs:
            assert fig <= b, (lc.case_id(c), gi, k, fig, b, pf)
            worst[c.family][k] = max(worst[c.family][k], fig / lc.yardstick(pf))
    for fam in lc.FAMILIES:
        print(fam, 'host model / yardstick, worst per tensor:', {k: round(v, 2) for k, v in worst[fam].items()})
        # K is twice the measured worst, rounded up: the model uses at most half of the bound, and K is not larger than that needs
        if fam != 'plain':
            top = max(worst[fam].values())
            assert math.ceil(2 * top) == lc.K[fam], (fam, top, lc.K[fam])
            assert abs(top - max(lc.MEASURED[fam].values())) <= 0.01, (fam, top)


DEFECT_CASES = [
    ('one_pass', dict(kind='width', family='offset', C=96, eps=1e-5)),
    ('one_pass', dict(kind='rows', family='offset', rows=16385)),
    ('eps_outside', dict(kind='width', family='small', C=96, eps=1e-5)),
    ('eps_outside', dict(kind='width', family='small', C=100, eps=1e-3)),
    ('c_minus_1', dict(kind='width', family='plain', C=128, eps=1e-5)),
    ('b_scale', dict(kind='width', family='plain', C=96, eps=1e-5)),
    ('b_scale', dict(kind='width', family='plain', C=4, eps=1e-5)),
    ('second_trip', dict(kind='rows', family='plain', rows=16385, C=96)),
    ('second_trip', dict(kind='rows', family='plain', rows=16385, C=4)),
    ('second_trip', dict(kind='rows', family='plain', rows=32773, C=128)),
    ('half_wave', dict(kind='rows', family='plain', rows=1, C=4)),
    ('half_wave', dict(kind='rows', family='plain', rows=16384, C=100)),
    ('half_wave', dict(kind='width', family='small', C=52, eps=1e-3)),
    ('reduce_tail', dict(kind='rows', family='plain', rows=513, C=96)),
    ('reduce_tail', dict(kind='rows', family='plain', rows=513, C=4)),
    ('reduce_tail', dict(kind='rows', family='plain', rows=16385, C=128)),
]


@pytest.mark.parametrize("defect,where", DEFECT_CASES, ids=lambda v: v if isinstance(v, str) else '-'.join(f'{k}{x}' for k, x in v.items()))
def test_defect_fails_a_bound_by_a_factor_of_two(defect, where):
    c = _first(**where)
    excess, _bad = _worst_excess(c, defect)
    print(defect, lc.case_id(c), 'figure / bound', excess)
    assert excess >= 2.0, (defect, lc.case_id(c), excess)


@pytest.mark.parametrize("C", [w for w in lc.WIDTHS if w < 128])
def test_unmasked_inactive_lanes_fail_at_every_width_below_128(C):
    for fam in lc.FAMILIES:
        c = _first(kind='width', family=fam, C=C, eps=1e-5)
        excess, _bad = _worst_excess(c, 'no_mask')
        assert excess >= 2.0, (lc.case_id(c), excess)
    # at 128 every lane is active: the defect changes nothing
    c = _first(kind='width', family='plain', C=128, eps=1e-5)
    p = lc.problems(c)[0][2]
    a, b = lc.host_model(p), lc.host_model(p, 'no_mask')
    assert all(np.array_equal(a[k], b[k]) for k in lc.TENSORS)


def test_eps_outside_fails_the_constant_row_rstd_check():
    for c in (c for c in lc.CASES if c.kind == 'const'):
        p = lc.problems(c)[0][2]
        bad = lc.constant_row_checks(p, lc.host_model(p, 'eps_outside'))
        n_const = int((~np.isnan(p.const.numpy())).sum())
        assert n_const >= 12 and sum(1 for what, *_ in bad if what.startswith('rstd')) == n_const, (lc.case_id(c), bad[:3])
        for what, val, lim in bad:
            if what.startswith('rstd'):
                assert val >= 2 * lim


@pytest.mark.parametrize("C", lc.WIDTHS)
def test_reference_scaled_by_a_thousandth_fails_plain_at_every_width(C):
    c = _first(kind='width', family='plain', C=C, eps=1e-5)
    p = lc.problems(c)[0][2]
    ref = lc.reference64(p)
    b = lc.bounds('plain', lc.figures(lc.port32(p), ref))
    for k in ('y', 'dx', 'dgamma', 'dbeta'):
        scaled = dict(ref)
        scaled[k] = ref[k] * 1.001
        fig = lc.figures(scaled, ref)
        assert fig[k] >= 2 * b[k], (C, k, fig[k], b[k])
        assert all(fig[o] == 0 for o in lc.TENSORS if o != k)


def test_input_conditions():
    worst = 0.0
    n_const = 0
    for c in lc.CASES:
        for _gi, _r0, p in lc.problems(c):
            ratio, exact = lc.check_conditions(p)
            assert ratio <= 4.0, (lc.case_id(c), ratio)
            assert exact, lc.case_id(c)
            worst = max(worst, ratio)
            cm = ~np.isnan(p.const.numpy())
            n_const += int(cm.sum())
            if c.kind == 'const':
                assert set(p.const.numpy()[cm]) == set(lc.CONSTANTS) and (~cm).sum() > cm.sum()      # mixed among plain rows
    print('sum |term| / largest |sum|, worst:', worst, '; constant rows:', n_const)
    assert n_const > 0


def test_families_are_what_they_claim():
    """offset: |mean| / sigma ~ 1e3 with both signs; small: var <= eps / 5 for both eps"""
    c = _first(kind='width', family='offset', C=96, eps=1e-5)
    x = lc.make_inputs(c)[0].double()
    assert ((x.mean(1).abs() / x.std(1)) > 500).all() and (x.mean(1) > 0).any() and (x.mean(1) < 0).any()
    c = _first(kind='width', family='small', C=96, eps=1e-5)
    x = lc.make_inputs(c)[0].double()
    assert (x.var(1, unbiased=False) <= 1e-5 / 5).all()


def test_coverage():
    assert {c.C for c in lc.CASES if c.kind == 'width'} == set(range(4, 129, 4)) and len(lc.WIDTHS) == 32
    for fam in lc.FAMILIES:
        for eps in lc.EPS:
            assert {c.C for c in lc.CASES if c.kind == 'width' and c.family == fam and c.eps == eps} == set(lc.WIDTHS)
    sizes = [n for c in lc.CASES for n in (c.sizes or (c.rows,)) if n]
    assert {1, 8, 9, 64, 65, 2048} <= {lc.ln_blocks(n) for n in sizes}
    assert {lc.trips(n) for n in sizes} == {1, 2, 3}
    assert lc.trips(16384) == 1 and lc.trips(16385) == 2 and lc.ln_blocks(513) == 65 and lc.ln_blocks(512) == 64
    assert max(c.rows * c.C for c in lc.CASES) == 32773 * 128
    assert {c.rows for c in lc.CASES if c.kind == 'rows' and c.family == 'plain'} == set(lc.ROWS)
    assert {c.rows for c in lc.CASES if c.family == 'offset' and c.kind == 'rows'} == {16383, 16384, 16385, 16391}
    assert {(c.sizes, c.C) for c in lc.CASES if c.kind == 'group'} == {(s, C) for s in lc.SPLITS for C in lc.SPLIT_WIDTHS}


def test_fma32_rounds_once():
    """float32 neighbours 16777218 and 16777220, half-way 16777219.  (1 + 2^-20)(1 - 2^-20) + 16777218 = 16777219 - 2^-40 lies below
    it, but is no float64: the float64 sum is the half-way point itself, and rounding that again goes to the even 16777220"""
    f32 = np.float32
    x, y, z = f32(1 + 2.0 ** -20), f32(1 - 2.0 ** -20), f32(16777218.0)
    assert np.float32(np.float64(x) * np.float64(y) + np.float64(z)) == 16777220.0          # rounded twice
    assert float(lc.fma32(x, y, z)) == 16777218.0                                            # rounded once
    # -16777217 - 2^-40 (twice: the even -16777216) and -16777219 + 2^-40 (twice: the even -16777220)
    assert float(lc.fma32(x, y, -z)) == -16777218.0 and float(lc.fma32(-x, y, -z)) == -16777218.0
    assert float(lc.fma32(f32(1), f32(1), z)) == 16777220.0                                  # a true tie: to even
    assert float(lc.fma32(x, x, z)) == 16777220.0                                            # above it
    got = lc.fma32(np.array([x, 1, 3], f32), np.array([y, 1, 0.5], f32), np.array([z, z, 0.25], f32))
    assert got.dtype == np.float32 and got.tolist() == [16777218.0, 16777220.0, 1.75]
