"""No GPU: what makes tests/test_msda_sharp_gpu.py trustworthy.  The table of tests/msda_cases.py reaches every instantiation and
branch, as reported by the library's own host-only selfocc_msda_plan (not by a copy of its group choice); every case keeps at least
99 % of its location gradients (cap); the float32 evaluation of the port stays at or below ONE FIFTH of every bound (yardstick: the
bounds are not tighter than float32 allows); deliberately defective results exceed a bound at least TWICE (negative controls: the
bounds are not looser than the defects they are there to catch).  The defects are built on the reference side; no kernel is
involved."""
import math

import pytest
import torch

import msda_cases as mc


@pytest.fixture(scope="module", params=mc.REF_CASES, ids=mc.ref_id)
def ref(request):
    return mc.reference(request.param)


def _reached(cases):
    """what the `shape` sweep of the table reaches, from the plan entry alone"""
    fused, plain = set(), set()
    for c in cases:
        p = mc.plan(c)
        assert p.rc == 0, (mc.case_id(c), p.error)
        if c.sweep != 'shape':
            continue
        if c.form == 'plain':
            plain.add((c.d, p.log2_group, c.mode))
        else:
            fused.add((c.form, c.d, p.log2_group, c.bf16))
    return fused, plain


def _coverage_gaps(cases):
    """-> list of what the dispatch tables hold and `cases` do not reach"""
    fused, plain = _reached(cases)
    want_f = {(form, d, lg, bf) for form in ('fused', 'cross') for d, lg, bf in mc.FUSED_TABLE}
    want_p = {(d, lg, mode) for d, lg in mc.PLAIN_TABLE for mode in ('banded', 'atomic')}
    gaps = sorted(want_f - fused) + sorted(want_p - plain)
    assert not (fused - want_f) and not (plain - want_p), "the plan entry reports a shape outside the dispatch tables"
    cross = [(c, mc.plan(c)) for c in cases if c.form == 'cross']
    for name, vals in (('count_here', {p.count_here for _, p in cross}), ('bin_vis', {p.bin_vis for _, p in cross})):
        gaps += [(name, v) for v in (0, 1) if v not in vals]
    # count_here on both sides at ONE group size, with nothing else different
    pairs = {}
    for c, p in cross:
        if c.sweep == 'count':
            pairs.setdefault((c.d, p.log2_group, c.L, c.P), set()).add(p.count_here)
    if not any(v == {0, 1} for v in pairs.values()):
        gaps.append(('count_here at one group size', pairs))
    # the addressing variants: with both forms where they apply, at no fewer than two head widths
    variants = {
        'pixel-major': lambda c: not c.head_major, 'head-major': lambda c: c.head_major,
        'dense': lambda c: not c.merged, 'merged': lambda c: c.merged,
        'sink': lambda c: c.sink, 'fresh g_value': lambda c: not c.sink,
    }
    for name, has in variants.items():
        for form in ('fused', 'cross'):
            widths = {c.d for c in cases if c.form == form and has(c)}
            if len(widths) < 2:
                gaps.append((name, form, widths))
    for kind in (0, 1, 2):
        if len({c.d for c in cases if c.form == 'fused' and c.ref_kind == kind}) < 2:
            gaps.append(('ref_kind', kind))
    if len({c.d for c in cases if c.form == 'cross' and c.vstride}) < 2:
        gaps.append(('value_stride',))
    for n in (1, 2):
        if len({c.d for c in cases if c.form == 'cross' and c.n == n}) < 2:
            gaps.append(('cameras', n))
    for small in (True, False):
        if not any(c.form == 'cross' and (c.P < 4) == small for c in cases):
            gaps.append(('camera loop P < 4', small))
    for d in (4, 8, 16, 32):
        for form, mode in (('plain', 'banded'), ('plain', 'atomic'), ('fused', '')) if d > 4 else (('plain', 'banded'), ('plain', 'atomic')):
            if not any(c.sweep == 'seam' and c.form == form and c.d == d and c.mode == mode for c in cases):
                gaps.append(('seam', form, d, mode))
    return gaps


def test_the_table_reaches_every_instantiation():
    assert len(mc.FUSED_TABLE) == 20 and len(mc.PLAIN_TABLE) == 22
    assert len({mc.case_id(c) for c in mc.CASES}) == len(mc.CASES) == 40 + 2 + 44 + 8 + 3
    assert _coverage_gaps(mc.CASES) == []
    for c in mc.CASES:
        assert c.L <= 4 and c.sink <= (c.head_major and not c.bf16) and c.vstride <= (c.form == 'cross' and not c.head_major)
        if c.form == 'cross':        # queries seen by no camera, by all, and (two cameras) by one
            vis = mc.make_inputs(c).vis.sum(0)
            assert {0, c.n} <= set(vis.tolist()) and (c.n == 1 or 1 in vis.tolist())


def test_the_coverage_check_notices_any_missing_case():
    for i in range(len(mc.CASES)):
        assert _coverage_gaps(mc.CASES[:i] + mc.CASES[i + 1:]) != [], mc.case_id(mc.CASES[i])


def test_rounds_are_ragged_wherever_the_dispatch_allows():
    """every fused / camera-loop case takes at least two rounds per lane with a ragged last one"""
    for c in mc.CASES:
        if c.form != 'plain' and c.sweep == 'shape':
            G = 1 << mc.plan(c).log2_group
            assert c.L * c.P > G and (c.L * c.P) % G, mc.case_id(c)


def test_band_seam_cases_split_a_level_and_fill_a_list_segment():
    for c in mc.CASES:
        if c.sweep != 'seam':
            continue
        p = mc.plan(c)
        assert p.banded == 1 and max(p.bands) >= 2, (mc.case_id(c), p)
        r = mc.reference(c)
        _, y0 = mc.cells(r.inp, r.port)                     # (n, nq, heads, 1, P)
        H, rows = c.maps[0][0], p.rows[0]
        inside = (y0 >= -1) & (y0 < H)
        lower = y0 + 1
        straddle = inside & (lower % rows == 0) & (lower > 0) & (lower < H)
        assert straddle.sum() > 100, mc.case_id(c)
        per_band = torch.bincount((y0.clamp(0, H - 1) // rows)[inside].flatten(), minlength=p.bands[0])
        # a list is per (batch, head) plane and band; the points are spread evenly over the n * heads planes
        assert per_band.max().item() / (c.n * mc.HEADS) > mc.K_BAND_SEG * 1.1, (mc.case_id(c), per_band)


def test_shapes_that_are_not_built_are_refused_by_name():
    widths = b"msda fused / camera-loop forms: channels per head must be 8, 16 or 32 (got 4); the plain form takes 4"
    bf16_only = b"msda: bfloat16 value is built for 16 channels per head only (got %d)"
    for form, d, bf16, message in [('fused', 4, False, widths), ('fused', 8, True, bf16_only % 8), ('fused', 32, True, bf16_only % 32),
                                   ('cross', 4, False, widths)]:
        p = mc.plan_of(form, 2, 70, 2, d, 2, 18, mc.MAPS[:2], bf16)
        assert p.rc != 0 and p.error == message, (form, d, bf16, p)
    assert mc.plan_of('plain', 2, 70, 2, 6, 2, 18, mc.MAPS[:2]).rc != 0
    assert mc.plan_of('fused', 2, 70, 2, 16, 2, 129, mc.MAPS[:2]).rc != 0          # L * P > 256


def test_the_plan_entry_reports_the_band_decomposition():
    p = mc.plan_of('fused', 6, 22016, 6, 16, 4, 8, ((96, 200), (48, 100), (24, 50), (12, 25)))
    assert p.rc == 0 and p.banded == 1 and p.rows == [2, 4, 8, 12] and p.bands == [48, 12, 3, 1] and p.log2_group == 5
    assert mc.plan_of('fused', 1, 1000, 2, 16, 1, 4, ((8, 5000),)).banded == 0      # a level wider than the LDS tile


def test_bounds_are_five_times_their_yardsticks():
    """5.5 x the yardstick rounded up to one digit: between 5.5 x and (1.0x -> 2) 12 x"""
    for fam, b in mc.BOUNDS.items():
        assert set(b) == set(mc.METRICS)
        for k, (bound, yard) in b.items():
            digit = bound / 10 ** math.floor(math.log10(bound))
            assert 5.5 * yard <= bound <= 12 * yard and abs(digit - round(digit)) < 1e-9, (fam, k, bound, yard)
    for (cid, k), (fig, why) in mc.EXCEPTIONS.items():
        case = next(c for c in mc.CASES if mc.case_id(c) == cid)
        assert fig > mc.BOUNDS[mc.family(case)][k][0] and why


def test_cap(ref):
    """>= 99 % of the points keep their location gradient; the float32 and the float64 port put every kept point into the same cell"""
    kept = ref.keep.float().mean().item()
    print(f"\n[{mc.ref_id(ref.inp.case)}] points {ref.keep.numel() // 2} kept {kept:.5f}")
    assert kept >= 0.99
    p32 = mc.port(ref.inp, torch.float32)
    (x64, y64), (x32, y32) = mc.cells(ref.inp, ref.port), mc.cells(ref.inp, p32)
    same = (x64 == x32) & (y64 == y32)
    if ref.inp.case.form == 'cross':
        same = (same | ~ref.inp.vis[:, :, None, None, None]).all(0)
    assert bool(same[ref.keep[..., 0]].all())


def test_yardstick(ref):
    """the float32 port against the float64 port: <= 1 / 5 of every bound of the case's family"""
    p32 = mc.port(ref.inp, torch.float32)
    m = mc.metrics(ref, p32.out, p32.gv, p32.gp, p32.gw)
    print(f"\n[{mc.ref_id(ref.inp.case)}] float32 port: " + " ".join(f"{k} {v:.2e}" for k, v in m.items()))
    for k, (bound, _yard) in mc.BOUNDS[mc.family(ref.inp.case)].items():
        assert m[k] <= bound / 5, (k, m[k], bound)


def test_negative_controls(ref):
    """each defect moves at least one metric to >= 2 x its bound, for every route of the case (the bounds of a route may hold
    listed exceptions)"""
    inp, case = ref.inp, ref.inp.case
    defects = ['level', 'corner']
    if case.form != 'plain':
        defects.append('normaliser')
    if case.form == 'cross':
        defects.append('count')
    res = {}
    for name in defects:
        p = mc.port(inp, defect=name)
        res[name] = mc.metrics(ref, p.out, p.gv, p.gp, p.gw)
    if case.sweep == 'seam':
        p = mc.port(inp, defect='seam', rows=mc.plan(case).rows)
        res['seam'] = mc.metrics(ref, p.out, p.gv, p.gp, p.gw)
    routes = [c for c in mc.CASES if mc.ref_key(c) == case]
    for name, m in res.items():
        worst = min(max(m[k] / b[k] for k in m) for b in map(mc.bounds, routes))
        print(f"\n[{mc.ref_id(case)}] control {name}: {worst:.0f} x  " + " ".join(f"{k} {v:.2e}" for k, v in m.items()))
        assert worst >= 2, (name, m)
