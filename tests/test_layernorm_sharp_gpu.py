"""GPU: the LayerNorm kernels (csrc/layernorm.hip) through their raw entries, on the table of tests/layernorm_cases.py — all 32
widths in three input families and two eps, the rows on both sides of every launch edge (the 8-row block, the reduce kernel's second
trip at 513 rows, the 2 048-block cap at 16 385 rows, three trips), constant rows, row groups.

* y, mean, rstd, dx, dgamma, dbeta against float64 within K x the float32 port's own error in the same case (plain: K = 5; the
  derived bounds of constant rows), outputs filled with NaN in front of four guard rows: every element written, no guard touched;
  a second launch gives the same bits; the forward without mean / rstd gives the bits of the one with them;
* all six tensors bit for bit equal to the numpy float32 model of the kernels (layernorm_cases.host_model);
* row groups: every group's rows and its dgamma / dbeta row are the bits of the ungrouped entry on that slice with that group's
  parameters, empty groups give exact zeros;
* refusals by name with the outputs untouched, among them every pointer that is not 16-byte aligned (never launched);
* the Python route (FastLayerNorm / _LayerNormFunction): non-contiguous input, a stride-0 dy, the nn.LayerNorm fallback widths and
  eps from build_norm_layer, by value; x and dy as contiguous views at element offsets 1, 2, 3 give the bits of the aligned call.

What the table and the bounds are worth: tests/test_layernorm_cases_cpu.py.  Every case appends its figures (kernel / bound,
port32 / bound, bits differing from the model) to layernorm_sharp.jsonl next to the render tests' log (one full run:
profiles/layernorm_sharp_parity.jsonl)."""
import json
import os

import numpy as np
import pytest
import torch

import layernorm_cases as lc
from test_render_bwd_gpu import LOG as TRAIN_SHAPE_LOG

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(TRAIN_SHAPE_LOG), "layernorm_sharp.jsonl")
SENTINEL = -12345.0
GUARD = 4


def _guarded(n, *tail):
    """(n + 4, ...) buffer: the n rows NaN, four guard rows of a sentinel behind them"""
    t = torch.full((n + GUARD, *tail), float('nan'), device=D0)
    t[n:] = SENTINEL
    return t


def _guards_intact(bufs, ns):
    return all(bool((b[n:] == SENTINEL).all()) for b, n in zip(bufs, ns))


def _launch(hip, x, dy, gamma, beta, eps, sizes=None, stats=True):
    """raw entries, grouped when `sizes` is given.  gamma, beta: (G, C).  -> dict of CPU tensors (dgamma, dbeta: (G, C)); without
    `stats` the forward alone, with mean = rstd = NULL"""
    from selfocc_amd import abi
    from selfocc_amd._lib import check, ptr, current_stream
    T, C = x.shape
    G = gamma.shape[0]
    assert sizes is not None or G == 1
    xd, dyd, gd, bd = (t.to(D0).contiguous() for t in (x, dy, gamma, beta))
    y, dx, mean, rstd = _guarded(T, C), _guarded(T, C), _guarded(T), _guarded(T)
    dg, db = _guarded(G, C), _guarded(G, C)
    groups = () if sizes is None else (abi.SoRowGroups.from_sizes(sizes),)
    fwd, bwd, wsp = ((hip.selfocc_layernorm_fwd, hip.selfocc_layernorm_bwd, hip.selfocc_layernorm_bwd_workspace) if sizes is None else
                     (hip.selfocc_layernorm_fwd_grouped, hip.selfocc_layernorm_bwd_grouped, hip.selfocc_layernorm_bwd_grouped_workspace))
    st = current_stream(D0)
    check(fwd(ptr(xd), ptr(gd), ptr(bd), ptr(y), ptr(mean) if stats else None, ptr(rstd) if stats else None, T, C, eps, *groups, st),
          "fwd")
    if stats:
        nbytes = int(wsp(T, C, *groups))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=D0)
        check(bwd(ptr(xd), ptr(gd), ptr(mean), ptr(rstd), ptr(dyd), ptr(dx), ptr(dg), ptr(db), T, C, *groups, ptr(ws), nbytes, st), "bwd")
    torch.cuda.synchronize()
    assert _guards_intact((y, dx, mean, rstd, dg, db), (T, T, T, T, G, G)), "a guard row was written"
    out = dict(y=y[:T], mean=mean[:T], rstd=rstd[:T], dx=dx[:T], dgamma=dg[:G], dbeta=db[:G])
    if not stats:
        assert all(bool(torch.isnan(out[k]).all()) for k in ('mean', 'rstd', 'dx', 'dgamma', 'dbeta'))
        out = dict(y=out['y'])
    return {k: v.cpu() for k, v in out.items()}


def _bits_differing(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


def _append(rec):
    print("\n" + json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_kernels_vs_float64_and_host_model(hip, case):
    x, gamma, beta, dy, _const = lc.make_inputs(case)
    got = _launch(hip, x, dy, gamma, beta, case.eps, case.sizes)
    for k in lc.TENSORS:          # every output element written (the inputs are finite, eps > 0)
        assert bool(torch.isfinite(got[k]).all()), k
    again = _launch(hip, x, dy, gamma, beta, case.eps, case.sizes)
    assert all(torch.equal(got[k], again[k]) for k in lc.TENSORS), "two launches differ"
    assert torch.equal(_launch(hip, x, dy, gamma, beta, case.eps, case.sizes, stats=False)['y'], got['y'])
    failures = []
    for gi, r0, p in lc.problems(case):
        n = p.x.shape[0]
        mine = {k: (got[k][gi] if k in ('dgamma', 'dbeta') else got[k][r0:r0 + n]).numpy() for k in lc.TENSORS}
        if case.sizes:            # a group = the ungrouped entry on its rows with its parameters, same bits
            alone = _launch(hip, p.x, p.dy, p.gamma[None], p.beta[None], case.eps)
            for k in lc.TENSORS:
                a = alone[k][0] if k in ('dgamma', 'dbeta') else alone[k]
                assert _bits_differing(a.numpy(), mine[k]) == 0, (gi, k, 'grouped != ungrouped')
        rec, bad = lc.check_problem(case.family, p, mine)
        model = lc.host_model(p)
        bits = {k: _bits_differing(mine[k], model[k]) for k in lc.TENSORS}
        _append(dict(case=lc.case_id(case), group=gi, rows=n, C=case.C, family=case.family, eps=case.eps, blocks=lc.ln_blocks(n),
                     trips=lc.trips(n), kernel_over_bound={k: (v[0] / v[1] if v[1] else 0.0) for k, v in rec.items()},
                     port32_over_bound={k: (v[2] / v[1] if v[1] else 0.0) for k, v in rec.items()}, bits_differing=bits,
                     constant_row_failures=len(bad)))
        failures += [(gi, k, 'bound', *v) for k, v in rec.items() if not v[0] <= v[1]]
        failures += [(gi, 'constant row', *b) for b in bad]
        failures += [(gi, k, 'bits differing from the host model', v) for k, v in bits.items() if v]
    for gi, n in enumerate(case.sizes or ()):
        if n == 0:
            assert not got['dgamma'][gi].any() and not got['dbeta'][gi].any(), gi
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: by name, before anything is launched
# ------------------------------------------------------------------------------------------------------------------------------
class _Raw:
    """buffers of a small aligned call (rows 16, C 8, G groups) and the four entries with every argument replaceable"""

    def __init__(self, hip, rows=16, C=8, G=1):
        from selfocc_amd._lib import current_stream
        self.hip, self.rows, self.C, self.G = hip, rows, C, G
        self.st = current_stream(D0)
        # inputs with room around them, so that a pointer 4 bytes further still lies inside the allocation
        self.x, self.dy = torch.randn(rows + 1, C, device=D0), torch.randn(rows + 1, C, device=D0)
        self.gamma, self.beta = torch.ones(G + 1, C, device=D0), torch.zeros(G + 1, C, device=D0)
        self.mean, self.rstd = torch.zeros(rows, device=D0), torch.ones(rows, device=D0)
        self.ws = torch.empty(int(hip.selfocc_layernorm_bwd_workspace(rows, C)) + 64, dtype=torch.uint8, device=D0)
        self.outs = dict(y=_guarded(rows + 1, C), dx=_guarded(rows + 1, C), mean_o=_guarded(rows), rstd_o=_guarded(rows),
                         dgamma=_guarded(G, C), dbeta=_guarded(G, C))

    def p(self, name, shift=0):
        from selfocc_amd._lib import ptr
        import ctypes
        t = self.outs[name] if name in self.outs else getattr(self, name)
        return ctypes.c_void_p(t.data_ptr() + shift) if shift else ptr(t)

    def groups(self, sizes=None):
        from selfocc_amd import abi
        return abi.SoRowGroups.from_sizes(sizes if sizes is not None else [self.rows] + [0] * (self.G - 1))

    def fwd(self, grouped=False, rows=None, C=None, shift=(), mean=True, rstd=True, sizes=None):
        q = lambda n: self.p(n, 4 if n in shift else 0)
        rows, C = self.rows if rows is None else rows, self.C if C is None else C
        args = (q('x'), q('gamma'), q('beta'), q('y'), self.p('mean_o') if mean else None, self.p('rstd_o') if rstd else None, rows, C, 1e-5)
        if grouped:
            return self.hip.selfocc_layernorm_fwd_grouped(*args, self.groups(sizes), self.st)
        return self.hip.selfocc_layernorm_fwd(*args, self.st)

    def bwd(self, grouped=False, rows=None, C=None, shift=(), short=0, sizes=None):
        q = lambda n: self.p(n, 4 if n in shift else 0)
        rows, C = self.rows if rows is None else rows, self.C if C is None else C
        gr = (self.groups(sizes),) if grouped else ()
        need = int((self.hip.selfocc_layernorm_bwd_grouped_workspace if grouped else self.hip.selfocc_layernorm_bwd_workspace)(
            self.rows, self.C, *((self.groups(),) if grouped else ())))
        args = (q('x'), q('gamma'), self.p('mean'), self.p('rstd'), q('dy'), q('dx'), self.p('dgamma'), self.p('dbeta'), rows, C, *gr,
                self.p('ws'), need - short, self.st)
        return (self.hip.selfocc_layernorm_bwd_grouped if grouped else self.hip.selfocc_layernorm_bwd)(*args)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t[:-GUARD]).all()) and bool((t[-GUARD:] == SENTINEL).all()) for t in self.outs.values())


def _refused(hip, r, rc, *words):
    msg = hip.selfocc_last_error().decode()
    assert rc != 0, ('accepted', words)
    for w in words:
        assert w in msg, (w, msg)
    assert r.untouched(), ('outputs written', msg)


@pytest.mark.parametrize("grouped", [False, True], ids=['plain', 'grouped'])
def test_refusals_name_the_cause_and_write_nothing(hip, grouped):
    r = _Raw(hip, G=2 if grouped else 1)
    for C in (0, 2, 6, 130, 132):
        _refused(hip, r, r.fwd(grouped, C=C), 'layernorm', 'C must be a multiple of 4 in [4, 128]', f'got {C}')
        _refused(hip, r, r.bwd(grouped, C=C), 'layernorm', 'C must be a multiple of 4 in [4, 128]', f'got {C}')
    _refused(hip, r, r.fwd(grouped, rows=-1), 'rows must be >= 0')
    _refused(hip, r, r.bwd(grouped, rows=-1), 'rows must be >= 0')
    _refused(hip, r, r.fwd(grouped, rstd=False), 'mean and rstd go together')
    _refused(hip, r, r.fwd(grouped, mean=False), 'mean and rstd go together')
    _refused(hip, r, r.bwd(grouped, short=1), 'workspace too small')
    if grouped:
        _refused(hip, r, r.fwd(True, sizes=[2] * 8 + [0]), 'n_groups must be in [1, 8]', 'got 9')
        _refused(hip, r, r.bwd(True, sizes=[2] * 8 + [0]), 'n_groups must be in [1, 8]', 'got 9')
        _refused(hip, r, r.fwd(True, sizes=[8, 7]), 'row_start[n_groups] = 15 must equal rows = 16')
        _refused(hip, r, r.bwd(True, sizes=[8, 7]), 'row_start[n_groups] = 15 must equal rows = 16')
        assert hip.selfocc_layernorm_grouped_supported(16, 8, r.groups([8, 7])) < 0
        assert hip.selfocc_layernorm_bwd_grouped_workspace(16, 8, r.groups([8, 7])) == 0


@pytest.mark.parametrize("grouped", [False, True], ids=['plain', 'grouped'])
def test_entries_refuse_a_misaligned_pointer_by_name(hip, grouped):
    """a pointer 4 bytes into an allocation: refused before the launch, named, nothing written.  (Such a pointer is never given to
    a kernel: what the hardware does with a misaligned 16-byte access is not measured here.)"""
    r = _Raw(hip, G=2 if grouped else 1)
    for name in ('x', 'gamma', 'beta', 'y'):
        _refused(hip, r, r.fwd(grouped, shift=(name,)), 'layernorm: ' + name + ' must be 16-byte aligned')
    for name in ('x', 'gamma', 'dy', 'dx'):
        _refused(hip, r, r.bwd(grouped, shift=(name,)), 'layernorm_bwd: ' + name + ' must be 16-byte aligned')
    # the same buffers, aligned: accepted
    assert r.fwd(grouped) == 0 and r.bwd(grouped) == 0
    torch.cuda.synchronize()
    assert not r.untouched()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python route
# ------------------------------------------------------------------------------------------------------------------------------
def _problem(C, rows=67, eps=1e-5, ones=False, seed=0):
    g = torch.Generator().manual_seed(424200 + 1000 * seed + C)
    x = torch.randn(rows, C, generator=g) * 3.0 + 1.5
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.1
    dy = torch.ones(rows, C) if ones else (0.7 + 0.5 * lc._xhat64(x, eps) + 0.5 * torch.randn(rows, C, generator=g).double()).float()
    return lc.Problem(x, gamma, beta, dy, eps, torch.full((rows,), float('nan'), dtype=torch.float64))


def _module_for(p, ln=None):
    from selfocc_amd.model.bricks import FastLayerNorm
    ln = (FastLayerNorm(p.x.shape[1], eps=p.eps) if ln is None else ln).to(D0)
    with torch.no_grad():
        ln.weight.copy_(p.gamma)
        ln.bias.copy_(p.beta)
    return ln


VALUE_TENSORS = ('y', 'dx', 'dgamma', 'dbeta')


def _check_values(p, ln, y, x):
    got = dict(y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dgamma=ln.weight.grad.cpu().numpy(), dbeta=ln.bias.grad.cpu().numpy())
    rec, _bad = lc.check_problem('plain', p, got, VALUE_TENSORS)
    print({k: (v[0], v[1]) for k, v in rec.items()})
    for k, (fig, bound, _pf) in rec.items():
        assert fig <= bound, (k, fig, bound)
    return got


@pytest.mark.parametrize("C", [96, 100])
def test_module_on_a_transposed_input(hip, C):
    p = _problem(C)
    ln = _module_for(p)
    xt = p.x.t().contiguous().to(D0).requires_grad_(True)          # (C, rows): its transpose is no contiguous tensor
    x = xt.t()
    assert not x.is_contiguous()
    x.retain_grad()
    y = ln(x)
    y.backward(p.dy.to(D0))
    _check_values(p, ln, y, x)


@pytest.mark.parametrize("C", [96, 100])
def test_module_with_a_stride_zero_dy(hip, C):
    p = _problem(C, ones=True)
    ln = _module_for(p)
    x = p.x.to(D0).requires_grad_(True)
    y = ln(x)
    y.sum().backward()
    _check_values(p, ln, y, x)


@pytest.mark.parametrize("C", [30, 132])
def test_module_fallback_widths_by_value(hip, C):
    """C % 4 != 0 or C > 128: nn.LayerNorm serves them — by value now, not by shape"""
    p = _problem(C)
    ln = _module_for(p)
    x = p.x.to(D0).requires_grad_(True)
    y = ln(x)
    y.backward(p.dy.to(D0))
    _check_values(p, ln, y, x)


@pytest.mark.parametrize("C", [96, 52])
def test_eps_of_build_norm_layer_reaches_the_kernel(hip, C):
    from selfocc_amd.model.bricks import build_norm_layer, FastLayerNorm
    name, ln = build_norm_layer(dict(type='LN', eps=1e-3), C)
    assert isinstance(ln, FastLayerNorm) and ln.eps == 1e-3
    # the small family: var = 1e-6, so that eps = 1e-3 against the default 1e-5 is a factor 10 in y
    g = torch.Generator().manual_seed(77 + C)
    x = torch.randn(67, C, generator=g) * 1e-3 + 0.25
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.1
    dy = (0.7 + 0.5 * lc._xhat64(x, 1e-3) + 0.5 * torch.randn(67, C, generator=g).double()).float()
    p = lc.Problem(x, gamma, beta, dy, 1e-3, torch.full((67,), float('nan'), dtype=torch.float64))
    ln = _module_for(p, ln)
    xd = x.to(D0).requires_grad_(True)
    y = ln(xd)
    y.backward(dy.to(D0))
    got = dict(y=y.detach().cpu().numpy(), dx=xd.grad.cpu().numpy(), dgamma=ln.weight.grad.cpu().numpy(), dbeta=ln.bias.grad.cpu().numpy())
    rec, _bad = lc.check_problem('small', p, got, VALUE_TENSORS)
    for k, (fig, bound, _pf) in rec.items():
        assert fig <= bound, (k, fig, bound)


@pytest.mark.parametrize("C", [96, 100])
def test_views_at_odd_storage_offsets_give_the_bits_of_the_aligned_call(hip, C):
    """x and dy as contiguous views 1, 2 and 3 floats into a larger buffer: _LayerNormFunction re-stages them"""
    p = _problem(C, seed=1)
    rows = p.x.shape[0]

    def run(off):
        ln = _module_for(p)
        if off is None:
            x, dy = p.x.to(D0), p.dy.to(D0)
        else:
            bx, bd = torch.zeros(rows * C + 8, device=D0), torch.zeros(rows * C + 8, device=D0)
            x, dy = bx[off:off + rows * C].view(rows, C), bd[off:off + rows * C].view(rows, C)
            x.copy_(p.x)
            dy.copy_(p.dy)
            assert x.is_contiguous() and x.data_ptr() % 16 == 4 * off and dy.data_ptr() % 16 == 4 * off
        x = x.detach().requires_grad_(True)
        y = ln(x)
        y.backward(dy)
        with torch.no_grad():
            y0 = ln(x.detach())                      # the no-grad route
        return y.detach(), y0, x.grad, ln.weight.grad, ln.bias.grad

    want = run(None)
    for off in (1, 2, 3):
        got = run(off)
        for name, a, b in zip(('y', 'y no_grad', 'dx', 'dgamma', 'dbeta'), got, want):
            assert torch.equal(a, b), (off, name)
    assert torch.equal(want[0], want[1])
