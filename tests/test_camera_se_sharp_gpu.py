"""GPU: the fused CameraAwareSE flatten (csrc/camera_se.hip) through its raw C entries, on the table of
tests/camera_se_sharp_cases.py: all seven (C, M) pairs — every instantiation of the forward, dgrad and wgrad templates — at
(B, N) = (2, 3), levels of 1, 2, 3, 63, 64, 65, 255, 257 / 256, 511, 512, 513 / 1025 / 1 pixels, two input families.

* out, every dfeat, dWc (B N, C, M) and colsum (L, N, C) — the kernels' raw outputs, not their folds — against float64:
  the exact family bit for bit, the random family per element within K[t] max(e(port32), 1) units of 2^-24 A (what the unit, K
  and the yardstick are worth: tests/test_camera_se_sharp_cpu.py);
* every output starts as NaN between two guard blocks, the workspace as NaN with a sentinel excess behind what
  selfocc_camera_se_flatten_bwd_workspace reports: no NaN is left in an output (so the reduce kernel read only partials the
  wgrad kernel wrote), every partial was written, no guard and no excess byte was touched;
* dfeat subsets (NULL altogether, even levels, the last level): the wanted gradients, dWc and colsum keep their bits, the
  unwanted buffers their fill;
* the Python route (_CameraSeFlatten.apply with a given gate) at (B, N) = (2, 3): value, the map gradients and the five folded
  gradients, bit for bit on the exact family, within the bounds on the random one; maps and upstream gradient as views 1, 2, 3
  floats off a 16-byte boundary give the aligned call's bits;
* refusals by name, before any launch, outputs untouched.

Every case appends its figures to parity_out/camera_se_sharp_parity.jsonl (one full run: profiles/camera_se_sharp_parity.jsonl)."""
import ctypes
import json
import math
import os

import pytest
import torch

import camera_se_sharp_cases as sc

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "camera_se_sharp_parity.jsonl")
SENTINEL = -12345.0
GUARD = 64                 # floats: 256 bytes, so that the guarded block keeps the allocation's alignment
WS_EXCESS = 1024           # floats behind the workspace the entry asks for


class Guarded:
    """`shape` floats of NaN between two guard blocks of a sentinel"""

    def __init__(self, shape):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device=D0)
        self.buf[GUARD:GUARD + self.n] = float('nan')
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return self.guards_intact() and bool(torch.isnan(self.t).all())


def _append(rec):
    print("\n" + json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def _device(inp):
    return {k: [m.to(D0).contiguous() for m in v] if k == 'maps' else v.to(D0).contiguous() for k, v in inp.items()}


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def launch(hip, d, wanted='all'):
    """forward and backward through the raw entries on device inputs `d`.  wanted: 'all', None (d_feats = NULL) or the set of
    levels whose gradient is asked for.  -> CPU tensors out, dx (list; None where not wanted), dWc, colsum"""
    from selfocc_amd._lib import check, ptr, current_stream
    maps = d['maps']
    B, N, M = maps[0].shape[:3]
    C, L = d['w'].shape[0], len(maps)
    hw = [m.shape[3] * m.shape[4] for m in maps]
    hwa, st = (ctypes.c_int32 * L)(*hw), current_stream(D0)
    out = Guarded((N, sum(hw), B, C))
    check(hip.selfocc_camera_se_flatten_fwd(_ptrs(maps), hwa, L, B, N, C, M, ptr(d['gate']), ptr(d['w']), ptr(d['bias']), ptr(d['cams']),
                                            ptr(d['lvls']), ptr(out.t), st), "selfocc_camera_se_flatten_fwd")
    dxs = [Guarded(tuple(m.shape)) for m in maps]
    asked = set(range(L)) if wanted == 'all' else set(wanted or ())
    dptrs = None if wanted is None else _ptrs([dxs[l].t if l in asked else None for l in range(L)])
    dwc, col = Guarded((B * N, C, M)), Guarded((L, N, C))
    need = int(hip.selfocc_camera_se_flatten_bwd_workspace(hwa, L, B, N, C, M))
    chunks = sum(len(sc.chunks_of(h)) for h in hw)
    assert need == 4 * B * N * chunks * (C * M + C), (need, chunks)
    ws = torch.full((need // 4 + WS_EXCESS,), SENTINEL, device=D0)
    ws[:need // 4] = float('nan')
    check(hip.selfocc_camera_se_flatten_bwd(ptr(d['g']), _ptrs(maps), hwa, L, B, N, C, M, ptr(d['gate']), ptr(d['w']), dptrs, ptr(dwc.t),
                                            ptr(col.t), ptr(ws), need + 4 * WS_EXCESS, st), "selfocc_camera_se_flatten_bwd")
    torch.cuda.synchronize()
    assert all(t.guards_intact() for t in [out, dwc, col] + dxs), "a guard block was written"
    assert bool((ws[need // 4:] == SENTINEL).all()), "the workspace was written past what the entry asked for"
    assert not bool(torch.isnan(ws[:need // 4]).any()), "a chunk partial was not written"
    for l in range(L):
        if l not in asked:
            assert dxs[l].untouched(), f"dfeat[{l}] was not asked for and was written"
    return dict(out=out.t.cpu(), dx=[dxs[l].t.cpu() if l in asked else None for l in range(L)], dWc=dwc.t.cpu(), colsum=col.t.cpu())


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_raw_entries_vs_float64(hip, c, family):
    inp, ref, A, yard = sc.problem(c, family)
    assert hip.selfocc_camera_se_supported(c.B, c.N, c.C, c.M, len(inp['maps'])) == 1
    got = launch(hip, _device(inp))
    for k in sc.RAW:
        assert not bool(torch.isnan(torch.from_numpy(sc.flat(got[k]))).any()), (k, 'NaN left: an element was not written')
    e, b = sc.figures(got, ref, A, sc.RAW), sc.bounds(yard, sc.RAW)
    bits = {k: sc.bits_differing(got[k], ref[k]) for k in sc.RAW}
    for k in sc.RAW:
        _append(dict(test='raw', case=sc.case_id(c), family=family, tensor=k, kernel=e[k], yardstick=yard[k], K=sc.K[k], bound=b[k],
                     kernel_over_bound=e[k] / b[k], bits_differing_from_float64=bits[k]))
    if family == 'exact':
        assert all(torch.equal(a, r.float()) for a, r in zip(got['dx'], ref['dx'])), bits
        assert all(torch.equal(got[k], ref[k].float()) for k in ('out', 'dWc', 'colsum')), bits
    for k in sc.RAW:
        assert e[k] <= b[k], (k, e[k], b[k], yard[k])


@pytest.mark.parametrize("wanted", [None, (0, 2, 4, 6), (7,)], ids=['null', 'even', 'last'])
def test_dfeat_subsets_keep_the_bits_of_the_full_launch(hip, wanted):
    c = sc.Case(64, 128, 2, 3, 'EDGE8')
    d = _device(sc.problem(c, 'random')[0])
    full, part = launch(hip, d), launch(hip, d, wanted)
    for l in range(8):
        if l in (wanted or ()):
            assert torch.equal(part['dx'][l], full['dx'][l]), l
        else:
            assert part['dx'][l] is None                       # launch() saw its buffer keep the fill
    assert torch.equal(part['dWc'], full['dWc']) and torch.equal(part['colsum'], full['colsum']) and torch.equal(part['out'], full['out'])


# ------------------------------------------------------------------------------------------------------------------------------
# the Python route
# ------------------------------------------------------------------------------------------------------------------------------
PY_TENSORS = ('out', 'dx') + sc.FOLDED


def _apply(d, maps=None, g=None):
    from selfocc_amd.model.encoder import camera_se
    C, M = d['w'].shape
    a = {k: d[k].clone().requires_grad_(True) for k in ('gate', 'w', 'bias', 'cams', 'lvls')}
    xs = [m.detach().requires_grad_(True) for m in (maps or d['maps'])]
    val = camera_se._CameraSeFlatten.apply(a['gate'], a['w'].reshape(C, M, 1, 1), a['bias'], a['cams'], a['lvls'], *xs)
    grads = torch.autograd.grad(val, list(a.values()) + xs, grad_outputs=d['g'] if g is None else g)
    r = dict(zip(('g_gate', 'g_w', 'g_bias', 'g_cam', 'g_lvl'), grads[:5]))
    r.update(out=val.detach(), dx=list(grads[5:]))
    return {k: [t.cpu() for t in v] if k == 'dx' else v.cpu() for k, v in r.items()}


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("c", [sc.Case(64, 128, 2, 3, 'EDGE8'), sc.Case(96, 96, 2, 3, 'CHUNK4')], ids=sc.case_id)
def test_python_route_with_a_given_gate(hip, c, family):
    inp, ref, A, yard = sc.problem(c, family)
    got = _apply(_device(inp))
    e, b = sc.figures(got, ref, A, PY_TENSORS), sc.bounds(yard, PY_TENSORS)
    for k in PY_TENSORS:
        _append(dict(test='python', case=sc.case_id(c), family=family, tensor=k, kernel=e[k], yardstick=yard[k], K=sc.K[k], bound=b[k],
                     kernel_over_bound=e[k] / b[k], bits_differing_from_float64=sc.bits_differing(got[k], ref[k])))
    if family == 'exact':
        for k in PY_TENSORS:
            assert sc.bits_differing(got[k], ref[k]) == 0, k
    for k in PY_TENSORS:
        assert e[k] <= b[k], (k, e[k], b[k], yard[k])


def _view_at(t, off):
    """a contiguous copy of t that starts `off` floats behind a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 8, device=D0)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def test_views_off_a_16_byte_boundary_give_the_bits_of_the_aligned_call(hip):
    c = sc.Case(32, 64, 2, 3, 'EDGE8')
    d = _device(sc.problem(c, 'random')[0])
    want = _apply(d)
    for off in (1, 2, 3):
        got = _apply(d, [_view_at(m, off) for m in d['maps']], _view_at(d['g'], off))
        for k in PY_TENSORS:
            assert sc.bits_differing(got[k], want[k]) == 0, (off, k)


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: by name, before anything is launched
# ------------------------------------------------------------------------------------------------------------------------------
class _Raw:
    """a small valid call (C = M = 32, B 1, N 2, levels of 5 and 8 pixels) in buffers large enough for every shape tried below, and
    the two entries with every argument replaceable"""
    ROOM = 1 << 17           # floats per buffer: dWc of (128, 256) at B N = 2 is 1 << 16

    def __init__(self, hip):
        from selfocc_amd._lib import current_stream
        self.hip, self.st = hip, current_stream(D0)
        self.ins = {k: torch.randn(self.ROOM, device=D0) for k in ('map0', 'map1', 'gate', 'w', 'bias', 'cams', 'lvls', 'g')}
        self.outs = {k: Guarded((self.ROOM,)) for k in ('out', 'd0', 'd1', 'dwc', 'colsum')}
        self.ws = Guarded((1 << 18,))

    def p(self, name, shift=()):
        t = self.ws.t if name == 'ws' else self.outs[name].t if name in self.outs else self.ins[name]
        return ctypes.c_void_p(t.data_ptr() + (4 if name in shift else 0))

    def call(self, which, C=32, M=32, hw=(5, 8), shift=(), ws_bytes=None):
        L = len(hw)
        q = lambda n: self.p(n, shift)
        feats = (ctypes.c_void_p * max(L, 1))(*[q('map%d' % (l & 1)) for l in range(L)])
        dfeats = (ctypes.c_void_p * max(L, 1))(*[q('d%d' % (l & 1)) for l in range(L)])
        hwa = (ctypes.c_int32 * max(L, 1))(*hw)
        if which == 'fwd':
            return self.hip.selfocc_camera_se_flatten_fwd(feats, hwa, L, 1, 2, C, M, q('gate'), q('w'), q('bias'), q('cams'), q('lvls'),
                                                          q('out'), self.st)
        if ws_bytes is None:
            ws_bytes = 4 * self.ws.n - 16
        return self.hip.selfocc_camera_se_flatten_bwd(q('g'), feats, hwa, L, 1, 2, C, M, q('gate'), q('w'), dfeats, q('dwc'), q('colsum'),
                                                      q('ws'), ws_bytes, self.st)

    def untouched(self):
        torch.cuda.synchronize()
        return all(t.untouched() for t in list(self.outs.values()) + [self.ws])


def _refused(r, rc, *words):
    msg = r.hip.selfocc_last_error().decode()
    assert rc < 0, ('accepted', words)
    for w in words:
        assert w in msg, (w, msg)
    assert r.untouched(), ('outputs written', msg)


def test_refusals_name_the_cause_and_write_nothing(hip):
    r = _Raw(hip)
    for name in ('map0', 'map1'):
        _refused(r, r.call('fwd', shift=(name,)), 'camera_se_flatten_fwd', 'map not 16-byte aligned')
        _refused(r, r.call('bwd', shift=(name,)), 'camera_se_flatten_bwd', 'map or gradient not 16-byte aligned')
    _refused(r, r.call('fwd', shift=('out',)), 'camera_se_flatten_fwd', 'out not 16-byte aligned')
    _refused(r, r.call('bwd', shift=('g',)), 'camera_se_flatten_bwd', 'g not 16-byte aligned')
    _refused(r, r.call('bwd', shift=('d1',)), 'camera_se_flatten_bwd', 'map or gradient not 16-byte aligned')
    _refused(r, r.call('bwd', shift=('ws',)), 'camera_se_flatten_bwd', 'workspace NULL, unaligned or too small')
    hwa = (ctypes.c_int32 * 2)(5, 8)
    need = int(hip.selfocc_camera_se_flatten_bwd_workspace(hwa, 2, 1, 2, 32, 32))
    assert need == 4 * 2 * 2 * (32 * 32 + 32)
    _refused(r, r.call('bwd', ws_bytes=need - 1), 'workspace NULL, unaligned or too small', f'({need - 1} bytes, need {need})')
    for C, M in ((48, 48), (32, 96), (64, 192), (128, 256)):                     # C = 48, M = 3 C (twice), (128, 256)
        assert hip.selfocc_camera_se_supported(1, 2, C, M, 2) == 0 and hip.selfocc_camera_se_flatten_bwd_workspace(hwa, 2, 1, 2, C, M) == 0
        for which in ('fwd', 'bwd'):
            _refused(r, r.call(which, C=C, M=M), 'unsupported shape', f'C {C}, M {M}')
    for hw in ((), (1,) * 9):
        assert hip.selfocc_camera_se_supported(1, 2, 32, 32, len(hw)) == 0
        for which in ('fwd', 'bwd'):
            _refused(r, r.call(which, hw=hw), 'unsupported shape', f'{len(hw)} levels')
    for which in ('fwd', 'bwd'):
        _refused(r, r.call(which, hw=(5, 0)), 'level 1', 'no pixels')
    assert hip.selfocc_camera_se_flatten_bwd_workspace((ctypes.c_int32 * 2)(5, 0), 2, 1, 2, 32, 32) == 0
    # the same buffers, unshifted, the workspace exactly as large as asked for: accepted
    assert r.call('fwd') == 0 and r.call('bwd', ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert all(t.guards_intact() for t in r.outs.values()) and not r.untouched()
    assert not bool(torch.isnan(r.outs['out'].t[:2 * 13 * 32]).any()) and bool(torch.isnan(r.outs['out'].t[2 * 13 * 32:]).all())
    assert not bool(torch.isnan(r.ws.t[:need // 4]).any()) and bool(torch.isnan(r.ws.t[need // 4:]).all())
