"""Shared by tests/test_msda_cases_cpu.py and tests/test_msda_sharp_gpu.py: the case table that reaches every instantiation of the
MSDA kernels (csrc/msda.hip: plain forward (D, log2 G); fused and camera-loop forward and backward point kernels (D, log2 G, value
type); the three plain backward kernels per D; the band kernel across band seams), the float64 reference of a case with the mask
of its non-comparable location gradients, the metrics and the bounds.

Which kernel a case reaches is NOT worked out here: selfocc_msda_plan (a host-only entry of the library) says which group size,
which branches of the camera-loop backward and which band decomposition a call gets; the CPU test compares what it reports for
the table with the full dispatch tables.

Reference.  oracle.torch_port.msda_port (the reference's F.grid_sample formulation) in float64 on the float32 inputs widened, the
prologue composed in float64 (loc = ref + off / (W_l, H_l), softmax over L * P, the mean over the visible cameras with
max(count, 1)), gradients by float64 autograd.  bfloat16 storage: `value` rounded to bfloat16 and widened.

Mask.  The bilinear value is continuous across pixel boundaries: out, g_value and g_logits / g_attw need none.  The derivative
with respect to the location is constant per cell: an element of g_off / g_loc is left out when its point (for the camera loop:
its point under any camera that sees the query) lies within MARGIN pixels of an integer value of loc * W - 0.5 or loc * H - 0.5, on
either axis, as decided from the float64 reference alone.  MARGIN = 1e-4 pixel: the maps here are at most 100 pixels wide (float32
ulp of a coordinate <= 7.6e-6, a few roundings in ref + off / W and * W - 0.5).  No case may leave out more than 1 % of its points.

Bounds.  Not taken from the kernels: per family and metric, five times (and a tenth) the largest error of the float32 evaluation of
the same port over the family's cases (the yardstick), rounded up to one significant digit; see BOUNDS.
"""
import collections
import ctypes as C
import math

import torch

from oracle import torch_port as tp
from selfocc_amd import abi

MARGIN = 1e-4
MAPS = ((6, 10), (3, 5), (5, 4), (2, 3))
SEAM_MAPS = {4: ((64, 100),), 8: ((30, 40),), 16: ((24, 50),), 32: ((30, 40),)}
K_BAND_SEG = 4096                       # kBandSeg of csrc/msda.hip: list entries per band-kernel block

Case = collections.namedtuple(
    'Case', 'sweep form d L P bf16 n nq maps ref_kind head_major merged sink vstride mode',
    defaults=(False, 2, 70, None, 1, False, False, False, False, ''))

# (D, log2 G, bfloat16) of so_with_msda_shape and (D, log2 G) of so_with_msda_plain_shape (csrc/msda.hip), restated: the CPU test
# holds what selfocc_msda_plan reports for the table against these
FUSED_TABLE = [(8, lg, False) for lg in range(1, 7)] + [(16, lg, bf) for bf in (False, True) for lg in range(2, 7)] + \
    [(32, lg, False) for lg in range(3, 7)]
PLAIN_TABLE = [(d, lg) for d in (4, 8, 16, 32) for lg in range(max(0, int(math.log2(d // 4))), 7)]

# (L, P) that the group choice of the library maps to (D, log2 G): found by asking selfocc_msda_plan for every L * P, and checked
# against it by the CPU test.  Every entry but plain (4, 0) (one lane per group: nothing is ragged) takes at least two rounds per
# lane with a ragged last round, the place where the shared softmax and corner-dot ladder can go wrong.
FUSED_LP = {
    (8, 1): (3, 3), (8, 2): (2, 9), (8, 3): (3, 7), (8, 4): (2, 21), (8, 5): (2, 35), (8, 6): (2, 65),
    (16, 2): (2, 5), (16, 3): (2, 11), (16, 4): (3, 15), (16, 5): (3, 22), (16, 6): (2, 65),
    (32, 3): (2, 18), (32, 4): (3, 15), (32, 5): (2, 35), (32, 6): (3, 43),
}
CROSS_LP = dict(FUSED_LP)
CROSS_LP.update({(8, 1): (1, 5), (8, 2): (3, 9), (16, 2): (3, 3), (16, 4): (2, 23), (32, 4): (2, 21), (32, 5): (3, 22)})
PLAIN_LP = {
    (4, 0): (3, 1), (4, 1): (3, 3), (4, 2): (2, 9), (4, 3): (3, 7), (4, 4): (3, 15), (4, 5): (3, 27), (4, 6): (3, 38),
    (8, 1): (3, 3), (8, 2): (1, 11), (8, 3): (3, 7), (8, 4): (1, 47), (8, 5): (3, 31), (8, 6): (2, 61),
    (16, 2): (3, 3), (16, 3): (2, 11), (16, 4): (3, 15), (16, 5): (3, 29), (16, 6): (2, 59),
    (32, 3): (1, 23), (32, 4): (3, 15), (32, 5): (3, 28), (32, 6): (2, 63),
}


def _cases():
    out = []
    i = 0
    for form, table in (('fused', FUSED_LP), ('cross', CROSS_LP)):
        for d, lg, bf in FUSED_TABLE:
            L, P = table[(d, lg)]
            hm = i % 2 == 1
            out.append(Case('shape', form, d, L, P, bf, n=2 if (form == 'fused' or i % 4) else 1, maps=MAPS[:L],
                            ref_kind=i % 3 if form == 'fused' else 1, head_major=hm, merged=(i // 2) % 2 == 1,
                            sink=hm and not bf and (i // 4) % 2 == 0,
                            vstride=form == 'cross' and not hm and not bf and (i // 2) % 2 == 0))
            i += 1
    # the LDS histogram of the camera-loop point kernel against the separate counting pass, at one group size (G = 8)
    out.append(Case('count', 'cross', 16, 2, 11, nq=20, maps=MAPS[:2]))
    out.append(Case('count', 'cross', 16, 2, 11, nq=150, maps=MAPS[:2], head_major=True, merged=True))
    for d, lg in PLAIN_TABLE:
        L, P = PLAIN_LP[(d, lg)]
        for mode in ('banded', 'atomic'):
            out.append(Case('shape', 'plain', d, L, P, maps=MAPS[:L], mode=mode))
    # band seams: a level cut into several bands, enough points that one band's list passes a list segment
    for d in (4, 8, 16, 32):
        for mode in ('banded', 'atomic'):
            out.append(Case('seam', 'plain', d, 1, 12, nq=4000, maps=SEAM_MAPS[d], mode=mode))
    for k, d in enumerate((8, 16, 32)):
        out.append(Case('seam', 'fused', d, 1, 12, nq=4000, maps=SEAM_MAPS[d], ref_kind=k, head_major=k == 1, sink=k == 1,
                        merged=k == 2))
    return out


CASES = _cases()


def ref_id(c):
    return f"{c.sweep}-{c.form}-d{c.d}{'bf16' if c.bf16 else ''}-L{c.L}P{c.P}-n{c.n}q{c.nq}" + (f"-k{c.ref_kind}" if c.form == 'fused' else '')


def case_id(c):
    route = ''.join(s for s, on in (('-hm', c.head_major), ('-merged', c.merged), ('-sink', c.sink), ('-vstride', c.vstride)) if on)
    return ref_id(c) + route + (f"-{c.mode}" if c.mode else '')


def ref_key(c):
    """what the inputs and the reference of a case depend on: everything but the route"""
    return c._replace(head_major=False, merged=False, sink=False, vstride=False, mode='')


REF_CASES = list(dict.fromkeys(ref_key(c) for c in CASES))

METRICS = ('out_max', 'out_l2', 'gv_max', 'gv_l2', 'gp_max', 'gp_l2', 'gw_max', 'gw_l2')   # gp: g_off / g_loc, gw: g_logits / g_attw

# Per family (form, sweep) and metric: (bound, yardstick).  The yardstick is the largest figure of the float32 port over the family's
# cases (tests/test_msda_cases_cpu.py::test_yardstick prints every case's); the bound is 5 x that and a tenth more (the float32 port
# sums in an order that may differ from one CPU to the next, and its largest error with it), rounded up to one significant digit.
# The seam cases are a family of their own: their maps are 40 to 100 pixels wide instead of 3 to 10, and the float32 rounding of a
# location (6e-8 of a coordinate in [-1, 1]) is that many times larger in pixels, i.e. in bilinear weight.
BOUNDS = {
    ('fused', 'shape'): dict(out_max=(5e-06, 8.37e-07), out_l2=(3e-06, 3.96e-07), gv_max=(5e-06, 7.60e-07), gv_l2=(3e-06, 5.05e-07),
                             gp_max=(4e-06, 6.00e-07), gp_l2=(2e-06, 3.46e-07), gw_max=(6e-06, 1.05e-06), gw_l2=(3e-06, 4.40e-07)),
    ('cross', 'shape'): dict(out_max=(6e-06, 1.02e-06), out_l2=(3e-06, 4.89e-07), gv_max=(5e-06, 8.48e-07), gv_l2=(3e-06, 5.01e-07),
                             gp_max=(4e-06, 7.18e-07), gp_l2=(3e-06, 4.32e-07), gw_max=(8e-06, 1.38e-06), gw_l2=(3e-06, 5.30e-07)),
    ('plain', 'shape'): dict(out_max=(4e-06, 6.06e-07), out_l2=(2e-06, 3.24e-07), gv_max=(5e-06, 7.31e-07), gv_l2=(3e-06, 3.98e-07),
                             gp_max=(4e-06, 6.35e-07), gp_l2=(2e-06, 2.39e-07), gw_max=(4e-06, 6.81e-07), gw_l2=(2e-06, 3.34e-07)),
    ('plain', 'seam'): dict(out_max=(3e-05, 3.91e-06), out_l2=(2e-05, 2.70e-06), gv_max=(2e-05, 3.31e-06), gv_l2=(2e-05, 2.72e-06),
                            gp_max=(2e-05, 2.76e-06), gp_l2=(9e-06, 1.52e-06), gw_max=(3e-05, 3.78e-06), gw_l2=(2e-05, 2.72e-06)),
    ('fused', 'seam'): dict(out_max=(3e-05, 3.94e-06), out_l2=(2e-05, 1.96e-06), gv_max=(2e-05, 2.38e-06), gv_l2=(2e-05, 1.98e-06),
                            gp_max=(3e-05, 3.89e-06), gp_l2=(8e-06, 1.36e-06), gw_max=(2e-05, 3.53e-06), gw_l2=(2e-05, 1.97e-06)),
}


def family(case):
    return case.form, 'seam' if case.sweep == 'seam' else 'shape'


# (case id, metric) -> (figure, reason): a correct kernel that needs more than a bound because it sums in another order than the
# float32 port the bound comes from.  The figure replaces the bound for that pair; it still has to meet the negative controls.
EXCEPTIONS = {}


def bounds(case):
    b = {k: v[0] for k, v in BOUNDS[family(case)].items()}
    for (cid, k), (fig, _why) in EXCEPTIONS.items():
        if cid == case_id(case):
            b[k] = fig
    return b


# ------------------------------------------------------------------------------------------------------------------------------
# what the library decides for a case
# ------------------------------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple('Plan', 'rc error log2_group banded count_here bin_vis bands rows')
FORMS = {'plain': abi.MSDA_PLAIN, 'fused': abi.MSDA_FUSED, 'cross': abi.MSDA_CROSS}


def plan_of(form, n, nq, heads, d, L, P, maps, bf16=False):
    from selfocc_amd._lib import lib
    a = abi.SoMsdaArgs(FORMS[form], n, sum(h * w for h, w in maps), nq, heads, d, L, P)
    a.value_dtype = abi.DTYPE_BF16 if bf16 else abi.DTYPE_F32
    host = (C.c_int32 * (2 * len(maps)))(*[v for hw in maps for v in hw])
    a.host_shapes = C.addressof(host)
    out = (C.c_int32 * abi.MSDA_PLAN_INTS)()
    rc = lib().selfocc_msda_plan(a, out)
    nl = min(L, 8)
    return Plan(rc, lib().selfocc_last_error() if rc else b'', out[abi.MSDA_PLAN_LOG2_GROUP], out[abi.MSDA_PLAN_BANDED],
                out[abi.MSDA_PLAN_COUNT_HERE], out[abi.MSDA_PLAN_BIN_VIS], list(out[abi.MSDA_PLAN_BANDS:abi.MSDA_PLAN_BANDS + nl]),
                list(out[abi.MSDA_PLAN_ROWS:abi.MSDA_PLAN_ROWS + nl]))


def plan(case):
    return plan_of(case.form, case.n, case.nq, HEADS, case.d, case.L, case.P, case.maps, case.bf16)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs of a case
# ------------------------------------------------------------------------------------------------------------------------------
HEADS = 2
Inputs = collections.namedtuple('Inputs', 'case shapes starts nv value off logits ref vis gout loc attw')


def make_inputs(case):
    c = ref_key(case)
    g = torch.Generator().manual_seed(2000 + REF_CASES.index(c))
    n, nq, H, L, P, d = c.n, c.nq, HEADS, c.L, c.P, c.d
    shapes = torch.tensor(c.maps)
    hw = shapes[:, 0] * shapes[:, 1]
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), hw.cumsum(0)[:-1]])
    nv = int(hw.sum())
    cross = c.form == 'cross'
    rows = (nq,) if cross else (n, nq)
    value = torch.randn(n, nv, H, d, generator=g)
    off = 1.5 * torch.randn(*rows, H, L, P, 2, generator=g)
    logits = 2 * torch.randn(*rows, H, L * P, generator=g)
    kind = 1 if cross else c.ref_kind
    ref = 1.3 * torch.rand(n, nq, *{0: (L, 2), 1: (P, 2), 2: (L, P, 2)}[kind], generator=g) - 0.15
    gout = torch.randn(*rows, H * d, generator=g)
    vis = None
    if cross:        # queries seen by no camera (0), by all (1), by one (2, with two cameras)
        vis = torch.rand(n, nq, generator=g) < 0.6
        vis[:, 0], vis[:, 1] = False, True
        vis[:, 2] = False
        vis[0, 2] = n > 1
    loc = attw = None
    if c.form == 'plain':     # the plain op's inputs are the float32 locations and weights themselves
        loc = (_expand_ref(ref, kind) + off / _norm(shapes, torch.float32)).contiguous()
        attw = logits.softmax(-1).view(n, nq, H, L, P).contiguous()
    return Inputs(c, shapes, starts, nv, value, off, logits, ref, vis, gout, loc, attw)


def _norm(shapes, dtype):
    return torch.stack([shapes[:, 1], shapes[:, 0]], -1).to(dtype)[:, None, :]          # (L, 1, 2): (W_l, H_l)


def _expand_ref(ref, kind):
    """-> broadcastable to (n, nq, heads, L, P, 2)"""
    return {0: lambda r: r[:, :, None, :, None, :], 1: lambda r: r[:, :, None, None, :, :], 2: lambda r: r[:, :, None, :, :, :]}[kind](ref)


# ------------------------------------------------------------------------------------------------------------------------------
# the port of a case in a working dtype
# ------------------------------------------------------------------------------------------------------------------------------
def _corner_geometry(inp, loc):
    """per point: pixel coordinates (x, y) = loc * (W, H) - 0.5 of its level, floor, and the level's (H, W, start)"""
    sh = inp.shapes.to(loc.dtype)
    W, Hh = sh[:, 1][:, None], sh[:, 0][:, None]                                           # (L, 1) against (..., L, P)
    return loc[..., 0] * W - 0.5, loc[..., 1] * Hh - 0.5


def corner_sum(inp, value, loc, aw, cmask):
    """sum over the points of aw * (bilinear weight * value) of the corners `cmask` (..., L, P, 4) selects, corners in the order
    (y0, x0), (y0, x1), (y1, x0), (y1, x1): the part of the op's output that comes through those corners.  -> (B, nq, heads * d)"""
    B, nq, H, L, P, _ = loc.shape
    x, y = _corner_geometry(inp, loc)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    Wl = inp.shapes[:, 1][:, None].expand(L, P)
    Hl = inp.shapes[:, 0][:, None].expand(L, P)
    st = inp.starts[:, None].expand(L, P)
    out = 0
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xx, yy = x0.long() + dx, y0.long() + dy
        ok = (xx >= 0) & (xx < Wl) & (yy >= 0) & (yy < Hl) & cmask[..., k]
        w = (fx if dx else 1 - fx) * (fy if dy else 1 - fy) * aw * ok.to(aw.dtype)
        idx = (st + yy.clamp(min=0) * Wl + xx.clamp(min=0)).clamp(max=inp.nv - 1) * ok.long()      # (B, nq, H, L, P)
        v = value.permute(0, 2, 1, 3)                                                             # (B, H, nv, d)
        gi = idx.permute(0, 2, 1, 3, 4).reshape(B, H, -1, 1).expand(-1, -1, -1, value.shape[-1])
        got = torch.gather(v, 2, gi).view(B, H, nq, L * P, -1)
        out = out + (got * w.permute(0, 2, 1, 3, 4).reshape(B, H, nq, L * P, 1)).sum(3)
    return out.permute(0, 2, 1, 3).reshape(B, nq, -1)


Port = collections.namedtuple('Port', 'out gv gp gw loc aw')


def port(inp, dtype=torch.float64, defect=None, rows=None):
    """forward and the gradients of (out * gout).sum() in `dtype`.  -> Port(out, g_value, g_off | g_loc, g_logits | g_attw, loc, aw)
    with loc (B, nq, heads, L, P, 2) and aw (B, nq, heads, L, P) as sampled (camera loop: B = cameras).
    defect: None, or one of the negative controls 'level' (the weights of level 0 x 1.001), 'corner' (the heaviest in-map corner of
    the heaviest point of every (query, head) group missing), 'normaliser' (the last of the L * P points left out of the softmax
    sum), 'count' (the camera count one too high for queries seen by every camera), 'seam' (g_value: the contributions that points
    of the band above bring to the first row of every band but the first lost; `rows`: rows per band of every level)."""
    c = inp.case
    n, nq, H, L, P = c.n, c.nq, HEADS, c.L, c.P
    cross, plain = c.form == 'cross', c.form == 'plain'
    seen = inp.value.to(torch.bfloat16).float() if c.bf16 else inp.value
    value = seen.to(dtype).requires_grad_(True)
    gout = inp.gout.to(dtype)
    if plain:
        loc, aw = inp.loc.to(dtype).requires_grad_(True), inp.attw.to(dtype).requires_grad_(True)
        leaves = (value, loc, aw)
    else:
        off, lg = inp.off.to(dtype).requires_grad_(True), inp.logits.to(dtype).requires_grad_(True)
        leaves = (value, off, lg)
        o, l_ = (off[None], lg[None]) if cross else (off, lg)
        loc = _expand_ref(inp.ref.to(dtype), 1 if cross else c.ref_kind) + o / _norm(inp.shapes, dtype)
        loc = loc.expand(n, nq, H, L, P, 2)
        if defect == 'normaliser':
            e = torch.exp(l_ - l_.amax(-1, keepdim=True))
            aw = e / e[..., :-1].sum(-1, keepdim=True)
        else:
            aw = l_.softmax(-1)
        aw = aw.view(-1, nq, H, L, P).expand(n, nq, H, L, P)
    aw_used = aw
    if defect == 'level':
        aw_used = torch.cat([aw[:, :, :, :1] * 1.001, aw[:, :, :, 1:]], 3)
    out = tp.msda_port(value, inp.shapes, loc, aw_used)
    if defect == 'corner':
        with torch.no_grad():
            x, y = _corner_geometry(inp, loc)
            fx, fy = x - torch.floor(x), y - torch.floor(y)
            Wl, Hl = inp.shapes[:, 1][:, None], inp.shapes[:, 0][:, None]
            w4 = []
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                xx, yy = torch.floor(x) + dx, torch.floor(y) + dy
                ok = (xx >= 0) & (xx < Wl) & (yy >= 0) & (yy < Hl)
                w4.append((fx if dx else 1 - fx) * (fy if dy else 1 - fy) * aw * ok)
            w4 = torch.stack(w4, -1).reshape(n, nq, H, L * P * 4)
            cmask = torch.zeros_like(w4, dtype=torch.bool).scatter_(-1, w4.argmax(-1, keepdim=True), True)
            cmask = cmask.view(n, nq, H, L, P, 4)
        out = out - corner_sum(inp, value, loc, aw_used, cmask)
    if cross:
        cnt = inp.vis.sum(0)
        den = cnt.clamp(min=1)
        if defect == 'count':
            den = den + (cnt == n).long()
        out = (out * inp.vis[:, :, None].to(dtype)).sum(0) / den[:, None].to(dtype)
    g = torch.autograd.grad((out * gout).sum(), leaves, retain_graph=defect == 'seam')
    gv = g[0]
    if defect == 'seam':
        with torch.no_grad():
            _, y = _corner_geometry(inp, loc)
            nxt = torch.floor(y).long() + 1                                                       # the row of the two lower corners
            r = torch.tensor(rows)[:, None]
            lower = (nxt % r == 0) & (nxt > 0)
            cmask = torch.stack([torch.zeros_like(lower), torch.zeros_like(lower), lower, lower], -1)
        lost = corner_sum(inp, value, loc, aw_used, cmask)
        gv = gv - torch.autograd.grad((lost * gout).sum(), value)[0]
    return Port(out.detach().double(), gv.double(), g[1].double(), g[2].double(), loc.detach(), aw.detach())


def keep_mask(inp, p):
    """elements of g_off / g_loc that are compared: (n, nq, heads, L, P, 2), camera loop (nq, heads, L, P, 2); from the float64 port"""
    x, y = _corner_geometry(inp, p.loc.double())
    near = lambda t: (t - torch.round(t)).abs() <= MARGIN
    bad = near(x) | near(y)
    if inp.case.form == 'cross':
        bad = (bad & inp.vis[:, :, None, None, None]).any(0)
    return (~bad)[..., None].expand(*bad.shape, 2)


def cells(inp, p):
    x, y = _corner_geometry(inp, p.loc)
    return torch.floor(x).long(), torch.floor(y).long()


Reference = collections.namedtuple('Reference', 'inp port keep')
_LAST = {}


def reference(case):
    """float64 reference of a case, shared by the cases that differ only in route: computed once, never modified.  Only the latest
    one is held: the tests run grouped by reference."""
    key = ref_key(case)
    if key not in _LAST:
        _LAST.clear()
        inp = make_inputs(case)
        p = port(inp)
        _LAST[key] = Reference(inp, p, keep_mask(inp, p))
    return _LAST[key]


# ------------------------------------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------------------------------------
def _pair(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / ref.abs().max()).item(), ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def metrics(r, out, gv, gp, gw):
    """got against the reference r, float64 on the CPU, in the reference's layouts"""
    m = {}
    for name, got, ref in (('out', out, r.port.out), ('gv', gv, r.port.gv), ('gp', gp.double()[r.keep], r.port.gp[r.keep]),
                           ('gw', gw, r.port.gw)):
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        m[name + '_max'], m[name + '_l2'] = _pair(got, ref)
    return m
