"""GPU: selfocc_reproj_pick_fwd / _bwd against their definition, with equality on every ray (index and value).

The reference is ``wnorm`` as selfocc_reproj_fwd writes it when the OTHER frame's transform is the invalid matrix
(loss/reproj.py: _invalid_on — how the mono loss calls that kernel), downloaded and put through the sequential rule
    j = 0, best = wn_0;  for i = 1 .. S-1: if (wn_i > best) { best = wn_i; j = i; }
on the host.  S covers every kernel instance (M = 1, 2, 4, 8 samples per lane), S that is no multiple of 64 and a last lane
that is partly dead; R = 200 leaves no partial block but 50 blocks of 4 waves.  Each case holds: rays whose pixel lies far
outside or that carry no weight (every sample masked in both frames: the pick is 0), rays only the previous frame loses, rows with two exactly equal
maxima (the smaller index wins), and with ``deltas`` samples with delta < eps (weight zeroed), some of them on the row's
largest weight."""
import numpy as np
import pytest
import torch

from selfocc_amd import abi
from selfocc_amd._lib import check, current_stream, lib, ptr
from selfocc_amd.reproj import ReprojPickFunction, reproj_pick

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
HI, WI, R = 96.0, 200.0, 200
INVALID = torch.diag(torch.tensor([1.0, 1.0, -1.0, 1.0]))


def make_case(S, with_deltas, seed):
    g = torch.Generator().manual_seed(seed)
    f = 0.8 * WI
    K = np.array([[f, 0, WI / 2, 0], [0, f, HI / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])

    def motion(yaw_deg, tx, tz):
        y = np.deg2rad(yaw_deg)
        Rm = np.array([[np.cos(y), 0, np.sin(y), tx], [0, 1, 0, 0.02], [-np.sin(y), 0, np.cos(y), tz], [0, 0, 0, 1]])
        return torch.tensor(K @ Rm @ np.linalg.inv(K), dtype=torch.float32)
    # the previous frame is turned far enough that a band of rays leaves it at every depth
    T_prev, T_next = motion(12.0, 0.3, -0.6), motion(-2.5, -0.2, 0.7)
    pix = torch.stack([torch.rand(R, generator=g) * WI, torch.rand(R, generator=g) * HI], -1)
    pix[20:50, 0] = -WI * (1.0 + torch.rand(30, generator=g))            # far outside: most of them leave both frames
    near = torch.rand(R, 1, generator=g) * 0.5
    far = 2.0 + torch.rand(R, 1, generator=g) * 40.0
    edges = near + (far - near) * torch.linspace(0, 1, S + 1)[None]
    ts = ((edges[:, :-1] + edges[:, 1:]) / 2).contiguous()
    weights = torch.softmax(torch.randn(R, S, generator=g) * 3, -1) * torch.rand(R, 1, generator=g)
    weights[100:105] = 0.0                                               # rays with no weight at all
    deltas = (edges[:, 1:] - edges[:, :-1]).contiguous() if with_deltas else None
    # rows with two exactly equal maxima: the same weight (and the same delta) at two samples, twice the row's largest
    a = torch.randint(0, S, (R,), generator=g)
    b = torch.randint(0, S, (R,), generator=g)
    tie = torch.arange(R)[(torch.arange(R) % 3 == 0) & (a != b)]
    top = 2.0 * weights.amax(1)
    weights[tie, a[tie]] = top[tie]
    weights[tie, b[tie]] = top[tie]
    if with_deltas:
        deltas[tie, b[tie]] = deltas[tie, a[tie]]
        dead = torch.rand(R, S, generator=g) < 0.05
        dead[tie] = False
        deltas[dead] = 0.0                                               # delta < eps: the sample's weight is zeroed
        rows = torch.arange(R)[torch.arange(R) % 7 == 1]
        deltas[rows, weights[rows].argmax(1)] = 1e-9                     # ... on the row's largest weight as well
    values = 0.3 * torch.randn(R, S, generator=g)
    return dict(weights=weights, ts=ts, deltas=deltas, pix=pix, T_prev=T_prev, T_next=T_next, values=values)


def wnorm_of(c, frame):
    """(R, S) normalised weights of one frame from selfocc_reproj_fwd, the other frame invalid; no image matters to them"""
    dev = {k: (None if v is None else v.to(D0).contiguous()) for k, v in c.items()}
    S = c['weights'].shape[1]
    img = torch.zeros(3, 2, 2, device=D0)
    rgb = torch.zeros(R, 3, device=D0)
    inv = INVALID.to(D0)
    Ts = (dev['T_prev'], inv) if frame == 0 else (inv, dev['T_next'])
    a = abi.SoReprojArgs()
    a.weights, a.ts, a.deltas = ptr(dev['weights']), ptr(dev['ts']), ptr(dev['deltas'])
    a.pix, a.curr_rgb = ptr(dev['pix']), ptr(rgb)
    a.T_prev, a.T_next = ptr(Ts[0]), ptr(Ts[1])
    a.img_prev, a.img_next = ptr(img), ptr(img)
    a.R, a.S, a.Hi, a.Wi, a.img_h, a.img_w = R, S, 2, 2, HI, WI
    wn = torch.full((R, S), float('nan'), device=D0)
    a.wnorm = ptr(wn)
    check(lib().selfocc_reproj_fwd(a, current_stream(D0)), "selfocc_reproj_fwd")
    torch.cuda.synchronize()
    return wn.cpu().numpy()


def sequential_pick(wn):
    j = np.zeros(wn.shape[0], dtype=np.int64)
    best = wn[:, 0].copy()
    for i in range(1, wn.shape[1]):
        upd = wn[:, i] > best
        best = np.where(upd, wn[:, i], best)
        j = np.where(upd, i, j)
    return j


CASES = [(S, d) for S in (12, 64, 100, 256, 300, 512) for d in (False, True)]
_REF = {}


def reference(S, with_deltas):
    """(case, wnorm of both frames, their sequential picks), computed once per case and left unchanged"""
    key = (S, with_deltas)
    if key not in _REF:
        c = make_case(S, with_deltas, seed=100 + S)
        wn = [wnorm_of(c, f) for f in (0, 1)]
        assert all(np.isfinite(w).all() for w in wn)
        _REF[key] = (c, wn, np.stack([sequential_pick(w) for w in wn], 1))
    return _REF[key]


def run_pick(c, requires_grad=False):
    dev = {k: (None if v is None else v.to(D0)) for k, v in c.items()}
    if requires_grad:
        dev['values'].requires_grad_(True)
    val, idx = reproj_pick(dev['values'], dev['weights'], dev['ts'], dev['deltas'], dev['pix'], dev['T_prev'], dev['T_next'],
                           HI, WI)
    return val, idx, dev['values']


@pytest.mark.parametrize("S,with_deltas", CASES)
def test_pick_equals_the_sequential_rule_on_wnorm(hip, S, with_deltas):
    c, wn, j = reference(S, with_deltas)
    val, idx, _ = run_pick(c)
    assert idx.dtype == torch.int32 and idx.shape == (R, 2) and val.shape == (R, 2)
    got = idx.cpu().numpy()
    assert np.array_equal(got, j), np.argwhere(got != j)[:8]
    want = torch.gather(c['values'], 1, torch.tensor(j))
    assert torch.equal(val.cpu(), want)
    # the case holds what it is meant to hold
    for f in (0, 1):
        top = wn[f].max(1)
        masked = top == 0
        assert (j[masked, f] == 0).all()
        dup = ((wn[f] == top[:, None]).sum(1) >= 2) & (top > 0)
        assert dup.sum() >= 10, (f, dup.sum())
        if S > 1:
            assert (j[:, f] > 0).sum() > R // 3
    lost_both = (wn[0].max(1) == 0) & (wn[1].max(1) == 0)
    assert lost_both[100:105].all() and lost_both[20:50].sum() >= 10, lost_both.sum()
    only_prev_lost = (wn[0].max(1) == 0) & (wn[1].max(1) > 0)
    assert only_prev_lost.sum() >= 5, only_prev_lost.sum()
    if with_deltas:
        zeroed = (c['deltas'].numpy() < np.finfo(np.float32).eps) & (c['weights'].numpy() > 0)
        assert zeroed.sum() >= 50 and (wn[0][zeroed] == 0).all() and (wn[1][zeroed] == 0).all()
    if S >= 100:
        assert (j >= 64 * ((S - 1) // 64)).any()            # a pick in the last, partly dead stretch of lanes


@pytest.mark.parametrize("S,with_deltas", [(12, False), (100, True), (300, False), (512, True)])
def test_pick_backward_is_the_dense_index_put(hip, S, with_deltas):
    c, wn, j = reference(S, with_deltas)
    val, idx, values = run_pick(c, requires_grad=True)
    g = torch.randn(R, 2, generator=torch.Generator().manual_seed(S))
    grad, = torch.autograd.grad(val, values, g.to(D0))
    rows = torch.arange(R)[:, None].expand(-1, 2)
    want = torch.zeros(R, S).index_put((rows, torch.tensor(j)), g, accumulate=True)
    assert grad.shape == (R, S) and torch.equal(grad.cpu(), want)
    same = j[:, 0] == j[:, 1]
    live_same = same & (wn[0].max(1) > 0) & (wn[1].max(1) > 0)
    assert live_same.sum() >= 10                                # both frames picked one sample: the two upstream values summed
    assert (want != 0).sum() == 2 * R - same.sum()
    # differentiable in `values` only
    dev = {k: (None if v is None else v.to(D0)) for k, v in c.items()}
    w = dev['weights'].requires_grad_(True)
    v2, _ = ReprojPickFunction.apply(dev['values'].requires_grad_(True), w, dev['ts'], dev['deltas'], dev['pix'], dev['T_prev'],
                                     dev['T_next'], HI, WI)
    assert torch.autograd.grad(v2.sum(), w, allow_unused=True)[0] is None


def test_pick_refuses_bad_shapes_by_name(hip):
    c = make_case(12, False, seed=1)
    dev = {k: (None if v is None else v.to(D0)) for k, v in c.items()}
    with pytest.raises(ValueError, match="shape of weights"):
        reproj_pick(dev['values'][:, :5], dev['weights'], dev['ts'], None, dev['pix'], dev['T_prev'], dev['T_next'], HI, WI)
    big = torch.zeros(4, 513, device=D0)
    from selfocc_amd._lib import SelfOccHipError
    with pytest.raises(SelfOccHipError, match="1 <= S <= 512"):
        reproj_pick(big, big, big + 1, None, dev['pix'][:4], dev['T_prev'], dev['T_next'], HI, WI)
    val, idx = reproj_pick(dev['values'][:0], dev['weights'][:0], dev['ts'][:0], None, dev['pix'][:0], dev['T_prev'],
                           dev['T_next'], HI, WI)
    assert val.shape == (0, 2) and idx.shape == (0, 2)
