"""GPU: selfocc_dropout_add_fwd / selfocc_dropout_bwd (csrc/dropout.hip) against tests/dropout_model.py, element for element.

test_encoder_glue_gpu.py checks rates only; it cannot tell which elements must go.  Here the kept SET is the model's at every
index and a kept value is x * scale bit for bit, so a decision per float4 group, a seed or index cut to 32 bits or a mask that
ignores the seed fails at once (tests/test_dropout_model_cpu.py shows the model itself is a sound mask).  Sizes reach what no
other test runs: the launch is capped at 8192 blocks x 1024 elements = 8 388 608, so
  * 8 388 608            the cap exactly, one trip of the grid-stride loop, every block full;
  * 8 388 609 / ...611   a second trip whose only work is the scalar tail (1 and 3 elements) in block 0;
  * 2 * 8 388 608 + 6    a third trip: a float4 group and a 2-element tail, on different threads;
  * 1 .. 7, 1023 .. 1025 the tail with and without a vector group before it, one block and two.
Then the autograd route (the drawn seed is read from y.grad_fn.seed) and operands that are contiguous views at element offsets
1, 2, 3 of a larger buffer: their data pointers are not 16-byte aligned, which the C entries refuse; dropout_add re-stages them."""
import functools

import numpy as np
import pytest
import torch

import dropout_model as dm

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")

CAP = 8192 * 1024
SMALL = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025]
LARGE = [CAP, CAP + 1, CAP + 3, 2 * CAP + 6]
N_MAX = max(LARGE)
SEEDS = [5, (1 << 32) + 5, (1 << 63) - 1, 123456789012345]       # the second equals the first in its low word
PS = [0.1, 0.5, 2.0 ** -24]                                     # 2^-24: only u == 0 is dropped
GUARD = 4
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def _u_max(seed):
    return dm.u_values(seed, N_MAX)


def _u(seed, n):
    return dm.u_values(seed, n) if n <= 4096 else _u_max(seed)[:n]         # the large sizes share one evaluation per seed


@functools.lru_cache(maxsize=None)
def _x():
    g = torch.Generator().manual_seed(11)
    return (torch.rand(N_MAX, generator=g) + 0.5).to(D0)          # [0.5, 1.5): no zeros, so kept <=> y != 0 under identity = 0


@functools.lru_cache(maxsize=None)
def _zeros():
    return torch.zeros(N_MAX, device=D0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run_direct(n, p, seed):
    """(y, gx) of the two C entries on x[:n] with identity = 0; the outputs sit in front of a guard that must stay untouched."""
    from selfocc_amd._lib import lib, check, ptr, current_stream
    x = _x()[:n]
    outs = []
    for which in ('fwd', 'bwd'):
        buf = torch.full((n + GUARD,), SENTINEL, device=D0)
        if which == 'fwd':
            check(lib().selfocc_dropout_add_fwd(ptr(x), ptr(_zeros()), ptr(buf), n, float(p), seed, current_stream(D0)), which)
        else:
            check(lib().selfocc_dropout_bwd(ptr(x), ptr(buf), n, float(p), seed, current_stream(D0)), which)
        assert torch.all(buf[n:] == SENTINEL), f"{which}: wrote past element n = {n}"
        outs.append(buf[:n])
    return outs


def _check_direct(n, p, seed, keep=None):
    keep = (_u(seed, n) >= np.float32(p)) if keep is None else keep
    y, gx = _run_direct(n, p, seed)
    k = torch.from_numpy(keep).to(D0)
    want = torch.where(k, _x()[:n] * torch.tensor(dm.scale(p), device=D0), _zeros()[:n])      # one float32 product
    what = f"n {n} p {p!r} seed {seed}"
    assert torch.equal(y != 0, k), f"{what}: kept set differs at {torch.nonzero((y != 0) != k)[:8].flatten().tolist()}"
    assert torch.equal(_bits(y), _bits(want)), f"{what}: kept values are not x * scale"
    assert torch.equal(_bits(gx), _bits(y)), f"{what}: backward mask or value differs from the forward's"
    return keep


def test_model_scale_is_the_launchers():
    assert dm.scale(0.5) == np.float32(2.0) and dm.scale(0.1) == np.float32(1.0) / np.float32(0.9)


@pytest.mark.parametrize("n", SMALL)
def test_direct_calls_equal_the_model_small(hip, n):
    for seed in SEEDS:
        for p in PS + [0.25, 0.9]:
            _check_direct(n, p, seed)


@pytest.mark.parametrize("seed", SEEDS[1:3])
@pytest.mark.parametrize("n", LARGE)
def test_direct_calls_equal_the_model_past_the_block_cap(hip, n, seed):
    for p in PS:
        _check_direct(n, p, seed)


@pytest.mark.parametrize("seed,i", [(0, 0), (38, 1101771), ((1 << 32) + 8, 3084966)])
def test_smallest_p_drops_exactly_the_elements_with_u_zero(hip, seed, i):
    """u[i] == 0 for these (seed, index) pairs (found by searching the model): p = 2^-24 drops them and nothing with u > 0,
    p = 0 keeps them (u >= 0)"""
    n = i + 2
    u = _u(seed, n)
    assert u[i] == 0 and (u == 0).sum() <= 2
    keep = _check_direct(n, 2.0 ** -24, seed)
    assert not keep[i] and keep.sum() == n - (u == 0).sum()
    assert _check_direct(n, 0.0, seed).all()


def test_seeds_equal_in_the_low_word_give_different_masks(hip):
    a, b = _run_direct(1025, 0.5, SEEDS[0])[0], _run_direct(1025, 0.5, SEEDS[1])[0]
    assert not torch.equal(a != 0, b != 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_threshold_is_greater_or_equal_in_float32(hip, seed):
    """p = u[i] keeps element i, the next float32 above drops it: the comparison is u >= p on exactly the model's u"""
    n = 1025
    u = _u(seed, n)
    i = int(np.nonzero((u > 0.05) & (u < 0.95))[0][0])
    for p, kept in ((u[i], True), (np.nextafter(u[i], np.float32(1.0)), False)):
        assert p.dtype == np.float32
        keep = _check_direct(n, float(p), seed)
        assert bool(keep[i]) is kept
        assert bool(_run_direct(n, float(p), seed)[0][i] != 0) is kept


# ---- the autograd route ------------------------------------------------------------------------------------------------

def _operands(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(*shape, generator=g) + 0.5).to(D0)
    idt = torch.randn(*shape, generator=g).to(D0)
    w = (torch.rand(*shape, generator=g) + 0.5).to(D0)
    return x, idt, w


@pytest.mark.parametrize("shape,p", [((3, 1001, 7), 0.5), ((1025,), 0.1), ((5,), 0.25)])
def test_autograd_route_uses_the_model_mask_of_its_drawn_seed(hip, shape, p):
    from selfocc_amd.dropout import dropout_add
    x, _, w = _operands(shape)
    x.requires_grad_(True)
    zero = torch.zeros(shape, device=D0)
    torch.manual_seed(77)
    y = dropout_add(x, zero, p, True)
    seed = y.grad_fn.seed
    assert isinstance(seed, int) and 0 <= seed < 1 << 63
    keep = torch.from_numpy(dm.keep(seed, x.numel(), p)).to(D0).view(shape)
    scale = torch.tensor(dm.scale(p), device=D0)
    assert torch.equal(y.detach() != 0, keep)
    assert torch.equal(_bits(y.detach()), _bits(torch.where(keep, x.detach() * scale, zero)))
    (y * w).sum().backward()
    assert torch.equal(x.grad != 0, keep)
    assert torch.equal(_bits(x.grad), _bits(torch.where(keep, w * scale, zero)))
    # the next call draws another seed; torch.manual_seed brings the first one back
    y2 = dropout_add(x, zero, p, True)
    assert y2.grad_fn.seed != seed
    torch.manual_seed(77)
    y3 = dropout_add(x, zero, p, True)
    assert y3.grad_fn.seed == seed and torch.equal(_bits(y3.detach()), _bits(y.detach()))


# ---- operands that are misaligned contiguous views ---------------------------------------------------------------------

N_VIEW = 1025


def _view(t, off):
    """`t` as a contiguous view at element offset `off` of a larger buffer: the data pointer is off 16-byte alignment"""
    buf = torch.full((t.numel() + 8,), SENTINEL, device=D0)
    v = buf[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    v = v.view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off and torch.equal(v, t)
    return v


@pytest.mark.parametrize("which", ["x", "identity", "both"])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_forward_accepts_misaligned_views(hip, off, which):
    from selfocc_amd.dropout import dropout_add
    x, idt, _ = _operands((N_VIEW,))
    xa, ia = x.clone().requires_grad_(True), idt.clone()
    assert xa.data_ptr() % 16 == 0 and ia.data_ptr() % 16 == 0
    torch.manual_seed(21)
    want = dropout_add(xa, ia, 0.5, True)
    xv = (_view(x, off) if which in ("x", "both") else x.clone()).requires_grad_(True)
    iv = _view(idt, off) if which in ("identity", "both") else idt.clone()
    torch.manual_seed(21)
    got = dropout_add(xv, iv, 0.5, True)
    assert got.grad_fn.seed == want.grad_fn.seed
    assert torch.equal(_bits(got.detach()), _bits(want.detach()))
    keep = torch.from_numpy(dm.keep(got.grad_fn.seed, N_VIEW, 0.5)).to(D0)
    assert torch.equal(got.detach() != idt, keep)                       # x * 2 >= 1 is never absorbed by |identity| < 2^23


@pytest.mark.parametrize("route", ["given", "cat"])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_backward_accepts_a_misaligned_upstream_gradient(hip, monkeypatch, off, route):
    """the gradient arrives as a view at element offset `off`: handed in as one, or sliced by cat's backward out of the gradient
    of a buffer in which y follows `off` other elements"""
    from selfocc_amd import dropout
    x, idt, w = _operands((N_VIEW,))
    seen = []
    real = dropout._aligned

    def spy(t):
        seen.append(t.data_ptr() % 16)
        return real(t)
    monkeypatch.setattr(dropout, "_aligned", spy)

    def run(aligned):
        xa, ia = x.clone().requires_grad_(True), idt.clone().requires_grad_(True)
        torch.manual_seed(33)
        y = dropout.dropout_add(xa, ia, 0.5, True)
        del seen[:]
        if aligned:
            y.backward(w.clone())
        elif route == "given":
            y.backward(_view(w, off))
        else:
            head = torch.ones(off, device=D0, requires_grad=True)
            (torch.cat([head, y]) * torch.cat([torch.ones(off, device=D0), w])).sum().backward()
        return y.grad_fn.seed, xa.grad, ia.grad, list(seen)
    seed_a, gx_a, gi_a, ptr_a = run(True)
    seed_v, gx_v, gi_v, ptr_v = run(False)
    assert ptr_a == [0] and ptr_v == [4 * off]                          # the case is what it claims to be
    assert seed_a == seed_v
    assert torch.equal(_bits(gx_v), _bits(gx_a)) and torch.equal(_bits(gi_v), _bits(gi_a)) and torch.equal(gi_a, w)
    keep = torch.from_numpy(dm.keep(seed_v, N_VIEW, 0.5)).to(D0)
    assert torch.equal(gx_v != 0, keep)


def test_c_entries_still_name_a_misaligned_pointer(hip):
    """the re-staging lives in dropout.py; the C entries keep refusing, with a message, what their float4 path cannot take"""
    from selfocc_amd._lib import lib, ptr, current_stream
    buf = torch.ones(16, device=D0)
    out = torch.empty(8, device=D0)
    assert lib().selfocc_dropout_add_fwd(ptr(buf[1:9]), ptr(buf[:8]), ptr(out), 8, 0.5, 1, current_stream(D0)) != 0
    assert b"16-byte aligned" in lib().selfocc_last_error()
    assert lib().selfocc_dropout_bwd(ptr(buf[2:10]), ptr(out), 8, 0.5, 1, current_stream(D0)) != 0
    assert b"16-byte aligned" in lib().selfocc_last_error()
