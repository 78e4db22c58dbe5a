"""CPU: bricks.stacked_view — the parameters of several Linears aliased into ONE stacked weight (no torch.cat per call) stay
ordinary parameters: names, values, gradients, optimiser updates, load_state_dict, deepcopy, re-aliasing after `.to()`,
inference mode, and autograd's in-place check through bricks._TallLinear (on its CPU fallbacks: addmm, batched-GEMM wgrad)."""
import copy

import pytest
import torch
import torch.nn as nn

from selfocc_amd.model.bricks import _TallLinear, stack_rows, stacked_view


def _lins():
    torch.manual_seed(0)
    return nn.Linear(8, 6), nn.Linear(8, 3)


def test_values_names_and_aliasing():
    a, b = _lins()
    wa, wb = a.weight.detach().clone(), b.weight.detach().clone()
    w = stacked_view([a.weight, b.weight])
    assert torch.equal(w, torch.cat([wa, wb], 0)) and torch.equal(a.weight, wa) and torch.equal(b.weight, wb)
    assert w.data_ptr() == a.weight.data_ptr() and b.weight.data_ptr() == a.weight.data_ptr() + a.weight.numel() * 4
    w2 = stacked_view([a.weight, b.weight])                   # second call: already aliased, no new buffer
    assert w2.data_ptr() == w.data_ptr()
    assert set(dict(a.named_parameters())) == {'weight', 'bias'}
    # 1-D parameters (biases)
    bb = stacked_view([a.bias, b.bias])
    assert torch.equal(bb, torch.cat([a.bias.detach(), b.bias.detach()])) and bb.data_ptr() == a.bias.data_ptr()


def test_in_place_updates_are_seen_and_gradients_stay_separate():
    a, b = _lins()
    w = stacked_view([a.weight, b.weight])
    x = torch.randn(5, 8)
    opt = torch.optim.AdamW(list(a.parameters()) + list(b.parameters()), lr=0.1)
    (a(x).sum() + 2 * b(x).sum()).backward()
    assert a.weight.grad.shape == (6, 8) and b.weight.grad.shape == (3, 8)
    assert a.weight.grad.untyped_storage().data_ptr() != b.weight.grad.untyped_storage().data_ptr()
    before = w.clone()
    opt.step()
    w_after = stacked_view([a.weight, b.weight])
    assert w_after.data_ptr() == w.data_ptr() and not torch.equal(w_after, before)
    assert torch.equal(w_after, torch.cat([a.weight.detach(), b.weight.detach()], 0))
    # load_state_dict copies in place: the aliasing survives
    sd = {k: torch.randn_like(v) for k, v in a.state_dict().items()}
    a.load_state_dict(sd)
    assert torch.equal(stacked_view([a.weight, b.weight])[:6], sd['weight']) and stacked_view([a.weight, b.weight]).data_ptr() == w.data_ptr()


def test_moved_or_replaced_parameters_are_realiased_and_non_parameters_refused():
    a, b = _lins()
    w = stacked_view([a.weight, b.weight])
    a = a.double().float()                                    # `.data =` new tensors: aliasing broken
    w2 = stacked_view([a.weight, b.weight])
    assert w2.data_ptr() != w.data_ptr() and torch.equal(w2, torch.cat([a.weight.detach(), b.weight.detach()], 0))
    assert b.weight.data_ptr() == a.weight.data_ptr() + a.weight.numel() * 4
    c = copy.deepcopy(nn.ModuleList([a, b]))                  # deepcopy keeps the sharing inside the copy
    w3 = stacked_view([c[0].weight, c[1].weight])
    assert w3.data_ptr() == c[0].weight.data_ptr() != w2.data_ptr()
    assert stacked_view([a.weight * 1.0, b.weight]) is None   # not a leaf parameter (functional_call views): the caller cats
    assert stacked_view([a.weight, nn.Parameter(torch.zeros(3, 7))]) is None


def _merged(a, b, x):
    """the (T, 9) projection of x through a | b: _TallLinear with two weight / bias groups"""
    return _TallLinear.apply(x, False, a.weight, a.bias, b.weight, b.bias)


def test_first_aliasing_under_inference_mode_then_training():
    a, b = _lins()
    a2, b2 = copy.deepcopy(a), copy.deepcopy(b)                # separate nn.Linear, never stacked
    with torch.inference_mode():
        w, bb = stacked_view([a.weight, b.weight]), stacked_view([a.bias, b.bias])
    assert w is not None and bb is not None and not w.is_inference() and not bb.is_inference()
    assert not any(p.is_inference() for m in (a, b) for p in m.parameters())
    assert b.weight.data_ptr() == a.weight.data_ptr() + a.weight.numel() * 4
    x = torch.randn(5, 8)
    gy = torch.randn(5, 9)
    xa = x.clone().requires_grad_(True)
    _merged(a, b, xa).backward(gy)
    xb = x.clone().requires_grad_(True)
    torch.cat([a2(xb), b2(xb)], 1).backward(gy)
    got = [xa.grad] + [p.grad for m in (a, b) for p in m.parameters()]
    want = [xb.grad] + [p.grad for m in (a2, b2) for p in m.parameters()]
    for g, t in zip(got, want):
        assert g is not None and g.shape == t.shape and torch.allclose(g, t, rtol=1e-5, atol=1e-6)


def test_in_place_change_between_forward_and_backward_raises():
    a, b = _lins()
    x = torch.randn(5, 8, requires_grad=True)
    y = _merged(a, b, x)
    assert b.weight.data_ptr() == a.weight.data_ptr() + a.weight.numel() * 4     # served from the stacked buffer
    with torch.no_grad():
        b.weight.mul_(0.5)                                    # e.g. an EMA or an optimiser step before this backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def test_inference_tensor_parameters_are_not_stacked():
    with torch.inference_mode():
        a, b = _lins()
    assert a.weight.is_inference()
    assert stacked_view([a.weight, b.weight]) is None
    with torch.inference_mode():
        assert stacked_view([a.weight, b.weight]) is None
        assert torch.equal(stack_rows([a.weight, b.weight]), torch.cat([a.weight, b.weight], 0))   # the caller cats
