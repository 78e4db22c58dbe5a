"""GPU: every instantiation of the MSDA kernels (plain forward and its three backward kernels; the fused and camera-loop forward and
backward point kernels per (D, log2 G, value type); the band kernel across band seams) through the public entries, against float64
autograd of the torch port, at bounds five times the float32 port's own error (a few 1e-6 of the largest element) instead of the
1e-3 .. 1e-4 of tests/test_msda_gpu.py.

Case table, reference, mask, metrics and bounds: tests/msda_cases.py.  What makes the bounds trustworthy (the float32 port a factor 5
below them, deliberately defective results a factor 2 above) and that the table reaches every instantiation, as the library's own
plan entry reports it: tests/test_msda_cases_cpu.py.  Every case appends its measured figures to msda_sharp.jsonl next to the render
tests' log (one full run: profiles/msda_sharp_parity.jsonl)."""
import json
import os

import pytest
import torch

import msda_cases as mc
import selfocc_amd.msda as M
from test_render_bwd_gpu import LOG as TRAIN_SHAPE_LOG

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
LOG = os.path.join(os.path.dirname(TRAIN_SHAPE_LOG), "msda_sharp.jsonl")


def _run_plain(case, inp, monkeypatch):
    monkeypatch.setattr(M, "BACKWARD_MODE", case.mode)
    v, loc, aw = (t.to(D0).requires_grad_(True) for t in (inp.value, inp.loc, inp.attw))
    out = M.MultiScaleDeformableAttnFunction.apply(v, inp.shapes.to(D0), inp.starts.to(D0), loc, aw, 64)
    out.backward(inp.gout.to(D0))
    return out.detach(), v.grad, loc.grad, aw.grad


def _run_sampling(case, inp):
    """the fused or the camera-loop Function on the case's route: value layout, a value that is a column block of a wider matrix,
    dense or merged offset / logit rows, a fresh g_value or a ValueGradSink"""
    n, nq, H, d, L, P = case.n, case.nq, mc.HEADS, case.d, case.L, case.P
    cross = case.form == 'cross'
    sh, st = inp.shapes.to(D0), inp.starts.to(D0)
    host = [int(x) for x in inp.shapes.reshape(-1)]
    assert M.msda_fused_supported(host, n, nq, H, d, L, P, case.bf16)
    wide = None
    if case.vstride:         # columns [H d, 2 H d) of rows 3 H d + 4 floats wide, other values around them
        wide = (100 * torch.randn(n, inp.nv, 3 * H * d + 4, generator=torch.Generator().manual_seed(1))).to(D0)
        wide[:, :, H * d:2 * H * d] = inp.value.reshape(n, inp.nv, H * d).to(D0)
        wide.requires_grad_(True)
        v = wide[:, :, H * d:2 * H * d].unflatten(-1, (H, d))
        assert not v.is_contiguous()
    else:
        v = (M.to_head_major(inp.value) if case.head_major else inp.value).to(D0).requires_grad_(True)
    if case.merged:
        rows = inp.off.shape[:-4]
        ol = torch.cat([inp.off.reshape(*rows, -1), inp.logits.reshape(*rows, -1)], -1).to(D0).requires_grad_(True)
        off, lg, merged_LP = ol, None, (L, P)
    else:
        off, lg, merged_LP = inp.off.to(D0).requires_grad_(True), inp.logits.to(D0).requires_grad_(True), None
    sink = M.ValueGradSink(2) if case.sink else None
    tail = (off, lg, host, case.head_major, case.bf16, merged_LP, (sink, 1) if sink else None)
    seen = v.detach().to(torch.bfloat16) if case.bf16 else v.detach()
    if cross:
        out = M.MSDACrossFunction.apply(v, sh, st, inp.ref.to(D0), inp.vis.to(D0), *tail)
        # the inference entry on the same route: the same kernel, the same bits
        assert torch.equal(out.detach(), M.msda_cross_inference(seen, sh, st, inp.ref.to(D0), inp.vis.to(D0), off.detach(),
                                                                None if lg is None else lg.detach(), case.head_major, merged_LP))
    else:
        out = M.MSDAFusedFunction.apply(v, sh, st, inp.ref.to(D0), case.ref_kind, *tail)
        assert torch.equal(out.detach(), M.msda_fused_inference(seen, sh, st, inp.ref.to(D0), case.ref_kind, off.detach(),
                                                                None if lg is None else lg.detach(), case.head_major, merged_LP))
    out.backward(inp.gout.to(D0))
    if wide is not None:
        gv = wide.grad[:, :, H * d:2 * H * d].unflatten(-1, (H, d))
        assert wide.grad[:, :, :H * d].abs().max() == 0 and wide.grad[:, :, 2 * H * d:].abs().max() == 0
    else:
        gv = v.grad.permute(0, 2, 1, 3) if case.head_major else v.grad
    if sink is not None:     # written into column block 1 of the shared pixel-major buffer, and nowhere else
        assert sink.buf is not None and torch.equal(gv, sink.buf[:, :, 1]) and sink.buf[:, :, 0].abs().max() == 0
    if case.merged:
        k = 2 * H * L * P
        g_off, g_lg = ol.grad[..., :k].reshape(inp.off.shape), ol.grad[..., k:].reshape(inp.logits.shape)
    else:
        g_off, g_lg = off.grad, lg.grad
    return out.detach(), gv, g_off, g_lg


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_msda_forward_and_backward_vs_float64_autograd(hip, case, monkeypatch):
    r = mc.reference(case)
    inp = r.inp
    got = _run_plain(case, inp, monkeypatch) if case.form == 'plain' else _run_sampling(case, inp)
    torch.cuda.synchronize()
    out, gv, gp, gw = (t.cpu().double() for t in got)
    assert gv.dtype == torch.float64 and got[1].dtype == torch.float32
    m = mc.metrics(r, out, gv, gp, gw.reshape(r.port.gw.shape))
    p = mc.plan(case)
    rec = dict(case=mc.case_id(case), form=case.form, d=case.d, log2_group=p.log2_group, bf16=case.bf16, L=case.L, P=case.P, n=case.n,
               nq=case.nq, banded=p.banded, bands=p.bands, count_here=p.count_here, bin_vis=p.bin_vis,
               points_compared=r.keep.float().mean().item(), **m)
    print("\n" + json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    b = mc.bounds(case)
    for k, val in m.items():
        assert val <= b[k], (k, val, b[k], rec)
    if case.form == 'cross':          # a query no camera sees: zero output, zero gradients
        assert out[0].abs().max() == 0 and gp[0].abs().max() == 0 and gw[0].abs().max() == 0
