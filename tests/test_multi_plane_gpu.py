"""GPU: the per-plane norm / FFN of the TPV encoder (MultiPlaneNorm, MultiPlaneFFN, TPVFormerLayer(multi_plane_ffn_norm=True)).

* selfocc_layernorm_fwd_grouped / _bwd_grouped (csrc/layernorm.hip): one launch per direction over the concatenated planes, each
  row normalised with the (gamma, beta) of the group it lies in — against float64 at the bounds tests/test_layernorm_gpu.py
  uses for the ungrouped kernels, on row splits that put group boundaries inside, at and next to the 8-row blocks; every group
  gets its own seed, so a row served with another group's parameters is an O(1) error; empty groups give exact zeros; one
  group is the ungrouped entry bit for bit; the backward is run-to-run bit-identical.  (Every group of a split against the
  ungrouped entry bit for bit, at more widths and with a group past the 2 048-block cap by one row, and the sharp float64
  bounds: tests/test_layernorm_sharp_gpu.py, tests/layernorm_cases.py.)
* the module fixture and the two encoder fixtures the REAL reference classes wrote (tests/golden/make_golden_multi_plane.py).
* launch counts, sync-freedom, torch.inference_mode().
"""
import json
import os

import numpy as np
import pytest
import torch

import multi_plane_cases as mpc
from util import grad_digest

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")
# the project's bounds for this fixture family (tests/test_golden_encoder_full_gpu.py): the arithmetic per row is the same
GRAD_TOL = 2e-5
OUT_TOL = 2e-5

SPLITS = [(1, 1, 1), (16, 16, 16), (17, 15, 33), (31, 0, 64), (0, 5, 0), (257, 63, 65), (2065, 201, 201), (7, 9), (40,),
          (3, 0, 0, 8, 8, 1, 0, 25), (20000, 3, 1000)]       # the last: a group on the 2 048-block cap (> 16 384 rows)


def _case(sizes, C, seed):
    """x, dy over the concatenated rows and one (gamma, beta) per group, each group from its own seed"""
    T, G = sum(sizes), len(sizes)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, C, generator=g) * 3.0 + 1.5
    dy = torch.randn(T, C, generator=g)
    gamma, beta = torch.empty(G, C), torch.empty(G, C)
    for i in range(G):
        gi = torch.Generator().manual_seed(1000 * seed + i)
        gamma[i] = torch.randn(C, generator=gi) * 0.5 + 1.0 + i
        beta[i] = torch.randn(C, generator=gi) * 0.1 - i
    return x, dy, gamma, beta


def _grouped(hip, x, dy, gamma, beta, sizes, eps=1e-5):
    """raw entry points: (y, mean, rstd, dx, dgamma, dbeta) on the GPU"""
    from selfocc_amd import abi
    from selfocc_amd._lib import check, ptr, current_stream
    T, C = x.shape
    G = len(sizes)
    gr = abi.SoRowGroups.from_sizes(sizes)
    x, dy, gamma, beta = x.to(D0), dy.to(D0), gamma.to(D0).contiguous(), beta.to(D0).contiguous()
    y, dx = torch.full_like(x, float('nan')), torch.full_like(x, float('nan'))
    mean, rstd = torch.full((T,), float('nan'), device=D0), torch.full((T,), float('nan'), device=D0)
    dg, db = torch.full((G, C), float('nan'), device=D0), torch.full((G, C), float('nan'), device=D0)
    st = current_stream(D0)
    check(hip.selfocc_layernorm_fwd_grouped(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), T, C, eps, gr, st), "fwd")
    nbytes = int(hip.selfocc_layernorm_bwd_grouped_workspace(T, C, gr))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=D0)
    check(hip.selfocc_layernorm_bwd_grouped(ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dg), ptr(db), T, C, gr,
                                            ptr(ws), nbytes, st), "bwd")
    torch.cuda.synchronize()
    return y, mean, rstd, dx, dg, db


def _reference64(x, dy, gamma, beta, sizes, eps=1e-5):
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ys = [torch.nn.functional.layer_norm(xp, (x.shape[1],), gr[i], br[i], eps) for i, xp in enumerate(torch.split(xr, list(sizes)))]
    y = torch.cat(ys)
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad


@pytest.mark.parametrize("C", [96, 32])
@pytest.mark.parametrize("sizes", SPLITS, ids=lambda s: 'x'.join(map(str, s)))
def test_grouped_layernorm_vs_float64(hip, sizes, C):
    x, dy, gamma, beta = _case(sizes, C, 7 + sum(sizes) + C)
    y, mean, rstd, dx, dg, db = _grouped(hip, x, dy, gamma, beta, sizes)
    yr, dxr, dgr, dbr = _reference64(x, dy, gamma, beta, sizes)
    # the bounds of tests/test_layernorm_gpu.py
    assert torch.allclose(y.cpu().double(), yr, rtol=1e-5, atol=1e-5), float((y.cpu().double() - yr).abs().max())
    assert torch.allclose(dx.cpu().double(), dxr, rtol=1e-4, atol=1e-5), float((dx.cpu().double() - dxr).abs().max())
    scale = max(1.0, float(dgr.abs().max()))
    assert torch.allclose(dg.cpu().double(), dgr, rtol=1e-4, atol=1e-4 * scale)
    assert torch.allclose(db.cpu().double(), dbr, rtol=1e-4, atol=1e-4 * scale)
    assert torch.allclose(mean.cpu().double(), x.double().mean(1), rtol=1e-5, atol=1e-5)
    for i, n in enumerate(sizes):
        if n == 0:          # an empty group: exact zeros, not a left-over
            assert torch.equal(dg[i].cpu(), torch.zeros(C)) and torch.equal(db[i].cpu(), torch.zeros(C)), i
    # run to run bit-identical (per-block partials, fixed-order reduction; no atomics)
    again = _grouped(hip, x, dy, gamma, beta, sizes)
    for a, b in zip((y, mean, rstd, dx, dg, db), again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rows,C", [(78899, 96), (1000, 32), (7, 128), (1, 4), (4099, 64)])
def test_one_group_is_the_ungrouped_entry_bit_for_bit(hip, rows, C):
    from selfocc_amd._lib import check, ptr, current_stream
    x, dy, gamma, beta = _case((rows,), C, rows + C)
    got = _grouped(hip, x, dy, gamma, beta, (rows,))
    x, dy, gamma, beta = x.to(D0), dy.to(D0), gamma[0].to(D0).contiguous(), beta[0].to(D0).contiguous()
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=D0), torch.empty(rows, device=D0)
    dg, db = torch.empty(C, device=D0), torch.empty(C, device=D0)
    st = current_stream(D0)
    check(hip.selfocc_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, C, 1e-5, st), "fwd")
    nbytes = int(hip.selfocc_layernorm_bwd_workspace(rows, C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=D0)
    check(hip.selfocc_layernorm_bwd(ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dy), ptr(dx), ptr(dg), ptr(db), rows, C, ptr(ws),
                                    nbytes, st), "bwd")
    torch.cuda.synchronize()
    for name, a, b in zip(('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta'), got, (y, mean, rstd, dx, dg[None], db[None])):
        assert torch.equal(a, b), name


def test_empty_tensor_gives_zero_parameter_gradients(hip):
    x, dy, gamma, beta = _case((0, 0, 0), 96, 1)
    y, mean, rstd, dx, dg, db = _grouped(hip, x, dy, gamma, beta, (0, 0, 0))
    assert torch.equal(dg.cpu(), torch.zeros(3, 96)) and torch.equal(db.cpu(), torch.zeros(3, 96))


@pytest.mark.parametrize("case", ['noid', 'id'])
def test_module_fixture_on_the_gpu(hip, case):
    """the real MultiPlaneFFN -> MultiPlaneNorm fixture with the row thresholds lowered so that the tall-Linear kernels serve
    the three planes' FFNs, and the grouped LayerNorm really ran"""
    from selfocc_amd.model import bricks
    z, ffn, norm = mpc.build_modules(D0)
    old = (bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows)
    n0 = bricks.GROUPED_LN_CALLS[0]
    try:
        bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = 1, 1
        got = mpc.run_modules(z, ffn, norm, case, D0)
        with torch.no_grad():
            xs = [torch.tensor(z[f'x.{p}']).to(D0) for p in range(3)]
            ids = [torch.tensor(z[f'identity.{p}']).to(D0) for p in range(3)] if case == 'id' else None
            inf = norm(ffn(xs, ids))
            fused = ffn(xs, ids, post_norm=norm)            # inference: each plane's norm in its FFN's last projection
    finally:
        bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = old
    assert bricks.GROUPED_LN_CALLS[0] - n0 == 2            # the training pass and the no_grad pass; `fused` needs none
    worst = 0.0
    for k, v in got.items():
        worst = max(worst, mpc.rel_err(v, z[k]))
        assert mpc.rel_err(v, z[k]) <= GRAD_TOL, (k, mpc.rel_err(v, z[k]))
    for p in range(3):
        assert mpc.rel_err(inf[p], z[f'{case}.norm.{p}']) <= OUT_TOL
        assert mpc.rel_err(fused[p], z[f'{case}.norm.{p}']) <= OUT_TOL
    print('module fixture', case, 'worst relative error', worst)


@pytest.mark.parametrize("case", ['noid', 'id'])
def test_module_fixture_through_the_grouped_linears(hip, case):
    """the same fixture on the concatenated planes (what TPVFormerLayer runs): MultiPlaneFFN.forward_cat through
    _GroupedTallLinear (forward, wgrad; the input gradient of K = 32 / 64 falls to matmuls) and MultiPlaneNorm.forward_cat,
    training pass and the two-launch inference form; the grouped Functions really ran"""
    from selfocc_amd.model import bricks
    z, ffn, norm = mpc.build_modules(D0)
    sizes = [z[f'x.{p}'].shape[1] for p in range(3)]
    cat = lambda key: torch.cat([torch.tensor(np.array(z[f'{key}.{p}'])) for p in range(3)], 1).to(D0)
    x, dirs = cat('x').requires_grad_(True), cat('dir')
    idt = cat('identity').requires_grad_(True) if case == 'id' else None
    old = bricks.LINEAR_FWD_MIN_ROWS
    f0, n0 = bricks.GROUPED_FFN_CALLS[0], bricks.GROUPED_LN_CALLS[0]
    try:
        bricks.LINEAR_FWD_MIN_ROWS = 1
        mid = ffn.forward_cat(x, sizes, idt)
        out = norm.forward_cat(mid, sizes)
        params = [(f'param.ffn.{n}', p) for n, p in ffn.named_parameters()] + [(f'param.norm.{n}', p) for n, p in norm.named_parameters()]
        grads = torch.autograd.grad((out * dirs).sum(), [p for _, p in params] + [x] + ([idt] if idt is not None else []))
        with torch.no_grad():
            fused = ffn.forward_cat(x.detach(), sizes, None if idt is None else idt.detach(), post_norm=norm)
    finally:
        bricks.LINEAR_FWD_MIN_ROWS = old
    assert bricks.GROUPED_FFN_CALLS[0] - f0 == 2 and bricks.GROUPED_LN_CALLS[0] - n0 == 1
    got = {f'{case}.grad.{n}': g for (n, _), g in zip(params, grads)}
    split = lambda t: torch.split(t, sizes, 1)
    for p in range(3):
        got[f'{case}.ffn.{p}'], got[f'{case}.norm.{p}'] = split(mid)[p], split(out)[p]
        got[f'{case}.grad.x.{p}'] = split(grads[len(params)])[p]
        if idt is not None:
            got[f'{case}.grad.identity.{p}'] = split(grads[len(params) + 1])[p]
        assert mpc.rel_err(split(fused)[p], z[f'{case}.norm.{p}']) <= OUT_TOL
    assert sorted(got) == sorted(k for k in z if k.startswith(case + '.'))
    for k, v in got.items():
        assert mpc.rel_err(v, z[k]) <= GRAD_TOL, (k, mpc.rel_err(v, z[k]))


def _setup(variant):
    z, spec, enc, lifter, feats, l2i, loss_dirs = mpc.setup_encoder_cpu(variant)
    enc, lifter = enc.to(D0).eval(), lifter.to(D0).eval()        # dropout off (as in the generator), autograd on
    feats = [f.to(D0).requires_grad_(True) for f in feats]
    metas = [dict(lidar2img=l2i, img_shape=tuple(spec['img_shape']))]
    return z, enc, lifter, feats, metas, [d.to(D0) for d in loss_dirs]


def _train_pass(enc, lifter, feats, metas, loss_dirs):
    out = enc(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
    loss = sum((o * d).sum() for o, d in zip(out, loss_dirs)) / sum(o.numel() for o in out)
    names = [('enc', n) for n, _ in enc.named_parameters()] + [('lift', n) for n, _ in lifter.named_parameters()] + \
        [('feat', str(i)) for i in range(len(feats))]
    grads = torch.autograd.grad(loss, list(enc.parameters()) + list(lifter.parameters()) + feats)
    return [o.detach() for o in out], loss.detach(), dict(zip(names, grads))


LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out", "encoder_mp_parity.jsonl")


def _report(tag, worst):
    """measured worst errors -> parity_out/encoder_mp_parity.jsonl (kept as profiles/encoder_mp_parity.jsonl)"""
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(dict(variant=tag, **worst)) + "\n")


def _check_out(tag, z, out, worst):
    for got, key in zip(out, mpc.PLANES):
        ref = torch.tensor(np.array(z[key]))
        err = (got.cpu() - ref).abs().max().item()
        worst['out'] = max(worst['out'], err)
        assert got.shape == ref.shape and torch.allclose(got.cpu(), ref, rtol=OUT_TOL, atol=OUT_TOL), (tag, key, err)


@pytest.mark.parametrize("min_rows", [None, 1], ids=['default', 'all_kernels'])
@pytest.mark.parametrize("variant", ['post', 'pre'])
def test_encoder_fixture_training_pass_vs_reference(hip, variant, min_rows):
    """outputs, loss and every stored gradient digest (post-norm: every parameter, the lifter, the FPN maps; pre-norm: the
    FFN / norm parameters) of the REAL TPVFormerEncoder with multi_plane_ffn_norm=True"""
    from selfocc_amd.model import bricks
    z, enc, lifter, feats, metas, loss_dirs = _setup(variant)
    old = (bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows)
    n0, f0 = bricks.GROUPED_LN_CALLS[0], bricks.GROUPED_FFN_CALLS[0]
    try:
        if min_rows is not None:
            bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = min_rows, min_rows
        out, loss, grads = _train_pass(enc, lifter, feats, metas, loss_dirs)
    finally:
        bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = old
    assert bricks.GROUPED_LN_CALLS[0] - n0 == 3 * len(enc.layers)      # every norm step was ONE grouped launch
    # 975 rows: below LINEAR_FWD_MIN_ROWS the FFN step is the per-plane composition, with the threshold at 1 the grouped Linears
    assert bricks.GROUPED_FFN_CALLS[0] - f0 == (0 if min_rows is None else len(enc.layers))
    tag = f'{variant}.train.{"default" if min_rows is None else "all_kernels"}'
    worst = dict(out=0.0, grad=0.0, grad_name='')
    _check_out(tag, z, out, worst)
    assert abs(loss.item() - float(np.asarray(z['loss']).reshape(-1)[0])) <= 1e-5 * max(1.0, abs(float(np.asarray(z['loss']).reshape(-1)[0]))), (tag, loss.item(), float(np.asarray(z['loss']).reshape(-1)[0]))
    n_checked = 0
    for (pref, n), g in grads.items():
        for kind, t in grad_digest(g).items():
            key = f'grad.{pref}.{n}.{kind}'
            if key not in z:
                assert variant == 'pre' and not ('.ffns.' in n or '.norms.' in n), key
                continue
            ref = torch.tensor(np.array(z[key]))
            assert t.shape == ref.shape, (tag, key)
            scale = ref.abs().max().item()
            assert scale > 0, key                   # every parameter and input receives gradient in the reference
            rel = (t - ref).abs().max().item() / scale
            if rel > worst['grad']:
                worst.update(grad=rel, grad_name=f'{pref}.{n}.{kind}')
            n_checked += 1
    _report(tag, worst)
    print(tag, worst)
    assert worst['grad'] <= GRAD_TOL, (tag, worst)
    assert n_checked == sum(1 for k in z if k.startswith('grad.'))


@pytest.mark.parametrize("min_rows", [None, 1], ids=['default', 'all_kernels'])
@pytest.mark.parametrize("variant", ['post', 'pre'])
def test_encoder_fixture_inference_vs_reference(hip, variant, min_rows):
    """no_grad: post-norm layers carry each plane's norm in the cross-attention's / FFN's last projection (min_rows = 1: through
    selfocc_linear_fwd), the norm after the self-attention is one grouped launch"""
    from selfocc_amd.model import bricks
    z, enc, lifter, feats, metas, loss_dirs = _setup(variant)
    old = bricks.LINEAR_FWD_MIN_ROWS
    n0, f0 = bricks.GROUPED_LN_CALLS[0], bricks.GROUPED_FFN_CALLS[0]
    try:
        if min_rows is not None:
            bricks.LINEAR_FWD_MIN_ROWS = min_rows
        with torch.no_grad():
            out = enc(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
    finally:
        bricks.LINEAR_FWD_MIN_ROWS = old
    assert bricks.GROUPED_LN_CALLS[0] - n0 == (1 if variant == 'post' else 3) * len(enc.layers)
    assert bricks.GROUPED_FFN_CALLS[0] - f0 == (0 if min_rows is None else len(enc.layers))
    tag = f'{variant}.no_grad.{"default" if min_rows is None else "all_kernels"}'
    worst = dict(out=0.0)
    _check_out(tag, z, out, worst)
    _report(tag, worst)


def _kernels(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_multi_plane_norm_launch_counts(hip):
    """no_grad: the per-plane norm of all three planes is exactly ONE kernel; training: forward + backward launch no more
    kernels than the shared LayerNorm on the same concatenated tensor (counted in the same test)"""
    from selfocc_amd.model import bricks
    sizes = [2065, 201, 201]
    mp = bricks.MultiPlaneNorm(96).to(D0)
    shared = bricks.FastLayerNorm(96).to(D0)
    x = torch.randn(1, sum(sizes), 96, device=D0)
    dy = torch.randn_like(x)

    def train(norm_fn, params):
        xr = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        return _kernels(lambda: torch.autograd.grad(norm_fn(xr), [xr] + list(params), dy))

    with torch.no_grad():
        mp.forward_cat(x, sizes)                         # warm-up: the parameters are aliased into their stacked buffers once
        names = _kernels(lambda: mp.forward_cat(x, sizes))
    assert len(names) == 1 and 'layernorm_fwd_kernel' in names[0], names
    train(lambda t: mp.forward_cat(t, sizes), mp.parameters())
    k_mp = train(lambda t: mp.forward_cat(t, sizes), mp.parameters())
    k_shared = train(shared, shared.parameters())
    assert len(k_mp) <= len(k_shared), (k_mp, k_shared)
    assert sum('layernorm' in n for n in k_mp) == 3, k_mp          # forward, backward, the per-group reduction


def test_multi_plane_ffn_and_norm_launch_counts(hip):
    """at the shipped plane sizes (66 049 / 6 425 / 6 425 rows, 96 / 192): under no_grad a post-norm layer's FFN plus its norm is
    exactly TWO kernels for all three planes (Linear + ReLU; Linear + identity + per-plane LayerNorm); in training, forward +
    backward of MultiPlaneFFN + MultiPlaneNorm launch no more kernels than the shared FFN + LayerNorm on the same concatenated
    tensor, counted here"""
    from selfocc_amd.model import bricks
    sizes = [257 * 257, 25 * 257, 257 * 25]
    ffn, norm = bricks.MultiPlaneFFN(96, 192, ffn_drop=0.1).to(D0).eval(), bricks.MultiPlaneNorm(96).to(D0).eval()
    sffn, snorm = bricks.FFN(96, 192, ffn_drop=0.1).to(D0).eval(), bricks.FastLayerNorm(96).to(D0).eval()
    x = torch.randn(1, sum(sizes), 96, device=D0)
    dy = torch.randn_like(x)
    n0 = bricks.GROUPED_FFN_CALLS[0]
    with torch.no_grad():
        ref = torch.cat(norm(ffn(torch.split(x, sizes, 1))), 1)           # per plane (also aliases the parameter stacks once)
        got = ffn.forward_cat(x, sizes, post_norm=norm)
        assert got is not None and torch.allclose(got, ref, rtol=1e-5, atol=1e-5)
        names = _kernels(lambda: ffn.forward_cat(x, sizes, post_norm=norm))
    assert len(names) == 2 and all('linear_fwd' in n for n in names), names

    def train(fn, params):
        xr = x.clone().requires_grad_(True)
        torch.cuda.synchronize()
        return _kernels(lambda: torch.autograd.grad(fn(xr), [xr] + list(params), dy))

    mp_fn = lambda t: norm.forward_cat(ffn.forward_cat(t, sizes), sizes)
    mp_params = list(ffn.parameters()) + list(norm.parameters())
    train(mp_fn, mp_params)
    k_mp = train(mp_fn, mp_params)
    sh_fn = lambda t: snorm(sffn(t))
    sh_params = list(sffn.parameters()) + list(snorm.parameters())
    train(sh_fn, sh_params)
    k_sh = train(sh_fn, sh_params)
    assert bricks.GROUPED_FFN_CALLS[0] - n0 == 4
    assert len(k_mp) <= len(k_sh), (len(k_mp), len(k_sh), k_mp, k_sh)


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def _new_frame(feats, metas, seed):
    g = torch.Generator().manual_seed(seed)
    f2 = [(f.detach().cpu() + 0.1 * torch.randn(f.shape, generator=g)).to(D0) for f in feats]
    l2i = metas[0]['lidar2img'].copy()
    l2i[:, :3, 3] += 0.01
    return f2, [dict(lidar2img=l2i, img_shape=metas[0]['img_shape'])]


def test_multi_plane_encoder_is_sync_free_and_runs_under_inference_mode(hip):
    """after a warm-up pass, a NEW inference frame and a NEW training step of the multi-plane encoder issue no host <-> device
    synchronisation; the inference frame also runs under torch.inference_mode() and equals the no_grad one, and training still
    works afterwards (the stacked parameter buffers never become inference tensors)"""
    from selfocc_amd.model import bricks
    z, enc, lifter, feats, metas, loss_dirs = _setup('post')
    old = (bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows)
    bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = 1, 1       # 975 rows: let the grouped Linears serve the FFN steps
    f0 = bricks.GROUPED_FFN_CALLS[0]
    try:
        _sync_free_body(enc, lifter, feats, metas, loss_dirs)
    finally:
        bricks.LINEAR_FWD_MIN_ROWS, bricks.TallLinear.min_rows = old
    assert bricks.GROUPED_FFN_CALLS[0] - f0 == 5 * len(enc.layers)


def _sync_free_body(enc, lifter, feats, metas, loss_dirs):
    def infer(f, m):
        return enc(lifter(f)['representation'], ms_img_feats=f, metas=m)['representation']

    with torch.inference_mode():
        first = infer([f.detach() for f in feats], metas)           # the very first call comes under inference mode
    with torch.no_grad():
        ref = infer([f.detach() for f in feats], metas)
        f2, m2 = _new_frame(feats, metas, 1)
        with no_sync():
            infer(f2, m2)
    for a, b in zip(first, ref):
        assert torch.equal(a, b)
    _train_pass(enc, lifter, feats, metas, loss_dirs)                # warm-up of the training path
    f3, m3 = _new_frame(feats, metas, 2)
    f3 = [f.requires_grad_(True) for f in f3]
    with no_sync():
        out, loss, grads = _train_pass(enc, lifter, f3, m3, loss_dirs)
    assert all(torch.isfinite(g).all() for g in grads.values()) and all(not p.is_inference() for p in enc.parameters())
