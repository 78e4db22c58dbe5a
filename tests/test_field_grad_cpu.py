"""CPU: the SDF-gradient entry points (selfocc_field_grad / selfocc_field_grad_bwd, csrc/field_grad.hip) — the struct against
the header through a compiled C program, the host-only argument checks, the compiler's resource report of the new kernels,
and the construction rules of the head's uniform eikonal points (NeuSHead(use_uniform_gradient=...))."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from kernel_report import HIPCC, report
from selfocc_amd import abi, synthetic as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP = sy.CONFIGS["cfg1"]["mapping"]
AABB = list(sy.CONFIGS["cfg1"]["aabb"])


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_field_grad_args_layout_matches_header(tmp_path):
    names = [f for f, _ in abi.SoFieldGradArgs._fields_]
    assert names == ['q', 'grad', 'mode', 'delta']
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_field_grad_args), offsetof(so_field_grad_args, {f}));' for f in names)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} printf("%zu %d %d %d\\n", sizeof(so_query_args), SO_GRAD_ANALYTIC, SO_GRAD_NUMERICAL, '
                   f'SELFOCC_ABI_VERSION); return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    for f, line in zip(names, lines):
        size, off = map(int, line.split())
        assert size == C.sizeof(abi.SoFieldGradArgs) and off == getattr(abi.SoFieldGradArgs, f).offset, f
    # the embedded query struct keeps its layout, the enum values are the mirror's, and the ABI version did not move
    assert lines[4].split() == [str(C.sizeof(abi.SoQueryArgs)), str(abi.GRAD_ANALYTIC), str(abi.GRAD_NUMERICAL), '35']
    assert (abi.GRAD_ANALYTIC, abi.GRAD_NUMERICAL) == (0, 1) and abi.ABI_VERSION == 35
    assert abi.SoFieldGradArgs().mode == abi.GRAD_ANALYTIC             # zero = analytic


def test_field_grad_symbols_exist_and_the_abi_version_is_unchanged():
    from selfocc_amd._lib import lib
    l = lib()
    assert l.selfocc_abi_version() == 35
    for name in ("selfocc_field_grad", "selfocc_field_grad_bwd"):
        assert name in abi.SYMBOLS and getattr(l, name) is not None


def _args(**kw):
    """a call that passes every check; the pointers are never dereferenced (each call below stops in the host checks)"""
    a = abi.SoFieldGradArgs()
    for ax, n in ((a.q.map.h, 32), (a.q.map.w, 32), (a.q.map.d, 4)):
        ax.tot_len, ax.size0, ax.range0 = n, float(n - 1), 12.8
    a.keep = C.create_string_buffer(64)
    a.q.sdf_vol = a.q.xyz = a.grad = C.addressof(a.keep)
    a.q.n, a.mode, a.delta = 0, abi.GRAD_ANALYTIC, 0.0
    for k, v in kw.items():
        if k in ('n', 'xyz', 'sdf_vol'):
            setattr(a.q, k, v)
        else:
            setattr(a, k, v)
    return a


def test_field_grad_argument_checks_are_pure_host_logic():
    """every refusal happens before any HIP call: rc < 0 and the key word in selfocc_last_error(); n == 0 returns 0"""
    from selfocc_amd._lib import lib
    l = lib()
    fake = C.create_string_buffer(64)
    g = C.addressof(fake)
    ok = [dict(), dict(mode=abi.GRAD_NUMERICAL, delta=0.01), dict(delta=-1.0)]        # analytic mode does not read delta
    for kw in ok:
        assert l.selfocc_field_grad(_args(**kw), None) == 0, (kw, l.selfocc_last_error())
        assert l.selfocc_field_grad_bwd(_args(**kw), g, g, g, None) == 0, (kw, l.selfocc_last_error())
    bad = [
        (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
        (dict(mode=abi.GRAD_NUMERICAL, delta=0.0), b"delta"), (dict(mode=abi.GRAD_NUMERICAL, delta=-0.01), b"delta"),
        (dict(mode=abi.GRAD_NUMERICAL, delta=float('nan')), b"delta"),
        (dict(n=-1), b"n must be"),
        (dict(n=5, xyz=None), b"xyz"), (dict(n=5, sdf_vol=None), b"sdf_vol"),
    ]
    for kw, word in bad:
        assert l.selfocc_field_grad(_args(**kw), None) < 0, kw
        err = l.selfocc_last_error()
        assert word in err, (kw, err)
        assert l.selfocc_field_grad_bwd(_args(**kw), g, g, g, None) < 0 and word in l.selfocc_last_error(), kw
    # the output pointers: checked where they are needed (n > 0), still before any launch
    assert l.selfocc_field_grad(_args(n=5, grad=None), None) < 0 and b"grad is NULL" in l.selfocc_last_error()
    assert l.selfocc_field_grad_bwd(_args(n=5), g, g, None, None) < 0 and b"g_sdf_vol" in l.selfocc_last_error()
    assert l.selfocc_field_grad_bwd(_args(n=5), None, None, None, None) == 0        # no upstream: nothing to scatter
    assert l.selfocc_field_grad(None, None) < 0 and b"args is NULL" in l.selfocc_last_error()
    bad_map = _args()
    bad_map.q.map.kind = 7
    assert l.selfocc_field_grad(bad_map, None) < 0 and b"mapping" in l.selfocc_last_error()


# ---- compiler report ---------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
def test_field_grad_kernels_use_no_scratch_and_reach_full_occupancy():
    """analytic / numerical x forward / backward x the two mapping kinds: pure gather / scatter, nothing may spill and nothing
    may cost a wave slot (8 waves per SIMD needs <= 64 VGPRs)"""
    ks = report("field_grad.hip")
    got = sorted((k.base, k.name.split('<')[1].split('>')[0]) for k in ks)        # (template, mapping kind)
    bases = ["field_grad_analytic_bwd_kernel", "field_grad_analytic_kernel", "field_grad_numerical_bwd_kernel",
             "field_grad_numerical_kernel"]
    assert got == sorted((b, mk) for b in bases for mk in ("0", "1")), got
    for k in ks:
        print(f"\n[field_grad resources] {k.base}<{k.name.split('<')[1].split('>')[0]}> VGPRs {k.res['VGPRs']} AGPRs {k.res.get('AGPRs', 0)} "
              f"SGPRs {k.res['TotalSGPRs']} scratch {k.res['ScratchSize']} occupancy {k.res['Occupancy']} LDS {k.res['LDS']}")
        assert k.res["ScratchSize"] == 0, k
        assert k.res["Occupancy"] == 8 and k.res["VGPRs"] + k.res.get("AGPRs", 0) <= 64, k
        assert k.res["LDS"] == 0, k


# ---- operator layer and head ---------------------------------------------------------------------------------------------------
def test_field_grad_is_exported_and_has_no_cpu_fallback():
    import selfocc_amd
    from selfocc_amd import occ
    assert selfocc_amd.field_grad is occ.field_grad and selfocc_amd.field_grad_autograd is occ.field_grad_autograd
    vol = sy.make_volume("cfg1")
    xyz = torch.rand(7, 3)
    for fn in (occ.field_grad, occ.field_grad_autograd):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(vol, xyz)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(vol, xyz, mode='numerical', delta=0.01)


def _head(**kw):
    from selfocc_amd.model.head import NeuSHead
    cfg = dict(roi_aabb=AABB, num_samples=16, num_samples_importance=0, num_up_sample_steps=0, use_numerical_gradients=False,
               ray_number=[4, 6], ray_img_size=[64, 64], mapping_args=MAP, embed_dims=16, color_dims=0, density_layers=2,
               tpv=True, two_split=False)
    cfg.update(kw)
    torch.manual_seed(0)
    return NeuSHead(**cfg)


def test_default_knobs_build_the_head_they_built_before():
    """use_uniform_gradient=False (the default): the three companion knobs are stored and change nothing that is built"""
    base = _head()
    assert (base.use_uniform_gradient, base.sample_gradient, base.nbr_gradient_points, base.uniform_gradient_delta) == \
        (False, False, 128 * 128 * 16, None)
    for kw in (dict(sample_gradient=True), dict(nbr_gradient_points=77, calculate_online=True), dict(uniform_gradient_delta=0.01),
               dict(use_uniform_gradient=True, nbr_gradient_points=77, sample_gradient=True)):
        other = _head(**kw)
        a, b = base.state_dict(), other.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), kw          # no parameter, no buffer, same init
        assert [n for n, _ in base.named_modules()] == [n for n, _ in other.named_modules()], kw
    # numerical gradients INSIDE the march stay refused
    with pytest.raises(NotImplementedError, match="use_numerical_gradients"):
        _head(use_numerical_gradients=True)


def test_uniform_gradient_knob_values_are_checked_by_name():
    with pytest.raises(ValueError, match="nbr_gradient_points"):
        _head(use_uniform_gradient=True, nbr_gradient_points=0)
    with pytest.raises(ValueError, match="uniform_gradient_delta"):
        _head(use_uniform_gradient=True, uniform_gradient_delta=0.0)
    with pytest.raises(ValueError, match="uniform_gradient_delta"):
        _head(use_uniform_gradient=True, uniform_gradient_delta=-0.01)
    with pytest.raises(NotImplementedError, match="use_uniform_gradient=True.*ray_shard"):
        _head(use_uniform_gradient=True, ray_shard=True)
    _head(use_uniform_gradient=False, ray_shard=True)                   # the knob off: ray sharding constructs as before


def test_env_ray_sharding_refuses_the_uniform_points(monkeypatch):
    """SELFOCC_RAY_SHARD=1 turns sharding on after construction: the same refusal, from the forward's own check"""
    import torch.distributed as dist
    from selfocc_amd.render import RaySet
    head = _head(use_uniform_gradient=True, nbr_gradient_points=8)
    monkeypatch.setenv('SELFOCC_RAY_SHARD', '1')
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda *a: 2)
    rays = RaySet(img2lidar=torch.eye(4)[None], nx=6, ny=4)
    with pytest.raises(NotImplementedError, match="use_uniform_gradient=True.*ray sharding"):
        head._sharding(rays)
    head.use_uniform_gradient = False
    assert head._sharding(rays) is True


def test_uniform_gradient_on_a_cpu_volume_fails_at_forward_not_at_construction():
    head = _head(use_uniform_gradient=True, nbr_gradient_points=32, sample_gradient=True).train()     # constructs on the CPU
    H, W, D, Cc = 32, 32, 4, 16
    g = torch.Generator().manual_seed(0)
    rep = [torch.randn(1, H * W, Cc, generator=g), torch.randn(1, D * H, Cc, generator=g), torch.randn(1, W * D, Cc, generator=g)]
    cams = sy.make_cameras("cfg1", 0).numpy()
    os.environ['eval'] = 'false'
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head(rep, [dict(img2lidar=cams)])
    # ... and the new query itself, on the volume the failed forward left behind
    assert head.model.field.volume is not None and not head.model.field.volume.sdf.is_cuda
    for kw in (dict(), dict(numerical=True, delta=0.01)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            head.model.field.gradient(torch.rand(5, 3), **kw)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
            head.model.field.gradient(torch.rand(5, 3), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head._uniform_eik_grad(torch.device('cpu'))
