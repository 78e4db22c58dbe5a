"""CPU: MultiPlaneFFN / MultiPlaneNorm / TPVFormerLayer(multi_plane_ffn_norm=True) — the reference's per-plane FFN and norm
(model/encoder/tpvformer/modules/split_fpn.py, split_norm.py, tpvformer_encoder_layer.py:57,186-217) — build through the
registry with the reference's parameter names, reproduce the fixture the REAL classes wrote (tests/golden/
make_golden_multi_plane.py) through the per-plane composition of the existing modules, and the grouped LayerNorm entry points
validate their row-group table in pure host logic."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import multi_plane_cases as mpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer_cfg(**over):
    layer = copy.deepcopy(mpc.cfg()['encoder']['transformerlayers'][0])
    layer.update(over)
    return layer


def test_the_three_configs_build_through_the_registry():
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    from selfocc_amd.model import bricks
    keys = mpc.cfg()['layer_keys']
    ffn = MODELS.build(dict(embed_dims=96, **keys['ffn_cfgs']))
    assert isinstance(ffn, bricks.MultiPlaneFFN) and len(ffn.ffns) == 3 and all(isinstance(f, bricks.FFN) for f in ffn.ffns)
    assert ffn.ffns[1].layers[0][0].weight.shape == (192, 96) and ffn.ffns[2].layers[0][2].p == 0.1
    name, norm = bricks.build_norm_layer(keys['norm_cfg'], 96)
    assert isinstance(norm, bricks.MultiPlaneNorm) and len(norm.norms) == 3 and norm.norms[0].eps == 1e-5
    assert bricks.build_norm_layer(dict(type='MultiPlaneNorm', norm_cfg=dict(type='LN', eps=1e-3)), 32)[1].norms[2].eps == 1e-3
    layer = MODELS.build(_layer_cfg())
    assert layer.multi_plane_ffn_norm and isinstance(layer.ffns[0], bricks.MultiPlaneFFN)
    assert all(isinstance(n, bricks.MultiPlaneNorm) for n in layer.norms) and len(layer.norms) == 3
    pre = MODELS.build(_layer_cfg(operation_order=mpc.cfg()['encoder_prenorm']['transformerlayers'][0]['operation_order']))
    assert pre.pre_norm and pre.multi_plane_ffn_norm


def test_parameter_names_are_the_references_and_its_state_dict_loads_strictly():
    z, ffn, norm = mpc.build_modules()          # load_state_dict(strict=True) of the real classes' state dicts inside
    names = mpc.cfg()['names']
    assert [n for n, _ in ffn.named_parameters()] == names['ffn']          # same names in the same registration order
    assert [n for n, _ in norm.named_parameters()] == names['norm']
    assert 'ffns.2.layers.0.0.weight' in names['ffn'] and 'ffns.0.layers.1.bias' in names['ffn'] and 'norms.1.weight' in names['norm']
    for which, m in (('ffn', ffn), ('norm', norm)):
        for k, v in m.state_dict().items():
            assert np.array_equal(v.numpy(), z[f'param.{which}.{k}']), k
    # the encoders: one reference parameter per parameter of ours, by name, in the reference's order
    for variant, key in (('post', 'encoder'), ('pre', 'encoder_prenorm')):
        _, _, enc, *_ = mpc.setup_encoder_cpu(variant)
        assert [n for n, _ in enc.named_parameters()] == names[key]
        assert any(n == 'layers.1.ffns.0.ffns.2.layers.0.0.weight' for n in names[key])
        assert any(n == 'layers.0.norms.2.norms.1.bias' for n in names[key])


@pytest.mark.parametrize("case", ['noid', 'id'])
def test_module_fixture_on_the_cpu_composition(case):
    """outputs and every gradient of the real MultiPlaneFFN -> MultiPlaneNorm to 1e-6 of each tensor's scale"""
    z, ffn, norm = mpc.build_modules()
    got = mpc.run_modules(z, ffn, norm, case)
    keys = [k for k in z if k.startswith(case + '.')]
    assert sorted(keys) == sorted(got) and len(keys) == (12 + 6 + 3 + 6 + (3 if case == 'id' else 0))
    for k in keys:
        assert got[k].shape == z[k].shape, k
        assert mpc.rel_err(got[k], z[k]) <= 1e-6, (k, mpc.rel_err(got[k], z[k]))
    # forward_cat (what TPVFormerLayer calls) is the same function of the concatenated planes
    mid = [torch.tensor(z[f'{case}.ffn.{p}']) for p in range(3)]
    cat = norm.forward_cat(torch.cat(mid, 1), [m.shape[1] for m in mid])
    for p, o in enumerate(torch.split(cat, [m.shape[1] for m in mid], 1)):
        assert mpc.rel_err(o, z[f'{case}.norm.{p}']) <= 1e-6


def test_both_fixtures_regenerate_from_seeds():
    from util import seeded_fill
    z, ffn, norm = mpc.build_modules()
    spec = mpc.cfg()['modules']
    seeded_fill(ffn, spec['seed_ffn'])
    seeded_fill(norm, spec['seed_norm'])
    assert np.allclose([sum(float(p.detach().double().sum()) for p in ffn.parameters())], z['check.ffn'], rtol=1e-9)
    assert np.allclose([sum(float(p.detach().double().sum()) for p in norm.parameters())], z['check.norm'], rtol=1e-9)
    inp = mpc.generator().module_inputs(spec)
    assert np.allclose([float(t.double().sum()) for planes in inp.values() for t in planes], z['check.inputs'], rtol=1e-9)
    for kind, planes in inp.items():
        for p, t in enumerate(planes):
            assert np.array_equal(t.numpy(), z[f'{kind}.{p}'])
    for variant in ('post', 'pre'):
        z, spec, enc, *_ = mpc.setup_encoder_cpu(variant)       # asserts the generator's checksums
        names = {n for n, _ in enc.named_parameters()}
        stored = {k[len('grad.enc.'):].rsplit('.', 1)[0] for k in z if k.startswith('grad.enc.')}
        if variant == 'post':
            assert names == stored                      # one reference gradient per parameter of ours, by name
        else:
            assert stored == {n for n in names if '.ffns.' in n or '.norms.' in n} and len(stored) == 2 * (12 + 18)
            # the generator picked this variant's parameter seed so that the reference's own rounding noise (against its float64
            # run, and under one ulp of noise on every Linear output) is an order of magnitude below the 2e-5 of the GPU test
            own = [float(np.asarray(v).reshape(-1)[0]) for k, v in z.items() if k.startswith(('spread.grad.', 'noise.grad.'))]
            assert len(own) == 2 * len(stored) and max(own) <= 2.5e-6, max(own)
        assert float(np.abs(z['loss']).max()) > 0
    for f in os.listdir(mpc.G):
        if f.startswith(('encoder_full_mp', 'multi_plane')):
            assert os.path.getsize(os.path.join(mpc.G, f)) < (1 << 20), f


def test_build_norm_layer_still_refuses_other_types():
    from selfocc_amd.model.bricks import build_norm_layer, FastLayerNorm
    assert isinstance(build_norm_layer(dict(type='LN'), 8)[1], FastLayerNorm)
    for bad, word in ((dict(type='BN'), 'BN'), (dict(type='GN', num_groups=2), 'GN'),
                      (dict(type='MultiPlaneNorm', norm_cfg=dict(type='BN')), 'MultiPlaneNorm of BN'),
                      (dict(type='MultiPlaneNorm', norm_cfg=dict(type='MultiPlaneNorm')), 'MultiPlaneNorm of MultiPlaneNorm')):
        with pytest.raises(NotImplementedError, match=word):
            build_norm_layer(bad, 8)


def test_multi_plane_switch_with_plain_ffn_or_norm_raises_by_name():
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    plain_ffn = dict(type='FFN', feedforward_channels=192, ffn_drop=0.1)
    for over in (dict(ffn_cfgs=plain_ffn), dict(norm_cfg=dict(type='LN')), dict(ffn_cfgs=plain_ffn, norm_cfg=dict(type='LN'))):
        with pytest.raises(ValueError, match='MultiPlaneFFN.*MultiPlaneNorm'):
            MODELS.build(_layer_cfg(**over))
    # the switch off: both module kinds still build (the reference would then fail in forward; so do we, elsewhere)
    assert not MODELS.build(_layer_cfg(multi_plane_ffn_norm=False, ffn_cfgs=plain_ffn, norm_cfg=dict(type='LN'))).multi_plane_ffn_norm


def test_row_sharding_is_refused_by_name():
    from selfocc_amd.registry import MODELS
    import selfocc_amd.model  # noqa: F401
    enc_cfg = copy.deepcopy(mpc.cfg()['encoder'])
    with pytest.raises(NotImplementedError, match='multi_plane_ffn_norm.*row_shard'):
        MODELS.build(dict(type='TPVFormerEncoder', row_shard=True, **enc_cfg))
    enc = MODELS.build(dict(type='TPVFormerEncoder', **enc_cfg))
    enc._row_sharding = lambda: True            # what SELFOCC_ENC_SHARD=1 with an initialised process group answers
    q = [torch.zeros(1, n, 96) for n in (625, 175, 175)]
    with pytest.raises(NotImplementedError, match='multi_plane_ffn_norm.*row sharding'):
        enc.forward_layers(q, None, None)


def test_multi_plane_modules_fall_back_to_the_per_plane_composition():
    """what the grouped kernel does not cover: CPU tensors (above), batch > 1, a width outside 4 .. 128, an eps per plane"""
    from selfocc_amd.model import bricks
    n0 = bricks.GROUPED_LN_CALLS[0]
    norm = bricks.MultiPlaneNorm(8)
    with torch.no_grad():
        for i, n in enumerate(norm.norms):
            n.weight.fill_(1.0 + i)
    tpv = [torch.randn(2, k, 8) for k in (5, 3, 1)]
    out = norm(tpv)
    for i, (o, t) in enumerate(zip(out, tpv)):
        assert torch.allclose(o, torch.nn.functional.layer_norm(t, (8,)) * (1.0 + i), atol=1e-6)
    cat = norm.forward_cat(torch.cat(tpv, 1), [5, 3, 1])
    assert torch.equal(cat, torch.cat(out, 1))
    ffn = bricks.MultiPlaneFFN(8, 16, num_fcs=3, act_cfg=dict(type='GELU')).eval()
    assert [o.shape for o in ffn(tpv)] == [t.shape for t in tpv]
    assert bricks.GROUPED_LN_CALLS[0] == n0


def _groups(n, starts):
    from selfocc_amd import abi
    g = abi.SoRowGroups()
    g.n_groups = n
    for i, s in enumerate(starts):
        g.row_start[i] = s
    return g


def test_grouped_layernorm_argument_checks_are_pure_host_logic():
    """T = 0: every bad table is refused with rc < 0 and a message before any HIP call (no GPU here)"""
    from selfocc_amd import abi
    from selfocc_amd._lib import lib
    l = lib()

    def fwd(T, Cc, g):
        return l.selfocc_layernorm_fwd_grouped(None, None, None, None, None, None, T, Cc, 1e-5, g, None)

    def bwd(T, Cc, g):
        return l.selfocc_layernorm_bwd_grouped(None, None, None, None, None, None, None, None, T, Cc, g, None, 0, None)

    def sup(T, Cc, g):
        return l.selfocc_layernorm_grouped_supported(T, Cc, g)

    bad = [
        (0, 96, _groups(3, [0, 5, 2, 0]), b'non-decreasing'),          # decreasing starts
        (0, 96, _groups(3, [0, 0, 0, 4]), b'must equal rows'),         # row_start[n] != T
        (0, 96, _groups(2, [1, 1, 0]), b'row_start[0]'),
        (0, 96, _groups(0, [0]), b'n_groups'),
        (0, 96, _groups(9, [0] * 9), b'n_groups'),
        (0, 98, _groups(3, [0, 0, 0, 0]), b'multiple of 4'),           # unsupported widths
        (0, 132, _groups(3, [0, 0, 0, 0]), b'multiple of 4'),
        (-1, 96, _groups(1, [0, -1]), b'rows'),
    ]
    for T, Cc, g, word in bad:
        for call in (fwd, bwd):
            rc = call(T, Cc, g)
            assert rc < 0 and word in l.selfocc_last_error(), (call.__name__, T, Cc, rc, l.selfocc_last_error())
    for T, Cc, g, word in bad[:5]:
        assert sup(T, Cc, g) < 0 and word in l.selfocc_last_error()
        assert l.selfocc_layernorm_bwd_grouped_workspace(T, Cc, g) == 0
    good = abi.SoRowGroups.from_sizes([66049, 6425, 6425])
    assert sup(78899, 96, good) == 1 and sup(78899, 98, good) == 0 and sup(78899, 256, good) == 0
    assert fwd(0, 96, _groups(3, [0, 0, 0, 0])) == 0                    # an empty tensor: nothing to launch
    # the workspace: one (2, C) partial per block, a group's blocks = what the ungrouped launch of its rows takes
    per = lambda r: min((r + 7) // 8, 2048)
    assert l.selfocc_layernorm_bwd_grouped_workspace(78899, 96, good) == (per(66049) + 2 * per(6425)) * 2 * 96 * 4
    assert l.selfocc_layernorm_bwd_grouped_workspace(78899, 96, abi.SoRowGroups.from_sizes([78899])) == \
        l.selfocc_layernorm_bwd_workspace(78899, 96)
    assert l.selfocc_layernorm_bwd_grouped_workspace(5, 96, abi.SoRowGroups.from_sizes([0, 5, 0])) == 1 * 2 * 96 * 4


def test_row_groups_struct_layout_matches_header(tmp_path):
    """so_row_groups is passed by value: sizeof / offsetof of the header through a compiled program against the ctypes mirror"""
    from selfocc_amd import abi
    src = tmp_path / "rg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s/include/selfocc_hip.h"\n'
                   'int main(void) { printf("%%zu %%zu %%zu %%zu\\n", sizeof(so_row_groups), offsetof(so_row_groups, n_groups), '
                   'offsetof(so_row_groups, row_start), sizeof(((so_row_groups *)0)->row_start)); return 0; }\n' % ROOT)
    exe = tmp_path / "rg"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    size, o_n, o_rs, s_rs = map(int, subprocess.check_output([str(exe)]).decode().split())
    assert (C.sizeof(abi.SoRowGroups), abi.SoRowGroups.n_groups.offset, abi.SoRowGroups.row_start.offset,
            abi.SoRowGroups.row_start.size) == (size, o_n, o_rs, s_rs) == (80, 0, 8, 72)
    g = abi.SoRowGroups.from_sizes([3, 0, 4])
    assert g.n_groups == 3 and list(g.row_start)[:4] == [0, 3, 3, 7]


def test_layernorm_kernels_with_row_groups_need_no_scratch():
    """the group table travels by value and is indexed with constants only: no scratch copy, the registers of the ungrouped
    kernels of the parent (36 / 54 / 14 VGPRs), full occupancy"""
    import kernel_report
    ks = {k.base: k.res for k in kernel_report.report('layernorm.hip')}
    assert set(ks) == {'layernorm_fwd_kernel', 'layernorm_bwd_kernel', 'layernorm_bwd_reduce_kernel'}, set(ks)
    for name, vgprs in (('layernorm_fwd_kernel', 36), ('layernorm_bwd_kernel', 54), ('layernorm_bwd_reduce_kernel', 14)):
        assert ks[name]['ScratchSize'] == 0 and ks[name]['VGPRs'] <= vgprs and ks[name]['Occupancy'] == 8, (name, ks[name])


def test_grouped_linear_argument_checks_are_pure_host_logic():
    """selfocc_linear_{fwd,dgrad,wgrad}_grouped with T = 0: every bad table, an unsupported N or K and a bad group stride give
    rc < 0 and a message before any HIP call (no GPU here); the support queries answer from host logic alone"""
    from selfocc_amd import abi
    from selfocc_amd._lib import lib
    l = lib()
    ok3 = _groups(3, [0, 0, 0, 0])

    def fwd(T, N, K, g, ws=None, ls=0):
        return l.selfocc_linear_fwd_grouped(None, None, None, None, 0, None, None, 0.0, None, N, None, None, None, T, N, K, 0, g,
                                            N * K if ws is None else ws, ls, None)

    def dgrad(T, N, K, g):
        return l.selfocc_linear_dgrad_grouped(None, None, None, T, N, K, g, None, 0, None)

    def wgrad(T, N, K, g):
        return l.selfocc_linear_wgrad_grouped(None, None, None, None, T, N, K, g, None, 0, None)

    tables = [(_groups(3, [0, 5, 2, 0]), b'non-decreasing'), (_groups(3, [0, 0, 0, 4]), b'must equal'),
              (_groups(0, [0]), b'n_groups'), (_groups(9, [0] * 9), b'n_groups'), (_groups(2, [1, 1, 0]), b'row_start[0]')]
    for call, sup in ((fwd, l.selfocc_linear_fwd_grouped_supported), (dgrad, l.selfocc_linear_dgrad_grouped_supported),
                      (wgrad, l.selfocc_linear_wgrad_grouped_supported)):
        for g, word in tables:
            rc = call(0, 192, 96, g)
            assert rc < 0 and word in l.selfocc_last_error(), (call.__name__, rc, l.selfocc_last_error())
            assert sup(0, 192, 96, g) < 0 and word in l.selfocc_last_error()
    for call, N, K in ((fwd, 192, 100), (fwd, 192, 256), (wgrad, 192, 100), (wgrad, 96, 48), (dgrad, 192, 64), (dgrad, 100, 96)):
        rc = call(0, N, K, ok3)
        assert rc < 0 and b'unsupported shape' in l.selfocc_last_error(), (call.__name__, N, K, rc, l.selfocc_last_error())
    assert fwd(0, 192, 96, ok3, ws=17) < 0 and b'w_group_stride' in l.selfocc_last_error()
    assert fwd(0, 96, 192, ok3, ls=5) < 0 and b'ln_group_stride' in l.selfocc_last_error()
    assert fwd(0, 192, 96, ok3) == 0 and fwd(0, 192, 96, ok3, ws=0) == 0 and dgrad(0, 192, 96, ok3) == 0      # empty: nothing to launch
    planes = abi.SoRowGroups.from_sizes([66049, 6425, 6425])
    for sup in (l.selfocc_linear_fwd_grouped_supported, l.selfocc_linear_dgrad_grouped_supported, l.selfocc_linear_wgrad_grouped_supported):
        assert sup(78899, 192, 96, planes) == 1 and sup(78899, 96, 192, planes) == 1
    assert l.selfocc_linear_fwd_grouped_supported(78899, 96, 100, planes) == 0
    assert l.selfocc_linear_dgrad_grouped_supported(78899, 64, 32, planes) == 0
    assert l.selfocc_linear_wgrad_grouped_supported(78899, 64, 48, planes) == 0
    # workspaces: every group's split planes of W^T; one (N K + N) partial per chunk, chunks never straddling a group
    assert l.selfocc_linear_dgrad_grouped_workspace(192, 96, planes) == 3 * l.selfocc_linear_dgrad_workspace(192, 96)
    one = abi.SoRowGroups.from_sizes([78899])
    assert l.selfocc_linear_wgrad_grouped_workspace(78899, 192, 96, one) == l.selfocc_linear_wgrad_workspace(78899, 192, 96)
    assert l.selfocc_linear_wgrad_grouped_workspace(78899, 192, 96, planes) >= l.selfocc_linear_wgrad_workspace(78899, 192, 96)
    assert l.selfocc_linear_wgrad_grouped_workspace(78899, 192, 96, _groups(3, [0, 5, 2, 0])) == 0


def test_group_table_unit_counts_at_the_group_edges():
    """the shared table builder through the workspace queries (host logic): one group takes the chunks of the ungrouped plan
    at row counts around the 64-row minimum of a chunk and at odd sizes; a group's LayerNorm blocks are what an ungrouped launch
    of its rows takes (an empty group none, 2 048 at the most)"""
    from selfocc_amd import abi
    from selfocc_amd._lib import lib
    l = lib()
    for T in (1, 63, 64, 65, 2467, 78899):
        for N, K in ((192, 96), (96, 192), (64, 32)):
            one = abi.SoRowGroups.from_sizes([T])
            want = l.selfocc_linear_wgrad_workspace(T, N, K)
            assert want > 0 and l.selfocc_linear_wgrad_grouped_workspace(T, N, K, one) == want, (T, N, K)
    per = lambda r: min((r + 7) // 8, 2048)
    for sizes in ((0, 5, 0), (8, 9, 16385), (66049, 6425, 6425)):
        got = l.selfocc_layernorm_bwd_grouped_workspace(sum(sizes), 96, abi.SoRowGroups.from_sizes(list(sizes)))
        assert got == sum(per(r) for r in sizes) * 2 * 96 * 4, (sizes, got)


def test_grouped_linear_kernels_need_no_more_scratch_than_their_ungrouped_twins():
    """-Rpass-analysis=kernel-resource-usage: every grouped instantiation (last template argument true) against the ungrouped
    one with the same other arguments"""
    import kernel_report
    n = 0
    for src in ('linear_fwd.hip', 'linear.hip'):
        ks = kernel_report.report(src)
        twins = {k.name: k.res for k in ks}
        for k in ks:
            if k.name.rstrip('>').rstrip().endswith('true') or ', true>(' in k.name or ',true>(' in k.name:
                other = k.name.replace(', true>', ', false>').replace('<true>', '<false>')
                assert other in twins and other != k.name, k.name
                assert k.res['ScratchSize'] <= twins[other]['ScratchSize'], (k.name, k.res, twins[other])
                n += 1
    assert n >= 20, n
