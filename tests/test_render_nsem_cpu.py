"""CPU: any semantic class count from 2 to 21 — the row-width table, the host-only accept / refuse list of the
C boundary, the backward workspace size, the construction rules of SDFField, the compiler's scratch report of the new
forward kernels, and the oracle's indifference to what the pad channels hold."""
import shutil

import pytest
import torch

import oracle
from selfocc_amd import abi, synthetic as sy
from selfocc_amd.render import SDFVolume
from nsem_cases import CLASS_COUNTS, CONTROLS, stride, volume
from kernel_report import HIPCC, kernels_of
from test_sh_cpu import SMALL_MAPPING, _args


def test_feat_width_is_the_row_rounded_up_to_four_floats():
    assert SDFVolume.feat_width(0, 0) == 0
    want = {0: 4, 1: 4, 2: 8, 3: 8, 4: 8, 5: 8, 6: 12, 7: 12, 8: 12, 9: 12, 10: 16, 11: 16, 12: 16, 13: 16, 14: 20, 15: 20,
            16: 20, 17: 20, 18: 24, 19: 24, 20: 24, 21: 24}
    assert {n: SDFVolume.feat_width(3, n) for n in range(22)} == want
    assert all(stride(n) == want[n] for n in range(2, 22))
    for n in CLASS_COUNTS + CONTROLS:
        v = sy.make_volume("cfg1", n_rgb=3, n_sem=n, seed=1)
        assert v.feat.shape[-1] == want[n] and v.feat[..., 3 + n:].abs().sum().item() == 0.0
        assert v.feat[..., 3 + n - 1].abs().max().item() > 0.0


def _both(l, kw):
    rc_f = l.selfocc_render_fwd(_args(**kw), None)
    err_f = l.selfocc_last_error()
    ba = abi.SoRenderBwdArgs()
    ba.fwd = _args(**kw)
    rc_b = l.selfocc_render_bwd(ba, None)
    return rc_f, err_f, rc_b, l.selfocc_last_error()


def test_class_count_argument_checks_are_pure_host_logic():
    """n_rays = 0: so_validate_render decides before any HIP call.  Built: n_sem 0 and 2 .. 21 at feat_stride = 3 + n_sem rounded
    up to 4, float32; bfloat16 at 21 classes only.  Everything else is refused by name."""
    from selfocc_amd._lib import lib
    l = lib()
    for n in range(2, 22):
        rc_f, err, rc_b, err_b = _both(l, dict(n_sem=n, feat_stride=stride(n)))
        assert rc_f == 0 and rc_b == 0, (n, err, err_b)
    assert _both(l, dict(n_sem=21, feat_stride=24, feat_dtype=abi.DTYPE_BF16))[::2] == (0, 0)
    bad = [
        (dict(n_sem=1, feat_stride=4), b"n_sem = 1"),
        (dict(n_sem=1, feat_stride=8), b"n_sem = 1"),
        (dict(n_sem=22, feat_stride=28), b"24 channels"),
        (dict(n_sem=29, feat_stride=32), b"24 channels"),
        (dict(n_sem=61, feat_stride=64), b"n_sem = 61"),
        (dict(n_sem=20, feat_stride=28), b"feat_stride"),     # a multiple of 4 that holds the row, but not THE stride
        (dict(n_sem=4, feat_stride=12), b"feat_stride"),
        (dict(n_sem=6, feat_stride=8), b"feat_stride"),
        (dict(n_sem=5, feat_stride=12), b"feat_stride"),
        (dict(n_sem=20, feat_stride=23), b"feat_stride"),
        (dict(n_sem=20, feat_stride=24, feat_dtype=abi.DTYPE_BF16), b"bfloat16"),
        (dict(n_sem=5, feat_stride=8, feat_dtype=abi.DTYPE_BF16), b"bfloat16"),
        (dict(n_sem=17, feat_stride=20, feat_dtype=abi.DTYPE_BF16), b"bfloat16"),
        (dict(n_sem=20, feat_stride=24, sh_act=abi.SH_SIGMOID), b"n_sem"),
        (dict(n_sem=11, feat_stride=28, sh_deg=2), b"n_sem"),
    ]
    for kw, word in bad:
        rc_f, err_f, rc_b, err_b = _both(l, kw)
        assert rc_f < 0 and word in err_f, (kw, err_f)
        assert rc_b < 0 and word in err_b, (kw, err_b)


def test_backward_workspace_answers_for_every_built_class_count():
    """rows of up to 8 floats bin into the 64-byte record, wider rows into the 128-byte one; a class count that is not built gets 0"""
    from selfocc_amd._lib import lib
    l = lib()
    ba = abi.SoRenderBwdArgs()
    for ax, n in ((ba.fwd.map.h, 257), (ba.fwd.map.w, 257), (ba.fwd.map.d, 25)):
        ax.tot_len = n
    ba.fwd.n_rays, ba.fwd.n_samples, ba.fwd.n_rgb = 2048, 256, 3
    total = 2048 * 256
    for n in range(2, 22):
        ba.fwd.n_sem, ba.fwd.feat_stride = n, stride(n)
        ws = l.selfocc_render_bwd_ws_bytes(ba)
        rec = 64 if stride(n) == 8 else 128
        assert total * rec <= ws <= total * rec + (8 << 20) and ws % 256 == 0, (n, ws)
    for n in (1, 22, 40):
        ba.fwd.n_sem, ba.fwd.feat_stride = n, stride(n)
        assert l.selfocc_render_bwd_ws_bytes(ba) == 0, n


def _field(color_dims, **kw):
    from selfocc_amd.model.head.neus_head import SDFField
    return SDFField(SMALL_MAPPING, embed_dims=16, color_dims=color_dims, density_layers=2, sh_deg=0, tpv=True, **kw)


def test_sdf_field_builds_padded_rows_and_refuses_unbuilt_class_counts_by_name():
    f = _field(23)                                    # SemanticKITTI: 20 classes
    assert (f.n_rgb, f.n_sem, f._feat_width()) == (3, 20, 24) and f.density_net[-1].out_features == 24
    H, W, D = f.size_h, f.size_w, f.size_d
    g = torch.Generator().manual_seed(0)
    rep = (torch.randn(1, H * W, 16, generator=g), torch.randn(1, D * H, 16, generator=g), torch.randn(1, W * D, 16, generator=g))
    with torch.no_grad():
        vol = f.pre_compute_density_color(rep)
    assert tuple(vol.feat.shape) == (H, W, D, 24) and (vol.n_rgb, vol.n_sem) == (3, 20)
    assert vol.feat[..., 23].abs().max().item() == 0.0 and vol.feat[..., 22].abs().max().item() > 0.0
    for color_dims, n_sem, F in ((20, 17, 20), (21, 18, 24), (22, 19, 24), (5, 2, 8), (9, 6, 12)):
        f = _field(color_dims)
        assert (f.n_sem, f._feat_width()) == (n_sem, F)
    with pytest.raises(NotImplementedError, match="n_sem=1 "):
        _field(4)
    with pytest.raises(NotImplementedError, match="n_sem=22 "):
        _field(25)
    with pytest.raises(NotImplementedError, match="n_sem=61 "):
        _field(64)


def test_volume_round_trips_through_the_reference_layout_at_20_classes():
    v = sy.make_volume("cfg1", n_rgb=3, n_sem=20, seed=5)
    ref = v.to_reference_layout()
    assert tuple(ref.shape) == (1, 24, *v.sdf.shape)                      # sdf + 3 + 20: the reference has no pad
    back = SDFVolume.from_reference_layout(v.mapping, ref, n_rgb=3, n_sem=20)
    assert tuple(back.feat.shape[-1:]) == (24,) and torch.equal(back.sdf, v.sdf) and torch.equal(back.feat, v.feat)
    assert torch.equal(volume("cfg1", 20, seed=5).to_reference_layout(), ref)   # whatever the pad holds


def test_marshalling_allocates_sem_without_the_pad():
    from selfocc_amd.render import marshal_render_args
    rays = sy.explicit_rays(sy.make_rays("cfg1"))
    a, out, _ = marshal_render_args(volume("cfg1", 17), rays, sy.make_render_config("cfg1"))
    assert (a.n_sem, a.feat_stride) == (17, 20) and tuple(out['sem'].shape) == (rays.n_rays, 17)


@pytest.mark.parametrize("n_sem", CLASS_COUNTS)
def test_the_oracle_ignores_the_pad_channels(n_sem):
    """the reference of the GPU tests, bit for bit the same with 0 and with 64 in the pad"""
    rays = sy.make_rays("cfg1", seed=3)
    cfg = sy.make_render_config("cfg1", inv_s=20.0)
    a = oracle.render_fwd(volume("cfg1", n_sem, seed=3, pad=0.0), rays, cfg, per_sample=True)
    b = oracle.render_fwd(volume("cfg1", n_sem, seed=3), rays, cfg, per_sample=True)
    assert tuple(a['sem'].shape) == (rays.n_rays, n_sem)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert (a['sem'].sum(-1) - a['acc']).abs().max() <= 5e-5


# ---- compiler report: the new forward kernels keep nothing in scratch -----------------------------------------------------------
@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not present")
@pytest.mark.parametrize("src,base,count", [("render_fwd.hip", "render_fwd_explicit", 15), ("render_fwd.hip", "render_fwd_pixgrid", 15),
                                            ("render_train.hip", "render_fwd_samples_kernel", 30)],
                         # the ids these cases have always had: the names of the kernels before they became instances of `base`
                         ids=["render_fwd.hip-render_ns_explicit-15", "render_fwd.hip-render_ns_pixgrid-15",
                              "render_train.hip-render_ns_samples_kernel-30"])
def test_masked_forward_kernels_use_no_scratch(src, base, count):
    """eval forward: 5 row widths x (canonical, canonical under 'linear_upscale', fast face-safe), explicit rays and pixel grid;
    training forward: 5 row widths x 3 waves-per-ray forms x 2 mapping kinds"""
    hits = kernels_of(src, base, lambda r: r.masked)
    assert len(hits) == count, [k.name for k in hits]
    assert sorted({k.row.nf for k in hits}) == [8, 12, 16, 20, 24] and not any(k.row.bf16 or k.row.nb for k in hits)
    for k in hits:
        assert k.res["ScratchSize"] == 0, k
        assert k.res["VGPRs"] + k.res.get("AGPRs", 0) <= 256, k
