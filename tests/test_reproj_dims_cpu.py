"""CPU: the host side of the channel-last reprojection entries (selfocc_reproj_c_fwd / _bwd, csrc/reproj.hip) and of the losses' ``dims``
knob: struct layout, every refusal before any device is touched, the loss classes' argument errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from selfocc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of every field of so_reproj_c_args, from a C program compiled against the header"""
    names = [f for f, _ in abi.SoReprojCArgs._fields_]
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_reproj_c_args), offsetof(so_reproj_c_args, {f}));' for f in names)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split()
    assert len(lines) == 2 * len(names)
    for i, f in enumerate(names):
        assert int(lines[2 * i]) == C.sizeof(abi.SoReprojCArgs), f
        assert int(lines[2 * i + 1]) == getattr(abi.SoReprojCArgs, f).offset, f


def _args(**kw):
    """a valid argument set on HOST memory: never dereferenced, every call below fails its checks first or has R == 0"""
    buf = C.create_string_buffer(256 + 16)
    base = (C.addressof(buf) + 15) & ~15            # 16-byte aligned, like an image base
    a = abi.SoReprojCArgs()
    a.keep = buf
    for f in ("weights", "ts", "deltas", "pix", "curr", "T_prev", "T_next", "img_prev", "img_next", "l1", "combine",
              "any_valid"):
        setattr(a, f, base)
    a.R, a.S, a.Hi, a.Wi, a.C, a.img_stride = 4, 12, 6, 10, 5, 8
    a.img_h, a.img_w = 48.0, 100.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a, base


REFUSALS = [
    (dict(C=0), b"1 <= C <= 512"), (dict(C=513, img_stride=516), b"1 <= C <= 512"),
    (dict(img_stride=4), b"img_stride"), (dict(img_stride=6), b"img_stride"), (dict(img_stride=7), b"img_stride"),
    (dict(S=0), b"1 <= S <= 512"), (dict(S=513), b"1 <= S <= 512"),
    (dict(R=-1), b"R >= 0"),
    (dict(weights=None), b"NULL"), (dict(ts=None), b"NULL"), (dict(pix=None), b"NULL"), (dict(curr=None), b"NULL"),
    (dict(T_prev=None), b"NULL"), (dict(T_next=None), b"NULL"), (dict(img_prev=None), b"NULL"), (dict(img_next=None), b"NULL"),
    (dict(Hi=0), b"image size"), (dict(Wi=0), b"image size"), (dict(img_h=0.0), b"image size"), (dict(img_w=-1.0), b"image size"),
    (dict(Wi=(1 << 24) + 1), b"image size"),
]


@pytest.mark.parametrize("bwd", [False, True])
def test_every_refusal_is_host_logic(bwd):
    """< 0 and the key word in selfocc_last_error(), forward and backward, with pointers no device could read"""
    from selfocc_amd._lib import lib
    l = lib()

    def call(a, base, g_weights="same"):
        if bwd:
            return l.selfocc_reproj_c_bwd(a, base, base, base if g_weights == "same" else g_weights, None)
        return l.selfocc_reproj_c_fwd(a, None)

    for kw, word in REFUSALS:
        a, base = _args(**kw)
        rc = call(a, base)
        assert rc < 0 and word in l.selfocc_last_error(), (kw, rc, l.selfocc_last_error())
    a, base = _args()
    a.img_prev = base + 4                                            # an image base off the 16-byte grid
    assert call(a, base) < 0 and b"16-byte aligned" in l.selfocc_last_error()
    assert (l.selfocc_reproj_c_bwd if bwd else l.selfocc_reproj_c_fwd)(None, *((None,) * (4 if bwd else 1))) < 0
    if bwd:
        a, base = _args()
        assert call(a, base, g_weights=None) < 0 and b"g_weights" in l.selfocc_last_error()


def test_empty_ray_set_succeeds_without_a_launch():
    from selfocc_amd._lib import lib
    l = lib()
    a, base = _args(R=0)
    assert l.selfocc_reproj_c_fwd(a, None) == 0
    assert l.selfocc_reproj_c_bwd(a, base, base, base, None) == 0
    a, base = _args(R=0, weights=None, img_prev=None)                # nothing is read: an empty tensor has no address
    assert l.selfocc_reproj_c_fwd(a, None) == 0
    assert l.selfocc_reproj_c_bwd(a, None, None, None, None) == 0
    a, base = _args(R=0, C=0)                                        # the scalar checks still hold
    assert l.selfocc_reproj_c_fwd(a, None) < 0


def _loss_inputs(chans, R=6, S=4, cams=2, hw=(5, 7)):
    g = torch.Generator().manual_seed(0)
    img = lambda c: torch.rand(1, cams, c, *hw, generator=g)
    eye = np.stack([np.eye(4)] * cams)
    return dict(curr_imgs=img(chans[0]), prev_imgs=img(chans[1]), next_imgs=img(chans[2]),
                ray_indices=[torch.arange(R).repeat_interleave(S)] * cams,
                weights=[torch.rand(R * S, generator=g) for _ in range(cams)],
                ts=[torch.rand(R * S, generator=g) + 1 for _ in range(cams)],
                metas=[dict(img2prevImg=eye, img2nextImg=eye)], ms_rays=torch.rand(R, 2, generator=g) * 5)


KEYS = dict(curr_imgs='curr_imgs', prev_imgs='prev_imgs', next_imgs='next_imgs', ray_indices='ray_indices',
            weights='weights', ts='ts', metas='metas', ms_rays='ms_rays')


@pytest.mark.parametrize("cls", ['ReprojLossMonoMultiNewCombine', 'ReprojLossMonoMultiNew'])
@pytest.mark.parametrize("dims,chans", [(3, (5, 5, 5)), (5, (3, 3, 3)), (5, (5, 5, 4)), (5, (5, 3, 5)), (16, (5, 16, 16)),
                                        (3, (3, 3, 1))])
def test_dims_channel_mismatch_is_a_value_error(cls, dims, chans):
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    lossf = OPENOCC_LOSS.build(dict(type=cls, weight=1.0, input_dict=KEYS, img_size=[5, 7], no_ssim=True, dims=dims))
    with pytest.raises(ValueError) as e:
        lossf(_loss_inputs(chans))
    msg = str(e.value)
    assert "dims" in msg and str((1, 2, chans[0], 5, 7)) in msg and str((1, 2, chans[2], 5, 7)) in msg, msg


@pytest.mark.parametrize("cls", ['ReprojLossMonoMultiNewCombine', 'ReprojLossMonoMultiNew'])
def test_ray_shard_with_other_dims_is_refused_by_name(cls):
    from selfocc_amd.dist import LocalRows
    from selfocc_amd.registry import OPENOCC_LOSS
    import selfocc_amd.loss  # noqa: F401
    lossf = OPENOCC_LOSS.build(dict(type=cls, weight=1.0, input_dict=KEYS, img_size=[5, 7], no_ssim=True, dims=5))
    inp = _loss_inputs((5, 5, 5))
    inp['weights'] = LocalRows(inp['weights'], shard=object())      # refused before the shard is looked at
    with pytest.raises(NotImplementedError) as e:
        lossf(inp)
    assert "dims=5" in str(e.value) and "ray-sharded" in str(e.value)


def test_dims_three_construction_is_unchanged():
    from selfocc_amd.loss.reproj import ReprojLossMonoMultiNew, ReprojLossMonoMultiNewCombine, _ReprojBase
    from selfocc_amd.reproj import ReprojSampleCFunction, ReprojSampleFunction, channel_last
    for cls in (ReprojLossMonoMultiNewCombine, ReprojLossMonoMultiNew):
        a, b = cls(img_size=[5, 7], ray_resize=[2, 3]), cls(img_size=[5, 7], ray_resize=[2, 3], dims=3)
        assert a.dims == b.dims == 3 and a.no_ssim == b.no_ssim is False and a.input_dict == b.input_dict
        assert cls(img_size=[5, 7], dims=16).dims == 16
        img = torch.rand(1, 2, 3, 5, 7)
        fn, as_image = a._sampler(img, img, img, None)
        one = img[0, 0]
        assert fn is ReprojSampleFunction and as_image(one) is one                        # the image itself, no copy
        fn, as_image = a._sampler(img, img, img, object())                                # sharding stays available at 3
        assert fn is ReprojSampleFunction
        f16 = torch.rand(1, 2, 16, 5, 7)
        fn, as_image = cls(img_size=[5, 7], dims=16)._sampler(f16, f16, f16, None)
        assert fn is ReprojSampleCFunction and as_image is channel_last
    assert _ReprojBase.supports_ray_shard


def test_channel_last_pads_the_pixel_stride_in_one_copy():
    from selfocc_amd.reproj import ChannelLastImage, channel_last
    for c, stride in ((1, 4), (3, 4), (4, 4), (5, 8), (16, 16), (99, 100)):
        img = torch.rand(2 * c, 5, 7)[::2]                           # a non-contiguous (C, Hi, Wi) view
        cl = channel_last(img)
        assert isinstance(cl, ChannelLastImage) and cl.C == c and cl.data.shape == (5, 7, stride)
        assert cl.data.is_contiguous() and cl.data.dtype == torch.float32 and cl.data.data_ptr() % 16 == 0
        assert torch.equal(cl.data[..., :c], img.permute(1, 2, 0))
        assert channel_last(cl) is cl
    with pytest.raises(ValueError):
        ChannelLastImage(torch.zeros(5, 7, 6), 5)
    with pytest.raises(ValueError):
        ChannelLastImage(torch.zeros(5, 7, 8), 9)
