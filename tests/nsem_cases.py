"""Shared by tests/test_render_nsem_cpu.py and tests/test_render_nsem_gpu.py: volumes with any class count whose PAD channels
hold 64.0 (the `_exact_volume` precedent of tests/test_occ_gpu.py: the logits are N(0, 1), so a pad channel that leaked into
a soft-max would take all of it)."""
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd.render import SDFVolume

PAD = 64.0
# pad sizes 0 - 3 and both ends of every row width: 2 / 4 -> 8 floats, 6 -> 12, 11 -> 16, 16 / 17 -> 20, 20 -> 24
CLASS_COUNTS = (2, 4, 6, 11, 16, 17, 20)
CONTROLS = (5, 21)                      # rows without a pad channel: the kernels every earlier version ran


def stride(n_sem):
    return (3 + n_sem + 3) & ~3


def fill_pad(vol, value=PAD):
    """the same volume with every pad channel overwritten"""
    feat = vol.feat.clone()
    feat[..., 3 + vol.n_sem:] = value
    return vol.with_tensors(vol.sdf, feat)


def volume(name, n_sem, seed=0, pad=PAD, **kw):
    vol = sy.make_volume(name, n_rgb=3, n_sem=n_sem, seed=seed, **kw)
    assert vol.feat.shape[-1] == stride(n_sem) == SDFVolume.feat_width(3, n_sem)
    return fill_pad(vol, pad)
