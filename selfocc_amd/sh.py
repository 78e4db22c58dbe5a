"""Spherical-harmonics colour, host side: the real basis of degrees 0 - 2 in the order, signs and normalisation the render
kernels use (csrc/sh_device.h; contract in include/selfocc_hip.h above ``so_render_args``).

The kernels evaluate the basis themselves, once per ray; this mirror exists for tests, fixtures and synthetic scenes.
Written from the closed forms of the real spherical harmonics Y_l^m on the unit sphere, listed per degree in the order
m = -l .. l, with the sign convention of the reference (model/head/utils/sh_render.py): odd-m terms carry (-1)^m.
"""
import math

import torch

SH_ACTS = ('relu', 'sigmoid')
MAX_SH_DEG = 2


def n_basis(deg):
    return (deg + 1) ** 2


def n_coef(deg):
    """colour channels of a degree-``deg`` head: 3 colours x (deg + 1)^2 basis functions, colour-major"""
    return 3 * n_basis(deg)


def feat_stride(deg):
    """floats per voxel row of the coefficient volume: ``n_coef`` rounded up to a multiple of 4 (16-byte loads)"""
    return (n_coef(deg) + 3) // 4 * 4


def check(deg, act):
    if deg not in range(MAX_SH_DEG + 1):
        raise ValueError(f"sh_deg={deg} is not built: the render kernels implement sh_deg 0, 1 and 2")
    if act not in SH_ACTS:
        raise ValueError(f"sh_act={act!r} is not built: the render kernels implement 'relu' and 'sigmoid'")


def sh_basis(deg, dirs):
    """dirs (..., 3) unit vectors (x, y, z) -> (..., (deg + 1)^2) basis values, in the dtype of ``dirs``."""
    check(deg, 'relu')
    x, y, z = dirs.unbind(-1)
    k0 = 0.5 / math.sqrt(math.pi)                       # Y_0^0
    out = [torch.full_like(x, k0)]
    if deg >= 1:
        k1 = math.sqrt(3.0 / (4.0 * math.pi))           # Y_1^{-1, 0, 1} = k1 * (y, z, x), odd m negated
        out += [-k1 * y, k1 * z, -k1 * x]
    if deg >= 2:
        ka = 0.5 * math.sqrt(15.0 / math.pi)            # Y_2^{-2}, Y_2^{-1}, Y_2^{1}: ka * (xy, yz, xz)
        kb = 0.25 * math.sqrt(5.0 / math.pi)            # Y_2^0 = kb * (3 z^2 - 1) = kb * (2 z^2 - x^2 - y^2)
        kc = 0.25 * math.sqrt(15.0 / math.pi)           # Y_2^2 = kc * (x^2 - y^2)
        out += [ka * (x * y), -ka * (y * z), kb * (2.0 * z * z - x * x - y * y), -ka * (x * z), kc * (x * x - y * y)]
    return torch.stack(out, -1)


def sh_colour(deg, act, dirs, feats):
    """The per-sample colour of the contract: feats (..., >= n_coef) interpolated channels (colour-major), dirs (..., 3)
    broadcastable against feats' leading shape -> (..., 3) = act(sum_k Y_k(dir) * f[c, k])."""
    check(deg, act)
    nb = n_basis(deg)
    f = feats[..., :3 * nb].reshape(*feats.shape[:-1], 3, nb)
    raw = (sh_basis(deg, dirs).unsqueeze(-2) * f).sum(-1)
    return torch.relu(raw + 0.5) if act == 'relu' else torch.sigmoid(raw)
