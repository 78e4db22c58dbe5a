"""Generate tests/golden/sh.npz by running the REAL reference ``eval_sh_bases`` / ``SHRender``
(model/head/utils/sh_render.py, loaded by file path from the read-only reference tree): the spherical-harmonics
basis of degrees 0 - 2 at ~200 unit directions and the rendered colour of random features for every
(degree, activation) the render kernels implement.  Data only: nothing of the reference's text is written.

Run:  python tests/golden/make_golden_sh.py        (needs the reference tree; < 1 s)
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402


def directions(n_random=160, seed=20240607):
    axes = torch.eye(3, dtype=torch.float64)
    d = [axes, -axes]
    s = torch.tensor([[sx, sy, sz] for sx in (-1., 1.) for sy in (-1., 1.) for sz in (-1., 1.)], dtype=torch.float64)
    d.append(s)                                                                   # 8 body diagonals
    f = torch.tensor([[1., 1., 0.], [1., -1., 0.], [1., 0., 1.], [1., 0., -1.], [0., 1., 1.], [0., 1., -1.]], dtype=torch.float64)
    d += [f, -f]                                                                  # 12 face diagonals
    g = torch.Generator().manual_seed(seed)
    d.append(torch.randn(n_random, 3, generator=g, dtype=torch.float64))
    d = torch.cat(d)
    return d / d.norm(dim=-1, keepdim=True)


def main():
    assert os.path.isdir(REF), f"{REF} not found: golden vectors can only be regenerated where the reference is mounted"
    spec = importlib.util.spec_from_file_location('ref_sh_render', os.path.join(REF, 'model', 'head', 'utils', 'sh_render.py'))
    shr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shr)
    dirs64 = directions()
    dirs = dirs64.float()
    out = {'dirs': dirs.numpy(), 'dirs64': dirs64.numpy()}
    g = torch.Generator().manual_seed(7)
    for deg in (0, 1, 2):
        out[f'basis.{deg}'] = shr.eval_sh_bases(deg, dirs).numpy()
        out[f'basis64.{deg}'] = shr.eval_sh_bases(deg, dirs64).numpy()
        feat = torch.randn(dirs.shape[0], 3 * (deg + 1) ** 2, generator=g)
        out[f'feat.{deg}'] = feat.numpy()
        for act in ('relu', 'sigmoid'):
            out[f'rgb.{deg}.{act}'] = shr.SHRender(None, dirs, feat, deg=deg, act=act).numpy()
    path = os.path.join(HERE, 'sh.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', dirs.shape[0], 'directions')


if __name__ == '__main__':
    main()
