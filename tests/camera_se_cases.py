"""Seeded inputs of the CameraAwareSE fixture (tests/golden/make_golden_camera_se.py) and of its tests: parameters,
BatchNorm statistics, camera metas, FPN maps and upstream gradients.  Everything is drawn in float64 from a CPU
torch.Generator and rounded to float32 once, so that the float64 reruns see exactly the float32 inputs.

The module's parameters are NOT the reference's init_weight() (fc2.bias = 10 opens the gate to 0.99995 and makes a test blind
to it), and the BatchNorm1d running statistics are of realistic size (focal lengths are ~1e3: with the default 0 / 1
statistics the eval-mode MLP saturates)."""
import glob
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# (name, in_channels = out_channels, mid_channels, cameras, levels); B = 1
CASES = {
    'c96m96': (96, 96, 6, ((4, 7), (2, 3), (1, 2))),
    'c96m192': (96, 192, 6, ((4, 7), (2, 3), (1, 2))),
    'enc32': (32, 32, 3, ((8, 8), (4, 4))),
}
SEEDS = {'c96m96': 9601, 'c96m192': 9602, 'enc32': 3201}

# typical nuScenes calibration: fx, fy, cx, cy, then cam2ego[:3, :] row by row (three rotation entries and one translation)
CAM_MEAN = [1260.0, 1260.0, 800.0, 450.0] + [0.0, 0.0, 0.0, 0.8, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5]
CAM_VAR = [900.0, 900.0, 400.0, 225.0] + [0.4, 0.4, 0.4, 1.0] * 3


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def seed_module(mod, seed):
    """Fill every parameter and buffer of a CameraAwareSE (the reference's or this project's: same names) in sorted-name order."""
    g = torch.Generator().manual_seed(seed)
    sd = mod.state_dict()
    new = {}
    for name in sorted(sd):
        t = sd[name]
        if name.endswith('num_batches_tracked'):
            new[name] = torch.zeros_like(t)
        elif name == 'bn.running_mean':
            v = torch.tensor(CAM_MEAN, dtype=torch.float64) + 0.05 * torch.tensor(CAM_VAR, dtype=torch.float64).sqrt() * _randn(g, 16)
        elif name == 'bn.running_var':
            v = torch.tensor(CAM_VAR, dtype=torch.float64) * (0.75 + 0.5 * torch.rand(16, generator=g, dtype=torch.float64))
        elif name.endswith('running_mean'):
            v = 0.1 * _randn(g, *t.shape)
        elif name.endswith('running_var'):
            v = 0.5 + torch.rand(*t.shape, generator=g, dtype=torch.float64)
        elif name in ('bn.weight', 'reduce_conv.1.weight'):
            v = 1.0 + 0.1 * _randn(g, *t.shape)
        elif t.dim() > 1:
            v = _randn(g, *t.shape) / float(t[0].numel()) ** 0.5
        else:
            v = 0.1 * _randn(g, *t.shape)
        if not name.endswith('num_batches_tracked'):
            new[name] = v.to(t.dtype)
    mod.load_state_dict(new, strict=True)
    return mod


def make_metas(seed, B, N, size=4):
    """`intrinsic` (size x size) and `cam2ego` (4 x 4) per camera: a ring of cameras with seeded scatter."""
    g = torch.Generator().manual_seed(seed + 17)
    metas = []
    for b in range(B):
        Ks, Es = [], []
        for n in range(N):
            r = _randn(g, 8).tolist()
            K = np.eye(size)
            K[0, 0] = 1260.0 + 30.0 * r[0]
            K[1, 1] = K[0, 0] + 3.0 * r[1]
            K[0, 2] = 800.0 + 20.0 * r[2]
            K[1, 2] = 450.0 + 15.0 * r[3]
            yaw = 2.0 * np.pi * n / N + 0.05 * r[4]
            E = np.eye(4)
            E[:3, :3] = np.array([[np.cos(yaw), 0.0, np.sin(yaw)], [np.sin(yaw), 0.0, -np.cos(yaw)], [0.0, 1.0, 0.0]])   # camera z forward, y down
            E[:3, 3] = [0.8 + 0.9 * r[5], 0.5 * r[6], 1.5 + 0.1 * r[7]]
            Ks.append(K.astype(np.float32))
            Es.append(E.astype(np.float32))
        metas.append({'intrinsic': Ks, 'cam2ego': Es})
    return metas


def make_maps(seed, B, N, C, levels):
    g = torch.Generator().manual_seed(seed + 31)
    maps = [_randn(g, B, N, C, h, w).float() for h, w in levels]
    ups = [_randn(g, B, N, C, h, w).float() for h, w in levels]
    return maps, ups


def case_inputs(name):
    C, M, N, levels = CASES[name]
    seed = SEEDS[name]
    maps, ups = make_maps(seed, 1, N, C, levels)
    return dict(C=C, M=M, N=N, levels=levels, seed=seed, maps=maps, ups=ups, metas=make_metas(seed, 1, N))


def checks(mod, inp):
    """float64 sums of the seeded inputs: the fixture stores them, the tests compare (a changed torch RNG shows here)."""
    sd = mod.state_dict()
    return {
        'check.params': np.array([sum(float(sd[k].double().sum()) for k in sorted(sd))]),
        'check.maps': np.array([float(m.double().sum()) for m in inp['maps']]),
        'check.ups': np.array([float(u.double().sum()) for u in inp['ups']]),
        'check.metas': np.array([sum(float(np.asarray(m[k], dtype=np.float64).sum()) for m in inp['metas'] for k in ('intrinsic', 'cam2ego'))]),
    }


def load_fixture():
    """All camera_se*.npz files of tests/golden as one dict (the data is split so that every file stays under 1 MiB)."""
    z = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'camera_se*.npz'))):
        with np.load(path) as f:
            for k in f.files:
                assert k not in z, k
                z[k] = f[k]
    return z


def sha256(path):
    return hashlib.sha256(open(path, 'rb').read()).hexdigest()
