"""Generate tests/golden/camera_se*.npz + camera_se_cfg.json by running the REAL reference ``CameraAwareSE``
(model/encoder/tpvformer/modules/camera_se_net.py, loaded by file path from the read-only reference tree) on the seeded
inputs of tests/camera_se_cases.py.  Data only: nothing of the reference's text is written.

Per case (c96m96, c96m192: B 1, N 6, levels 4x7 / 2x3 / 1x2; enc32: N 3, levels 8x8 / 4x4, maps and metas stored too) and
mode (train / eval), all from the real class in float32:
    <case>.<mode>.out.<l>              the module's output maps (B, N, C, h, w)
    <case>.<mode>.grad.map.<l>         gradient of sum_l (out_l * up_l).sum() w.r.t. the input maps
    <case>.<mode>.grad.<parameter>     ... w.r.t. every parameter
    <case>.train.buf.<buffer>          the BatchNorm buffers after the training-mode call
    <case>.<mode>.spread.<name>        ONE scalar per tensor above: max |float32 - float64| / max |float64| of the same class
                                       run in float64 on the same inputs (the reference's own rounding noise); for
                                       grad.reduce_conv.0.bias in training mode (mathematically zero: a bias in front of a
                                       BatchNorm) relative to the scale of grad.reduce_conv.0.weight
    <case>.check.*                     float64 sums of the seeded inputs
The data is split over four files so that each stays under 1 MiB: camera_se.npz (c96m96, enc32), camera_se_wide.npz (c96m192
without the two gradients of the 3x3 reduce_conv weight, 650 KB each), camera_se_wide_rc_train.npz / _rc_eval.npz (those).
Archive members carry a fixed timestamp: the files regenerate bit for bit.

Run:  python tests/golden/make_golden_camera_se.py        (needs the reference tree; a few seconds)
"""
import importlib.util
import io
import json
import os
import sys
import zipfile

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
import camera_se_cases as cases  # noqa: E402


def write_npz(path, arrs):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(path, os.path.getsize(path), 'bytes,', len(arrs), 'arrays')


def run(mod, inp, dtype, train):
    mod = mod.to(dtype).train(train)
    maps = [m.to(dtype).requires_grad_(True) for m in inp['maps']]
    outs = mod(maps, inp['metas'])
    loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs, inp['ups']))
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(loss, maps + list(params.values()))
    res = {}
    for l, o in enumerate(outs):
        res[f'out.{l}'] = o.detach()
    for l in range(len(maps)):
        res[f'grad.map.{l}'] = grads[l]
    for name, gr in zip(params, grads[len(maps):]):
        res[f'grad.{name}'] = gr
    if train:
        for name, b in mod.named_buffers():
            res[f'buf.{name}'] = b.detach().clone()
    return res


def main():
    assert os.path.isdir(REF), f"{REF} not found: golden vectors can only be regenerated where the reference is mounted"
    torch.set_num_threads(1)
    spec = importlib.util.spec_from_file_location(
        'ref_camera_se_net', os.path.join(REF, 'model', 'encoder', 'tpvformer', 'modules', 'camera_se_net.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    files = {'camera_se.npz': {}, 'camera_se_wide.npz': {}, 'camera_se_wide_rc_train.npz': {}, 'camera_se_wide_rc_eval.npz': {}}
    cfg = {}
    for name in cases.CASES:
        inp = cases.case_inputs(name)
        C, M = inp['C'], inp['M']

        def fresh():
            return cases.seed_module(ref.CameraAwareSE(C, M, C), inp['seed'])
        cfg[name] = {'in_channels': C, 'mid_channels': M, 'out_channels': C, 'num_cams': inp['N'], 'levels': [list(s) for s in inp['levels']],
                     'state_dict': {k: list(v.shape) for k, v in fresh().state_dict().items()}}
        main_file = files['camera_se_wide.npz' if name == 'c96m192' else 'camera_se.npz']
        for k, v in cases.checks(fresh(), inp).items():
            main_file[f'{name}.{k}'] = v
        if name == 'enc32':
            for l, m in enumerate(inp['maps']):
                main_file[f'{name}.maps.{l}'] = m.numpy()
            main_file[f'{name}.metas.intrinsic'] = np.asarray([m['intrinsic'] for m in inp['metas']])
            main_file[f'{name}.metas.cam2ego'] = np.asarray([m['cam2ego'] for m in inp['metas']])
        for mode in ('train', 'eval'):
            r32 = run(fresh(), inp, torch.float32, mode == 'train')
            r64 = run(fresh(), inp, torch.float64, mode == 'train')
            for k, v in r32.items():
                dst = main_file
                if name == 'c96m192' and k == 'grad.reduce_conv.0.weight':
                    dst = files[f'camera_se_wide_rc_{mode}.npz']
                dst[f'{name}.{mode}.{k}'] = v.numpy()
                if k.endswith('num_batches_tracked'):
                    continue
                scale_key = 'grad.reduce_conv.0.weight' if (k == 'grad.reduce_conv.0.bias' and mode == 'train') else k
                scale = float(r64[scale_key].abs().max())
                main_file[f'{name}.{mode}.spread.{k}'] = np.array(float((v.double() - r64[k]).abs().max()) / scale)
    for fn, arrs in files.items():
        write_npz(os.path.join(HERE, fn), arrs)
    with open(os.path.join(HERE, 'camera_se_cfg.json'), 'w') as f:
        json.dump(cfg, f, indent=1, sort_keys=True)
        f.write('\n')
    worst = max((float(v), k) for arrs in files.values() for k, v in arrs.items() if '.spread.' in k)
    print('largest spread: %.3g (%s)' % worst)


if __name__ == '__main__':
    main()
