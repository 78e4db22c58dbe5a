"""Generate tests/golden/pos_lifter.npz + pos_lifter_cfg.json by running the REAL reference ``TPVPositionLifter``
(model/lifter/tpv_pos_lifter.py, loaded by file path from the read-only reference tree) on the CPU.  Data only: nothing of
the reference's text is written.

Two mappings: ``linear`` (the 9 x 7 x 3 planes of make_golden.golden_encoder) and ``linear_upscale`` (h_size = w_size =
[4, 2], d_size = [2, 1]; the reference asserts h_size == w_size there).  num_freqs = [3, 4, 5], embed_dims = 32, bs = 2.
Per mapping <m>:
    <m>.sd.<key>        the state dict (the three Linears; the feature buffers are non-persistent)
    <m>.buf.<name>      hw_freq_feat / zh_freq_feat / wz_freq_feat
    <m>.out.<p>         the planes hw / zh / wz, (2, N_p, 32)
    <m>.G.<p>           a random upstream gradient of the same shape
    <m>.grad.<key>      d sum_p (out_p * G_p).sum() / d parameter

Run:  python tests/golden/make_golden_pos_lifter.py        (needs the reference tree; a second)
"""
import json
import os
import sys

sys.dont_write_bytecode = True

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, namespace, ref_import  # noqa: E402
from make_golden_camera_se import write_npz  # noqa: E402

CFGS = {
    'linear': dict(embed_dims=32, tot_range=[-6.0, -8.0, -1.0, 6.0, 8.0, 3.0], num_freqs=[3, 4, 5],
                   mapping_args=dict(nonlinear_mode='linear', h_size=[4, 0], h_range=[8.0, 0], h_half=False, w_size=[3, 0],
                                     w_range=[6.0, 0], w_half=False, d_size=[2, 0], d_range=[-1.0, 3.0, 3.0])),
    'linear_upscale': dict(embed_dims=32, tot_range=[-14.0, -14.0, -1.0, 14.0, 14.0, 6.0], num_freqs=[3, 4, 5],
                           mapping_args=dict(nonlinear_mode='linear_upscale', h_size=[4, 2], h_range=[8.0, 6.0], w_size=[4, 2],
                                             w_range=[8.0, 6.0], d_size=[2, 1], d_range=[-1.0, 3.0, 6.0])),
}
BS = 2
PLANES = ('hw', 'zh', 'wz')


def main():
    install_stubs()
    for p in ('model', 'model.encoder', 'model.encoder.bevformer', 'model.lifter'):
        namespace(p)
    mod = ref_import('model.lifter.tpv_pos_lifter')
    arrs = {}
    for i, (name, cfg) in enumerate(CFGS.items()):
        torch.manual_seed(20 + i)
        lifter = mod.TPVPositionLifter(**json.loads(json.dumps(cfg)))
        g = torch.Generator().manual_seed(40 + i)
        outs = lifter([torch.zeros(BS, 1)])['representation']
        Gs = [torch.randn(o.shape, generator=g) for o in outs]
        params = dict(lifter.named_parameters())
        grads = torch.autograd.grad(sum((o * G).sum() for o, G in zip(outs, Gs)), list(params.values()))
        assert sorted(lifter.state_dict()) == sorted(params)
        for k, v in lifter.state_dict().items():
            arrs[f'{name}.sd.{k}'] = v.detach().numpy()
        for k, v in lifter.named_buffers():
            arrs[f'{name}.buf.{k}'] = v.numpy()
        for p, o, G in zip(PLANES, outs, Gs):
            arrs[f'{name}.out.{p}'] = o.detach().numpy()
            arrs[f'{name}.G.{p}'] = G.numpy()
        for k, gr in zip(params, grads):
            arrs[f'{name}.grad.{k}'] = gr.numpy()
        print(name, 'sizes', lifter.mapping.size_h, lifter.mapping.size_w, lifter.mapping.size_d, [tuple(o.shape) for o in outs])
    write_npz(os.path.join(HERE, 'pos_lifter.npz'), arrs)
    with open(os.path.join(HERE, 'pos_lifter_cfg.json'), 'w') as f:
        json.dump(dict(bs=BS, lifters={k: dict(type='TPVPositionLifter', **v) for k, v in CFGS.items()}), f, indent=1)


if __name__ == '__main__':
    main()
