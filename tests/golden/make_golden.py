#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the REAL reference code (/root/reference, read
only) on seeded inputs, on CPU.

The reference cannot be imported as a package here (mmengine / mmcv / mmseg / nerfstudio are
absent), so this script
  * installs tiny stand-ins for the third-party symbols the reference files import
    (registries, BaseModule, init helpers, FFN / LayerNorm builders, MMLogger) — vendor
    plumbing, none of it hot-path arithmetic;
  * provides the one absent hot-path dependency, mmcv's ``multi_scale_deformable_attn_pytorch``
    (the function the reference itself calls on CPU, image_cross_attention.py:344), from
    oracle/torch_port.py;
  * exposes the reference's directories as namespace packages WITHOUT executing their
    ``__init__.py`` (which would pull in mmseg backbones), then imports single files.
Nothing from /root/reference is copied: only numeric inputs / outputs / state dicts are saved.
The sdfstudio-fork renderer (NeuSCustomModel) is absent from the reference tree, so no golden
vector exists for it ("parity unpinned", see oracle/oracle_render.c).

Run:  python tests/golden/make_golden.py        (needs /root/reference; ~10 s)
"""
import importlib
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True      # /root/reference is read-only input: importing its files must not leave __pycache__ there

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SELFOCC_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)


# --------------------------------------------------------------------------------------------
# third-party stand-ins
# --------------------------------------------------------------------------------------------
class _Registry:
    def __init__(self, name='ref'):
        self.name, self._d = name, {}

    def register_module(self, name=None, force=False, module=None):
        def reg(cls):
            self._d[name or cls.__name__] = cls
            return cls
        return reg(module) if module is not None else reg

    def build(self, cfg, **kw):
        cfg = dict(cfg)
        return self._d[cfg.pop('type')](**cfg, **kw)


class _BaseModule(nn.Module):
    def __init__(self, init_cfg=None):
        super().__init__()
        self.init_cfg = init_cfg

    def init_weights(self):  # mmengine.model.BaseModule: recurse into children that define init_weights
        for m in self.children():
            if hasattr(m, 'init_weights'):
                m.init_weights()


def _xavier_init(m, gain=1, bias=0, distribution='normal'):
    (nn.init.xavier_uniform_ if distribution == 'uniform' else nn.init.xavier_normal_)(m.weight, gain=gain)
    if m.bias is not None:
        nn.init.constant_(m.bias, bias)


def _constant_init(m, val, bias=0):
    nn.init.constant_(m.weight, val)
    if m.bias is not None:
        nn.init.constant_(m.bias, bias)


class _Logger:
    _instance_dict = {}

    @classmethod
    def get_instance(cls, name, **kw):
        return cls()

    def info(self, *a, **k):
        pass


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_stubs():
    from oracle.torch_port import msda_port
    REG = _Registry('reference_models')
    LOSS_REG = _Registry('reference_losses')

    class FFN(_BaseModule):
        """mmcv==2.0.1 mmcv/cnn/bricks/transformer.py FFN, restated from the published source (mmcv is absent; nothing
        of selfocc_amd is imported here): [Linear, act, Dropout] x (num_fcs - 1), Linear, Dropout; identity + out."""
        def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type='ReLU', inplace=True),
                     ffn_drop=0., dropout_layer=None, add_identity=True, init_cfg=None, **kwargs):
            super().__init__(init_cfg)
            assert num_fcs >= 2 and act_cfg['type'] == 'ReLU' and dropout_layer is None
            layers, in_ch = [], embed_dims
            for _ in range(num_fcs - 1):
                layers.append(nn.Sequential(nn.Linear(in_ch, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(ffn_drop)))
                in_ch = feedforward_channels
            layers += [nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop)]
            self.layers = nn.Sequential(*layers)
            self.dropout_layer = nn.Identity()
            self.add_identity = add_identity

        def forward(self, x, identity=None):
            out = self.layers(x)
            if not self.add_identity:
                return self.dropout_layer(out)
            return (x if identity is None else identity) + self.dropout_layer(out)
    REG.register_module(module=FFN)

    class MSDABase(_BaseModule):
        """parameter layout of mmcv MultiScaleDeformableAttention (forward is overridden by the
        reference's CrossViewHybridAttention)."""
        def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1,
                     batch_first=False, norm_cfg=None, init_cfg=None, value_proj_ratio=1.0):
            super().__init__(init_cfg)
            self.batch_first, self.im2col_step, self.embed_dims = batch_first, im2col_step, embed_dims
            self.num_levels, self.num_heads, self.num_points = num_levels, num_heads, num_points
            self.dropout = nn.Dropout(dropout)
            self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
            self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
            self.value_proj = nn.Linear(embed_dims, int(embed_dims * value_proj_ratio))
            self.output_proj = nn.Linear(int(embed_dims * value_proj_ratio), embed_dims)

        def init_weights(self):
            pass

        def forward(self, query, key=None, value=None, identity=None, query_pos=None, key_padding_mask=None,
                    reference_points=None, spatial_shapes=None, level_start_index=None, **kwargs):
            """mmcv==2.0.1 mmcv/ops/multi_scale_deform_attn.py MultiScaleDeformableAttention.forward, restated from
            the published algorithm (mmcv is absent here; the reference's BEVFormerLayer uses this class as its
            self-attention, config/nuscenes/nuscenes_occ_bev.py:222): value_proj, offset / weight linears, softmax over
            levels x points, loc = ref + off / (W_l, H_l), MSDA, output_proj, dropout + identity."""
            value = query if value is None else value
            identity = query if identity is None else identity
            if query_pos is not None:
                query = query + query_pos
            if not self.batch_first:
                query, value = query.permute(1, 0, 2), value.permute(1, 0, 2)
            bs, nq, _ = query.shape
            nv = value.shape[1]
            assert int((spatial_shapes[:, 0] * spatial_shapes[:, 1]).sum()) == nv
            value = self.value_proj(value)
            if key_padding_mask is not None:
                value = value.masked_fill(key_padding_mask[..., None], 0.0)
            value = value.view(bs, nv, self.num_heads, -1)
            off = self.sampling_offsets(query).view(bs, nq, self.num_heads, self.num_levels, self.num_points, 2)
            aw = self.attention_weights(query).view(bs, nq, self.num_heads, self.num_levels * self.num_points).softmax(-1)
            aw = aw.view(bs, nq, self.num_heads, self.num_levels, self.num_points)
            assert reference_points.shape[-1] == 2
            normalizer = torch.stack([spatial_shapes[..., 1], spatial_shapes[..., 0]], -1)
            loc = reference_points[:, :, None, :, None, :] + off / normalizer[None, None, None, :, None, :]
            out = self.output_proj(msda_port(value, spatial_shapes, loc, aw))
            if not self.batch_first:
                out = out.permute(1, 0, 2)
            return self.dropout(out) + identity

    def deprecated_api_warning(*a, **k):
        return lambda f: f

    build = lambda cfg, *a, **k: REG.build(cfg)
    _mod('mmengine', ConfigDict=dict, MMLogger=_Logger)
    _mod('mmengine.model', BaseModule=_BaseModule, ModuleList=nn.ModuleList, xavier_init=_xavier_init,
         constant_init=_constant_init)
    _mod('mmengine.registry', MODELS=REG, Registry=lambda *a, **k: LOSS_REG)
    _mod('mmengine.logging', MMLogger=_Logger)
    _mod('mmengine.utils', deprecated_api_warning=deprecated_api_warning)
    _mod('mmcv')
    _mod('mmcv.cnn', build_norm_layer=lambda cfg, n: ('ln', nn.LayerNorm(n)))
    _mod('mmcv.cnn.bricks')
    _mod('mmcv.cnn.bricks.transformer', build_attention=build, build_feedforward_network=build,
         build_positional_encoding=build, build_transformer_layer=build)
    _mod('mmcv.ops')
    _mod('mmcv.ops.multi_scale_deform_attn', MultiScaleDeformableAttention=MSDABase,
         MultiScaleDeformableAttnFunction=None, multi_scale_deformable_attn_pytorch=msda_port)
    _mod('mmcv.utils', IS_CUDA_AVAILABLE=False, IS_MLU_AVAILABLE=False)
    _mod('mmseg')
    _mod('mmseg.registry', MODELS=REG)
    _mod('mmseg.models', HEADS=REG)
    tb = _mod('utils.tb_wrapper', WrappedTBWriter=_Logger)
    pkg = types.ModuleType('utils'); pkg.__path__ = []; pkg.tb_wrapper = tb
    sys.modules['utils'] = pkg
    return REG, LOSS_REG


def namespace(pkg):
    """Expose a reference directory as a package without running its __init__.py."""
    m = types.ModuleType(pkg)
    m.__path__ = [os.path.join(REF, *pkg.split('.'))]
    m.__package__ = pkg
    sys.modules[pkg] = m
    return m


def ref_import(name):
    return importlib.import_module(name)


def to_np(sd):
    return {k: v.detach().cpu().numpy() for k, v in sd.items()}


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, keys={len(arrs)}")


# --------------------------------------------------------------------------------------------
def golden_geometry():
    mp = ref_import('model.encoder.bevformer.mappings')
    out = {}
    g = torch.Generator().manual_seed(0)
    cfgs = {
        'occ': dict(nonlinear_mode='linear', h_size=[128, 0], h_range=[40.0, 0], h_half=False, w_size=[128, 0],
                    w_range=[40.0, 0], w_half=False, d_size=[24, 0], d_range=[-1.0, 5.4, 5.4]),
        'kitti': dict(nonlinear_mode='linear', h_size=[256, 0], h_range=[51.2, 0], h_half=True, w_size=[128, 0],
                      w_range=[25.6, 0], w_half=False, d_size=[32, 0], d_range=[-2.0, 4.4, 4.4]),
        'twoseg': dict(nonlinear_mode='linear', h_size=[128, 32], h_range=[51.2, 28.8], h_half=False,
                       w_size=[128, 32], w_range=[51.2, 28.8], w_half=False, d_size=[20, 10], d_range=[-4.0, 4.0, 12.0]),
        'upscale': dict(nonlinear_mode='linear_upscale', h_size=[128, 32], h_range=[51.2, 28.8], h_half=False,
                        w_size=[128, 32], w_range=[51.2, 28.8], w_half=False, d_size=[20, 10], d_range=[-4.0, 4.0, 12.0]),
    }
    for name, kw in cfgs.items():
        m = mp.GridMeterMapping(**kw)
        lo = torch.tensor([-75.0, -75.0, -3.5]) if name != 'kitti' else torch.tensor([-25.0, 0.5, -1.9])
        hi = torch.tensor([75.0, 75.0, 11.0]) if name != 'kitti' else torch.tensor([25.0, 51.0, 4.3])
        xyz = lo + (hi - lo) * torch.rand(400, 3, generator=g)
        grid = torch.rand(400, 3, generator=g) * torch.tensor([m.size_h - 1.0, m.size_w - 1.0, m.size_d - 1.0])
        out[f'{name}.xyz'] = xyz.numpy(); out[f'{name}.grid'] = grid.numpy()
        out[f'{name}.m2g'] = m.meter2grid(xyz.clone()).numpy()
        out[f'{name}.m2g_norm'] = m.meter2grid(xyz.clone(), True).numpy()
        out[f'{name}.g2m'] = m.grid2meter(grid.clone()).numpy()
        out[f'{name}.sizes'] = np.array([m.size_h, m.size_w, m.size_d])
    # the reference's only in-tree KAT (mappings.py:312-318): grid -> metre -> grid round trip
    m = mp.GridMeterMapping(**cfgs['twoseg'])
    kat = torch.tensor([[0, 0, 0], [128, 128, 10], [160, 160, 20], [192, 192, 25], [320, 320, 30], [64, 256, 5]], dtype=torch.float)
    out['kat.grid'] = kat.numpy(); out['kat.meter'] = m.grid2meter(kat).numpy()
    out['kat.back'] = m.meter2grid(m.grid2meter(kat)).numpy()

    rs = ref_import('model.head.nerfacc_head.ray_sampler')
    s = rs.RaySampler('fixed', [5, 8], [90, 160])
    out['rays.fixed'] = s().numpy()
    np.random.seed(123)
    s = rs.RaySampler('cellular', [6, 10], [96, 200], ray_upper_crop=8)
    out['rays.cellular'] = np.stack([s().numpy() for _ in range(3)])

    bu = ref_import('model.encoder.bevformer.utils')
    tu = ref_import('model.encoder.tpvformer.utils')
    out['cvref'] = tu.get_cross_view_ref_points(5, 4, 3, [4, 4, 4]).numpy()
    ref3d = torch.rand(1, 3, 50, 3, generator=g) * torch.tensor([60.0, 60.0, 6.0]) - torch.tensor([30.0, 30.0, 1.0])
    l2i = []
    for i in range(3):
        yaw = 2.1 * i
        R = np.array([[np.sin(yaw), -np.cos(yaw), 0, 0.3], [0, 0, -1, 1.5], [np.cos(yaw), np.sin(yaw), 0, 0.1], [0, 0, 0, 1]])
        K = np.array([[300.0, 0, 200, 0], [0, 300.0, 112, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        l2i.append(K @ R)
    metas = [dict(lidar2img=np.stack(l2i), img_shape=(224, 400))]
    cam, mask = bu.point_sampling(ref3d.clone(), metas)
    out['ps.ref3d'] = ref3d.numpy(); out['ps.lidar2img'] = np.stack(l2i); out['ps.cam'] = cam.numpy(); out['ps.mask'] = mask.numpy()
    metas[0].update(focal_ratios_x=[1.0, 1.1, 0.9], focal_ratios_y=[1.0, 0.95, 1.05])
    cam2, mask2 = bu.point_sampling(ref3d.clone(), metas)
    out['ps.cam_focal'] = cam2.numpy()

    sh = ref_import('model.head.utils.sh_render')
    feats = torch.randn(64, 3, generator=g)
    out['sh.feat'] = feats.numpy()
    out['sh.rgb'] = sh.SHRender(None, torch.randn(64, 3, generator=g), feats, 0, 'relu').numpy()
    save('geometry.npz', **out)


def loss_case(g, R_hw=(6, 10), S=12, Hi=48, Wi=100, num_cams=2):
    R = R_hw[0] * R_hw[1]
    K = np.array([[0.8 * Wi, 0, Wi / 2, 0], [0, 0.8 * Wi, Hi / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    def motion(yaw, tx, tz):
        y = np.deg2rad(yaw)
        Rm = np.array([[np.cos(y), 0, np.sin(y), tx], [0, 1, 0, 0.02], [-np.sin(y), 0, np.cos(y), tz], [0, 0, 0, 1]])
        return K @ Rm @ np.linalg.inv(K)
    metas = [dict(img2prevImg=np.stack([motion(2.0 + c, 0.3, -0.6) for c in range(num_cams)]),
                  img2nextImg=np.stack([motion(-2.5 - c, -0.2, 0.7) for c in range(num_cams)]))]
    imgs = {k: torch.rand(1, num_cams, 3, Hi, Wi, generator=g) for k in ('curr', 'prev', 'next')}
    xs = torch.arange(R_hw[1], dtype=torch.float) * (Wi / R_hw[1]) + 1.7
    ys = torch.arange(R_hw[0], dtype=torch.float) * (Hi / R_hw[0]) + 0.9
    rays = torch.stack([xs[None].expand(R_hw[0], -1), ys[:, None].expand(-1, R_hw[1])], -1).flatten(0, 1)
    weights, ts, deltas = [], [], []
    for c in range(num_cams):
        near = torch.rand(R, 1, generator=g) * 0.5
        far = 2.0 + torch.rand(R, 1, generator=g) * 40.0
        edges = near + (far - near) * torch.linspace(0, 1, S + 1)[None]
        ts.append(((edges[:, :-1] + edges[:, 1:]) / 2).flatten())
        deltas.append((edges[:, 1:] - edges[:, :-1]).flatten())
        weights.append((torch.softmax(torch.randn(R, S, generator=g) * 3, -1) * torch.rand(R, 1, generator=g)).flatten())
    ray_idx = [torch.arange(R).unsqueeze(-1).repeat(1, S).flatten()] * num_cams
    return metas, imgs, rays, weights, ts, deltas, ray_idx, (R, S, Hi, Wi)


def golden_losses(LOSS_REG):
    namespace('loss')
    base = ref_import('loss.base_loss')
    sys.modules['loss'].OPENOCC_LOSS = LOSS_REG
    combine = ref_import('loss.reproj_loss_mono_multi_new_combine')
    mono = ref_import('loss.reproj_loss_mono_multi_new')
    rgbms = ref_import('loss.rgb_loss_ms')
    edge = ref_import('loss.edge_loss_3d_ms')
    g = torch.Generator().manual_seed(7)
    metas, imgs, rays, weights, ts, deltas, ray_idx, (R, S, Hi, Wi) = loss_case(g)
    out = dict(rays=rays.numpy(), img2prevImg=metas[0]['img2prevImg'], img2nextImg=metas[0]['img2nextImg'],
               curr=imgs['curr'].numpy(), prev=imgs['prev'].numpy(), next=imgs['next'].numpy(),
               weights=torch.stack(weights).numpy(), ts=torch.stack(ts).numpy(), deltas=torch.stack(deltas).numpy(),
               dims=np.array([R, S, Hi, Wi, 6, 10]))
    variants = {
        'combine_ssim': (combine.ReprojLossMonoMultiNewCombine, dict(img_size=[Hi, Wi], ray_resize=[6, 10]), False),
        'combine_nossim_deltas': (combine.ReprojLossMonoMultiNewCombine, dict(img_size=[Hi, Wi], no_ssim=True), True),
        'combine_noautomask': (combine.ReprojLossMonoMultiNewCombine, dict(img_size=[Hi, Wi], ray_resize=[6, 10], no_automask=True), False),
        'mono_ssim': (mono.ReprojLossMonoMultiNew, dict(img_size=[Hi, Wi], ray_resize=[6, 10]), False),
        'mono_nossim_deltas': (mono.ReprojLossMonoMultiNew, dict(img_size=[Hi, Wi], no_ssim=True), True),
    }
    keys = dict(curr_imgs='curr_imgs', prev_imgs='prev_imgs', next_imgs='next_imgs', ray_indices='ray_indices',
                weights='weights', ts='ts', metas='metas', ms_rays='ms_rays')
    for name, (cls, kw, use_d) in variants.items():
        idict = dict(keys, deltas='deltas') if use_d else keys
        lossf = cls(weight=1.0, input_dict=idict, **kw)
        lossf.writer = None
        w = [x.clone().requires_grad_(True) for x in weights]
        inp = dict(curr_imgs=imgs['curr'], prev_imgs=imgs['prev'], next_imgs=imgs['next'], ray_indices=ray_idx,
                   weights=w, ts=ts, metas=metas, ms_rays=rays, deltas=deltas)
        val = lossf(inp)
        val.backward()
        out[f'{name}.loss'] = val.detach().numpy()
        out[f'{name}.gw'] = torch.stack([x.grad for x in w]).numpy()
    # the small per-ray losses
    colors = torch.rand(1, 2, R, 3, generator=g)
    out['colors'] = colors.numpy()
    out['rgb_l1.loss'] = rgbms.RGBLossMS(1.0, [Hi, Wi], True, None)(dict(ms_colors=[colors], ms_rays=rays, gt_imgs=imgs['curr'])).numpy()
    out['rgb_ssim.loss'] = rgbms.RGBLossMS(1.0, [Hi, Wi], False, [6, 10])(dict(ms_colors=[colors], ms_rays=rays, gt_imgs=imgs['curr'])).numpy()
    sem = torch.softmax(torch.randn(1, 2, R, 5, generator=g), -1)
    semgt = torch.randint(0, 5, (2, Hi, Wi), generator=g)
    out['sem'] = sem.numpy(); out['semgt'] = semgt.numpy()
    smeta = [dict(sem=semgt)]
    out['semce.loss'] = rgbms.SemCELossMS(1.0, [Hi, Wi], [6, 10])(dict(sem=[sem], metas=smeta, ms_rays=rays)).numpy()
    out['sembce.loss'] = rgbms.SemLossMS(1.0, [Hi, Wi], [6, 10])(dict(sem=[sem], metas=smeta, ms_rays=rays)).numpy()
    depth = torch.rand(1, 2, R, generator=g) * 30 + 1
    out['depth'] = depth.numpy()
    out['edge.loss'] = edge.EdgeLoss3DMS(1.0, None, img_size=[Hi, Wi], ray_resize=[6, 10])(
        dict(curr_imgs=imgs['curr'], ms_depths=[depth], ms_rays=rays)).numpy()
    save('losses.npz', **out)


def golden_more(LOSS_REG):
    """The remaining importable pieces of the path: Img2LiDAR, BEVNeRF (the authors' in-repo
    field: MLP + tri-plane sum + grid_sample lookup), the small volume losses and MeanIoU."""
    out = {}
    g = torch.Generator().manual_seed(11)
    # ---- Img2LiDAR (model/head/nerfacc_head/img2lidar.py:25-70); `dataset.utils.get_rm` is its only import ----
    ds = types.ModuleType('dataset'); ds.__path__ = [os.path.join(REF, 'dataset')]; sys.modules['dataset'] = ds
    i2l = ref_import('model.head.nerfacc_head.img2lidar')
    mats = np.stack([np.linalg.inv(np.array([[300.0, 0, 200, 0], [0, 300.0, 112, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))] * 3)
    for i in range(3):
        yaw = 0.7 + 2.1 * i
        c2w = np.eye(4); c2w[:3, :3] = np.array([[np.sin(yaw), 0, np.cos(yaw)], [-np.cos(yaw), 0, np.sin(yaw)], [0, -1, 0]])
        c2w[:3, 3] = [0.3 * i, -0.2, 1.5]
        mats[i] = c2w @ mats[i]
    tem = mats.copy(); tem[:, :3, 3] += 0.25
    metas = [dict(img2lidar=list(mats), temImg2lidar=list(tem))]
    rays = torch.rand(37, 2, generator=g) * torch.tensor([400.0, 224.0])
    out['i2l.img2lidar'] = mats; out['i2l.temImg2lidar'] = tem; out['i2l.rays'] = rays.numpy()
    os.environ['eval'] = 'false'
    o, dvec = i2l.Img2LiDAR('img2lidar')(metas, rays)
    out['i2l.single.origin'], out['i2l.single.dir'] = o.numpy(), dvec.numpy()
    o, dvec = i2l.Img2LiDAR(['img2lidar', 'temImg2lidar'])(metas, rays)
    out['i2l.split.origin'], out['i2l.split.dir'] = o.numpy(), dvec.numpy()
    o, dvec = i2l.Img2LiDAR('temImg2lidar', novel_view=[0.5, -1.0, 0.25, 12.0])(metas, rays)
    out['i2l.novel.origin'], out['i2l.novel.dir'] = o.numpy(), dvec.numpy()
    os.environ['eval'] = 'true'
    o, dvec = i2l.Img2LiDAR('temImg2lidar', trans_kw_eval=['img2lidar'])(metas, rays)
    out['i2l.eval.origin'], out['i2l.eval.dir'] = o.numpy(), dvec.numpy()
    os.environ['eval'] = 'false'

    # ---- BEVNeRF (model/head/nerfacc_head/bev_nerf.py:8-140): volume + lookup, TPV and BEV forms ----
    bn = ref_import('model.head.nerfacc_head.bev_nerf')
    mapping_args = dict(nonlinear_mode='linear', h_size=[4, 0], h_range=[8.0, 0], h_half=False, w_size=[3, 0],
                        w_range=[6.0, 0], w_half=False, d_size=[2, 0], d_range=[-1.0, 3.0, 3.0])
    H, W, Z, C = 9, 7, 3, 16
    for tpv in (True, False):
        torch.manual_seed(5)
        f = bn.BEVNeRF(mapping_args, embed_dims=C, color_dims=3, sem_dims=4, density_layers=2, sh_deg=0, tpv=tpv)
        tag = 'tpv' if tpv else 'bev'
        rep = [torch.randn(1, H * W, C, generator=g), torch.randn(1, Z * H, C, generator=g), torch.randn(1, W * Z, C, generator=g)]
        with torch.no_grad():
            f.pre_compute_density_color(rep if tpv else rep[0])
        xyz = torch.rand(200, 3, generator=g) * torch.tensor([14.0, 18.0, 5.0]) - torch.tensor([7.0, 9.0, 1.5])
        grid = f.mapping.meter2grid(xyz, True)
        grid = (2 * grid - 1).reshape(1, -1, 1, 1, 3)
        looked = torch.nn.functional.grid_sample(f.density_color, grid[..., [2, 1, 0]], mode='bilinear', align_corners=True)
        out.update({f'bevnerf.{tag}.sd.{k}': v for k, v in to_np(f.state_dict()).items()})
        out[f'bevnerf.{tag}.volume'] = f.density_color.detach().numpy()
        out[f'bevnerf.{tag}.xyz'] = xyz.numpy()
        out[f'bevnerf.{tag}.lookup'] = looked.permute(0, 2, 3, 4, 1).flatten(0, 3).detach().numpy()
        out[f'bevnerf.{tag}.softplus_density'] = f.query_density(xyz).detach().numpy()
        for i, r in enumerate(rep):
            out[f'bevnerf.{tag}.rep{i}'] = r.numpy()

    # ---- the small volume losses (loss/eikonal_loss.py, second_grad_loss.py, sparsity_loss.py) ----
    eik = ref_import('loss.eikonal_loss'); sg = ref_import('loss.second_grad_loss'); sp = ref_import('loss.sparsity_loss')
    grad = torch.randn(500, 3, generator=g); second = torch.randn(3000, generator=g) * 0.1
    dens = torch.randn(12, 10, 4, generator=g)
    out['vl.eik_grad'], out['vl.second_grad'], out['vl.density'] = grad.numpy(), second.numpy(), dens.numpy()
    out['vl.eikonal'] = eik.EikonalLoss(0.1)(dict(eik_grad=grad)).numpy()
    out['vl.second'] = sg.SecondGradLoss(0.01)(dict(second_grad=second)).numpy()
    out['vl.sparsity'] = sp.SparsityLoss(0.5, scale=0.7)(dict(density=dens)).numpy()
    out['vl.soft_sparsity'] = sp.SoftSparsityLoss(0.005, input_dict={'density': 'uniform_sdf'})(dict(uniform_sdf=dens)).numpy()
    out['vl.hard_sparsity'] = sp.HardSparsityLoss(1.0, scale=2.0, thresh=0.3, crop=[[1, 2], [0, 1], [0, 0]])(
        dict(density=dens.clone())).numpy()
    S = 6
    ts = [torch.rand(20 * S, generator=g) * 30 for _ in range(2)]
    sdfs = [torch.randn(20 * S, generator=g) for _ in range(2)]
    depths = [torch.rand(1, 2, 20, generator=g) * 20]
    out['vl.ts'], out['vl.sdfs'], out['vl.depths'] = torch.stack(ts).numpy(), torch.stack(sdfs).numpy(), depths[0].numpy()
    out['vl.adaptive_sparsity'] = sp.AdaptiveSparsityLoss(1.0, slack=4.0)(dict(sdfs=sdfs, ts=ts, ms_depths=depths)).numpy()

    # ---- MeanIoU (utils/metric_util.py:66-165); its .cuda() calls are made no-ops for this CPU run ----
    torch.Tensor.cuda = lambda self, *a, **k: self
    mu_path = os.path.join(REF, 'utils', 'metric_util.py')
    spec = importlib.util.spec_from_file_location('ref_metric_util', mu_path)
    mu = importlib.util.module_from_spec(spec); spec.loader.exec_module(mu)
    classes = list(range(1, 17))
    pred = torch.randint(0, 18, (40, 40, 8), generator=g)
    tgt = torch.randint(0, 18, (40, 40, 8), generator=g)
    tgt[..., 6:] = 17; tgt[..., :1] = 17
    mask = torch.rand(40, 40, 8, generator=g) > 0.4
    out['iou.pred'], out['iou.tgt'], out['iou.mask'] = pred.numpy(), tgt.numpy(), mask.numpy()
    m = mu.MeanIoU(classes, 17, [str(c) for c in classes], use_mask=True, dataset_empty_label=17)
    m.reset()
    m._after_step(pred.clone(), tgt.clone(), mask)
    m._after_step(pred.flip(0).clone(), tgt.clone(), None)
    out['iou.tensor.seen'], out['iou.tensor.correct'], out['iou.tensor.positive'] = \
        m.total_seen.numpy(), m.total_correct.numpy(), m.total_positive.numpy()
    miou, occ = m._after_epoch()
    out['iou.tensor.miou'], out['iou.tensor.occ_iou'] = np.float64(miou), np.float64(occ)
    m.reset()   # Occ3D form: dict targets, z-range crop of the prediction, camera mask
    m._after_step(pred.clone(), dict(semantics=tgt.numpy().copy(), mask_camera=mask.numpy().astype(np.uint8)))
    out['iou.dict.seen'], out['iou.dict.correct'], out['iou.dict.positive'] = \
        m.total_seen.numpy(), m.total_correct.numpy(), m.total_positive.numpy()
    miou, occ = m._after_epoch()
    out['iou.dict.miou'], out['iou.dict.occ_iou'] = np.float64(miou), np.float64(occ)
    lut_in = torch.arange(21)
    out['iou.openseed2nuscenes'] = mu.openseed2nuscenes(lut_in).numpy()
    save('more.npz', **out)


def golden_segmentor(REG):
    """The calling protocol of the reference's own TPVSegmentor (model/segmentor/tpv_segmentor.py:87-123) over
    lifter / encoder / head: which method of which stage is called with which keyword arguments, in the three modes
    train.py / eval_depth.py / eval_iou.py use.  Recording stand-ins take the place of the five sub-modules, so the
    fixture pins the reference's control flow itself; tests/test_golden_gpu.py replays it over OUR lifter / encoder
    / head (the reference tree is not available on the GPU box)."""
    import json
    calls = []

    class Rec(nn.Module):
        def __init__(self, stage):
            super().__init__()
            self.stage = stage

        def _rec(self, method, kw):
            calls.append(dict(stage=self.stage, method=method, kwargs=sorted(kw)))

        def forward(self, *args, **kw):
            assert not args
            self._rec('forward', kw)
            return {'representation': 'rep'} if self.stage in ('lifter', 'encoder') else {'head_out': 1}

        def prepare(self, *args, **kw):
            self._rec('prepare', kw); return {}

        def forward_occ(self, *args, **kw):
            self._rec('forward_occ', kw); return {'sdf': 0}

    class Backbone(nn.Module):
        def forward(self, x):
            return [torch.zeros(x.shape[0], 8, 8 >> i, 8 >> i) for i in range(4)]

    class Neck(nn.Module):
        def forward(self, feats):
            return [f[:, :4] for f in feats]

    SEG = _Registry('segmentors')
    builder = types.SimpleNamespace(build_backbone=lambda cfg: Backbone(), build_neck=lambda cfg: Neck(),
                                    build_head=lambda cfg: Rec(cfg['stage']))
    sys.modules['mmseg.models'].SEGMENTORS = SEG
    sys.modules['mmseg.models'].builder = builder
    sys.modules['mmseg.models'].build_backbone = builder.build_backbone
    _mod('mmdet3d'); _mod('mmdet3d.registry', MODELS=REG)
    namespace('model.segmentor')
    ref_import('model.segmentor.base_segmentor')
    seg_mod = ref_import('model.segmentor.tpv_segmentor')
    seg = seg_mod.TPVSegmentor(img_backbone=dict(type='B'), img_neck=dict(type='N'), lifter=dict(stage='lifter'),
                               encoder=dict(stage='encoder'), head=dict(stage='head'), img_backbone_out_indices=[1, 2, 3])
    imgs = torch.zeros(1, 2, 3, 16, 16)
    metas = [dict(flip=False)]
    protocol = {}
    for mode, kw in (('train', dict(global_iter=7)), ('prepare', dict(prepare=True)), ('occ_only', dict(occ_only=True, aabb=[0] * 6, resolution=0.4))):
        calls.clear()
        res = seg(imgs=imgs, metas=metas, points=None, **kw)
        protocol[mode] = dict(calls=list(calls), result_keys=sorted(res))
    with open(os.path.join(HERE, 'segmentor_protocol.json'), 'w') as f:
        json.dump(protocol, f, indent=1)
    print("wrote segmentor_protocol.json:", {m: [(c['stage'], c['method']) for c in v['calls']] for m, v in protocol.items()})


def golden_encoder(REG):
    for p in ('model', 'model.encoder', 'model.encoder.bevformer', 'model.encoder.bevformer.attention',
              'model.encoder.tpvformer', 'model.encoder.tpvformer.attention', 'model.encoder.tpvformer.modules',
              'model.lifter'):
        if p not in sys.modules:
            namespace(p)
    ica = ref_import('model.encoder.bevformer.attention.image_cross_attention')
    sys.modules['model.encoder.bevformer.attention'].BEVCrossAttention = ica.BEVCrossAttention
    sys.modules['model.encoder.bevformer.attention'].BEVDeformableAttention = ica.BEVDeformableAttention
    cv = ref_import('model.encoder.tpvformer.attention.cross_view_hybrid_attention')
    tca = ref_import('model.encoder.tpvformer.attention.image_cross_attention')
    sys.modules['model.encoder.tpvformer.attention'].TPVCrossAttention = tca.TPVCrossAttention
    sys.modules['model.encoder.tpvformer.attention'].CrossViewHybridAttention = cv.CrossViewHybridAttention
    sys.modules['model.encoder.tpvformer.modules'].CameraAwareSE = object
    ref_import('model.encoder.tpvformer.tpvformer_pos_embed')
    ref_import('model.encoder.tpvformer.tpvformer_encoder_layer')
    enc_mod = ref_import('model.encoder.tpvformer.tpvformer_encoder')
    lift = ref_import('model.lifter.tpv_query_lifter')

    torch.manual_seed(0)
    dim, heads = 32, 2
    mapping_args = dict(nonlinear_mode='linear', h_size=[4, 0], h_range=[8.0, 0], h_half=False, w_size=[3, 0],
                        w_range=[6.0, 0], w_half=False, d_size=[2, 0], d_range=[-1.0, 3.0, 3.0])
    H, W, Z = 9, 7, 3
    layer = dict(type='TPVFormerLayer',
                 attn_cfgs=[dict(type='CrossViewHybridAttention', embed_dims=dim, num_heads=heads, num_levels=3,
                                 num_points=4, dropout=0.1, batch_first=True),
                            dict(type='TPVCrossAttention', embed_dims=dim, num_cams=2, dropout=0.1, batch_first=True,
                                 num_heads=heads, num_levels=2, num_points=[3, 3, 2])],
                 feedforward_channels=2 * dim, ffn_dropout=0.1,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    cfg = dict(mapping_args=mapping_args, embed_dims=dim, num_cams=2, num_feature_levels=2,
               positional_encoding=dict(type='TPVPositionalEncoding', num_freqs=[3] * 3, embed_dims=dim,
                                        tot_range=[-6.0, -8.0, -1.0, 6.0, 8.0, 3.0]),
               num_points_cross=[3, 3, 2], num_points_self=[4] * 3, transformerlayers=[layer, layer], num_layers=2)
    import copy
    enc = enc_mod.TPVFormerEncoder(**copy.deepcopy(cfg))
    enc.init_weights()
    # make the offset / weight linears non-trivial (init zeroes them)
    g = torch.Generator().manual_seed(1)
    for n, p in enc.named_parameters():
        if 'sampling_offsets.weight' in n or 'attention_weights' in n:
            p.data = 0.2 * torch.randn(p.shape, generator=g)
    enc.eval()
    lifter = lift.TPVQueryLifter(H, W, Z, dim)
    feats = [torch.randn(1, 2, dim, 6, 10, generator=g), torch.randn(1, 2, dim, 3, 5, generator=g)]
    l2i = []
    for i in range(2):
        yaw = 1.3 + 3.1 * i
        R = np.array([[np.sin(yaw), -np.cos(yaw), 0, 0.1], [0, 0, -1, 1.2], [np.cos(yaw), np.sin(yaw), 0, 0.4], [0, 0, 0, 1]])
        K = np.array([[40.0, 0, 40, 0], [0, 40.0, 24, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        l2i.append(K @ R)
    metas = [dict(lidar2img=np.stack(l2i), img_shape=(48, 80))]
    rep = lifter(feats)['representation']
    with torch.no_grad():
        out = enc(rep, ms_img_feats=feats, metas=metas)['representation']
        # standalone attention outputs of layer 0 for finer-grained pinning
        lay = enc.layers[0]
    arrs = {f'enc.{k}': v for k, v in to_np(enc.state_dict()).items()}
    arrs.update({f'lift.{k}': v for k, v in to_np(lifter.state_dict()).items()})
    arrs.update(feat0=feats[0].numpy(), feat1=feats[1].numpy(), lidar2img=np.stack(l2i),
                out_hw=out[0].numpy(), out_zh=out[1].numpy(), out_wz=out[2].numpy(),
                ref_3d_hw=enc.ref_3d_hw.numpy(), cross_view_ref_points=enc.cross_view_ref_points.numpy())
    save('encoder.npz', **arrs)
    import json
    with open(os.path.join(HERE, 'encoder_cfg.json'), 'w') as f:
        json.dump(dict(encoder=cfg, lifter=dict(tpv_h=H, tpv_w=W, tpv_z=Z, dim=dim), img_shape=[48, 80]), f, indent=1)


def golden_bev_encoder(REG):
    """The BEV lifter family (config/nuscenes/nuscenes_occ_bev.py): the REAL BEVFormerEncoder / BEVFormerLayer /
    BEVPositionalEncoding / BEVCrossAttention / BEVQueryLifter; the layer's self-attention is mmcv's
    MultiScaleDeformableAttention, restated in install_stubs (mmcv is absent)."""
    for p in ('model', 'model.encoder', 'model.encoder.bevformer', 'model.encoder.bevformer.attention', 'model.lifter'):
        if p not in sys.modules:
            namespace(p)
    ica = ref_import('model.encoder.bevformer.attention.image_cross_attention')
    sys.modules['model.encoder.bevformer.attention'].BEVCrossAttention = ica.BEVCrossAttention
    sys.modules['model.encoder.bevformer.attention'].BEVDeformableAttention = ica.BEVDeformableAttention
    ref_import('model.encoder.bevformer.bevformer_pos_embed')
    ref_import('model.encoder.bevformer.bevformer_encoder_layer')
    enc_mod = ref_import('model.encoder.bevformer.bevformer_encoder')
    lift = ref_import('model.lifter.bev_query_lifter')
    REG.register_module(name='MultiScaleDeformableAttention', module=sys.modules['mmcv.ops.multi_scale_deform_attn'].MultiScaleDeformableAttention, force=True)

    torch.manual_seed(3)
    dim, heads = 32, 2
    mapping_args = dict(nonlinear_mode='linear', h_size=[4, 0], h_range=[8.0, 0], h_half=False, w_size=[3, 0],
                        w_range=[6.0, 0], w_half=False, d_size=[2, 0], d_range=[-1.0, 3.0, 3.0])
    H, W = 9, 7
    layer = dict(type='BEVFormerLayer',
                 attn_cfgs=[dict(type='MultiScaleDeformableAttention', embed_dims=dim, num_heads=heads, num_levels=1,
                                 num_points=4, dropout=0.1, batch_first=True),
                            dict(type='BEVCrossAttention', embed_dims=dim, num_cams=2, dropout=0.1, batch_first=True,
                                 deformable_attention=dict(type='BEVDeformableAttention', embed_dims=dim, num_heads=heads,
                                                           num_levels=2, num_points=3, dropout=0.1, batch_first=True))],
                 feedforward_channels=2 * dim, ffn_dropout=0.1,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    cfg = dict(mapping_args=mapping_args, embed_dims=dim, num_cams=2, num_feature_levels=2,
               positional_encoding=dict(type='BEVPositionalEncoding', num_freqs=3, embed_dims=dim,
                                        tot_range=[-6.0, -8.0, -1.0, 6.0, 8.0, 3.0]),
               num_points_cross=3, num_points_self=4, transformerlayers=[layer, layer], num_layers=2)
    import copy
    enc = enc_mod.BEVFormerEncoder(**copy.deepcopy(cfg))
    enc.init_weights()
    g = torch.Generator().manual_seed(4)
    for n, p in enc.named_parameters():
        if 'sampling_offsets.weight' in n or 'attention_weights' in n:
            p.data = 0.2 * torch.randn(p.shape, generator=g)
        if n.endswith('attentions.0.sampling_offsets.bias'):      # the stub's init_weights leaves these at nn.Linear's
            p.data = torch.randn(p.shape, generator=g)
    enc.eval()
    lifter = lift.BEVQueryLifter(H, W, dim)
    feats = [torch.randn(1, 2, dim, 6, 10, generator=g), torch.randn(1, 2, dim, 3, 5, generator=g)]
    l2i = []
    for i in range(2):
        yaw = 0.7 + 3.1 * i
        R = np.array([[np.sin(yaw), -np.cos(yaw), 0, 0.1], [0, 0, -1, 1.2], [np.cos(yaw), np.sin(yaw), 0, 0.4], [0, 0, 0, 1]])
        K = np.array([[40.0, 0, 40, 0], [0, 40.0, 24, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        l2i.append(K @ R)
    metas = [dict(lidar2img=np.stack(l2i), img_shape=(48, 80))]
    rep = lifter(feats)['representation']
    with torch.no_grad():
        out = enc(rep, ms_img_feats=feats, metas=metas)['representation']
    arrs = {f'enc.{k}': v for k, v in to_np(enc.state_dict()).items()}
    arrs.update({f'lift.{k}': v for k, v in to_np(lifter.state_dict()).items()})
    arrs.update(feat0=feats[0].numpy(), feat1=feats[1].numpy(), lidar2img=np.stack(l2i), out=out.numpy(),
                ref_3d=enc.ref_3d.numpy(), ref_2d=enc.ref_2d.numpy())
    save('bev_encoder.npz', **arrs)
    import json
    with open(os.path.join(HERE, 'bev_encoder_cfg.json'), 'w') as f:
        json.dump(dict(encoder=cfg, lifter=dict(bev_h=H, bev_w=W, dim=dim), img_shape=[48, 80]), f, indent=1)


def install_nerfstudio_stubs():
    """Stand-ins for the absent sdfstudio fork (`nerfstudio.*`, docs/installation.md:28-39) so that the REAL
    model/head/neus_head/neus_head.py can be imported and run.  ``NeuSCustomModel.__call__`` /
    ``pre_compute_density_color`` / ``forward_geonetwork`` / ``forward_sdfnetwork`` are served by the declared
    restatement in oracle/torch_port.py (render_port, field_lookup) over the authors' own in-repo field BEVNeRF
    (model/head/nerfacc_head/bev_nerf.py); what the fixture pins is therefore everything neus_head.py itself does —
    ray construction, ts / deltas / max-depth post-math, get_uniform_sdf, forward_occ, two-split, dict assembly —
    NOT the fork's internals (still "parity unpinned", oracle/oracle_render.c)."""
    from oracle import torch_port as tp
    bn = ref_import('model.head.nerfacc_head.bev_nerf')
    DRAWS = {}          # random draws of the last call, replayed by the GPU test

    class FieldHeadNames:
        SDF = 'sdf'

    class SceneBox:
        def __init__(self, aabb, near=None, far=None, collider_type=None, **kw):
            self.aabb, self.near, self.far, self.collider_type = aabb, near, far, collider_type

    class RayBundle:
        def __init__(self, origins, directions, directions_norm=None, pixel_area=None, **kw):
            self.origins, self.directions, self.directions_norm, self.pixel_area = origins, directions, directions_norm, pixel_area

    class Frustums:
        def __init__(self, origins, directions, starts, ends):
            self.origins, self.directions, self.starts, self.ends = origins, directions, starts, ends

        def get_positions(self):
            return self.origins[:, None] + self.directions[:, None] * (self.starts + self.ends) / 2

    class RaySamples:
        def __init__(self, frustums):
            self.frustums = frustums

    class SDFCustomFieldConfig:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    class Field(nn.Module):
        def __init__(self, c):
            super().__init__()
            # colour + semantic logits share `color_dims` in NeuSHead configs (neus_head.py:284-288: h[..., 1:4] rgb, 4: sem)
            self.net = bn.BEVNeRF(c.mapping_args, embed_dims=c.embed_dims, color_dims=c.color_dims, sem_dims=0,
                                  density_layers=c.density_layers, sh_deg=c.sh_deg, sh_act=c.sh_act, tpv=c.tpv)
            self.mapping = self.net.mapping
            self.variance = nn.Parameter(c.beta_init * torch.ones(1), requires_grad=c.beta_learnable)
            self.color_dims, self.return_sem = c.color_dims, c.return_sem
            self.n_rgb = 3 if c.color_dims >= 3 else 0
            self.n_sem = c.color_dims - 3 if c.color_dims > 3 else 0

        def set_numerical_gradients_delta(self, delta):
            self.delta = delta

        def pre_compute_density_color(self, representation, **kw):
            self.net.pre_compute_density_color(representation)

        def forward_geonetwork(self, xyz):
            return tp.field_lookup(self.mapping, self.net.density_color, xyz.reshape(-1, 3))

        def forward_sdfnetwork(self, xyz):
            return self.forward_geonetwork(xyz)[:, 0]

        def inv_s(self):
            return torch.exp(self.variance * 10.0).clip(1e-6, 1e6)

    class Model(nn.Module):
        def __init__(self, cfg, scene_box):
            super().__init__()
            self.cfg, self.scene_box = cfg, scene_box
            self.field = Field(cfg.sdf_field)

        def forward(self, ray_bundle, iter=None):
            c, f = self.cfg, self.field
            o, d, dn = ray_bundle.origins, ray_bundle.directions, ray_bundle.directions_norm[:, 0]
            N = o.shape[0]
            bk = {'white': (1, (1., 1., 1.)), 'black': (1, (0., 0., 0.)), 'random': (2, (0., 0., 0.))}[c.background_color]
            rc = types.SimpleNamespace(aabb=self.scene_box.aabb.flatten().tolist(), n_samples=c.num_samples, near_plane=c.near_plane,
                                       sample_pos=0, inv_s=float(f.inv_s()), depth_div_norm=True, bkgd_mode=bk[0], bkgd=bk[1],
                                       clamp_rgb=not self.training)
            t_rand = torch.rand(N) if (self.training and c.perturb) else None
            if t_rand is not None and getattr(self, 'face_safe', 0.0) > 0:
                t_rand = self._face_safe_jitter(t_rand, o, d, rc)
            bkr = torch.rand(N, 3) if bk[0] == 2 else None
            if t_rand is not None:
                DRAWS['t_rand'] = t_rand
            if bkr is not None:
                DRAWS.setdefault('bkgd', []).append(bkr)
            if getattr(self, 'differentiable', False):
                # golden_train_step: the same restatement with every op differentiable w.r.t. the volume and inv_s
                # (float64 inside; the dict goes back to float32, the dtype the real head and losses compute in)
                dd = torch.float64
                r = tp.render_port_differentiable(
                    f.mapping, f.net.density_color[0].to(dd), f.n_rgb, f.n_sem if c.return_sem else 0, o.to(dd), d.to(dd),
                    dn.to(dd), rc, f.inv_s().to(dd), t_rand=None if t_rand is None else t_rand.to(dd),
                    bkgd_rays=None if bkr is None else bkr.to(dd))
                r = {k: v.float() for k, v in r.items()}
            else:
                with torch.no_grad():
                    r = tp.render_port(f.mapping, f.net.density_color.detach(), f.n_rgb, f.n_sem if c.return_sem else 0, o, d, dn,
                                       rc, t_rand=t_rand, bkgd_rays=bkr, return_samples=True)
            g = r['grad']
            normal = (r['weights'][..., None] * (g / g.norm(dim=-1, keepdim=True).clamp_min(1e-12))).sum(1)
            out = {'rgb': r['rgb'] if 'rgb' in r else o.new_zeros(N, 0), 'accumulation': r['acc'][:, None],
                   'depth': r['depth'][:, None], 'fars': r['fars'][:, None], 'weights': r['weights'][..., None],
                   'normal_vis': (normal + 1.0) / 2.0, 'inv_s': rc.inv_s,
                   'ray_samples': RaySamples(Frustums(o, d, r['starts'][..., None], r['ends'][..., None])),
                   'field_outputs': {FieldHeadNames.SDF: r['sdf'][..., None]},
                   'eik_grad': g.reshape(-1, 3)}
            if 'sem' in r:
                out['sem'] = r['sem']
            if c.sdf_field.second_derivative:
                s = f.net.density_color[0, 0]
                out['field_outputs']['second_grad'] = torch.cat([
                    (s[2:] - 2 * s[1:-1] + s[:-2]).flatten(), (s[:, 2:] - 2 * s[:, 1:-1] + s[:, :-2]).flatten(),
                    (s[:, :, 2:] - 2 * s[:, :, 1:-1] + s[:, :, :-2]).flatten()])
            return out

    def _face_safe_jitter(self, t_rand, o, d, rc):
        """Fixtures that compare GRADIENTS over many iterations (round 6): re-draw the jitter of every ray that has an in-volume
        sample within ``self.face_safe`` voxels of a voxel face (float64).  The trilinear SDF's gradient is piece-wise constant:
        a sample within float32 rounding (~2e-6 voxel here) of a face is evaluated in either cell by two correct float32 /
        float64 implementations, and through the eikonal term ONE such sample moves a few entries of d loss / d volume by
        ~3e-4 of its maximum (measured: tests/golden K-step trajectory, iteration 2, two samples 7e-8 / 1.6e-7 voxel from a
        face).  The draws are recorded and replayed, so both sides see the same — unambiguous — samples."""
        dd = torch.float64
        f = self.field
        S = rc.n_samples
        nears, fars = tp.aabb_collider(o.to(dd), d.to(dd), rc.aabb, rc.near_plane)
        hi = torch.tensor([f.mapping.size_h - 1, f.mapping.size_w - 1, f.mapping.size_d - 1], dtype=dd)
        bins0 = torch.linspace(0.0, 1.0, S + 1, dtype=dd)[None, :]
        centers = (bins0[..., 1:] + bins0[..., :-1]) / 2.0
        upper, lower = torch.cat([centers, bins0[..., -1:]], -1), torch.cat([bins0[..., :1], centers], -1)
        t_rand = t_rand.clone()
        todo = torch.arange(t_rand.numel())
        for _ in range(50):
            tr = t_rand[todo].to(dd)[:, None]
            bins = lower + (upper - lower) * tr
            edges = bins * fars[todo] + (1 - bins) * nears[todo]
            pos = o[todo].to(dd)[:, None, :] + d[todo].to(dd)[:, None, :] * edges[:, :-1, None]
            g = f.mapping.meter2grid(pos.reshape(-1, 3)).reshape(len(todo), S, 3)
            fr = g - torch.floor(g)
            marg = torch.minimum(fr, 1 - fr)
            inside = ((g >= 0) & (g <= hi)).all(-1, keepdim=True)
            bad = (torch.where(inside, marg, torch.ones_like(marg)).amin(dim=(1, 2)) < self.face_safe)
            if not bad.any():
                return t_rand
            todo = todo[bad]
            t_rand[todo] = torch.rand(len(todo))
        raise RuntimeError("face-safe jitter did not converge")
    Model._face_safe_jitter = _face_safe_jitter

    class NeuSCustomModelConfig:
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def setup(self, scene_box=None, num_train_data=0, **kw):
            return Model(self, scene_box)

    _mod('nerfstudio'); _mod('nerfstudio.models'); _mod('nerfstudio.fields'); _mod('nerfstudio.data')
    _mod('nerfstudio.cameras'); _mod('nerfstudio.field_components')
    _mod('nerfstudio.models.neus_custom', NeuSCustomModelConfig=NeuSCustomModelConfig)
    _mod('nerfstudio.fields.sdf_custom_field', SDFCustomFieldConfig=SDFCustomFieldConfig)
    _mod('nerfstudio.data.scene_box', SceneBox=SceneBox)
    _mod('nerfstudio.cameras.rays', RayBundle=RayBundle)
    _mod('nerfstudio.field_components.field_heads', FieldHeadNames=FieldHeadNames)
    return DRAWS


def _flatten_out(prefix, d, arrs):
    """Every entry of a NeuSHead output dict -> npz arrays (lists get an index suffix; None is recorded as absent)."""
    for k, v in d.items():
        if v is None:
            arrs[f'{prefix}.{k}.none'] = np.zeros(0)
        elif isinstance(v, (list, tuple)):
            arrs[f'{prefix}.{k}.len'] = np.array(len(v))
            for i, t in enumerate(v):
                arrs[f'{prefix}.{k}.{i}'] = t.detach().cpu().numpy()
        else:
            arrs[f'{prefix}.{k}'] = v.detach().cpu().numpy()


def _cams(n, seed, img=(64, 64), f=60.0):
    rng = np.random.RandomState(seed)
    Kinv = np.linalg.inv(np.array([[f, 0, img[1] / 2, 0], [0, f, img[0] / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    out = []
    for i in range(n):
        yaw = 0.4 + 2 * np.pi * i / n + 0.1 * rng.randn()
        c2w = np.eye(4)
        c2w[:3, :3] = np.array([[np.sin(yaw), 0, np.cos(yaw)], [-np.cos(yaw), 0, np.sin(yaw)], [0, -1, 0]])
        c2w[:3, 3] = [0.6 * rng.randn(), 0.6 * rng.randn(), 0.4 + 0.2 * rng.randn()]
        out.append(c2w @ Kinv)
    return np.stack(out)



# the SHIPPED head of config/nuscenes/nuscenes_occ.py:303-352, key for key: 256 samples, 6 cameras, color_dims 24
# (rgb + 21 semantic logits), cellular lattice on the 768 x 1600 image, random background, learnable beta 0.1,
# the 80 m x 80 m x 6.4 m box.  Reduced for a CPU fixture: the TPV grid (65 x 65 x 13 instead of 257 x 257 x 25)
# the lattice (6 x 10 rays per camera instead of 48 x 100) and the dense-query resolution (1.6 m instead of 0.4);
# `use_compact_2nd_grad=True` because the fork's non-compact form is not on disk (README).
# Saved to its own file (head_occ.npz): training forward, prepare + render, forward_occ.
OCC_HEAD_CFG = dict(
    roi_aabb=[-40.0, -40.0, -1.0, 40.0, 40.0, 5.4], resolution=1.6, near_plane=0.0, far_plane=1e10, num_samples=256, num_samples_importance=0, num_up_sample_steps=0, base_variance=4, beta_init=0.1,
            beta_max=0.195, total_iters=3516 * 11, beta_hand_tune=False, use_numerical_gradients=False,
            sample_gradient=True, return_uniform_sdf=False, return_second_grad=True, use_compact_2nd_grad=True,
            return_sem=True, return_sample_sdf=False, ray_sample_mode='cellular', ray_number=[6, 10],
            ray_img_size=[768, 1600], ray_upper_crop=0, trans_kw='temImg2lidar', novel_view=None,
            render_bkgd='random',
            mapping_args=dict(nonlinear_mode='linear', h_size=[32, 0], h_range=[40.0, 0], h_half=False,
                              w_size=[32, 0], w_range=[40.0, 0], w_half=False, d_size=[12, 0], d_range=[-1.0, 5.4, 5.4]),
            embed_dims=96, color_dims=24, density_layers=2, sh_deg=0, sh_act='relu', two_split=False, tpv=True)


_HEAD_ENV = []


def _head_env():
    """(the reference's neus_head module, the stand-ins' record of random draws); stubs installed once per process"""
    if not _HEAD_ENV:
        if 'dataset' not in sys.modules:
            ds = types.ModuleType('dataset'); ds.__path__ = [os.path.join(REF, 'dataset')]; sys.modules['dataset'] = ds
        namespace('model.head.neus_head')
        draws = install_nerfstudio_stubs()
        ref_import('model.head.base_head')
        _HEAD_ENV.extend([ref_import('model.head.neus_head.neus_head'), draws])
    return _HEAD_ENV


def golden_head(REG):
    """The REAL NeuSHead (model/head/neus_head/neus_head.py) over the nerfstudio stand-ins: forward (train: cellular
    rays, two-split; eval: fixed rays), prepare + render (chunked and unchunked), forward_occ, for a TPV and a BEV
    configuration.  Every key of every returned dict is saved together with the inputs, the state and the random draws."""
    import json
    nh, DRAWS = _head_env()
    cams = _cams

    cfgs = {
        # TPV, colour + semantics, cellular training lattice, two-split (first half: depth cams, second half: temporal)
        'tpv': dict(roi_aabb=[-12.8, -12.8, -1.0, 12.8, 12.8, 3.0], resolution=0.8, near_plane=0.0, far_plane=1e10,
                    num_samples=32, num_samples_importance=0, num_up_sample_steps=0, base_variance=4, beta_init=0.25,
                    beta_hand_tune=False, use_numerical_gradients=False, sample_gradient=True, return_uniform_sdf=True,
                    return_second_grad=True, use_compact_2nd_grad=True, return_sem=True, return_max_depth=True,
                    return_sample_sdf=True, ray_sample_mode='cellular', ray_number=[6, 10], ray_img_size=[64, 64],
                    ray_upper_crop=4, trans_kw=['img2lidar', 'temImg2lidar'], render_bkgd='random',
                    mapping_args=dict(nonlinear_mode='linear', h_size=[8, 0], h_range=[12.8, 0], h_half=False,
                                      w_size=[8, 0], w_range=[12.8, 0], w_half=False, d_size=[11, 0], d_range=[-1.0, 3.0, 3.0]),
                    embed_dims=96, color_dims=8, density_layers=2, sh_deg=0, sh_act='relu', two_split=True, tpv=True,
                    print_freq=50),
        # BEV, SDF only (the nuscenes_depth / kitti form), fixed lattice, single key with an eval key and a novel view
        'bev': dict(roi_aabb=[-8.0, 0.0, -1.0, 8.0, 16.0, 3.0], resolution=0.5, near_plane=0.0, far_plane=1e10,
                    num_samples=24, num_samples_importance=0, num_up_sample_steps=0, base_variance=4, beta_init=0.3,
                    beta_hand_tune=False, use_numerical_gradients=False, sample_gradient=True, return_uniform_sdf=False,
                    return_second_grad=False, return_sem=False, return_max_depth=True,
                    ray_sample_mode='fixed', ray_number=[5, 8], ray_img_size=[48, 80],
                    trans_kw='temImg2lidar', trans_kw_eval=['img2lidar'], novel_view=[0.3, -0.2, 0.1, 8.0], render_bkgd='white',
                    mapping_args=dict(nonlinear_mode='linear', h_size=[32, 0], h_range=[16.0, 0], h_half=True,
                                      w_size=[8, 0], w_range=[8.0, 0], w_half=False, d_size=[4, 0], d_range=[-1.0, 3.0, 3.0]),
                    embed_dims=32, color_dims=0, density_layers=2, sh_deg=0, sh_act='relu', two_split=False, tpv=False),
        'occ': OCC_HEAD_CFG,          # the shipped nuscenes_occ head (module level: golden_train_step uses it too)
    }
    arrs, meta_json = {}, {}
    occ_arrs, occ_json = {}, {}
    for tag, cfg in cfgs.items():
        light = tag == 'occ'            # the shipped-shape case: 92 k samples per per-sample tensor, fewer calls recorded
        if light:
            arrs, meta_json = occ_arrs, occ_json
        torch.manual_seed({'tpv': 21, 'bev': 22, 'occ': 23}[tag])
        import copy
        head = nh.NeuSHead(**copy.deepcopy(cfg))
        f = head.model.field
        with torch.no_grad():
            f.net.density_net[-1].bias[0] = 0.4          # surfaces inside the box
        H, W, D, C = f.mapping.size_h, f.mapping.size_w, f.mapping.size_d, cfg['embed_dims']
        g = torch.Generator().manual_seed(5)
        if cfg['tpv']:
            rep = [torch.randn(1, H * W, C, generator=g), torch.randn(1, D * H, C, generator=g), torch.randn(1, W * D, C, generator=g)]
        else:
            rep = torch.randn(1, H * W, C, generator=g)
        n_cams = 6 if tag == 'occ' else 2
        img = tuple(cfg['ray_img_size'])
        foc = 1266.0 if tag == 'occ' else 60.0          # nuScenes focal length on the 1600-pixel image
        c0, c1 = cams(n_cams, 1, img, foc), cams(n_cams, 2, img, foc)
        if tag == 'bev':
            c0[:, 1, 3] += 6.0; c1[:, 1, 3] += 6.0        # the KITTI-like box lies in front of the rig
        metas = [dict(img2lidar=list(c0), temImg2lidar=list(c1))]
        for k, v in to_np(head.state_dict()).items():
            arrs[f'{tag}.sd.{k}'] = v
        for i, r in enumerate(rep if cfg['tpv'] else [rep]):
            arrs[f'{tag}.rep{i}'] = r.numpy()
        arrs[f'{tag}.img2lidar'], arrs[f'{tag}.temImg2lidar'] = c0, c1
        meta_json[tag] = cfg

        # ---- train.py: head.forward in training mode (perturbed samples, cellular lattice drawn from numpy) ----
        os.environ['eval'] = 'false'
        head.train()
        DRAWS.clear()
        np.random.seed(77)
        torch.manual_seed(100)
        out = head(rep, metas, global_iter=7)
        _flatten_out(f'{tag}.train', out, arrs)
        arrs[f'{tag}.train.draw.t_rand'] = DRAWS['t_rand'].numpy()
        if 'bkgd' in DRAWS:
            arrs[f'{tag}.train.draw.bkgd'] = DRAWS['bkgd'][0].numpy()
        if cfg['return_uniform_sdf']:
            # the shift of get_uniform_sdf(shift=True) (neus_head.py:283-285) is the LAST torch.rand_like of the call:
            # re-draw it from the recorded generator state by re-running the same sequence
            torch.manual_seed(100)
            N = out['origin'].shape[0]
            torch.rand(N)
            if 'bkgd' in DRAWS:
                torch.rand(N, 3)
            n = int(np.prod(out['uniform_sdf'].shape))
            arrs[f'{tag}.train.draw.shift'] = torch.rand_like(torch.empty(n, 3)).numpy()

        # ---- head.forward in eval mode (no perturbation; eval key / eval lattice) ----
        os.environ['eval'] = 'true'
        head.eval()
        DRAWS.clear()
        torch.manual_seed(101)
        if not light:
            with torch.no_grad():
                out = head(rep, metas)
            _flatten_out(f'{tag}.evalfwd', out, arrs)
            if 'bkgd' in DRAWS:
                arrs[f'{tag}.evalfwd.draw.bkgd'] = DRAWS['bkgd'][0].numpy()
        if cfg['return_uniform_sdf'] and not light:
            torch.manual_seed(101)
            N = out['origin'].shape[0]
            if 'bkgd' in DRAWS:
                torch.rand(N, 3)
            n = int(np.prod(out['uniform_sdf'].shape))
            arrs[f'{tag}.evalfwd.draw.shift'] = torch.rand_like(torch.empty(n, 3)).numpy()

        # ---- eval_depth.py:165-166: prepare + render, unchunked and in chunks of 50 rays ----
        for name, batch in ((('render0', 0),) if light else (('render0', 0), ('render50', 50))):
            DRAWS.clear()
            torch.manual_seed(102)
            with torch.no_grad():
                head.prepare(rep, metas)
                out = head.render(metas, batch=batch)
            _flatten_out(f'{tag}.{name}', out, arrs)
            if 'bkgd' in DRAWS:
                arrs[f'{tag}.{name}.draw.bkgd'] = torch.cat(DRAWS['bkgd']).numpy()

        # ---- eval_iou.py: forward_occ with its own aabb / resolution, and with the head's defaults ----
        with torch.no_grad():
            out = head.forward_occ(rep, metas, aabb=[-6.0, -5.0, -0.5, 6.0, 7.0, 2.5], resolution=0.5)
            out.pop('rep')
            _flatten_out(f'{tag}.occ', out, arrs)
            if not light:
                out = head.forward_occ(rep, metas)
                out.pop('rep')
                _flatten_out(f'{tag}.occdef', out, arrs)
        os.environ['eval'] = 'false'
        if light:
            save('head_occ.npz', **occ_arrs)
            with open(os.path.join(HERE, 'head_occ_cfg.json'), 'w') as fjs:
                json.dump(occ_json, fjs, indent=1)
            arrs, meta_json = {}, {}
        elif tag == 'bev':
            save('head.npz', **arrs)
            with open(os.path.join(HERE, 'head_cfg.json'), 'w') as fjs:
                json.dump(meta_json, fjs, indent=1)


TRAIN_STEP = dict(n_cams=6, img=(768, 1600), focal=1266.0, n_sem=21, seed_params=23, seed_rep=5, seed_imgs=41, seed_np=77,
                  seed_torch=100, global_iter=7)


def train_step_inputs(spec=TRAIN_STEP):
    """Seeded inputs of the training-step fixture that are too large to commit (354 MB of float32 images): the four image
    stacks train.py:205-208 moves to the device, the OpenSeeD label map train.py:214-215 puts into the metas, and the
    pixel-depth transforms to the temporal frames.  Shared with tests/test_golden_train_step_gpu.py, which regenerates
    them from the same seeds (CPU generator: the same numbers wherever the same torch build runs).
    Images are smooth (a bilinear blow-up of 48 x 100 noise, like photographs at the scale of a ray footprint) plus 2 % of
    pixel noise: on white noise the bilinear taps would amplify the float32 rounding of a projected pixel coordinate by
    the full dynamic range, which says nothing about either implementation."""
    g = torch.Generator().manual_seed(spec['seed_imgs'])
    H, W = spec['img']
    N = spec['n_cams']
    imgs = {}
    for k in ('curr_imgs', 'prev_imgs', 'next_imgs', 'color_imgs'):
        low = torch.rand(N, 3, 48, 100, generator=g)
        up = torch.nn.functional.interpolate(low, size=(H, W), mode='bilinear', align_corners=True)
        imgs[k] = (0.96 * up + 0.04 * torch.rand(N, 3, H, W, generator=g)).unsqueeze(0).contiguous()
    sem_low = torch.randint(0, spec['n_sem'], (N, 1, 24, 50), generator=g).float()
    sem = torch.nn.functional.interpolate(sem_low, size=(H, W), mode='nearest')[:, 0].long()
    f = spec['focal']
    K = np.array([[f, 0, W / 2, 0], [0, f, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])

    def motion(yaw, tx, tz):
        y = np.deg2rad(yaw)
        Rm = np.array([[np.cos(y), 0, np.sin(y), tx], [0, 1, 0, 0.02], [-np.sin(y), 0, np.cos(y), tz], [0, 0, 0, 1]])
        return K @ Rm @ np.linalg.inv(K)
    prev = np.stack([motion(2.0 + 0.3 * c, 0.3, -0.6) for c in range(N)])
    nxt = np.stack([motion(-2.5 - 0.3 * c, -0.2, 0.7) for c in range(N)])
    return imgs, sem, prev, nxt


def shipped_loss_cfg(ray_resize):
    """`loss` and `loss_input_convertion` of the SHIPPED config/nuscenes/nuscenes_occ.py:111-186, read by executing the
    config file itself (plain Python; `_base_` is only a list of paths), with `num_rays` replaced by the fixture's lattice."""
    path = os.path.join(REF, 'config', 'nuscenes', 'nuscenes_occ.py')
    src = open(path).read()
    ns = {}
    exec(compile(src, path, 'exec'), ns)
    assert ns['num_rays'] == [48, 100] and ns['img_size'] == [768, 1600]
    loss = ns['loss']
    for c in loss['loss_cfgs']:
        if 'ray_resize' in c:
            c['ray_resize'] = list(ray_resize)
    return loss, ns['loss_input_convertion']


def golden_train_step(REG, LOSS_REG):
    """ONE training step of the head + losses exactly as train.py:219-239 runs it: the REAL NeuSHead.forward
    (model/head/neus_head/neus_head.py:473-713) at the shipped nuscenes_occ head configuration -> `loss_input_convertion`
    -> the REAL MultiLoss (loss/multi_loss.py:24-43) over the REAL loss classes wired by the shipped `loss` list
    (config/nuscenes/nuscenes_occ.py:111-186) -> loss.backward().  The absent sdfstudio fork is served by the declared
    restatement in its differentiable float64 form (oracle/torch_port.py: render_port_differentiable).  Saved: the
    total, every loss term, the gradients w.r.t. the three TPV planes, every field-MLP parameter, `variance`, and the
    dense field volume (which separates the renderer's backward from the MLP's)."""
    import copy
    import json
    nh, DRAWS = _head_env()
    namespace('loss')
    sys.modules['loss'].OPENOCC_LOSS = LOSS_REG
    for m in ('base_loss', 'reproj_loss_mono_multi_new_combine', 'rgb_loss_ms', 'eikonal_loss', 'second_grad_loss', 'multi_loss'):
        ref_import('loss.' + m)
    spec = TRAIN_STEP
    cfg = copy.deepcopy(OCC_HEAD_CFG)
    torch.manual_seed(spec['seed_params'])
    head = nh.NeuSHead(**copy.deepcopy(cfg))
    head.model.differentiable = True
    f = head.model.field
    with torch.no_grad():
        f.net.density_net[-1].bias[0] = 0.4          # surfaces inside the box (as in golden_head)
    H, W, D, C = f.mapping.size_h, f.mapping.size_w, f.mapping.size_d, cfg['embed_dims']
    g = torch.Generator().manual_seed(spec['seed_rep'])
    rep = [torch.randn(1, H * W, C, generator=g).requires_grad_(True), torch.randn(1, D * H, C, generator=g).requires_grad_(True),
           torch.randn(1, W * D, C, generator=g).requires_grad_(True)]
    img = tuple(cfg['ray_img_size'])
    c0, c1 = _cams(spec['n_cams'], 1, img, spec['focal']), _cams(spec['n_cams'], 2, img, spec['focal'])
    imgs, sem, prev, nxt = train_step_inputs(spec)
    img_metas = [dict(img2lidar=list(c0), temImg2lidar=list(c1), img2prevImg=prev, img2nextImg=nxt, sem=sem)]
    loss_cfg, conv = shipped_loss_cfg(cfg['ray_number'])
    loss_func = LOSS_REG.build(copy.deepcopy(loss_cfg))

    os.environ['eval'] = 'false'
    head.train()
    DRAWS.clear()
    np.random.seed(spec['seed_np'])
    torch.manual_seed(spec['seed_torch'])
    # ---- train.py:219-239 ----
    result_dict = head(rep, img_metas, global_iter=spec['global_iter'])
    vol = f.net.density_color
    vol.retain_grad()
    loss_input = {'curr_imgs': imgs['curr_imgs'], 'prev_imgs': imgs['prev_imgs'], 'next_imgs': imgs['next_imgs'],
                  'curr_feats': imgs['curr_imgs'], 'prev_feats': imgs['prev_imgs'], 'next_feats': imgs['next_imgs'],
                  'metas': img_metas, 'color_imgs': imgs['color_imgs']}
    for loss_input_key, loss_input_val in conv.items():
        loss_input.update({loss_input_key: result_dict[loss_input_val]})
    # per-term gradient digests w.r.t. the field volume (which terms reach the renderer, and how strongly), taken from the
    # same graph before the step's own backward
    term_digest = {}
    for lf in loss_func.losses:
        gv, = torch.autograd.grad(lf(loss_input), vol, retain_graph=True)
        term_digest[lf.__class__.__name__] = np.array([float(gv.double().abs().sum()), float(gv.double().sum()),
                                                       float(gv.abs().max())])
    vol.grad = None                 # retain_grad's hook also fires under autograd.grad
    loss, loss_dict = loss_func(loss_input)
    loss.backward()

    arrs = {f'sd.{k}': v for k, v in to_np(head.state_dict()).items()}
    for k, v in term_digest.items():
        arrs[f'termgrad.{k}'] = v
    for i, r in enumerate(rep):
        arrs[f'rep{i}'] = r.detach().numpy()
        arrs[f'grad.rep{i}'] = r.grad.numpy()
    for n, p in head.named_parameters():
        assert p.grad is not None, n
        arrs[f'grad.sd.{n}'] = p.grad.numpy()
    arrs['grad.volume'] = vol.grad[0].numpy()                    # (1 + color_dims, H, W, D): d loss / d density_color
    arrs['img2lidar'], arrs['temImg2lidar'], arrs['img2prevImg'], arrs['img2nextImg'] = c0, c1, prev, nxt
    arrs['draw.t_rand'] = DRAWS['t_rand'].numpy()
    arrs['draw.bkgd'] = DRAWS['bkgd'][0].numpy()
    arrs['loss.total'] = loss.detach().numpy()
    for k, v in loss_dict.items():
        arrs[f'loss.{k}'] = np.float64(v)
    _flatten_out('out', {k: result_dict[k] for k in ('ms_depths', 'ms_colors', 'ms_accs', 'ms_rays', 'sem', 'second_grad')}, arrs)
    # digests of the regenerated inputs: the GPU test checks that its seeds gave the same images
    for k, v in imgs.items():
        arrs[f'digest.{k}'] = np.array([float(v.double().sum()), float(v[0, :, :, ::97, ::101].double().sum())])
    arrs['digest.sem'] = np.array([int(sem.sum()), int(sem[:, ::97, ::101].sum())])
    save('train_step.npz', **arrs)
    with open(os.path.join(HERE, 'train_step_cfg.json'), 'w') as fjs:
        json.dump(dict(head=cfg, loss=loss_cfg, loss_input_convertion=conv, spec=spec), fjs, indent=1)
    print('train_step: total', float(loss), loss_dict, '|g_vol|', float(vol.grad.abs().max()),
          {n: float(p.grad.abs().max()) for n, p in head.named_parameters()}, {k: v.tolist() for k, v in term_digest.items()})


# jitter draws of the round-6 fixtures keep every in-volume sample at least this many voxels from a voxel face (see
# install_nerfstudio_stubs: _face_safe_jitter); train_step.npz (round 5) is left as drawn
FACE_SAFE = 2e-5


# ---- the two shipped loss COMPOSITIONS no fixture covered until round 6 (review item 1) -----------------------------------
# Head and loss dictionaries are read from the shipped config files themselves (executed: plain Python); only the grids, the
# lattice and the dense-query resolution are reduced for a CPU fixture — everything else is the shipped value, key for key.
VARIANTS = {
    # config/nuscenes/nuscenes_occ_bev.py: BEV field (tpv=False: the MLP emits (1 + color_dims) * Z outputs per BEV cell),
    # SemLossMS (binary cross-entropy on clamped probabilities) + SoftSparsityLoss on the shifted uniform SDF lattice
    'occ_bev': dict(config='config/nuscenes/nuscenes_occ_bev.py',
                    head_over=dict(mapping_args=dict(nonlinear_mode='linear', h_size=[16, 0], h_range=[40.0, 0], h_half=False,
                                                     w_size=[16, 0], w_range=[40.0, 0], w_half=False, d_size=[8, 0],
                                                     d_range=[-1.0, 5.4, 5.4]),
                                   ray_number=[6, 10], resolution=1.6, use_compact_2nd_grad=True),
                    spec=dict(n_cams=6, img=(768, 1600), focal=1266.0, n_sem=21, seed_params=123, seed_rep=105, seed_imgs=141,
                              seed_np=177, seed_torch=200, global_iter=11), shift_y=0.0, sdf_bias=0.4),
    # config/kitti_raw/kitti_raw_depth.py: one camera, SDF-only field (color_dims=0), ReprojLossMonoMultiNew (two temporal
    # candidates) + EdgeLoss3DMS on the mean-normalised depth lattice, half-form h axis (the box lies in front of the rig)
    'kitti_raw': dict(config='config/kitti_raw/kitti_raw_depth.py',
                      head_over=dict(mapping_args=dict(nonlinear_mode='linear', h_size=[64, 0], h_range=[51.2, 0], h_half=True,
                                                       w_size=[16, 0], w_range=[25.6, 0], w_half=False, d_size=[8, 0],
                                                       d_range=[-2.0, 4.4, 4.4]),
                                     ray_number=[6, 10]),
                      spec=dict(n_cams=1, img=(370, 1216), focal=707.0, n_sem=2, seed_params=223, seed_rep=205, seed_imgs=241,
                                seed_np=277, seed_torch=300, global_iter=3), shift_y=8.0, sdf_bias=0.4),
}


def shipped_config_ns(rel):
    path = os.path.join(REF, rel)
    ns = {}
    exec(compile(open(path).read(), path, 'exec'), ns)
    return ns


def _variant_setup(tag, LOSS_REG):
    """(head, rep (leaf tensors), metas, images, loss_func, head cfg, loss cfg, conversion, spec) of a VARIANTS entry"""
    import copy
    v = VARIANTS[tag]
    nh, DRAWS = _head_env()
    namespace('loss')
    sys.modules['loss'].OPENOCC_LOSS = LOSS_REG
    for m in ('base_loss', 'reproj_loss_mono_multi_new_combine', 'reproj_loss_mono_multi_new', 'rgb_loss_ms', 'eikonal_loss',
              'second_grad_loss', 'edge_loss_3d_ms', 'sparsity_loss', 'multi_loss'):
        ref_import('loss.' + m)
    ns = shipped_config_ns(v['config'])
    cfg = copy.deepcopy(ns['model']['head'])
    assert cfg.pop('type') == 'NeuSHead'
    cfg.update(copy.deepcopy(v['head_over']))
    loss_cfg = copy.deepcopy(ns['loss'])
    for c in loss_cfg['loss_cfgs']:
        if 'ray_resize' in c:
            c['ray_resize'] = list(cfg['ray_number'])
    conv = dict(ns['loss_input_convertion'])
    spec = dict(v['spec'])
    torch.manual_seed(spec['seed_params'])
    head = nh.NeuSHead(**copy.deepcopy(cfg))
    head.model.differentiable = True
    head.model.face_safe = FACE_SAFE
    f = head.model.field
    with torch.no_grad():
        f.net.density_net[-1].bias[0] = v['sdf_bias']          # surfaces inside the box
    H, W, D, C = f.mapping.size_h, f.mapping.size_w, f.mapping.size_d, cfg['embed_dims']
    g = torch.Generator().manual_seed(spec['seed_rep'])
    if cfg['tpv']:
        rep = [torch.randn(1, H * W, C, generator=g).requires_grad_(True), torch.randn(1, D * H, C, generator=g).requires_grad_(True),
               torch.randn(1, W * D, C, generator=g).requires_grad_(True)]
    else:
        rep = [torch.randn(1, H * W, C, generator=g).requires_grad_(True)]
    img = tuple(cfg['ray_img_size'])
    assert img == tuple(spec['img'])
    c0, c1 = _cams(spec['n_cams'], 1, img, spec['focal']), _cams(spec['n_cams'], 2, img, spec['focal'])
    c0[:, 1, 3] += v['shift_y']; c1[:, 1, 3] += v['shift_y']
    imgs, sem, prev, nxt = train_step_inputs(spec)
    metas = [dict(img2lidar=list(c0), temImg2lidar=list(c1), img2prevImg=prev, img2nextImg=nxt, sem=sem)]
    loss_func = LOSS_REG.build(copy.deepcopy(loss_cfg))
    return nh, DRAWS, head, rep, metas, imgs, sem, (c0, c1, prev, nxt), loss_func, cfg, loss_cfg, conv, spec


class _RecordRandLike:
    """records every torch.rand_like draw of the wrapped region (the lattice shift of get_uniform_sdf(shift=True),
    neus_head.py:283-285)"""

    def __enter__(self):
        self.draws, self._orig = [], torch.rand_like
        torch.rand_like = lambda t, **k: self.draws.append(self._orig(t, **k)) or self.draws[-1]
        return self

    def __exit__(self, *a):
        torch.rand_like = self._orig


def golden_train_step_variants(REG, LOSS_REG):
    """golden_train_step for the compositions of VARIANTS: REAL NeuSHead.forward -> the config's loss_input_convertion -> REAL
    MultiLoss over the config's own loss list -> backward (train.py:219-239); train_step_<tag>.npz + _cfg.json."""
    import json
    for tag in VARIANTS:
        nh, DRAWS, head, rep, metas, imgs, sem, (c0, c1, prev, nxt), loss_func, cfg, loss_cfg, conv, spec = _variant_setup(tag, LOSS_REG)
        f = head.model.field
        os.environ['eval'] = 'false'
        head.train()
        DRAWS.clear()
        np.random.seed(spec['seed_np'])
        torch.manual_seed(spec['seed_torch'])
        with _RecordRandLike() as rl:
            result_dict = head(rep if cfg['tpv'] else rep[0], metas, global_iter=spec['global_iter'])
        vol = f.net.density_color
        vol.retain_grad()
        loss_input = {'curr_imgs': imgs['curr_imgs'], 'prev_imgs': imgs['prev_imgs'], 'next_imgs': imgs['next_imgs'],
                      'curr_feats': imgs['curr_imgs'], 'prev_feats': imgs['prev_imgs'], 'next_feats': imgs['next_imgs'],
                      'metas': metas, 'color_imgs': imgs['color_imgs']}
        for k, val in conv.items():
            loss_input[k] = result_dict[val]
        term_digest, term_var = {}, {}
        for lf in loss_func.losses:
            gv, gs = torch.autograd.grad(lf(loss_input), [vol, f.variance], retain_graph=True, allow_unused=True)
            term_digest[lf.__class__.__name__] = np.array([float(gv.double().abs().sum()), float(gv.double().sum()), float(gv.abs().max())])
            term_var[lf.__class__.__name__] = 0.0 if gs is None else float(gs)
        vol.grad = None
        f.variance.grad = None
        loss, loss_dict = loss_func(loss_input)
        loss.backward()
        arrs = {f'sd.{k}': val for k, val in to_np(head.state_dict()).items()}
        # d loss / d variance is ONE number summed over every sample of every loss term with both signs; what its error can be
        # compared with is the size of what was summed, of which the per-term gradients are a (lower) bound
        arrs['gradscale.sd.model.field.variance'] = np.float64(sum(abs(v) for v in term_var.values()))
        for k, val in term_digest.items():
            arrs[f'termgrad.{k}'] = val
        for i, r in enumerate(rep):
            arrs[f'rep{i}'] = r.detach().numpy()
            arrs[f'grad.rep{i}'] = r.grad.numpy()
        for n, p in head.named_parameters():
            assert p.grad is not None, n
            arrs[f'grad.sd.{n}'] = p.grad.numpy()
        arrs['grad.volume'] = vol.grad[0].numpy()
        arrs['img2lidar'], arrs['temImg2lidar'], arrs['img2prevImg'], arrs['img2nextImg'] = c0, c1, prev, nxt
        arrs['draw.t_rand'] = DRAWS['t_rand'].numpy()
        arrs['draw.bkgd'] = DRAWS['bkgd'][0].numpy()
        if cfg.get('return_uniform_sdf'):
            assert len(rl.draws) == 1
            arrs['draw.shift'] = rl.draws[0].numpy()
        arrs['loss.total'] = loss.detach().numpy()
        for k, val in loss_dict.items():
            arrs[f'loss.{k}'] = np.float64(val)
        keys = [k for k in ('ms_depths', 'ms_colors', 'ms_accs', 'ms_rays', 'sem', 'second_grad', 'uniform_sdf') if result_dict.get(k) is not None]
        _flatten_out('out', {k: result_dict[k] for k in keys}, arrs)
        for k, val in imgs.items():
            arrs[f'digest.{k}'] = np.array([float(val.double().sum()), float(val[0, :, :, ::97, ::101].double().sum())])
        arrs['digest.sem'] = np.array([int(sem.sum()), int(sem[:, ::97, ::101].sum())])
        save(f'train_step_{tag}.npz', **arrs)
        with open(os.path.join(HERE, f'train_step_{tag}_cfg.json'), 'w') as fjs:
            json.dump(dict(head=cfg, loss=loss_cfg, loss_input_convertion=conv, spec=spec, source=VARIANTS[tag]['config']), fjs, indent=1)
        print(f'train_step_{tag}: total', float(loss), loss_dict, '|g_vol|', float(vol.grad.abs().max()),
              {k: val.tolist() for k, val in term_digest.items()})


# ---- K optimiser steps, not one (review item 4) ------------------------------------------------------------------------------
# train.py:219-254 driven for K iterations with gradient accumulation: loss / grad_accumulation, backward, and every
# grad_accumulation-th iteration clip_grad_norm_(grad_max_norm) + AdamW.step() + zero_grad(); a fresh cellular lattice
# (numpy RNG), jitter and random background (torch RNG) per iteration, global_iter advancing.  Two trajectories: the SHIPPED
# optimizer dict (config/_base_/optimizer.py: AdamW lr 2e-5, weight_decay 1e-4 — at that rate two steps move the losses by
# ~1e-5, i.e. a skipped or stale update would hide inside any tolerance) and the same with lr x 100, where stale state
# (cached lattice, inv_s, workspaces, gradients not zeroed) shows up in the next iteration's losses.
TRAIN_STEPS_K = dict(K=4, grad_accumulation=2, lr_mults=[1.0, 100.0], seed_np=377, seed_torch=400, first_iter=52,
                     head_over=dict(mapping_args=dict(nonlinear_mode='linear', h_size=[16, 0], h_range=[40.0, 0], h_half=False,
                                                      w_size=[16, 0], w_range=[40.0, 0], w_half=False, d_size=[8, 0],
                                                      d_range=[-1.0, 5.4, 5.4])))


def golden_train_steps(REG, LOSS_REG):
    import copy
    import json
    nh, DRAWS = _head_env()
    namespace('loss')
    sys.modules['loss'].OPENOCC_LOSS = LOSS_REG
    for m in ('base_loss', 'reproj_loss_mono_multi_new_combine', 'rgb_loss_ms', 'eikonal_loss', 'second_grad_loss', 'multi_loss'):
        ref_import('loss.' + m)
    spec, ks = TRAIN_STEP, TRAIN_STEPS_K
    cfg = copy.deepcopy(OCC_HEAD_CFG)
    cfg.update(copy.deepcopy(ks['head_over']))
    opt_ns = shipped_config_ns('config/_base_/optimizer.py')
    opt_cfg = dict(opt_ns['optimizer']['optimizer'])
    assert opt_cfg.pop('type') == 'AdamW'
    grad_max_norm = opt_ns['grad_max_norm']
    img = tuple(cfg['ray_img_size'])
    c0, c1 = _cams(spec['n_cams'], 1, img, spec['focal']), _cams(spec['n_cams'], 2, img, spec['focal'])
    imgs, sem, prev, nxt = train_step_inputs(spec)            # the images of train_step.npz (the GPU test shares its cache)
    metas = [dict(img2lidar=list(c0), temImg2lidar=list(c1), img2prevImg=prev, img2nextImg=nxt, sem=sem)]
    loss_cfg, conv = shipped_loss_cfg(cfg['ray_number'])
    arrs = {'img2lidar': c0, 'temImg2lidar': c1, 'img2prevImg': prev, 'img2nextImg': nxt}
    for k, v in imgs.items():
        arrs[f'digest.{k}'] = np.array([float(v.double().sum()), float(v[0, :, :, ::97, ::101].double().sum())])
    arrs['digest.sem'] = np.array([int(sem.sum()), int(sem[:, ::97, ::101].sum())])
    for ti, lr_mult in enumerate(ks['lr_mults']):
        torch.manual_seed(spec['seed_params'])
        head = nh.NeuSHead(**copy.deepcopy(cfg))
        head.model.differentiable = True
        head.model.face_safe = FACE_SAFE
        f = head.model.field
        with torch.no_grad():
            f.net.density_net[-1].bias[0] = 0.4
        H, W, D, C = f.mapping.size_h, f.mapping.size_w, f.mapping.size_d, cfg['embed_dims']
        g = torch.Generator().manual_seed(spec['seed_rep'])
        rep = [torch.nn.Parameter(torch.randn(1, n, C, generator=g)) for n in (H * W, D * H, W * D)]
        named = [(f'rep{i}', r) for i, r in enumerate(rep)] + [('sd.' + n, p) for n, p in head.named_parameters()]
        params = [p for _, p in named]
        if ti == 0:
            for n, p in named:
                arrs[f'init.{n}'] = p.detach().numpy().copy()
        optimizer = torch.optim.AdamW(params, **dict(opt_cfg, lr=opt_cfg['lr'] * lr_mult))
        loss_func = LOSS_REG.build(copy.deepcopy(loss_cfg))
        os.environ['eval'] = 'false'
        head.train()
        np.random.seed(ks['seed_np'])
        torch.manual_seed(ks['seed_torch'])
        pre = f't{ti}'
        n_steps = 0
        reliable = {n: np.ones(p.shape, dtype=bool) for n, p in named}
        for it in range(ks['K']):
            global_iter = ks['first_iter'] + it
            DRAWS.clear()
            # ---- train.py:219-254 ----
            result_dict = head(rep, metas, global_iter=global_iter)
            loss_input = {'curr_imgs': imgs['curr_imgs'], 'prev_imgs': imgs['prev_imgs'], 'next_imgs': imgs['next_imgs'],
                          'curr_feats': imgs['curr_imgs'], 'prev_feats': imgs['prev_imgs'], 'next_feats': imgs['next_imgs'],
                          'metas': metas, 'color_imgs': imgs['color_imgs']}
            for k, v in conv.items():
                loss_input[k] = result_dict[v]
            loss, loss_dict = loss_func(loss_input)
            loss = loss / ks['grad_accumulation']
            loss.backward()
            arrs[f'{pre}.it{it}.loss.total'] = loss.detach().numpy()
            for k, v in loss_dict.items():
                arrs[f'{pre}.it{it}.loss.{k}'] = np.float64(v)
            arrs[f'{pre}.it{it}.draw.t_rand'] = DRAWS['t_rand'].numpy()
            arrs[f'{pre}.it{it}.draw.bkgd'] = DRAWS['bkgd'][0].numpy()
            arrs[f'{pre}.it{it}.ms_rays'] = result_dict['ms_rays'].detach().numpy()
            arrs[f'{pre}.it{it}.inv_s'] = np.float64(float(f.inv_s()))
            if (global_iter + 1) % ks['grad_accumulation'] == 0:
                gn = torch.nn.utils.clip_grad_norm_(params, grad_max_norm)
                arrs[f'{pre}.step{n_steps}.grad_norm'] = np.float64(float(gn))
                for n, p in named:      # Adam divides by sqrt(v): an element whose gradient is noise moves by +-lr whatever its sign
                    ga = p.grad.abs()
                    reliable[n] &= (ga > 1e-3 * ga.max()).numpy()
                    # the accumulated gradient the optimiser sees at this step: whole for the MLP / variance, every 8th row of a plane
                    arrs[f'{pre}.step{n_steps}.grad.{n}'] = (p.grad[0, ::8] if n.startswith('rep') else p.grad).numpy().copy()
                optimizer.step()
                optimizer.zero_grad()
                n_steps += 1
        for n, p in named:
            arrs[f'{pre}.final.{n}'] = p.detach().numpy().copy()
            arrs[f'{pre}.exp_avg.{n}'] = optimizer.state[p]['exp_avg'].numpy().copy()
            arrs[f'{pre}.reliable.{n}'] = np.packbits(reliable[n].reshape(-1))
        print(f'train_steps_k {pre}: lr x{lr_mult}', [float(arrs[f"{pre}.it{i}.loss.total"]) for i in range(ks['K'])],
              'grad_norm', [float(arrs[f"{pre}.step{i}.grad_norm"]) for i in range(n_steps)],
              'inv_s', [float(arrs[f"{pre}.it{i}.inv_s"]) for i in range(ks['K'])],
              'reliable frac', {n: round(float(reliable[n].mean()), 3) for n, _ in named})
    save('train_steps_k.npz', **arrs)
    with open(os.path.join(HERE, 'train_steps_k_cfg.json'), 'w') as fjs:
        json.dump(dict(head=cfg, loss=loss_cfg, loss_input_convertion=conv, spec=spec, steps=ks, optimizer=dict(opt_cfg, type='AdamW'),
                       grad_max_norm=grad_max_norm), fjs, indent=1)


FULL_ENCODER = dict(dim=96, heads=6, cams=6, tpv=(25, 25, 7), fpn=((12, 25), (6, 13), (3, 7), (2, 4)), img_shape=(96, 200),
                    seed_params=31, seed_lifter=32, seed_feats=33, seed_loss=34)


def full_encoder_inputs(spec=FULL_ENCODER):
    """Seeded inputs of the shipped-structure encoder fixture (shared with tests/test_golden_encoder_full_gpu.py, which
    regenerates them instead of loading megabytes): FPN maps, camera matrices, loss direction per plane."""
    g = torch.Generator().manual_seed(spec['seed_feats'])
    feats = [torch.randn(1, spec['cams'], spec['dim'], h, w, generator=g) for h, w in spec['fpn']]
    Hi, Wi = spec['img_shape']
    f = Wi / 2 / np.tan(np.deg2rad(35.0))
    l2i = []
    for i in range(spec['cams']):
        yaw = 0.3 + 2 * np.pi * i / spec['cams']
        R = np.array([[np.sin(yaw), -np.cos(yaw), 0, 0.2 * np.cos(3 * i)], [0, 0, -1, 1.5], [np.cos(yaw), np.sin(yaw), 0, 0.3 * np.sin(2 * i)],
                      [0, 0, 0, 1]])
        K = np.array([[f, 0, Wi / 2, 0], [0, f, Hi / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        l2i.append(K @ R)
    H, W, Z = spec['tpv']
    g = torch.Generator().manual_seed(spec['seed_loss'])
    loss_dirs = [torch.randn(1, n, spec['dim'], generator=g) for n in (H * W, Z * H, W * Z)]
    return feats, np.stack(l2i), loss_dirs


def full_encoder_cfg(spec=FULL_ENCODER):
    """config/nuscenes/nuscenes_occ.py:190-301 with a reduced grid: 96 dims, 6 heads x 16, 6 cameras, 4 FPN levels,
    num_points_cross = [48, 48, 8], num_points_self = 12, two of the four identical layers."""
    dim, heads = spec['dim'], spec['heads']
    H, W, Z = spec['tpv']
    mapping_args = dict(nonlinear_mode='linear', h_size=[(H - 1) // 2, 0], h_range=[40.0, 0], h_half=False,
                        w_size=[(W - 1) // 2, 0], w_range=[40.0, 0], w_half=False, d_size=[Z - 1, 0], d_range=[-1.0, 5.4, 5.4])
    layer = dict(type='TPVFormerLayer',
                 attn_cfgs=[dict(type='CrossViewHybridAttention', embed_dims=dim, num_heads=heads, num_levels=3,
                                 num_points=12, dropout=0.1, batch_first=True),
                            dict(type='TPVCrossAttention', embed_dims=dim, num_cams=spec['cams'], dropout=0.1, batch_first=True,
                                 num_heads=heads, num_levels=4, num_points=[48, 48, 8])],
                 feedforward_channels=2 * dim, ffn_dropout=0.1,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    return dict(mapping_args=mapping_args, embed_dims=dim, num_cams=spec['cams'], num_feature_levels=4,
                positional_encoding=dict(type='TPVPositionalEncoding', num_freqs=[12] * 3, embed_dims=dim,
                                         tot_range=[-40.0, -40.0, -1.0, 40.0, 40.0, 5.4]),
                num_points_cross=[48, 48, 8], num_points_self=[12] * 3, transformerlayers=[layer, layer], num_layers=2)


def golden_encoder_full(REG):
    """The REAL TPVFormerEncoder at the SHIPPED structure (the kernel instantiations nuscenes_occ runs: <16,5|6> camera
    loop, <16,3> self-attention, 6 x 16 head-major projections, pillar points that leave the image), forward planes AND
    the reference's autograd gradients of a seeded scalar w.r.t. every parameter, the query planes and the four FPN maps.
    Parameters / inputs are regenerated from seeds on the test side (tests/util.seeded_fill); stored: outputs, loss,
    gradients (large ones as every 8th row + all row norms), checksums of the regenerated tensors."""
    import copy
    import json
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from util import seeded_fill, grad_digest
    for p in ('model', 'model.encoder', 'model.encoder.bevformer', 'model.encoder.bevformer.attention',
              'model.encoder.tpvformer', 'model.encoder.tpvformer.attention', 'model.encoder.tpvformer.modules',
              'model.lifter'):
        if p not in sys.modules:
            namespace(p)
    ica = ref_import('model.encoder.bevformer.attention.image_cross_attention')
    sys.modules['model.encoder.bevformer.attention'].BEVCrossAttention = ica.BEVCrossAttention
    sys.modules['model.encoder.bevformer.attention'].BEVDeformableAttention = ica.BEVDeformableAttention
    cv = ref_import('model.encoder.tpvformer.attention.cross_view_hybrid_attention')
    tca = ref_import('model.encoder.tpvformer.attention.image_cross_attention')
    sys.modules['model.encoder.tpvformer.attention'].TPVCrossAttention = tca.TPVCrossAttention
    sys.modules['model.encoder.tpvformer.attention'].CrossViewHybridAttention = cv.CrossViewHybridAttention
    sys.modules['model.encoder.tpvformer.modules'].CameraAwareSE = object
    ref_import('model.encoder.tpvformer.tpvformer_pos_embed')
    ref_import('model.encoder.tpvformer.tpvformer_encoder_layer')
    enc_mod = ref_import('model.encoder.tpvformer.tpvformer_encoder')
    lift = ref_import('model.lifter.tpv_query_lifter')

    spec = FULL_ENCODER
    cfg = full_encoder_cfg(spec)
    torch.manual_seed(0)
    enc = enc_mod.TPVFormerEncoder(**copy.deepcopy(cfg))
    enc.init_weights()
    lifter = lift.TPVQueryLifter(*spec['tpv'], spec['dim'])
    seeded_fill(enc, spec['seed_params'])
    seeded_fill(lifter, spec['seed_lifter'])
    enc.eval()                                            # dropout off, autograd on
    feats, l2i, loss_dirs = full_encoder_inputs(spec)
    feats = [f.requires_grad_(True) for f in feats]
    metas = [dict(lidar2img=l2i, img_shape=spec['img_shape'])]
    out = enc(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
    loss = sum((o * d).sum() for o, d in zip(out, loss_dirs)) / sum(o.numel() for o in out)
    names = [n for n, _ in enc.named_parameters()]
    lnames = [n for n, _ in lifter.named_parameters()]
    grads = torch.autograd.grad(loss, list(enc.parameters()) + list(lifter.parameters()) + feats)
    arrs = dict(loss=loss.detach().numpy(), out_hw=out[0].detach().numpy(), out_zh=out[1].detach().numpy(),
                out_wz=out[2].detach().numpy())
    k = 0
    for pref, ns in (('enc', names), ('lift', lnames), ('feat', [str(i) for i in range(len(feats))])):
        for n in ns:
            for kind, t in grad_digest(grads[k]).items():
                arrs[f'grad.{pref}.{n}.{kind}'] = t.numpy()
            k += 1
    # checksums of what the test regenerates from the seeds
    arrs['check.enc'] = np.array([sum(float(p.double().sum()) for p in enc.parameters()),
                                  sum(float(p.double().abs().sum()) for p in enc.parameters())])
    arrs['check.lift'] = np.array([sum(float(p.double().sum()) for p in lifter.parameters())])
    arrs['check.feats'] = np.array([float(f.double().sum()) for f in feats])
    arrs['lidar2img'] = l2i
    # how many pillar points fall outside every image (the inside-point compaction / zero-padding paths are exercised)
    bu = ref_import('model.encoder.bevformer.utils')
    for nm in ('hw', 'zh', 'wz'):
        _, mask = bu.point_sampling(getattr(enc, f'ref_3d_{nm}').unsqueeze(0).clone(), metas)
        arrs[f'visible_frac.{nm}'] = np.array(float(mask.float().mean()))
    save('encoder_full.npz', **arrs)
    with open(os.path.join(HERE, 'encoder_full_cfg.json'), 'w') as fjs:
        json.dump(dict(spec=spec, encoder=cfg, lifter=dict(tpv_h=spec['tpv'][0], tpv_w=spec['tpv'][1], tpv_z=spec['tpv'][2],
                                                             dim=spec['dim'])), fjs, indent=1)
    print('encoder_full: loss', float(loss), 'visible', {n: float(arrs[f'visible_frac.{n}']) for n in ('hw', 'zh', 'wz')})


def golden_shipped_configs():
    """shipped_configs_sha256.json: per experiment config the reference ships (config/{nuscenes,kitti,kitti_raw}/*.py, read
    through selfocc_amd.config), its path and the digest of its hot-path part (tests/util.shipped_cfg_digest) — pins
    scripts/shipped_cfg/*.json without carrying the configs themselves"""
    import glob
    import json
    from selfocc_amd.config import Config
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from util import shipped_cfg_digest
    out = {}
    for path in sorted(f for d in ("nuscenes", "kitti", "kitti_raw") for f in glob.glob(os.path.join(REF, "config", d, "*.py"))):
        out[os.path.basename(path)[:-3]] = dict(source=os.path.relpath(path, REF),
                                                sha256=shipped_cfg_digest(Config.fromfile(path).to_dict()))
    path = os.path.join(HERE, "shipped_configs_sha256.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(out)} configs")


if __name__ == '__main__':
    assert os.path.isdir(REF), f"{REF} not found: golden vectors can only be regenerated where the reference is mounted"
    sys.path.insert(0, REF)
    REG, LOSS_REG = install_stubs()
    for p in ('model', 'model.encoder', 'model.encoder.bevformer', 'model.encoder.tpvformer', 'model.head',
              'model.head.nerfacc_head', 'model.head.utils'):
        namespace(p)
    only = sys.argv[1:]          # e.g. `python make_golden.py bev_encoder` regenerates one fixture
    todo = dict(geometry=golden_geometry, losses=lambda: golden_losses(LOSS_REG), more=lambda: golden_more(LOSS_REG),
                encoder=lambda: golden_encoder(REG), bev_encoder=lambda: golden_bev_encoder(REG),
                segmentor=lambda: golden_segmentor(REG), head=lambda: golden_head(REG),
                train_step=lambda: golden_train_step(REG, LOSS_REG),
                train_step_variants=lambda: golden_train_step_variants(REG, LOSS_REG),
                train_steps_k=lambda: golden_train_steps(REG, LOSS_REG),
                encoder_full=lambda: golden_encoder_full(REG), shipped_configs=golden_shipped_configs)
    for name, fn in todo.items():
        if not only or name in only:
            fn()
