"""Stage timing of ONE full-resolution depth-evaluation frame of the hot path (eval_depth.py:150-227, the path behind the
reference's "about 90 min"), built from the SHIPPED config/nuscenes/nuscenes_depth.py (scripts/shipped_cfg/nuscenes_depth.json)
with the reference's eval-time overrides (utils/config_tools.py: 450x800 fixed lattice, trans_kw img2lidar): TPV 257x257x31,
aabb +-51.2 x [-4, 5], color_dims 0, 6 x 450x800 rays, 256 samples.  Random FPN features stand in for ResNet50 + FPN (out of
scope).  JSON of per-stage milliseconds."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import hotpath_common as hc

os.environ['eval'] = 'true'
d = torch.device("cuda:0")
torch.manual_seed(0)
cfg = hc.modify_for_eval(hc.shipped("nuscenes_depth"), 'nuscenes')
lifter, encoder, head, _ = hc.build(cfg, d)
encoder.eval(); head.eval(); lifter.eval()
img = tuple(cfg['img_size'])
dim = cfg['model']['encoder']['embed_dims']
c2w, l2i, K = hc.ring_cameras(6, img, 1266.0)
metas = [dict(lidar2img=l2i, img2lidar=c2w, img_shape=img)]
feats = hc.fpn_feats(6, dim, img, d)
st = {}
with torch.no_grad():
    for it in range(7):
        e0 = hc.ev()
        rep = encoder(lifter(feats)['representation'], ms_img_feats=feats, metas=metas)['representation']
        e1 = hc.ev()
        head.prepare(rep, metas)
        e2 = hc.ev()
        out = head.render(metas, batch=90000)
        e3 = hc.ev()
        torch.cuda.synchronize()
        if it >= 2:
            for k, (a, b) in dict(encoder_fwd=(e0, e1), prepare_volume=(e1, e2), render_2p16M_rays=(e2, e3)).items():
                st.setdefault(k, []).append(a.elapsed_time(b))
res = {k: round(sum(v) / len(v), 3) for k, v in st.items()}
res['frame_total_ms'] = round(sum(res.values()), 2)
res['depth_mean'] = round(out['ms_depths'][0].mean().item(), 3)
res['n_rays'] = int(out['ms_depths'][0].numel())
res['built_from'] = cfg['source']
res['max_mem_GB'] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
print(json.dumps(res))
