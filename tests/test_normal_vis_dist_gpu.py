"""GPU (one MI355X, two processes sharing cuda:0 over gloo, as tests/test_median_depth_dist_gpu.py): under ray sharding every
rank renders the normals of its row block of every camera from one launch (render_normal_vis), and `vis_normal` is all-gathered
into the full frame like every other per-ray map.  A ray-sharded head used to return zeros for it."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_gpu import _free_port

pytestmark = pytest.mark.gpu


def _worker(rank, ws, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        import test_head_gpu as th
        msgs = []
        os.environ['eval'] = 'true'
        rep, metas, _ = th.make_inputs()
        kw = dict(ray_sample_mode='fixed', ray_number=[7, 10], render_bkgd='white')
        sharded = th.make_head(ray_shard=True, **kw).eval()
        whole = th.make_head(ray_shard=False, **kw).eval()          # the same seed: the same weights
        with torch.no_grad():
            for h in (sharded, whole):
                h.prepare(rep, metas)
            vol = sharded.model.field.volume
            full, _pix, num_cams, num_rays = sharded._rays(metas, vol.sdf.device)
            if not sharded._sharding(full) or whole._sharding(full):
                msgs.append("the sharded head does not shard, or the plain one does")
            got = sharded.render(metas, vis_normal=True)
            want = whole.render(metas, vis_normal=True)
            off = sharded.render(metas)
        if (num_cams, num_rays) != (2, 70):
            msgs.append(f"unexpected frame {(num_cams, num_rays)}")
        g, w = got['vis_normal'][0], want['vis_normal'][0]
        if g.shape != (1, 2, 70, 3) or g.shape != w.shape:
            msgs.append(f"shape {tuple(g.shape)} / {tuple(w.shape)}")
        elif not torch.equal(g, w):
            msgs.append(f"{int((g != w).any(-1).sum())} of {w[..., 0].numel()} rays differ from the unsharded head's")
        if not ((w - 0.5).abs() > 1e-4).any():
            msgs.append("no ray shows a normal: the scene shows nothing")
        if torch.count_nonzero(off['vis_normal'][0]) != 0:
            msgs.append("the default call does not return zeros")
        ret[rank] = msgs
    except Exception as e:   # surface the failure in the parent
        import traceback
        ret[rank] = [f"exception: {e!r}\n{traceback.format_exc()}"]
    finally:
        os.environ['eval'] = 'false'
        dist.destroy_process_group()


def test_ray_sharded_head_gathers_vis_normal_world2(hip):
    ws = 2
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, ret)) for r in range(ws)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(ws):
        assert ret.get(r) == [], f"rank {r}: {ret.get(r)}"
