"""GPU (one MI355X, two processes sharing cuda:0 over gloo, as tests/test_dist_gpu.py): under ray sharding every rank marches
its row block of every camera, and `ms_depths_median` is all-gathered into the full frame like every other per-ray map."""
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
        from selfocc_amd import dist as sdist
        from selfocc_amd.render import render_median_depth
        msgs = []
        os.environ['eval'] = 'true'
        rep, metas, _ = th.make_inputs()
        h = th.make_head(ray_sample_mode='fixed', ray_number=[7, 10], render_bkgd='white', ray_shard=True,
                         return_median_depth=True).eval()
        with torch.no_grad():
            h.prepare(rep, metas)
            out = h.render(metas)
        fwd = h(rep, metas, global_iter=0)              # eval(): no jitter, so forward() marches the same rays
        if fwd['ms_depths_median'][0].requires_grad:
            msgs.append("forward: the median is attached to the graph")
        # what the frame must be: the row blocks of both ranks (4 + 3 rows of every camera), each from the direct call
        vol = h.model.field.volume.detached()
        full, _pix, num_cams, num_rays = h._rays(metas, vol.sdf.device)
        cfg = h._render_cfg(False)
        cfg.inv_s_dev = h.model.field.inv_s_device()
        blocks = []
        for r in range(ws):
            sub = sdist.shard_rays(full, r, ws)
            blocks.append(render_median_depth(vol, sub, cfg)['median_depth'].reshape(num_cams, sub.ny, sub.nx))
        want = torch.cat(blocks, 1).reshape(1, num_cams, num_rays)
        if [b.shape[1] for b in blocks] != [4, 3] or (num_cams, num_rays) != (2, 70):
            msgs.append(f"unexpected split {[tuple(b.shape) for b in blocks]}")
        for name, o in (('render', out), ('forward', fwd)):
            got = o.get('ms_depths_median')
            if got is None or got[0].shape != want.shape or got[0].shape != o['ms_depths'][0].shape:
                msgs.append(f"{name}: key missing or shape {None if got is None else tuple(got[0].shape)}")
            elif not torch.equal(got[0], want):
                msgs.append(f"{name}: {int((got[0] != want).sum())} of {want.numel()} rays differ from the row blocks")
        if not (want > 0).any():
            msgs.append("every median depth is zero: the scene shows nothing")
        ret[rank] = msgs
    except Exception as e:   # surface the failure in the parent
        import traceback
        ret[rank] = [f"exception: {e!r}\n{traceback.format_exc()}"]
    finally:
        os.environ['eval'] = 'false'
        dist.destroy_process_group()


def test_ray_sharded_head_gathers_the_median_world2(hip):
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
