"""Generate tests/golden/reproj_dims.npz by running the REAL reference ``ReprojLossMonoMultiNewCombine`` and
``ReprojLossMonoMultiNew`` (loss/reproj_loss_mono_multi_new_combine.py, loss/reproj_loss_mono_multi_new.py, loaded by file path
from the read-only reference tree) on the CPU with ``dims=C`` on C-channel feature maps, on the geometry of
``make_golden.loss_case`` (R = 60, S = 12, 2 cameras, ``img_size`` = [48, 100]).  Data only: nothing of the reference's text is
written.

Channel counts and the resolution of their ``torch.rand`` maps (1, 2, C, h, w); ``img_size`` stays [48, 100] for all of them:
    C = 1: (48, 100)      C = 5: (24, 50)      C = 16: (12, 25)
Variants, those of losses.npz:  combine_ssim, combine_nossim_deltas, combine_noautomask, mono_ssim, mono_nossim_deltas
(ssim: ray_resize=[6, 10];  nossim_deltas: no_ssim=True with weights / deltas).
Per C and variant:  c<C>.<v>.loss,  c<C>.<v>.gw (d loss / d weights),  c<C>.<v>.gap.

The auto-mask minimum picks one candidate per ray, so a fixture must not sit on a tie that float32 rounding could flip:
``gap`` is the smallest difference, over cameras and rays, between the two smallest candidates as the reference stacks them
(the input of ``torch.min(proj_loss, dim=-1)`` / ``proj_loss.min(dim=2)``, recorded while it runs; pairs that both hold the
1e3 of a ray without a valid sample tie exactly and are no margin; no_automask has no minimum in the Combine loss: inf).
The seed is the first of 7, 8, ... for which every C and variant has gap > 1e-4 (stored as ``seed``).

Run:  python tests/golden/make_golden_reproj_dims.py        (needs the reference tree; a few seconds)
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import install_stubs, namespace, ref_import, loss_case  # noqa: E402
from make_golden_camera_se import write_npz  # noqa: E402

MAPS = {1: (48, 100), 5: (24, 50), 16: (12, 25)}
VARIANTS = {
    'combine_ssim': ('combine', dict(ray_resize=[6, 10]), False),
    'combine_nossim_deltas': ('combine', dict(no_ssim=True), True),
    'combine_noautomask': ('combine', dict(ray_resize=[6, 10], no_automask=True), False),
    'mono_ssim': ('mono', dict(ray_resize=[6, 10]), False),
    'mono_nossim_deltas': ('mono', dict(no_ssim=True), True),
}


class RecordMin:
    """records the stacked candidates the reference reduces: (r, K) through ``torch.min(x, dim=-1)`` in the Combine loss,
    (1, 1, K, r) through ``x.min(dim=2)`` in the mono loss; kept as (K, r)"""

    def __enter__(self):
        self.seen, self.fn, self.method = [], torch.min, torch.Tensor.min
        rec = self

        def note(t, a, k):
            dim = a[0] if a else k.get('dim')
            if torch.is_tensor(t) and t.dim() == 2 and dim == -1:
                rec.seen.append(t.detach().clone().transpose(0, 1))
            elif torch.is_tensor(t) and t.dim() == 4 and dim == 2:
                rec.seen.append(t.detach().clone()[0, 0])

        def fn(t, *a, **k):
            note(t, a, k)
            return rec.fn(t, *a, **k)

        def method(t, *a, **k):
            note(t, a, k)
            return rec.method(t, *a, **k)
        torch.min, torch.Tensor.min = fn, method
        return self

    def __exit__(self, *a):
        torch.min, torch.Tensor.min = self.fn, self.method


def cand_gap(seen):
    gap = np.inf
    for c in seen:                                  # (K, r)
        two = c.double().topk(2, dim=0, largest=False).values
        tie_of_masked = (two[0] == 1e3) & (two[1] == 1e3)
        g = (two[1] - two[0])[~tie_of_masked]
        if g.numel():
            gap = min(gap, g.min().item())
    return gap


def run(classes, seed):
    g = torch.Generator().manual_seed(seed)
    metas, _, rays, weights, ts, deltas, ray_idx, (R, S, Hi, Wi) = loss_case(g)
    out = dict(seed=np.array(seed), rays=rays.numpy(), img2prevImg=metas[0]['img2prevImg'], img2nextImg=metas[0]['img2nextImg'],
               weights=torch.stack(weights).numpy(), ts=torch.stack(ts).numpy(), deltas=torch.stack(deltas).numpy(),
               dims=np.array([R, S, Hi, Wi, 6, 10]), channels=np.array(sorted(MAPS)))
    keys = dict(curr_imgs='curr_imgs', prev_imgs='prev_imgs', next_imgs='next_imgs', ray_indices='ray_indices',
                weights='weights', ts='ts', metas='metas', ms_rays='ms_rays')
    for C, (h, w_) in MAPS.items():
        feats = {k: torch.rand(1, len(weights), C, h, w_, generator=g) for k in ('curr', 'prev', 'next')}
        for k, v in feats.items():
            out[f'c{C}.{k}'] = v.numpy()
        for name, (which, kw, use_d) in VARIANTS.items():
            idict = dict(keys, deltas='deltas') if use_d else keys
            lossf = classes[which](weight=1.0, input_dict=idict, img_size=[Hi, Wi], dims=C, **kw)
            lossf.writer = None
            w = [x.clone().requires_grad_(True) for x in weights]
            inp = dict(curr_imgs=feats['curr'], prev_imgs=feats['prev'], next_imgs=feats['next'], ray_indices=ray_idx,
                       weights=w, ts=ts, metas=metas, ms_rays=rays, deltas=deltas)
            with RecordMin() as rec:
                val = lossf(inp)
            val.backward()
            assert len(rec.seen) == (0 if name == 'combine_noautomask' else len(weights)), (name, len(rec.seen))
            assert all(c.shape == (3 if which == 'combine' else 4, R) for c in rec.seen), [c.shape for c in rec.seen]
            gap = cand_gap(rec.seen)
            print(f"seed {seed} C {C} {name}: loss {val.item():.6f}  cand_gap {gap:.3e}")
            if not gap > 1e-4:
                return None
            assert torch.isfinite(val)
            out[f'c{C}.{name}.loss'] = val.detach().numpy()
            out[f'c{C}.{name}.gw'] = torch.stack([x.grad for x in w]).numpy()
            out[f'c{C}.{name}.gap'] = np.array(gap)
    return out


def main():
    _, LOSS_REG = install_stubs()
    namespace('loss')
    ref_import('loss.base_loss')
    sys.modules['loss'].OPENOCC_LOSS = LOSS_REG
    classes = dict(combine=ref_import('loss.reproj_loss_mono_multi_new_combine').ReprojLossMonoMultiNewCombine,
                   mono=ref_import('loss.reproj_loss_mono_multi_new').ReprojLossMonoMultiNew)
    for seed in range(7, 200):
        out = run(classes, seed)
        if out is not None:
            write_npz(os.path.join(HERE, 'reproj_dims.npz'), out)
            return
    raise SystemExit("no seed holds the margins")


if __name__ == '__main__':
    main()
