"""GPU: the phases of the code-ahead skip marcher (csrc/render_fwd.hip, so_march_fast_ahead) and their hand-over points.

A wave looks for its sure-interior range [i_lo, i_hi] within the first and the last 8 steps of the march.  The steps before
i_lo (the head) and from i_hi on (the tail) run the general step, with the interior test; the steps between run a loop that
leaves the test, the `all_interior` flags and the range compares out; a wave without a range runs the general loop alone.
This file puts the boundaries where they can go wrong: S <= 8 (the scan covers the whole march), S = 1 (i_lo == i_hi, no
sure loop), both parities of i_lo and of i_hi - i_lo (rays that enter through a face at varying depth), waves that mix
rays that miss the volume with rays that hit it (no range), and marches that end early in each phase.

The reference is the independent route through the same library, ``ahead=False`` (so_march_fast, step by step); all five
outputs must be torch.equal, with face-safe cell selection on and off.  Every launch takes the brick path.

So that no case is vacuous, each one counts from its own outputs, per 8 x 8 tile (= wavefront) of the 72 x 52 lattice x 2
cameras (126 tiles): tiles that mix missing rays (fars - nears <= 2e-6) with hitting ones, tiles whose rays all enter
through a face (nears > 1e-3: a non-empty head), tiles that start inside, and tiles that end early (acc > 0.999 on every
ray).  With the C oracle on the CPU the outside cameras give 34 mixed and 54 face-entering tiles in the small volume, 28
and 14 in the tiny one, whatever S and inv_s; with the inside cameras all 126 tiles start inside.  Early-ending tiles appear
at inv_s 200 only: 27 (small, boxes, outside), 54 - 57 (small, boxes, inside), 3 - 8 (tiny, outside) and 12 - 32 (tiny,
inside, S >= 2); those cases require at least one.
"""
import functools

import pytest
import torch

from selfocc_amd import synthetic as sy
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.render import SDFVolume

from test_render_skip_run_gpu import small_volume, lattice, camera, INSIDE, OUTSIDE, AABB, _both_routes, _assert_equal

pytestmark = pytest.mark.gpu

NX, NY, TILE = 72, 52, 8
N_TILES = 2 * ((NX + TILE - 1) // TILE) * ((NY + TILE - 1) // TILE)     # 126
MIN_TILES = 10

TINY_AABB = (0.0, 0.0, -1.0, 1.6, 2.0, 0.2)
TINY_INSIDE = (camera((0.3, 1.0, -0.3), 10, -6), camera((1.2, 0.4, -0.2), 120, -10))
TINY_OUTSIDE = (camera((-2.0, 1.0, -0.3), 5, -3), camera((0.8, 4.0, 0.6), -92, -12))


@functools.lru_cache(maxsize=None)
def tiny_volume():
    """6 x 5 x 4 cells (D % 4 == 0 but != 16): 7 488 rays take the brick path from S = 1"""
    m = GridMeterMapping(nonlinear_mode='linear', h_size=[5, 0], h_range=[2.0, 0], h_half=True, w_size=[4, 0], w_range=[1.6, 0],
                         w_half=True, d_size=[3, 0], d_range=[-1.0, 0.2, 0.2])
    z = sy.grid_points_meter(m)[..., 2]
    sdf = z + 0.75 + 0.02 * torch.randn(z.shape, generator=torch.Generator().manual_seed(3))
    assert tuple(sdf.shape) == (6, 5, 4)
    return SDFVolume(m, sdf.contiguous().float())


def tile_stats(out):
    """per 8 x 8 tile of the lattice, from the outputs: (mixed missing / hitting, all rays enter through a face, all rays
    start inside, all rays end with acc > 0.999) as counts of tiles"""
    nears, fars, acc = (out[k].detach().cpu().view(2, NY, NX) for k in ("nears", "fars", "acc"))
    miss = (fars - nears) <= 2e-6
    real = torch.ones_like(miss)

    def tiles(x):       # (2, 7, 9, 64), lanes beyond the lattice edge False
        pad = torch.zeros(2, (NY + TILE - 1) // TILE * TILE, (NX + TILE - 1) // TILE * TILE, dtype=torch.bool)
        pad[:, :NY, :NX] = x
        return pad.view(2, -1, TILE, pad.shape[2] // TILE, TILE).permute(0, 1, 3, 2, 4).reshape(2, -1, pad.shape[2] // TILE, TILE * TILE)

    n_real = tiles(real).sum(-1)
    assert n_real.numel() == N_TILES and int(n_real.min()) > 0
    every = lambda x: tiles(x).sum(-1) == n_real
    some = lambda x: tiles(x).sum(-1) > 0
    mixed = some(miss) & some(~miss)
    face = every(~miss & (nears > 1e-3))
    inside = every(~miss & (nears <= 1e-3))
    early = every(acc > 0.999)
    return int(mixed.sum()), int(face.sum()), int(inside.sum()), int(early.sum())


def _check(vol, cams, outside, aabb, inv_s, S, face_safe, label, want_early):
    run, ref = _both_routes(vol, lattice(*cams), dict(inv_s=inv_s, face_safe=face_safe), aabb, S)
    mixed, face, inside, early = tile_stats(run)
    print(f"[skip-phases] {label}: tiles mixed={mixed} face-entering={face} inside={inside} early-ending={early} of {N_TILES}")
    _assert_equal(run, ref, label)
    if outside:
        assert mixed >= MIN_TILES, (label, mixed)      # waves without a sure range: the general loop for the whole march
        assert face >= MIN_TILES, (label, face)        # waves with a non-empty head
    else:
        assert inside == N_TILES, (label, inside)
    if want_early:
        assert early >= 1, (label, early)


SMALL_S = [8, 9, 15, 16, 17, 33]
TINY_S = [1, 2, 3, 5, 7]


@pytest.mark.parametrize("face_safe", [True, False], ids=["face_safe", "no_face_safe"])
@pytest.mark.parametrize("inv_s", [20.0, 200.0])
@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("kind", ["boxes", "free"])
@pytest.mark.parametrize("S", SMALL_S)
def test_phases_equal_step_by_step_small(hip, S, kind, where, inv_s, face_safe):
    """24 x 20 x 7 cells; S = 8 is the smallest S that takes the brick path here (7 488 * 8 >= 16 * 3 360)"""
    outside = where == "outside"
    _check(small_volume(kind, inv_s), OUTSIDE if outside else INSIDE, outside, AABB, inv_s, S, face_safe,
           f"small {kind} {where} inv_s={inv_s} S={S} face_safe={face_safe}", want_early=kind == "boxes" and inv_s == 200.0)


@pytest.mark.parametrize("face_safe", [True, False], ids=["face_safe", "no_face_safe"])
@pytest.mark.parametrize("inv_s", [20.0, 200.0])
@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("S", TINY_S)
def test_phases_equal_step_by_step_tiny(hip, S, where, inv_s, face_safe):
    """6 x 5 x 4 cells: S in {1, 2, 3, 5, 7}, all below the scan length of 8"""
    outside = where == "outside"
    _check(tiny_volume(), TINY_OUTSIDE if outside else TINY_INSIDE, outside, TINY_AABB, inv_s, S, face_safe,
           f"tiny {where} inv_s={inv_s} S={S} face_safe={face_safe}", want_early=inv_s == 200.0 and (outside or S >= 2))
