"""GPU: the pipelined low loop of the code-ahead skip marcher (csrc/render_fwd.hip, `low` in so_march_fast_ahead).

Low mode marches a stretch of interpolated steps that some lane's corner proves unskippable.  Its loop loads the records of
step i + 1 while it interpolates step i, into a second register set, and its body is unrolled by two so that the two sets
ping-pong.  What the unroll adds that can go wrong is WHICH HALF of the body a stretch ends in, and for which reason: a half
that reads the other half's record set, or an exit that takes the pair in flight for the current step's, composites wrong
corners.  A stretch of n trips leaves the loop from its first half if n is odd and from its second half if n is even, and
there are four reasons to leave:

  * range end      the next step would be the last of the sure range (i + 1 >= i_hi);
  * near face      a lane of the next step lies within the near-face margin of a voxel face;
  * unproven       no lane's corner proved the step just composited: its code was loaded after all, and the sure loop goes on;
  * transmittance  every lane's T fell under 1e-10: the march is over.

The scenes are those of tests/test_render_skip_low_mode_gpu.py (the 12 x 10 x 6 volume, lattices 24 x 16 and 37 x 19), at
sample counts that move the end of the sure range by one step (S = 9 | 10, 17 | 18, 33), plus the floor camera looking up out
of the provable layers, its height stepped so that stretches of 5, 4, 3, 2 and 1 trips occur, the ramp (unproven steps,
kept and skipped), a face-cold placement turned by 1e-5 rad (a near-face exit in mid-stretch), and the floor at inv_s 200,
where the rays that reach it saturate within a few steps (the transmittance exit inside a stretch).

Reference: ``ahead=False`` (so_march_fast), all five outputs torch.equal, every launch with the brick workspace.

`stretches` restates the march on the CPU with the tables of the existing test (wave_tables) and lists every entry of low
mode as (trips, reason).  test_every_exit_on_both_halves asserts over all cases of this file that each of the four reasons
occurs at an odd and at an even trip count, and that stretches of one and of two trips occur; every case asserts the exits
it is there for.  These are conditions on the inputs, not on the kernel.
"""
import collections
import functools
import importlib.util
import os

import pytest
import torch

from selfocc_amd import synthetic as sy

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_low_mode_scenes", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "test_render_skip_low_mode_gpu.py"))
_lm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_lm)

REASONS = ("range_end", "near_face", "unproven", "transmittance")


# ---- the stretches of low mode, restated on the CPU ------------------------------------------------------------------
def walk_stretches(S, i_lo, i_hi, t, w, face_safe=True):
    """One wave through so_march_fast_ahead, as walk_wave of the low-mode test walks it; returns [(trips, reason)], one
    entry per entry of low mode.  A trip composites one step; the reason is the first condition of the loop's `go` that
    fails, in the order the kernel evaluates them: unproven, transmittance, range_end, near_face."""
    free, prov, hint, near, exit_ = t["free"][w], t["provable"][w], t["hint"][w], t["near"][w], t["exit"][w]
    out = []
    i = 0
    while i < min(i_lo, S):
        i += 1
        if i >= S or exit_[i - 1]:
            return out
    hinted = 0
    while i < i_hi:
        entered = False
        for half in (0, 1):
            sk = bool(free[i])
            hinted = hinted + 1 if (not sk and hint[i]) else 0
            i += 1
            if exit_[i - 1]:
                return out
            while sk and i < i_hi and free[i]:
                i += 1
                if exit_[i - 1]:
                    return out
            if i >= i_hi:
                break
            entered = half == 1 and hinted >= _lm.ENTER_AFTER
        if entered:
            trips = 0
            while True:
                if i + 1 >= i_hi:
                    out.append((trips, "range_end"))
                    break
                if face_safe and near[i]:
                    out.append((trips, "near_face"))
                    break
                trips += 1
                proven = bool(prov[i])
                i += 1
                if not proven:
                    out.append((trips, "unproven"))
                    if exit_[i - 1]:
                        return out
                    break
                if exit_[i - 1]:
                    out.append((trips, "transmittance"))
                    return out
    return out


@functools.lru_cache(maxsize=None)
def stretches(kind, poses, nx, ny, mode, S, inv_s):
    """Counter of (trips, reason) over the waves of a launch, and the counts of the low-mode test's own walk"""
    sdf, mp, rays = _lm.scene_sdf(kind), _lm.mapping(), _lm.lattice(nx, ny, len(poses), poses)
    codes, _ = _lm._sr.skip_codes_torch(sdf, mp, _lm.AABB, S, inv_s)
    e = sy.explicit_rays(rays)
    lanes = _lm.wave_lanes(rays, mode)
    t, i_lo, i_hi = _lm.wave_tables(sdf.numpy(), codes.numpy(), mp.to_abi(), _lm.AABB, S, inv_s, e.origins.numpy().astype(_lm.f32),
                                    e.dirs.numpy().astype(_lm.f32), lanes)
    got, ref = collections.Counter(), collections.Counter()
    for w in range(lanes.shape[0]):
        got.update(walk_stretches(S, int(i_lo[w]), int(i_hi[w]), t, w))
        ref.update(_lm.walk_wave(S, int(i_lo[w]), int(i_hi[w]), t, w))
    # the two walks agree on what they both count
    assert sum(got.values()) == ref["low_entries"], (got, ref)
    assert sum(n * c for (n, _), c in got.items()) == ref["low_proven"] + ref["low_unproven_kept"] + ref["low_unproven_skipped"]
    assert sum(c for (_, r), c in got.items() if r == "unproven") == ref["low_unproven_kept"] + ref["low_unproven_skipped"]
    return got


def by_half(n):
    """{(reason, trips % 2): count} of the stretches that ran at least one trip"""
    out = collections.Counter()
    for (trips, reason), c in n.items():
        if trips > 0:
            out[(reason, trips % 2)] += c
    return out


def _show(case, n):
    print(f"[low-prefetch] {case}: " + ", ".join(f"{r}/{'odd' if p else 'even'}={c}" for (r, p), c in sorted(by_half(n).items()))
          + "; lengths " + str(sorted({trips for trips, _ in n})))


def run_case(kind, poses, nx, ny, mode, S, inv_s, how="value"):
    rays = _lm.lattice(nx, ny, len(poses), poses)
    got, ref = _lm.both_routes(_lm.volume(kind), rays, mode, _lm.AABB, S, inv_s, how)
    for k in _lm.KEYS:
        assert torch.equal(got[k], ref[k]), (kind, nx, ny, mode, S, inv_s, how, k,
                                             int((got[k].view(torch.int32) != ref[k].view(torch.int32)).sum()))


# ---- the cases --------------------------------------------------------------------------------------------------------
SAMPLES = (9, 10, 17, 18, 33)
FLOOR = [(("floor" if inv_s == 20.0 else "floor200"), _lm.POSES[:n_cams], nx, ny, mode, S, inv_s)
         for nx, ny in ((24, 16), (37, 19)) for n_cams in (1, 3) for mode in ("pixgrid", "explicit") for S in SAMPLES
         for inv_s in (20.0, 200.0)]


def _ids(cases):
    return ["-".join(str(x) for x in (c[0], len(c[1]), c[2], c[3], c[4], c[5], c[6])) for c in cases]


@pytest.mark.parametrize("how", ("value", "device"))
@pytest.mark.parametrize("case", FLOOR, ids=_ids(FLOOR))
def test_floor(hip, case, how):
    """the floor of the low-mode test at sample counts one step apart: the end of the sure range moves by one step"""
    n = stretches(*case)
    _show(case, n)
    assert sum(c for (trips, _), c in n.items() if trips > 0) > 0, (case, n)
    run_case(*case, how)


# The floor camera's place, looking 16 degrees up.  A step is proven while some lane's cell has its own grid point under
# 0.875 m above the floor, which the grid points of the three lowest layers are and those of the fourth (z = 0.32) are not: a
# level camera never leaves them, a rising one leaves them after a number of steps that its height sets.  The heights are
# stepped so that the stretch of the tiles' upper rows has 5, 4, 3, 2 and 1 trips (found with `stretches`, asserted below).
HEIGHTS = ((-0.1, 5), (0.0, 4), (0.1, 3), (0.2, 2), (0.24, 1))
GRAZE = [("floor", (((0.15, 2.7, z), 0.0, 16.0),), 24, 16, mode, S, 20.0) for z, _ in HEIGHTS for mode in ("pixgrid", "explicit")
         for S in (17, 18)]


@pytest.mark.parametrize("case", GRAZE, ids=_ids(GRAZE))
def test_grazed_floor_short_stretches(hip, case):
    n = stretches(*case)
    _show(case, n)
    want = dict(HEIGHTS)[case[1][0][0][2]]
    assert any(trips == want for trips, _ in n), (case, want, n)
    run_case(*case)


RAMP = [(kind, _lm.POSES, 16, 33, mode, S, inv_s) for kind, inv_s in (("ramp", 20.0), ("ramp200", 200.0))
        for mode in ("pixgrid", "explicit") for S in (9, 10, 33)]


@pytest.mark.parametrize("case", RAMP, ids=_ids(RAMP))
def test_ramp_unproven(hip, case):
    """a step that no corner proves, kept or skipped by its code: the loop leaves with the code loads behind the pair in flight"""
    n = stretches(*case)
    _show(case, n)
    assert sum(c for (trips, r), c in n.items() if r == "unproven") > 0, (case, n)
    run_case(*case)


FACE = [(("floor" if inv_s == 20.0 else "floor200"), _lm.face_poses(axis, 0), 24, 16, mode, S, inv_s)
        for axis in ("h", "w", "d") for mode in ("pixgrid", "explicit") for S in (33, 34) for inv_s in (20.0, 200.0)]


@pytest.mark.parametrize("case", FACE, ids=_ids(FACE))
def test_near_face_in_mid_stretch(hip, case):
    """a face-cold placement turned by 1e-5 rad: a lane comes within the margin of a face inside a proven stretch"""
    n = stretches(*case)
    _show(case, n)
    assert sum(c for (trips, r), c in n.items() if r == "near_face" and trips > 0) > 0, (case, n)
    run_case(*case)


def test_range_end_right_behind_a_stretch():
    """sample counts one apart put i_hi behind a stretch of odd and of even length"""
    n = collections.Counter()
    for case in FLOOR:
        n.update(by_half(stretches(*case)))
    assert n[("range_end", 0)] > 0 and n[("range_end", 1)] > 0, n


def test_transmittance_exit_inside_a_stretch():
    """inv_s 200 over the floor: the rays that reach it saturate within a few steps, inside a proven stretch"""
    n = collections.Counter()
    for case in FLOOR + GRAZE + FACE:
        if case[6] == 200.0:
            n.update(by_half(stretches(*case)))
    assert n[("transmittance", 0)] > 0 and n[("transmittance", 1)] > 0, n


def test_every_exit_on_both_halves():
    n, lengths = collections.Counter(), set()
    for case in FLOOR + GRAZE + RAMP + FACE:
        s = stretches(*case)
        n.update(by_half(s))
        lengths |= {trips for trips, _ in s}
    print("[low-prefetch] exits by (reason, trips % 2):", dict(n), "lengths", sorted(lengths))
    for reason in REASONS:
        for parity in (0, 1):
            assert n[(reason, parity)] > 0, (reason, parity, n)
    assert {1, 2} <= lengths, lengths
