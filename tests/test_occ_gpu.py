"""GPU parity of the occupancy evaluation tail: bit-exact integer occupancy / semantics /
IoU counts against the torch ops the reference calls (run on CPU)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import torch_port as tp
from selfocc_amd import synthetic as sy
from selfocc_amd._lib import SelfOccHipError
from selfocc_amd.mapping import GridMeterMapping
from selfocc_amd.occ import field_query, uniform_lattice, occ_resample, MeanIoU, OPENSEED2NUSCENES
from selfocc_amd.render import SDFVolume

pytestmark = pytest.mark.gpu
D0 = torch.device("cuda:0")


@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16])
def test_field_query_bit_exact(hip, feat_dtype):
    vol = sy.make_volume("cfg5", n_rgb=3, n_sem=21, feat_dtype=feat_dtype, seed=2)
    aabb = sy.CONFIGS["cfg5"]["aabb"]
    xyz = uniform_lattice(aabb, 0.4, "cpu", shift=True).reshape(-1, 3)[::7].contiguous()
    got = field_query(vol.to(D0), xyz.to(D0), want_sdf=True, want_logits=True, want_argmax=True)
    ref_sdf, _ = oracle.field_sdf(vol.mapping, vol.sdf, xyz, want_grad=False)
    assert torch.equal(got['sdf'].cpu(), ref_sdf)
    # forward_geonetwork h[..., 4:] = grid_sample of the (1, C, H, W, D) volume (neus_head.py:284-288)
    h = tp.field_lookup(vol.mapping, vol.to_reference_layout(), xyz)
    assert torch.equal(got['sdf'].cpu(), h[:, 0])
    assert torch.equal(got['logits'].cpu(), h[:, 4:])
    assert torch.equal(got['argmax'].cpu().long(), torch.argmax(h[:, 4:], dim=-1))


def _ego2lidar(seed):
    r = np.random.RandomState(seed)
    yaw = math.radians(r.uniform(-3, 3))
    m = np.eye(4)
    m[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    m[:3, 3] = r.uniform(-0.5, 0.5, 3) * [1, 1, 0.2]
    return m


@pytest.mark.parametrize("seed", [0, 1])
def test_occ3d_tail_bit_exact(hip, seed):
    """eval_iou.py:198-250 with scene_size 4 (aabb -40..40, -1..5.4, res 0.4): dense SDF query ->
    ego-frame resample -> (sdf <= thresh) -> crops -> argmax -> LUT.  Integer outputs bit-exact."""
    vol = sy.make_volume("cfg5", n_rgb=3, n_sem=21, seed=seed)
    pcr, expansion = [-40.0, -40.0, -1.0, 40.0, 40.0, 5.4], [80.0, 80.0, 6.4]
    lat = uniform_lattice(pcr, 0.4, "cpu")            # (H, W, D, 3) = (200, 200, 16, 3)
    H, W, D = lat.shape[:3]
    q = field_query(vol.to(D0), lat.reshape(-1, 3).to(D0), want_sdf=True, want_logits=True)
    sdf = q['sdf'].reshape(H, W, D)
    logits = q['logits'].reshape(H, W, D, -1)
    thresh = 0.05
    pred_occ, pred_miou, lidar_points, sampled = tp.occ_tail_port(sdf.cpu(), logits.cpu(), _ego2lidar(seed), pcr,
                                                                  expansion, thresh)
    coords = lidar_points[..., [1, 0, 2]].contiguous()   # normalised along (H<->y, W<->x, D<->z)
    got = occ_resample(sdf, coords.to(D0), thresh, logits=logits, lut=OPENSEED2NUSCENES,
                       crop=(6, 6, 6, 6, 0, 4), want_sampled=True)
    assert torch.equal(got['sampled'].cpu(), sampled)
    assert torch.equal(got['occ'].cpu(), pred_occ)
    assert torch.equal(got['sem'].cpu(), pred_miou.to(torch.int32))
    assert 0.01 < pred_occ.float().mean() < 0.9


def test_iou_counts_exact(hip):
    g = torch.Generator().manual_seed(0)
    pred = torch.randint(0, 18, (200, 200, 16), generator=g, dtype=torch.int32)
    tgt = torch.randint(0, 18, (200, 200, 16), generator=g, dtype=torch.int32)
    mask = torch.rand(200, 200, 16, generator=g) > 0.4
    cls = list(range(1, 17))
    for use_mask in (False, True):
        m = MeanIoU(cls, 0, [str(c) for c in cls], True, 0)
        m.reset()
        m._after_step(pred.to(D0), tgt.to(D0), mask.to(D0) if use_mask else None)
        m._after_step(tgt.to(D0), pred.to(D0), mask.to(D0) if use_mask else None)
        ref = tp.mean_iou_counts_port(pred, tgt, cls, 0, mask if use_mask else None) + \
            tp.mean_iou_counts_port(tgt, pred, cls, 0, mask if use_mask else None)
        assert torch.equal(m.counts.cpu(), ref)
        miou, iou = m._after_epoch()
        r = ref.double()
        assert abs(iou - (r[1, -1] / (r[0, -1] + r[2, -1] - r[1, -1])).item() * 100) < 1e-9
        exp_miou = np.mean([(r[1, i] / (r[0, i] + r[2, i] - r[1, i])).item() for i in range(16)]) * 100
        assert abs(miou - exp_miou) < 1e-9


def test_iou_counts_binary_and_empty(hip):
    m = MeanIoU([1], 0, ['occupied'], True, 0)
    m.reset()
    e = torch.zeros(0, dtype=torch.int32, device=D0)
    m._after_step(e, e)
    assert int(m.counts.sum()) == 0
    p = torch.tensor([1, 1, 0, 0, 1], dtype=torch.int32, device=D0)
    t = torch.tensor([1, 0, 0, 1, 1], dtype=torch.int32, device=D0)
    m._after_step(p, t)
    assert m.counts.cpu().tolist() == [[3, 3], [2, 2], [3, 3]]


# ---------------------------------------------------------------------------------------------------------------------
# The class lookup (so_team_lookup: 8 lanes per point, lane j owns channels j, j + 8, ...) on inputs where float32
# arithmetic is exact — integer values on a small grid, coordinates on a dyadic lattice — so that tied maxima survive the
# interpolation and the first-maximum rule across lanes and rounds decides the result; channel counts below, at and
# above the team width, so that lanes without a channel exist.
# ---------------------------------------------------------------------------------------------------------------------
CHANNELS = [1, 2, 7, 8, 9, 17, 32]
GRID = (5, 9, 3)


def _first_max(v):
    """index of the first maximum along the last axis, without relying on argmax's tie rule"""
    idx = torch.arange(v.shape[-1]).expand_as(v)
    return torch.where(v == v.max(dim=-1, keepdim=True).values, idx, torch.full_like(idx, v.shape[-1])).min(dim=-1).values


_EXACT = {}


def _exact_resample_case(C):
    """(grid, logits, coords, sampled, sampled logits, first-maximum class): integers in [-2, 2] on a 5 x 9 x 3 grid, every
    multiple of 1 / 16 from -4 / 16 to 20 / 16 per axis (15 625 points = 488 x 32 + 9, some in the zero padding).
    Plain torch on the CPU, computed once per C; float32 grid_sample equals float64 bit for bit on these inputs."""
    if C not in _EXACT:
        g = torch.Generator().manual_seed(100 + C)
        grid = torch.randint(-2, 3, GRID, generator=g).float()
        logits = torch.randint(-2, 3, GRID + (C,), generator=g).float()
        ax = torch.arange(-4, 21, dtype=torch.float32) / 16
        coords = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), dim=-1).contiguous()       # along (H, W, D)
        gs = (coords[..., [2, 1, 0]] * 2 - 1)[None]
        sampled = F.grid_sample(grid[None, None], gs, mode='bilinear', align_corners=True)[0, 0]
        sl = F.grid_sample(logits.permute(3, 0, 1, 2)[None], gs, mode='bilinear', align_corners=True)[0]
        for a32, src in ((sampled, grid[None, None]), (sl, logits.permute(3, 0, 1, 2)[None])):
            a64 = F.grid_sample(src.double(), gs.double(), mode='bilinear', align_corners=True)
            assert torch.equal(a32.double().reshape(-1), a64.reshape(-1))
        sl = sl.permute(1, 2, 3, 0).contiguous()
        cls = _first_max(sl)
        assert torch.equal(torch.argmax(sl, dim=-1), cls)          # torch.argmax returns the first maximum too
        _EXACT[C] = (grid, logits, coords, sampled, sl, cls)
    return _EXACT[C]


def test_exact_cases_have_ties():
    """the inputs do what they are for: at C = 17 a large share of the points has a tied maximum, away from the padding too"""
    _, _, coords, _, sl, _ = _exact_resample_case(17)
    tied = ((sl == sl.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1)
    inside = ((coords > 0) & (coords < 1)).all(dim=-1)
    padded_out = (sl == 0).all(dim=-1)                      # every corner in the zero padding: a tie of another kind
    assert tied.float().mean() > 0.3 and (tied & ~padded_out).float().mean() > 0.15 and tied[inside].float().mean() > 0.1
    assert (~inside).any() and padded_out.any()


CROPS = [(0, 0, 0, 0, 0, 0), (1, 2, 3, 0, 0, 4), (13, 12, 0, 0, 0, 0)]      # the last one empties the first axis


@pytest.mark.parametrize("permute_lut", [False, True], ids=["identity_lut", "permuted_lut"])
@pytest.mark.parametrize("C", CHANNELS)
def test_occ_resample_exact_ties_and_thresholds(hip, C, permute_lut):
    grid, logits, coords, sampled, sl, cls = _exact_resample_case(C)
    lut = torch.randperm(C, generator=torch.Generator().manual_seed(C)).tolist() if permute_lut else list(range(C))
    thresh = 0.5
    assert (sampled == thresh).any() and (sampled < thresh).any() and (sampled > thresh).any()
    n = coords.shape[0]
    gd, cd, ld = grid.to(D0), coords.to(D0), logits.to(D0)
    for density in (False, True):
        for crop in CROPS:
            occ = ((sampled >= thresh) if density else (sampled <= thresh)).to(torch.int32)
            occ[:crop[0]] = 0
            occ[n - crop[1]:] = 0
            occ[:, :crop[2]] = 0
            occ[:, n - crop[3]:] = 0
            occ[:, :, :crop[4]] = 0
            occ[:, :, n - crop[5]:] = 0
            sem = occ * torch.tensor(lut, dtype=torch.int32)[cls]
            got = occ_resample(gd, cd, thresh, logits=ld, lut=lut, crop=crop, density=density, want_sampled=True)
            assert torch.equal(got['sampled'].cpu(), sampled), (density, crop)
            assert torch.equal(got['occ'].cpu(), occ), (density, crop)
            assert torch.equal(got['sem'].cpu(), sem), (density, crop)
            assert (occ.sum() == 0) == (crop == CROPS[2])


def test_occ_resample_too_many_classes_raises(hip):
    grid, _, coords, _, _, _ = _exact_resample_case(1)
    logits = torch.zeros(GRID + (33,))
    with pytest.raises(SelfOccHipError, match="33"):
        occ_resample(grid.to(D0), coords.to(D0), 0.5, logits=logits.to(D0), lut=list(range(33)))


def _exact_volume(n_rgb, n_sem, feat_dtype, seed):
    """5 x 9 x 3 voxels over 8 m x 16 m x 4 m (a voxel is 2 m), integer SDF and logits; the colour channels and three pad
    channels past n_rgb + n_sem hold 64, which would win every arg-max if a lane read them"""
    mapping = GridMeterMapping(nonlinear_mode='linear', h_size=[4, 0], h_range=[8.0, 0], h_half=True, w_size=[8, 0],
                               w_range=[16.0, 0], w_half=True, d_size=[2, 0], d_range=[0.0, 4.0, 4.0])
    assert (mapping.size_h, mapping.size_w, mapping.size_d) == GRID
    g = torch.Generator().manual_seed(seed)
    sdf = torch.randint(-2, 3, GRID, generator=g).float()
    feat = torch.full(GRID + (n_rgb + n_sem + 3,), 64.0)
    feat[..., n_rgb:n_rgb + n_sem] = torch.randint(-2, 3, GRID + (n_sem,), generator=g).float()
    return SDFVolume(mapping, sdf, feat.to(feat_dtype), n_rgb, n_sem)


def _exact_lattice():
    """metres whose grid coordinates are multiples of 1 / 4 (h, d) and 1 / 2 (w): voxel centres, cell midpoints, and a
    margin outside the volume; 21 x 19 x 11 = 4 389 points = 137 x 32 + 5"""
    ys = torch.arange(-2, 19, dtype=torch.float32) * 0.5
    xs = torch.arange(-1, 18, dtype=torch.float32)
    zs = torch.arange(-1, 10, dtype=torch.float32) * 0.5
    return torch.stack(torch.meshgrid(xs, ys, zs, indexing='ij'), dim=-1).reshape(-1, 3).contiguous()


@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_rgb", [0, 3])
@pytest.mark.parametrize("n_sem", CHANNELS)
def test_field_query_exact_ties(hip, n_sem, n_rgb, feat_dtype):
    vol = _exact_volume(n_rgb, n_sem, feat_dtype, seed=10 * n_sem + n_rgb)
    assert vol.feat.shape[3] > n_rgb + n_sem
    xyz = _exact_lattice()
    h = tp.field_lookup(vol.mapping, vol.to_reference_layout(), xyz)
    h64 = tp.field_lookup(vol.mapping, vol.to_reference_layout().double(), xyz.double())
    assert torch.equal(h.double(), h64)                             # the reference itself is exact on these inputs
    ref_logits = h[:, 1 + n_rgb:]
    assert ref_logits.shape[1] == n_sem and ref_logits.abs().max() <= 2
    cls = _first_max(ref_logits)
    assert torch.equal(torch.argmax(ref_logits, dim=-1), cls)
    if n_sem >= 7:
        assert ((ref_logits == ref_logits.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).float().mean() > 0.15
    got = field_query(vol.to(D0), xyz.to(D0), want_sdf=True, want_logits=True, want_argmax=True)
    assert torch.equal(got['sdf'].cpu(), h[:, 0])
    assert torch.equal(got['logits'].cpu(), ref_logits)
    assert torch.equal(got['argmax'].cpu().long(), cls)


def test_field_query_too_many_classes_raises(hip):
    vol = _exact_volume(0, 33, torch.float32, seed=0)
    with pytest.raises(SelfOccHipError, match="33"):
        field_query(vol.to(D0), _exact_lattice().to(D0), want_logits=True, want_argmax=True)
