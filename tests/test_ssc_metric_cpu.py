"""CPU: the committed fixture tests/golden/ssc_metric.npz (the reference's IoU, SSCMetrics and MeanIoU on synthetic
frames, tests/golden/make_golden_ssc_metric.py) agrees with a numpy restatement of the counts and of the get_stats /
_after_epoch formulas; the LUT constants of selfocc_amd/ssc_metric.py equal the reference's tables; the
so_ssc_metric_args mirror matches the header; the new entry points reject bad arguments before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from selfocc_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "ssc_metric.npz"))
KITTI_SHAPES = [(256, 256, 32), (64, 48, 16), (40, 36, 10), (24, 20, 8)]
LUT = np.array([9, 11, 13, 13, 14, 18, 19, 19, 15, 17, 0, 6, 7, 1, 4, 5, 5, 3, 2])


def sdf_of(q):
    return np.where(q == -128, np.float32(np.nan), q.astype(np.float32) * np.float32(0.25))


def unpack(bits, shape):
    return np.unpackbits(bits, count=int(np.prod(shape))).reshape(shape).astype(bool)


def kitti_pred(q):
    """(sdf <= 0) with the crops d >= D - 4, the last 6 h, the first / last 6 w"""
    with np.errstate(invalid='ignore'):
        p = (sdf_of(q) <= 0).astype(np.int64)
    D = q.shape[2]
    p[..., D - 4:] = 0
    p[-6:] = 0
    p[:, :6] = 0
    p[:, -6:] = 0
    return p


def ssc_counts(p, t, n_classes, sem_mask, comp_mask):
    """completion (tp, fp, fn) over comp_mask and per-class (tp, fp, fn) over sem_mask of the binned form"""
    tt, pp = t[comp_mask], p[comp_mask]
    comp = np.array([np.sum((tt > 0) & (pp > 0)), np.sum((tt <= 0) & (pp > 0)), np.sum((tt > 0) & (pp <= 0))])
    tt, pp = t[sem_mask], p[sem_mask]
    sem = np.zeros((3, n_classes), np.int64)
    for j in range(n_classes):
        sem[:, j] = [np.sum((tt == j) & (pp == j)), np.sum((tt != j) & (pp == j)), np.sum((tt == j) & (pp != j))]
    return comp, sem


def stats(comp, sem):
    """SSCMetrics.get_stats in float32"""
    tp, fp, fn = comp.astype(np.float32)
    s = sem.astype(np.float32)
    iou_ssc = s[0] / (s[0] + s[1] + s[2] + np.float32(1e-5))
    return dict(precision=tp / (tp + fp), recall=tp / (tp + fn), iou=tp / (tp + fp + fn), iou_ssc=iou_ssc,
                iou_ssc_mean=np.mean(iou_ssc[1:], dtype=np.float64))


def test_kitti_frames_agree_with_a_numpy_restatement():
    iou = np.zeros(3, np.int64)
    comp, sem = np.zeros(3, np.int64), np.zeros((3, 2), np.int64)
    miou = np.zeros((3, 20), np.int64)
    for k, shape in enumerate(KITTI_SHAPES):
        q, lab, s = GOLD[f'f{k}.sdf_q'], GOLD[f'f{k}.gt'], GOLD[f'f{k}.sem']
        assert q.shape == lab.shape == s.shape == shape
        p = kitti_pred(q)
        assert np.array_equal(unpack(GOLD[f'f{k}.occ'], shape), p.astype(bool))
        t = np.flip(lab, 1).astype(np.int64)
        occ = (t != 0) & (t != 255)
        d = np.nonzero(occ)[2]
        assert list(GOLD[f'f{k}.d_range']) == ([d.min(), d.max()] if d.size else [-1, -1])
        iou += [occ.sum(), p[occ].sum(), p.sum()]
        c, m = ssc_counts(p, t, 2, t != 255, t != 255)
        comp += c
        sem += m
        pm, valid = p * LUT[s.astype(np.int64)], t != 255
        tv, pv = t[valid], pm[valid]
        for j, c in enumerate(range(1, 20)):
            miou[:, j] += [np.sum(tv == c), np.sum((tv == c) & (pv == c)), np.sum(pv == c)]
        miou[:, 19] += [np.sum(tv != 0), np.sum((tv != 0) & (pv != 0)), np.sum(pv != 0)]
        for i, name in enumerate(('total_seen', 'total_correct', 'total_positive')):
            assert GOLD[f'after{k}.iou.{name}'][0] == iou[i], (k, name)
            assert np.array_equal(GOLD[f'after{k}.miou.{name}'], miou[i]), (k, name)
        for i, name in enumerate(('completion_tp', 'completion_fp', 'completion_fn')):
            assert GOLD[f'after{k}.ssc.{name}'][0] == comp[i], (k, name)
        for i, name in enumerate(('tps', 'fps', 'fns')):
            assert np.array_equal(GOLD[f'after{k}.ssc.{name}'], sem[i]), (k, name)
    assert KITTI_SHAPES[0] == (256, 256, 32) and list(GOLD['f3.d_range']) == [-1, -1]
    f = iou.astype(np.float32)
    assert GOLD['kitti.iou_epoch'] == float(f[1] / ((f[0] + f[2]) - f[1])) * 100       # f32 iou, .item(), * 100
    ref = stats(comp, sem)
    for key in ('precision', 'recall', 'iou', 'iou_ssc'):
        assert np.array_equal(GOLD[f'kitti.stats.{key}'].reshape(-1), np.atleast_1d(ref[key])), key
    assert np.isclose(GOLD['kitti.stats.iou_ssc_mean'], ref['iou_ssc_mean'], rtol=1e-6)


def test_ssc20_direct_coords_and_occ3d_agree_with_a_numpy_restatement():
    comp, sem = np.zeros(3, np.int64), np.zeros((3, 20), np.int64)
    for k in range(2):
        p, t = GOLD[f's{k}.pred'].astype(np.int64), GOLD[f's{k}.gt'].astype(np.int64)
        ne, ns = unpack(GOLD[f's{k}.nonempty'], t.shape), unpack(GOLD[f's{k}.nonsurface'], t.shape)
        assert p.max() >= 20 and t.max() == 255 and (t[t != 255] >= 20).any()     # labels outside the bins
        c, m = ssc_counts(p, t, 20, (t != 255) & ne, (t != 255) & ne & ns)
        comp += c
        sem += m
        for i, name in enumerate(('completion_tp', 'completion_fp', 'completion_fn')):
            assert GOLD[f's{k}.after.{name}'][0] == comp[i]
        for i, name in enumerate(('tps', 'fps', 'fns')):
            assert np.array_equal(GOLD[f's{k}.after.{name}'], sem[i])
    ref = stats(comp, sem)
    for key in ('precision', 'recall', 'iou', 'iou_ssc'):
        assert np.array_equal(GOLD[f'ssc20.stats.{key}'].reshape(-1), np.atleast_1d(ref[key])), key
    # get_score_* with nonempty=None: t == 255 counts as (t, p) = (0, 0)
    p, t = GOLD['s0.pred'].astype(np.int64), GOLD['s0.gt'].astype(np.int64)
    p, t = np.where(t == 255, 0, p), np.where(t == 255, 0, t)
    every = np.ones(t.shape, bool)
    c, m = ssc_counts(p, t, 20, every, every)
    assert np.array_equal(GOLD['direct.completion'], c) and np.array_equal(GOLD['direct.semantic'], m)
    seen = correct = positive = 0
    for k in range(2):
        out, co = GOLD[f'c{k}.outputs'].astype(np.int64), GOLD[f'c{k}.coords']
        assert len(np.unique(co, axis=0)) < len(co)                               # duplicated rows
        seen, correct, positive = seen + len(co), correct + out[tuple(co.T)].sum(), positive + out.sum()
        assert [GOLD[f'c{k}.after.{n}'][0] for n in ('total_seen', 'total_correct', 'total_positive')] == \
            [seen, correct, positive]
    for tag in ('plain', 'masked'):
        acc = np.zeros(3, np.int64)
        for k in range(2):
            sems, shape = GOLD[f'o{k}.semantics'], (200, 200, 16)
            out = unpack(GOLD[f'o{k}.outputs'], shape).astype(np.int64)
            m = unpack(GOLD[f'o{k}.mask'], shape) if tag == 'masked' else np.ones(shape, bool)
            acc += [np.sum((sems != 17) & m), out[(sems != 17) & m].sum(), out[m].sum()]
            assert [GOLD[f'o{k}.{tag}.{n}'][0] for n in ('total_seen', 'total_correct', 'total_positive')] == list(acc)


def test_lut_constants_equal_the_reference_tables():
    from selfocc_amd.ssc_metric import CITYSCAPES2SEMANTICKITTI, KITTI_CROP
    from selfocc_amd.occ import OPENSEED2NUSCENES
    assert list(GOLD['lut.cityscapes2semantickitti']) == CITYSCAPES2SEMANTICKITTI == list(LUT)
    assert list(GOLD['lut.openseed2nuscenes']) == OPENSEED2NUSCENES
    assert KITTI_CROP == (0, 6, 6, 6, 0, 4)


def test_ssc_metric_args_layout_and_abi_version_match_header(tmp_path):
    fields = [f for f, _ in abi.SoSscMetricArgs._fields_]
    body = "\n".join(f'printf("%zu %zu\\n", sizeof(so_ssc_metric_args), offsetof(so_ssc_metric_args, {f}));'
                     for f in fields)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{ROOT}/include/selfocc_hip.h"\n'
                   f'int main(void) {{ {body} return 0; }}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split()
    for k, f in enumerate(fields):
        assert int(lines[2 * k]) == C.sizeof(abi.SoSscMetricArgs), f
        assert int(lines[2 * k + 1]) == getattr(abi.SoSscMetricArgs, f).offset, f
    assert abi.ABI_VERSION == 35


def _valid():
    a = abi.SoSscMetricArgs()
    a.H, a.W, a.D = 4, 4, 4
    a.gt, a.gt_dtype = 0x1000, abi.LBL_F32
    a.pred, a.pred_dtype = 0x2000, abi.LBL_I32
    a.iou, a.bad, a.coords, a.n_coords = 0x3000, 0x4000, 0x5000, 7
    a.iou_ignore = -1
    return a


@pytest.mark.parametrize("case, entry, text", [
    ("null_args", "selfocc_ssc_metric", "args is NULL"),
    ("huge", "selfocc_ssc_metric", "2^31"),
    ("no_gt", "selfocc_ssc_metric", "gt is NULL"),
    ("bad_gt_dtype", "selfocc_ssc_metric", "gt_dtype"),
    ("pred_and_sdf", "selfocc_ssc_metric", "exactly one of pred / sdf"),
    ("f32_pred", "selfocc_ssc_metric", "pred_dtype"),
    ("classes", "selfocc_ssc_metric", "n_classes"),
    ("miou_no_sem", "selfocc_ssc_metric", "miou needs sem"),
    ("d_range_no_ws", "selfocc_ssc_metric", "d_range needs ws"),
    ("nothing", "selfocc_ssc_metric", "no output"),
    ("neg_crop", "selfocc_ssc_metric", "negative crop"),
    ("coords_null", "selfocc_iou_coords", "coords is NULL"),
    ("coords_no_bad", "selfocc_iou_coords", "iou / bad is NULL"),
    ("coords_huge", "selfocc_iou_coords", "2^31"),
])
def test_bad_arguments_are_rejected_before_any_launch(case, entry, text):
    from selfocc_amd._lib import lib
    a = _valid()
    if case == "huge" or case == "coords_huge":
        a.H = a.W = a.D = 1300
    elif case == "no_gt":
        a.gt = None
    elif case == "bad_gt_dtype":
        a.gt_dtype = 7
    elif case == "pred_and_sdf":
        a.sdf = 0x6000
    elif case == "f32_pred":
        a.pred_dtype = abi.LBL_F32
    elif case == "classes":
        a.semantic, a.n_classes = 0x7000, 300
    elif case == "miou_no_sem":
        a.miou = 0x7000
    elif case == "d_range_no_ws":
        a.d_range = 0x7000
    elif case == "nothing":
        a.iou = None
    elif case == "neg_crop":
        a.crop[3] = -1
    elif case == "coords_null":
        a.coords = None
    elif case == "coords_no_bad":
        a.bad = None
    rc = getattr(lib(), entry)(None if case == "null_args" else a, None)
    assert rc < 0
    assert text in lib().selfocc_last_error().decode(), lib().selfocc_last_error()
