"""CPU: the lane maps of the three products in csrc/camera_se.hip, replayed in numpy.  `mfma` places operands and results as
v_mfma_f32_16x16x4_f32 does (A[l & 15][l >> 4], B[l >> 4][l & 15], D row 4 (l >> 4) + r, column l & 15); the loops below index
global memory and LDS exactly as the kernels' lanes do, for one wave (forward, dgrad) / one block (wgrad) on a partial tile
(23 pixels: not a multiple of 4 or 16), and must give the plain matrix products."""
import numpy as np

C, M, HW = 32, 32, 23
MP, GP, XP = M + 4, C + 16, 68


def mfma(a, b, acc):
    A, Bm = np.zeros((16, 4)), np.zeros((4, 16))
    for l in range(64):
        A[l & 15][l >> 4] = a[l]
        Bm[l >> 4][l & 15] = b[l]
    D = A @ Bm
    for l in range(64):
        for r in range(4):
            acc[l][r] += D[4 * (l >> 4) + r][l & 15]


def _data():
    rng = np.random.default_rng(0)
    Wg, x, g = rng.standard_normal((C, M)), rng.standard_normal((M, HW)), rng.standard_normal((HW, C))
    wl = np.zeros(C * MP)
    for c in range(C):
        wl[c * MP:c * MP + M] = Wg[c]
    return Wg, x, g, wl


def test_forward_lane_map():
    Wg, x, _, wl = _data()
    CT, out = C // 16, np.zeros((HW, C))
    acc = np.zeros((CT, 4, 64, 4))
    for kk in range(M // 4):
        cur = np.zeros((64, 4))
        for l in range(64):
            m, q = l & 15, l >> 4
            for j in range(4):
                if 4 * m + j < HW:
                    cur[l][j] = x[4 * kk + q][4 * m + j]
        for ct in range(CT):
            av = np.array([wl[(l & 15) * MP + 4 * kk + (l >> 4) + ct * 16 * MP] for l in range(64)])
            for j in range(4):
                mfma(av, cur[:, j], acc[ct][j])
    for l in range(64):
        m, q = l & 15, l >> 4
        for j in range(4):
            if 4 * m + j < HW:
                for ct in range(CT):
                    out[4 * m + j][ct * 16 + 4 * q:ct * 16 + 4 * q + 4] = acc[ct][j][l]
    assert np.abs(out - (Wg @ x).T).max() < 1e-12


def test_dgrad_lane_map():
    Wg, _, g, wl = _data()
    MT = M // 16
    acc = np.zeros((MT, 4, 64, 4))
    for cc in range(C // 16):
        cur = np.zeros((4, 64, 4))
        for j in range(4):
            for l in range(64):
                m, q = l & 15, l >> 4
                if 16 * j + m < HW:
                    cur[j][l] = g[16 * j + m][16 * cc + 4 * q:16 * cc + 4 * q + 4]
        for r in range(4):
            for kt in range(MT):
                bv = np.array([wl[(16 * cc + 4 * (l >> 4) + r) * MP + (l & 15) + kt * 16] for l in range(64)])
                for j in range(4):
                    mfma(cur[j][:, r], bv, acc[kt][j])
    dx = np.zeros((M, HW))
    for l in range(64):
        m, q = l & 15, l >> 4
        for j in range(4):
            for kt in range(MT):
                for r in range(4):
                    if 16 * j + 4 * q + r < HW:
                        dx[16 * kt + m][16 * j + 4 * q + r] = acc[kt][j][l][r]
    assert np.abs(dx - Wg.T @ g.T).max() < 1e-12


def test_wgrad_lane_map():
    _, x, g, _ = _data()
    gs, xs = np.zeros(64 * GP), np.zeros(M * XP)
    for p in range(HW):
        gs[p * GP:p * GP + C] = g[p]
    for k in range(M):
        xs[k * XP:k * XP + HW] = x[k]
    CT2, MT2, dw = C // 32, M // 32, np.zeros((C, M))
    for wave in range(4):
        c_base, k_base = (wave & 1) * (C // 2), (wave >> 1) * (M // 2)
        acc = np.zeros((CT2, MT2, 64, 4))
        for s in range(16):
            for ct in range(CT2):
                av = np.array([gs[(4 * s + (l >> 4)) * GP + c_base + 16 * ct + (l & 15)] for l in range(64)])
                for kt in range(MT2):
                    bv = np.array([xs[(k_base + 16 * kt + (l & 15)) * XP + 4 * s + (l >> 4)] for l in range(64)])
                    mfma(av, bv, acc[ct][kt])
        for l in range(64):
            m, q = l & 15, l >> 4
            for ct in range(CT2):
                for kt in range(MT2):
                    for r in range(4):
                        dw[c_base + 16 * ct + 4 * q + r][k_base + 16 * kt + m] = acc[ct][kt][l][r]
    assert np.abs(dw - g.T @ x.T).max() < 1e-12
