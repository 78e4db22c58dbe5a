"""Case table, float64 reference, float32 yardstick and a numpy float32 model of the fused CameraAwareSE flatten
(csrc/camera_se.hip), for tests/test_camera_se_sharp_cpu.py and tests/test_camera_se_sharp_gpu.py.

Shapes: all seven (C, M) pairs selfocc_camera_se_supported accepts, at (B, N) = (2, 3), on level sets whose pixel counts sit on
the kernels' own edges (the 64-pixel wave slice / wgrad step, the 256-pixel block tile, the 512-pixel wgrad chunk, hw % 4 for the
float4 path).  Two input families per case, drawn in float64 from a seeded CPU generator and rounded to float32 once:
  exact    small integers and eighths: every product and partial sum is a multiple of 1/8 below 2^24 / 8, so float32 gives the
           float64 result in ANY summation order; the kernels must reproduce the reference bit for bit;
  random   gate = sigmoid(randn), w = randn / sqrt(M), the rest randn.

Error unit: per tensor, e(t) = max over elements of |t - f64| / (2^-24 A), A = the same formula evaluated on absolute values
(the per-element sum of |terms|).  The bound of a tensor in a case is K[t] max(e(port32), 1): port32 is the float32 torch CPU
evaluation of the same formulas in that case, in plain ascending order (see port32 for why not einsum), K[t] the smallest of 2, 4, 8 that admits the kernel-order model below on every
case (test_camera_se_sharp_cpu.py recomputes it).

The model restates the kernels' summation order, not their lane maps (those: test_camera_se_lanemap_cpu.py): the forward's
k-ascending fmaf chain from (bias + cams) + lvls, the dgrad's chain in its step order c = 16 cc + 4 q + r (r outside q), the
wgrad's pixel-ascending chain inside 512-pixel chunks with the chunk partials added in ascending order, colsum as
camera_se_reduce_kernel adds it (64-pixel sums, chunk sums, batch outermost).  fmaf is the float64 product-sum rounded to
float32 (rounded twice: differs from fmaf only where the float64 sum falls exactly between two float32, ~2^-29 of all steps,
by one ulp; irrelevant for a figure that is a maximum over elements and exact on the exact family)."""
import collections
import functools
import zlib

import numpy as np
import torch

f32, f64 = np.float32, np.float64
U = 2.0 ** -24

CS_TILE, CS_CHUNK, CS_STEP = 256, 512, 64

PAIRS = ((32, 32), (32, 64), (64, 64), (64, 128), (96, 96), (96, 192), (128, 128))

LEVELS = {
    # hw = 1, 2, 3, 63, 64, 65, 255, 257: odd level starts, float4 (64) and scalar levels, both sides of the wave slice and the tile
    'EDGE8': ((1, 1), (1, 2), (1, 3), (7, 9), (8, 8), (5, 13), (15, 17), (1, 257)),
    # hw = 256, 511, 512, 513: a full tile, a chunk one pixel short, a full chunk, a chunk plus one pixel
    'CHUNK4': ((16, 16), (7, 73), (16, 32), (19, 27)),
    # 1025 pixels: five tiles, three chunks, one pixel in the last wave slice
    'ONE': ((25, 41),),
    'PIXEL': ((1, 1),),
}

Case = collections.namedtuple('Case', 'C M B N levels')
CASES = tuple(
    [Case(C, M, 2, 3, s) for C, M in PAIRS for s in ('EDGE8', 'CHUNK4')]
    + [Case(64, 128, 2, 3, 'ONE'), Case(96, 96, 2, 3, 'ONE'), Case(32, 32, 2, 3, 'PIXEL'), Case(128, 128, 2, 3, 'PIXEL'),
       Case(96, 192, 1, 1, 'EDGE8')])
FAMILIES = ('exact', 'random')
RAW = ('out', 'dx', 'dWc', 'colsum')
FOLDED = ('g_gate', 'g_w', 'g_bias', 'g_cam', 'g_lvl')
TENSORS = RAW + FOLDED

# the smallest of 2, 4, 8 admitting the kernel-order model on every case (test_camera_se_sharp_cpu.py asserts these are that).
# Worst model / max(e(port32), 1): out 4.16 (c96m192 EDGE8: the kernel's chain STARTS at bias + cams + lvls, so every one of its M
# roundings is relative to a sum that carries the embeddings; port32 adds them last), dx 1.75, every other tensor <= 1.00.
# Model / bound, worst: out 0.52, dx 0.87, dWc 0.50, colsum 0.50, g_gate 0.45, the other folds 0.50.  Worst e(port32): out 4.71,
# dx 6.24, dWc 6.49, colsum 2.09, g_gate 2.27, g_w 3.61, g_bias 1.22, g_cam 1.17, g_lvl 2.09.  The precision defects are at
# least 82 x (10-bit mantissa, dWc) and 350 x (bfloat16, dWc) the bound on every raw tensor of every case.
K = {'out': 8, 'dx': 2, 'dWc': 2, 'colsum': 2, 'g_gate': 2, 'g_w': 2, 'g_bias': 2, 'g_cam': 2, 'g_lvl': 2}

INDEX_DEFECTS = ('gate_row', 'lvl_neighbour', 'cams_next', 'drop_last_pixel', 'drop_last_k', 'drop_last_step', 'colsum_row_past')
PRECISION_DEFECTS = ('bf16_operand', 'mant10_operand')


def case_id(c):
    return f'c{c.C}m{c.M}-b{c.B}n{c.N}-{c.levels}'


def hws(c):
    return [h * w for h, w in LEVELS[c.levels]]


def case_bytes(c):
    """the largest tensor of a case (the maps), in bytes"""
    return 4 * c.B * c.N * sum(hws(c)) * max(c.C, c.M)


def chunks_of(hw, per=CS_CHUNK):
    return [(p, min(hw, p + per)) for p in range(0, hw, per)]


def make_inputs(c, family):
    """dict of float32 CPU tensors: gate (B N, M), w (C, M), bias (C), cams (N, C), lvls (L, C), maps [(B, N, M, h, w)],
    g (N, S, B, C)"""
    gen = torch.Generator().manual_seed(zlib.crc32(f'{case_id(c)}/{family}'.encode()))
    lv, S = LEVELS[c.levels], sum(hws(c))
    BN = c.B * c.N
    if family == 'exact':
        ints = lambda *s: torch.randint(-4, 5, s, generator=gen).double()
        gate = torch.randint(1, 9, (BN, c.M), generator=gen).double() / 8.0
        w, bias, cams, lvls = ints(c.C, c.M), ints(c.C), ints(c.N, c.C), ints(len(lv), c.C)
        maps = [ints(c.B, c.N, c.M, h, ww) for h, ww in lv]
        g = ints(c.N, S, c.B, c.C)
    else:
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
        gate = torch.sigmoid(rn(BN, c.M))
        w, bias, cams, lvls = rn(c.C, c.M) / c.M ** 0.5, rn(c.C), rn(c.N, c.C), rn(len(lv), c.C)
        maps = [rn(c.B, c.N, c.M, h, ww) for h, ww in lv]
        g = rn(c.N, S, c.B, c.C)
    return dict(gate=gate.float(), w=w.float(), bias=bias.float(), cams=cams.float(), lvls=lvls.float(),
                maps=[m.float() for m in maps], g=g.float())


def _permuted(inp, order):
    """the inputs with the three reduction axes (map channels k, output channels c, pixels of every level) reordered, and the
    function that puts an evaluate() result back into the original order.  order: 'reversed' or a seed."""
    C, M = inp['w'].shape
    if order == 'reversed':
        perm = lambda n: torch.arange(n - 1, -1, -1)
    else:
        gen = torch.Generator().manual_seed(int(order))
        perm = lambda n: torch.randperm(n, generator=gen)
    pc, pk = perm(C), perm(M)
    pp = [perm(m.shape[3] * m.shape[4]) for m in inp['maps']]
    starts = np.cumsum([0] + [len(p) for p in pp])
    ps = torch.cat([p + int(s) for p, s in zip(pp, starts)])
    q = dict(gate=inp['gate'][:, pk], w=inp['w'][pc][:, pk], bias=inp['bias'][pc], cams=inp['cams'][:, pc], lvls=inp['lvls'][:, pc],
             maps=[m.flatten(3)[:, :, pk][:, :, :, p].reshape(m.shape) for m, p in zip(inp['maps'], pp)],
             g=inp['g'][:, ps][:, :, :, pc])
    ic, ik, ips = torch.argsort(pc), torch.argsort(pk), torch.argsort(ps)

    def back(r):
        return dict(out=r['out'][:, ips][:, :, :, ic],
                    dx=[d.flatten(3)[:, :, ik][:, :, :, torch.argsort(p)].reshape(d.shape) for d, p in zip(r['dx'], pp)],
                    dWc=r['dWc'][:, ic][:, :, ik], colsum=r['colsum'][:, :, ic], g_gate=r['g_gate'][:, ik],
                    g_w=r['g_w'][ic][:, ik], g_bias=r['g_bias'][ic], g_cam=r['g_cam'][:, ic], g_lvl=r['g_lvl'][:, ic])
    return q, back


def fold(dWc, colsum, w, gate):
    """the five folded gradients of _CameraSeFlatten.backward from the kernels' raw outputs"""
    return dict(g_gate=(dWc * w).sum(1), g_w=(dWc * gate[:, None, :]).sum(0), g_bias=colsum.sum((0, 1)), g_cam=colsum.sum(0),
                g_lvl=colsum.sum(1))


def evaluate(inp, dtype, absolute=False, order=None):
    """the fold of DESIGN 3.13 in plain torch ops of `dtype` on the CPU: out (N, S, B, C), dx [(B, N, M, h, w)], dWc (B N, C, M),
    colsum (L, N, C) and the five folded gradients.  absolute: on |inputs|: the per-element sum of |terms| (A)."""
    if order is not None:
        q, back = _permuted(inp, order)
        return back(evaluate(q, dtype, absolute))
    cast = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    gate, w, bias, cams, lvls, g = (cast(inp[k]) for k in ('gate', 'w', 'bias', 'cams', 'lvls', 'g'))
    maps = [cast(m) for m in inp['maps']]
    B, N, M = maps[0].shape[:3]
    C = w.shape[0]
    Wg = w[None] * gate[:, None, :]                                              # (B N, C, M)
    outs, dxs, cols, dWc, s0 = [], [], [], torch.zeros(B * N, C, M, dtype=dtype), 0
    for l, x in enumerate(maps):
        xf = x.reshape(B * N, M, -1)
        hw = xf.shape[2]
        y = torch.einsum('ick,ikp->ipc', Wg, xf).unflatten(0, (B, N)) + bias     # (B, N, hw, C)
        outs.append((y + cams[None, :, None, :]) + lvls[l])
        gl = g[:, s0:s0 + hw].permute(2, 0, 1, 3).reshape(B * N, hw, C)
        dxs.append(torch.einsum('ipc,ick->ikp', gl, Wg).reshape(x.shape))
        dWc = dWc + torch.einsum('ipc,ikp->ick', gl, xf)
        cols.append(g[:, s0:s0 + hw].sum((1, 2)))
        s0 += hw
    r = dict(out=torch.cat(outs, 2).permute(1, 2, 0, 3).contiguous(), dx=dxs, dWc=dWc, colsum=torch.stack(cols))
    r.update(fold(r['dWc'], r['colsum'], w, gate))
    return r


def flat(v):
    """a tensor, a numpy array or a list of them (dx) as one float64 vector"""
    if isinstance(v, (list, tuple)):
        return np.concatenate([flat(t) for t in v])
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(f64).ravel()


def figures(got, ref, A, tensors=None):
    """e(t) per tensor: max |got - f64| / (2^-24 A).  Where A = 0 every term is zero: anything but 0 there is infinitely wrong."""
    e = {}
    for k in tensors or [k for k in TENSORS if k in got]:
        d, a = np.abs(flat(got[k]) - flat(ref[k])), flat(A[k])
        assert d.shape == a.shape, (k, d.shape, a.shape)
        if np.isnan(d).any():
            e[k] = float('inf')
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(a > 0, d / (U * a), np.where(d > 0, np.inf, 0.0))
        e[k] = float(q.max())
    return e


def _seq_sum(t, dim):
    """the sum over `dim` in ascending order, one float addition per step"""
    parts = t.unbind(dim)
    s = parts[0].clone()
    for q in parts[1:]:
        s = s + q
    return s


def port32(inp):
    """The yardstick: the same formulas in float32 torch ops on the CPU, every sum a plain ascending chain of separately rounded
    products and additions.  NOT einsum / matmul: what a BLAS does with a float32 sum depends on the host (threads, vector width).
    The einsum form of evaluate() measured e(dWc) = 1.85 on one host and 1.18 on another for the same case (c96m96, 1025 pixels),
    and a bound must not move with the host.  Elementwise float32 operations are the same everywhere."""
    gate, w, bias, cams, lvls, g = (inp[k].float() for k in ('gate', 'w', 'bias', 'cams', 'lvls', 'g'))
    maps = inp['maps']
    B, N, M = maps[0].shape[:3]
    C = w.shape[0]
    hw = [m.shape[3] * m.shape[4] for m in maps]
    S = sum(hw)
    Wg = w[None] * gate[:, None, :]                                              # (B N, C, M)
    x = torch.cat([m.float().reshape(B * N, M, -1) for m in maps], 2)            # (B N, M, S)
    gl = g.permute(2, 0, 1, 3).reshape(B * N, S, C)                              # (B N, S, C)
    acc = torch.zeros(B * N, C, S)
    for k in range(M):
        acc = acc + Wg[:, :, k, None] * x[:, None, k, :]
    lv = torch.cat([lvls[l][:, None].expand(C, h) for l, h in enumerate(hw)], 1)                       # (C, S)
    y = ((acc.unflatten(0, (B, N)) + bias[None, None, :, None]) + cams[None, :, :, None]) + lv          # (B, N, C, S)
    out = y.permute(1, 3, 0, 2).contiguous()
    acc = torch.zeros(B * N, M, S)
    for c in range(C):
        acc = acc + Wg[:, c, :, None] * gl[:, None, :, c]
    dWc = torch.zeros(B * N, C, M)
    for p in range(S):
        dWc = dWc + gl[:, p, :, None] * x[:, None, :, p]
    dx, cols, s0 = [], [], 0
    for m, h in zip(maps, hw):
        dx.append(acc[:, :, s0:s0 + h].reshape(m.shape))
        cols.append(_seq_sum(_seq_sum(g[:, s0:s0 + h], 1), 1))                  # pixels, then the batch: (N, C)
        s0 += h
    colsum = torch.stack(cols)
    r = dict(out=out, dx=dx, dWc=dWc, colsum=colsum, g_gate=_seq_sum(dWc * w, 1), g_w=_seq_sum(dWc * gate[:, None, :], 0),
             g_bias=_seq_sum(_seq_sum(colsum, 0), 0), g_cam=_seq_sum(colsum, 0), g_lvl=_seq_sum(colsum, 1))
    return r


def reference(inp):
    """(float64 reference, A, e(port32)) of a problem: compute once, share"""
    ref, A = evaluate(inp, torch.float64), evaluate(inp, torch.float64, absolute=True)
    return ref, A, figures(port32(inp), ref, A)


@functools.lru_cache(maxsize=None)
def problem(c, family):
    """(inputs, float64 reference, A, e(port32)) of a case: computed once per process, shared, never changed"""
    inp = make_inputs(c, family)
    return (inp, *reference(inp))


def bounds(yard, tensors=TENSORS):
    return {k: K[k] * max(yard[k], 1.0) for k in tensors}


def bits_differing(a, b):
    a, b = flat(a).astype(f32), flat(b).astype(f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' order in numpy float32
# ---------------------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    r = np.multiply(a, b, dtype=f64)
    r += c
    return r.astype(f32)


def _bf16(x):
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(f32)


def _mant10(x):
    return (np.ascontiguousarray(x, f32).view(np.uint32) & np.uint32(0xFFFFE000)).view(f32)


def _operand(x, defect):
    return _bf16(x) if defect == 'bf16_operand' else _mant10(x) if defect == 'mant10_operand' else x


def applies(defect, c):
    hw = hws(c)
    return {'gate_row': c.B > 1, 'lvl_neighbour': len(hw) > 1, 'cams_next': c.N > 1, 'drop_last_pixel': any(h % 4 for h in hw),
            'colsum_row_past': any(h % CS_STEP for h in hw[:-1])}.get(defect, True)


def _np(inp):
    B, N, M = inp['maps'][0].shape[:3]
    d = {k: inp[k].numpy() for k in ('gate', 'w', 'bias', 'cams', 'lvls')}
    d['x'] = np.concatenate([m.numpy().reshape(B * N, M, -1) for m in inp['maps']], 2)               # (B N, M, S)
    d['g'] = np.ascontiguousarray(inp['g'].numpy().transpose(2, 0, 1, 3)).reshape(B * N, -1, inp['w'].shape[0])   # (B N, S, C)
    d['hw'] = [m.shape[3] * m.shape[4] for m in inp['maps']]
    d['B'], d['N'] = B, N
    return d


def _weights(d, defect):
    """Wg (B N, C, M) as cs_stage_weights rounds it.  gate_row: the row of camera n instead of b N + n"""
    rows = np.arange(d['B'] * d['N'])
    if defect == 'gate_row':
        rows = rows % d['N']
    return d['w'][None] * d['gate'][rows][:, None, :]


def model_fwd(inp, defect=None):
    d = _np(inp)
    B, N, hw = d['B'], d['N'], d['hw']
    C, M = d['w'].shape
    Wg, x = _weights(d, defect), _operand(d['x'], defect).copy()
    cam = np.tile(d['cams'][(np.arange(N) + (defect == 'cams_next')) % N], (B, 1))                   # (B N, C)
    acc, s0 = np.empty((B * N, C, x.shape[2]), f32), 0
    for l, h in enumerate(hw):
        acc[:, :, s0:s0 + h] = ((d['bias'] + cam) + d['lvls'][l])[:, :, None]
        if defect == 'lvl_neighbour' and l > 0:          # the first tile of a level takes the level before it
            acc[:, :, s0:s0 + min(h, CS_TILE)] = ((d['bias'] + cam) + d['lvls'][l - 1])[:, :, None]
        if defect == 'drop_last_pixel' and h % 4:        # the ragged end of a scalar level is not loaded
            x[:, :, s0 + h - 1] = 0.0
        s0 += h
    for k in range(M - 4 if defect == 'drop_last_k' else M):
        acc = fma(Wg[:, :, k, None], x[:, None, k, :], acc)
    return np.ascontiguousarray(acc.reshape(B, N, C, -1).transpose(1, 3, 0, 2))                      # (N, S, B, C)


def model_dgrad(inp, defect=None):
    d = _np(inp)
    C, M = d['w'].shape
    Wg, g = _weights(d, defect), _operand(d['g'], defect)
    acc = np.zeros((g.shape[0], M, g.shape[1]), f32)
    for cc in range(C // 16):
        for r in range(4):
            for q in range(4):
                c = 16 * cc + 4 * q + r
                acc = fma(Wg[:, c, :, None], g[:, None, :, c], acc)
    out, s0 = [], 0
    for m in inp['maps']:
        h = m.shape[3] * m.shape[4]
        out.append(np.ascontiguousarray(acc[:, :, s0:s0 + h]).reshape(m.shape))
        s0 += h
    return out


def model_wgrad(inp, defect=None, want=('dWc', 'colsum')):
    """-> dWc (B N, C, M), colsum (L, N, C) through the chunk partials"""
    d = _np(inp)
    B, N, hw = d['B'], d['N'], d['hw']
    C, M = d['w'].shape
    x, g = d['x'], d['g']
    gc = _operand(g, defect)
    if 'dWc' in want:
        x = _operand(x, defect)
    dWc, colsum, s0 = np.zeros((B * N, C, M), f32), np.zeros((len(hw), N, C), f32), 0
    for l, h in enumerate(hw):
        part_c = []
        for p0, p1 in chunks_of(h):
            steps = [(q0, min(p1, q0 + CS_STEP)) for q0 in range(p0, p1, CS_STEP)]
            if defect == 'drop_last_step':
                steps = steps[:-1]
            acc, col = np.zeros((B * N, C, M), f32), np.zeros((B * N, C), f32)
            for q0, q1 in steps:
                if 'dWc' in want:
                    for p in range(s0 + q0, s0 + q1):
                        acc = fma(g[:, p, :, None], x[:, None, :, p], acc)
                if 'colsum' in want:
                    past = defect == 'colsum_row_past' and l + 1 < len(hw) and q1 == h and h % CS_STEP
                    s = np.zeros((B * N, C), f32)
                    for p in range(s0 + q0, s0 + q1 + (1 if past else 0)):
                        s = s + gc[:, p]
                    col = col + s
            dWc = dWc + acc                                  # chunk partials in ascending order, all levels
            part_c.append(col.reshape(B, N, C))
        s = np.zeros((N, C), f32)
        for b in range(B):                                   # batch outermost, then the level's chunks
            for col in part_c:
                s = s + col[b]
        colsum[l] = s
        s0 += h
    return dWc, colsum


def model(inp, defect=None, tensors=TENSORS):
    r = {}
    if 'out' in tensors:
        r['out'] = model_fwd(inp, defect)
    if 'dx' in tensors:
        r['dx'] = model_dgrad(inp, defect)
    want = [k for k in ('dWc', 'colsum') if k in tensors or (k == 'dWc' and {'g_gate', 'g_w'} & set(tensors))
            or (k == 'colsum' and {'g_bias', 'g_cam', 'g_lvl'} & set(tensors))]
    if want:
        dWc, colsum = model_wgrad(inp, defect, want)
        fo = fold(torch.from_numpy(dWc), torch.from_numpy(colsum), inp['w'], inp['gate'])
        r.update({k: v for k, v in dict(dWc=dWc, colsum=colsum, **fo).items() if k in tensors})
    return r
