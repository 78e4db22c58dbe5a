"""Host model of the dropout mask of csrc/dropout.hip, written from the documented algorithm (not by calling the kernel):

    z  = seed + idx * 0x9E3779B97F4A7C15                      (all arithmetic modulo 2^64)
    z  = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z  = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z ^= z >> 31                                               (splitmix64's finaliser of seed + idx * golden)
    u  = float32(z >> 40) * 2^-24                              (24 uniform bits in [0, 1): exact in float32)
    keep element idx  <=>  u >= float32(p)

numpy uint64 ARRAY arithmetic wraps around silently, which is the arithmetic the description asks for; nothing here uses a
uint64 scalar product (numpy warns on those).  tests/test_dropout_model_cpu.py checks that the model has the distribution the
kernel's header claims; tests/test_dropout_gpu.py holds the kernels to it element for element."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB
_CHUNK = 1 << 22


def _u64(v):
    return np.full(1, int(v) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)


def u_at(seed, idx):
    """The uniform float32 value in [0, 1) of every element index of `idx` (any integer array; taken modulo 2^64)."""
    idx = np.asarray(idx).astype(np.uint64)
    z = _u64(seed) + idx * _u64(GOLDEN)
    z = (z ^ (z >> np.uint64(30))) * _u64(MUL1)
    z = (z ^ (z >> np.uint64(27))) * _u64(MUL2)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def u_values(seed, n, start=0):
    """u of the indices start .. start + n - 1 as float32 (n,)."""
    out = np.empty(n, dtype=np.float32)
    for s in range(0, n, _CHUNK):                   # bounded temporaries at the 16 M element sizes of the GPU test
        e = min(n, s + _CHUNK)
        out[s:e] = u_at(seed, np.arange(start + s, start + e, dtype=np.uint64))
    return out


def keep(seed, n, p, start=0):
    """Boolean (n,): True where dropout with probability p keeps element start + i under `seed`."""
    return u_values(seed, n, start) >= np.float32(p)


def scale(p):
    """The factor of a kept element as the launcher computes it: float32(1) / (float32(1) - float32(p))."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))
