"""No GPU: what makes tests/test_dropout_gpu.py meaningful.  That module holds the dropout kernels to tests/dropout_model.py
element for element; this one shows that the model itself is a dropout mask — every element kept with probability 1 - p,
independently of its neighbours, of its column in the encoder's (-1, 96) activations and of the mask of the next seed — and
that the statistics used have the power to notice the defects a hash-of-index mask is prone to (power controls).

Every statistic is a z-score under the hypothesis "independent Bernoulli(1 - p)"; the bound is |z| <= 5.  Over the
5 seeds x 4 p x (1 + 9 + 1 + 96) scores of this module a true i.i.d. source would exceed it with probability ~1e-3; the
model's masks are fixed, so the outcome is the same on every run."""
import functools

import numpy as np
import pytest
import torch

import dropout_model as dm

N = 1 << 22
SEEDS = [0, 1, 5, 2 ** 63 - 1, 123456789012345]
PS = [0.1, 0.25, 0.5, 0.9]
LAGS = [1, 2, 3, 4, 7, 64, 96, 256, 1024]
Z_MAX = 5.0
IDX = np.arange(N, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _u(seed):
    return dm.u_values(seed, N)


def z_scores(k, k_other, p):
    """{name: z} of a boolean mask `k` (and the mask `k_other` of another seed) against independent Bernoulli(1 - p)."""
    p = float(np.float32(p))
    q, n = 1.0 - p, k.size
    z = {'keep rate': (k.mean(dtype=np.float64) - q) / np.sqrt(p * q / n)}
    c = k.astype(np.float64) - q                           # mean 0, variance p q under the hypothesis
    for lag in LAGS:                                       # products of independent centred terms: mean 0, variance (p q)^2
        z[f'lag {lag}'] = np.dot(c[:-lag], c[lag:]) / (p * q) / np.sqrt(n - lag)
    z['other seed'] = np.dot(c, k_other.astype(np.float64) - q) / (p * q) / np.sqrt(n)
    rows = n // 96
    col = k[:rows * 96].reshape(rows, 96).mean(0, dtype=np.float64)
    zc = (col - q) / np.sqrt(p * q / rows)
    z['column of 96'] = zc[np.argmax(np.abs(zc))]
    return z


def chi_square(u, bins=256):
    counts = np.bincount((u.astype(np.float64) * bins).astype(np.int64), minlength=bins)    # u * 256 is exact: u = m / 2^24
    e = u.size / bins
    return float(((counts - e) ** 2).sum() / e)


def chi_square_quantile(dof, upper):
    """x with P(chi^2_dof > x) = upper, by bisection on the regularised upper incomplete gamma function."""
    a = torch.tensor(dof / 2.0, dtype=torch.float64)
    lo, hi = float(dof), 10.0 * dof
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64)).item() > upper:
            lo = mid
        else:
            hi = mid
    return hi


CHI2_MAX = chi_square_quantile(255, 1e-6)


def test_chi_square_quantile_is_the_tabulated_one():
    assert abs(chi_square_quantile(255, 0.05) - 293.2478) < 1e-3            # standard table, 255 degrees of freedom
    assert abs(chi_square_quantile(1, 0.05) - 3.841459) < 1e-5
    assert 370.0 < CHI2_MAX < 385.0                                         # Wilson-Hilferty: 377.2


def test_u_is_a_24_bit_fraction_in_the_half_open_unit_interval():
    for seed in SEEDS:
        u = _u(seed)
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
        assert np.array_equal(u * np.float32(2 ** 24), np.floor(u * np.float32(2 ** 24)))
    assert np.array_equal(dm.u_values(5, 1000, start=12345), _u(5)[12345:13345])
    assert np.array_equal(dm.keep(5, 1000, 0.25, start=7), _u(5)[7:1007] >= np.float32(0.25))
    # the hash by hand for (seed, idx) = (0, 0) and in Python integers for a few large operands
    assert dm.u_at(0, [0])[0] == 0.0

    def by_hand(seed, idx):
        m = (1 << 64) - 1
        z = (seed + idx * dm.GOLDEN) & m
        z = ((z ^ (z >> 30)) * dm.MUL1) & m
        z = ((z ^ (z >> 27)) * dm.MUL2) & m
        z ^= z >> 31
        return np.float32(z >> 40) * np.float32(2.0 ** -24)
    for seed, idx in [(1, 0), (0, 1), (2 ** 63 - 1, 3), (123456789012345, 2 ** 24 + 6), (2 ** 32 + 17, 2 ** 31 + 5)]:
        assert dm.u_at(seed, [idx])[0] == by_hand(seed, idx)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("seed", SEEDS)
def test_model_mask_is_independent_bernoulli(seed, p):
    k, k1 = _u(seed) >= np.float32(p), _u(seed + 1) >= np.float32(p)
    z = z_scores(k, k1, p)
    print(f"seed {seed} p {p}: " + ", ".join(f"{n} {v:+.2f}" for n, v in z.items()))
    bad = {n: v for n, v in z.items() if not abs(v) <= Z_MAX}
    assert not bad, bad


@pytest.mark.parametrize("seed", sorted(set(SEEDS + [s + 1 for s in SEEDS])))
def test_model_u_is_uniform_over_256_bins(seed):
    x2 = chi_square(_u(seed))
    print(f"seed {seed}: chi-square {x2:.1f} (255 degrees of freedom, bound {CHI2_MAX:.1f})")
    assert x2 <= CHI2_MAX


def _failed(k, k_other, p):
    return {n for n, v in z_scores(k, k_other, p).items() if not abs(v) <= Z_MAX}


@pytest.mark.parametrize("p", PS)
def test_power_one_decision_per_group_of_four(p):
    """a mask drawn once per float4 group: the neighbours of a group are equal"""
    k = dm.u_at(5, IDX >> np.uint64(2)) >= np.float32(p)
    k1 = dm.u_at(6, IDX >> np.uint64(2)) >= np.float32(p)
    assert {'lag 1', 'lag 2', 'lag 3'} <= _failed(k, k1, p)


@pytest.mark.parametrize("p", PS)
def test_power_seed_truncated_to_32_bits(p):
    """two seeds equal in the low word give one mask: the correlation between the masks of two seeds is 1"""
    a, b = 123456789012345, 123456789012345 + (7 << 32)
    assert 'other seed' not in _failed(_u(a) >= np.float32(p), dm.keep(b, N, p), p)            # the model tells them apart
    ka, kb = dm.u_at(a & 0xFFFFFFFF, IDX) >= np.float32(p), dm.u_at(b & 0xFFFFFFFF, IDX) >= np.float32(p)
    assert 'other seed' in _failed(ka, kb, p)


@pytest.mark.parametrize("p", PS)
def test_power_index_truncated_to_16_bits(p):
    """a mask of period 65 536: every value of u occurs 64 times, and a column of the (-1, 96) view sees 2048 decisions"""
    u = dm.u_at(5, IDX & np.uint64(0xFFFF))
    assert chi_square(u) > CHI2_MAX
    assert 'column of 96' in _failed(u >= np.float32(p), _u(6) >= np.float32(p), p)
