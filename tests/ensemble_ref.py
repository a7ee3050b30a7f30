"""float64 numpy restatements for the ensemble tests: the five quantities of csrc/ensemble_scores.hip straight from their
definitions (the pairwise |x_i - x_j|, not the sorted form the kernel uses), the bound the kernel's fp32 per-point arithmetic
is held to, and the member streams of csrc/philox_normal.hpp (counter word 2 = member) on tests/philox_ref.py."""
import numpy as np

import philox_ref

U = 2.0 ** -24


def latitude_weights(lats_deg):
    w = np.cos(np.deg2rad(np.asarray(lats_deg, dtype=np.float64)))
    return (w / w.mean()).astype(np.float32).astype(np.float64)          # the fp32 weights the kernel reads


def sums_and_ranks(ens, target, latw, scale=None):
    """ens [M, B, K, C, H, W], target [B, K, C, H, W], latw [H], scale [C] or None ->
    (sums float64 [4, K, C], ranks int64 [K, C, M + 1])"""
    x = np.asarray(ens, dtype=np.float64)
    y = np.asarray(target, dtype=np.float64)
    m, b, k, c, h, w = x.shape
    s = np.ones(c) if scale is None else np.asarray(scale, dtype=np.float64)
    s = s.reshape(1, 1, c, 1, 1)
    wt = np.asarray(latw, dtype=np.float64).reshape(1, 1, 1, h, 1)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).sum(axis=0) / (m - 1)
    abs_err = np.abs(x - y).mean(axis=0)
    pairs = np.zeros_like(y)
    for i in range(m):
        for j in range(i + 1, m):
            pairs += np.abs(x[i] - x[j])
    q = [wt * (s * (mean - y)) ** 2, wt * s ** 2 * var, wt * s * abs_err, wt * s * pairs]
    sums = np.stack([v.sum(axis=(0, 3, 4)) for v in q])
    r = (x < y).sum(axis=0)                                              # strict
    ranks = np.zeros((k, c, m + 1), dtype=np.int64)
    for kk in range(k):
        for cc in range(c):
            ranks[kk, cc] = np.bincount(r[:, kk, cc].reshape(-1), minlength=m + 1)
    return sums, ranks


def sorted_pairs(ens):
    """sum_i (2i - M + 1) x_(i) per point: what sum_{i<j} |x_i - x_j| equals"""
    x = np.sort(np.asarray(ens, dtype=np.float64), axis=0)
    m = x.shape[0]
    coef = (2.0 * np.arange(m) - m + 1).reshape((m,) + (1,) * (x.ndim - 1))
    return (coef * x).sum(axis=0)


def bounds(ens, target, latw, scale=None):
    """float64 [4, K, C]: with A = max(max_m |x_m|, |y|) per point and u = 2^-24,
    4 (M + 4) u sum w s^2 A^2 for sums 0 and 1, 4 (M + 4) u sum w s A for sums 2, 4 (M + 4) M u sum w s A for sums 3"""
    x = np.asarray(ens, dtype=np.float64)
    y = np.asarray(target, dtype=np.float64)
    m, b, k, c, h, w = x.shape
    s = np.ones(c) if scale is None else np.abs(np.asarray(scale, dtype=np.float64))
    s = s.reshape(1, 1, c, 1, 1)
    wt = np.asarray(latw, dtype=np.float64).reshape(1, 1, 1, h, 1)
    a = np.maximum(np.abs(x).max(axis=0), np.abs(y))
    sq = (wt * s ** 2 * a ** 2).sum(axis=(0, 3, 4))
    lin = (wt * s * a).sum(axis=(0, 3, 4))
    f = 4.0 * (m + 4) * U
    return np.stack([f * sq, f * sq, f * lin, f * m * lin])


def scores(sums, ranks, count, members, cells):
    """the formulas of metrics.ensemble_scores in numpy"""
    m = members
    n = (np.asarray(count, dtype=np.float64) * cells).reshape(-1, 1)
    rmse = np.sqrt(sums[0] / n)
    spread = np.sqrt(sums[1] / n)
    return {"rmse_mean": rmse, "spread": spread, "spread_skill": np.sqrt((m + 1) / m) * spread / rmse,
            "crps": (sums[2] - sums[3] / (m * (m - 1))) / n, "crps_ens": (sums[2] - sums[3] / m ** 2) / n,
            "rank_histogram": ranks}


def member_normals(seed: int, member: int, offset: int, n: int):
    """float64 [n]: elements offset .. offset + n - 1 of the stream of `member` -- philox_ref.normals with counter word 2 = member"""
    assert offset % 4 == 0 and offset >= 0 and 0 <= member < 1 << 32
    nb = (n + 3) // 4
    q = np.uint64(offset // 4) + np.arange(nb, dtype=np.uint64)
    mask = np.uint64(philox_ref.MASK)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox_ref.philox4x32_10([q & mask, q >> np.uint64(32), np.full(nb, member, dtype=np.uint64), np.zeros(nb, dtype=np.uint64)],
                                 (seed & philox_ref.MASK, seed >> 32))
    out = np.empty((nb, 4), dtype=np.float64)
    for pair in (0, 1):
        ua, ub = philox_ref.uniform01(x[2 * pair]), philox_ref.uniform01(x[2 * pair + 1])
        r = np.sqrt(-2.0 * np.log(ua.astype(np.float64)))
        theta = (np.float32(6.2831855) * ub).astype(np.float64)          # the product in fp32, as the kernel
        out[:, 2 * pair] = r * np.cos(theta)
        out[:, 2 * pair + 1] = r * np.sin(theta)
    return out.reshape(-1)[:n]
