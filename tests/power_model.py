"""Detection power and limit of detection, the definition restated in pure Python -- TEST INFRASTRUCTURE.

A cell (sample, record, base) whose status is OK with minimum reads min_fw >= 1, min_bw >= 1 on a record with FW forward and BW
reverse reads: a variant at allele fraction v turns each read of a strand into an alternative read independently with probability
v, the depths stay fixed, background alternative reads are ignored, and the gate passes exactly when k_fw >= min_fw and k_bw >= min_bw:
  tail(n, k, v) = P[Bin(n, v) >= k] = I_v(k, n - k + 1),  tail(n, k, 1) = 1
  power(v)      = tail(FW, min_fw, v) * tail(BW, min_bw, v)
  LoD(c)        = the v in (0, 1] with power(v) = c, by up to 200 bisections in ln v over [ln 1e-12, 0]
Every other cell has power 0 and LoD 0.

The tail is math.fsum over pmf terms.  ONE term is taken from math.lgamma, the others follow by the exact ratio of neighbouring terms.
Where an argument of lgamma is 1000 or more the term is NOT formed as lgamma(n + 1) - lgamma(k + 1) - lgamma(n - k + 1): at 2^30 each of
those carries an absolute error of 4e-6, more than the tolerance this model is the reference for.  The three are then written as
Stirling's formula plus its error d(x) = lgamma(x + 1) - ((x + 1/2) ln x - x + 1/2 ln 2 pi), the Stirling parts are combined on paper into
1/2 ln(n / (2 pi k (n - k))) - n KL(k/n || v), and d(x) comes from math.lgamma below 1000 and from its asymptotic series above.
tests/test_power_host.py pins the result to scipy.special.betainc and to mpmath at 40 digits.
"""
from __future__ import annotations

import functools
import math

import numpy as np

LN_LO = math.log(1e-12)


def _stirling_err(x):
    if x < 1000:
        return math.lgamma(x + 1.0) - ((x + 0.5) * math.log(x) - x + 0.5 * math.log(2 * math.pi))
    r = 1.0 / (x * x)
    return (1.0 / 12 - (1.0 / 360 - (1.0 / 1260 - (1.0 / 1680 - 1.0 / 1188 * r) * r) * r) * r) / x


def _dev(x, m):
    """x ln(x / m) + m - x"""
    if x == 0:
        return m
    t = (x - m) / m
    return m * ((1.0 + t) * math.log1p(t) - t)


def log_pmf(n, j, v):
    if j == 0:
        return n * math.log1p(-v)
    if j == n:
        return n * math.log(v)
    if n < 1000:
        return math.lgamma(n + 1.0) - math.lgamma(j + 1.0) - math.lgamma(n - j + 1.0) + j * math.log(v) + (n - j) * math.log1p(-v)
    return (0.5 * math.log(n / (2 * math.pi * j * (n - j))) + _stirling_err(n) - _stirling_err(j) - _stirling_err(n - j)
            - _dev(j, n * v) - _dev(n - j, n * (1.0 - v)))


def tail(n, k, v):
    """P[Bin(n, v) >= k]: the terms from k upwards when k is above the mean, else one minus the terms from k - 1 downwards; a sum
    ends where a term no longer changes it (below 1e-30 of the first, largest one)"""
    n, k, v = int(n), int(k), float(v)
    if k > n or v <= 0:
        return 0.0
    if k <= 0 or v >= 1:
        return 1.0
    odds = v / (1.0 - v)
    up = k > n * v
    j = k if up else k - 1
    t = math.exp(log_pmf(n, j, v))
    terms = [t]
    floor = t * 1e-30
    if up:
        while j < n:
            t *= (n - j) / (j + 1.0) * odds
            j += 1
            if t <= floor:
                break
            terms.append(t)
    else:
        while j > 0:
            t *= j / (n - j + 1.0) / odds
            j -= 1
            if t <= floor:
                break
            terms.append(t)
    s = math.fsum(terms)
    return min(s, 1.0) if up else max(0.0, 1.0 - s)


def power(FW, min_fw, BW, min_bw, v):
    return tail(FW, min_fw, v) * tail(BW, min_bw, v)


@functools.lru_cache(maxsize=None)
def lod(FW, min_fw, BW, min_bw, c):
    lo, hi = LN_LO, 0.0  # power(e^lo) < c <= power(e^hi) = 1
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:  # the doubles between them are used up: the remaining bisections change nothing
            break
        if power(FW, min_fw, BW, min_bw, math.exp(mid)) < c:
            lo = mid
        else:
            hi = mid
    return math.exp(hi)


@functools.lru_cache(maxsize=None)
def powers(FW, min_fw, BW, min_bw, levels):
    return tuple(power(FW, min_fw, BW, min_bw, float(np.float32(v))) for v in levels)


def slope(FW, min_fw, BW, min_bw, v):
    """d power / d ln v = k_fw pmf_fw(k_fw) tail_bw + tail_fw k_bw pmf_bw(k_bw)"""
    def kpmf(n, k):
        return k * math.exp(log_pmf(n, k, v)) if v < 1 else 0.0
    return kpmf(FW, min_fw) * tail(BW, min_bw, v) + tail(FW, min_fw, v) * kpmf(BW, min_bw)


def is_ok(status, min_reads, FW, BW):
    """the cells of the definition: status uint8 [..., 4], min_reads [..., 4, 2], FW / BW [...]"""
    mf, mb = min_reads[..., 0], min_reads[..., 1]
    return ((status & 0x87) == 0) & (mf >= 1) & (mb >= 1) & (mf <= FW[..., None]) & (mb <= BW[..., None])
