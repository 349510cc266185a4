"""Score planes for the false-discovery tests, built directly -- no scorer is needed -- and the grid the host library and
the kernels are both held to.  A plane of one (P, mode) has one ROW PER KIND, so one model evaluation serves every test of that shape;
the rows are independent by contract, and the tests run them in batches of 1, 3 and 5 rows."""
import functools

import numpy as np

from tests import fdr_model

TILE_KEYS, SCAN_BLOCK = 4096, 512  # AMPLI_FDR_TILE_KEYS, AMPLI_FDR_SCAN_BLOCK (tests/test_fdr_host.py reads them from the header too)

KINDS = ("exponential", "five_values", "all_hundred", "all_zero", "all_na", "one_tested", "digit0", "digit1", "digit2", "digit3", "negative_zero",
         "exponential_dense")
BATCHES = ((0, 1), (1, 4), (4, 9), (9, 12))  # rows [lo, hi): 1, 3, 5 and 3 rows


def edges():
    """P on the edges of the sort tile, of two tiles, and of what one second-level scan step covers (65536 positions: it runs in
    well under a second, so the largest edge is tested as it is)."""
    out = [1, 2, 15, 16, 17, 63, 64, 65, 1000]
    for e in (TILE_KEYS // 4, 2 * (TILE_KEYS // 4), SCAN_BLOCK * SCAN_BLOCK // 4):
        out += [e - 1, e, e + 1]
    return out


def _from_bits(bits, sign):
    a = np.asarray(bits, np.uint32).view(np.float32)
    return np.stack([a * sign, a * sign], axis=-1).astype(np.float32)


def row(kind, P, two_sided, seed):
    """One row float32 [P, 4, 2] of the given kind, with a fraction of NA cells where the kind leaves room for them."""
    rng = np.random.default_rng([seed, P, int(two_sided), KINDS.index(kind)])
    n = 4 * P
    na = np.float32(-999.0 if two_sided else -1.0)
    sign = rng.choice(np.array([1.0, -1.0], np.float32), n) if two_sided else np.ones(n, np.float32)
    i = rng.permutation(n).astype(np.uint32)
    if kind in ("exponential", "exponential_dense"):
        s = np.minimum(rng.exponential(8.0, (n, 2)), 100.0).astype(np.float32)
        s[rng.random(n) < 0.3] *= np.float32(0.0)                       # cells without evidence
        s = s * sign[:, None]
        if two_sided:
            s[rng.random(n) < 0.1, 1] *= np.float32(-1.0)               # strands on opposite sides: a = 0
    elif kind == "five_values":
        s = _from_bits(rng.choice(np.array([3.0, 13.0, 13.5, 40.0, 100.0], np.float32), n).view(np.uint32), sign)
    elif kind == "all_hundred":
        s = _from_bits(np.full(n, np.float32(100.0)).view(np.uint32), sign)
    elif kind == "all_zero":
        s = np.zeros((n, 2), np.float32)
    elif kind == "all_na":
        s = np.full((n, 2), na, np.float32)
        s[rng.random(n) < 0.3] = np.float32(np.nan)
        s[rng.random(n) < 0.1, 0] = np.float32(100.0001)
    elif kind == "one_tested":
        s = np.full((n, 2), na, np.float32)
        s[int(rng.integers(n))] = np.array([17.25, 30.0], np.float32) * sign[0]
    elif kind == "digit0":
        s = _from_bits(np.uint32(0x3F800000) + i, sign)                  # only the lowest digit differs (and carries into the next)
    elif kind == "digit1":
        s = _from_bits(np.uint32(0x3F800000) + ((i % np.uint32(256)) << np.uint32(8)), sign)
    elif kind == "digit2":
        s = _from_bits(np.uint32(0x3F800000) + ((i % np.uint32(64)) << np.uint32(16)), sign)
    elif kind == "digit3":
        s = _from_bits(((i % np.uint32(0x43)) << np.uint32(24)) | np.uint32(0x00800000), sign)  # 2^-126 .. 64
    elif kind == "negative_zero":
        s = np.minimum(rng.exponential(8.0, (n, 2)), 100.0).astype(np.float32) + np.float32(0.5)
        z = rng.random(n) < 0.2
        s[z, 0] = np.float32(-0.0)
        s[z & (rng.random(n) < 0.5), 1] = np.float32(-0.0)
    else:
        raise ValueError(kind)
    if kind not in ("all_na", "one_tested", "exponential_dense"):
        s[rng.random(n) < 0.1] = na
    return np.ascontiguousarray(s.reshape(P, 4, 2))


@functools.lru_cache(maxsize=6)
def case(P, two_sided, seed=20260121):
    """(plane float32 [len(KINDS), P, 4, 2], A float64, m, R) -- computed once per shape and never changed."""
    s = np.stack([row(k, P, two_sided, seed) for k in KINDS])
    A, m, R = fdr_model.adjust(s, two_sided)
    for x in (s, A, m, R):
        x.setflags(write=False)
    return s, A, m, R
