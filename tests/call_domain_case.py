"""One small crafted tumour cohort at the edges of the int32 count domain, for tests/test_gpu_call_domain.py (every kernel of
poisson_call) and tests/test_call_domain_case.py (the case is not vacuous: decided on the CPU, from the oracle and the inputs alone).

Shape: T = 5 rows (no multiple of 4 waves x rows per wave), P = 130 positions and E = 7 extra occurrences, so R = 137 records per
row: no multiple of 4 or 64, three 64-record tiles; ext_pos holds positions 0 and P - 1.  int32 layout.  Every strand sum and
FW + BW stays <= INT32_MAX, the domain the ASEQ parser admits.

Thresholds, one value per position for its eight cells: 0.002, 1e-5, 0.25, 0 (the magic 0.0010008f), -1 (no estimate), and positions
with 0.002 and ONE cell at -0.002.  Records, by kind (alt counts are placed against the position's own thresholds):
  depth   RD = FW + BW in {2^24 - 1, 2^24, 2^24 + 1}, per strand an alt count of floor(m) - 1, floor(m), floor(m) + 1, floor(m) + 3 or
          floor(m + 3 sqrt m) with m = strand depth x threshold: the fp32 skip (RD < 2^24 only), the exact k <= m of the drain and
          calls occur on both sides of AMPLI_COUNT_LIMIT
  bigalt  alt counts >= 2^24 on strands of 2^25 reads
  tabend  alt counts 65535 / 65536 / 65537 on strands of 4 (k - 536) reads: Q around 17 at a threshold of 0.25, kf_lgamma(k + 1) read
          across the end of the table
  top     FW = 2^31 - 2, BW = 1 (the reverse read is the alt)
  absent  no line for the position
  plain   a 2000x record, clean or with a planted variant
RD column (optional), per record: none (ABSENT), BW (forward depth 0: the drain's m == 0 arm, Q = 100), BW - 1 (forward depth -1: NaN,
no call), 0, 2^31 - 1, -2^30."""
import functools

import numpy as np

from oracle import pyoracle as orc

ABSENT = np.iinfo(np.int32).min
INT32_MAX = (1 << 31) - 1
LIMIT = 1 << 24  # AMPLI_COUNT_LIMIT
T, P, E = 5, 130, 7
R = P + E
THR_MENU = (0.002, 1e-5, 0.25, 0.0, -1.0, "negcell")
KINDS = ("depth", "depth", "depth", "depth", "bigalt", "tabend", "tabend", "top", "absent", "plain", "plain")
RD_MENU = ("none", "none", "none", "bw", "bw-1", "zero", "max", "neg")


def _eff(t):
    t = np.float32(t)
    return np.float32(0.0010008) if t == 0 else t


def _alt_count(depth, thr, delta, rng):
    """a count next to the mean of `depth` reads at threshold thr (a small one where there is no positive mean)"""
    if thr == -1 or thr < 0:
        return int(rng.integers(0, 9))
    m = float(depth) * float(_eff(thr))
    k = int(np.floor(m + 3 * np.sqrt(m))) if delta == "far" else int(np.floor(m)) + delta
    return max(0, min(k, depth))


def _inputs():
    rng = np.random.default_rng(20240)
    choice = [THR_MENU[i % len(THR_MENU)] for i in range(P)]
    order = rng.permutation(P)
    choice = [choice[i] for i in order]
    choice[0], choice[P - 1] = 0.25, 0.002
    thr = np.empty((2, 4, P), np.float32)
    for p, c in enumerate(choice):
        if c == "negcell":
            thr[:, :, p] = 0.002
            thr[rng.integers(0, 2), rng.integers(0, 4), p] = -0.002
        else:
            thr[:, :, p] = c
    ref_code = rng.integers(0, 4, P).astype(np.uint8)
    ref_code[[17, 64, 101]] = 255
    ext_pos = np.array([0, P - 1, 17, 3, 64, 77, 128], np.uint32)
    assert ext_pos.size == E
    pos = np.concatenate([np.arange(P), ext_pos.astype(np.int64)])
    recs = np.zeros((T, R, 8), np.int32)
    kinds = np.array([KINDS[i % len(KINDS)] for i in range(T * R)])
    kinds = kinds[rng.permutation(T * R)].reshape(T, R)
    deltas = (-1, 0, 1, 3, "far")
    for t in range(T):
        for r in range(R):
            p = int(pos[r])
            ref = int(ref_code[p]) & 3
            alt = (ref + 1 + int(rng.integers(0, 3))) % 4
            kind = kinds[t, r]
            if kind == "absent":
                recs[t, r, 0] = ABSENT
                continue
            if kind == "plain":
                recs[t, r, ref], recs[t, r, 4 + ref] = 1000, 950
                if rng.random() < 0.5:
                    recs[t, r, alt], recs[t, r, 4 + alt] = 40, 35
                continue
            if kind == "depth":
                rd = (LIMIT - 1, LIMIT, LIMIT + 1)[int(rng.integers(0, 3))]
                fw = rd // 2
                depth = (fw, rd - fw)
            elif kind == "bigalt":
                depth = (1 << 25, 1 << 25)
            elif kind == "tabend":
                depth = None
            else:
                depth = (INT32_MAX - 1, 1)
            for st in range(2):
                t_cell = float(thr[st, alt, p])
                if kind == "tabend":
                    k = (65535, 65536, 65537)[int(rng.integers(0, 3))]
                    d = 4 * (k - 536)
                elif kind == "bigalt":
                    d, k = depth[st], LIMIT + int(rng.integers(0, 7))
                elif kind == "top" and st == 1:
                    d, k = 1, 1
                else:
                    d = depth[st]
                    k = _alt_count(d, t_cell, deltas[int(rng.choice(5, p=[0.15, 0.15, 0.15, 0.15, 0.4]))], rng)
                recs[t, r, 4 * st + alt] = k
                recs[t, r, 4 * st + ref] = d - k
    rd = np.full((T, R), ABSENT, np.int32)
    menu = np.array([RD_MENU[i % len(RD_MENU)] for i in range(T * R)])[rng.permutation(T * R)].reshape(T, R)
    bw = recs[:, :, 4:].astype(np.int64).sum(-1)
    for name, val in (("bw", bw), ("bw-1", bw - 1), ("zero", 0 * bw), ("max", 0 * bw + INT32_MAX), ("neg", 0 * bw - (1 << 30))):
        rd[menu == name] = val[menu == name].astype(np.int32)
    for a in (thr, ref_code, ext_pos, recs, rd, pos):
        a.setflags(write=False)
    return dict(thr=thr, ref_code=ref_code, ext_pos=ext_pos, recs=recs, rd=rd, pos=pos)


@functools.lru_cache(maxsize=None)
def case(cov, with_rd):
    """The inputs, the oracle's result, and what the oracle and the inputs say about the case (all asserted here).  Read-only."""
    c = dict(_inputs())
    recs, thr, ref_code, pos = c["recs"], c["thr"], c["ref_code"], c["pos"]
    assert recs[:, :, :4].astype(np.int64).sum(-1).max() <= INT32_MAX and recs.astype(np.int64).sum(-1).max() <= INT32_MAX
    present = recs[:, :, 0] != ABSENT
    assert (recs[present] >= 0).all() and (~present).any()
    rd = c["rd"] if with_rd else None
    exp = orc.poisson_call(recs, P, thr, ref_code, cov, E=E, ext_pos=c["ext_pos"], rd=rd)
    mask, q = exp["call_mask"], exp["q"]
    FW = np.where(present, recs[:, :, :4].astype(np.int64).sum(-1), 0)
    BW = np.where(present, recs[:, :, 4:].astype(np.int64).sum(-1), 0)
    RD = FW + BW if rd is None else np.where(rd != ABSENT, rd.astype(np.int64), FW + BW)
    ref = ref_code[pos].astype(np.int64)
    live = present & (ref[None, :] <= 3) & (FW >= cov) & (BW >= cov)
    called = np.stack([(mask >> nt) & 1 for nt in range(4)], -1).astype(bool)   # [T][R][4]
    pair = live[:, :, None] & (np.arange(4)[None, None, :] != ref[None, :, None])  # the pairs the stream kernel looks at
    # the streaming kernel's fp32 test, as it is written there: a pair is queued unless one strand is provably below its mean
    te = np.where(thr == 0, np.float32(0.0010008), np.where(thr == -1, np.float32(np.inf), thr)).astype(np.float32)[:, :, pos]  # [2][4][R]
    d = np.stack([RD - BW, BW])                                                   # [2][T][R]
    exact = (RD >= 0) & (RD < LIMIT) & (d[0] >= 0)
    k = np.stack([recs[:, :, :4], recs[:, :, 4:]]).astype(np.int64)               # [2][T][R][4]
    with np.errstate(invalid="ignore", over="ignore"):
        cf = (d.astype(np.float32) * np.float32(0.999999))[:, :, :, None] * np.moveaxis(te, 1, 2)[:, None, :, :]
        skip = exact[None, :, :, None] & (k < LIMIT) & (k.astype(np.float32) <= cf)
    queued = pair & ~skip[0] & ~skip[1]
    assert (queued | ~called).all()  # nothing called is skipped
    # the drain's arm of each strand of a queued pair: it evaluates where k > m, by the sign of m = depth x effective error
    with np.errstate(invalid="ignore"):
        m = d.astype(np.float64)[:, :, :, None] * np.moveaxis(te, 1, 2).astype(np.float64)[:, None, :, :]
        ev = queued[None] & ~np.isinf(np.moveaxis(te, 1, 2))[:, None, :, :] & (k.astype(np.float64) > m)
    arms = {"m > 0": int((ev & (m > 0)).sum()), "m == 0": int((ev & (m == 0)).sum()), "m < 0": int((ev & (m < 0)).sum())}
    calls = int(called.sum())
    big_not_called = int((queued & ~called & (RD >= LIMIT)[:, :, None]).sum())
    small_skipped = int((pair & ~queued).sum())
    qc = q[called]                                                                # [calls][2]
    stats = dict(calls=calls, queued=int(queued.sum()), skipped_in_fp32=small_skipped, queued_not_called_rd_ge_2p24=big_not_called, arms=arms,
                 q100_calls=int((qc == 100).any(-1).sum()), midrange_calls=int(((qc > 5) & (qc < 100)).all(-1).sum()),
                 calls_rd_ge_2p24=int((called & (RD >= LIMIT)[:, :, None]).sum()), calls_rd_lt_2p24=int((called & (RD < LIMIT)[:, :, None]).sum()),
                 calls_at_forward_depth_0=int((called & (d[0] == 0)[:, :, None]).sum()), records=T * R, present=int(present.sum()))
    assert not with_rd or stats["calls_at_forward_depth_0"] > 0, stats  # the m == 0 arm's Q = 100 carries calls
    assert calls > 0 and stats["q100_calls"] > 0 and stats["midrange_calls"] > 0, stats
    assert big_not_called > 0 and small_skipped > 0 and stats["calls_rd_ge_2p24"] > 0, stats
    assert arms["m > 0"] > 0 and (not with_rd or (arms["m == 0"] > 0 and arms["m < 0"] > 0)), stats
    assert arms["m < 0"] > 0, stats  # the negative threshold cells give that arm without an RD column too
    # a count >= 2^24 and a count on each side of the table's end are among the queued pairs' strands
    kq = k[np.broadcast_to(queued[None], k.shape)]
    assert (kq >= LIMIT).any() and (kq == 65535).any() and (kq == 65537).any()
    # no score of a live pair lies so close to the gate that the device could decide it the other way or flag it borderline
    ql = q[pair]
    with np.errstate(invalid="ignore"):
        assert not (np.abs(ql - 5.0) < 1e-4).any()
    assert np.isnan(ql).any() and (ql == -888).any() and (ql == 0).any()  # the dense scores hold every special value
    c.update(exp=exp, cov=cov, with_rd=with_rd, stats=stats, rd=rd)
    return c
