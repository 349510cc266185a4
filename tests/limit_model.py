"""Detection limits of the calling gate, the literal model on top of the CPU oracle -- TEST INFRASTRUCTURE.

For a present record (counts c[8], FW, BW, RD: the RD column where the line carries its own), the position's reference code and the
thresholds thr[2][4][P] as poisson_call takes them, every base nt != ref is a pair with a status:
  LOWDEPTH     FW < cov or BW < cov
  NOESTIMATE   a strand's threshold is -1 (the scorer's -888 branch)
  UNREACHABLE  a strand has no k in 1 .. its reads with oracle_score(k, depth, thr) >= 5 (also a forward depth RD - BW <= 0)
  OK           min_fw / min_bw = the smallest such k per strand, scanning upwards; MinAF = float32(min_fw + min_bw) / float32(RD)
Called = the gate of VC:898 on the observed counts.  ref > 3: no pairs, the line is counted as NOREF.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from oracle import pyoracle as orc

ABSENT = np.iinfo(np.int32).min
OK, REF, NOREF, LOWDEPTH, NOESTIMATE, UNREACHABLE, ABSENT_CODE = range(7)
CALLED, RECHECK = 0x40, 0x80
COUNTERS = 6
NAMES = {OK: "OK", LOWDEPTH: "LOWDEPTH", NOESTIMATE: "NOESTIMATE", UNREACHABLE: "UNREACHABLE"}


def score(k, depth, thr):
    return float(orc.lib().oracle_score(int(k), int(depth), C.c_float(float(thr))))


def strand_limit(depth, thr, bound, from_one=True):
    """the smallest k in 1 .. bound with Q(k, depth, thr) >= 5; -1: no estimate (thr == -1); 0: none.  from_one=False starts the scan
    at floor(m) - 2 (nothing passes at k <= m: tests/test_limit_host.py), for the cases where a scan from 1 would take minutes."""
    thr = np.float32(thr)
    if thr == np.float32(-1):
        return -1
    if depth <= 0:
        return 0
    k0 = 1
    if not from_one:
        m = float(depth) * float(np.float32(0.0010008) if thr == 0 else thr)
        if math.isfinite(m) and m > 4:
            k0 = min(int(math.floor(m)) - 2, 1 << 31)
    L = orc.lib()
    cthr = C.c_float(float(thr))
    for k in range(k0, bound + 1):
        if float(L.oracle_score(k, int(depth), cthr)) >= 5:
            return k
    return 0


def pair_limit(rec, RD, nt, thr_fw, thr_bw, cov, from_one=True):
    """(status, min_fw, min_bw, called) of one (record, base) pair"""
    rec = [int(x) for x in rec]
    FW, BW = sum(rec[:4]), sum(rec[4:])
    if FW < cov or BW < cov:
        return LOWDEPTH, 0, 0, False
    called = score(rec[nt], RD - BW, thr_fw) >= 5 and score(rec[4 + nt], BW, thr_bw) >= 5
    if np.float32(thr_fw) == -1 or np.float32(thr_bw) == -1:
        return NOESTIMATE, 0, 0, called
    mf = strand_limit(RD - BW, thr_fw, FW, from_one)
    mb = strand_limit(BW, thr_bw, BW, from_one) if mf > 0 else 0
    if mf <= 0 or mb <= 0:
        return UNREACHABLE, 0, 0, called
    assert called == (rec[nt] >= mf and rec[4 + nt] >= mb), (rec, RD, nt, thr_fw, thr_bw, mf, mb)
    return OK, mf, mb, called


def min_af(mf, mb, RD):
    return np.float32(np.float32(mf + mb) / np.float32(RD))


def limit_model(recs, P, thr, ref_code, cov=100, E=0, ext_pos=None, rd=None, levels=(), from_one=True):
    """recs int32 [n][P+E][8], thr float32 [2][4][P], rd optional int32 [n][P+E] (INT32_MIN where the line is regular).
    Returns min_reads int32 [n][R][4][2], status uint8 [n][R][4] (CALLED in bit 6) and counts int64 [n][6 + len(levels)]."""
    recs = np.asarray(recs, np.int32)
    n, R = recs.shape[0], recs.shape[1]
    assert R == P + E
    lv = np.asarray(levels, np.float32)
    min_reads = np.zeros((n, R, 4, 2), np.int32)
    status = np.zeros((n, R, 4), np.uint8)
    counts = np.zeros((n, COUNTERS + len(lv)), np.int64)
    for r in range(R):
        p = r if r < P else int(ext_pos[r - P])
        ref = int(ref_code[p])
        for s in range(n):
            rec = recs[s, r]
            if rec[0] == ABSENT:
                status[s, r] = ABSENT_CODE
                continue
            if ref > 3:
                status[s, r] = NOREF
                counts[s, 0] += 1
                continue
            tot = int(rec.astype(np.int64).sum())
            RD = tot if rd is None or rd[s, r] == ABSENT else int(rd[s, r])
            for nt in range(4):
                if nt == ref:
                    status[s, r, nt] = REF
                    continue
                st, mf, mb, called = pair_limit(rec, RD, nt, thr[0, nt, p], thr[1, nt, p], cov, from_one)
                min_reads[s, r, nt] = (mf, mb)
                status[s, r, nt] = st | (CALLED if called else 0)
                counts[s, {OK: 1, LOWDEPTH: 2, NOESTIMATE: 3, UNREACHABLE: 4}[st]] += 1
                if st == OK:
                    counts[s, COUNTERS:] += min_af(mf, mb, RD) <= lv
    return dict(min_reads=min_reads, status=status, counts=counts)


def settle(res, recs, P, thr, ref_code, cov, E=0, ext_pos=None, rd=None, levels=()):
    """the RECHECK cells of a device result (numpy arrays, changed in place) decided by the host library's literal scan
    (ampli_host_limit_reads) and its guard score for the called bit.  Returns the number of cells settled."""
    from amplisolve_amd import host_lib

    H = host_lib()
    lv = np.asarray(levels, np.float32)
    cells = np.argwhere(res["status"] & RECHECK)
    for s, r, nt in cells:
        assert res["status"][s, r, nt] == RECHECK and not res["min_reads"][s, r, nt].any()
        p = r if r < P else int(ext_pos[r - P])
        rec = [int(x) for x in recs[s, r]]
        FW, BW = sum(rec[:4]), sum(rec[4:])
        RD = FW + BW if rd is None or rd[s, r] == ABSENT else int(rd[s, r])
        tf, tb = float(thr[0, nt, p]), float(thr[1, nt, p])
        assert FW >= cov and BW >= cov and tf != -1 and tb != -1  # those statuses need no arithmetic
        called = H.ampli_host_guard_score(rec[nt], RD - BW, tf, None, None) >= 5 and H.ampli_host_guard_score(rec[4 + nt], BW, tb, None, None) >= 5
        mf = H.ampli_host_limit_reads(RD - BW, tf, FW)
        mb = H.ampli_host_limit_reads(BW, tb, BW) if mf > 0 else 0
        st = OK if mf > 0 and mb > 0 else UNREACHABLE
        res["min_reads"][s, r, nt] = (mf, mb) if st == OK else (0, 0)
        res["status"][s, r, nt] = st | (CALLED if called else 0)
        res["counts"][s, 5] -= 1
        res["counts"][s, 1 if st == OK else 4] += 1
        if st == OK:
            res["counts"][s, COUNTERS:] += min_af(mf, mb, RD) <= lv
    return len(cells)
