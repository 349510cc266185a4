"""The read-evidence kernels' test model -- TEST INFRASTRUCTURE (never imported by the product).

Restatements of the definitions in the contract comments of ampli_pileup_evidence and ampli_evidence_score (include/amplisolve_hip.h,
DESIGN 29) over the read dicts and record streams of tests/pileup_model.py, written differently on purpose so that they check each other:
  * count: numpy over the flat columns of all kept reads -- every column of every match run, looked up among the keys;
  * walk:  a per-read Python loop in plain integers, one operation at a time, the keys merged into the walk;
  * score: the score in numpy doubles, in the contract's order of operations;
  * score_exact: the same quantities with Python integers and fractions.Fraction.
`wrong=` switches count or score to one deliberately wrong variant (WRONG_VARIANTS); tests/test_evidence_model.py shows that each of them
is caught by a named deterministic case (CAUGHT_BY).  geometry() reads the kernel's constexpr lines; cases() is the named case table, and
every case that claims to sit on an edge asserts so while the table is built.  files() is what computeReadEvidence writes.
"""
from __future__ import annotations

import bisect
import collections
import functools
import math
import os
import re
import struct
import zlib
from fractions import Fraction

import numpy as np

from tests import pileup_model as pm
from tests.pileup_model import build_stream, make_keys, read, span_keys  # noqa: F401

KERNEL_SOURCE = os.path.join(pm.ROOT, "amplisolve_amd", "csrc", "ampli_evidence.hip")
TYPES_HEADER = os.path.join(pm.ROOT, "include", "amplisolve_types.h")
M_OPS, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P = (0, 7, 8), 1, 2, 3, 4, 5, 6
METRICS, BINS, BQ, MQ, POS = 3, 64, 0, 1, 2  # the contract's numbers; geometry() holds the header's, compared in tests/test_evidence_model.py
METRIC_NAMES, FLAG_NAMES = ("BQ", "MQ", "POS"), ("LOW_BQ", "LOW_MQ", "READ_END")

Geometry = collections.namedtuple("Geometry", "reads window metrics bins bq mq pos")


@functools.lru_cache(None)
def geometry():
    """(reads per workgroup, listed keys of the LDS window) as ampli_evidence.hip states them, and the constants of the header"""
    text = open(KERNEL_SOURCE).read()
    vals = []
    for name in ("READS", "WINDOW"):
        m = re.search(r"^constexpr\s+int\s+EVIDENCE_%s\s*=\s*(\d+);" % name, text, re.M)
        assert m, f"no `constexpr int EVIDENCE_{name} = ...;` line in {KERNEL_SOURCE}"
        vals.append(int(m.group(1)))
    types = open(TYPES_HEADER).read()
    for name in ("METRICS", "BINS", "BQ", "MQ", "POS"):
        m = re.search(r"^#define\s+AMPLI_EVIDENCE_%s\s+(\d+)" % name, types, re.M)
        assert m, f"no AMPLI_EVIDENCE_{name} in include/amplisolve_types.h"
        vals.append(int(m.group(1)))
    return Geometry(*vals)


# name -> what is wrong; count(..., wrong=name) or score(..., wrong=name) computes that variant.  One per rule of the definition.
COUNT_VARIANTS = {
    "i_without_soft_clips": "soft-clipped bases in front of the column do not count towards i",
    "i_not_advanced_by_I": "inserted bases in front of the column do not count towards i",
    "i_advanced_by_D": "deleted bases in front of the column count towards i",
    "d_from_i_alone": "d = i instead of min(i, l_seq - 1 - i)",
    "hard_clip_in_l_seq": "hard-clipped bases are counted in l_seq",
    "bins_clamped_at_62": "bins are clamped at 62",
    "bins_not_clamped": "bins are not clamped: what lies beyond 63 is lost",
    "mapq_not_shifted": "the MQ bin is mapq instead of mapq >> 2",
    "mbq_off_by_one": "quality > mbq instead of >=",
    "mrq_off_by_one": "MAPQ > mrq instead of >=",
}
SCORE_VARIANTS = {
    "ties_counted_whole": "a tie between an alt and a ref read counts 1 instead of 1/2",
    "tie_term_dropped": "the variance is not corrected for ties",
    "median_upper": "the median is the smallest b with 2 cum_b > n",
    "choose_takes_ref": "`choose` may take the reference nt",
    "choose_ties_upwards": "`choose` breaks ties towards the highest index",
}
WRONG_VARIANTS = {**COUNT_VARIANTS, **SCORE_VARIANTS}

Result = collections.namedtuple("Result", "hist stats")  # int64 [P][4][3][64], (reads kept, columns counted)
Score = collections.namedtuple("Score", "ints med z2 alt_used")  # int64 [P][3][3], int64 [P][3][2], float64 [P][3], int64 [P]


def _clamp(x, wrong):
    """(bin, kept) of the values x"""
    if wrong == "bins_not_clamped":
        return x, (x >= 0) & (x < BINS)
    return np.minimum(x, 62 if wrong == "bins_clamped_at_62" else BINS - 1), x >= 0  # (only a wrong variant goes below 0)


def count(src, keys, mbq, mrq, wrong=None, detail=False):
    """Result of the stream `src` (read dicts or (buf, rec_off)) on the panel `keys`: the vectorised restatement.  detail=True adds
    (read index, key index, leading soft clip, inserted bases in front, the three unclamped values) of every counted column."""
    assert wrong is None or wrong in COUNT_VARIANTS, wrong
    buf, rec_off = pm.as_stream(src)
    keys = np.asarray(keys, np.uint64)
    P = len(keys)
    h = pm.headers(buf, rec_off)
    keep = (h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & pm.READ_MASK) == 0) & ((h.mapq > mrq) if wrong == "mrq_off_by_one" else (h.mapq >= mrq))
    rd = np.flatnonzero(keep)
    nc = h.n_cigar[rd]
    o_read = np.repeat(rd, nc)
    first = np.cumsum(nc) - nc
    o_idx = np.arange(len(o_read)) - np.repeat(first, nc)
    v = pm._le(buf, h.cig[o_read] + 4 * o_idx, 4)
    op, ln = v & 15, v >> 4

    def before(ops):  # what the read's earlier operations of these kinds are long, together
        adv = np.where(np.isin(op, ops), ln, 0)
        c = np.cumsum(adv) - adv
        return c - np.repeat(c[first[nc > 0]], nc[nc > 0]) if len(c) else c

    rbef, qbef, sbef, ibef, dbef = before(pm.REF_OPS), before(pm.QUERY_OPS), before((OP_S,)), before((OP_I,)), before((OP_D,))
    hard = np.bincount(o_read, weights=np.where(op == OP_H, ln, 0), minlength=len(rec_off)).astype(np.int64)
    runs = np.flatnonzero(np.isin(op, M_OPS) & (ln > 0))
    col_run = np.repeat(runs, ln[runs])
    j = np.arange(len(col_run)) - np.repeat(np.cumsum(ln[runs]) - ln[runs], ln[runs])
    rd_of = o_read[col_run]
    key = pm._key_of(h.ref_id[rd_of], h.pos[rd_of] + 1 + rbef[col_run] + j)
    ki = np.searchsorted(keys, key)
    sel = np.flatnonzero(keys[np.minimum(ki, P - 1)] == key)
    rd_of, ki, col_run, q = rd_of[sel], ki[sel], col_run[sel], (qbef[col_run] + j)[sel]
    byte = buf[h.seq[rd_of] + (q >> 1)].astype(np.int64)
    b4 = pm._B4[np.where((q & 1) == 0, byte >> 4, byte & 15)]
    qual = buf[h.qual[rd_of] + q].astype(np.int64)
    good = (b4 >= 0) & ((qual > mbq) if wrong == "mbq_off_by_one" else (qual >= mbq))
    rd_of, ki, col_run, q, b4, qual = rd_of[good], ki[good], col_run[good], q[good], b4[good], qual[good]
    i = q - (sbef[col_run] if wrong == "i_without_soft_clips" else 0) - (ibef[col_run] if wrong == "i_not_advanced_by_I" else 0) + \
        (dbef[col_run] if wrong == "i_advanced_by_D" else 0)
    l_seq = h.l_seq[rd_of] + (hard[rd_of] if wrong == "hard_clip_in_l_seq" else 0)
    d = i if wrong == "d_from_i_alone" else np.minimum(i, l_seq - 1 - i)
    values = (qual, h.mapq[rd_of] if wrong == "mapq_not_shifted" else h.mapq[rd_of] >> 2, d)
    hist = np.zeros(P * 4 * METRICS * BINS, np.int64)
    for m, x in enumerate(values):
        b, ok = _clamp(x, wrong)
        hist += np.bincount((((ki * 4 + b4) * METRICS + m) * BINS + b)[ok], minlength=len(hist))
    res = Result(hist.reshape(P, 4, METRICS, BINS), (int(keep.sum()), int(len(ki))))
    return res + ((rd_of, ki, sbef[col_run], ibef[col_run], values),) if detail else res


def walk(src, keys, mbq, mrq):
    """Result of the same stream one read and one operation at a time, in plain integers: the sorted keys are merged into the walk"""
    buf, rec_off = pm.as_stream(src)
    b = bytes(buf)
    ks = [int(k) for k in np.asarray(keys, np.uint64).tolist()]
    P = len(ks)
    hist = np.zeros((P, 4, METRICS, BINS), np.int64)
    kept = columns = 0
    for o in np.asarray(rec_off, np.uint64).tolist():
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, o + 4)
        if ref_id < 0 or pos < 0 or flag & pm.READ_MASK or mapq < mrq:
            continue
        kept += 1
        cig = o + 36 + l_name
        seq = cig + 4 * n_cigar
        qual = seq + (l_seq + 1) // 2
        k = bisect.bisect_left(ks, (ref_id << 32) | (pos + 1))
        refpos, i = pos + 1, 0  # 1-based position and index into SEQ of the next column
        for c in range(n_cigar):
            v, = struct.unpack_from("<I", b, cig + 4 * c)
            o_, n = v & 15, v >> 4
            if n == 0 or o_ == OP_P:
                continue
            if o_ in M_OPS:
                while k < P and ks[k] >> 32 == ref_id and (ks[k] & 0xffffffff) < refpos + n:
                    at = i + (ks[k] & 0xffffffff) - refpos
                    nib = (b[seq + at // 2] >> (0 if at & 1 else 4)) & 15
                    if nib in (1, 2, 4, 8) and b[qual + at] >= mbq:
                        nt = (1, 2, 4, 8).index(nib)
                        hist[k, nt, BQ, min(b[qual + at], 63)] += 1
                        hist[k, nt, MQ, min(mapq >> 2, 63)] += 1
                        hist[k, nt, POS, min(at, l_seq - 1 - at, 63)] += 1
                        columns += 1
                    k += 1
                refpos, i = refpos + n, i + n
            elif o_ in (OP_I, OP_S):
                i += n
            elif o_ in (OP_D, OP_N):
                refpos += n
                assert refpos < 1 << 32
                k = bisect.bisect_left(ks, (ref_id << 32) | refpos, k)
    return Result(hist, (kept, columns))


# ---------------------------------------------------------------------------------------------------------------------------
# the score
# ---------------------------------------------------------------------------------------------------------------------------
def score(hist, ref_nt, alt_nt, wrong=None):
    """Score of the planes `hist` [P][4][3][64] with the alleles ref_nt, alt_nt [P]: numpy doubles in the contract's order"""
    assert wrong is None or wrong in SCORE_VARIANTS, wrong
    hist = np.asarray(hist, np.int64).reshape(-1, 4, METRICS, BINS)
    P = len(hist)
    ref, alt = np.asarray(ref_nt, np.int64).reshape(P), np.asarray(alt_nt, np.int64).reshape(P)
    rows = np.arange(P)
    ref_ok = (ref >= 0) & (ref <= 3)
    tot = hist[:, :, BQ, :].sum(2)
    if wrong != "choose_takes_ref":
        tot[rows[ref_ok], ref[ref_ok]] = np.iinfo(np.int64).min
    chosen = 3 - np.argmax(tot[:, ::-1], 1) if wrong == "choose_ties_upwards" else np.argmax(tot, 1)
    used = np.where(alt == -1, chosen, np.where((alt >= 0) & (alt <= 3) & (alt != ref), alt, -1))
    used = np.where(ref_ok, used, -1)
    a = np.where((used >= 0)[:, None, None], hist[rows, np.maximum(used, 0)], 0)  # [P][3][64]
    r = np.where(ref_ok[:, None, None], hist[rows, np.clip(ref, 0, 3)], 0)
    n1, n2 = a.sum(2), r.sum(2)
    N = n1 + n2
    ca, cr = np.cumsum(a, 2), np.cumsum(r, 2)
    u2 = (a * (2 * (cr - r) + (2 if wrong == "ties_counted_whole" else 1) * r)).sum(2)

    def median(cum, n):
        reached = 2 * cum > n[..., None] if wrong == "median_upper" else 2 * cum >= n[..., None]
        return np.where(n > 0, np.argmax(reached, 2), -1)

    Td = np.zeros(n1.shape, np.float64)
    if wrong != "tie_term_dropped":
        for b in range(BINS):
            t = (a[..., b] + r[..., b]).astype(np.float64)
            Td = Td + ((t * t) * t - t)
    Nd = N.astype(np.float64)
    with np.errstate(all="ignore"):
        c = (Nd + 1.0) - Td / (Nd * (Nd - 1.0))
        v = (n1.astype(np.float64) * n2.astype(np.float64)) * c
        tested = (n1 > 0) & (n2 > 0) & (N < 1 << 30) & (v > 0)
        D = u2 - n1 * n2
        Dd = D.astype(np.float64)
        z2 = ((3.0 * Dd) * Dd) / v
    z2 = np.where(tested, np.where(D < 0, -z2, z2), 0.0)
    return Score(np.stack([n2, n1, np.where(tested, u2, -1)], 2), np.stack([median(cr, n2), median(ca, n1)], 2), z2, used)


def score_exact(plane, ref, alt):
    """One position (plane [4][3][64]) in Python integers and Fractions: per metric a dict with n_ref, n_alt, u2 (-1: untested), med_ref,
    med_alt, z2 (a Fraction, signed) and c (the exact variance factor, None for N < 2), plus the alt that was used"""
    plane = [[[int(x) for x in m] for m in nt] for nt in np.asarray(plane).reshape(4, METRICS, BINS)]
    used = -1
    if 0 <= ref <= 3:
        if alt == -1:
            used = max((nt for nt in range(4) if nt != ref), key=lambda nt: (sum(plane[nt][BQ]), -nt))
        elif 0 <= alt <= 3 and alt != ref:
            used = alt
    out = []
    for m in range(METRICS):
        a = plane[used][m] if used >= 0 else [0] * BINS
        r = plane[ref][m] if 0 <= ref <= 3 else [0] * BINS
        n1, n2 = sum(a), sum(r)
        N = n1 + n2
        u2 = sum(a[b] * (2 * sum(r[:b]) + r[b]) for b in range(BINS))

        def med(x, n):
            return -1 if n == 0 else next(b for b in range(BINS) if 2 * sum(x[:b + 1]) >= n)

        c = Fraction(N + 1) - Fraction(sum((a[b] + r[b]) ** 3 - (a[b] + r[b]) for b in range(BINS)), N * (N - 1)) if N >= 2 else None
        tested = n1 > 0 and n2 > 0 and N < 1 << 30 and c is not None and c > 0
        D = u2 - n1 * n2
        z2 = Fraction(3 * D * D, 1) / (n1 * n2 * c) * (-1 if D < 0 else 1) if tested else Fraction(0)
        out.append(dict(n_ref=n2, n_alt=n1, u2=u2 if tested else -1, med_ref=med(r, n2), med_alt=med(a, n1), z2=z2, c=c, N=N))
    return out, used


# ---------------------------------------------------------------------------------------------------------------------------
# the command's two files
# ---------------------------------------------------------------------------------------------------------------------------
def nt_code(allele, choose):
    """0 .. 3, -1 for "." where `choose` allows it, -2 for anything else"""
    if len(allele) == 1 and allele.upper() in "ACGT":
        return "ACGT".index(allele.upper())
    return -1 if choose and allele == "." else -2


def files(lines, planes, min_alt=4, z_min=3.0, scorer=score):
    """(EVIDENCE.txt, EVIDENCE.HIST.txt) as text for the listed lines [(chrom, pos, ref, alt)] and their planes [L][4][3][64]"""
    planes = np.asarray(planes, np.int64).reshape(len(lines), 4, METRICS, BINS)
    ref = [nt_code(x[2], False) for x in lines]
    s = scorer(planes, ref, [nt_code(x[3], True) for x in lines])
    ev, hs = [], []
    for l, (chrom, pos, ref_text, alt_text) in enumerate(lines):
        used = int(s.alt_used[l])
        n_ref, n_alt = int(s.ints[l, 0, 0]), int(s.ints[l, 0, 1])
        cols = [chrom, str(pos), ref_text, "ACGT"[used] if used >= 0 else alt_text, str(n_ref), str(n_alt)]
        flags = []
        for m in range(METRICS):
            cols += [str(int(s.med[l, m, 0])), str(int(s.med[l, m, 1]))]
            if s.ints[l, m, 2] < 0:
                cols.append(".")
                continue
            z2 = float(s.z2[l, m])
            cols.append("%.4f" % (-math.sqrt(-z2) if z2 < 0 else math.sqrt(z2)))
            if z2 <= -(z_min * z_min):
                flags.append(FLAG_NAMES[m])
        tested = used >= 0 and n_alt >= min_alt and n_ref >= min_alt
        ev.append("\t".join(cols + ["UNTESTED" if not tested else ",".join(flags) or "PASS"]) + "\n")
        for nt in (ref[l] if 0 <= ref[l] <= 3 else -1, used):
            if nt < 0:
                continue
            for m in range(METRICS):
                for b in np.flatnonzero(planes[l, nt, m]):
                    hs.append(f"{chrom}\t{pos}\t{'ACGT'[nt]}\t{METRIC_NAMES[m]}\t{b}\t{planes[l, nt, m, b]}\n")
    return "".join(ev), "".join(hs)


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, src, keys, mbq=20, mrq=20, reads=None):
        self.name, self.mbq, self.mrq = name, int(mbq), int(mrq)
        self.reads = src if not isinstance(src, tuple) else reads
        self.buf, self.rec_off = pm.as_stream(src)
        self.keys = np.asarray(keys, np.uint64)
        assert len(self.keys) > 0 and np.all(self.keys[1:] > self.keys[:-1]), name
        self._want = None

    @property
    def n_reads(self):
        return len(self.rec_off)

    @property
    def stream(self):
        return self.buf, self.rec_off

    def want(self, **kw):
        if kw:
            return count(self.stream, self.keys, self.mbq, self.mrq, **kw)
        if self._want is None:  # computed once, shared by every test, never changed
            self._want = count(self.stream, self.keys, self.mbq, self.mrq)
            self._want.hist.setflags(write=False)
        return self._want

    def outside_window(self):
        """the distinct (workgroup, key) pairs of counted columns whose key lies outside the workgroup's LDS window"""
        geo = geometry()
        assert geo.reads == pm.geometry().reads  # pm.window_bases groups the reads as this kernel does
        rd, ki = self.want(detail=True)[2][:2]
        g = rd // geo.reads
        rel = ki - pm.window_bases(self.stream, self.keys)[g]
        out = (rel < 0) | (rel >= geo.window)
        return len(set(zip(g[out].tolist(), ki[out].tolist())))

    def __repr__(self):
        return f"Case({self.name}: {self.n_reads} reads, {len(self.keys)} keys, mbq={self.mbq}, mrq={self.mrq})"


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _nz(a):
    """{bin: count} of one histogram"""
    return {int(b): int(a[b]) for b in np.flatnonzero(a)}


@functools.lru_cache(None)
def deterministic_cases():
    geo = geometry()
    R, W = geo.reads, geo.window
    out = []

    def add(name, src, keys, mbq=20, mrq=20, reads=None):
        c = Case(name, src, keys, mbq, mrq, reads)
        out.append(c)
        return c

    K = span_keys(0, 990, 1200)
    at = lambda p: p - 990  # noqa: E731  (index of position p in K)
    allA = lambda n: "A" * n  # noqa: E731
    bins = lambda c, m: _nz(c.want().hist[:, :, m, :].sum((0, 1)))  # noqa: E731  (the pooled histogram of metric m)
    # ---- the clamp of each metric ----
    c = add("qualities_62_63_64_93", [read(0, 999, "4M", _rng("q"), qual=[62, 63, 64, 93], seq=allA(4))], K)
    assert bins(c, BQ) == {62: 1, 63: 3}
    c = add("mapq_3_4_251_252_255_with_mrq_0", [read(0, 999, "1M", _rng("m"), mapq=m, seq="C", qual=[30]) for m in (3, 4, 251, 252, 255)], K, mrq=0)
    assert bins(c, MQ) == {0: 1, 1: 1, 62: 1, 63: 2}
    c = add("mapq_60_is_bin_15", [read(0, 999, "3M", _rng("m60"), mapq=60)], K)
    assert bins(c, MQ) == {15: 3}
    c = add("d_63_and_64_on_a_130_base_read", [read(0, 999, "130M", _rng("130"))], K)
    assert bins(c, POS)[63] == 4 and bins(c, POS)[62] == 2 and sum(bins(c, POS).values()) == 130  # i = 63 .. 66: d = 63, 64, 64, 63
    # ---- where in the read ----
    c = add("odd_l_seq_9", [read(0, 999, "9M", _rng("9"))], K)
    assert bins(c, POS) == {0: 2, 1: 2, 2: 2, 3: 2, 4: 1}
    c = add("even_l_seq_10", [read(0, 999, "10M", _rng("10"))], K)
    assert bins(c, POS) == {0: 2, 1: 2, 2: 2, 3: 2, 4: 2}
    for name, cigar, want in (("leading_5S", "5S10M", {0: 1, 1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 2, 7: 1}), ("leading_5H", "5H10M", {0: 2, 1: 2, 2: 2, 3: 2, 4: 2}),
                              ("insertion_in_front", "5M2I5M", {0: 2, 1: 2, 2: 2, 3: 2, 4: 2}), ("deletion_in_front", "5M2D5M", {0: 2, 1: 2, 2: 2, 3: 2, 4: 2}),
                              ("clips_at_both_ends", "3S6M3S2H", {3: 2, 4: 2, 5: 2})):
        c = add(name + "_" + cigar, [read(0, 999, cigar, _rng(name))], K)
        assert bins(c, POS) == want, (name, bins(c, POS))
    c = add("insertion_shifts_i_5M2I5M_one_key", [read(0, 999, "5M2I5M", _rng("ins1"))], K[at(1005):at(1005) + 1])
    assert bins(c, POS) == {4: 1}  # the column at 1005 is i = 7 of 12
    c = add("deletion_does_not_shift_i_5M2D5M_one_key", [read(0, 999, "5M2D5M", _rng("del1"))], K[at(1007):at(1007) + 1])
    assert bins(c, POS) == {4: 1}  # the column at 1007 is i = 5 of 10
    # ---- what is no counted column ----
    c = add("key_inside_an_N_gap_and_one_past_the_end", [read(0, 999, "5M10N5M", _rng("gap"))], make_keys([(0, 1002), (0, 1010), (0, 1016), (0, 1021)]))
    assert c.want().hist.sum((1, 2, 3)).tolist() == [3, 0, 3, 0]
    c = add("key_inside_a_deletion_dense_keys", [read(0, 999, "10M20D10M", _rng("dd")), read(0, 999, "10M20N10M", _rng("dn"))], K)
    assert c.want().stats == (2, 40) and c.want().hist[at(1010):at(1030)].sum() == 0
    c = add("non_ACGT_base_at_the_key", [read(0, 999, "5M", _rng("n"), seq="ACNGT"), read(0, 999, "5M", _rng("n2"), seq="ACRGT")], K[at(1002):at(1002) + 1])
    assert c.want().stats == (2, 0)
    c = add("key_on_a_reference_without_reads", [read(0, 999, "5M", _rng("r"))], np.concatenate([K, span_keys(7, 1000, 1004)]))
    assert c.want().hist[len(K):].sum() == 0 and c.want().stats == (1, 5)
    # ---- thresholds ----
    c = add("quality_below_and_at_mbq", [read(0, 999, "3M", _rng("mbq"), qual=[19, 20, 21], seq=allA(3))], K)
    assert bins(c, BQ) == {20: 1, 21: 1}
    c = add("mapq_below_and_at_mrq", [read(0, 999, "2M", _rng("mrq"), mapq=m) for m in (19, 20, 21)], K)
    assert c.want().stats == (2, 4) and bins(c, MQ) == {5: 4}
    bits = [1 << b for b in range(12)]
    c = add("each_flag_bit_alone", [read(0, 999, "4M", _rng("fl"), flag=f) for f in [0] + bits], K)
    assert c.want().stats == (1 + 12 - 4, 4 * 9)
    c = add("unplaced_reads_first", [read(-1, 999, "4M", _rng("un")), read(0, -1, "4M", _rng("un")), read(0, 999, "4M", _rng("un"))], K)
    assert c.want().stats == (1, 4)
    c = add("removed_operations_5M0D2I1P5M0N", [read(0, 999, "5M0D2I1P5M0N", _rng("rm"))], K)
    assert c.want().stats == (1, 10)
    c = add("all_sixteen_base_codes", [read(0, 999, "32M", _rng("codes"), seq=pm.SEQ_CODE * 2)], K, mbq=0)
    assert c.want().stats == (1, 8)
    top = (1 << 31) - 1
    c = add("keys_at_the_top_of_the_coordinate_range", [read(top, top - 30, "10M2I10M5D5M", _rng("top"), flag=0x10)], span_keys(top, top - 40, top))
    assert int(c.keys[-1]) == (top << 32) | top and c.want().stats == (1, 25)
    # ---- workgroups and order ----
    rs = [read(0, 999 + (i % 3), "30M", _rng(f"wg{i}"), flag=0x10 * (i & 1)) for i in range(R + 1)]
    c = add("257_reads", rs, make_keys([(0, 1010), (0, 1020)]))
    assert c.n_reads == R + 1 and c.want().stats == (R + 1, 2 * (R + 1))
    rg = _rng("walk")
    walk_reads = [read(0, 999 + 3 * i, ("40M2I40M", "40M3D40M", "80M", "5S30M1I20M1D30M")[i % 4], rg, flag=0x10 * (i & 1)) for i in range(600)]
    wide = span_keys(0, 1000, 2999)
    c = add("walk_across_2000_positions_dense", walk_reads, wide)
    assert c.outside_window() >= 10
    sparse = wide[::37]
    c = add("walk_across_2000_positions_sparse", walk_reads, sparse)
    add("reads_in_random_order", [walk_reads[i] for i in _rng("perm").permutation(len(walk_reads))], sparse)
    add("two_references", [read(3, 999, "10M2I10M", _rng("tr")), read(4, 999, "10M2D10M", _rng("tr"), flag=0x10)],
        np.concatenate([span_keys(3, 1000, 1009), span_keys(4, 1005, 1030)]))
    # ---- the LDS window: the W keys from the first key not below the start of the workgroup's first placed read ----
    wk = make_keys([(0, 1000 + 5 * i) for i in range(W + 3)])
    c = add("the_windows_last_key_and_the_first_beyond", [read(0, 999, f"{5 * (W + 3)}M", _rng("win"))], wk)
    assert pm.window_bases(c.stream, c.keys)[0] == 0 and c.outside_window() == 3 and np.all(c.want().hist.sum((1, 2, 3)) == 3)
    c = add("second_read_starts_in_front_of_the_window", [read(0, 1009, "40M", _rng("w1")), read(0, 999, "40M", _rng("w2"), flag=0x10)], make_keys([(0, 1005), (0, 1012), (0, 1030)]))
    assert pm.window_bases(c.stream, c.keys)[0] == 1 and c.want().hist.sum((1, 2, 3)).tolist() == [3, 6, 6] and c.outside_window() == 1
    for P in (1, W - 1, W, W + 1):
        c = add(f"list_of_{P}_keys", [read(0, 999 + 2 * s, "40M1D20M", _rng(f"l{P}{s}"), flag=0x10 * (s & 1)) for s in range(12)], make_keys([(0, 1003 + 6 * i) for i in range(P)]))
        assert len(c.keys) == P
    c = add("all_reads_behind_the_last_key", [read(0, 5999, "10M", _rng("bh")) for _ in range(5)], K)
    assert c.want().stats == (5, 0)
    c = add("all_reads_before_the_first_key", [read(0, 99, "10M", _rng("bf")) for _ in range(5)], K)
    assert c.want().stats == (5, 0)
    return tuple(out)


DEPTH_READS = 20_000


@functools.lru_cache(None)
def depth_case(n=DEPTH_READS):
    """n identical reads over one listed key: every column lands in one bin of every metric"""
    r = read(0, 999, "80M", np.random.default_rng(5), flag=0x10, name="d", qual=[37] * 80, seq="ACGT" * 20)
    c = Case(f"depth_{n}_identical_reads_one_key", [r] * n, make_keys([(0, 1030)]))
    w = c.want()
    assert w.stats == (n, n) and _nz(w.hist[0, 2, BQ]) == {37: n} and _nz(w.hist[0, 2, MQ]) == {15: n} and _nz(w.hist[0, 2, POS]) == {30: n} and w.hist.sum() == 3 * n
    return c


FUZZ_SEEDS = (29001, 29002, 29003)


def sharpen(rng, reads, share=0.3):
    """helpers.random_amplicon_reads draws qualities up to 40 and MAPQ up to 60: `share` of the reads get values at and beyond the last bin"""
    for r in reads:
        if rng.random() < share:
            r["mapq"] = int(rng.choice([251, 252, 255, 100]))
            r["qual"] = [int(x) for x in rng.choice([19, 20, 40, 62, 63, 64, 93, 255], size=len(r["qual"]))]
    return reads


@functools.lru_cache(None)
def fuzz_cases():
    """three seeded streams of <= 3000 reads of helpers.random_amplicon_reads(odd_ops=0.3), each once with a sparse list and once with
    every position listed; together they must hold enough of everything (asserted here, on the CPU, while the table is built)"""
    from tests import helpers

    out = []
    clamped = [0, 0, 0]
    soft = ins = outside = 0
    for k, seed in enumerate(FUZZ_SEEDS):
        rng = np.random.default_rng(seed)
        n_amp = int(rng.integers(10, 24))
        amps, pairs = [], []
        for a in range(n_amp):
            ref_id = a * 3 // n_amp
            start = 500 + 170 * a + int(rng.integers(0, 40))
            amps.append((ref_id, start, start + 130))
            pairs += [(ref_id, p) for p in range(start - 10, start + 190)]
        dense = make_keys(pairs)
        sparse = np.sort(rng.choice(dense, size=3 * n_amp, replace=False))
        n = (3000, 1777, 2500)[k]
        reads = sharpen(rng, helpers.random_amplicon_reads(rng, None, amps, n, read_len=(40, 150), name_len=(1, 40), odd_ops=0.3, unplaced=0.02))
        if k == 1:
            reads = [reads[i] for i in rng.permutation(len(reads))]
        gaps = {int(i): int(rng.integers(1, 70)) for i in rng.integers(0, len(reads), size=20)}
        src = build_stream(reads, lead=int(rng.integers(0, 40)), gaps=gaps, trail=int(rng.integers(16, 64)))
        for style, keys in (("sparse", sparse), ("dense", dense)):
            c = Case(f"fuzz_{seed}_{len(reads)}_reads_{style}", src, keys, mbq=(20, 21, 10)[k], mrq=(20, 5, 21)[k], reads=reads)
            _, _, (rd, ki, sb, ib, values) = c.want(detail=True)
            for m in range(METRICS):
                clamped[m] += int((values[m] >= BINS - 1).sum())  # in the last bin (a MAPQ never lies beyond it: 255 >> 2 = 63)
            soft += int((sb > 0).sum())
            ins += int((ib > 0).sum())
            outside += c.outside_window()
            out.append(c)
    assert min(clamped) >= 50, clamped
    assert soft >= 50 and ins >= 50, (soft, ins)
    assert outside >= 10, outside
    return tuple(out)


@functools.lru_cache(None)
def cases():
    """the whole table: deterministic cases, the depth case, the fuzz streams"""
    return deterministic_cases() + (depth_case(),) + fuzz_cases()


# variant -> the deterministic cases that must catch it (tests/test_evidence_model.py asserts that each of them does)
CAUGHT_BY = {
    "i_without_soft_clips": ("leading_5S_5S10M", "clips_at_both_ends_3S6M3S2H"),
    "i_not_advanced_by_I": ("insertion_in_front_5M2I5M", "insertion_shifts_i_5M2I5M_one_key"),
    "i_advanced_by_D": ("deletion_in_front_5M2D5M", "deletion_does_not_shift_i_5M2D5M_one_key"),
    "d_from_i_alone": ("odd_l_seq_9", "even_l_seq_10", "d_63_and_64_on_a_130_base_read"),
    "hard_clip_in_l_seq": ("leading_5H_5H10M", "clips_at_both_ends_3S6M3S2H"),
    "bins_clamped_at_62": ("qualities_62_63_64_93", "mapq_3_4_251_252_255_with_mrq_0", "d_63_and_64_on_a_130_base_read"),
    "bins_not_clamped": ("qualities_62_63_64_93", "d_63_and_64_on_a_130_base_read"),
    "mapq_not_shifted": ("mapq_3_4_251_252_255_with_mrq_0", "mapq_60_is_bin_15"),
    "mbq_off_by_one": ("quality_below_and_at_mbq",),
    "mrq_off_by_one": ("mapq_below_and_at_mrq",),
}


# ---------------------------------------------------------------------------------------------------------------------------
# score cases: (name, planes [P][4][3][64], ref_nt, alt_nt); every plane holds the same histogram under all three metrics unless said
# ---------------------------------------------------------------------------------------------------------------------------
def plane(**nts):
    """one position's [4][3][64] from {nt letter: {bin: count}} (the same histogram under every metric)"""
    p = np.zeros((4, METRICS, BINS), np.int64)
    for nt, h in nts.items():
        for b, n in h.items():
            p[" ACGT".index(nt) - 1, :, b] = n
    return p


@functools.lru_cache(None)
def score_cases():
    out = []

    def add(name, planes, ref, alt):
        out.append((name, np.stack(planes), np.asarray(ref, np.int64), np.asarray(alt, np.int64)))
        return score(*out[-1][1:])

    s = add("all_reads_in_one_bin", [plane(A={40: 100}, C={40: 7})], [0], [1])
    assert s.ints[0, 0].tolist() == [100, 7, -1] and s.z2[0, 0] == 0.0 and s.med[0, 0].tolist() == [40, 40]  # v = 0
    s = add("no_alt_reads", [plane(A={40: 100, 30: 5})], [0], [1])
    assert s.ints[0, 0].tolist() == [105, 0, -1] and s.med[0, 0].tolist() == [40, -1]
    s = add("no_ref_reads", [plane(C={40: 100, 30: 5})], [0], [1])
    assert s.ints[0, 0].tolist() == [0, 105, -1] and s.med[0, 0].tolist() == [-1, 40]
    s = add("alt_wholly_below_ref", [plane(A={40: 50, 41: 50}, C={20: 5, 21: 5})], [0], [1])
    assert s.ints[0, 0].tolist() == [100, 10, 0] and s.z2[0, 0] < -9
    s = add("alt_wholly_above_ref", [plane(A={20: 50, 21: 50}, C={40: 5, 41: 5})], [0], [1])
    assert s.ints[0, 0].tolist() == [100, 10, 2 * 100 * 10] and s.z2[0, 0] > 9
    s = add("ties_only_partly", [plane(G={10: 3, 11: 4, 12: 2}, T={10: 1, 11: 2, 13: 1})], [2], [3])
    assert s.ints[0, 0].tolist() == [9, 4, 1 * 3 + 2 * (2 * 3 + 4) + 1 * (2 * 9)]  # T at 10: 3 ties; at 11: 3 below, 4 ties; at 13: all 9 below
    s = add("medians_of_even_and_odd_sides", [plane(A={5: 2, 9: 2}, C={5: 2, 9: 3})], [0], [1])
    assert s.med[0, 0].tolist() == [5, 9]  # 2 cum >= n is reached at bin 5 for n = 4 and only at bin 9 for n = 5
    big = (1 << 29)
    s = add("N_is_2_to_the_30_minus_1", [plane(A={10: big, 20: big - 2}, C={12: 1})], [0], [1])
    assert int(s.ints[0, 0, :2].sum()) == (1 << 30) - 1 and s.ints[0, 0, 2] == 2 * big
    s = add("N_is_2_to_the_30", [plane(A={10: big, 20: big - 1}, C={12: 1})], [0], [1])
    assert int(s.ints[0, 0, :2].sum()) == 1 << 30 and s.ints[0, 0, 2] == -1 and s.z2[0, 0] == 0.0
    s = add("choose_with_a_tie", [plane(A={30: 90, 31: 9}, C={20: 4, 25: 1}, T={22: 5}), plane(G={30: 50}, A={29: 3}, C={28: 3}, T={31: 3})], [0, 2], [-1, -1])
    assert s.alt_used.tolist() == [1, 0]
    s = add("choose_when_the_reference_has_the_most_reads", [plane(A={30: 90, 31: 9}, T={22: 5})], [0], [-1])
    assert s.alt_used.tolist() == [3]
    s = add("choose_without_any_other_read", [plane(C={30: 90, 31: 9})], [1], [-1])
    assert s.alt_used.tolist() == [0] and s.ints[0, 0].tolist() == [99, 0, -1]
    s = add("ref_equals_alt_and_unusable_alleles", [plane(A={30: 9, 31: 9}, C={20: 5, 33: 1})] * 5, [0, -2, 0, 4, 1], [0, 1, -2, 1, 4])
    assert s.alt_used.tolist() == [-1] * 5 and s.ints[:, 0, 2].tolist() == [-1] * 5 and s.ints[:, 0, 0].tolist() == [18, 0, 18, 0, 6] and s.ints[:, 0, 1].tolist() == [0] * 5
    p = plane(A={40: 60, 41: 40}, C={40: 6, 41: 4})
    p[1, MQ] = 0
    p[1, MQ, 3] = 10
    p[1, POS] = 0
    p[1, POS, 50] = 10
    s = add("a_different_histogram_under_every_metric", [p], [0], [1])
    assert s.z2[0, 0] == 0.0 and s.ints[0, 0, 2] == 100 * 10 and s.z2[0, 1] < 0 and s.z2[0, 2] > 0
    return tuple(out)


SCORE_CAUGHT_BY = {
    "ties_counted_whole": ("ties_only_partly", "a_different_histogram_under_every_metric"),
    "tie_term_dropped": ("ties_only_partly", "all_reads_in_one_bin"),
    "median_upper": ("medians_of_even_and_odd_sides",),
    "choose_takes_ref": ("choose_when_the_reference_has_the_most_reads", "choose_with_a_tie"),
    "choose_ties_upwards": ("choose_with_a_tie", "choose_without_any_other_read"),
}


def random_planes(rng, P):
    """P random positions: a few populated bins per nt and metric, depths from a handful to thousands, some empty sides, some single bins"""
    hist = np.zeros((P, 4, METRICS, BINS), np.int64)
    for p in range(P):
        for nt in range(4):
            depth = int(rng.choice([0, 1, 3, 10, 40, 300, 5000, 200000]))
            for m in range(METRICS):
                nb = int(rng.integers(1, 7))
                b = rng.choice(BINS, size=nb, replace=False)
                hist[p, nt, m, b] = rng.multinomial(depth, rng.dirichlet(np.ones(nb)))
    return hist, rng.integers(-1, 5, size=P), rng.integers(-2, 5, size=P)


# ---------------------------------------------------------------------------------------------------------------------------
# the table on a device
# ---------------------------------------------------------------------------------------------------------------------------
def upload(case, first=0, last=None):
    """(bam, rec_off, keys) of the case's reads [first, last) as device tensors for Context.read_evidence"""
    import torch

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
    return up(case.buf, np.uint8), up(case.rec_off[first:last], np.int64), up(case.keys, np.int64)


def device_result(ctx, hist, stats):
    import torch

    ctx.sync()
    torch.cuda.synchronize()
    return Result(hist.cpu().numpy().astype(np.int64), None if stats is None else tuple(int(x) for x in stats.cpu().tolist()))


def differences(got, want, stats=True):
    """[] or what differs between a device Result and the model's"""
    bad = []
    if not np.array_equal(got.hist, want.hist):
        at = np.argwhere(got.hist != want.hist)
        bad.append(f"{len(at)} bins differ, first at (key index, nt, metric, bin) {at[0].tolist()}: {int(got.hist[tuple(at[0])])} != {int(want.hist[tuple(at[0])])}")
    if stats and tuple(got.stats) != tuple(want.stats):
        bad.append(f"stats {got.stats} != {want.stats}")
    return bad


def score_differences(got, want):
    """[] or what differs between two Scores: the integers, and z2 bit for bit"""
    bad = []
    for name, g, w in (("ints", got.ints, want.ints), ("med", got.med, want.med), ("alt_used", got.alt_used, want.alt_used)):
        if not np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)):
            at = np.argwhere(np.asarray(g, np.int64) != np.asarray(w, np.int64))
            bad.append(f"{name}: {len(at)} differ, first at {at[0].tolist()}: {np.asarray(g)[tuple(at[0])]} != {np.asarray(w)[tuple(at[0])]}")
    gz, wz = np.ascontiguousarray(got.z2, np.float64).view(np.uint64), np.ascontiguousarray(want.z2, np.float64).view(np.uint64)
    if not np.array_equal(gz, wz):
        at = np.argwhere(gz != wz)
        bad.append(f"z2: {len(at)} differ in their bits, first at {at[0].tolist()}: {np.asarray(got.z2)[tuple(at[0])]!r} != {np.asarray(want.z2)[tuple(at[0])]!r}")
    return bad
