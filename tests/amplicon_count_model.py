"""The amplicon counting kernels' test model -- TEST INFRASTRUCTURE (never imported by the product).

Two restatements of the definition in the contract comment of ampli_pileup_amplicon_count (include/amplisolve_hip.h) over the
read dicts and record streams of tests/pileup_model.py, written differently on purpose so that they check each other:
  * count: numpy over flat arrays -- every kept read against EVERY amplicon (a reads x amplicons matrix, no candidate search), every
    column of every match run at once;
  * walk:  a per-read Python loop in plain integers: the candidate range from `reach` and `lo` by bisection, one operation and one
    column at a time.
`wrong=` switches count (and layers) to one deliberately wrong variant (WRONG_VARIANTS); tests/test_amplicon_count_model.py shows that
each of them is caught by named deterministic cases (CAUGHT_BY).  layers is the gather of ampli_amplicon_layers.  geometry() reads the
kernel's constexpr lines; cases() is the named case table, and every case that claims an edge asserts it while the table is built.
"""
from __future__ import annotations

import bisect
import collections
import functools
import os
import re
import struct
import zlib

import numpy as np

from tests import pileup_model as pm
from tests.pileup_model import build_stream, read  # noqa: F401

KERNEL_SOURCE = os.path.join(pm.ROOT, "amplisolve_amd", "csrc", "ampli_amplicon_count.hip")
ABSENT = np.iinfo(np.int32).min

Geometry = collections.namedtuple("Geometry", "reads window")


@functools.lru_cache(None)
def geometry():
    """(reads per workgroup, walk entries of the LDS window) as ampli_amplicon_count.hip states them"""
    text = open(KERNEL_SOURCE).read()
    vals = {}
    for name in ("READS", "WINDOW"):
        m = re.search(r"^constexpr\s+int\s+AMPCOUNT_%s\s*=\s*([0-9][0-9\s*]*);" % name, text, re.M)
        assert m, f"no `constexpr int AMPCOUNT_{name} = ...;` line in {KERNEL_SOURCE}"
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        vals[name] = v
    return Geometry(vals["READS"], vals["WINDOW"])


# ---------------------------------------------------------------------------------------------------------------------------
# the amplicons
# ---------------------------------------------------------------------------------------------------------------------------
Amplicons = collections.namedtuple("Amplicons", "lo hi reach amp_off row_of ref first last")


def make_amplicons(intervals):
    """[(ref_id, first, last)] in BED order -> the sorted arrays of the contract: lo, hi, reach uint64 [A], amp_off int64 [A + 1], row_of
    (sorted index -> index into `intervals`), and ref / first / last int64 [A] for the model's own arithmetic"""
    iv = [(int(r), int(f), int(l)) for r, f, l in intervals]
    assert all(r >= 0 and 1 <= f <= l < 2 ** 31 for r, f, l in iv)
    order = sorted(range(len(iv)), key=lambda k: ((iv[k][0] << 32) | iv[k][1], (iv[k][0] << 32) | iv[k][2], k))
    ref = np.asarray([iv[k][0] for k in order], np.int64)
    first = np.asarray([iv[k][1] for k in order], np.int64)
    last = np.asarray([iv[k][2] for k in order], np.int64)
    lo = (ref.astype(np.uint64) << np.uint64(32)) | first.astype(np.uint64)
    hi = (ref.astype(np.uint64) << np.uint64(32)) | last.astype(np.uint64)
    reach = np.maximum.accumulate(hi) if len(hi) else hi
    amp_off = np.concatenate([[0], np.cumsum(last - first + 1)]).astype(np.int64)
    return Amplicons(lo, hi, reach, amp_off, np.asarray(order, np.int64), ref, first, last)


# name -> what is wrong; count(..., wrong=name) / layers(..., wrong=name) computes that variant.  One per rule of the definition.
WRONG_VARIANTS = {
    "tie_highest_index": "among equal overlap and equal anchor distance the highest index wins",
    "anchor_ignores_strand": "the anchor distance of a reverse read is taken at its first position too",
    "span_from_l_seq": "the span is taken as pos + 1 .. pos + l_seq: D and N do not lengthen it, S and I do",
    "outside_counted": "columns outside the amplicon's interval are counted, in whatever cell the arithmetic gives",
    "threshold_strict": "overlap x 100 > min_overlap x span instead of >=",
    "search_on_hi": "the candidate range starts at the first a with hi[a] >= span_first: a nested amplicon hides its container",
    "reverse_not_added": "reverse reads do not add to slot + 4",
    "cell_off_by_one": "the cell of position x is amp_off[a] + x - first[a] + 1",
    "non_acgt_counted": "a base that is not A/C/G/T is counted as A",
    "offtarget_to_nearest": "a read whose assignment does not stand is given to the nearest amplicon of its reference",
    "total_drops_beyond_L": "d_total sums the first L covering amplicons only",
}

# count's result: counts int64 [W][8], amp_reads int64 [A][2], stats (kept, assigned, bases counted, bases clipped), and per read of the
# stream: assigned (sorted amplicon index; -1 off-target or R = 0; -2 not kept), decided (0 overlap, 1 anchor, 2 index; -1 not assigned),
# under (kept, some overlap >= 1, under the threshold), n_clipped (clipped columns)
Result = collections.namedtuple("Result", "counts amp_reads stats assigned decided under n_clipped")


def _flat_ops(buf, h, rd):
    """every CIGAR operation of the reads rd, flat: (read, op, len, reference and query positions consumed by the read's earlier ones)"""
    nc = h.n_cigar[rd]
    o_read = np.repeat(rd, nc)
    first = np.cumsum(nc) - nc
    o_idx = np.arange(len(o_read)) - np.repeat(first, nc)
    v = pm._le(buf, h.cig[o_read] + 4 * o_idx, 4)
    op, ln = v & 15, v >> 4
    radv, qadv = np.where(np.isin(op, pm.REF_OPS), ln, 0), np.where(np.isin(op, pm.QUERY_OPS), ln, 0)

    def before(adv):
        c = np.cumsum(adv) - adv
        return c - np.repeat(c[first[nc > 0]], nc[nc > 0]) if len(c) else c

    return o_read, op, ln, radv, before(radv), before(qadv)


def count(src, amps, mbq, mrq, min_overlap=50, wrong=None):
    """Result of the stream `src` (read dicts or (buf, rec_off)) on the amplicons `amps`: the vectorised restatement"""
    assert wrong is None or wrong in WRONG_VARIANTS, wrong
    buf, rec_off = pm.as_stream(src)
    n, A, W = len(rec_off), len(amps.lo), int(amps.amp_off[-1])
    h = pm.headers(buf, rec_off)
    keep = (h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & pm.READ_MASK) == 0) & (h.mapq >= mrq)
    rd = np.flatnonzero(keep)
    rev = (h.flag & 0x10) != 0
    o_read, op, ln, radv, rbef, qbef = _flat_ops(buf, h, rd)
    R = np.bincount(o_read, weights=radv, minlength=n).astype(np.int64)
    if wrong == "span_from_l_seq":
        R = h.l_seq.copy()
    sf, sl = h.pos + 1, h.pos + R
    assigned = np.where(keep, -1, -2).astype(np.int64)
    decided = np.full(n, -1, np.int64)
    under = np.zeros(n, bool)
    cand = rd[R[rd] > 0]
    if len(cand) and A:
        c_sf, c_sl, c_rev = sf[cand, None], sl[cand, None], rev[cand, None]
        same = h.ref_id[cand, None] == amps.ref[None, :]
        ov = np.where(same, np.maximum(np.minimum(c_sl, amps.last[None, :]) - np.maximum(c_sf, amps.first[None, :]) + 1, 0), 0)
        an = np.where(same, np.where(c_rev & (wrong != "anchor_ignores_strand"), np.abs(c_sl - amps.last[None, :]), np.abs(c_sf - amps.first[None, :])), 0)
        if wrong == "search_on_hi":  # the candidates: from the bisection's answer on the (unsorted) hi to the last lo <= span_last
            key_f = (h.ref_id[cand].astype(np.uint64) << np.uint64(32)) | sf[cand].astype(np.uint64)
            c0 = np.asarray([_bisect_left(amps.hi, int(k)) for k in key_f])
            ov = np.where(np.arange(A)[None, :] >= c0[:, None], ov, -1)
        best = ov.max(1)
        m1 = ov == best[:, None]
        an1 = np.where(m1, an, np.iinfo(np.int64).max)
        m2 = m1 & (an1 == an1.min(1)[:, None])
        idx = A - 1 - np.argmax(m2[:, ::-1], 1) if wrong == "tie_highest_index" else np.argmax(m2, 1)
        lhs, rhs = best * 100, min_overlap * R[cand]
        stands = (best >= 1) & ((lhs > rhs) if wrong == "threshold_strict" else (lhs >= rhs))
        assigned[cand[stands]] = idx[stands]
        decided[cand[stands]] = np.where(m1.sum(1) == 1, 0, np.where(m2.sum(1) == 1, 1, 2))[stands]
        under[cand] = (best >= 1) & ~stands
        if wrong == "offtarget_to_nearest":
            gap = np.where(same, np.maximum(np.maximum(amps.first[None, :] - c_sl, c_sf - amps.last[None, :]), 0), np.iinfo(np.int64).max)
            near = same.any(1) & ~stands
            assigned[cand[near]] = np.argmin(gap, 1)[near]
    counts = np.zeros(W * 8, np.int64)
    amp_reads = np.zeros(A * 2, np.int64)
    on = np.flatnonzero(assigned >= 0)
    amp_reads += np.bincount(assigned[on] * 2 + rev[on], minlength=A * 2)
    # the columns of the match runs of the assigned reads
    runs = np.flatnonzero(np.isin(op, pm.MATCH_OPS) & (ln > 0) & (assigned[o_read] >= 0))
    rl = ln[runs]
    base_run = np.repeat(runs, rl)
    j = np.arange(len(base_run)) - np.repeat(np.cumsum(rl) - rl, rl)
    r_ = o_read[base_run]
    a_ = assigned[r_]
    x = h.pos[r_] + 1 + rbef[base_run] + j
    q = qbef[base_run] + j
    inside = (x >= amps.first[a_]) & (x <= amps.last[a_])
    n_clipped = np.bincount(r_[~inside], minlength=n)
    w = amps.amp_off[a_] + x - amps.first[a_] + (1 if wrong == "cell_off_by_one" else 0)
    ok = (inside if wrong != "outside_counted" else np.ones(len(x), bool)) & (w >= 0) & (w < W)
    byte = buf[h.seq[r_] + (q >> 1)].astype(np.int64)
    nt = pm._B4[np.where((q & 1) == 0, byte >> 4, byte & 15)]
    if wrong == "non_acgt_counted":
        nt = np.maximum(nt, 0)
    ok &= (nt >= 0) & (buf[h.qual[r_] + q].astype(np.int64) >= mbq)
    counts += np.bincount(w[ok] * 8 + nt[ok], minlength=W * 8)
    if wrong != "reverse_not_added":
        okr = ok & rev[r_]
        counts += np.bincount(w[okr] * 8 + 4 + nt[okr], minlength=W * 8)
    return Result(counts.reshape(W, 8), amp_reads.reshape(A, 2), (int(keep.sum()), len(on), int(ok.sum()), int((~inside).sum())), assigned, decided, under,
                  n_clipped)


def _bisect_left(v, key):
    """the kernel's bisection for the first element >= key, on a sequence that need not be sorted"""
    a, b = 0, len(v)
    while a < b:
        mid = (a + b) >> 1
        if int(v[mid]) < key:
            a = mid + 1
        else:
            b = mid
    return a


def walk(src, amps, mbq, mrq, min_overlap=50):
    """(counts, amp_reads, stats) of the same stream, one read, one candidate, one operation and one column at a time, in Python integers"""
    buf, rec_off = pm.as_stream(src)
    b = bytes(buf)
    lo, hi, reach, off = (x.tolist() for x in (amps.lo, amps.hi, amps.reach, amps.amp_off))
    A, W = len(lo), off[-1]
    counts = np.zeros((W, 8), np.int64)
    amp_reads = np.zeros((A, 2), np.int64)
    kept = assigned = added = clipped = 0
    for o in np.asarray(rec_off, np.uint64).tolist():
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, o + 4)
        if ref_id < 0 or pos < 0 or flag & pm.READ_MASK or mapq < mrq:
            continue
        kept += 1
        cig = o + 36 + l_name
        seq = cig + 4 * n_cigar
        qual = seq + (l_seq + 1) // 2
        rev = 1 if flag & 0x10 else 0
        ops = [(v & 15, v >> 4) for v in struct.unpack_from(f"<{n_cigar}I", b, cig)]
        R = sum(ln for op_, ln in ops if op_ in pm.REF_OPS)
        if R == 0:
            continue
        sf, sl = pos + 1, pos + R
        best = None  # (-overlap, anchor distance, index): the smallest wins
        for a in range(bisect.bisect_left(reach, (ref_id << 32) | sf), bisect.bisect_right(lo, (ref_id << 32) | sl)):
            if lo[a] >> 32 != ref_id:
                continue
            first, last = lo[a] & 0xffffffff, hi[a] & 0xffffffff
            key = (-max(min(sl, last) - max(sf, first) + 1, 0), abs(sl - last) if rev else abs(sf - first), a)
            if best is None or key < best:
                best = key
        if best is None or -best[0] < 1 or -best[0] * 100 < min_overlap * (sl - sf + 1):
            continue
        a = best[2]
        assigned += 1
        amp_reads[a, rev] += 1
        first, last = lo[a] & 0xffffffff, hi[a] & 0xffffffff
        x, q = sf, 0
        for op_, ln in ops:
            if op_ in pm.MATCH_OPS:
                for k in range(ln):
                    if not first <= x + k <= last:
                        clipped += 1
                        continue
                    byte = b[seq + ((q + k) >> 1)]
                    nt = {1: 0, 2: 1, 4: 2, 8: 3}.get(byte & 15 if (q + k) & 1 else byte >> 4)
                    if nt is None or b[qual + q + k] < mbq:
                        continue
                    wi = off[a] + (x + k - first)
                    counts[wi, nt] += 1
                    if rev:
                        counts[wi, 4 + nt] += 1
                    added += 1
            if op_ in pm.REF_OPS:
                x += ln
            if op_ in pm.QUERY_OPS:
                q += ln
    return counts, amp_reads, (kept, assigned, added, clipped)


Layers = collections.namedtuple("Layers", "layers layer_amp total")  # int64 [L][P][8], [L][P], [P][8]


def covering(amps, key):
    """the sorted indices of the amplicons over the position `key` (ref_id << 32 | position)"""
    key = int(key)
    return [a for a in range(len(amps.lo)) if int(amps.lo[a]) <= key <= int(amps.hi[a])]


def layers(counts, amps, keys, L, wrong=None):
    """the gather of ampli_amplicon_layers over the walk counts `counts` [W][8]"""
    assert wrong in (None, "total_drops_beyond_L")
    P = len(keys)
    lay = np.zeros((L, P, 8), np.int64)
    lay[:, :, 0] = ABSENT
    amp = np.full((L, P), -1, np.int64)
    total = np.zeros((P, 8), np.int64)
    for p, key in enumerate(np.asarray(keys, np.uint64).tolist()):
        for l, a in enumerate(covering(amps, key)):
            rec = counts[int(amps.amp_off[a]) + key - int(amps.lo[a])]
            if l < L:
                lay[l, p], amp[l, p] = rec, a
            if l < L or wrong is None:
                total[p] += rec
    return Layers(lay, amp, total)


def window_bases(src, amps, res):
    """int64 [groups]: the walk entry the group's first assigned read begins in -- where its LDS window starts; 0 for a group without one"""
    buf, rec_off = pm.as_stream(src)
    h = pm.headers(buf, rec_off)
    R = geometry().reads
    out = np.zeros((len(rec_off) + R - 1) // R, np.int64)
    for g in range(len(out)):
        idx = np.flatnonzero(res.assigned[g * R:(g + 1) * R] >= 0)
        if len(idx):
            i = g * R + idx[0]
            a = res.assigned[i]
            out[g] = amps.amp_off[a] + max(int(h.pos[i]) + 1 - int(amps.first[a]), 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, src, intervals, keys=None, L=2, mbq=20, mrq=20, min_overlap=50):
        self.name, self.L, self.mbq, self.mrq, self.min_overlap = name, int(L), int(mbq), int(mrq), int(min_overlap)
        self.buf, self.rec_off = pm.as_stream(src)
        self.intervals = list(intervals)
        self.amps = make_amplicons(intervals)
        # the listed positions of the gather: every position of every amplicon and ten on either side, unless given; any order, repeats allowed
        if keys is None:
            keys = np.unique(np.concatenate([(np.uint64(r) << np.uint64(32)) | np.arange(max(f - 10, 1), l + 11, dtype=np.uint64) for r, f, l in intervals]))
        self.keys = np.asarray(keys, np.uint64)
        self._want = self._layers = None

    @property
    def n_reads(self):
        return len(self.rec_off)

    @property
    def stream(self):
        return self.buf, self.rec_off

    def want(self, **kw):
        if kw:
            return count(self.stream, self.amps, self.mbq, self.mrq, self.min_overlap, **kw)
        if self._want is None:  # computed once, shared by every test, never changed
            self._want = count(self.stream, self.amps, self.mbq, self.mrq, self.min_overlap)
            for a in (self._want.counts, self._want.amp_reads):
                a.setflags(write=False)
        return self._want

    def want_layers(self, wrong=None):
        if wrong:
            return layers(self.want().counts, self.amps, self.keys, self.L, wrong)
        if self._layers is None:
            self._layers = layers(self.want().counts, self.amps, self.keys, self.L)
        return self._layers

    def bases(self):
        return window_bases(self.stream, self.amps, self.want())

    def __repr__(self):
        return f"Case({self.name}: {self.n_reads} reads, {len(self.intervals)} amplicons, {len(self.keys)} keys)"


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def key_of(ref_id, pos):
    return (int(ref_id) << 32) | int(pos)


def tiled_amplicons(rng, n_amp, refs=3):
    """tiles of 100 .. 140 positions along `refs` references, every second one overlapping its predecessor by 25 positions; and, so
    that every rule of the assignment meets reads, one amplicon nested two positions into a longer one, one amplicon listed twice and
    one of 40 positions, shorter than any read"""
    out = []
    for r in range(refs):
        at = 500 + int(rng.integers(0, 40))
        for k in range(n_amp // refs):
            length = int(rng.integers(100, 141))
            first = at - 25 if k % 2 else at + int(rng.integers(5, 60))
            out.append((r, first, first + length - 1))
            at = first + length
    s = 20000
    out += [(0, s, s + 299), (0, s + 2, s + 199), (1, s, s + 149), (1, s, s + 149), (2, s, s + 39)]
    return out


FUZZ_SEEDS = (28001, 28002, 28003)
DEPTH_READS = 20_000


@functools.lru_cache(None)
def deterministic_cases():
    """the named cases (a tuple), each built from a fixed seed; every claimed edge is asserted here"""
    R_, WIN = geometry()
    out = []

    def add(name, src, intervals, **kw):
        c = Case(name, src, intervals, **kw)
        assert name not in [o.name for o in out]
        out.append(c)
        return c

    rg = _rng("amplicon")
    one = [(0, 1000, 1099)]
    c = add("read_equals_its_amplicon_A_is_1", [read(0, 999, "100M", rg)], one)
    w = c.want()
    assert w.stats == (1, 1, 100, 0) and w.assigned.tolist() == [0] and w.counts.sum(1).tolist() == [1] * 100 and len(c.amps.lo) == 1
    two = [(0, 1000, 1099), (0, 1100, 1199)]
    c = add("read_one_column_into_the_neighbour", [read(0, 999, "101M", rg), read(0, 1099, "100M", rg, flag=0x10)], two)
    w = c.want()
    assert w.stats == (2, 2, 200, 1) and w.assigned.tolist() == [0, 1] and w.counts[100].sum() == 2  # the neighbour's first cell: its own read only
    over = [(0, 1000, 1100), (0, 1050, 1150)]
    c = add("read_inside_the_overlap_forward", [read(0, 1059, "31M", rg)], over)
    assert c.want().assigned.tolist() == [1] and c.want().decided.tolist() == [1]
    c = add("read_inside_the_overlap_reverse", [read(0, 1059, "31M", rg, flag=0x10)], over)
    assert c.want().assigned.tolist() == [0] and c.want().decided.tolist() == [1] and c.want().counts[:, 4:].sum() == 31
    c = add("equal_overlap_equal_anchor_lowest_index", [read(0, 1009, "50M", rg), read(0, 1049, "50M", rg, flag=0x10)], [(0, 1000, 1100), (0, 1000, 1100), (0, 1000, 1100)])
    assert c.want().assigned.tolist() == [0, 0] and c.want().decided.tolist() == [2, 2]
    nest = [(0, 1000, 1300), (0, 1100, 1150), (0, 1160, 1180)]
    c = add("amplicons_nested_in_a_larger_one", [read(0, 999, "300M", rg), read(0, 1099, "51M", rg), read(0, 1109, "41M", rg, flag=0x10), read(0, 1159, "21M", rg),
                                                 read(0, 1199, "90M", rg), read(0, 1199, "90M", rg, flag=0x10)], nest)
    assert c.want().assigned.tolist() == [0, 1, 1, 2, 0, 0]
    assert _bisect_left(c.amps.hi, key_of(0, 1200)) == 3 and int(c.amps.reach[2]) == key_of(0, 1300)  # hi hides the container, reach does not
    three = [(0, 1000, 1100), (0, 1050, 1150), (0, 1090, 1190)]
    c = add("three_amplicons_over_one_position_L_2", [read(0, 999, "101M", rg), read(0, 1049, "101M", rg, flag=0x10), read(0, 1089, "101M", rg)] * 3, three)
    p = int(np.flatnonzero(c.keys == np.uint64(key_of(0, 1095)))[0])
    lay = c.want_layers()
    assert covering(c.amps, key_of(0, 1095)) == [0, 1, 2] and lay.layer_amp[:, p].tolist() == [0, 1]
    assert lay.total[p].sum() > lay.layers[:, p].sum() > 0 and c.want().assigned.tolist() == [0, 1, 2] * 3
    c = add("span_100_overlap_50_and_49_at_min_overlap_50", [read(0, 999, "100M", rg), read(0, 1000, "100M", rg), read(0, 1000, "100M", rg, flag=0x10)], [(0, 1000, 1049)])
    assert c.want().assigned.tolist() == [0, -1, -1] and c.want().under.tolist() == [False, True, True] and c.want().stats == (3, 1, 50, 50)
    c = add("same_coordinates_on_another_reference", [read(0, 999, "100M", rg), read(1, 999, "100M", rg), read(2, 999, "100M", rg)], [(1, 1000, 1099), (0, 1000, 1099)])
    assert c.want().assigned.tolist() == [0, 1, -1] and c.amps.row_of.tolist() == [1, 0] and not c.want().under.any()
    c = add("D_and_N_carry_the_span_past_the_end", [read(0, 999, "60M30D30M", rg), read(0, 999, "70M25N25M", rg, flag=0x10)], one)
    assert c.want().assigned.tolist() == [0, 0] and c.want().n_clipped.tolist() == [20, 20]
    c = add("N_makes_the_span_too_long", [read(0, 999, "20M200N20M", rg)], [(0, 1000, 1049), (0, 1200, 1249)])
    assert c.want().assigned.tolist() == [-1] and c.want().under.tolist() == [True] and c.want(wrong="span_from_l_seq").assigned.tolist() == [0]
    c = add("soft_and_hard_clips_outside_the_span", [read(0, 999, "5H60S50M10S", rg), read(0, 999, "3S50M60S4H", rg, flag=0x10)], [(0, 1000, 1049), (0, 1050, 1120)])
    assert c.want().assigned.tolist() == [0, 0] and c.want().stats[3] == 0 and c.want(wrong="span_from_l_seq").assigned.tolist() == [1, 1]
    c = add("read_of_only_S_and_I", [read(0, 1009, "10S5I", rg), read(0, 1009, "10M", rg)], one)
    assert c.want().assigned.tolist() == [-1, 0] and c.want().stats[:2] == (2, 1) and not c.want().under[0]
    c = add("amplicon_of_length_1", [read(0, 999, "1M", rg), read(0, 998, "3M", rg), read(0, 999, "2M", rg, flag=0x10)], [(0, 1000, 1000)])
    assert c.want().assigned.tolist() == [0, -1, 0] and c.want().stats == (3, 2, 2, 1) and c.want().counts.shape == (1, 8)
    shifted = [(0, 1000 + i, 1100 + i) for i in range(65)]
    c = add("65_amplicons_shifted_by_one_second_round_of_lanes", [read(0, 1063, "37M", rg), read(0, 1063, "37M", rg, flag=0x10), read(0, 1031, "20M", rg)], shifted)
    assert c.want().assigned.tolist() == [64, 0, 32] and c.want().decided.tolist() == [1, 1, 1] and len(covering(c.amps, key_of(0, 1080))) == 65
    qn = [30] * 10
    c = add("non_ACGT_bases_and_low_qualities", [read(0, 999, "10M", rg, seq="ACGTNRMACG", qual=qn), read(0, 999, "10M", rg, seq="ACGTACGTAC", qual=[19, 20, 21] + [5] * 7)], one)
    assert c.want().stats == (2, 2, 7 + 2, 0)
    c = add("filtered_reads", [read(0, 999, "100M", rg, flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800, 0x1)] + [read(0, 999, "100M", rg, mapq=19), read(0, 999, "100M", rg, mapq=20),
                               read(-1, 999, "100M", rg), read(0, -1, "100M", rg)], one)
    assert c.want().assigned.tolist() == [-2, -2, -2, -2, 0, 0, -2, 0, -2, -2]
    # ---- the LDS window: WIN consecutive walk entries from the one the group's first assigned read begins in ----
    long_ = [(0, 1000, 1000 + WIN + 199), (0, 5000, 5099)]
    c = add("reads_straddle_the_windows_first_and_last_entry", [read(0, 1009, "50M", rg), read(0, 999, "60M", rg), read(0, 1009 + WIN - 30, "30M", rg, flag=0x10),
                                                                read(0, 1009 + WIN - 30, "60M", rg), read(0, 1009 + WIN, "40M", rg)], long_)
    assert c.bases().tolist() == [10] and c.want().assigned.tolist() == [0] * 5
    rel = np.flatnonzero(c.want().counts.sum(1)) - 10
    assert {-10, -1, 0, WIN - 1, WIN, WIN + 39} <= set(rel.tolist())  # cells before, on both ends of, and behind the window
    c = add("read_assigned_outside_the_window_unsorted_stream", [read(0, 4999, "100M", rg), read(0, 999, "100M", rg, flag=0x10), read(0, 4999, "100M", rg)], long_)
    assert c.bases().tolist() == [WIN + 200] and c.want().assigned.tolist() == [1, 0, 1]
    r = read(0, 999, "100M", rg, flag=0x10, name="g")
    c = add("one_read_more_than_a_read_group", [r] * (R_ + 1), one)
    assert c.want().stats == (R_ + 1, R_ + 1, 100 * (R_ + 1), 0) and len(c.bases()) == 2
    c = add("a_group_without_an_assigned_read_then_one_with", [read(0, 2999, "50M", rg, name="o")] * R_ + [read(0, 999, "100M", rg, name="i")] * 3, one)
    assert c.bases().tolist() == [0, 0] and c.want().stats[:2] == (R_ + 3, 3)
    return tuple(out)


@functools.lru_cache(None)
def depth_case(n=DEPTH_READS):
    """n identical reverse reads on one amplicon: every LDS counter takes n / workgroups adds per workgroup, every flush adds to the same cells"""
    r = read(0, 1004, "90M", np.random.default_rng(5), flag=0x10, name="d")
    c = Case(f"depth_{n}_identical_reads", [r] * n, [(0, 1000, 1099)])
    w = c.want()
    assert w.stats == (n, n, 90 * n, 0) and w.amp_reads.tolist() == [[0, n]] and w.counts[5:95].sum(1).tolist() == [2 * n] * 90
    return c


@functools.lru_cache(None)
def fuzz_cases():
    """three seeded streams of <= 3000 reads of helpers.random_amplicon_reads(odd_ops=0.3) over tiled amplicons; together they must hold
    enough of every class (asserted here, on the CPU, while the table is built)"""
    from tests import helpers

    out = []
    tally = collections.Counter()
    for k, seed in enumerate(FUZZ_SEEDS):
        rng = np.random.default_rng(seed)
        iv = tiled_amplicons(rng, int(rng.integers(9, 19)))
        reads = helpers.random_amplicon_reads(rng, None, iv, (3000, 1777, 2500)[k], read_len=(40, 150), name_len=(1, 40), odd_ops=0.3, unplaced=0.02)
        if k == 1:
            reads = [reads[i] for i in rng.permutation(len(reads))]
        gaps = {int(i): int(rng.integers(1, 70)) for i in rng.integers(0, len(reads), size=20)}
        src = build_stream(reads, lead=int(rng.integers(0, 40)), gaps=gaps, trail=int(rng.integers(16, 64)))
        order = rng.permutation(len(iv))  # the BED order is not the sorted order
        c = Case(f"fuzz_{seed}_{len(reads)}_reads", src, [iv[i] for i in order], mbq=(20, 21, 10)[k], mrq=(20, 5, 21)[k], min_overlap=(50, 50, 80)[k])
        w = c.want()
        rev = (pm.headers(*c.stream).flag & 0x10) != 0
        for name, mask in (("anchor", w.decided == 1), ("index", w.decided == 2), ("under", w.under), ("clipped", (w.n_clipped > 0) & (w.assigned >= 0))):
            tally[name] += int(mask.sum())
            tally[name + "_reverse"] += int((mask & rev).sum())
        tally["clipped_columns"] += w.stats[3]
        out.append(c)
    assert tally["anchor"] >= 50 and tally["index"] >= 10 and tally["under"] >= 10 and tally["clipped_columns"] >= 100, dict(tally)
    assert all(tally[k + "_reverse"] >= 10 for k in ("anchor", "index", "under", "clipped")), dict(tally)
    return tuple(out)


@functools.lru_cache(None)
def cases():
    """the whole table: deterministic cases, the depth case, the fuzz streams"""
    return deterministic_cases() + (depth_case(),) + fuzz_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# the table on a device
# ---------------------------------------------------------------------------------------------------------------------------
def _up(a, t=np.int64):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(t) if a.dtype.itemsize == np.dtype(t).itemsize else a.astype(t)).cuda()


def upload(case, first=0, last=None):
    """(bam, rec_off, lo, hi, reach, amp_off) of the case's reads [first, last) as device tensors for Context.amplicon_count"""
    return (_up(case.buf, np.uint8), _up(case.rec_off[first:last])) + upload_amplicons(case)


def upload_amplicons(case):
    a = case.amps
    return _up(a.lo), _up(a.hi), _up(a.reach), _up(a.amp_off)


def host(ctx, *tensors):
    """device tensors as int64 numpy arrays (None stays None), behind a sync"""
    import torch

    ctx.sync()
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy().astype(np.int64) for t in tensors)


def differences(got_counts, got_reads, got_stats, want):
    """[] or what differs between the device's three outputs (int64 numpy; stats may be None) and the model's Result"""
    bad = []
    d = got_counts - want.counts
    if np.any(d):
        rows = np.flatnonzero(np.any(d != 0, 1))
        bad.append(f"{len(rows)} of {len(d)} walk entries differ, first at {rows[0]}: got - want = {d[rows[0]].tolist()}")
    if not np.array_equal(got_reads, want.amp_reads):
        at = np.argwhere(got_reads != want.amp_reads)
        bad.append(f"amp_reads differs at {len(at)} cells, first at {at[0].tolist()}: {int(got_reads[tuple(at[0])])} != {int(want.amp_reads[tuple(at[0])])}")
    if got_stats is not None and tuple(int(x) for x in got_stats) != tuple(want.stats):
        bad.append(f"stats {tuple(int(x) for x in got_stats)} != {want.stats}")
    return bad


# variant -> the deterministic cases that must catch it (tests/test_amplicon_count_model.py asserts that each of them does)
CAUGHT_BY = {
    "tie_highest_index": ("equal_overlap_equal_anchor_lowest_index",),
    "anchor_ignores_strand": ("read_inside_the_overlap_reverse", "65_amplicons_shifted_by_one_second_round_of_lanes"),
    "span_from_l_seq": ("N_makes_the_span_too_long", "soft_and_hard_clips_outside_the_span"),
    "outside_counted": ("read_one_column_into_the_neighbour",),
    "threshold_strict": ("span_100_overlap_50_and_49_at_min_overlap_50",),
    "search_on_hi": ("amplicons_nested_in_a_larger_one",),
    "reverse_not_added": ("read_inside_the_overlap_reverse", "read_one_column_into_the_neighbour"),
    "cell_off_by_one": ("read_equals_its_amplicon_A_is_1", "amplicon_of_length_1"),
    "non_acgt_counted": ("non_ACGT_bases_and_low_qualities",),
    "offtarget_to_nearest": ("span_100_overlap_50_and_49_at_min_overlap_50", "amplicon_of_length_1"),
    "total_drops_beyond_L": ("three_amplicons_over_one_position_L_2",),
}
