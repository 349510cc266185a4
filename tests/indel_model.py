"""The indel counting kernel's test model -- TEST INFRASTRUCTURE (never imported by the product).

Two restatements of the definition in the contract comment of ampli_pileup_indel_count (include/amplisolve_hip.h) over the
read dicts and record streams of tests/pileup_model.py, written differently on purpose so that they check each other:
  * count: numpy over flat arrays of the reads' EFFECTIVE operations, with look-ahead -- "what follows the last column of a match run";
  * walk:  a per-read Python loop that is the state machine of the contract, operation by operation, no look-ahead.  It also tallies
    why a junction was NOT counted (REJECTIONS), which is how the fuzz streams are shown to meet every rejection rule.
`wrong=` switches count to one deliberately wrong variant (WRONG_VARIANTS); tests/test_indel_model.py shows that each of them is caught
by a named deterministic case (CAUGHT_BY).  geometry() reads the kernel's constexpr lines; cases() is the named case table, and every
case that claims to sit on an edge of the kernel's LDS window asserts so while the table is built.
"""
from __future__ import annotations

import collections
import functools
import os
import re
import struct
import zlib

import numpy as np

from tests import pileup_model as pm
from tests.pileup_model import build_stream, make_keys, read, span_keys, write_bam_of  # noqa: F401  (write_bam_of: for the users of this module)

KERNEL_SOURCE = os.path.join(pm.ROOT, "amplisolve_amd", "csrc", "ampli_indel.hip")
TYPES_HEADER = os.path.join(pm.ROOT, "include", "amplisolve_types.h")
M_OPS, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P = (0, 7, 8), 1, 2, 3, 4, 5, 6

Geometry = collections.namedtuple("Geometry", "reads window bins")


@functools.lru_cache(None)
def geometry():
    """(reads per workgroup, panel positions of the LDS window) as ampli_indel.hip states them, and the length bins of the header"""
    text = open(KERNEL_SOURCE).read()
    vals = {}
    for name in ("READS", "WINDOW"):
        m = re.search(r"^constexpr\s+int\s+INDEL_%s\s*=\s*([0-9][0-9\s*]*);" % name, text, re.M)
        assert m, f"no `constexpr int INDEL_{name} = ...;` line in {KERNEL_SOURCE}"
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        vals[name] = v
    m = re.search(r"^#define\s+AMPLI_INDEL_LEN_BINS\s+(\d+)", open(TYPES_HEADER).read(), re.M)
    assert m, "no AMPLI_INDEL_LEN_BINS in include/amplisolve_types.h"
    return Geometry(vals["READS"], vals["WINDOW"], int(m.group(1)))


BINS = 32  # the contract's number; geometry().bins is the header's, and the two are compared in tests/test_indel_model.py

# name -> what is wrong; count(..., wrong=name) computes that variant.  One per rule of the definition.
WRONG_VARIANTS = {
    "ops_not_removed": "zero-length and P operations are not removed: they separate what the definition calls adjacent",
    "edge_indel_counted": "an insertion or deletion that opens or closes the alignment is counted",
    "I_and_D_counted": "an I directly followed by a D (or D by I) is counted as the first of the two",
    "anchor_one_column_off": "events land on p + 1 instead of p",
    "mbq_from_next_base": "the quality tested is that of the base behind the junction",
    "reverse_not_added": "reverse-strand reads do not add to slot + 4",
    "bin_without_minus_one": "the length bin is min(L, 32) instead of min(L, 32) - 1",
    "N_counted_as_reference": "the junction in front of an N is counted as a reference junction",
    "last_column_counted": "the read's last aligned column is counted as a reference junction",
}
# why the walk did not count a junction (or an indel): the rejection rules of the definition
REJECTIONS = ("last_column", "clip", "skip", "I_then_D", "D_then_I", "two_I", "indel_opens", "indel_closes")

Result = collections.namedtuple("Result", "counts lengths stats")  # int64 [P][8], int64 [P][2][BINS], (reads kept, junctions counted)


def _shift(a, k, fill):
    """a[i + k], `fill` behind the end"""
    out = np.full(len(a), fill, a.dtype)
    if k < len(a):
        out[:len(a) - k] = a[k:]
    return out


def count(src, keys, mbq, mrq, wrong=None):
    """Result of the stream `src` (read dicts or (buf, rec_off)) on the panel `keys`: the vectorised restatement"""
    assert wrong is None or wrong in WRONG_VARIANTS, wrong
    buf, rec_off = pm.as_stream(src)
    keys = np.asarray(keys, np.uint64)
    P = len(keys)
    h = pm.headers(buf, rec_off)
    keep = (h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & pm.READ_MASK) == 0) & (h.mapq >= mrq)
    rd = np.flatnonzero(keep)
    counts = np.zeros(P * 8, np.int64)
    lengths = np.zeros(P * 2 * BINS, np.int64)
    # every CIGAR operation of the kept reads, flat, with what the read's earlier operations consumed
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

    rbef, qbef = before(radv), before(qadv)
    # the effective operations
    eff = np.ones(len(op), bool) if wrong == "ops_not_removed" else (ln > 0) & (op != OP_P)
    e_read, e_op, e_len = o_read[eff], op[eff], ln[eff]
    e_ref, e_q = h.pos[e_read] + 1 + rbef[eff], qbef[eff]  # 1-based position and query index of the operation's first column
    same = lambda k: _shift(e_read, k, -1) == e_read  # noqa: E731  (operation i + k belongs to the same read)
    nxt = [np.where(same(k), _shift(e_op, k, -1), -1) for k in (1, 2, 3)]  # the next three effective operations, -1: none
    prv = np.full(len(e_op), -1, np.int64)
    if len(e_op) > 1:
        prv[1:] = np.where(e_read[1:] == e_read[:-1], e_op[:-1], -1)
    is_m = np.isin(e_op, M_OPS)
    m1, m2, m3 = (np.isin(x, M_OPS) for x in nxt)
    l1 = _shift(e_len, 1, 0)

    # (read, anchor position, query index of the anchor, slot, length) of every candidate junction
    cand = []
    # the len - 1 inner junctions of every match run
    runs = np.flatnonzero(is_m & (e_len > 1))
    n_in = e_len[runs] - 1
    r_of = np.repeat(runs, n_in)
    j = np.arange(len(r_of)) - np.repeat(np.cumsum(n_in) - n_in, n_in)
    cand.append((e_read[r_of], e_ref[r_of] + j, e_q[r_of] + j, np.zeros(len(r_of), np.int64), np.zeros(len(r_of), np.int64)))
    # the last column of every match run: what follows decides
    slot = np.full(len(e_op), -1, np.int64)
    slot[is_m & m1] = 0
    ev = is_m & np.isin(nxt[0], (OP_I, OP_D)) & m2
    slot[ev] = nxt[0][ev]
    if wrong == "I_and_D_counted":
        both = is_m & np.isin(nxt[0], (OP_I, OP_D)) & np.isin(nxt[1], (OP_I, OP_D)) & (nxt[0] != nxt[1]) & m3
        slot[both] = nxt[0][both]
    if wrong == "N_counted_as_reference":
        slot[is_m & (nxt[0] == OP_N) & m2] = 0
    if wrong == "last_column_counted":
        slot[is_m & (nxt[0] == -1)] = 0
    if wrong == "edge_indel_counted":
        closes = is_m & np.isin(nxt[0], (OP_I, OP_D)) & np.isin(nxt[1], (-1, OP_S, OP_H))
        slot[closes] = nxt[0][closes]
    last = np.flatnonzero(slot >= 0)
    p_end = e_ref[last] + e_len[last] - 1
    if wrong == "anchor_one_column_off":
        p_end = p_end + (slot[last] > 0)
    cand.append((e_read[last], p_end, e_q[last] + e_len[last] - 1, slot[last], np.where(slot[last] > 0, l1[last], 0)))
    c_read, c_pos, c_q, c_slot, c_len = (np.concatenate(x) for x in zip(*cand))
    if wrong == "mbq_from_next_base":
        c_q = np.minimum(c_q + 1, h.l_seq[c_read] - 1)
    good = buf[h.qual[c_read] + c_q].astype(np.int64) >= mbq
    if wrong == "edge_indel_counted":  # an indel that opens the alignment: anchored on the column in front of the read, no base to test
        opens = np.flatnonzero(np.isin(e_op, (OP_I, OP_D)) & np.isin(prv, (-1, OP_S, OP_H)) & m1)
        c_read, c_pos = np.concatenate([c_read, e_read[opens]]), np.concatenate([c_pos, e_ref[opens] - 1])
        c_slot, c_len = np.concatenate([c_slot, e_op[opens]]), np.concatenate([c_len, e_len[opens]])
        good = np.concatenate([good, np.ones(len(opens), bool)])
    good &= c_pos >= 1
    key = pm._key_of(h.ref_id[c_read], np.maximum(c_pos, 0))
    ki = np.searchsorted(keys, key)
    good &= keys[np.minimum(ki, P - 1)] == key
    ki, c_slot, c_len, c_read = ki[good], c_slot[good], c_len[good], c_read[good]
    counts += np.bincount(ki * 8 + c_slot, minlength=P * 8)
    if wrong != "reverse_not_added":
        rev = (h.flag[c_read] & 0x10) != 0
        counts += np.bincount(ki[rev] * 8 + 4 + c_slot[rev], minlength=P * 8)
    e = c_slot > 0
    at = (ki[e] * 2 + c_slot[e] - 1) * BINS + np.minimum(c_len[e], BINS) - (0 if wrong == "bin_without_minus_one" else 1)
    at = at[(at >= 0) & (at < len(lengths))]  # only a wrong variant leaves the table
    lengths += np.bincount(at, minlength=len(lengths))
    return Result(counts.reshape(P, 8), lengths.reshape(P, 2, BINS), (int(keep.sum()), int(len(ki))))


def walk(src, keys, mbq, mrq, tally=None):
    """Result of the same stream by the contract's state machine, one read and one operation at a time.  tally (a dict or Counter):
    += 1 per rejection (REJECTIONS), whatever the panel and the qualities, and "events_reverse" per counted event of a reverse read."""
    buf, rec_off = pm.as_stream(src)
    b = bytes(buf)
    index = {int(k): i for i, k in enumerate(np.asarray(keys, np.uint64).tolist())}
    P = len(index)
    counts = np.zeros((P, 8), np.int64)
    lengths = np.zeros((P, 2, BINS), np.int64)
    kept = junctions = 0
    tally = tally if tally is not None else collections.Counter()
    for o in np.asarray(rec_off, np.uint64).tolist():
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, o + 4)
        if ref_id < 0 or pos < 0 or flag & pm.READ_MASK or mapq < mrq:
            continue
        kept += 1
        cig = o + 36 + l_name
        qual = cig + 4 * n_cigar + (l_seq + 1) // 2
        rev = bool(flag & 0x10)

        def add(p, q, slot, length):
            nonlocal junctions
            i = index.get((ref_id << 32) | p)
            if i is None or b[qual + q] < mbq:
                return
            junctions += 1
            counts[i, slot] += 1
            if rev:
                counts[i, slot + 4] += 1
            if slot:
                lengths[i, slot - 1, min(length, BINS) - 1] += 1
                if rev:
                    tally["events_reverse"] += 1

        refpos, qpos = pos + 1, 0  # 1-based position and query index of the next column
        run = False                # the previous effective operation was a match run, ending at column run_p with query index run_q ...
        run_p = run_q = 0
        pend = None                # ... plus at most one pending indel: (slot, length)
        for c in range(n_cigar):
            v, = struct.unpack_from("<I", b, cig + 4 * c)
            o_, n = v & 15, v >> 4
            if n == 0 or o_ == OP_P:
                continue
            if o_ in M_OPS:
                if run:  # settle: the pending event at its anchor, or a reference junction between two adjacent match runs
                    add(run_p, run_q, *(pend or (0, 0)))
                for k in range(n - 1):  # its own inner junctions
                    add(refpos + k, qpos + k, 0, 0)
                refpos, qpos = refpos + n, qpos + n
                run, run_p, run_q, pend = True, refpos - 1, qpos - 1, None
                continue
            if o_ in (OP_I, OP_D) and run and pend is None:
                pend = (o_, n)
            else:  # every other case clears both states
                if o_ in (OP_I, OP_D):
                    tally[{(OP_I, OP_D): "I_then_D", (OP_D, OP_I): "D_then_I", (OP_I, OP_I): "two_I"}.get((pend[0], o_), "two_D") if run else "indel_opens"] += 1
                elif run:
                    tally["indel_closes" if pend else "clip" if o_ in (OP_S, OP_H) else "skip"] += 1
                run, pend = False, None
            if o_ in (OP_I, OP_S):
                qpos += n
            elif o_ in (OP_D, OP_N):
                refpos += n
        if run:
            tally["indel_closes" if pend else "last_column"] += 1
    return Result(counts, lengths, (kept, junctions))


def covering(src, keys, mrq):
    """int64 [P]: the kept reads whose alignment spans key p (first to last reference position, whatever lies between)"""
    buf, rec_off = pm.as_stream(src)
    keys = np.asarray(keys, np.uint64)
    h = pm.headers(buf, rec_off)
    out = np.zeros(len(keys), np.int64)
    for i in np.flatnonzero((h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & pm.READ_MASK) == 0) & (h.mapq >= mrq)):
        span = 0
        for c in range(int(h.n_cigar[i])):
            v = int(pm._le(buf, np.asarray([h.cig[i] + 4 * c]), 4)[0])
            if v & 15 in pm.REF_OPS:
                span += v >> 4
        lo, hi = (np.searchsorted(keys, np.uint64((int(h.ref_id[i]) << 32) | (int(h.pos[i]) + 1 + d))) for d in (0, span))
        out[lo:hi] += 1
    return out


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
        assert np.all(self.rec_off[1:] > self.rec_off[:-1]), name  # the contract: ascending offsets
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
            for a in self._want[:2]:
                a.setflags(write=False)
        return self._want

    def __repr__(self):
        return f"Case({self.name}: {self.n_reads} reads, {len(self.keys)} keys, mbq={self.mbq}, mrq={self.mrq})"


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _first_key_index(case):
    """index of the first key at or behind the start of the case's first placed read: where the first workgroup's window starts"""
    h = pm.headers(*case.stream)
    i = int(np.flatnonzero((h.ref_id >= 0) & (h.pos >= 0))[0])
    return int(np.searchsorted(case.keys, np.uint64((int(h.ref_id[i]) << 32) | (int(h.pos[i]) + 1))))


def roughen(rng, reads, share=0.25):
    """helpers.random_amplicon_reads never puts two indels side by side nor an indel at an end of the alignment.  This rewrites the
    CIGAR of `share` of the reads so that the streams also hold those: I then D, D then I, two I, an indel that opens the alignment and
    one that closes it.  Inserted bases get a sequence and qualities of their own, so CIGAR and l_seq still agree."""
    for r in reads:
        if rng.random() >= share:
            continue
        cig = list(r["cigar"])
        kind = int(rng.integers(5))
        idx_i = [k for k, (o, n) in enumerate(cig) if o == "I" and n > 0]
        idx_d = [k for k, (o, n) in enumerate(cig) if o == "D" and n > 0]
        m_first = next(k for k, (o, n) in enumerate(cig) if o in "M=X" and n > 0)
        m_last = max(k for k, (o, n) in enumerate(cig) if o in "M=X" and n > 0)
        extra_at = None  # (cigar index in front of which query bases are inserted, how many)
        if kind == 0 and idx_i:
            cig.insert(idx_i[0] + 1, ("D", int(rng.integers(1, 5))))
        elif kind == 1 and idx_d:
            extra_at = (idx_d[0] + 1, int(rng.integers(1, 4)))
        elif kind == 2 and idx_i:
            extra_at = (idx_i[0] + 1, int(rng.integers(1, 4)))
        elif kind == 3:
            if rng.random() < 0.5:
                extra_at = (m_first, int(rng.integers(1, 4)))
            else:
                cig.insert(m_first, ("D", int(rng.integers(1, 4))))
        elif kind == 4:
            if rng.random() < 0.5:
                extra_at = (m_last + 1, int(rng.integers(1, 4)))
            else:
                cig.insert(m_last + 1, ("D", int(rng.integers(1, 4))))
        if extra_at:
            at, n = extra_at
            q = sum(k for o, k in cig[:at] if o in "MIS=X")
            r["seq"] = r["seq"][:q] + "".join(rng.choice(list("ACGT"), size=n)) + r["seq"][q:]
            r["qual"] = list(r["qual"][:q]) + [int(x) for x in rng.choice([10, 20, 30, 40], size=n)] + list(r["qual"][q:])
            cig.insert(at, ("I", n))
        r["cigar"] = cig
        assert sum(n for o, n in cig if o in "MIS=X") == len(r["seq"]) == len(r["qual"])
    return reads


FUZZ_SEEDS = (27001, 27002, 27003)
DEPTH_READS = 20_000


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
    q40 = lambda n, **at: [at.get(f"q{i}", 40) for i in range(n)]  # noqa: E731
    one = lambda name, cigar, flag=0, keys=K, **kw: add(name, [read(0, 999, cigar, _rng(name), flag=flag, **kw)], keys)  # noqa: E731
    # ---- the two events ----
    c = one("insertion_forward_10M2I10M", "10M2I10M")
    w = c.want()
    assert w.counts[:, :3].sum(0).tolist() == [18, 1, 0] and w.counts[1009 - 990].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and w.lengths[1009 - 990, 0, 1] == 1
    c = one("deletion_reverse_10M3D10M", "10M3D10M", flag=0x10)
    w = c.want()
    assert w.counts[1009 - 990].tolist() == [0, 0, 1, 0, 0, 0, 1, 0] and w.lengths[1009 - 990, 1, 2] == 1 and w.counts[:, 4].sum() == 18
    assert w.counts[1010 - 990: 1013 - 990].sum() == 0  # the deleted positions are anchors of nothing
    # ---- what is not an event ----
    for cigar, total in (("2I10M", 9), ("3S2I10M", 9), ("10M2I", 9), ("10M2I3S", 9), ("10M2I3D10M", 18), ("10M3D2I10M", 18), ("10M5N10M", 18), ("1M", 0),
                         ("10M3D", 9), ("3D10M", 9), ("7H10M2I4H", 9)):
        c = one("no_event_" + cigar, cigar)
        w = c.want()
        assert w.counts[:, 0].sum() == total and w.counts[:, 1:].sum() == 0 and w.lengths.sum() == 0, cigar
    c = one("removed_operations_10M0D2I1P10M", "10M0D2I1P10M")
    assert c.want().counts[1009 - 990].tolist()[:3] == [0, 1, 0]
    c = one("zero_length_insertion_10M0I10M", "10M0I10M")
    assert c.want().counts[:, 0].sum() == 19 and c.want().counts[:, 1:].sum() == 0
    c = one("adjacent_match_runs_5M5=5X", "5M5=5X", flag=0x10)
    assert c.want().counts[:, 0].sum() == 14 and c.want().counts[:, 4].sum() == 14
    c = one("padding_between_match_runs_5M2P5M0N5M", "5M2P5M0N5M")
    assert c.want().counts[:, 0].sum() == 14
    # ---- qualities and filters ----
    for name, qa, qn, counted in (("anchor_quality_below_mbq", 19, 40, 0), ("anchor_quality_at_mbq", 20, 19, 1)):
        rs = [read(0, 999, "10M2I10M", _rng(name), qual=q40(22, q9=qa, q10=qn, q11=qn)), read(0, 999, "10M3D10M", _rng(name), flag=0x10, qual=q40(20, q9=qa, q10=qn))]
        c = add(name, rs, K)
        assert c.want().counts[1009 - 990].tolist() == [0, counted, counted, 0, 0, 0, counted, 0]
    rs = [read(0, 999, "10M2I10M", _rng("mq"), mapq=m, flag=0x10 * (i & 1)) for i, m in enumerate((19, 20, 0, 255))]
    c = add("mapq_below_and_at_mrq", rs, K)
    assert c.want().stats[0] == 2 and c.want().counts[1009 - 990, 1] == 2
    bits = [1 << b for b in range(12)]
    c = add("each_flag_bit_alone", [read(0, 999, "10M3D10M", _rng("fl"), flag=f) for f in [0] + bits], K)
    assert c.want().stats[0] == 1 + 12 - 4 and c.want().counts[1009 - 990, 2] == 9 and c.want().counts[1009 - 990, 6] == 1
    un = [read(-1, 999, "10M2I10M", _rng("un")), read(0, -1, "10M2I10M", _rng("un"))]
    c = add("unplaced_reads_first", un + [read(0, 999, "10M2I10M", _rng("un"))], K)
    assert c.want().stats == (1, 19)
    # ---- the panel ----
    c = one("anchor_no_key_next_position_is", "10M2I10M", keys=np.delete(K, 1009 - 990))
    assert c.want().counts[:, 1].sum() == 0 and c.want().counts[:, 0].sum() == 18
    c = one("anchor_is_the_last_key", "10M3D10M", keys=span_keys(0, 990, 1009))
    assert c.want().counts[-1].tolist()[:3] == [0, 0, 1] and c.want().counts[:, 0].sum() == 9
    c = one("gap_in_the_keys_behind_the_anchor", "10M2I10M", keys=np.delete(K, np.r_[1010 - 990:1015 - 990]))
    assert c.want().counts[1009 - 990, 1] == 1 and c.want().counts[:, 0].sum() == 18 - 5
    c = one("every_second_position", "10M2I10M3D10M", keys=K[1::2])
    assert c.want().counts[:, 1:3].sum() == 2
    c = add("two_references", [read(3, 999, "10M2I10M", _rng("tr")), read(4, 999, "10M2D10M", _rng("tr"), flag=0x10)],
            np.concatenate([span_keys(3, 1000, 1009), span_keys(4, 1005, 1030)]))
    assert c.want().counts[:, 1].sum() == 1 and c.want().counts[:, 6].sum() == 1
    top = (1 << 31) - 1
    c = add("keys_at_the_top_of_the_coordinate_range", [read(top, top - 30, "10M2I10M5D10M", _rng("top"), flag=0x10)], span_keys(top, top - 40, top))
    assert c.want().counts[:, 1:3].sum() == 2 and int(c.keys[-1]) == (top << 32) | top
    # ---- lanes: match runs around the wave's width with an indel behind them ----
    for n in (63, 64, 65, 129):
        c = add(f"match_run_of_{n}_then_indel", [read(0, 999, f"{n}M2I{n}M1D3M", _rng(f"mr{n}"), flag=0x10 * (n & 1))], span_keys(0, 990, 1000 + 2 * n + 20))
        w = c.want()
        assert w.counts[:, 0].sum() == 2 * (n - 1) + 2 and w.counts[9 + n, 1] == 1 and w.counts[9 + 2 * n, 2] == 1
    # ---- lengths ----
    for L in (1, 31, 32, 33, 1000):
        c = add(f"length_{L}", [read(0, 999, f"10M{L}I10M{L}D10M", _rng(f"len{L}")), read(0, 999, f"10M{L}D10M{L}I10M", _rng(f"len{L}"), flag=0x10)], span_keys(0, 990, 2100))
        w = c.want()
        assert w.lengths[:, 0, min(L, 32) - 1].sum() == 2 and w.lengths[:, 1, min(L, 32) - 1].sum() == 2 and w.lengths.sum() == 4
    # ---- workgroups ----
    c = add("257_reads_with_one_junction", [read(0, 999, "2M", _rng("257"), flag=0x10 * (i % 3 == 0)) for i in range(R + 1)], K)
    assert c.n_reads == R + 1 and (c.n_reads + R - 1) // R == 2 and c.want().counts[10].tolist() == [R + 1, 0, 0, 0, (R + 3) // 3, 0, 0, 0]
    rg = _rng("walk")
    walk_reads = [read(0, 999 + 3 * i, ("40M2I40M", "40M3D40M", "80M", "30M1I20M1D30M")[i % 4], rg, flag=0x10 * (i & 1)) for i in range(600)]
    wide = span_keys(0, 1000, 2999)
    c = add("walk_across_2000_positions", walk_reads, wide)
    assert c.want().counts[:, 1].sum() == 300 and c.want().counts[:, 2].sum() == 300
    add("reads_in_random_order", [walk_reads[i] for i in _rng("perm").permutation(len(walk_reads))], wide)
    add("holes_in_the_panel", walk_reads, np.delete(wide, [20, 21, 22, 50, 75, 76, 130, 200, 201, 202, 203, 383, 384, 500, 1023, 1024]))
    # ---- the LDS window: keys [base, base + W) of the workgroup's first read ----
    wk = span_keys(0, 1000, 1000 + W + 60)
    anchor = read(0, 999, "30M", rg)
    for name, start, cigar, idx in (("reference_junction_on_the_windows_last_position", W - 50, "51M", W - 1),  # inner anchors end at index W - 1
                                    ("reference_junction_just_outside_the_window", W - 49, "51M", W),
                                    ("adjacent_runs_meet_on_the_windows_last_position", W - 5, "5M5=", W - 1),   # the settled junction at index W - 1
                                    ("adjacent_runs_meet_just_outside_the_window", W - 4, "5M5=", W),
                                    ("event_on_the_windows_last_position", W - 10, "10M4I10M", W - 1),
                                    ("event_just_outside_the_window", W - 9, "10M7D10M", W)):
        c = add(name, [anchor, read(0, 999 + start, cigar, rg, flag=0x10)], wk)
        assert _first_key_index(c) == 0
        alone = count([c.reads[1]], wk, 20, 20)
        if "event" in name:
            assert np.flatnonzero(alone.counts[:, 1:3].sum(1)).tolist() == [idx]
        elif "adjacent" in name:
            assert alone.counts[idx, 0] == 1 and alone.counts[idx + 1, 0] == 1 and alone.counts[:, 0].sum() == 9
        else:
            assert np.flatnonzero(alone.counts[:, 0]).max() == idx
    c = add("second_read_starts_before_the_window", [read(0, 1009, "40M", rg), read(0, 1004, "20M2I20M", rg, flag=0x10)], wide)
    assert _first_key_index(c) == 10 and np.flatnonzero(c.want().counts[:, 4]).min() == 5
    for P in (1, W - 1, W, W + 1):
        rs = [read(0, 999 + s, "30M1D29M", rg, flag=0x10 * (i & 1)) for i, s in enumerate(range(0, P + 30, 17))]
        c = add(f"panel_of_{P}_positions", rs, span_keys(0, 1000, 1000 + P - 1))
        assert len(c.keys) == P
    c = add("all_reads_behind_the_last_key", [read(0, 5999, "10M2I10M", rg) for _ in range(5)], K)
    assert _first_key_index(c) == len(K) and c.want().stats == (5, 0)
    c = add("all_reads_before_the_first_key", [read(0, 99, "10M2I10M", rg) for _ in range(5)], K)
    assert c.want().stats == (5, 0)
    return tuple(out)


@functools.lru_cache(None)
def depth_case(n=DEPTH_READS):
    """n identical reads that all show the same deletion: one LDS counter per reference junction takes n / workgroups adds per
    workgroup, and the event's two global counters and its length bin take all n"""
    r = read(0, 999, "40M15D40M", np.random.default_rng(5), flag=0x10, name="d")
    c = Case(f"depth_{n}_identical_deletions", [r] * n, span_keys(0, 990, 1120))
    w = c.want()
    assert w.counts[1039 - 990].tolist() == [0, 0, n, 0, 0, 0, n, 0] and w.lengths[1039 - 990, 1, 14] == n and w.stats == (n, 79 * n)
    return c


@functools.lru_cache(None)
def fuzz_cases():
    """three seeded streams of <= 3000 reads of helpers.random_amplicon_reads(odd_ops=0.3), roughened; together they must hold enough of
    everything (asserted here, on the CPU, while the table is built)"""
    from tests import helpers

    out = []
    tally = collections.Counter()
    ins = dele = 0
    for k, seed in enumerate(FUZZ_SEEDS):
        rng = np.random.default_rng(seed)
        n_amp = int(rng.integers(10, 24))
        amps, pairs = [], []
        for a in range(n_amp):
            ref_id = a * 3 // n_amp
            start = 500 + 170 * a + int(rng.integers(0, 40))
            amps.append((ref_id, start, start + 130))
            pairs += [(ref_id, p) for p in range(start - 10, start + 190)]
        keys = make_keys(pairs)
        if k == 1:
            keys = keys[rng.random(len(keys)) < 0.6]
        elif k == 2:
            keys = np.delete(keys, rng.integers(0, len(keys), size=len(keys) // 25))
        n = (3000, 1777, 2500)[k]
        reads = roughen(rng, helpers.random_amplicon_reads(rng, None, amps, n, read_len=(40, 150), name_len=(1, 40), odd_ops=0.3, unplaced=0.02))
        if k == 1:
            reads = [reads[i] for i in rng.permutation(len(reads))]
        gaps = {int(i): int(rng.integers(1, 70)) for i in rng.integers(0, len(reads), size=20)}
        src = build_stream(reads, lead=int(rng.integers(0, 40)), gaps=gaps, trail=int(rng.integers(16, 64)))
        c = Case(f"fuzz_{seed}_{len(reads)}_reads", src, keys, mbq=(20, 21, 10)[k], mrq=(20, 5, 21)[k], reads=reads)
        got = walk(c.stream, c.keys, c.mbq, c.mrq, tally)
        ins += int(got.counts[:, 1].sum())
        dele += int(got.counts[:, 2].sum())
        out.append(c)
    assert ins >= 50 and dele >= 50, (ins, dele)
    assert all(tally[r] >= 10 for r in REJECTIONS), {r: tally[r] for r in REJECTIONS}
    assert tally["events_reverse"] >= 10, tally["events_reverse"]
    return tuple(out)


@functools.lru_cache(None)
def cases():
    """the whole table: deterministic cases, the depth case, the fuzz streams"""
    return deterministic_cases() + (depth_case(),) + fuzz_cases()


# ---------------------------------------------------------------------------------------------------------------------------
# the table on a device
# ---------------------------------------------------------------------------------------------------------------------------
def upload(case, first=0, last=None):
    """(bam, rec_off, keys) of the case's reads [first, last) as device tensors for Context.indel_count"""
    import torch

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
    return up(case.buf, np.uint8), up(case.rec_off[first:last], np.int64), up(case.keys, np.int64)


def device_result(ctx, counts, lengths, stats):
    """the three outputs of Context.indel_count as a Result of int64 numpy arrays (None where an output was not asked for)"""
    import torch

    ctx.sync()
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy().astype(np.int64)  # noqa: E731
    return Result(host(counts), host(lengths), None if stats is None else tuple(int(x) for x in stats.cpu().tolist()))


def differences(got, want, lengths=True, stats=True):
    """[] or what differs between a device Result and the model's"""
    bad = []
    d = got.counts - want.counts
    if np.any(d):
        rows = np.flatnonzero(np.any(d != 0, 1))
        bad.append(f"{len(rows)} of {len(d)} positions differ, first at key index {rows[0]}: got - want = {d[rows[0]].tolist()}")
    if lengths and not np.array_equal(got.lengths, want.lengths):
        at = np.argwhere(got.lengths != want.lengths)
        bad.append(f"{len(at)} length bins differ, first at (key index, kind, bin) {at[0].tolist()}: {int(got.lengths[tuple(at[0])])} != {int(want.lengths[tuple(at[0])])}")
    if stats and tuple(got.stats) != tuple(want.stats):
        bad.append(f"stats {got.stats} != {want.stats}")
    return bad


# variant -> the deterministic cases that must catch it (tests/test_indel_model.py asserts that each of them does)
CAUGHT_BY = {
    "ops_not_removed": ("removed_operations_10M0D2I1P10M", "zero_length_insertion_10M0I10M", "padding_between_match_runs_5M2P5M0N5M"),
    "edge_indel_counted": ("no_event_2I10M", "no_event_3S2I10M", "no_event_10M2I", "no_event_10M2I3S", "no_event_10M3D", "no_event_3D10M", "no_event_7H10M2I4H"),
    "I_and_D_counted": ("no_event_10M2I3D10M", "no_event_10M3D2I10M"),
    "anchor_one_column_off": ("insertion_forward_10M2I10M", "deletion_reverse_10M3D10M", "anchor_is_the_last_key"),
    "mbq_from_next_base": ("anchor_quality_below_mbq", "anchor_quality_at_mbq"),
    "reverse_not_added": ("deletion_reverse_10M3D10M", "adjacent_match_runs_5M5=5X"),
    "bin_without_minus_one": ("length_1", "length_31", "length_32", "length_33", "length_1000"),
    "N_counted_as_reference": ("no_event_10M5N10M",),
    "last_column_counted": ("no_event_1M", "insertion_forward_10M2I10M"),
}
