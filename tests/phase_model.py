"""The read-phasing kernels' test model -- TEST INFRASTRUCTURE (never imported by the product).

Restatements of the definitions in the contract comments of ampli_pileup_phase and ampli_phase_score (include/amplisolve_hip.h)
over the read dicts and record streams of tests/pileup_model.py, written differently on purpose so that they check each other:
  * count: numpy over the flat (read, covered key) entries of all kept reads -- a read's range of keys from two searches, the states of
           its counted columns looked up among the keys, the pairs as shifted views of the flat arrays;
  * walk:  a per-read Python loop in plain integers, one operation at a time, the keys merged into the walk and the shift register
           written out as a list of the latest states;
  * score: the pair's integers in Python integers, the score from tests/paired_model.py's restatement of the exact test;
  * files: what computePhasing writes.
`wrong=` switches count or score to one deliberately wrong variant (WRONG_VARIANTS); tests/test_phase_model.py shows that each of them is
caught by a named deterministic case (CAUGHT_BY).  geometry() reads the kernel's constexpr lines; cases() is the named case table, and
every case that claims to sit on an edge asserts so while the table is built.
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
from tests.pileup_model import build_stream, make_keys, read, span_keys  # noqa: F401

KERNEL_SOURCE = os.path.join(pm.ROOT, "amplisolve_amd", "csrc", "ampli_phase.hip")
TYPES_HEADER = os.path.join(pm.ROOT, "include", "amplisolve_types.h")
M_OPS, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P = (0, 7, 8), 1, 2, 3, 4, 5, 6
K, STATES, OTHER = 8, 5, 4  # the contract's numbers; geometry() holds the header's, compared in tests/test_phase_model.py
PAIR = STATES * STATES

Geometry = collections.namedtuple("Geometry", "reads window partners states other")


@functools.lru_cache(None)
def geometry():
    """(reads per workgroup, listed keys of the LDS window) as ampli_phase.hip states them, and the constants of the header"""
    text = open(KERNEL_SOURCE).read()
    vals = []
    for name in ("READS", "WINDOW"):
        m = re.search(r"^constexpr\s+int\s+PHASE_%s\s*=\s*(\d+);" % name, text, re.M)
        assert m, f"no `constexpr int PHASE_{name} = ...;` line in {KERNEL_SOURCE}"
        vals.append(int(m.group(1)))
    types = open(TYPES_HEADER).read()
    for name in ("PARTNERS", "STATES", "OTHER"):
        m = re.search(r"^#define\s+AMPLI_PHASE_%s\s+(\d+)" % name, types, re.M)
        assert m, f"no AMPLI_PHASE_{name} in include/amplisolve_types.h"
        vals.append(int(m.group(1)))
    return Geometry(*vals)


# name -> what is wrong; count(..., wrong=name) or score(..., wrong=name) computes that variant.  One per rule of the definition.
COUNT_VARIANTS = {
    "D_not_covered": "a key inside a D is not covered",
    "N_not_covered": "a key inside an N is not covered",
    "low_bq_dropped": "a base below mbq is dropped instead of counted as OTHER",
    "partner_K_plus_1_counted": "the partner K + 1 is counted",
    "partner_K_dropped": "the partner K is dropped",
    "one_past_end_covered": "the key one past the read's last column is covered",
    "first_column_not_covered": "the read's first column is not covered",
    "soft_clips_shift_columns": "soft clips advance the reference position",
    "I_advances_reference": "an I advances the reference position",
    "mrq_off_by_one": "MAPQ > mrq instead of >=",
    "mbq_off_by_one": "quality > mbq instead of >=",
    "table_transposed": "the table is [s_j][s_i]",
}
SCORE_VARIANTS = {
    "presence_without_share": "a group is present from min_alt reads, whatever its share",
    "share_strict": "the share rule with > instead of >=",
    "class_bits_swapped": "class bits 1 and 2 are swapped",
}
WRONG_VARIANTS = {**COUNT_VARIANTS, **SCORE_VARIANTS}

Result = collections.namedtuple("Result", "table stats")  # int64 [P][K][5][5], (reads kept, reads covering two keys, cells incremented)
Score = collections.namedtuple("Score", "ints score cls exact")  # int64 [Q][6], float32 [Q], int64 [Q], the unrounded scores [Q]
Detail = collections.namedtuple("Detail", "read key state lo hi kept")  # flat covered (read, key index, state); per kept read its key range


def count(src, keys, mbq, mrq, wrong=None, detail=False):
    """Result of the stream `src` (read dicts or (buf, rec_off)) on the list `keys`: the vectorised restatement.  detail=True adds a Detail."""
    assert wrong is None or wrong in COUNT_VARIANTS, wrong
    buf, rec_off = pm.as_stream(src)
    keys = np.asarray(keys, np.uint64)
    P, n = len(keys), len(rec_off)
    h = pm.headers(buf, rec_off)
    keep = (h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & pm.READ_MASK) == 0) & ((h.mapq > mrq) if wrong == "mrq_off_by_one" else (h.mapq >= mrq))
    rd = np.flatnonzero(keep)
    inv = np.full(n, -1, np.int64)
    inv[rd] = np.arange(len(rd))
    nc = h.n_cigar[rd]
    o_read = np.repeat(rd, nc)
    first = np.cumsum(nc) - nc
    o_idx = np.arange(len(o_read)) - np.repeat(first, nc)
    v = pm._le(buf, h.cig[o_read] + 4 * o_idx, 4)
    op, ln = v & 15, v >> 4
    ref_ops = pm.REF_OPS + ((OP_S,) if wrong == "soft_clips_shift_columns" else ()) + ((OP_I,) if wrong == "I_advances_reference" else ())

    def before(ops):  # what the read's earlier operations of these kinds are long, together
        adv = np.where(np.isin(op, ops), ln, 0)
        c = np.cumsum(adv) - adv
        return c - np.repeat(c[first[nc > 0]], nc[nc > 0]) if len(c) else c

    rbef, qbef = before(ref_ops), before(pm.QUERY_OPS)
    L = np.bincount(o_read, weights=np.where(np.isin(op, ref_ops), ln, 0), minlength=n).astype(np.int64)[rd]
    # the keys a kept read covers: [lo, hi)
    ref_k, pos_k = h.ref_id[rd], h.pos[rd]
    lo = np.searchsorted(keys, pm._key_of(ref_k, pos_k + (2 if wrong == "first_column_not_covered" else 1)))
    hi = np.searchsorted(keys, pm._key_of(ref_k, pos_k + L + (1 if wrong == "one_past_end_covered" else 0)), side="right")
    hi = np.where(L > 0, np.maximum(hi, lo), lo)
    ncov = hi - lo
    start = np.cumsum(ncov) - ncov
    f_kept = np.repeat(np.arange(len(rd)), ncov)
    f_off = np.arange(len(f_kept)) - np.repeat(start, ncov)
    f_ki = lo[f_kept] + f_off
    st = np.full(len(f_kept), OTHER, np.int64)
    cov = np.ones(len(f_kept), bool)
    # the match columns that fall on a listed key
    runs = np.flatnonzero(np.isin(op, M_OPS) & (ln > 0))
    col_run = np.repeat(runs, ln[runs])
    j = np.arange(len(col_run)) - np.repeat(np.cumsum(ln[runs]) - ln[runs], ln[runs])
    rd_of = o_read[col_run]
    key = pm._key_of(h.ref_id[rd_of], h.pos[rd_of] + 1 + rbef[col_run] + j)
    ki = np.searchsorted(keys, key)
    kr = inv[rd_of]
    sel = np.flatnonzero((keys[np.minimum(ki, P - 1)] == key) & (ki >= lo[kr]) & (ki < hi[kr]))
    rd_of, ki, kr, q = rd_of[sel], ki[sel], kr[sel], (qbef[col_run] + j)[sel]
    inside = q < h.l_seq[rd_of]  # (only a wrong variant walks off the sequence)
    rd_of, ki, kr, q = rd_of[inside], ki[inside], kr[inside], q[inside]
    byte = buf[h.seq[rd_of] + (q >> 1)].astype(np.int64)
    b4 = pm._B4[np.where((q & 1) == 0, byte >> 4, byte & 15)]
    qual = buf[h.qual[rd_of] + q].astype(np.int64)
    q_ok = (qual > mbq) if wrong == "mbq_off_by_one" else (qual >= mbq)
    at = start[kr] + (ki - lo[kr])
    good = (b4 >= 0) & q_ok
    st[at[good]] = b4[good]
    if wrong == "low_bq_dropped":
        cov[at[~q_ok]] = False
    if wrong in ("D_not_covered", "N_not_covered"):
        for g in np.flatnonzero((op == (OP_D if wrong == "D_not_covered" else OP_N)) & (ln > 0)).tolist():
            r = o_read[g]
            p0 = h.pos[r] + 1 + rbef[g]
            a = np.searchsorted(keys, pm._key_of(h.ref_id[r:r + 1], np.asarray([p0]))[0])
            b = np.searchsorted(keys, pm._key_of(h.ref_id[r:r + 1], np.asarray([p0 + ln[g] - 1]))[0], side="right")
            x = inv[r]
            for kk in range(max(a, lo[x]), min(b, hi[x])):
                cov[start[x] + kk - lo[x]] = False
    # the pairs: entry a with the entry 1 + k behind it in the same read
    table = np.zeros(P * K * PAIR, np.int64)
    cells = 0
    partners = K + 1 if wrong == "partner_K_plus_1_counted" else K - 1 if wrong == "partner_K_dropped" else K
    for k in range(partners):
        a = np.flatnonzero(f_off + 1 + k < ncov[f_kept])
        b = a + 1 + k
        ok = cov[a] & cov[b]
        a, b = a[ok], b[ok]
        sa, sb = (st[b], st[a]) if wrong == "table_transposed" else (st[a], st[b])
        idx = ((f_ki[a] * K + k) * STATES + sa) * STATES + sb
        idx = idx[idx < len(table)]
        table += np.bincount(idx, minlength=len(table))
        cells += len(idx)
    two = int((np.bincount(f_kept[cov], minlength=len(rd)) >= 2).sum())
    res = Result(table.reshape(P, K, STATES, STATES), (int(keep.sum()), two, int(cells)))
    return res + (Detail(rd[f_kept], f_ki, st, lo, hi, rd),) if detail else res


def walk(src, keys, mbq, mrq):
    """Result of the same stream one read and one operation at a time, in plain integers: the sorted keys are merged into the walk, the
    states of the latest covered keys are a list, newest first"""
    buf, rec_off = pm.as_stream(src)
    b = bytes(buf)
    ks = [int(k) for k in np.asarray(keys, np.uint64).tolist()]
    P = len(ks)
    table = np.zeros((P, K, STATES, STATES), np.int64)
    kept = two = cells = 0
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
        latest, covered = [], 0
        for c in range(n_cigar):
            v, = struct.unpack_from("<I", b, cig + 4 * c)
            o_, n = v & 15, v >> 4
            if n == 0 or o_ == OP_P:
                continue
            if o_ in M_OPS or o_ in (OP_D, OP_N):
                while k < P and ks[k] >> 32 == ref_id and (ks[k] & 0xffffffff) < refpos + n:
                    s = OTHER
                    if o_ in M_OPS:
                        at = i + (ks[k] & 0xffffffff) - refpos
                        nib = (b[seq + at // 2] >> (0 if at & 1 else 4)) & 15
                        if nib in (1, 2, 4, 8) and b[qual + at] >= mbq:
                            s = (1, 2, 4, 8).index(nib)
                    for t, sp in enumerate(latest, 1):  # key k - t showed sp
                        table[k - t, t - 1, sp, s] += 1
                        cells += 1
                    latest = ([s] + latest)[:K]
                    covered += 1
                    k += 1
                refpos += n
                if o_ in M_OPS:
                    i += n
            elif o_ in (OP_I, OP_S):
                i += n
        two += covered >= 2
    return Result(table, (kept, two, cells))


# ---------------------------------------------------------------------------------------------------------------------------
# the score
# ---------------------------------------------------------------------------------------------------------------------------
def pair_cell(i, j):
    """the cell of key i with key j, i < j <= i + K"""
    assert 0 < j - i <= K
    return i * K + (j - i - 1)


def tested(cell, P, nt):
    if not 0 <= cell < P * K or cell // K + 1 + cell % K >= P:
        return False
    return all(0 <= int(x) <= 3 for x in nt) and nt[0] != nt[1] and nt[2] != nt[3]


def present(x, m, min_alt, min_share, wrong=None):
    if x < min_alt:
        return False
    if wrong == "presence_without_share":
        return True
    return 100 * x > min_share * m if wrong == "share_strict" else 100 * x >= min_share * m


def score(table, pair_cells, pair_nt, min_alt=4, min_share=10, wrong=None):
    """Score of the pairs over `table` [P][K][5][5] in Python integers; the exact test from tests/paired_model.py"""
    from tests import paired_model as pdm

    assert wrong is None or wrong in SCORE_VARIANTS, wrong
    table = np.asarray(table).reshape(-1, K, STATES, STATES)
    P = len(table)
    flat = table.reshape(-1, STATES, STATES)
    ints, scores, classes, exact = [], [], [], []
    for cell, nt in zip([int(c) for c in pair_cells], np.asarray(pair_nt, np.int64).reshape(-1, 4).tolist()):
        if not tested(cell, P, nt):
            ints.append([-1] * 6)
            scores.append(0.0)
            classes.append(-1)
            exact.append(0.0)
            continue
        c = [[int(x) for x in row] for row in flat[cell]]
        ri, ai, rj, aj = nt
        rr, ra, ar, aa = c[ri][rj], c[ri][aj], c[ai][rj], c[ai][aj]
        joint = sum(sum(row) for row in c)
        ints.append([rr, ra, ar, aa, joint, joint - (rr + ra + ar + aa)])
        scores.append(pdm.pair_s(aa, aa + ar, ra, ra + rr))
        exact.append(float(pdm.pair_s_exact(aa, aa + ar, ra, ra + rr)))
        m = aa + ar + ra
        bits = [present(x, m, min_alt, min_share, wrong) for x in (aa, ar, ra)]
        if wrong == "class_bits_swapped":
            bits = [bits[0], bits[2], bits[1]]
        classes.append(bits[0] | bits[1] << 1 | bits[2] << 2)
    return Score(np.asarray(ints, np.int64).reshape(-1, 6), np.asarray(scores, np.float32), np.asarray(classes, np.int64), np.asarray(exact, np.float64))


def host_score(table, cells, nts, min_alt=4, min_share=10):
    """the same pairs through ampli_host_phase_score, the host library's twin of the kernel (no GPU); exact = None"""
    import ctypes as C

    from amplisolve_amd import host_lib

    table = np.ascontiguousarray(np.asarray(table).reshape(-1, K, STATES, STATES), np.int32)
    cells, nts = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(nts, np.int8).reshape(-1, 4)
    Q = len(cells)
    ints, sc, cls = np.full((Q, 6), 7, np.int64), np.full(Q, 7.0, np.float32), np.full(Q, 7, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert host_lib().ampli_host_phase_score(ptr(table), len(table), ptr(cells), ptr(nts), Q, min_alt, min_share, ptr(ints), ptr(sc), ptr(cls)) == 0
    return Score(ints, sc, cls, None)


def invariant_failures(case, table):
    """what the invariant finds wrong in `table` on the cells of `case` whose precondition holds"""
    counts = pm.count(case.stream, case.keys, case.mbq, case.mrq)[0]
    bad = []
    for i, k in case.invariant_cells():
        j = i + 1 + k
        if table[i, k, :4].sum(1).tolist() != counts[i, :4].tolist():
            bad.append((i, k, "rows", table[i, k, :4].sum(1).tolist(), counts[i, :4].tolist()))
        if table[i, k, :, :4].sum(0).tolist() != counts[j, :4].tolist():
            bad.append((i, k, "columns", table[i, k, :, :4].sum(0).tolist(), counts[j, :4].tolist()))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the command's two files
# ---------------------------------------------------------------------------------------------------------------------------
def nt_code(allele):
    return "ACGT".index(allele.upper()) if len(allele) == 1 and allele.upper() in "ACGT" else -2


def verdict(cls, s, q_min):
    if cls in (1, 3, 5):
        return {1: "CIS", 3: "NESTED_B", 5: "NESTED_A"}[cls] if float(s) >= q_min else "UNRESOLVED"
    return {6: "TRANS", 7: "MIXED"}.get(cls, "UNTESTED")


def pairs_of(lines, key_index, max_dist):
    """[(a, b)]: the indices of every two listed lines with a key on one chromosome, 0 < pos_b - pos_a <= max_dist, by (key a, key b, a, b)"""
    out = []
    for a, la in enumerate(lines):
        for b_, lb in enumerate(lines):
            if key_index[a] >= 0 and key_index[b_] >= 0 and la[0] == lb[0] and 0 < lb[1] - la[1] <= max_dist:
                out.append((key_index[a], key_index[b_], a, b_))
    return [(a, b_) for _, _, a, b_ in sorted(out)]


def files(lines, key_index, table, min_alt=4, min_share=10, q_min=13.0, max_dist=200, scorer=score, rows=False):
    """(PHASE.txt, PHASE.MNV.txt) as text for the listed lines [(chrom, pos, ref, alt)], their key indices (-1: unknown chromosome) and the
    table [P][K][5][5]; rows=True: also [(a, b, verdict, exact score or None)]"""
    pairs = pairs_of(lines, key_index, max_dist)
    formed = [(a, b) for a, b in pairs if key_index[b] - key_index[a] <= K]
    s = scorer(table, [pair_cell(key_index[a], key_index[b]) for a, b in formed], [[nt_code(lines[a][2]), nt_code(lines[a][3]), nt_code(lines[b][2]), nt_code(lines[b][3])]
                                                                                  for a, b in formed], min_alt, min_share)
    slot = {p: i for i, p in enumerate(formed)}
    text, seen, out_rows = [], {}, []
    for a, b in pairs:
        la, lb = lines[a], lines[b]
        head = [la[0], str(la[1]), la[2], la[3], str(lb[1]), lb[2], lb[3]]
        i = slot.get((a, b))
        if i is None or s.cls[i] < 0:
            v = "NOT_FORMED" if i is None else "UNTESTED"
            text.append("\t".join(head + ["."] * 8 + [v]) + "\n")
            seen[a, b] = (v, 0)
            out_rows.append((a, b, v, None))
            continue
        rr, ra, ar, aa, joint, other = (int(x) for x in s.ints[i])
        four = rr + ra + ar + aa
        exp = "%.2f" % (float(aa + ar) * float(aa + ra) / float(four)) if four else "."
        v = verdict(int(s.cls[i]), s.score[i], q_min)
        text.append("\t".join(head + [str(x) for x in (joint, rr, ra, ar, aa, other)] + [exp, "%.4f" % float(s.score[i]), v]) + "\n")
        seen[a, b] = (v, aa)
        out_rows.append((a, b, v, float(s.exact[i]) if s.exact is not None else None))
    # chains, greedily in (key, list) order
    order = sorted((x for x in range(len(lines)) if key_index[x] >= 0), key=lambda x: (key_index[x], x))
    used, mnv = set(), []
    for a in order:
        if a in used:
            continue
        chain = [a]
        while len(chain) < 3:
            nxt = [x for x in order if x not in used and x not in chain and lines[x][0] == lines[chain[-1]][0] and lines[x][1] == lines[chain[-1]][1] + 1
                   and all(seen.get((m, x), ("", 0))[0] == "CIS" for m in chain)]
            if not nxt:
                break
            chain.append(nxt[0])
        if len(chain) >= 2:
            used.update(chain)
            reads = min(seen[chain[x], chain[y]][1] for x in range(len(chain)) for y in range(x + 1, len(chain)))
            mnv.append(f"{lines[a][0]}\t{lines[a][1]}\t{''.join(lines[x][2] for x in chain)}\t{''.join(lines[x][3] for x in chain)}\t{reads}\n")
    res = ("".join(text), "".join(mnv))
    return res + (out_rows,) if rows else res


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
            self._want.table.setflags(write=False)
        return self._want

    def window_bases(self):
        assert geometry().reads == pm.geometry().reads  # pm.window_bases groups the reads as this kernel does
        return pm.window_bases(self.stream, self.keys)

    def outside_window(self):
        """the distinct (workgroup, key i) of incremented cells whose key i lies outside the workgroup's LDS window"""
        geo = geometry()
        d = self.want(detail=True)[2]
        if not len(d.read):
            return 0
        kept_of = np.searchsorted(d.kept, d.read)
        has_partner = d.key + 1 < d.hi[kept_of]  # key i of at least one cell of this read
        g = d.read // geo.reads
        rel = d.key - self.window_bases()[g]
        out = has_partner & ((rel < 0) | (rel >= geo.window))
        return len(set(zip(g[out].tolist(), d.key[out].tolist())))

    def invariant_cells(self):
        """[(i, k)]: the cells whose two keys are covered by the same kept reads, at least one (the precondition of the invariant)"""
        d = self.want(detail=True)[2]
        P = len(self.keys)
        cover = np.zeros((len(d.kept), P), bool) if len(d.kept) * P <= 1 << 24 else None
        assert cover is not None, "too large for the dense coverage matrix"
        for x, (a, b) in enumerate(zip(d.lo.tolist(), d.hi.tolist())):
            cover[x, a:b] = True
        out = []
        for i in range(P):
            for k in range(min(K, P - 1 - i)):
                if cover[:, i].any() and np.array_equal(cover[:, i], cover[:, i + 1 + k]):
                    out.append((i, k))
        return out

    def __repr__(self):
        return f"Case({self.name}: {self.n_reads} reads, {len(self.keys)} keys, mbq={self.mbq}, mrq={self.mrq})"


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _seq(n, fill="A", **at):
    """n bases `fill` with the base of every at[iN] = base at index N"""
    s = [fill] * n
    for k, base in at.items():
        s[int(k[1:])] = base
    return "".join(s)


@functools.lru_cache(None)
def deterministic_cases():
    geo = geometry()
    R, W = geo.reads, geo.window
    out = []

    def add(name, src, keys, mbq=20, mrq=20, reads=None):
        c = Case(name, src, keys, mbq, mrq, reads)
        out.append(c)
        return c

    two = make_keys([(0, 1005), (0, 1010)])
    q30 = lambda n: [30] * n  # noqa: E731
    nz = lambda t: {tuple(int(x) for x in at): int(t[tuple(at)]) for at in np.argwhere(t)}  # noqa: E731  {(i, k, s_i, s_j): count}
    # ---- the states ----
    rs = []
    for si in range(STATES):
        for sj in range(STATES):
            qual = q30(20)
            if sj == OTHER:
                qual[10] = 10  # OTHER at key j: a base below mbq; at key i: a base that is none of A C G T
            rs.append(read(0, 999, "20M", _rng("st"), seq=_seq(20, i5="ACGTN"[si], i10="ACGTA"[sj]), qual=qual))
    c = add("two_keys_one_read_of_each_of_the_25_state_pairs", rs, two)
    assert np.array_equal(c.want().table[0, 0], np.ones((STATES, STATES), np.int64)) and c.want().table.sum() == 25 and c.want().stats == (25, 25, 25)
    # ---- the partners ----
    c = add("nine_keys_inside_one_read", [read(0, 999, "30M", _rng("9k"))], make_keys([(0, 1000 + 3 * i) for i in range(K + 1)]))
    assert c.want().table[0, K - 1].sum() == 1 and c.want().stats == (1, 1, (K + 1) * K // 2) and c.want().table[:, :, OTHER].sum() == 0
    c = add("ten_keys_inside_one_read", [read(0, 999, "30M", _rng("10k"))], make_keys([(0, 1000 + 3 * i) for i in range(K + 2)]))
    assert c.want().table[0].sum() == K and c.want().table[1, K - 1].sum() == 1 and c.want().table[1, 0].sum() == 1 and c.want().stats == (1, 1, (K + 1) * K // 2 + K)
    # ---- the ends of a read ----
    c = add("a_read_that_ends_on_a_key_and_one_that_ends_a_base_before_it", [read(0, 999, "21M", _rng("e1")), read(0, 999, "20M", _rng("e2"))], make_keys([(0, 1005), (0, 1020)]))
    assert c.want().table.sum() == 1 and c.want().stats == (2, 1, 1)
    c = add("a_read_that_starts_on_a_key_and_one_that_starts_a_base_behind_it", [read(0, 999, "20M", _rng("s1")), read(0, 1000, "20M", _rng("s2"))], make_keys([(0, 1000), (0, 1010)]))
    assert c.want().table.sum() == 1 and c.want().stats == (2, 1, 1)
    # ---- D and N: covered, in state OTHER ----
    gap_keys = make_keys([(0, p) for p in (1005, 1010, 1012, 1014, 1015, 1020)])
    for name, cigar in (("D", "10M5D10M"), ("N", "10M5N10M")):
        c = add(f"keys_in_the_middle_and_at_both_ends_of_a_{name}_{cigar}", [read(0, 999, cigar, _rng(name), seq="C" * 20, qual=q30(20))], gap_keys)
        d = c.want(detail=True)[2]
        assert d.state.tolist() == [1, OTHER, OTHER, OTHER, 1, 1] and c.want().stats == (1, 1, 15)
        assert c.want().table[0, 0, 1, OTHER] == 1 and c.want().table[1, 0, OTHER, OTHER] == 1 and c.want().table[3, 0, OTHER, 1] == 1 and c.want().table[0, 3, 1, 1] == 1
    # ---- clips and insertions ----
    c = add("leading_5S", [read(0, 999, "5S20M", _rng("5s"), seq="T" * 5 + _seq(20, i5="C"), qual=q30(25))], two)
    assert nz(c.want().table) == {(0, 0, 1, 0): 1}
    c = add("leading_5H", [read(0, 999, "5H20M", _rng("5h"), seq=_seq(20, i5="C"), qual=q30(20))], two)
    assert nz(c.want().table) == {(0, 0, 1, 0): 1}
    c = add("an_I_between_the_two_keys", [read(0, 999, "8M2I12M", _rng("ins"), seq=_seq(22, i5="C", i12="G"), qual=q30(22))], two)
    assert nz(c.want().table) == {(0, 0, 1, 2): 1}
    # ---- references and gaps in the list ----
    c = add("keys_on_two_references", [read(3, 999, "20M", _rng("r3")), read(4, 999, "20M", _rng("r4"))], make_keys([(3, 1005), (3, 1010), (4, 1005), (4, 1010)]))
    assert c.want().table[[0, 2], 0].sum() == 2 and c.want().table.sum() == 2  # no cell between the last key of one reference and the first of the next
    c = add("a_gap_in_the_keys_wider_than_a_read", [read(0, 999, "20M", _rng("g1")), read(0, 4999, "20M", _rng("g2"))], make_keys([(0, 1005), (0, 1010), (0, 5005), (0, 5010)]))
    assert c.want().table[[0, 2], 0].sum() == 2 and c.want().table.sum() == 2
    # ---- the filter and the thresholds ----
    c = add("a_filtered_an_unplaced_and_reads_at_mrq_and_below", [read(0, 999, "20M", _rng("f"), flag=0x400), read(-1, 999, "20M", _rng("f")), read(0, -1, "20M", _rng("f")),
                                                                   read(0, 999, "20M", _rng("f"), mapq=20), read(0, 999, "20M", _rng("f"), mapq=19)], two)
    assert c.want().stats == (1, 1, 1)
    lowq = q30(20)
    lowq[5] = 19
    atq = q30(20)
    atq[5] = 20
    c = add("quality_below_and_at_mbq", [read(0, 999, "20M", _rng("q"), seq=_seq(20, i5="G"), qual=lowq), read(0, 999, "20M", _rng("q"), seq=_seq(20, i5="G"), qual=atq)], two)
    assert nz(c.want().table) == {(0, 0, OTHER, 0): 1, (0, 0, 2, 0): 1}
    # ---- the LDS window: the W keys from the first key not below the start of the workgroup's first placed read; a cell belongs to key i ----
    wk = make_keys([(0, 1000 + 3 * i) for i in range(W + 10)])
    c = add("the_windows_last_key_with_the_first_beyond_and_pairs_wholly_beyond", [read(0, 999, f"{3 * (W + 10)}M", _rng("win"))], wk)
    assert c.window_bases()[0] == 0 and c.want().table[W - 1, 0].sum() == 1 and c.want().table[W:].sum() == sum(min(K, 9 - i) for i in range(10)) and c.outside_window() == 9
    c = add("a_read_that_starts_in_front_of_the_windows_first_key", [read(0, 1009, "40M", _rng("w1")), read(0, 999, "40M", _rng("w2"), flag=0x10)],
            make_keys([(0, 1005), (0, 1012), (0, 1030)]))
    assert c.window_bases()[0] == 1 and c.outside_window() == 1 and c.want().table[0].sum() == 2 and c.want().table[1, 0].sum() == 2
    rg = _rng("walk")
    walk_reads = [read(0, 999 + 3 * i, ("40M2I40M", "40M3D40M", "80M", "5S30M1I20M1D30M")[i % 4], rg, flag=0x10 * (i & 1)) for i in range(300)]
    dense = span_keys(0, 1000, 1999)
    c = add("a_stream_in_descending_position_order_dense", walk_reads[::-1], dense)
    assert c.outside_window() >= 10
    add("a_stream_in_ascending_position_order_sparse", walk_reads, dense[::7])
    # ---- workgroups ----
    for n in (R, R + 1):
        rs = [read(0, 999 + (i % 3), "30M", _rng(f"wg{i}"), flag=0x10 * (i & 1)) for i in range(n)]
        c = add(f"{n}_reads", rs, make_keys([(0, 1010), (0, 1020)]))
        assert c.n_reads == n and c.want().stats == (n, n, n)
    return tuple(out)


DEPTH_READS = 20_000


@functools.lru_cache(None)
def depth_case(n=DEPTH_READS):
    """n identical reads over two listed keys: every increment lands in one cell"""
    r = read(0, 999, "80M", np.random.default_rng(5), flag=0x10, name="d", qual=[37] * 80, seq="ACGT" * 20)
    c = Case(f"depth_{n}_identical_reads_one_cell", [r] * n, make_keys([(0, 1030), (0, 1041)]))
    w = c.want()
    assert w.stats == (n, n, n) and w.table[0, 0, 2, 1] == n and w.table.sum() == n  # indices 30 and 41 of ACGT ACGT ...: G, then C
    return c


FUZZ_SEEDS = (32001, 32002, 32003)


@functools.lru_cache(None)
def fuzz_cases():
    """three seeded streams of helpers.random_amplicon_reads(odd_ops=0.3), each once with a sparse list and once with every position listed;
    together they must hold enough of everything (asserted here, on the CPU, while the table is built)"""
    from tests import helpers

    out = []
    one_other = far = outside = 0
    for k, seed in enumerate(FUZZ_SEEDS):
        rng = np.random.default_rng(seed)
        n_amp = int(rng.integers(6, 12))
        amps, pairs = [], []
        for a in range(n_amp):
            ref_id = a * 3 // n_amp
            start = 500 + 170 * a + int(rng.integers(0, 40))
            amps.append((ref_id, start, start + 130))
            pairs += [(ref_id, p) for p in range(start - 10, start + 190)]
        dense = make_keys(pairs)
        sparse = np.sort(rng.choice(dense, size=12 * n_amp, replace=False))
        n = (900, 777, 600)[k]
        reads = helpers.random_amplicon_reads(rng, None, amps, n, read_len=(40, 150), name_len=(1, 40), odd_ops=0.3, unplaced=0.02)
        if k == 1:
            reads = [reads[i] for i in rng.permutation(len(reads))]
        gaps = {int(i): int(rng.integers(1, 70)) for i in rng.integers(0, len(reads), size=20)}
        src = build_stream(reads, lead=int(rng.integers(0, 40)), gaps=gaps, trail=int(rng.integers(16, 64)))
        for style, keys in (("sparse", sparse), ("dense", dense)):
            c = Case(f"fuzz_{seed}_{len(reads)}_reads_{style}", src, keys, mbq=(20, 21, 10)[k], mrq=(20, 5, 21)[k], reads=reads)
            t = c.want().table
            one_other += int(t[:, :, OTHER, :OTHER].sum() + t[:, :, :OTHER, OTHER].sum())
            far += int(t[:, K - 1].sum())
            outside += c.outside_window()
            out.append(c)
    assert one_other >= 50 and far >= 50 and outside >= 10, (one_other, far, outside)
    return tuple(out)


@functools.lru_cache(None)
def cases():
    """the whole table: deterministic cases, the depth case, the fuzz streams"""
    return deterministic_cases() + (depth_case(),) + fuzz_cases()


# the cases the invariant is tested on, with the fewest cells whose precondition must hold there (asserted in tests/test_phase_model.py)
INVARIANT_CASES = {"two_keys_one_read_of_each_of_the_25_state_pairs": 1, "nine_keys_inside_one_read": 36, "leading_5S": 1, "an_I_between_the_two_keys": 1,
                   "keys_in_the_middle_and_at_both_ends_of_a_D_10M5D10M": 15, f"{256}_reads": 1, f"depth_{DEPTH_READS}_identical_reads_one_cell": 1,
                   f"fuzz_{FUZZ_SEEDS[0]}_900_reads_sparse": 20}

# variant -> the deterministic cases that must catch it (tests/test_phase_model.py asserts that each of them does)
CAUGHT_BY = {
    "D_not_covered": ("keys_in_the_middle_and_at_both_ends_of_a_D_10M5D10M",),
    "N_not_covered": ("keys_in_the_middle_and_at_both_ends_of_a_N_10M5N10M",),
    "low_bq_dropped": ("quality_below_and_at_mbq", "two_keys_one_read_of_each_of_the_25_state_pairs"),
    "partner_K_plus_1_counted": ("ten_keys_inside_one_read",),
    "partner_K_dropped": ("nine_keys_inside_one_read", "ten_keys_inside_one_read"),
    "one_past_end_covered": ("a_read_that_ends_on_a_key_and_one_that_ends_a_base_before_it",),
    "first_column_not_covered": ("a_read_that_starts_on_a_key_and_one_that_starts_a_base_behind_it",),
    "soft_clips_shift_columns": ("leading_5S",),
    "I_advances_reference": ("an_I_between_the_two_keys",),
    "mrq_off_by_one": ("a_filtered_an_unplaced_and_reads_at_mrq_and_below",),
    "mbq_off_by_one": ("quality_below_and_at_mbq",),
    "table_transposed": ("leading_5S", "an_I_between_the_two_keys", "quality_below_and_at_mbq"),
}


# ---------------------------------------------------------------------------------------------------------------------------
# score cases: (name, table [P][K][5][5], pair cells, pair nts, min_alt, min_share)
# ---------------------------------------------------------------------------------------------------------------------------
def one_cell(rr=0, ra=0, ar=0, aa=0, other=0, P=2):
    """a table of P keys whose cell (0, 0) holds the corners for ref A, alt C at both keys, and `other` reads with OTHER at both"""
    t = np.zeros((P, K, STATES, STATES), np.int64)
    t[0, 0, 0, 0], t[0, 0, 0, 1], t[0, 0, 1, 0], t[0, 0, 1, 1], t[0, 0, OTHER, OTHER] = rr, ra, ar, aa, other
    return t


AC = (0, 1, 0, 1)


@functools.lru_cache(None)
def score_cases():
    out = []

    def add(name, table, cells, nts, min_alt=4, min_share=10):
        out.append((name, np.asarray(table, np.int64), [int(c) for c in cells], np.asarray(nts, np.int64).reshape(-1, 4), min_alt, min_share))
        return score(*out[-1][1:])

    s = add("all_four_corners_zero", one_cell(other=9), [0], [AC])
    assert s.ints[0].tolist() == [0, 0, 0, 0, 9, 9] and s.score[0] == 0 and s.cls[0] == 0
    s = add("only_aa", one_cell(aa=40), [0], [AC])
    assert s.ints[0].tolist() == [0, 0, 0, 40, 40, 0] and s.score[0] == 0 and s.cls[0] == 1
    s = add("only_ar_and_ra", one_cell(ar=40, ra=40), [0], [AC])
    assert s.cls[0] == 6 and s.score[0] < -13  # alt at j on none of the 40 reads with alt at i, on all 40 with ref at i
    want_cls = {0: dict(rr=300), 1: dict(rr=300, aa=40), 2: dict(rr=300, ar=40), 3: dict(rr=300, aa=40, ar=40), 4: dict(rr=300, ra=40), 5: dict(rr=300, aa=40, ra=40),
                6: dict(rr=300, ar=40, ra=40), 7: dict(rr=300, aa=40, ar=40, ra=40)}
    s = add("each_of_the_classes_0_to_7", np.concatenate([one_cell(**kw) for kw in want_cls.values()]), [2 * i * K for i in range(8)], [AC] * 8)
    assert s.cls.tolist() == list(range(8)) and s.score[1] > 13 and s.score[6] < -13 and s.score[0] == 0
    s = add("min_alt_minus_1_and_min_alt", np.concatenate([one_cell(rr=100, aa=3, ar=50), one_cell(rr=100, aa=4, ar=36)]), [0, 2 * K], [AC] * 2)
    assert s.cls.tolist() == [2, 3]
    s = add("the_share_met_exactly_and_one_read_short_of_it", np.concatenate([one_cell(rr=100, aa=10, ar=90), one_cell(rr=100, aa=9, ar=90)]), [0, 2 * K], [AC] * 2)
    assert s.cls.tolist() == [3, 2]  # 100 x 10 = 10 x 100; 100 x 9 < 10 x 99
    s = add("a_large_group_below_the_share", one_cell(rr=100, aa=50, ar=1000), [0], [AC])
    assert s.cls[0] == 2
    s = add("ref_equals_alt_and_nts_of_4_and_minus_1", one_cell(rr=100, aa=40), [0] * 5, [(0, 0, 0, 1), (0, 1, 1, 1), (4, 1, 0, 1), (0, 1, 0, -1), AC])
    assert s.cls.tolist() == [-1] * 4 + [1] and s.ints[:4].tolist() == [[-1] * 6] * 4 and not s.score[:4].any()
    s = add("pair_cells_at_and_beyond_the_end_of_the_table", one_cell(rr=100, aa=40, P=3), [3 * K, 3 * K + 5, -1, 1, 1 * K + 1, 2 * K, 1 * K, 0], [AC] * 8)
    assert s.cls.tolist() == [-1, -1, -1, 0, -1, -1, 0, 1]  # P K; beyond; negative; (0, 1): tested; i + 1 + k = P twice; (1, 0): tested; (0, 0)
    big = (1 << 31) - 1
    s = add("counts_near_2_to_the_31_in_one_corner", np.concatenate([one_cell(rr=big, aa=5, ar=4, ra=4), one_cell(aa=big, rr=7, ar=2, ra=3)]), [0, 2 * K], [AC] * 2)
    assert s.ints[0, 0] == big and s.ints[1, 3] == big and s.cls.tolist() == [7, 1] and s.score[0] > 13
    return tuple(out)


SCORE_CAUGHT_BY = {
    "presence_without_share": ("the_share_met_exactly_and_one_read_short_of_it", "a_large_group_below_the_share"),
    "share_strict": ("the_share_met_exactly_and_one_read_short_of_it",),
    "class_bits_swapped": ("each_of_the_classes_0_to_7", "min_alt_minus_1_and_min_alt"),
}


def random_tables(rng, P):
    """P random keys: depths from nothing to thousands in the corners, some in the other states; (table, cells, nts): every cell of the
    table once, and some cells and alleles outside their ranges"""
    t = np.zeros((P, K, STATES, STATES), np.int64)
    for i in range(P):
        for k in range(min(K, P - 1 - i)):
            depth = int(rng.choice([0, 1, 5, 30, 200, 3000]))
            t[i, k] = rng.multinomial(depth, rng.dirichlet(np.ones(PAIR) * 0.3)).reshape(STATES, STATES)
    cells = np.concatenate([np.arange(P * K), rng.integers(-5, P * K + 5, size=40), [-1, -5, P * K, P * K + 4]])
    nts = rng.integers(0, 4, size=(len(cells), 4))
    bad = rng.random(len(cells)) < 0.1
    nts[bad, rng.integers(0, 4, size=int(bad.sum()))] = rng.choice([-1, 4, 5, -2], size=int(bad.sum()))
    return t, cells, nts


# ---------------------------------------------------------------------------------------------------------------------------
# the command's cases: (name, reads, lines [(chrom, pos, ref, alt)], parameters); chromosome names: the reference ids of the BAM header
# tests/test_gpu_phase_cli.py writes (ref_id r is "chr<r + 1>")
# ---------------------------------------------------------------------------------------------------------------------------
CliCase = collections.namedtuple("CliCase", "name reads lines params expect")


def planted_reads():
    """one amplicon, 400 reads of 100 bases over 1000 .. 1099, reference A everywhere; the alts planted by read index"""
    plant = {1010: ("C", range(0, 40)), 1011: ("C", range(0, 40)),                       # adjacent, the alt on the same 40 reads
             1020: ("G", range(40, 80)), 1050: ("G", range(80, 120)),                    # 30 apart, the alts on disjoint sets of 40 reads
             1060: ("T", range(120, 160)), 1065: ("T", range(120, 140)),                 # B's alt on 20 of A's 40 alt reads
             1070: ("C", list(range(160, 180)) + list(range(180, 200))), 1075: ("C", list(range(160, 180)) + list(range(200, 220))),  # 20 in each of aa, ar, ra
             1090: ("G", range(220, 222))}                                               # a variant with 2 alt reads
    reads = []
    for r in range(400):
        seq = ["A"] * 100
        for pos, (alt, who) in plant.items():
            if r in who:
                seq[pos - 1000] = alt
        reads.append(read(0, 999, "100M", None, flag=0x10 * (r & 1), seq="".join(seq), qual=[30] * 100, name=f"p{r}"))
    lines = [("chr1", pos, "A", alt) for pos, (alt, _) in sorted(plant.items())]
    expect = {(1010, 1011): "CIS", (1020, 1050): "TRANS", (1060, 1065): "NESTED_B", (1070, 1075): "MIXED", (1075, 1090): "UNTESTED"}
    return reads, lines, expect


@functools.lru_cache(None)
def cli_cases():
    reads, lines, expect = planted_reads()
    out = [CliCase("planted_pairs", reads, lines, {}, expect)]
    out.append(CliCase("a_position_listed_twice_with_two_alts", reads, [("chr1", 1010, "A", "C"), ("chr1", 1010, "A", "T"), ("chr1", 1011, "A", "C"), ("chr1", 1011, "a", "g")], {},
                       {}))
    out.append(CliCase("an_unknown_chromosome_and_a_multi_base_alt", reads, [("chr1", 1010, "A", "C"), ("chrUn", 1010, "A", "C"), ("chrUn", 1011, "A", "C"), ("chr1", 1011, "A", "CT"),
                                                                              ("chr1", 1012, "N", "C"), ("chr1", 1020, "A", "G")], {}, {}))
    far = [("chr1", 1005 + 5 * i, "A", "C") for i in range(K + 3)]
    out.append(CliCase("a_pair_beyond_K_keys_and_a_short_max_dist", reads, far, dict(max_dist=48, min_alt=2, min_share=0, q_min=3.5), {}))
    return tuple(out)


def cli_keys(case):
    """(keys, key_index per line) of a command case: the distinct (ref_id, pos) of the lines on a known chromosome (chr1 = reference 0)"""
    keys = make_keys([(0, l[1]) for l in case.lines if l[0] == "chr1"])
    index = [int(np.searchsorted(keys, np.uint64(l[1]))) if l[0] == "chr1" else -1 for l in case.lines]
    return keys, index


def cli_params(case):
    return {**dict(mbq=20, mrq=20, min_alt=4, min_share=10, q_min=13.0, max_dist=200), **case.params}


# ---------------------------------------------------------------------------------------------------------------------------
# the table on a device
# ---------------------------------------------------------------------------------------------------------------------------
def upload(case, first=0, last=None):
    """(bam, rec_off, keys) of the case's reads [first, last) as device tensors for read_phase"""
    import torch

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
    return up(case.buf, np.uint8), up(case.rec_off[first:last], np.int64), up(case.keys, np.int64)


def device_result(ctx, table, stats):
    import torch

    ctx.sync()
    torch.cuda.synchronize()
    return Result(table.cpu().numpy().astype(np.int64), None if stats is None else tuple(int(x) for x in stats.cpu().tolist()))


def differences(got, want, stats=True):
    """[] or what differs between a device Result and the model's"""
    bad = []
    if not np.array_equal(got.table, want.table):
        at = np.argwhere(got.table != want.table)
        bad.append(f"{len(at)} cells differ, first at (key i, partner k, s_i, s_j) {at[0].tolist()}: {int(got.table[tuple(at[0])])} != {int(want.table[tuple(at[0])])}")
    if stats and tuple(got.stats) != tuple(want.stats):
        bad.append(f"stats {got.stats} != {want.stats}")
    return bad


S_TOL = 1e-5  # the tolerance tests/test_paired_host.py holds ampli_pair_score to


def score_differences(got, want):
    """[] or what differs between two Scores: the integers and classes exactly, the scores within S_TOL"""
    bad = []
    for name, g, w in (("ints", got.ints, want.ints), ("cls", got.cls, want.cls)):
        g, w = np.asarray(g, np.int64), np.asarray(w, np.int64)
        if g.shape != w.shape or not np.array_equal(g, w):
            at = np.argwhere(g != w) if g.shape == w.shape else [["shape"]]
            bad.append(f"{name}: {len(at)} differ, first at {list(at[0])}")
    g, w = np.asarray(got.score, np.float64), np.asarray(want.score, np.float64)
    off = np.abs(g - w)
    if g.shape != w.shape or not np.all(off <= S_TOL):
        bad.append(f"score: the largest difference is {off.max() if off.size else None!r}")
    return bad
