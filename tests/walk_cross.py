"""Every read walk over every case table -- TEST INFRASTRUCTURE of tests/test_gpu_walks_cross_tables.py and tests/test_scale_shapes.py.

The four kernels that walk alignment records share csrc/ampli_bam.h (the record decode, bam_window_base, bam_window_find, the
bisections), and each has a case table written for its own geometry: tests/pileup_model.py, indel_model.py, evidence_model.py and
amplicon_count_model.py.  The models take any stream, so every table serves every kernel:
  * a pileup, indel or evidence case is (stream, keys, mbq, mrq) and goes to the other two of those as it is;
  * for ampli_pileup_amplicon_count a design is derived from the case's keys (design_of);
  * an amplicon-count case goes to the other three with the union of its amplicons' positions as keys.
Every table is used whole but for LEFT_OUT.  Models are computed once per (kernel, case) and never changed."""
import collections
import functools

import numpy as np

from tests import amplicon_count_model as am
from tests import evidence_model as em
from tests import indel_model as im
from tests import pileup_model as pm

KERNELS = ("pileup", "indel", "evidence", "amplicon")
# the one case left out of the cross runs: 300 000 reads take the indel and evidence models 8-9 s each
LEFT_OUT = "depth_300000_identical_starts"
LONG_RUN = 40  # a run of consecutive keys longer than this gets a second, overlapping amplicon
# min_overlap of the derived designs and of the amplicon table's own: the default, and for every second case of a table the strictest
# value, at which a read is off-target unless it lies wholly inside its amplicon (the threshold's arithmetic at equality)
MIN_OVERLAPS = (50, 100)

Stream = collections.namedtuple("Stream", "table name buf rec_off keys intervals mbq mrq min_overlap")


def _tables():
    return {"pileup": pm.cases(), "indel": im.cases(), "evidence": em.cases(), "amplicon": am.cases()}


def runs_of(keys):
    """[(ref_id, first, last)]: the maximal runs of consecutive keys on one reference"""
    k = np.asarray(keys, np.uint64).astype(np.int64)  # (ref ids of the tables are small: the keys fit 63 bits)
    if len(k) == 0:
        return []
    cut = np.flatnonzero(np.diff(k) != 1) + 1  # a step to the next reference is never 1: positions are >= 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(k)]]) - 1
    return [(int(k[s] >> 32), int(k[s] & 0xFFFFFFFF), int(k[e] & 0xFFFFFFFF)) for s, e in zip(starts, ends)]


def design_of(keys):
    """The amplicons derived from a panel: every maximal run of consecutive keys is an amplicon; a run of more than LONG_RUN positions
    gets a second one that starts in the middle of the run and ends a quarter of its length behind it, so that the reads of the run's
    second half lie on two amplicons and the assignment has something to decide.  In the order found (not the sorted order)."""
    out = []
    for ref_id, first, last in runs_of(keys):
        out.append((ref_id, first, last))
        n = last - first + 1
        if n > LONG_RUN:
            out.append((ref_id, first + n // 2, min(last + n // 4, 2 ** 31 - 2)))
    return out


def keys_of(intervals):
    """the union of the amplicons' positions as sorted unique keys"""
    return np.unique(np.concatenate([(np.uint64(r) << np.uint64(32)) | np.arange(f, l + 1, dtype=np.uint64) for r, f, l in intervals]))


@functools.lru_cache(None)
def streams(table):
    """the table's cases as Streams, whole but for LEFT_OUT"""
    out = []
    for i, c in enumerate(_tables()[table]):
        if c.name == LEFT_OUT:
            continue
        if table == "amplicon":  # (the amplicon kernel never runs over its own table here: min_overlap is unused)
            out.append(Stream(table, c.name, c.buf, c.rec_off, keys_of(c.intervals), tuple(c.intervals), c.mbq, c.mrq, c.min_overlap))
        else:
            out.append(Stream(table, c.name, c.buf, c.rec_off, c.keys, tuple(design_of(c.keys)), c.mbq, c.mrq, MIN_OVERLAPS[i % len(MIN_OVERLAPS)]))
    assert len(out) == len(_tables()[table]) - (table == "pileup"), table
    return tuple(out)


def staged_stream(s):
    """(buf, rec_off) as ampli_pileup_count takes them: offsets ascending (the other three walks take any order; the counts do not
    depend on it) and 16 readable bytes behind the last record"""
    off = np.sort(np.asarray(s.rec_off, np.uint64))
    end = int(pm.headers(s.buf, off).end.max())
    buf = s.buf if len(s.buf) - end >= 16 else np.concatenate([s.buf, np.frombuffer(pm.garbage(16 - (len(s.buf) - end)), np.uint8)])
    return buf, off


_MODELS = {}


def model(kernel, s):
    """the kernel's own model on the stream; (result, non-zero?)"""
    key = (kernel, s.table, s.name)
    if key not in _MODELS:
        src = (s.buf, s.rec_off)
        if kernel == "pileup":
            r = pm.count(staged_stream(s), s.keys, s.mbq, s.mrq)
            nz = r[2] > 0
        elif kernel == "indel":
            r = im.count(src, s.keys, s.mbq, s.mrq)
            nz = r.stats[1] > 0
        elif kernel == "evidence":
            r = em.count(src, s.keys, s.mbq, s.mrq)
            nz = r.stats[1] > 0
        else:
            r = am.count(src, am.make_amplicons(s.intervals), s.mbq, s.mrq, s.min_overlap)
            nz = r.stats[2] > 0
        _MODELS[key] = (r, bool(nz))
    return _MODELS[key]


def decided_by_overlap(s, r):
    """how many assigned reads of the stream overlap two amplicons or more of its design and went to the one of strictly largest
    overlap (Result.decided == 0 alone also holds for a read with one candidate)"""
    amps = am.make_amplicons(s.intervals)
    h = pm.headers(s.buf, s.rec_off)
    rd = np.flatnonzero((r.assigned >= 0) & (r.decided == 0))
    if len(rd) == 0:
        return 0
    o_read, _, _, radv, _, _ = am._flat_ops(s.buf, h, rd)
    R = np.bincount(o_read, weights=radv, minlength=len(s.rec_off)).astype(np.int64)[rd]
    sf, sl = h.pos[rd, None] + 1, h.pos[rd, None] + R[:, None]
    ov = (h.ref_id[rd, None] == amps.ref[None, :]) & (np.minimum(sl, amps.last[None, :]) >= np.maximum(sf, amps.first[None, :]))
    return int((ov.sum(1) >= 2).sum())


PAIRS = tuple((k, t) for k in KERNELS for t in KERNELS if t != k)


@functools.lru_cache(None)
def non_vacuity():
    """{(kernel, table): (cases, cases with a non-zero model result)} and, per foreign table of the amplicon kernel, (designs with
    reads decided by overlap among several candidates, designs with kept reads left off-target, designs with both) -- asserted here,
    where the parameters are built, and again by tests/test_scale_shapes.py"""
    share, designs = {}, {}
    for kernel, table in PAIRS:
        res = [model(kernel, s) for s in streams(table)]
        share[kernel, table] = (len(res), sum(nz for _, nz in res))
        assert 2 * share[kernel, table][1] >= share[kernel, table][0], (kernel, table, share[kernel, table])
        if kernel == "amplicon":
            by_overlap = [decided_by_overlap(s, r) > 0 for s, (r, _) in zip(streams(table), res)]
            off_target = [bool((r.assigned == -1).any()) for r, _ in res]
            designs[table] = (sum(by_overlap), sum(off_target), sum(a and b for a, b in zip(by_overlap, off_target)))
            assert designs[table][2] >= 1, (table, designs[table])
    return share, designs
