"""The pileup counting kernel's test model -- TEST INFRASTRUCTURE (never imported by the product).

Four things, all host-side numpy:
  * build_stream: read dicts (the format of helpers.write_bam) -> (buf, rec_off), the raw uncompressed alignment records exactly
    as ampli_pileup_count takes them, with control over what the executable otherwise chooses: the 16-byte phase of the first
    record, filler between records, the length of every read name, the trailing padding.  Filler and padding are non-zero garbage.
  * count: a vectorised restatement of the header comment of ampli_pileup_count (include/amplisolve_hip.h), i.e. of
    oracle/pileup_oracle.pileup, from flat arrays (np.repeat / searchsorted / bincount): half a million reads in seconds.
    `wrong=` switches on one deliberately wrong variant (WRONG_VARIANTS); tests/test_pileup_model.py shows that every one of
    them is caught by a deterministic case of the table below.
  * the kernel's geometry, read from the constexpr lines of ampli_pileup.hip (geometry()), and what it implies for a stream:
    group_spans (the bytes a workgroup stages) and window_bases (where its LDS window starts).
  * cases(): the named case table.  Every case that claims to sit on an edge asserts so with the geometry helpers while the table
    is built, so a retuned kernel either keeps its edge cases on its edges or fails here, on the CPU.
device_check / `python -m tests.pileup_model --child LIB` run the table against a library on the GPU.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os
import re
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "amplisolve_amd", "csrc", "ampli_pileup.hip")
OPS = "MIDNSHP=X"
SEQ_CODE = "=ACMGRSVTWYHKDBN"
READ_MASK = 0x4 | 0x100 | 0x200 | 0x400
REF_OPS, QUERY_OPS, MATCH_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8), (0, 7, 8)
_CODE_OF = bytes.maketrans(SEQ_CODE.encode(), bytes(range(16)))
_B4 = np.full(16, -1, np.int64)
_B4[[1, 2, 4, 8]] = [0, 1, 2, 3]

Geometry = collections.namedtuple("Geometry", "reads stage window")


@functools.lru_cache(None)
def geometry(path=KERNEL_SOURCE):
    """(reads per workgroup, bytes of the LDS stage, panel positions of the staged kernel's window) as the kernel source states them"""
    text = open(path).read()
    vals = {}
    for name in ("READS", "STAGE", "SWINDOW"):
        m = re.search(r"^constexpr\s+int\s+PILEUP_%s\s*=\s*([0-9][0-9\s*]*);" % name, text, re.M)
        assert m, f"no `constexpr int PILEUP_{name} = ...;` line in {path}"
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        vals[name] = v
    return Geometry(vals["READS"], vals["STAGE"], vals["SWINDOW"])


# ---------------------------------------------------------------------------------------------------------------------------
# the record stream
# ---------------------------------------------------------------------------------------------------------------------------
def garbage(n, salt=0):
    """n non-zero bytes that look like nothing a record holds"""
    return bytes(((i + salt) * 37 + 11) % 255 + 1 for i in range(n))


def encode_record(r, k=0):
    """one alignment record, block_size included; the name is r["name"] ("" allowed: l_read_name = 1) or r<k>"""
    name = (r["name"] if r.get("name") is not None else f"r{k}").encode() + b"\0"
    assert 1 <= len(name) <= 255
    seq = r["seq"]
    codes = np.frombuffer(seq.encode().translate(_CODE_OF) + (b"\0" if len(seq) & 1 else b""), np.uint8)
    packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
    cig = b"".join(struct.pack("<I", (n << 4) | OPS.index(op)) for op, n in r["cigar"])
    body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(seq), -1, -1, 0)
    body += name + cig + packed + bytes(r["qual"])
    return struct.pack("<I", len(body)) + body


def build_stream(reads, lead=0, gaps=None, trail=16):
    """(buf uint8, rec_off uint64): the records of `reads` in order.  lead: filler bytes in front of the first record (its offset
    mod 16 is lead mod 16); gaps: {k: filler bytes in front of record k} -- what a record the host scanner dropped leaves behind;
    trail: garbage behind the last record (>= 16: the kernel copies whole 16-byte pieces).  Upload buf 16-byte aligned."""
    assert trail >= 16
    gaps = gaps or {}
    parts, offs, o = [garbage(lead)], [], lead
    memo = {}
    for k, r in enumerate(reads):
        g = gaps.get(k, 0)
        if g:
            parts.append(garbage(g, k))
            o += g
        rec = memo.get(id(r)) if r.get("name") is not None else None  # a read object listed many times is encoded once
        if rec is None:
            rec = encode_record(r, k)
            if r.get("name") is not None:
                memo[id(r)] = rec
        offs.append(o)
        parts.append(rec)
        o += len(rec)
    parts.append(garbage(trail, 5))
    return np.frombuffer(bytearray(b"".join(parts)), np.uint8), np.asarray(offs, np.uint64)


def records_only(buf, rec_off):
    """the listed records' own bytes, back to back (no filler): what a BAM file of them holds behind its header"""
    b = bytes(buf)
    out = []
    for o in rec_off.tolist():
        bs, = struct.unpack_from("<I", b, o)
        out.append(b[o:o + 4 + bs])
    return b"".join(out)


def write_bam_of(path, buf, rec_off, block=60000):
    """a BAM file (BGZF-framed, empty header text, no reference) holding exactly the listed records"""
    raw = b"BAM\1" + struct.pack("<ii", 0, 0) + records_only(buf, rec_off)
    out = bytearray()
    for o in range(0, len(raw), block):
        piece = raw[o:o + block]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        data = co.compress(piece) + co.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(data) + 25) + data
        out += struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    with open(path, "wb") as f:
        f.write(bytes(out))


def as_stream(src):
    """src: a list of read dicts (default stream) or (buf, rec_off)"""
    if isinstance(src, tuple):
        return np.asarray(src[0], np.uint8), np.asarray(src[1], np.uint64)
    return build_stream(src)


def make_keys(pairs):
    """sorted unique uint64 keys (reference id << 32 | 1-based position) of (ref_id, pos) pairs"""
    return np.unique(np.asarray([(int(r) << 32) | int(p) for r, p in pairs], np.uint64))


def _le(b, at, nbytes):
    v = np.zeros(len(at), np.int64)
    for i in range(nbytes):
        v |= b[at + i].astype(np.int64) << (8 * i)
    return v


Headers = collections.namedtuple("Headers", "off ref_id pos l_name mapq n_cigar flag l_seq cig seq qual end")


def headers(buf, rec_off):
    """the fixed fields of every listed record and the offsets of its CIGAR, sequence and quality arrays in buf"""
    o = np.asarray(rec_off, np.uint64).astype(np.int64)
    i32 = lambda at: _le(buf, at, 4).astype(np.uint32).astype(np.int32).astype(np.int64)  # noqa: E731
    l_name, n_cigar, l_seq = _le(buf, o + 12, 1), _le(buf, o + 16, 2), i32(o + 20)
    cig = o + 36 + l_name
    seq = cig + 4 * n_cigar
    return Headers(o, i32(o + 4), i32(o + 8), l_name, _le(buf, o + 13, 1), n_cigar, _le(buf, o + 18, 2), l_seq, cig, seq, seq + (l_seq + 1) // 2,
                   o + 4 + _le(buf, o, 4))


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's geometry on a stream
# ---------------------------------------------------------------------------------------------------------------------------
def group_spans(buf, rec_off):
    """int64 [groups][2]: per workgroup of geometry().reads consecutive records, the bytes it looks at as the kernel defines
    them -- from its first record's offset rounded down to 16 to the end of its last record.  It stages them iff their number
    is <= geometry().stage."""
    R = geometry().reads
    o = np.asarray(rec_off, np.uint64).astype(np.int64)
    n = len(o)
    first = o[0::R]
    last = o[np.minimum(np.arange(len(first)) * R + R, n) - 1]
    return np.stack([first & ~np.int64(15), last + 4 + _le(np.asarray(buf, np.uint8), last, 4)], 1)


def _key_of(ref_id, pos1):
    return (ref_id.astype(np.uint64) << np.uint64(32)) | pos1.astype(np.uint64)


def window_bases(src, keys):
    """int64 [groups]: the index of the first key at or behind the start of the group's first placed read (ref_id >= 0 and
    pos >= 0, whatever its flags); 0 for a group without one.  The group's LDS window is keys[base : base + geometry().window]."""
    buf, rec_off = as_stream(src)
    h = headers(buf, rec_off)
    R = geometry().reads
    n = len(rec_off)
    placed = (h.ref_id >= 0) & (h.pos >= 0)
    at = np.searchsorted(np.asarray(keys, np.uint64), _key_of(np.where(placed, h.ref_id, 0), np.where(placed, h.pos + 1, 0)))
    out = np.zeros((n + R - 1) // R, np.int64)
    for g in range(len(out)):
        idx = np.flatnonzero(placed[g * R:(g + 1) * R])
        if len(idx):
            out[g] = at[g * R + idx[0]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the vectorised reference
# ---------------------------------------------------------------------------------------------------------------------------
# name -> what is wrong; count(..., wrong=name) computes that variant
WRONG_VARIANTS = {
    "mbq_strict": "quality > mbq instead of >=",
    "mrq_strict": "MAPQ > mrq instead of >=",
    "mask_without_0x4": "unmapped reads kept",
    "mask_without_0x100": "secondary reads kept",
    "mask_without_0x200": "QC-fail reads kept",
    "mask_without_0x400": "duplicates kept",
    "mask_with_0x800": "supplementary reads dropped",
    "reverse_from_0x20": "reverse planes taken from the mate's strand bit",
    "I_consumes_reference": "insertions advance the reference position",
    "N_consumes_nothing": "reference skips do not advance the reference position",
    "P_consumes_query": "padding advances the query position",
    "nibble_parity_swapped": "even query offsets read the low nibble",
    "key_off_by_one": "bases land one panel position too far",
    "last_read_dropped": "the last read of the stream is not walked",
    "last_partial_group_dropped": "the reads behind the last whole group are not walked",
    "window_last_key_dropped": "bases on the window's last key are lost",
    "behind_window_dropped": "bases behind the window are lost",
    "before_window_dropped": "bases before the window are lost",
    "straddling_runs_dropped": "runs that start inside the window and end behind it are lost",
    "unstaged_groups_dropped": "reads of groups whose bytes exceed the stage are not walked",
}
# Not in the list, with the reason: "bases behind the LAST key dropped" -- there is no key behind the last one, so nothing is ever
# counted there: equivalent to the reference by construction.

Counted = collections.namedtuple("Counted", "read key")


def count(src, keys, mbq, mrq, wrong=None, detail=False, chunk=1 << 22):
    """(counts int64 [P][8], reads kept, bases counted) of the stream `src` (read dicts or (buf, rec_off)) on the panel `keys`;
    with detail=True a fourth value Counted(read, key): for every counted base the index of its read in the stream and of its
    key in `keys`."""
    assert wrong is None or wrong in WRONG_VARIANTS, wrong
    buf, rec_off = as_stream(src)
    keys = np.asarray(keys, np.uint64)
    P = len(keys)
    geo = geometry()
    h = headers(buf, rec_off)
    n = len(rec_off)
    mask = READ_MASK
    if wrong and wrong.startswith("mask_without_"):
        mask &= ~int(wrong[len("mask_without_"):], 16)
    if wrong == "mask_with_0x800":
        mask |= 0x800
    keep = (h.ref_id >= 0) & (h.pos >= 0) & ((h.flag & mask) == 0) & ((h.mapq > mrq) if wrong == "mrq_strict" else (h.mapq >= mrq))
    if wrong == "last_read_dropped":
        keep[n - 1:] = False
    if wrong == "last_partial_group_dropped":
        keep[n - n % geo.reads:n] = n % geo.reads == 0
    group = np.arange(n) // geo.reads
    if wrong == "unstaged_groups_dropped":
        sp = group_spans(buf, rec_off)
        keep &= (sp[:, 1] - sp[:, 0] <= geo.stage)[group]
    windowed = wrong in ("window_last_key_dropped", "behind_window_dropped", "before_window_dropped", "straddling_runs_dropped")
    wb = window_bases((buf, rec_off), keys) if windowed else None
    counts = np.zeros(P * 8, np.int64)
    kept = int(keep.sum())
    rd = np.flatnonzero(keep)
    out_read, out_key = [], []
    # CIGAR operations of the kept reads, flat
    nc = h.n_cigar[rd]
    op_read = np.repeat(rd, nc)
    first_op = np.cumsum(nc) - nc
    op_idx = np.arange(len(op_read)) - np.repeat(first_op, nc)
    v = _le(buf, h.cig[op_read] + 4 * op_idx, 4)
    op, ln = v & 15, v >> 4
    ref_ops = REF_OPS + (1,) if wrong == "I_consumes_reference" else tuple(x for x in REF_OPS if not (wrong == "N_consumes_nothing" and x == 3))
    query_ops = QUERY_OPS + (6,) if wrong == "P_consumes_query" else QUERY_OPS
    radv, qadv = np.where(np.isin(op, ref_ops), ln, 0), np.where(np.isin(op, query_ops), ln, 0)

    def before(adv):  # what the read's earlier operations consumed
        c = np.cumsum(adv) - adv
        return c - np.repeat(c[first_op[nc > 0]], nc[nc > 0]) if len(c) else c

    rbef, qbef = before(radv), before(qadv)
    runs = np.flatnonzero(np.isin(op, MATCH_OPS) & (ln > 0))
    run_read, run_len = op_read[runs], ln[runs]
    run_ref = h.pos[run_read] + 1 + rbef[runs]  # 1-based position of the run's first base
    run_q = qbef[runs]
    added = 0
    if len(runs):  # whole runs, a few million bases at a time
        edges = np.concatenate([[0], np.flatnonzero(np.diff((np.cumsum(run_len) - run_len) // chunk)) + 1, [len(runs)]])
    else:
        edges = np.zeros(1, np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        rl = run_len[a:b]
        base_run = np.repeat(np.arange(a, b), rl)
        j = np.arange(len(base_run)) - np.repeat(np.cumsum(rl) - rl, rl)
        read = run_read[base_run]
        refp = run_ref[base_run] + j + (1 if wrong == "key_off_by_one" else 0)
        key = _key_of(h.ref_id[read], refp)
        ki = np.searchsorted(keys, key)
        ok = keys[np.minimum(ki, P - 1)] == key
        q = run_q[base_run] + j
        ok &= q < h.l_seq[read]  # only a wrong variant can walk off the sequence
        if windowed:
            rel = ki - wb[group[read]]
            if wrong == "window_last_key_dropped":
                ok &= rel != geo.window - 1
            elif wrong == "behind_window_dropped":
                ok &= rel < geo.window
            elif wrong == "before_window_dropped":
                ok &= rel >= 0
            else:
                g = group[run_read[a:b]]
                nw = np.minimum(P - wb[g], geo.window)
                k0 = _key_of(h.ref_id[run_read[a:b]], run_ref[a:b])
                wk0, wkl = keys[np.minimum(wb[g], P - 1)], keys[np.clip(wb[g] + nw - 1, 0, P - 1)]
                straddle = (nw > 0) & (k0 >= wk0) & (k0 <= wkl) & (k0 + (rl - 1).astype(np.uint64) > wkl)
                ok &= ~straddle[base_run - a]
        sel = np.flatnonzero(ok)
        read, ki, q = read[sel], ki[sel], q[sel]
        byte = buf[h.seq[read] + (q >> 1)].astype(np.int64)
        even = (q & 1) == 0
        if wrong == "nibble_parity_swapped":
            even = ~even
        b4 = _B4[np.where(even, byte >> 4, byte & 15)]
        qual = buf[h.qual[read] + q].astype(np.int64)
        good = (b4 >= 0) & ((qual > mbq) if wrong == "mbq_strict" else (qual >= mbq))
        read, ki, b4 = read[good], ki[good], b4[good]
        rev = (h.flag[read] & (0x20 if wrong == "reverse_from_0x20" else 0x10)) != 0
        counts += np.bincount(ki * 8 + b4, minlength=P * 8)
        counts += np.bincount(ki[rev] * 8 + 4 + b4[rev], minlength=P * 8)
        added += len(ki)
        if detail:
            out_read.append(read)
            out_key.append(ki)
    res = (counts.reshape(P, 8), kept, added)
    if detail:
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)  # noqa: E731
        res += (Counted(cat(out_read), cat(out_key)),)
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, src, keys, mbq=20, mrq=20, reads=None):
        self.name, self.mbq, self.mrq = name, int(mbq), int(mrq)
        self.reads = src if not isinstance(src, tuple) else reads  # the read dicts when the case has them
        self.buf, self.rec_off = as_stream(src)
        self.keys = np.asarray(keys, np.uint64)
        assert len(self.keys) > 0 and np.all(self.keys[1:] > self.keys[:-1]), name
        assert np.all(self.rec_off[1:] > self.rec_off[:-1]), name  # the contract: ascending offsets
        h = headers(self.buf, self.rec_off)
        assert len(self.buf) - int(h.end.max()) >= 16 and int(h.end.max()) <= len(self.buf), name

    @property
    def n_reads(self):
        return len(self.rec_off)

    @property
    def stream(self):
        return self.buf, self.rec_off

    def spans(self):
        return group_spans(self.buf, self.rec_off)

    def staged(self):
        s = self.spans()
        return s[:, 1] - s[:, 0] <= geometry().stage

    def bases(self):
        return window_bases(self.stream, self.keys)

    def want(self, **kw):
        return count(self.stream, self.keys, self.mbq, self.mrq, **kw)

    def __repr__(self):
        return f"Case({self.name}: {self.n_reads} reads, {len(self.keys)} keys, mbq={self.mbq}, mrq={self.mrq})"


def read(ref_id, pos, cigar, rng, flag=0, mapq=60, name=None, qual=None, seq=None):
    """one read dict; cigar as [(op, len)] or a string like "5S100M"; random A/C/G/T and qualities 20..60 unless given"""
    if isinstance(cigar, str):
        cigar = [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    qlen = sum(n for op, n in cigar if op in "MIS=X")
    if seq is None:
        seq = "".join("ACGT"[i] for i in rng.integers(0, 4, size=qlen))
    if qual is None:
        qual = rng.integers(20, 61, size=len(seq)).tolist()
    return dict(ref_id=int(ref_id), pos=int(pos), mapq=int(mapq), flag=int(flag), cigar=cigar, seq=seq, qual=list(qual), name=name)


def span_keys(ref_id, first, last):
    """contiguous keys first..last (1-based, inclusive) on one reference"""
    return (np.uint64(ref_id) << np.uint64(32)) | np.arange(first, last + 1, dtype=np.uint64)


def _rel_index(case, read_idx):
    """window-relative key indices of the bases read `read_idx` of the case counts"""
    _, _, _, d = case.want(detail=True)
    R = geometry().reads
    return d.key[d.read == read_idx] - case.bases()[read_idx // R]


def fit_span(reads, target, lead, with_filler):
    """name lengths (and, with_filler, filler in front of the last record) such that the records of `reads`, the first at offset
    `lead`, end exactly `target` bytes behind the start of the 16-byte piece the first one lies in"""
    for r in reads:
        r["name"] = ""
    buf, off = build_stream(reads, lead=lead)
    need = target - int(group_spans(buf, off)[0, 1] - group_spans(buf, off)[0, 0])
    assert need >= 0, "the reads are too long for this target"
    gaps = {}
    if with_filler:
        gaps[len(reads) - 1] = need % 97
        need -= need % 97
    k = 0
    while need > 0:
        take = min(254 - len(reads[k]["name"]), need, 61 + k % 7)
        reads[k]["name"] += "n" * take
        need -= take
        k = (k + 1) % len(reads)
    return build_stream(reads, lead=lead, gaps=gaps)


def _amplicon(rng, n, ref_id=0, start=1000, length=120, jitter=True):
    return [read(ref_id, start - 1 + (int(rng.integers(0, 4)) if jitter else 0), f"{length - 10}M", rng, flag=0x10 * int(rng.integers(2))) for _ in range(n)]


@functools.lru_cache(None)
def deterministic_cases():
    """the named cases (a tuple), each built from a fixed seed"""
    geo = geometry()
    R, STAGE, W = geo
    out = []

    def add(name, src, keys, mbq=20, mrq=20, reads=None):
        c = Case(name, src, keys, mbq, mrq, reads)
        out.append(c)
        return c

    def rng_of(tag):
        return np.random.default_rng(zlib.crc32(tag.encode()))

    amp_keys = span_keys(0, 1000, 1119)
    # ---- group sizes ----
    for n in (1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 4 * R + 1):
        c = add(f"group_size_{n}", _amplicon(rng_of(f"gs{n}"), n), amp_keys)
        assert c.n_reads == n and np.all(c.staged())
    # ---- stage threshold ----
    for res in (0, 1, 7, 8, 15):
        for d in (-1, 0, 1):
            rs = _amplicon(rng_of(f"st{res}{d}"), R)
            c = add(f"stage_{'under' if d < 0 else 'over' if d > 0 else 'exact'}_phase{res}", fit_span(rs, STAGE + d, res, with_filler=(res % 2 == 1)), amp_keys,
                    reads=rs)
            s = c.spans()
            assert len(s) == 1 and s[0, 1] - s[0, 0] == STAGE + d and int(c.rec_off[0]) % 16 == res and bool(c.staged()[0]) == (d <= 0)
    rg = rng_of("mid")
    rs = _amplicon(rg, R) + [read(0, 999, "110M", rg, name="L" * 200) for _ in range(R)] + _amplicon(rg, R - 7)
    c = add("only_middle_group_unstaged", rs, amp_keys)
    assert c.staged().tolist() == [True, False, True]
    # ---- alignment inside LDS ----
    rg = rng_of("align")
    rs = [read(0, 999 + i % 5, f"{i % 3}S{18 + i % 8}M" if i % 3 else f"{18 + i % 8}M", rg, flag=0x10 * (i & 1), name="x" * (i % 255)) for i in range(2 * 255 + R)]
    c = add("name_lengths_1_to_255", (*build_stream(rs, lead=3),), amp_keys, reads=rs)
    h = headers(*c.stream)
    assert np.all(c.staged()) and set(h.l_name.tolist()) == set(range(1, 256))
    assert {int(a) % 4 for a in h.cig} == {0, 1, 2, 3} and {int(a) % 4 for a in h.seq} == {0, 1, 2, 3} and {int(a) % 4 for a in h.qual} == {0, 1, 2, 3}
    assert {int(x) & 1 for x in h.l_seq} == {0, 1}
    rs = [read(0, 999, f"{s}S{30 + i}M", rg) if s else read(0, 999, f"{30 + i}M", rg) for i in range(4) for s in (0, 1, 2, 3)]
    add("match_runs_at_odd_and_even_query_offsets", rs, amp_keys)
    # ---- the window ----
    wide = span_keys(0, 1000, 2999)
    rg = rng_of("walk")
    walk = [read(0, 999 + 3 * i, "100M", rg, flag=0x10 * (i & 1)) for i in range(600)]
    c = add("walk_across_2000_positions", walk, wide)
    rel = np.concatenate([_rel_index(c, 0), _rel_index(c, R - 1)])
    assert rel.min() == 0 and rel.max() >= W, "the first group must count inside and behind its window"
    anchor = read(0, 999, "30M", rg)
    c = add("run_ends_on_the_last_window_key", [anchor, read(0, 999 + W - 50, "50M", rg, flag=0x10)], span_keys(0, 1000, 1000 + W + 50))
    assert c.bases()[0] == 0 and _rel_index(c, 1).max() == W - 1
    c = add("run_ends_one_past_the_window", [anchor, read(0, 999 + W - 49, "50M", rg, flag=0x10)], span_keys(0, 1000, 1000 + W + 50))
    assert c.bases()[0] == 0 and _rel_index(c, 1).max() == W and _rel_index(c, 1).min() == W - 49
    c = add("second_read_starts_one_before_the_window", [read(0, 1009, "40M", rg), read(0, 1008, "40M", rg, flag=0x10)], wide)
    assert c.bases()[0] == 10 and _rel_index(c, 1).min() == -1
    rs = [read(0, 999 + 7 * i, "100M", rg, flag=0x10 * (i & 1)) for i in range(120)]
    add("every_second_position", rs, wide[::2])
    add("random_half_of_the_positions", rs, np.sort(rng_of("half").choice(wide, size=len(wide) // 2, replace=False)))
    add("isolated_single_positions", rs, wide[::53])
    holes = np.delete(wide, [20, 21, 22, 50, 75, 76, 130, 200, 201, 202, 203, 383, 384, 500])
    c = add("holes_inside_match_runs", rs, holes)
    three = np.concatenate([span_keys(r, 100, 139) for r in (5, 6, 7)])
    rs = [read(5, 99, "40M", rg), read(5, 129, "50M", rg, flag=0x10), read(6, 99, "45M", rg), read(6, 119, "21M", rg), read(7, 89, "30M", rg),
          read(7, 134, "20M", rg, flag=0x10)]
    c = add("three_references_in_one_window", rs, three)
    assert c.bases()[0] == 0 and len(three) < W and len({int(k) >> 32 for k in three[:W]}) == 3
    for P in (1, W - 1, W, W + 1):
        rs = [read(0, 999 + s, "60M", rg, flag=0x10 * (i & 1)) for i, s in enumerate(range(0, P + 30, 17))]
        c = add(f"panel_of_{P}_positions", rs, span_keys(0, 1000, 1000 + P - 1))
        assert len(c.keys) == P
    c = add("all_reads_before_the_first_key", _amplicon(rg, 40), span_keys(0, 5000, 5100))
    assert c.want()[2] == 0 and c.want()[1] == 40
    c = add("all_reads_behind_the_last_key", _amplicon(rg, 40, start=6000), span_keys(0, 5000, 5100))
    assert c.bases()[0] == len(c.keys) and c.want()[2] == 0
    add("key_at_position_1", [read(0, 0, "50M", rg), read(0, 1, "3S20M", rg, flag=0x10)], span_keys(0, 1, 40))
    top, big = (1 << 31) - 1, (1 << 31) - 1
    c = add("keys_at_the_top_of_the_coordinate_range", [read(big, top - 40, "40M", rg), read(big, top - 25, "2S20M1I5M", rg, flag=0x10), read(big - 1, top - 30, "30M", rg)],
            np.concatenate([span_keys(big - 1, top - 10, top), span_keys(big, top - 60, top)]))
    assert int(c.keys[-1]) == (big << 32) | top and c.want()[2] == 40 + 25 + 11
    # ---- CIGAR ----
    gap_keys = np.delete(span_keys(0, 1000, 1199), np.r_[40:60, 100:103])
    add("all_nine_operations", [read(0, 999, "5H3S10M2I5M3D4M20N6M2P7=8X2S3H", rg), read(0, 1004, "4S30=1P1I1P20X", rg, flag=0x10)], gap_keys)
    add("zero_length_operations", [read(0, 999, "0H0S10M0I0D5M0N0P0=7=0X4X0M0S0H", rg), read(0, 1010, "0M0=0X", rg), read(0, 1003, "0I12M0D", rg, flag=0x10)], gap_keys)
    add("leading_and_trailing_clips_and_pads", [read(0, 999, "7H20M9H", rg), read(0, 1001, "7S20M9S", rg, flag=0x10), read(0, 1002, "3P20M4P", rg),
                                                read(0, 1003, "2H3S1P20M1P3S2H", rg)], gap_keys)
    add("deletions_and_skips_over_holes_and_keys", [read(0, 1029, "10M20D10M", rg), read(0, 1029, "10M20N10M", rg, flag=0x10), read(0, 999, "10M15D10M", rg),
                                                    read(0, 999, "10M15N10M", rg, flag=0x10), read(0, 1089, "10M3D5M", rg), read(0, 1094, "5M3N1M1D1M1N9M", rg)], gap_keys)
    add("reads_without_cigar_or_sequence", [read(0, 999, "20M", rg), dict(read(0, 1000, "", rg), seq="ACGTACGTA", qual=[40] * 9), read(0, 1001, "", rg),
                                            read(0, 1002, "3D", rg), read(0, 1003, "20M", rg, flag=0x10)], gap_keys)
    add("one_base_reads", [read(0, 999 + i, "1M", rg, flag=0x10 * (i & 1)) for i in range(70)], gap_keys)
    rs = _amplicon(rg, 5, start=1500) + [read(0, 999, "100000M", rg, flag=0x10)] + _amplicon(rg, 5, start=2500)
    c = add("one_read_of_100000_bases", rs, wide)
    assert not c.staged()[0]
    c = add("two_thousand_alternating_1M1I", [read(0, 999, "1M1I" * 2000, rg), read(0, 1004, "1M1I" * 1999 + "1M", rg, flag=0x10)], wide)
    assert c.staged()[0]
    # ---- filters ----
    bits = [1 << b for b in range(12)]
    c = add("each_flag_bit_alone", [read(0, 999 + i, "60M", rg, flag=f) for i, f in enumerate([0] + bits)], amp_keys)
    assert c.want()[1] == 1 + 12 - 4
    _, _, _, d = c.want(detail=True)
    assert set(np.unique(d.read).tolist()) == {0} | {1 + b for b in range(12) if bits[b] not in (0x4, 0x100, 0x200, 0x400)}
    w = c.want()[0]
    assert w[:, 4:].sum() == 60 and count([c.reads[1 + 5]], amp_keys, 20, 20)[0][:, 4:].sum() == 0  # only 0x10 is reverse; 0x20 is not
    rs = [read(0, 999 + i, "50M", rg, mapq=m, flag=0x10 * (i & 1)) for i, m in enumerate([0, 1, 19, 20, 21, 254, 255])]
    for mrq, kept in ((0, 7), (20, 4), (255, 1)):
        c = add(f"mapq_around_mrq_{mrq}", rs, amp_keys, mrq=mrq)
        assert c.want()[1] == kept
    qs = [0, 1, 19, 20, 21, 254, 255]
    rs = [read(0, 999 + i, "49M", rg, qual=[qs[(i + j) % 7] for j in range(49)], flag=0x10 * (i & 1)) for i in range(9)]
    for mbq, per_read in ((0, 49), (20, 28), (255, 7), (256, 0)):
        c = add(f"quality_around_mbq_{mbq}", rs, amp_keys, mbq=mbq)
        assert c.want()[2] == 9 * per_read
    add("all_sixteen_base_codes", [read(0, 999, "32M", rg, seq=SEQ_CODE * 2), read(0, 1000, "33M", rg, seq=SEQ_CODE[::-1] * 2 + "A", flag=0x10)], amp_keys, mbq=0)
    # ---- order ----
    perm = rng_of("perm").permutation(len(walk))
    add("random_permutation_of_a_sorted_stream", [walk[i] for i in perm], wide)
    un = [read(-1, 1200, "50M", rg), read(0, -1, "50M", rg), read(-1, -1, "50M", rg)]
    c = add("first_reads_of_the_group_unplaced", un + [read(0, 1199, "50M", rg), read(0, 1190, "50M", rg, flag=0x10)], wide)
    assert c.bases()[0] == 200 and c.want()[1] == 2
    c = add("a_whole_group_unplaced", [un[i % 3] for i in range(R)] + _amplicon(rg, 30, start=1400, jitter=False), wide)
    assert c.bases().tolist() == [0, 400] and c.want()[1] == 30
    return tuple(out)


DEPTH_READS = 300_000


def depth_case(n=DEPTH_READS):
    """n reads that all start on the same position of one 120-position amplicon, both strands: every workgroup's updates fall on
    the same few hundred LDS counters, and n of them on one cell"""
    rg = np.random.default_rng(77)
    pool = [read(0, 999, "120M", rg, flag=0x10 * (i & 1), name=f"d{i}") for i in range(16)]
    c = Case(f"depth_{n}_identical_starts", [pool[int(i)] for i in rg.integers(0, 16, size=n)], span_keys(0, 1000, 1119))
    assert c.want()[0][:, :4].sum(1).min() == n
    return c


def fuzz_reads(rng, n, amplicons, **kw):
    """n coordinate-sorted reads in the style of helpers.random_amplicon_reads; beyond a few thousand the stream repeats the
    reads of a drawn pool (drawing every base of 50 000 reads in Python would take the time of the whole suite)"""
    from tests import helpers

    pool = helpers.random_amplicon_reads(rng, None, amplicons, min(n, 3000), **kw)
    for k, r in enumerate(pool):
        r.setdefault("name", f"f{k}")
    if n <= len(pool):
        return pool
    return [pool[int(i)] for i in np.sort(rng.integers(0, len(pool), size=n))]


FUZZ_SIZES = (1, 2, 3, 17, 64, 255, 256, 257, 300, 777, 1000, 1500, 2048, 3000, 4097, 6000, 8000, 12000, 16385, 20000, 30000, 50000)


def fuzz_cases(max_reads=None):
    """seeded random streams that mix everything above, on panels several windows wide; max_reads cuts every stream"""
    W = geometry().window
    out = []
    for seed, n in enumerate(FUZZ_SIZES):
        rng = np.random.default_rng(9000 + seed)
        n_amp = int(rng.integers(12, 40))
        amps, pairs = [], []
        for a in range(n_amp):
            ref_id = a * 3 // n_amp
            start = 500 + 150 * a + int(rng.integers(0, 40))
            amps.append((ref_id, start, start + 130))
            pairs += [(ref_id, p) for p in range(start - 10, start + 160)]
        keys = make_keys(pairs)
        style = seed % 4
        if style == 1:
            keys = keys[rng.random(len(keys)) < 0.5]
        elif style == 2:
            keys = keys[::2]
        elif style == 3:
            keys = np.delete(keys, rng.integers(0, len(keys), size=len(keys) // 25))
        assert len(keys) > 2 * W
        shape = dict(read_len=(120, 320), name_len=(1, 40)) if seed % 4 == 3 else dict(read_len=(20, 40), name_len=(1, 200)) if seed % 5 == 0 else \
            dict(read_len=(20, 90), name_len=(1, 30))  # long reads leave the stage; short ones with every name length stay in it
        reads = fuzz_reads(rng, n if max_reads is None else min(n, max_reads), amps, odd_ops=0.2, unplaced=0.02, **shape)
        if seed % 7 == 3:
            reads = [reads[i] for i in rng.permutation(len(reads))]
        gaps = {int(k): int(rng.integers(1, 70)) for k in rng.integers(0, len(reads), size=min(len(reads), 20))}
        src = build_stream(reads, lead=int(rng.integers(0, 40)), gaps=gaps, trail=int(rng.integers(16, 64)))
        out.append(Case(f"fuzz_{seed}_{len(reads)}_reads", src, keys, mbq=int(rng.choice([0, 10, 20, 21, 30, 40])), mrq=int(rng.choice([0, 5, 20, 21, 40, 60])), reads=reads))
    return out


@functools.lru_cache(None)
def cases():
    """the whole table: deterministic cases, the depth case, the fuzz streams"""
    return deterministic_cases() + (depth_case(),) + tuple(fuzz_cases())


# ---------------------------------------------------------------------------------------------------------------------------
# the table on a device
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A
STATS_BASE = (1000, 2000)


def base_pattern(P):
    """the non-zero values the counts buffer holds before the call"""
    return (np.arange(P * 8, dtype=np.int64) % 97 + 1).reshape(P, 8)


class DeviceBuffers:
    """what one or more calls of ampli_pileup_count accumulate into: counts with a guard row on either side, and the stats"""

    def __init__(self, P):
        import torch

        self.P = P
        host = np.full((P + 2, 8), SENTINEL, np.int32)
        host[1:-1] = base_pattern(P)
        self.counts = torch.from_numpy(host).cuda()
        self.stats = torch.tensor(STATS_BASE, dtype=torch.int64).cuda()

    def call(self, lib, h, case, stats=True, n_reads=None):
        import torch

        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
        bam, off, keys = up(case.buf, np.uint8), up(case.rec_off, np.int64), up(case.keys, np.int64)
        assert bam.data_ptr() % 16 == 0
        rc = lib.ampli_pileup_count(h, bam.data_ptr(), off.data_ptr(), case.n_reads if n_reads is None else n_reads, keys.data_ptr(), self.P, case.mbq, case.mrq,
                                    self.counts.data_ptr() + 32, self.stats.data_ptr() if stats else None)
        rc = rc or lib.ampli_sync(h)
        torch.cuda.synchronize()
        return rc

    def mismatches(self, want_counts, want_kept, want_added, stats=True):
        """[] or what differs from base + want"""
        got = self.counts.cpu().numpy().astype(np.int64)
        st = self.stats.cpu().numpy()
        bad = []
        if not (np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL)):
            bad.append(f"guard rows touched: {got[0].tolist()} {got[-1].tolist()}")
        diff = got[1:-1] - base_pattern(self.P) - want_counts
        if np.any(diff):
            rows = np.flatnonzero(np.any(diff != 0, 1))
            bad.append(f"{len(rows)} of {self.P} positions differ, first at key index {rows[0]}: got - want = {diff[rows[0]].tolist()}")
        want_st = [STATS_BASE[0] + (want_kept if stats else 0), STATS_BASE[1] + (want_added if stats else 0)]
        if st.tolist() != want_st:
            bad.append(f"stats {st.tolist()} != {want_st}")
        return bad


def device_check(lib, h, case):
    """one call of ampli_pileup_count on the case; [] or the mismatches against the reference"""
    d = DeviceBuffers(len(case.keys))
    rc = d.call(lib, h, case)
    if rc != 0:
        return [f"ampli_pileup_count returned {rc}: {lib.ampli_last_error(h).decode()}"]
    return d.mismatches(*case.want())


def _child(lib_path):
    """the table against the library at lib_path, which need export no more than the few symbols bound here"""
    import torch

    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib = C.CDLL(lib_path)
    for name, res, args in (("ampli_ctx_create", C.c_int, [C.c_int, vp, C.POINTER(vp)]), ("ampli_ctx_destroy", None, [vp]), ("ampli_last_error", C.c_char_p, [vp]),
                            ("ampli_sync", C.c_int, [vp]), ("ampli_pileup_count", C.c_int, [vp, vp, vp, i64, vp, i64, i32, i32, vp, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if not torch.cuda.is_available():
        print("CHILD no GPU")
        return 3
    torch.cuda.set_device(0)
    h = vp()
    rc = lib.ampli_ctx_create(0, vp(torch.cuda.current_stream().cuda_stream), C.byref(h))
    if rc != 0:
        print(f"CHILD ampli_ctx_create returned {rc}")
        return 3
    bad = 0
    for case in cases():
        found = device_check(lib, h, case)
        print(f"CASE {case.name} {'ok' if not found else 'MISMATCH ' + '; '.join(found)}", flush=True)
        bad += bool(found)
    lib.ampli_ctx_destroy(h)
    print(f"CHILD done: {len(cases())} cases, {bad} with mismatches", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child", "usage: python -m tests.pileup_model --child <library>"
    sys.exit(_child(sys.argv[2]))
