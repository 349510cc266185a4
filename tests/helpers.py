"""Shared test helpers (host-side synthetic panels through the product's host library)."""
import contextlib
import ctypes as C
import gzip
import os

import numpy as np

from amplisolve_amd import host_lib

SEED = 0xA3F15017

# ---- fixtures under tests/golden/, wherever the checkout lies ----
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIST_AS = "AMPLISOLVE_LIST_DIR_AS"
# The order a directory's files are visited in is the iteration order of a hash map keyed by <directory string>/<file name> (EE:794-841,
# VC:580-627), and the expected outputs under tests/golden/ were generated with the files under another directory string.  What they
# depend on is that ORDER, recorded beside them: per fixture directory (relative to its root), the file that lists it.
ORDER_FILES = {
    "golden": {"toy_subset/NORMAL": "toy_subset/expected_visit_order.txt", "toy_subset/TUMOUR": "vc_ref/toy_subset_TUMOUR.order",
               "mini_edge/NORMAL": "mini_edge/expected_visit_order.txt", "irregular/NORMAL": "irregular/expected_visit_order.txt"},
    "toy_data": {"NORMAL_ASEQ_DIR": "toy/visit_order.txt", "TUMOUR_ASEQ_DIR": "toy/tumour_visit_order.txt"},
}
_ALIASES = {}


def recorded_order(rel, name="golden"):
    """the sample names of fixture directory `rel` in the order the outputs of tests/golden/ were generated with"""
    with open(os.path.join(GOLDEN, ORDER_FILES[name][rel])) as f:
        return [l.split()[0] for l in f if l.strip()]


def recorded(path, root=GOLDEN, name="golden"):
    """a directory string under which the host visits the files of fixture directory `path` (or of a copy of it) in the recorded order
    (`path` itself for a directory that is not a fixture).  Found once per fixture directory among fixed candidate strings, with the
    host's own sample_order as the judge: the key of a file is <string>/<file name> whatever directory the files lie in."""
    from amplisolve_amd.hostio import sample_order

    path = str(path)
    if not path.startswith(str(root) + os.sep):
        return path
    rel = path[len(str(root)) + 1:]
    if (name, rel) not in _ALIASES:
        want = recorded_order(rel, name)
        old = os.environ.get(LIST_AS)
        try:
            for k in range(100000):
                os.environ[LIST_AS] = f"{name}-{k}/{rel}"
                if sample_order(path) == want:
                    _ALIASES[name, rel] = os.environ[LIST_AS]
                    break
            else:
                raise AssertionError(f"no candidate directory string visits {rel} in the order {want}")
        finally:
            if old is None:
                del os.environ[LIST_AS]
            else:
                os.environ[LIST_AS] = old
    return _ALIASES[name, rel]


def listed_as(path, root=GOLDEN, name="golden"):
    """environment that makes the host visit a fixture directory's files in the recorded order (AMPLISOLVE_LIST_DIR_AS)"""
    return {LIST_AS: recorded(path, root, name)}


def cli_env(args, env=None):
    """os.environ for a command line over fixture directories: the recorded order of its germline_dir= / tumour_dir= token (if
    any), then the caller's own variables (which win)"""
    e = dict(os.environ)
    for a in args:
        a = str(a)
        if a.startswith(("germline_dir=", "tumour_dir=")):
            e.update(listed_as(a.split("=", 1)[1]))
    e.update(env or {})
    return e


@contextlib.contextmanager
def listing(path, root=GOLDEN, name="golden"):
    """in-process twin of listed_as: the host library reads AMPLISOLVE_LIST_DIR_AS from this process's environment"""
    alias = listed_as(path, root, name)
    old = os.environ.get(LIST_AS)
    os.environ.update(alias)
    try:
        yield
    finally:
        if old is None:
            del os.environ[LIST_AS]
        else:
            os.environ[LIST_AS] = old


def golden_cohort(bed_or_table, aseq_dir=None, **kw):
    """HostCohort over a fixture directory, its files visited in the recorded order"""
    from amplisolve_amd.hostio import HostCohort

    with listing(aseq_dir or ""):
        return HostCohort(bed_or_table, aseq_dir, **kw)


def toy_data(dst):
    """the reference's Toy_data (panel BED, 5 normal and 3 tumour .PILEUP.ASEQ files), unpacked from tests/golden/toy_data/ into dst;
    list its directories with listed_as(..., root=dst, name="toy_data")"""
    src = os.path.join(GOLDEN, "toy_data")
    for dirpath, _, files in os.walk(src):
        out = os.path.join(str(dst), os.path.relpath(dirpath, src))
        os.makedirs(out, exist_ok=True)
        for f in files:
            with open(os.path.join(out, f[:-3]), "wb") as o:
                o.write(gzip.open(os.path.join(dirpath, f)).read())
    return str(dst)


FENCE_GUARD = 4096  # bytes of guard on either side of a fenced payload
FENCE_ALIGN = 256   # the payload starts where a device allocation would


def fenced(shape, dtype, poison=0xFF, device="cuda"):
    """An output buffer whose prior content exposes a missed or a stray store: ONE uint8 tensor, guard | payload | guard (4096 bytes
    each side, the payload 256-byte aligned and rounded up to 16 bytes), every byte of it `poison`.  Returns the typed payload view
    and check(): both guards (every byte of the tensor outside the payload) still hold the poison, and so does the payload's own
    tail behind the view -- all of it, or all but the first `pad` bytes (check(pad=k): the k bytes a contract lets a call write
    there, such as the call mask's rounding to 4 bytes).  check.raw is the whole tensor, check.repoison() fills it again.
    0xFF is NaN as f32 / f64, -1 as int32, 255 as uint8, and a call-mask byte with four impossible bits.  Outputs only: never
    poison what a kernel reads as an index, a count or a bound."""
    import torch

    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = 1
    for d in shape:
        n *= d
    nbytes = n * torch.empty(0, dtype=dtype).element_size()
    payload = (nbytes + 15) // 16 * 16
    raw = torch.empty(FENCE_GUARD + FENCE_ALIGN + payload + FENCE_GUARD, dtype=torch.uint8, device=device)
    raw.fill_(poison)
    off = FENCE_GUARD + (-(raw.data_ptr() + FENCE_GUARD)) % FENCE_ALIGN
    view = raw[off: off + nbytes].view(dtype).view(*shape)
    assert view.data_ptr() % FENCE_ALIGN == 0 and off >= FENCE_GUARD and raw.numel() - (off + payload) >= FENCE_GUARD

    def check(pad=0):
        lo, hi = raw[:off], raw[off + nbytes + pad:]
        bad_lo, bad_hi = int((lo != poison).sum()), int((hi != poison).sum())
        assert bad_lo == 0, f"{bad_lo} byte(s) written in front of the payload, the nearest {off - int((lo != poison).nonzero().max())} byte(s) before it"
        assert bad_hi == 0, f"{bad_hi} byte(s) written behind the payload, the nearest {int((hi != poison).nonzero().min()) + pad} byte(s) past its end"

    check.raw = raw
    check.repoison = lambda: raw.fill_(poison)
    return view, check


def assert_misaligned_refused(ctx, call, good, shifts, outputs, message=b"bad argument"):
    """`call(*good)` would succeed (ctx.h first, device pointers as integers).  For every (index, bytes) of `shifts` the same call with
    that pointer moved by so many bytes -- below the alignment the contract gives it -- returns AMPLI_E_INVALID (-1) with `message`, and
    afterwards every byte of the fenced `outputs` ((view, check) pairs of fenced(), stats included) and of their guards still holds the
    poison: a refusal launches nothing."""
    import torch

    for at, by in shifts:
        args = list(good)
        assert isinstance(args[at], int) and args[at] % 16 == 0 and 0 < by < 16, at
        args[at] += by
        assert call(*args) == -1, f"argument {at} moved by {by} byte(s) was not refused"
        assert message in ctx.lib.ampli_last_error(ctx.h), ctx.lib.ampli_last_error(ctx.h)
    ctx.sync()
    torch.cuda.synchronize()
    for view, check in outputs:
        assert bool((check.raw == check.raw[0]).all()), "a refused call wrote to an output"
        check()


def synth_recs(P, n, first=0, seed=SEED, depth=2000, tumour=False):
    out = np.empty((n, P, 8), np.int32)
    rc = host_lib().ampli_host_synth_fill(out.ctypes.data_as(C.c_void_p), P, n, first, seed, depth, int(tumour))
    assert rc == 0
    return out


def synth_ref(P, seed=SEED):
    out = np.empty((P,), np.uint8)
    assert host_lib().ampli_host_synth_ref(out.ctypes.data_as(C.c_void_p), P, seed) == 0
    return out


def edge_case_recs(P, S, rng):
    """Random records that hit every branch of the gate: absent cells, FW or BW == 0, depth around the
    coverage cutoff, AF around 5 %, homozygous alts, zero counts."""
    recs = np.zeros((S, P, 8), np.int32)
    depth = rng.choice([0, 1, 50, 99, 100, 101, 200, 1000, 5000, 33395], size=(S, P, 2))
    for st in range(2):
        d = depth[:, :, st]
        frac = rng.choice([0.0, 0.0005, 0.002, 0.01, 0.0499, 0.05, 0.0501, 0.06, 0.3, 0.5, 1.0], size=(S, P, 3))
        alts = np.minimum((d[:, :, None] * frac).astype(np.int64) + rng.integers(0, 2, size=(S, P, 3)), d[:, :, None])
        # make the alts fit: scale down when they exceed the depth
        tot = alts.sum(-1)
        over = tot > d
        alts[over] = 0
        ref = d - alts.sum(-1)
        ref_nt = rng.integers(0, 4, size=(P,))
        for p in range(P):
            order = [nt for nt in range(4) if nt != ref_nt[p]]
            recs[:, p, st * 4 + ref_nt[p]] = ref[:, p]
            for j, nt in enumerate(order):
                recs[:, p, st * 4 + nt] = alts[:, p, j]
    absent = rng.random((S, P)) < 0.1
    recs[absent] = 0
    recs[absent, 0] = np.iinfo(np.int32).min
    return recs


def borderline_triples(want=12, seed=5, gate=5.0, eps=1e-6, errs=(0.000001, 0.000002, 0.000003, 0.000005, 0.000007, 0.000011, 0.000013)):
    """(k, RD, err, Q) with the REFERENCE's Q (the oracle's scorer is bit-identical to it, tests/test_oracle_golden.py) within
    eps of the gate, on both sides of it.  err has at most six decimals so that it survives the error table's "%f"; the fine
    knob is RD: Q falls as RD grows, bisection finds the crossing and its neighbours are kept when they are close enough."""
    from oracle import pyoracle as orc

    L = orc.lib()
    rng = np.random.default_rng(seed)
    out = []
    tries = 0
    while len(out) < want and tries < 4000:
        tries += 1
        err = float(np.float32(rng.choice(errs)))
        k = int(rng.integers(3, 60))
        lo, hi = 100, (1 << 31) - 2  # Q(lo) high (tiny mean), Q(hi) low
        if not (float(L.oracle_score(k, lo, err)) >= gate > float(L.oracle_score(k, hi, err))):
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if float(L.oracle_score(k, mid, err)) >= gate:
                lo = mid
            else:
                hi = mid
        for rd in (lo - 1, lo, hi, hi + 1):
            q = float(L.oracle_score(k, rd, err))
            if abs(q - gate) <= eps and (k, rd, err) not in [(a, b, c) for a, b, c, _ in out]:
                out.append((k, rd, err, q))
    return out


# ---- BAM files for the pileup step (computeCounts): a minimal writer, BGZF framing included ----
def write_bam(path, refs, reads, rng=None, max_block=60000, level=6, corrupt_block_size=None):
    """refs: [(name, length)]; reads: dicts with ref_id, pos (0-based), mapq, flag, cigar [(op char, len)], seq (str), qual (list),
    optional name.  The stream is cut into BGZF blocks of random sizes (records span block boundaries).
    corrupt_block_size = (k, value): record k is written with that block_size instead of its length (a corrupt file)."""
    import struct
    import zlib

    ops = "MIDNSHP=X"
    codes = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    text = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(f"@SQ\tSN:{n}\tLN:{l}\n".encode() for n, l in refs)
    raw = bytearray(b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)))
    for n, l in refs:
        raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    for k, r in enumerate(reads):
        name = (r.get("name") or f"r{k}").encode() + b"\0"
        seq = r["seq"]
        packed = bytearray((len(seq) + 1) // 2)
        for i, c in enumerate(seq):
            packed[i >> 1] |= codes[c] << (4 if i % 2 == 0 else 0)
        cig = b"".join(struct.pack("<I", (n << 4) | ops.index(op)) for op, n in r["cigar"])
        body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(seq), -1, -1, 0)
        body += name + cig + bytes(packed) + bytes(r["qual"])
        raw += struct.pack("<I", corrupt_block_size[1] if corrupt_block_size and corrupt_block_size[0] == k else len(body)) + body
    out = bytearray()
    o = 0
    while o < len(raw):
        n = min(len(raw) - o, int(rng.integers(1, max_block)) if rng is not None else max_block)
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        data = co.compress(bytes(raw[o:o + n])) + co.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(data) + 25) + data
        out += struct.pack("<II", zlib.crc32(bytes(raw[o:o + n])) & 0xffffffff, n)
        o += n
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")  # the EOF marker block
    open(path, "wb").write(bytes(out))
    return len(raw)


def random_amplicon_reads(rng, refs, amplicons, n_reads, read_len=(60, 140), name_len=None, odd_ops=0.0, unplaced=0.0):
    """Reads in the style of amplicon sequencing: every read of an amplicon starts near its start; soft clips, insertions,
    deletions, reverse strands, filtered flags, low qualities and N bases are all drawn.  Drawn only when asked for (the defaults
    leave the stream of random numbers as it was): name_len = (lo, hi): read names of lo..hi bytes, the NUL included; odd_ops: the
    share of reads that also get padding, zero-length operations and a leading hard clip; unplaced: the share of reads with pos -1."""
    reads = []
    for _ in range(n_reads):
        ref_id, start, end = amplicons[int(rng.integers(len(amplicons)))]
        pos = max(0, start - 1 + int(rng.integers(-5, 6)))
        target = int(rng.integers(*read_len))
        cigar, used = [], 0
        if rng.random() < 0.3:
            cigar.append(("S", int(rng.integers(1, 8))))
        while used < target:
            n = int(rng.integers(5, 60))
            cigar.append(("M" if rng.random() < 0.9 else ("=" if rng.random() < 0.5 else "X"), n))
            used += n
            u = rng.random()
            if u < 0.10:
                cigar.append(("I", int(rng.integers(1, 4))))
            elif u < 0.20:
                cigar.append(("D", int(rng.integers(1, 6))))
            elif u < 0.23:
                cigar.append(("N", int(rng.integers(10, 40))))
        if cigar[-1][0] in "IDN":
            cigar.append(("M", 3))
        if rng.random() < 0.3:
            cigar.append(("S", int(rng.integers(1, 8))))
        if rng.random() < 0.1:
            cigar.append(("H", 5))
        if odd_ops and rng.random() < odd_ops:
            at = int(rng.integers(1, len(cigar) + 1))
            cigar[at:at] = [("P", int(rng.integers(0, 4))), ("MIDNSHP=X"[int(rng.integers(9))], 0)]
            if cigar[0][0] != "H" and rng.random() < 0.5:
                cigar.insert(0, ("H", int(rng.integers(0, 9))))
        qlen = sum(n for op, n in cigar if op in "MIS=X")
        seq = "".join(rng.choice(list("ACGT"), size=qlen))
        if rng.random() < 0.2:
            i = int(rng.integers(qlen))
            seq = seq[:i] + rng.choice(["N", "R", "M"]) + seq[i + 1:]
        flag = 0x10 if rng.random() < 0.5 else 0
        for bit, pr in ((0x4, 0.02), (0x100, 0.03), (0x200, 0.02), (0x400, 0.05), (0x800, 0.03), (0x1, 0.3)):
            if rng.random() < pr:
                flag |= bit
        reads.append(dict(ref_id=ref_id if rng.random() > 0.01 else -1, pos=pos, mapq=int(rng.choice([0, 5, 19, 20, 21, 40, 60])), flag=flag, cigar=cigar, seq=seq,
                          qual=[int(x) for x in rng.choice([2, 10, 19, 20, 21, 30, 40], size=qlen)]))
        if name_len:
            reads[-1]["name"] = "q" * (int(rng.integers(name_len[0], name_len[1] + 1)) - 1)
        if unplaced and rng.random() < unplaced:
            reads[-1]["pos"] = -1
    reads.sort(key=lambda r: (r["ref_id"] if r["ref_id"] >= 0 else 1 << 30, r["pos"]))
    return reads


def write_fresh_panel(d, seed, depth=None, S=11, amplicons=7):
    """A freshly drawn panel in directory d (pathlib): p.bed (every second amplicon overlaps its predecessor by 25 positions ->
    positions listed twice), r.txt (reference bases), d.txt (duplicated positions), N/S??.PILEUP.ASEQ (absent lines, heterozygous
    sites, low-coverage cells from the synthetic generator).  Returns the number of duplicated positions."""
    import numpy as np

    rng = np.random.default_rng(seed)
    chroms = ["chr1", "chr2", "chr7", "chrX"]
    rows, walk = [], []
    for i in range(amplicons):
        c = chroms[i % len(chroms)]
        start = 100_000 + (i // len(chroms)) * 50_000
        if i % 2 == 1:
            c, start = rows[-1][0], rows[-1][2] - 24
        n = int(rng.integers(150, 260))
        rows.append((c, start, start + n - 1))
        walk += [(c, start + j) for j in range(n)]
    W = len(walk)
    recs = synth_recs(W, S, seed=seed, depth=int(rng.choice([400, 2000, 6000])) if depth is None else depth)
    uniq = {}
    for k in walk:
        uniq.setdefault(k, len(uniq))
    refb = synth_ref(len(uniq), seed=seed)
    (d / "N").mkdir()
    with open(d / "p.bed", "w") as f:
        f.write("".join(f"{c}\t{a}\t{b}\tAMPL{i}\trs{i}\tGENE{i}\n" for i, (c, a, b) in enumerate(rows)))
    seen, dups = set(), []
    with open(d / "r.txt", "w") as f:
        for k in walk:
            f.write(f"{k[0]}\t{k[1]}\t{'ACGT'[refb[uniq[k]]]}\n")
            if k in seen and k not in dups:
                dups.append(k)
            seen.add(k)
    with open(d / "d.txt", "w") as f:
        f.write("".join(f"{c}\t{p}\n" for c, p in sorted(dups)))
    for s_ in range(S):
        r = recs[s_].astype(np.int64)
        with open(d / "N" / f"S{s_:02d}.PILEUP.ASEQ", "w") as f:
            f.write("chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n")
            for w, (c, p) in enumerate(walk):
                if r[w, 0] == np.iinfo(np.int32).min:
                    continue  # the sample has no line for this amplicon position
                tot = r[w, :4] + r[w, 4:]
                f.write(f"{c}\t{p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[w,4]}\t{r[w,5]}\t{r[w,6]}\t{r[w,7]}\n")
    return len(dups)


def write_fresh_tumours(d, seed, T=4, depth=None, spike=0.06, sub="T"):
    """Tumour ASEQ files d/<sub>/*.PILEUP.ASEQ for the panel write_fresh_panel put in d (the BED walk, so positions of overlapping
    amplicons are listed twice per file): the synthetic generator's tumour family plus, in `spike` of the cells, an alternative allele
    moved onto both strands at 0.3-40 % (so that a small panel emits hundreds of calls of every tier: few reads, LowQ, strand-skewed
    ones).  File names of both shapes the reference's `%[^_]_%[^_]` split sees (VC:701).  Returns the number of lines written."""
    import numpy as np

    rng = np.random.default_rng(seed ^ 0x7A11)
    walk = []
    for row in (d / "p.bed").read_text().splitlines():
        c, a, b = row.split("\t")[:3]
        walk += [(c, x) for x in range(int(a), int(b) + 1)]
    W = len(walk)
    recs = synth_recs(W, T, seed=seed, depth=int(rng.choice([400, 2000, 6000])) if depth is None else depth, tumour=True).astype(np.int64)
    # the major allele of every line = the panel's reference base of that walk row (write_fresh_panel draws the bases per unique
    # position, the records per walk row: without this every position behind the first overlap would be a 100 % variant)
    refrow = [l.split("\t")[2] for l in (d / "r.txt").read_text().splitlines()]
    for w in range(W):
        b = "ACGT".find(refrow[w])
        if b >= 0:
            for t in range(T):
                m = int(np.argmax(recs[t, w, :4] + recs[t, w, 4:]))
                if m != b and recs[t, w, 0] != np.iinfo(np.int32).min:
                    recs[t, w, [m, b]] = recs[t, w, [b, m]]
                    recs[t, w, [4 + m, 4 + b]] = recs[t, w, [4 + b, 4 + m]]
    (d / sub).mkdir()
    n = 0
    for t in range(T):
        r = recs[t]
        name = f"P{t:02d}_T{t}_x" if t % 2 else f"K{t:02d}"
        with open(d / sub / f"{name}.PILEUP.ASEQ", "w") as f:
            f.write("chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n")
            for w, (c, x) in enumerate(walk):
                if r[w, 0] == np.iinfo(np.int32).min:
                    continue
                rec = r[w].copy()
                if rng.random() < spike:
                    major, alt = int(np.argmax(rec[:4] + rec[4:])), int(rng.integers(0, 4))
                    share = float(rng.choice([0.002, 0.003, 0.004, 0.006, 0.01, 0.02, 0.05, 0.2, 0.4]))
                    for st, skew in ((0, 1.0), (4, float(rng.choice([1.0, 1.0, 0.3, 2.5])))):
                        k = min(int(rec[st + major]), int(round(rec[st + major] * share * skew)) + int(rng.integers(0, 3)))
                        if alt != major:
                            rec[st + major] -= k
                            rec[st + alt] += k
                tot = rec[:4] + rec[4:]
                f.write(f"{c}\t{x}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{rec[4]}\t{rec[5]}\t{rec[6]}\t{rec[7]}\n")
                n += 1
    return n


def write_envelope_panel(d, seed, S=9, n=120, twice=True):
    """a panel whose threshold sums are NOT order-free at coverage_cutoff = 1: a few reads deep lines (tiny fp32 products with low bits)
    among lines tens of millions deep with alternative counts just under 5 % (sums beyond 2^53 ulps of the tiny addends)"""
    import numpy as np

    rng = np.random.default_rng(seed)
    walk = [("chr1", 1000 + i) for i in range(n)]
    if twice:
        walk += [("chr1", 1000 + i) for i in range(n - 20, n)]  # the last 20 positions listed twice
    (d / "N").mkdir()
    (d / "p.bed").write_text(f"chr1\t1000\t{1000 + n - 1}\ta\tb\tc\n" + (f"chr1\t{1000 + n - 20}\t{1000 + n - 1}\ta2\tb2\tc2\n" if twice else ""))
    (d / "r.txt").write_text("".join(f"{c}\t{x}\tA\n" for c, x in walk))
    (d / "d.txt").write_text("".join(f"chr1\t{1000 + i}\n" for i in range(n - 20, n)) if twice else "")
    for s in range(S):
        with open(d / "N" / f"E{s:02d}.PILEUP.ASEQ", "w") as f:
            f.write("chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n")
            for c, x in walk:
                if rng.random() < 0.05:
                    continue
                if rng.random() < 0.35:
                    fw, bw = int(rng.integers(1, 9)), int(rng.integers(1, 9))          # a few reads
                    alt = [0, 0, 0]
                    altr = [0, 0, 0]
                else:
                    fw, bw = int(rng.integers(20_000_000, 45_000_000)), int(rng.integers(20_000_000, 45_000_000))
                    alt = [int(fw * rng.uniform(0.0, 0.0499)) for _ in range(3)]
                    altr = [int(bw * rng.uniform(0.0, 0.0499)) for _ in range(3)]
                a_f, a_r = fw - sum(alt), bw - sum(altr)
                tot = [a_f + a_r] + [alt[i] + altr[i] for i in range(3)]
                f.write(f"{c}\t{x}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{sum(tot)}\t{a_r}\t{altr[0]}\t{altr[1]}\t{altr[2]}\n")
