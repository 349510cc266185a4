"""The indel counting kernel beside the pileup counting kernel on the same stream of alignment records.

The stream is tools/pileup_bench.py's: 2 M reads of 120 bases on 400 amplicons of one chromosome, every read of an amplicon starting at
its start, one `120M` operation per read, qualities 15 .. 40, both strands (same generator, same seed).  Three kinds of call, alternated in
one process, each repetition bracketed by HIP events after a warm-up of every kind:
  * ampli_pileup_indel_count with the length plane,
  * ampli_pileup_indel_count without it (d_lengths = NULL),
  * ampli_pileup_count: the yardstick -- the same bytes read, a base extracted per column on top.
--indels F gives that share of the reads `60M2I58M` / `60M3D60M` instead (records of another length; off by default, so that the default
is the yardstick's own stream).  The counts are checked against what the stream holds (computed here from the qualities) before anything
is timed.  Reported: milliseconds (median, min, max, all), the two ratios over the yardstick with the spread of each kind, and GB/s of
algorithmic bytes (the records once, 8 bytes of offset per read).  No time is fixed in advance.  One JSON line on stdout; --out also
writes it.  Not a replacement for bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def records(np, rng, n, L, cigar, amp_pos, flags):
    """n records of one CIGAR (a list of (op code, length)) as a structured array, block_size included"""
    q = sum(k for o, k in cigar if o in (0, 1))
    name = b"r\0"
    rec_len = 32 + len(name) + 4 * len(cigar) + (q + 1) // 2 + q
    dt = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"),
                   ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "S2"), ("cig", "<u4", (len(cigar),)), ("seq", "u1", ((q + 1) // 2,)), ("qual", "u1", (q,))])
    assert dt.itemsize == rec_len + 4
    a = np.zeros(n, dt)
    a["bs"], a["ref"], a["pos"], a["lname"], a["mapq"], a["bin"], a["ncig"] = rec_len, 0, amp_pos, len(name), 60, 4680, len(cigar)
    a["flag"], a["lseq"], a["nref"], a["npos"], a["name"] = flags, q, -1, -1, name
    a["cig"] = np.asarray([(k << 4) | o for o, k in cigar], np.uint32)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n, 2 * ((q + 1) // 2)))]
    a["seq"] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    a["qual"] = rng.integers(15, 41, (n, q)).astype(np.uint8)
    return a


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=120)
    ap.add_argument("--indels", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    N, L = a.reads, a.read_len
    rng = np.random.default_rng(1)
    n_amp = 400
    amp_start = 10_000 + np.arange(n_amp) * 2_000
    amp = np.sort(rng.integers(0, n_amp, N))
    flags = (rng.integers(0, 2, N) * 0x10).astype(np.uint16)
    plain = records(np, rng, N, L, [(0, L)], amp_start[amp] - 1, flags)
    want_ref = int((plain["qual"][:, :L - 1] >= 20).sum())
    want_ins = want_del = 0
    if a.indels > 0:  # a share of the reads, in runs of 64, carries an event: the stream stays sorted, records of three lengths
        runs = (N + 63) // 64
        kind = np.repeat(np.where(rng.random(runs) < a.indels, 1 + rng.integers(0, 2, runs), 0), 64)[:N]
        parts, offs, o = [], np.zeros(N, np.int64), 0
        cut = np.flatnonzero(np.diff(kind)) + 1
        for lo, hi in zip(np.r_[0, cut], np.r_[cut, N]):
            k = int(kind[lo])
            rec = plain[lo:hi] if k == 0 else records(np, rng, hi - lo, L, [(0, L // 2), (1, 2), (0, L - L // 2 - 2)] if k == 1 else [(0, L // 2), (2, 3), (0, L // 2)],
                                                      amp_start[amp[lo:hi]] - 1, flags[lo:hi])
            offs[lo:hi] = o + np.arange(hi - lo, dtype=np.int64) * rec.dtype.itemsize
            o += (hi - lo) * rec.dtype.itemsize
            parts.append(rec.tobytes())
        raw = b"".join(parts)
        want_ref = None  # left to the invariants below
        want_ins, want_del = int((kind == 1).sum()), int((kind == 2).sum())
    else:
        raw = plain.tobytes()
        offs = np.arange(N, dtype=np.int64) * plain.dtype.itemsize
    del plain

    ctx = Context(0)
    d_bam = torch.frombuffer(bytearray(raw + bytes(64)), dtype=torch.uint8).cuda()
    off = torch.from_numpy(offs).cuda()
    keys = torch.from_numpy(np.concatenate([(np.int64(s) + np.arange(L + 8, dtype=np.int64)) for s in amp_start])).cuda()  # ref id 0 << 32 | pos
    P = int(keys.numel())
    counts = torch.zeros((P, 8), dtype=torch.int32, device="cuda")
    lengths = torch.zeros((P, 2, 32), dtype=torch.int32, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    pcounts = torch.zeros((P, 8), dtype=torch.int32, device="cuda")
    pstats = torch.zeros(2, dtype=torch.int64, device="cuda")
    kinds = {"indel_with_lengths": lambda: ctx.indel_count(d_bam, off, keys, 20, 20, counts=counts, lengths=lengths, stats=stats),
             "indel_without_lengths": lambda: ctx.indel_count(d_bam, off, keys, 20, 20, counts=counts, lengths=False, stats=stats),
             "pileup_count": lambda: ctx._check(ctx.lib.ampli_pileup_count(ctx.h, d_bam.data_ptr(), off.data_ptr(), N, keys.data_ptr(), P, 20, 20, pcounts.data_ptr(),
                                                                           pstats.data_ptr()))}
    # one call, checked: what the stream holds
    kinds["indel_with_lengths"]()
    torch.cuda.synchronize()
    c, st = counts.cpu().numpy().astype(np.int64), stats.cpu().tolist()
    assert st[0] == N and st[1] == c[:, :3].sum() and not c[:, 3].any() and not c[:, 7].any(), st
    assert a.indels > 0 or (c[:, 1].sum(), c[:, 2].sum()) == (0, 0)
    assert want_ref is None or c[:, 0].sum() == want_ref, (int(c[:, 0].sum()), want_ref)
    assert np.array_equal(lengths.cpu().numpy().sum(2), c[:, 1:3])
    if a.indels > 0:  # anchors with quality < 20 are not counted: at most the planted events, and most of them
        assert 0.5 * want_ins <= c[:, 1].sum() <= want_ins and 0.5 * want_del <= c[:, 2].sum() <= want_del
    junctions = st[1]
    for _ in range(a.warmup):
        for fn in kinds.values():
            fn()
    torch.cuda.synchronize()
    t0, t1 = ctx.event(), ctx.event()
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            ctx.record(t0)
            fn()
            ctx.record(t1)
            times[k].append(ctx.elapsed_ms(t0, t1))
    med = statistics.median
    b = len(raw) + 8 * N
    line = dict(kind="indel_bench", reads=N, read_len=L, amplicons=n_amp, positions=P, indel_share=a.indels, record_bytes=len(raw), algorithmic_bytes=b, reps=a.reps,
                warmup=a.warmup, device=torch.cuda.get_device_properties(0).name, junctions_per_call=junctions, insertions_per_call=int(c[:, 1].sum()),
                deletions_per_call=int(c[:, 2].sum()))
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
        line[k + "_GBps"] = b / (med(v) * 1e-3) / 1e9
        line[k + "_spread"] = (max(v) - min(v)) / med(v)
    for k in ("indel_with_lengths", "indel_without_lengths"):
        line[f"ratio_{k}_over_pileup_count"] = med(times[k]) / med(times["pileup_count"])
        line[f"ratio_{k}_over_pileup_count_range"] = [min(times[k]) / max(times["pileup_count"]), max(times[k]) / min(times["pileup_count"])]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
