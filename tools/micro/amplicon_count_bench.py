"""The amplicon counting kernel beside the pileup counting kernel on the same stream of alignment records.

The stream is tools/pileup_bench.py's: 2 M reads of 120 bases on 400 amplicons of one chromosome, every read of an amplicon starting at
its start, one `120M` operation per read, qualities 15 .. 40, both strands (same generator, same seed).  Two kinds of call, alternated in
one process, each repetition bracketed by HIP events after a warm-up of both:
  * ampli_pileup_amplicon_count: the assignment per read, then the columns without a key search,
  * ampli_pileup_count: the yardstick -- the same bytes read, a key search per run on top.
--overlap gives the second stream: every second amplicon overlaps its predecessor by 25 positions and 5 % of the reads lie 1000
positions behind their amplicon, off-target.  The counts are checked against what the stream holds (computed here from the qualities)
before anything is timed; on the first stream the two kernels must count the same bases.  Reported: milliseconds (median, min, max, all),
the spread of each kind, the ratio over the yardstick and GB/s of algorithmic bytes (the records once, 8 bytes of offset per read).  No
time is fixed in advance.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.micro.indel_bench import records  # noqa: E402  (the record generator of the three benches of the BAM walks)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=120)
    ap.add_argument("--overlap", action="store_true")
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
    amp_len = L + 8
    amp_start = 10_000 + np.arange(n_amp) * 2_000
    if a.overlap:  # every second amplicon starts 25 positions in front of its predecessor's end
        amp_start[1::2] = amp_start[0::2] + amp_len - 25
    amp = np.sort(rng.integers(0, n_amp, N))
    flags = (rng.integers(0, 2, N) * 0x10).astype(np.uint16)
    off_target = rng.random(N) < 0.05 if a.overlap else np.zeros(N, bool)
    pos = amp_start[amp] - 1 + np.where(off_target, 1000, 0)
    order = np.argsort(pos, kind="stable")  # the stream stays sorted
    pos, flags, off_target = pos[order], flags[order], off_target[order]
    plain = records(np, rng, N, L, [(0, L)], pos, flags)
    want_bases = int((plain["qual"][~off_target] >= 20).sum())
    raw = plain.tobytes()
    offs = np.arange(N, dtype=np.int64) * plain.dtype.itemsize
    del plain

    ctx = Context(0)
    d_bam = torch.frombuffer(bytearray(raw + bytes(64)), dtype=torch.uint8).cuda()
    off = torch.from_numpy(offs).cuda()
    # the amplicons, sorted (they are): ref id 0 << 32 | position
    lo = torch.from_numpy(amp_start.astype(np.int64)).cuda()
    hi = torch.from_numpy((amp_start + amp_len - 1).astype(np.int64)).cuda()
    reach = torch.from_numpy(np.maximum.accumulate(amp_start + amp_len - 1).astype(np.int64)).cuda()
    amp_off = torch.from_numpy((np.arange(n_amp + 1, dtype=np.int64) * amp_len)).cuda()
    W = n_amp * amp_len
    keys = torch.from_numpy(np.unique(np.concatenate([(np.int64(s) + np.arange(amp_len, dtype=np.int64)) for s in amp_start]))).cuda()
    P = int(keys.numel())
    counts = torch.zeros((W, 8), dtype=torch.int32, device="cuda")
    amp_reads = torch.zeros((n_amp, 2), dtype=torch.int64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    pcounts = torch.zeros((P, 8), dtype=torch.int32, device="cuda")
    pstats = torch.zeros(2, dtype=torch.int64, device="cuda")
    kinds = {"amplicon_count": lambda: ctx.amplicon_count(d_bam, off, lo, hi, reach, amp_off, 20, 20, 50, counts=counts, amp_reads=amp_reads, stats=stats),
             "pileup_count": lambda: ctx._check(ctx.lib.ampli_pileup_count(ctx.h, d_bam.data_ptr(), off.data_ptr(), N, keys.data_ptr(), P, 20, 20, pcounts.data_ptr(),
                                                                           pstats.data_ptr()))}
    # one call of each, checked: what the stream holds
    for fn in kinds.values():
        fn()
    torch.cuda.synchronize()
    st, pst = stats.cpu().tolist(), pstats.cpu().tolist()
    n_off = int(off_target.sum())
    assert st == [N, N - n_off, want_bases, 0], (st, N - n_off, want_bases)
    assert int(counts[:, :4].sum()) == want_bases and int(amp_reads.sum()) == N - n_off
    assert a.overlap or (pst[1] == want_bases and int(pcounts.sum()) == int(counts.sum()))
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
    line = dict(kind="amplicon_count_bench", stream="overlap_25_off_target_5pct" if a.overlap else "pileup_bench", reads=N, read_len=L, amplicons=n_amp, walk_entries=W,
                positions=P, off_target_reads=n_off, record_bytes=len(raw), algorithmic_bytes=b, reps=a.reps, warmup=a.warmup,
                device=torch.cuda.get_device_properties(0).name, bases_per_call=want_bases)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
        line[k + "_GBps"] = b / (med(v) * 1e-3) / 1e9
        line[k + "_spread"] = (max(v) - min(v)) / med(v)
    line["ratio_amplicon_count_over_pileup_count"] = med(times["amplicon_count"]) / med(times["pileup_count"])
    line["amplicon_count_minus_pileup_count_ms"] = med(times["amplicon_count"]) - med(times["pileup_count"])
    line["pileup_count_spread_ms"] = max(times["pileup_count"]) - min(times["pileup_count"])
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
