"""The read-evidence counting kernel beside the pileup counting kernel on the same stream of alignment records.

The stream is tools/pileup_bench.py's and tools/micro/indel_bench.py's: 2 M reads of 120 bases on 400 amplicons of one chromosome, every
read of an amplicon starting at its start, one `120M` operation per read, qualities 15 .. 40, both strands (same generator, same seed).
Kinds of call, alternated in one process, each repetition bracketed by HIP events after a warm-up of every kind:
  * evidence_sparse: ampli_pileup_evidence on a call list, one listed position per amplicon (the intended input: the LDS window);
  * evidence_dense:  ampli_pileup_evidence on every panel position (the global-atomic path: expected to be slow);
  * pileup_count:    the yardstick, ampli_pileup_count on the same records and every panel position (what computeCounts runs);
  * pileup_sparse:   ampli_pileup_count on the sparse list, for reference.
Then, in the same process, the stream of --identical identical reads over one listed key (every column in one bin of every metric):
evidence_identical beside pileup_identical.  The histograms are checked against the pileup counts (the invariant of DESIGN 29.1) before
anything is timed.  Reported: milliseconds (median, min, max, all), the spread of each kind, and the ratios over the yardstick.  No time
is fixed in advance.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from indel_bench import records  # noqa: E402  (the generator of the shared stream)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=120)
    ap.add_argument("--identical", type=int, default=20_000)
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
    raw = plain.tobytes()
    offs = np.arange(N, dtype=np.int64) * plain.dtype.itemsize
    same = np.repeat(plain[:1], a.identical)
    raw_same = same.tobytes()
    offs_same = np.arange(a.identical, dtype=np.int64) * plain.dtype.itemsize
    key_same = np.asarray([int(plain["pos"][0]) + 1 + L // 2], np.int64)
    del plain, same

    ctx = Context(0)
    up = lambda b: torch.frombuffer(bytearray(b + bytes(64)), dtype=torch.uint8).cuda()  # noqa: E731
    d_bam, off = up(raw), torch.from_numpy(offs).cuda()
    d_same, off_same, k_same = up(raw_same), torch.from_numpy(offs_same).cuda(), torch.from_numpy(key_same).cuda()
    dense = torch.from_numpy(np.concatenate([(np.int64(s) + np.arange(L + 8, dtype=np.int64)) for s in amp_start])).cuda()  # ref id 0 << 32 | pos
    sparse = torch.from_numpy((amp_start + L // 2).astype(np.int64)).cuda()
    zeros = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    h_dense, h_sparse, h_same = zeros(dense.numel(), 4, 3, 64), zeros(sparse.numel(), 4, 3, 64), zeros(1, 4, 3, 64)
    c_dense, c_sparse, c_same = zeros(dense.numel(), 8), zeros(sparse.numel(), 8), zeros(1, 8)
    st = {k: zeros(2, dtype=torch.int64) for k in ("ed", "es", "ei", "pd", "ps", "pi")}

    def pileup(bam, o, keys, counts, stats):
        ctx._check(ctx.lib.ampli_pileup_count(ctx.h, bam.data_ptr(), o.data_ptr(), int(o.numel()), keys.data_ptr(), int(keys.numel()), 20, 20, counts.data_ptr(),
                                              stats.data_ptr()))

    kinds = {"evidence_sparse": lambda: ctx.read_evidence(d_bam, off, sparse, 20, 20, hist=h_sparse, stats=st["es"]),
             "evidence_dense": lambda: ctx.read_evidence(d_bam, off, dense, 20, 20, hist=h_dense, stats=st["ed"]),
             "pileup_count": lambda: pileup(d_bam, off, dense, c_dense, st["pd"]),
             "pileup_sparse": lambda: pileup(d_bam, off, sparse, c_sparse, st["ps"])}
    kinds_same = {"evidence_identical": lambda: ctx.read_evidence(d_same, off_same, k_same, 20, 20, hist=h_same, stats=st["ei"]),
                  "pileup_identical": lambda: pileup(d_same, off_same, k_same, c_same, st["pi"])}
    # one call of each, checked: per position, nt and metric the bins sum to the pileup count
    for fn in list(kinds.values()) + list(kinds_same.values()):
        fn()
    torch.cuda.synchronize()
    columns = {}
    for name, h, c, s_e, s_p in (("dense", h_dense, c_dense, "ed", "pd"), ("sparse", h_sparse, c_sparse, "es", "ps"), ("identical", h_same, c_same, "ei", "pi")):
        hs = h.sum(3, dtype=torch.int64)
        for m in range(3):
            assert torch.equal(hs[:, :, m], c[:, :4].to(torch.int64)), (name, m)
        assert st[s_e].tolist() == st[s_p].tolist() and st[s_e].tolist()[1] == int(c[:, :4].sum()), (name, st[s_e].tolist(), st[s_p].tolist())
        columns[name] = st[s_e].tolist()[1]
    assert st["ed"].tolist()[0] == N and st["ei"].tolist()[0] == a.identical

    t0, t1 = ctx.event(), ctx.event()
    times = {}
    for group in (kinds, kinds_same):
        for _ in range(a.warmup):
            for fn in group.values():
                fn()
        torch.cuda.synchronize()
        for k in group:
            times[k] = []
        for _ in range(a.reps):
            for k, fn in group.items():
                ctx.record(t0)
                fn()
                ctx.record(t1)
                times[k].append(ctx.elapsed_ms(t0, t1))
    med = statistics.median
    line = dict(kind="evidence_bench", reads=N, read_len=L, amplicons=n_amp, positions_dense=int(dense.numel()), positions_sparse=int(sparse.numel()),
                identical_reads=a.identical, record_bytes=len(raw), reps=a.reps, warmup=a.warmup, device=torch.cuda.get_device_properties(0).name,
                columns_per_call=columns)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
        line[k + "_spread"] = (max(v) - min(v)) / med(v)
    for k, y in (("evidence_sparse", "pileup_count"), ("evidence_sparse", "pileup_sparse"), ("evidence_dense", "pileup_count"), ("evidence_identical", "pileup_identical")):
        line[f"ratio_{k}_over_{y}"] = med(times[k]) / med(times[y])
        line[f"ratio_{k}_over_{y}_range"] = [min(times[k]) / max(times[y]), max(times[k]) / min(times[y])]
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
