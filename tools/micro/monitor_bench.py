"""The two gathers of tumour-informed monitoring beside the parent's gather of the same form.

Config 3's shape by default: 352 samples (256 synthetic normals and 96 tumours, uint16 records) over 100 000 positions, 1000 lists of 32
cells drawn over the panel, thresholds from the normals' own error table.  Every repetition is cold for the caches (256 MiB written in
between), bracketed by HIP events, the kinds alternated in one process:
  * ampli_monitor_sums_records: every (sample, list);
  * ampli_amplicon_depth_records over the SAME CSR of positions -- the parent's kernel of the same form (a wave per list and strip of rows,
    entries in registers, one shuffle reduction per cell): the yardstick.  It decodes the same records and stores four sums where the
    monitoring kernel stores six and two doubles, picks no base and forms no products;
  * ampli_monitor_control_records: 96 (row, list) pairs x 1000 replicates, a wave per (pair, replicate), every entry a Philox draw and a
    dependent chain of three loads (candidate, thresholds, record).
Reported: milliseconds, the ratio, and the bytes the definition moves (records gathered + outputs stored; the lists, thresholds and
reference bases are a few hundred KB and stay in L2).  No time is fixed in advance.  One JSON line on stdout; --out also writes it.
Not a replacement for bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--normals", type=int, default=256)
    ap.add_argument("--tumours", type=int, default=96)
    ap.add_argument("--lists", type=int, default=1000)
    ap.add_argument("--entries", type=int, default=32)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P, N, T, L, E, R = a.P, a.normals, a.tumours, a.lists, a.entries, a.replicates
    n = N + T
    n32 = ctx.synth_fill(P, N)
    acc = ctx.error_reduce(n32, P, 0.002, 100)
    thr = ctx.error_finalize(acc, 0.002, 100).thr.contiguous()
    all32 = torch.cat([n32, ctx.synth_fill(P, T, tumour=True)], 0).contiguous()
    recs, fits = ctx.pack(all32, "u16")
    assert fits
    del n32, all32
    ref = ctx.synth_ref(P)
    rec = ctx.records(recs, "u16", n)

    rng = np.random.default_rng(24)
    ref_h = ref.cpu().numpy()
    pos = rng.integers(0, P, L * E)
    base = (ref_h[pos].astype(np.int64) + rng.integers(1, 4, L * E)) & 3  # never the reference base
    off = (np.arange(L + 1) * E).astype(np.int32)
    d_off = torch.from_numpy(off).to(ctx.device)
    d_cell = torch.from_numpy((4 * pos + base).astype(np.int32)).to(ctx.device)
    d_pos = torch.from_numpy(pos.astype(np.int32)).to(ctx.device)
    parts = [np.nonzero(ref_h == g)[0] for g in range(4)]
    cand_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)).to(ctx.device)
    cand_pos = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(ctx.device)
    pairs = torch.stack([torch.arange(N, n, dtype=torch.int32), torch.arange(T, dtype=torch.int32) % L], dim=1).contiguous().to(ctx.device)

    sums, lam = ctx.monitor_sums(rec, P, thr, ref, d_off, d_cell)
    depth = ctx.amplicon_depth(rec, P, d_off, d_pos)
    csums, clam = ctx.monitor_controls(rec, P, thr, ref, d_off, d_cell, pairs, cand_off, cand_pos, R, seed=24)
    torch.cuda.synchronize()
    evaluated = int(sums[:, :, 0].sum().item())

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {"monitor_sums": lambda: ctx.monitor_sums(rec, P, thr, ref, d_off, d_cell, sums=sums, lam=lam),
             "amplicon_depth": lambda: ctx.amplicon_depth(rec, P, d_off, d_pos, out=depth),
             "monitor_controls": lambda: ctx.monitor_controls(rec, P, thr, ref, d_off, d_cell, pairs, cand_off, cand_pos, R, seed=24, sums=csums, lam=clam)}
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    gathered = n * L * E * 16
    line = dict(kind="monitor_bench", P=P, samples=n, lists=L, entries=E, pairs=T, replicates=R, layout="u16", reps=a.reps,
                device=torch.cuda.get_device_properties(0).name, evaluated_entries=evaluated, entries_total=n * L * E,
                monitor_sums_bytes=gathered + n * L * 64, amplicon_depth_bytes=gathered + n * L * 32, monitor_controls_bytes=T * R * E * 16 + T * R * 64)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
        line[k + "_GBps"] = line[k + "_bytes"] / (med(v) * 1e-3) / 1e9
    line["ratio_monitor_sums_over_amplicon_depth"] = med(times["monitor_sums"]) / med(times["amplicon_depth"])
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
