"""Detection-limit pass (limit_pairs_kernel) against poisson_call on the same resident tumour records.

Config 3's tumour shape by default: 96 synthetic tumours x 100 000 positions, uint16 records, thresholds from the configuration's 256
synthetic normals.  Every repetition is cold (256 MiB written in between), bracketed by HIP events, the three kinds alternated in one
process: the limits, poisson_call in the all-scores mode (every live pair scored once) and in the prefilter mode.  Also reports the
mean and the largest number of scorer evaluations per searched strand (the kernel's own counters) and the yardstick of the operation
count: all-scores time x mean evaluations x 1.25.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 0xA3F15017 + 2  # bench.py's config 3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--T", type=int, default=96)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import LIMIT_RECHECK, POISSON_FULL, POISSON_PREFILTER

    ctx = Context(0)
    P, S, T = a.P, a.S, a.T
    levels = (0.002, 0.005, 0.01)
    ref = ctx.synth_ref(P, seed=SEED)
    ctx.set_record_layout("u16")
    normals, fits = ctx.pack(ctx.synth_fill(P, S, seed=SEED), "u16")
    assert fits
    table = ctx.error_estimate(normals, P, 0.002, 100)
    del normals
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, seed=SEED, tumour=True), "u16")
    assert fits
    rec = ctx.records(tumours, "u16", T)
    cap = 1 << 22
    ctx.limit_stats(reset=True)
    lim = ctx.detection_limits(rec, P, table.thr, ref, 100, levels)
    torch.cuda.synchronize()
    strands, evals, worst = ctx.limit_stats()
    counts = lim["counts"].sum(dim=0).cpu().tolist()
    n_recheck = int((lim["status"] & LIMIT_RECHECK).ne(0).sum().item())
    full = ctx.poisson_call_records(rec, P, table.thr, ref, 100, mode=POISSON_FULL, capacity=cap)
    pre = ctx.poisson_call_records(rec, P, table.thr, ref, 100, mode=POISSON_PREFILTER, capacity=cap)
    torch.cuda.synchronize()
    assert ctx.flags() & 4 == 0
    called = int((lim["status"] & 0x40).ne(0).sum().item())
    assert called == int(sum(bin(int(v)).count("1") * int(c) for v, c in zip(*[x.tolist() for x in torch.unique(pre["call_mask"], return_counts=True)])))

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_lim, t_full, t_pre = [], [], []
    for _ in range(a.reps):
        t_lim.append(timed(lambda: ctx.detection_limits(rec, P, table.thr, ref, 100, levels, counts=lim["counts"])))
        t_full.append(timed(lambda: ctx.poisson_call_records(rec, P, table.thr, ref, 100, mode=POISSON_FULL, capacity=cap, call_mask=full["call_mask"],
                                                             calls_buf=full["calls_buf"], n_calls=full["n_calls"])))
        t_pre.append(timed(lambda: ctx.poisson_call_records(rec, P, table.thr, ref, 100, mode=POISSON_PREFILTER, capacity=cap, call_mask=pre["call_mask"],
                                                            calls_buf=pre["calls_buf"], n_calls=pre["n_calls"])))
    med = statistics.median
    mean_evals = evals / max(1, strands)
    yard = med(t_full) * mean_evals * 1.25
    out_bytes = T * P * 4 * 9
    line = dict(kind="limit_bench", P=P, S=S, T=T, layout="u16", reps=a.reps, levels=list(levels),
                limit_ms=med(t_lim), limit_ms_min=min(t_lim), poisson_full_ms=med(t_full), poisson_full_ms_min=min(t_full),
                poisson_prefilter_ms=med(t_pre), poisson_prefilter_ms_min=min(t_pre),
                strands_searched=strands, evaluations=evals, mean_evaluations_per_strand=mean_evals, max_evaluations_per_strand=worst,
                yardstick_ms=yard, limit_over_yardstick=med(t_lim) / yard, limit_over_poisson_full=med(t_lim) / med(t_full),
                output_bytes=out_bytes, record_bytes=T * P * 16, output_GBps_at_limit_ms=out_bytes / med(t_lim) / 1e6,
                counts=dict(noref_lines=counts[0], ok=counts[1], lowdepth=counts[2], noestimate=counts[3], unreachable=counts[4], recheck=counts[5],
                            min_af_le=counts[6:]), recheck_cells=n_recheck, called_pairs=called)
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
