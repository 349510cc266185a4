"""The tumour-fraction kernel beside the monitoring gather over the same lists.

Config 3's shape by default: 352 samples (256 synthetic normals and 96 tumours, uint16 records) over 100 000 positions,
1000 lists of 32 cells drawn over the panel, thresholds from the normals' own error table, weights uniform in [0.2, 0.6].  Every
repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated in one process:
  * ampli_fraction_records: every (sample, list): the gather of monitoring, then up to 182 evaluations of the two sums, each a double
    division per cell and a butterfly of two doubles over the wave;
  * ampli_monitor_sums_records over the SAME CSR: the yardstick -- the same gather with one butterfly per (sample, list);
  * ampli_fraction_records once more with the thresholds scaled by --low (0.1): under the table's own thresholds, which lie above the
    synthetic background, nearly every pair is decided by the first rules (F_HAT = 0, F_HI = 0: 2 evaluations); under the scaled ones
    nearly every pair runs all three bisections -- the kernel's full cost, 182 evaluations a pair.
Reported: milliseconds, the ratio, the evaluations the definition makes on this input (counted on the host from the kernel's outputs: 2,
and 60 more for each bisection a pair runs), and the double operations behind them: per evaluation and evaluated cell 7 (multiply, add,
divide, multiply, subtract, add; multiply, add: 8 with the division as one) plus 2 x 6 additions of the butterfly per lane.  No time is
fixed in advance.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py."""
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--low", type=float, default=0.1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import TF_F_HAT, TF_F_HI, TF_F_LO, TF_ITERS, TF_NA, TF_T0, TF_Z2_95

    ctx = Context(0)
    P, N, T, L, E = a.P, a.normals, a.tumours, a.lists, a.entries
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
    d_w = torch.from_numpy(rng.uniform(0.2, 0.6, L * E).astype(np.float32)).to(ctx.device)

    thr_low = torch.where(thr > 0, thr * a.low, thr).contiguous()
    sums, lam = ctx.monitor_sums(rec, P, thr, ref, d_off, d_cell)
    est, count = ctx.tumour_fraction(rec, P, thr, ref, d_off, d_cell, d_w)
    est_low, count_low = ctx.tumour_fraction(rec, P, thr_low, ref, d_off, d_cell, d_w)
    torch.cuda.synchronize()

    def work(est_, count_):
        """the evaluations the definition makes, from the outputs"""
        e, c = est_.cpu().numpy().reshape(-1, 4), count_.cpu().numpy().reshape(-1, 2)
        live = e[:, TF_F_HAT] != TF_NA
        inner = live & (e[:, TF_F_HAT] > 0) & (e[:, TF_F_HAT] < 1)   # F_HAT by bisection
        lower = live & (e[:, TF_T0] > TF_Z2_95)                       # F_LO by bisection
        upper = live & (e[:, TF_F_HI] > 0) & (e[:, TF_F_HI] < 1)      # F_HI by bisection
        evals = 2 * live + TF_ITERS * (inner.astype(np.int64) + lower + upper)
        cell_evals = int((evals * 2 * c[:, 0]).sum())
        return dict(pairs_estimated=int(live.sum()), evaluated_entries=int(c[:, 0].sum()), evaluations_total=int(evals.sum()),
                    evaluations_per_pair_mean=float(evals.mean()), evaluations_per_pair_max=int(evals.max()),
                    bisections=dict(f_hat=int(inner.sum()), f_lo=int(lower.sum()), f_hi=int(upper.sum())), cell_evaluations=cell_evals,
                    fp64_ops_cells=8 * cell_evals, fp64_ops_butterfly_per_lane=12 * int(evals.sum()), fp64_divisions=cell_evals)

    w_table, w_low = work(est, count), work(est_low, count_low)

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {"fraction": lambda: ctx.tumour_fraction(rec, P, thr, ref, d_off, d_cell, d_w, est=est, count=count),
             "monitor_sums": lambda: ctx.monitor_sums(rec, P, thr, ref, d_off, d_cell, sums=sums, lam=lam),
             "fraction_full": lambda: ctx.tumour_fraction(rec, P, thr_low, ref, d_off, d_cell, d_w, est=est_low, count=count_low)}
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    line = dict(kind="fraction_bench", P=P, samples=n, lists=L, entries=E, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                pairs=n * L, entries_total=n * L * E, low=a.low, work_fraction=w_table, work_fraction_full=w_low)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
    line["ratio_fraction_over_monitor_sums"] = med(times["fraction"]) / med(times["monitor_sums"])
    line["ratio_fraction_full_over_monitor_sums"] = med(times["fraction_full"]) / med(times["monitor_sums"])
    line["fraction_full_ns_per_pair"] = med(times["fraction_full"]) * 1e6 / (n * L)
    line["fraction_full_cell_GFLOPs"] = w_low["fp64_ops_cells"] / (med(times["fraction_full"]) * 1e-3) / 1e9
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
