"""Detection-power pass (limit_power_kernel) beside the detection-limit pass (limit_pairs_kernel) on the same resident tumour records.

Config 3's tumour shape by default: 96 synthetic tumours x 100 000 positions, uint16 records, thresholds from the configuration's 256
synthetic normals, levels 0.001 / 0.005 / 0.01, confidence 0.95.  The limits pass runs first and its minimum reads and statuses feed
the power pass as they are (cells the device left open count as not OK here; the command line settles them first).  Every repetition
is cold (256 MiB written in between), bracketed by HIP events, the kinds alternated in one process: the power pass with the root
search, the power pass at the levels only, and the limits pass.  Also reports the kernel's own counters -- tails and pmf terms per OK
pair, the most terms of one tail.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
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
    ap.add_argument("--confidence", type=float, default=0.95)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import LIMIT_RECHECK

    ctx = Context(0)
    P, S, T = a.P, a.S, a.T
    levels = (0.001, 0.005, 0.01)
    ref = ctx.synth_ref(P, seed=SEED)
    ctx.set_record_layout("u16")
    normals, fits = ctx.pack(ctx.synth_fill(P, S, seed=SEED), "u16")
    assert fits
    table = ctx.error_estimate(normals, P, 0.002, 100)
    del normals
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, seed=SEED, tumour=True), "u16")
    assert fits
    rec = ctx.records(tumours, "u16", T)
    lim = ctx.detection_limits(rec, P, table.thr, ref, 100, ())
    n_recheck = int((lim["status"] & LIMIT_RECHECK).ne(0).sum().item())
    ctx.power_stats(reset=True)
    pw = ctx.detection_power(rec, P, lim["min_reads"], lim["status"], levels, a.confidence)
    torch.cuda.synchronize()
    tails, terms, most = ctx.power_stats(reset=True)
    lv_only = ctx.detection_power(rec, P, lim["min_reads"], lim["status"], levels, a.confidence, want_lod=False)
    torch.cuda.synchronize()
    tails_lv, terms_lv, _ = ctx.power_stats(reset=True)
    counts = pw["counts"].sum(dim=0).cpu().tolist()
    n_ok = int(counts[0])
    assert n_ok == int(lim["counts"][:, 1].sum().item()) and counts == lv_only["counts"].sum(dim=0).cpu().tolist()
    lod_ok = pw["lod"][pw["lod"] > 0]
    assert lod_ok.numel() == n_ok
    quant = torch.quantile(lod_ok[:: max(1, n_ok // 1_000_000)].double(), torch.tensor([0.05, 0.5, 0.95], dtype=torch.float64, device=ctx.device)).cpu().tolist()

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_pow, t_lv, t_lim = [], [], []
    for _ in range(a.reps):
        t_pow.append(timed(lambda: ctx.detection_power(rec, P, lim["min_reads"], lim["status"], levels, a.confidence, counts=pw["counts"])))
        t_lv.append(timed(lambda: ctx.detection_power(rec, P, lim["min_reads"], lim["status"], levels, a.confidence, counts=lv_only["counts"],
                                                      want_lod=False)))
        t_lim.append(timed(lambda: ctx.detection_limits(rec, P, table.thr, ref, 100, (), counts=lim["counts"])))
    med = statistics.median
    cells = T * P * 4
    out_bytes = cells * 4 * (len(levels) + 1)
    line = dict(kind="power_bench", P=P, S=S, T=T, layout="u16", reps=a.reps, levels=list(levels), confidence=a.confidence,
                power_ms=med(t_pow), power_ms_min=min(t_pow), power_ms_max=max(t_pow),
                power_levels_only_ms=med(t_lv), power_levels_only_ms_min=min(t_lv),
                limit_ms=med(t_lim), limit_ms_min=min(t_lim), power_over_limit=med(t_pow) / med(t_lim),
                ok_pairs=n_ok, recheck_cells_left_out=n_recheck, pairs_with_power_ge_confidence=counts[1:],
                tails=tails, terms=terms, tails_per_ok_pair=tails / max(1, n_ok), terms_per_ok_pair=terms / max(1, n_ok),
                terms_per_tail=terms / max(1, tails), max_terms_of_one_tail=most,
                search_evaluations_per_ok_pair=(tails - tails_lv) / 2 / max(1, n_ok),
                lod_quantiles_5_50_95=quant,
                output_bytes=out_bytes, input_bytes=cells * 9 + T * P * 16, output_GBps_at_power_ms=out_bytes / med(t_pow) / 1e6)
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
