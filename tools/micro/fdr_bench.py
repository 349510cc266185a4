"""The false-discovery adjustment beside the scorer that feeds it.

Config 3's shape by default: 96 synthetic tumours over 100 000 positions, uint16 records, scored by ampli_nb_score_records with omega
NULL; the plane it writes is what ampli_fdr_adjust sorts and adjusts, 96 rows of 400 000 keys.  Every repetition is cold for the caches
(256 MiB written in between), bracketed by HIP events, the kinds alternated in one process:
  * ampli_fdr_adjust over the 96 rows, with and without the ranks;
  * ampli_nb_score_records over the 96 tumours -- the parent's pass that produces the plane, the yardstick.
The entry is one call of 20 launches; its kernel groups (keys, the four sort passes, adjust, lookup) are timed by running this script
under a kernel trace, not here.  bytes_model is what the entry has to move: the plane read twice (keys, lookup), the keys written once,
read twice and written once per sort pass, read and written once by the adjustment, d_a (and d_rank) written once, plus the digit
histograms; the binary search's reads stay in L2 and are not counted.  Nobody measured this before, so no expectation is asserted.  One
JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
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

TILE_KEYS = 4096  # AMPLI_FDR_TILE_KEYS


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--rows", type=int, default=96)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import FDR_NA

    ctx = Context(0)
    P, T = a.P, a.rows
    normals, fits = ctx.pack(ctx.synth_fill(P, T), "u16")
    assert fits
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, tumour=True), "u16")
    assert fits
    ref = ctx.synth_ref(P)
    rt = ctx.records(tumours, "u16", T)
    ctx.set_record_layout("u16")
    table = ctx.error_estimate(normals, P, 0.002, 100)
    q = ctx.nb_score(rt, P, table.thr, ref, None, 100)
    work = torch.empty((ctx.fdr_workspace_bytes(T, P),), dtype=torch.uint8, device=ctx.device)
    adj, m, rank = ctx.fdr_adjust(q, False, rank=True, work=work)
    torch.cuda.synchronize()
    tested = float((adj != FDR_NA).float().mean().item())
    positive = float((rank > 0).float().mean().item())
    found = int((adj >= 13.0103).sum().item())  # fdr 0.05

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {
        "fdr_adjust": lambda: ctx.fdr_adjust(q, False, a=adj, m=m, rank=rank, work=work),
        "fdr_adjust_no_rank": lambda: ctx.fdr_adjust(q, False, a=adj, m=m, rank=False, work=work),
        "nb_score_poisson": lambda: ctx.nb_score(rt, P, table.thr, ref, None, 100, q=q),
    }
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    n = 4 * P
    tiles = (n + TILE_KEYS - 1) // TILE_KEYS
    hist = 256 * tiles * 4
    per_row = dict(keys=32 * P + 4 * n, sort=4 * (3 * 4 * n + 4 * hist), adjust=2 * 4 * n, lookup=32 * P + 2 * 4 * n)
    line = dict(kind="fdr_bench", P=P, rows=T, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name, workspace_MB=work.numel() / 1e6,
                tested_fraction=tested, positive_key_fraction=positive, cells_at_fdr_0_05=found, launches_per_call=20,
                bytes_model_per_group={k: v * T for k, v in per_row.items()}, bytes_model=sum(per_row.values()) * T)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
    line["ratio_fdr_adjust_over_nb_score_poisson"] = med(times["fdr_adjust"]) / med(times["nb_score_poisson"])
    line["fdr_adjust_keys_per_s"] = T * n / (med(times["fdr_adjust"]) * 1e-3)
    line["fdr_adjust_model_bytes_per_s"] = line["bytes_model"] / (med(times["fdr_adjust"]) * 1e-3)
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
