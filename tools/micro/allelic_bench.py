"""The three stages of allelic imbalance beside error_estimate over the same records.

Config 3's shape by default: 256 synthetic normals and 96 tumours over 100 000 positions, uint16 records; one region per 500 positions
and ALL.  Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated in one
process:
  * ampli_hetsite_reference_records over the normals, beside error_reduce over the same records (both read every record once);
  * ampli_allelic_site_records over the tumours with their own genotypes, beside error_reduce over the tumours' records;
  * ampli_allelic_region_sums over the tumours' site planes.
Reported: milliseconds, the ratios, and the bytes the definition moves (records and planes read, outputs stored).  No time is fixed in
advance.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py."""
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
    ap.add_argument("--region", type=int, default=500)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P, N, T = a.P, a.normals, a.tumours
    n16, fits_n = ctx.pack(ctx.synth_fill(P, N), "u16")
    t16, fits_t = ctx.pack(ctx.synth_fill(P, T, tumour=True), "u16")
    assert fits_n and fits_t
    nrec, trec = ctx.records(n16, "u16", N), ctx.records(t16, "u16", T)
    pl_n, pl_t = ctx.genotype_planes(nrec, P), ctx.genotype_planes(trec, P)
    row_g = torch.arange(T, dtype=torch.int32, device=ctx.device)
    ref = ctx.hetsite_reference(nrec, P, pl_n, 100)
    q, km, v, code = ctx.allelic_sites(trec, P, pl_t, row_g, ref, 100, 5, True)
    R = (P + a.region - 1) // a.region + 1
    off = np.concatenate([np.minimum(np.arange(R) * a.region, P), [2 * P]]).astype(np.int32)
    pos = np.concatenate([np.arange(P), np.arange(P)]).astype(np.int32)
    d_off, d_pos = torch.from_numpy(off).to(ctx.device), torch.from_numpy(pos).to(ctx.device)
    sums = ctx.allelic_regions(q, km, v, code, d_off, d_pos, 20.0)
    acc_n, acc_t = ctx.new_acc(P), ctx.new_acc(P)
    torch.cuda.synchronize()
    st = (code >> 3).cpu().numpy()
    tested, het_ref = int((st >= 5).sum()), int((ref[0] > 0).sum().item())

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {"hetsite_reference": lambda: ctx.hetsite_reference(nrec, P, pl_n, 100, ref=ref),
             "error_reduce_normals": lambda: ctx.error_reduce_records(nrec, P, acc_n, summary=True),
             "allelic_sites": lambda: ctx.allelic_sites(trec, P, pl_t, row_g, ref, 100, 5, True, q=q, km=km, v=v, code=code),
             "error_reduce_tumours": lambda: ctx.error_reduce_records(trec, P, acc_t, summary=True),
             "allelic_regions": lambda: ctx.allelic_regions(q, km, v, code, d_off, d_pos, 20.0, out=sums)}
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    W = (P + 63) // 64
    line = dict(kind="allelic_bench", P=P, normals=N, tumours=T, regions=R, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                tested_cells=tested, reference_cells=het_ref,
                hetsite_reference_bytes=N * P * 16 + N * 6 * W * 8 + 2 * 18 * P * 8, error_reduce_normals_bytes=N * P * 16,
                allelic_sites_bytes=T * P * 16 + T * 6 * W * 8 + T * P * 21 + tested * 24, error_reduce_tumours_bytes=T * P * 16,
                allelic_regions_bytes=2 * T * P * 1 + 2 * tested * 20 + T * R * 40)
    for k, vals in times.items():
        line[k + "_ms"] = med(vals)
        line[k + "_ms_min"] = min(vals)
        line[k + "_ms_max"] = max(vals)
        line[k + "_ms_all"] = [round(x, 4) for x in vals]
        line[k + "_GBps"] = line[k + "_bytes"] / (med(vals) * 1e-3) / 1e9
    line["ratio_hetsite_reference_over_error_reduce"] = med(times["hetsite_reference"]) / med(times["error_reduce_normals"])
    line["ratio_allelic_sites_over_error_reduce"] = med(times["allelic_sites"]) / med(times["error_reduce_tumours"])
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
