"""The kernel of the paired comparison beside the parent's comparable pass.

Config 3's shape by default: 96 pairs -- synthetic tumour i against synthetic normal i, two resident chunks -- over 100 000 positions,
uint16 records.  Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated
in one process:
  * ampli_pair_score_records over the 96 pairs;
  * ampli_nb_score_records with omega NULL over the 96 tumours -- the parent's pass with the same grid shape (a wave per row of a
    64-position tile, a lane's six tails in one loop) and the same store volume (96 x P x 8 floats).  It reads one record per lane
    where the paired kernel reads two.
Nobody measured a kernel of this form before, so no expectation is asserted.  One JSON line on stdout; --out also writes it.  Not a
replacement for bench.py.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=96)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import NB_NA, PAIR_NA

    ctx = Context(0)
    P, T = a.P, a.pairs
    normals, fits = ctx.pack(ctx.synth_fill(P, T), "u16")
    assert fits
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, tumour=True), "u16")
    assert fits
    ref = ctx.synth_ref(P)
    rn, rt = ctx.records(normals, "u16", T), ctx.records(tumours, "u16", T)
    ctx.set_record_layout("u16")
    table = ctx.error_estimate(normals, P, 0.002, 100)
    pairs = torch.stack([torch.arange(T, dtype=torch.int32), torch.arange(T, dtype=torch.int32)], dim=1).contiguous().to(ctx.device)
    s = ctx.pair_score(rt, rn, P, pairs, ref, 100)
    q = ctx.nb_score(rt, P, table.thr, ref, None, 100)
    torch.cuda.synchronize()
    ev = s[..., 0] != PAIR_NA
    evaluated = float(ev.float().mean().item())
    summed = float((ev[..., None] & (s != 0)).float().mean().item())   # cells whose score needed at least a first term
    clamped = float((ev[..., None] & (s.abs() == 100)).float().mean().item())
    nb_scored = float(((q != NB_NA) & (q != 0)).float().mean().item())

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {
        "pair_score": lambda: ctx.pair_score(rt, rn, P, pairs, ref, 100, s=s),
        "nb_score_poisson": lambda: ctx.nb_score(rt, P, table.thr, ref, None, 100, q=q),
    }
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    line = dict(kind="paired_bench", P=P, pairs=T, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                evaluated_fraction=evaluated, summed_fraction=summed, clamped_fraction=clamped, nb_scored_fraction=nb_scored)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
    line["ratio_pair_score_over_nb_score_poisson"] = med(times["pair_score"]) / med(times["nb_score_poisson"])
    line["pair_score_cells_per_s"] = T * P * 6 / (med(times["pair_score"]) * 1e-3)
    line["pair_score_bytes_per_s"] = (2 * T * P * 16 + T * P * 32) / (med(times["pair_score"]) * 1e-3)  # two records read, eight floats stored per position
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
