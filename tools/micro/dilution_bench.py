"""The kernel of the in-silico dilution beside the parent's comparable pass.

Config 3's shape by default: 96 mixtures -- synthetic tumour i into synthetic normal i at fraction 0.1, scale 1, two resident chunks --
over 100 000 positions, uint16 records.  Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP events,
the kinds alternated in one process:
  * ampli_dilute_records (the 16 lists of a record walked one after the other; the form that lays them end to end was measured with
    this script too: tools/experiments/dilution_flat_form.patch and .log);
  * ampli_pair_score_records over the same grid -- the parent's pass that also reads row i of two chunks -- for orientation only: it
    does other work.
Reported: milliseconds, reads drawn per second and Philox blocks per second (the reads and blocks of the records both of whose
files have a line; a block is four reads of one list or its remainder).  Nobody measured a kernel of this form before, so no
expectation is asserted.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
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
    ap.add_argument("--mixtures", type=int, default=96)
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context, host_lib

    ctx = Context(0)
    P, T = a.P, a.mixtures
    n32, t32 = ctx.synth_fill(P, T), ctx.synth_fill(P, T, tumour=True)
    absent = -(1 << 31)
    both = (n32[:, :, 0] != absent) & (t32[:, :, 0] != absent)
    reads = int((n32.long() + t32.long())[both].sum().item())
    blocks = int((((n32.long() + 3) >> 2) + ((t32.long() + 3) >> 2))[both].sum().item())
    normals, fits = ctx.pack(n32, "u16")
    assert fits
    tumours, fits = ctx.pack(t32, "u16")
    assert fits
    del n32, t32
    ref = ctx.synth_ref(P)
    rn, rt = ctx.records(normals, "u16", T), ctx.records(tumours, "u16", T)
    keep = host_lib().ampli_host_dilute_keep
    mix = [(i, i, keep(a.fraction), keep(1.0 - a.fraction), (0x9E3779B97F4A7C15 * (i + 1)) & 0x7FFFFFFFFFFFFFFF) for i in range(T)]
    pairs = torch.stack([torch.arange(T, dtype=torch.int32), torch.arange(T, dtype=torch.int32)], dim=1).contiguous().to(ctx.device)
    out, flags = ctx.dilute(rt, rn, P, mix)
    d_mix = torch.tensor([[i | (i << 32), ka, kb, key] for i, _, ka, kb, key in mix], dtype=torch.int64, device=ctx.device)  # the descriptors, resident
    out, flags = ctx.dilute(rt, rn, P, d_mix, out=out, flags=flags)
    torch.cuda.synchronize()
    assert not bool(flags.any().item())
    kept = int(out[out[:, :, 0] != absent].long().sum().item())
    s = ctx.pair_score(rt, rn, P, pairs, ref, 100)

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {"dilute": lambda: ctx.dilute(rt, rn, P, d_mix, out=out, flags=flags), "pair_score": lambda: ctx.pair_score(rt, rn, P, pairs, ref, 100, s=s)}
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    line = dict(kind="dilution_bench", P=P, mixtures=T, fraction=a.fraction, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                reads=reads, philox_blocks=blocks, reads_kept=kept, records_mixed_fraction=float(both.float().mean().item()))
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
    line["dilute_reads_per_s"] = reads / (med(times["dilute"]) * 1e-3)
    line["dilute_blocks_per_s"] = blocks / (med(times["dilute"]) * 1e-3)
    line["ratio_dilute_over_pair_score"] = med(times["dilute"]) / med(times["pair_score"])
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
