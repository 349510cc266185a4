"""The contamination kernel at config 3's and config 4's sample counts: every sample against every sample.

contamination_kernel at N = 352 and N = 2048 recipients against themselves as sources, P = 100 000, uint16 records resident in one
chunk: time, (position, source) pairs per second, and the share of the VALU issue rate that implies, from the instruction count of
the compiled loops (read off the gfx950 assembly of the uint16 kernel): VALU_PER_HOM_POSITION vector instructions per position at which
the recipient is validly homozygous (the scalar bit walk skips the others) and VECTOR_PER_WORD per plane word around that walk, each for
one wave = 64 sources.  The arithmetic is that of tools/micro/concordance_bench.py.
Every GPU repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the shapes alternated in one process.
One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
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

# the inner loop of ct_half<unsigned>: 6 v_readlane, 9 v_bfe_i32, 10 v_and, 8 v_add_u32, 1 v_add3_u32 (the seven sums of a half word are 32-bit)
VALU_PER_HOM_POSITION = 34
# around it, per plane word: 7 loads (six plane words, one record), the record's decode, the masks, three 64-bit popcounts, and twice
# seven 64-bit adds of the half words' sums
VECTOR_PER_WORD = 185
MAX_SLICES, MIN_WORDS, WAVES_PER_CU = 16, 4, 32  # ct_slices of ampli_contamination.hip


def slices(waves: int, n_cu: int, W: int):
    want = max(1, min(MAX_SLICES, (WAVES_PER_CU * n_cu + waves - 1) // waves))
    wps = max(MIN_WORDS, (W + want - 1) // want)
    return (W + wps - 1) // wps, wps


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--N", type=int, nargs="+", default=[352, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=256, help="samples generated and encoded at a time")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P = a.P
    d = ctx.device
    W = (P + 63) // 64
    n_max = max(a.N)
    # n_max synthetic normals as uint16 records in one resident buffer, and their planes
    recs16 = torch.empty((n_max, P, 8), dtype=torch.int16, device=d)
    planes = torch.empty((n_max, 6, W), dtype=torch.int64, device=d)
    buf32 = torch.empty((a.chunk, P, 8), dtype=torch.int32, device=d)
    for lo in range(0, n_max, a.chunk):
        n = min(a.chunk, n_max - lo)
        ctx.synth_fill(P, n, first_sample=lo, out=buf32[:n])
        packed, fits = ctx.pack(buf32[:n], "u16")
        assert fits
        recs16[lo:lo + n] = packed.view(torch.int16).reshape(n, P, 8)
        ctx.genotype_planes(ctx.records(buf32[:n], "i32", n), P, out=planes[lo:lo + n])
    del buf32
    ctx.set_record_layout("u16")
    torch.cuda.synchronize()
    pl = planes.cpu().numpy().view(np.uint64)
    hom = pl[:, 0] & ~pl[:, 5]
    hom_positions = np.unpackbits(hom.view(np.uint8), axis=1).sum(axis=1).astype(np.int64)  # per sample
    sums = {n: torch.empty((n, n, 9), dtype=torch.int64, device=d) for n in a.N}
    recs = {n: ctx.records(recs16, "u16", n) for n in a.N}

    def run(n):
        ctx._check(ctx.lib.ampli_contamination_records(ctx.h, recs[n], P, planes.data_ptr(), planes.data_ptr(), n, sums[n].data_ptr()))

    for n in a.N:
        run(n)  # warm
    torch.cuda.synchronize()
    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=d)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t = {n: [] for n in a.N}
    for _ in range(a.reps):
        for n in a.N:
            t[n].append(timed(lambda: run(n)))
    med = statistics.median
    props = torch.cuda.get_device_properties(0)
    n_cu = props.multi_processor_count
    clock_hz = float(getattr(props, "clock_rate", 2_400_000)) * 1e3  # kHz
    valu_rate = n_cu * 4 * clock_hz / 2  # wave instructions per second, as tools/micro/concordance_bench.py counts them
    line = dict(kind="contamination_bench", P=P, W=W, layout="u16", reps=a.reps, device=props.name, compute_units=n_cu, clock_hz=clock_hz,
                valu_per_hom_position_and_wave=VALU_PER_HOM_POSITION, vector_per_word_and_wave=VECTOR_PER_WORD, shapes=[])
    for n in a.N:
        tiles = (n + 63) // 64
        n_slices, wps = slices(n * tiles, n_cu, W)
        hp = int(hom_positions[:n].sum())
        wave_instr = tiles * (hp * VALU_PER_HOM_POSITION + n * W * VECTOR_PER_WORD)
        ms = med(t[n])
        bound_ms = wave_instr / valu_rate * 1e3
        s = sums[n].cpu().numpy()
        line["shapes"].append(dict(N=n, ordered_pairs=n * n, ms=ms, ms_min=min(t[n]), ms_max=max(t[n]), ms_all=[round(v, 4) for v in t[n]],
                                   position_pairs_per_s=n * n * P / (ms * 1e-3), waves=n * tiles * n_slices, slices=n_slices, words_per_slice=wps,
                                   wave_slots=n_cu * 4 * 5, hom_position_share=hp / (n * P), wave_instructions=wave_instr,
                                   valu_issue_bound_ms=bound_ms, valu_issue_fraction=bound_ms / ms,
                                   record_bytes=n * P * 16, plane_bytes=n * 6 * W * 8, sum_bytes=n * n * 72,
                                   informative_sites_median=float(np.median(s[:, :, 0] + s[:, :, 3])), background_sites_median=float(np.median(s[:, :, 6]))))
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
