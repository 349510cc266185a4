"""The sample-identity kernels: the encode pass beside one error_estimate on the same resident records, the pair kernel at
config 3's and config 4's sample counts, and the same matrix from the numpy model for scale.

1. genotype_planes_kernel over config 3's normals (256 x 100 000 positions, uint16 records, one chunk) against error_estimate on the
   same records, as a ratio.
2. concordance_pairs_kernel at N = 352 and N = 2048 samples (the set against itself: the upper triangle computed and mirrored),
   P = 100 000: time, pair-words per second, and the share of the VALU issue rate that implies, from the instruction count of the
   compiled inner loop (VALU_PER_8_PAIR_WORDS below, read off the gfx950 assembly of one word step of one thread: 8 pairs).
3. the 2048-sample matrix from tests/concordance_model.py (float64 matrix products on the host's cores) over --model-P positions,
   scaled to P: for scale only.
Every GPU repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated in one process.
One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# one word step of one thread of concordance_pairs_kernel = 8 pairs (4 a rows x 2 b rows): 418 VALU instructions (112 v_and, 80 v_bcnt,
# 64 v_xor, 48 v_or, 32 v_or3, 32 v_bfi, 47 v_add, 3 of the loop) and 12 ds_read_b128 + 6 ds_read2_b64 = 288 bytes from LDS
VALU_PER_8_PAIR_WORDS = 418
LDS_BYTES_PER_8_PAIR_WORDS = 288
TILE_A, TILE_B, SLAB = 32, 64, 8


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--S", type=int, default=256, help="normals of the encode pass")
    ap.add_argument("--N", type=int, nargs="+", default=[352, 2048], help="samples of the pair kernel")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--model-P", type=int, default=1600, help="positions the numpy model is timed on (0 = skip)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P, S = a.P, a.S
    d = ctx.device
    W = (P + 63) // 64
    normals32 = ctx.synth_fill(P, S)
    normals, fits = ctx.pack(normals32, "u16")
    assert fits
    del normals32
    ctx.set_record_layout("u16")
    rec = ctx.records(normals, "u16", S)
    n_max = max(a.N)
    planes = torch.empty((n_max, 6, W), dtype=torch.int64, device=d)
    ctx.genotype_planes(rec, P, out=planes[:S])  # warm
    table = ctx.error_estimate(normals, P, 0.002, 100)
    # the other samples of the pair kernel: further synthetic normals, a chunk at a time, each encoded into its rows and dropped
    buf32 = torch.empty((S, P, 8), dtype=torch.int32, device=d)
    for lo in range(S, n_max, S):
        n = min(S, n_max - lo)
        ctx.synth_fill(P, n, first_sample=lo, out=buf32[:n])
        ctx.genotype_planes(ctx.records(buf32[:n], "i32", n), P, out=planes[lo:lo + n])
    del buf32
    counts = {n: torch.empty((n, n, 5), dtype=torch.int32, device=d) for n in a.N}
    for n in a.N:
        ctx._check(ctx.lib.ampli_concordance_pairs(ctx.h, P, planes.data_ptr(), n, planes.data_ptr(), n, counts[n].data_ptr()))  # warm
    torch.cuda.synchronize()

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=d)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_enc, t_ee = [], []
    t_pairs = {n: [] for n in a.N}
    for _ in range(a.reps):
        t_enc.append(timed(lambda: ctx.genotype_planes(rec, P, out=planes[:S])))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        for n in a.N:
            t_pairs[n].append(timed(lambda: ctx._check(ctx.lib.ampli_concordance_pairs(ctx.h, P, planes.data_ptr(), n, planes.data_ptr(), n,
                                                                                       counts[n].data_ptr()))))
    med = statistics.median
    props = torch.cuda.get_device_properties(0)
    n_cu = props.multi_processor_count
    clock_hz = float(getattr(props, "clock_rate", 2_400_000)) * 1e3  # kHz
    valu_rate = n_cu * 4 * clock_hz / 2  # wave instructions per second: a wave64 VALU instruction occupies its SIMD (32 lanes per cycle) for 2 cycles
    lds_rate = n_cu * 256 * clock_hz     # bytes per second the LDS arrays can read: 256 B per clock and CU
    enc_bytes = S * P * 16 + S * 6 * W * 8
    line = dict(kind="concordance_bench", P=P, W=W, reps=a.reps, device=props.name, compute_units=n_cu, clock_hz=clock_hz,
                encode=dict(S=S, layout="u16", bytes_read=S * P * 16, bytes_written=S * 6 * W * 8, ms=med(t_enc), ms_min=min(t_enc), ms_max=max(t_enc),
                            ms_all=[round(v, 4) for v in t_enc], tb_per_s=enc_bytes / (med(t_enc) * 1e-3) / 1e12,
                            error_estimate_ms=med(t_ee), error_estimate_ms_min=min(t_ee), error_estimate_ms_max=max(t_ee),
                            ratio_encode_over_error_estimate=med(t_enc) / med(t_ee)),
                valu_instructions_per_8_pair_words=VALU_PER_8_PAIR_WORDS, valu_instructions_per_pair_word=VALU_PER_8_PAIR_WORDS / 8,
                lds_bytes_per_pair_word=LDS_BYTES_PER_8_PAIR_WORDS / 8, pairs=[])
    for n in a.N:
        ta, tb = (n + TILE_A - 1) // TILE_A, (n + TILE_B - 1) // TILE_B
        tiles = sum(1 for i in range(ta) for j in range(tb) if (j + 1) * TILE_B - 1 >= i * TILE_A)  # the tiles that are not wholly below the diagonal
        computed = tiles * TILE_A * TILE_B * ((W + SLAB - 1) // SLAB * SLAB)  # pair-words the kernel evaluates, edge padding included
        ms = med(t_pairs[n])
        wave_instr = computed / 64 * VALU_PER_8_PAIR_WORDS / 8
        line["pairs"].append(dict(N=n, pairs_in_matrix=n * n, ms=ms, ms_min=min(t_pairs[n]), ms_max=max(t_pairs[n]), ms_all=[round(v, 4) for v in t_pairs[n]],
                                  matrix_pair_words_per_s=n * n * W / (ms * 1e-3), tiles_computed=tiles, tiles_in_matrix=ta * tb,
                                  computed_pair_words=computed, computed_pair_words_per_s=computed / (ms * 1e-3),
                                  valu_issue_fraction=wave_instr / (ms * 1e-3) / valu_rate,
                                  lds_read_tb_per_s=computed * LDS_BYTES_PER_8_PAIR_WORDS / 8 / (ms * 1e-3) / 1e12,
                                  lds_read_fraction=computed * LDS_BYTES_PER_8_PAIR_WORDS / 8 / (ms * 1e-3) / lds_rate,
                                  workgroups=tiles, workgroup_slots=n_cu * 4,
                                  plane_bytes=n * 6 * W * 8, count_bytes=n * n * 20))
    if a.model_P:
        from tests.concordance_model import classify, pair_counts

        mp = min(a.model_P, P)
        rows = torch.empty((n_max, mp, 8), dtype=torch.int32, device=d)
        for lo in range(0, n_max, S):
            n = min(S, n_max - lo)
            full = ctx.synth_fill(P, n, first_sample=lo)
            rows[lo:lo + n] = full[:, :mp]
            del full
        host = rows.cpu().numpy()
        t = time.perf_counter()
        bits = classify(host)
        t_classify = time.perf_counter() - t
        t = time.perf_counter()
        model = pair_counts(bits, bits)
        t_pair = time.perf_counter() - t
        line["numpy_model_for_scale"] = dict(N=n_max, positions_timed=mp, classify_s=t_classify, pair_counts_s=t_pair,
                                             pair_counts_s_scaled_to_P=t_pair * P / mp, threads=os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"]),
                                             note="float64 matrix products of tests/concordance_model.py on the host's cores, timed on positions_timed positions and scaled linearly to P")
        # and, while both are here: the device's matrix over the same positions equals the model's
        sub = ctx.genotype_planes(ctx.records(rows, "i32", n_max), mp)
        got = ctx.concordance(sub, sub, mp).cpu().numpy()
        line["numpy_model_for_scale"]["device_equals_model"] = bool(np.array_equal(got, model))
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
