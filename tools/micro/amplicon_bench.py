"""The amplicon depth kernel against one error_estimate on the same resident records.

Config 3's shape by default: 256 synthetic normals x 100 000 positions, uint16 records resident in one buffer, amplicons of 130
positions laid end to end (the last one shorter).  Every repetition is cold for the caches (256 MiB written in between), bracketed by
HIP events, the kinds alternated in one process: ampli_amplicon_depth_records, error_estimate (the parent's kernel, unchanged), a
device-to-device copy of the record buffer (the box's copy rate, read + written bytes), and the two stage-2 calls on the 256 x A
matrix, which are reported in microseconds only.  The figure of merit is depth_ms / error_estimate_ms.  One JSON line on stdout; --out
also writes it.  Not a replacement for bench.py.
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
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--amplicon", type=int, default=130)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P, S, L = a.P, a.S, a.amplicon
    normals32 = ctx.synth_fill(P, S)
    normals, fits = ctx.pack(normals32, "u16")
    assert fits
    del normals32
    ctx.set_record_layout("u16")
    rec = ctx.records(normals, "u16", S)
    off = np.minimum(np.arange(0, P + L, L), P).astype(np.int32)
    A = len(off) - 1
    d_off = torch.from_numpy(off).to(ctx.device)
    d_pos = torch.arange(P, dtype=torch.int32, device=ctx.device)
    use = torch.ones((A,), dtype=torch.uint8, device=ctx.device)
    sums = ctx.amplicon_depth(rec, P, d_off, d_pos)
    table = ctx.error_estimate(normals, P, 0.002, 100)
    ref = ctx.amplicon_reference(sums, use, 5)
    ctx.amplicon_ratio(sums, use, ref)
    copy = torch.empty_like(normals)
    torch.cuda.synchronize()
    s = sums.cpu().numpy()
    assert (s[:, :, 0] <= np.diff(off)[None, :]).all() and s[:, :, 1:3].sum() > 0

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_depth, t_ee, t_copy, t_ref, t_ratio = [], [], [], [], []
    for _ in range(a.reps):
        t_depth.append(timed(lambda: ctx.amplicon_depth(rec, P, d_off, d_pos, out=sums)))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        t_copy.append(timed(lambda: copy.copy_(normals)))
        t_ref.append(timed(lambda: ctx.amplicon_reference(sums, use, 5)))
        t_ratio.append(timed(lambda: ctx.amplicon_ratio(sums, use, ref)))
    med = statistics.median
    rec_bytes = S * P * 16
    copy_rate = 2 * rec_bytes / (med(t_copy) * 1e-3)
    depth_rate = (rec_bytes + S * A * 32) / (med(t_depth) * 1e-3)
    line = dict(kind="amplicon_bench", P=P, S=S, A=A, amplicon=L, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                depth_ms=med(t_depth), depth_ms_min=min(t_depth), depth_ms_max=max(t_depth), error_estimate_ms=med(t_ee),
                error_estimate_ms_min=min(t_ee), error_estimate_ms_max=max(t_ee), ratio_depth_over_error_estimate=med(t_depth) / med(t_ee),
                expected_ratio_at_most=1.25, record_bytes=rec_bytes, copy_ms=med(t_copy), copy_bytes_per_s=copy_rate,
                depth_bytes_per_s=depth_rate, depth_fraction_of_copy_rate=depth_rate / copy_rate,
                reference_us=med(t_ref) * 1e3, reference_us_min=min(t_ref) * 1e3, ratio_us=med(t_ratio) * 1e3, ratio_us_min=min(t_ratio) * 1e3,
                depth_ms_all=[round(v, 4) for v in t_depth], error_estimate_ms_all=[round(v, 4) for v in t_ee])
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
