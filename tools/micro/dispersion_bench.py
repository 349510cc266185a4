"""The dispersion pass (dispersion_stream_kernel + dispersion_sample_reduce_kernel) against one error_estimate on the same resident records.

Config 3's normals by default: 256 synthetic normals x 100 000 positions, uint16 records, one chunk (410 MB, read once by either).
Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the two kinds alternated in one process.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=100_000)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context

    ctx = Context(0)
    P, S = a.P, a.S
    normals32 = ctx.synth_fill(P, S)
    normals, fits = ctx.pack(normals32, "u16")
    assert fits
    del normals32
    ctx.set_record_layout("u16")
    rec = ctx.records(normals, "u16", S)
    acc0 = ctx.new_acc(P)
    ctx.error_reduce_records(rec, P, acc0, 0.0, 100, summary=True)
    d = ctx.device
    x2 = torch.empty((2, 4, P), dtype=torch.float64, device=d)
    rinv = torch.empty((2, 4, P), dtype=torch.float64, device=d)
    sx = torch.empty((S,), dtype=torch.float64, device=d)
    se = torch.empty((S,), dtype=torch.float64, device=d)
    st = torch.empty((S,), dtype=torch.int64, device=d)
    z = torch.empty((2, 4, P), dtype=torch.float64, device=d)
    phi = torch.empty((2, 4, P), dtype=torch.float32, device=d)
    status = torch.empty((2, 4, P), dtype=torch.uint8, device=d)
    counts = torch.zeros((4,), dtype=torch.int64, device=d)
    ctx.dispersion_records(rec, P, acc0, 100, x2, rinv, sample_x2=sx, sample_expect=se, sample_terms=st)  # warm: the workspace is sized here
    ctx.dispersion_finalize(P, acc0, x2, rinv, 4.0, z, phi, status, counts)
    table = ctx.error_estimate(normals, P, 0.002, 100)
    torch.cuda.synchronize()
    cells = [int(v) for v in counts.cpu()]

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=d)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_pass, t_nosamp, t_fin, t_ee = [], [], [], []
    for _ in range(a.reps):
        t_pass.append(timed(lambda: ctx.dispersion_records(rec, P, acc0, 100, x2, rinv, sample_x2=sx, sample_expect=se, sample_terms=st)))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        t_nosamp.append(timed(lambda: ctx.dispersion_records(rec, P, acc0, 100, x2, rinv)))
        t_fin.append(timed(lambda: ctx.dispersion_finalize(P, acc0, x2, rinv, 4.0, z, phi, status, counts)))
    med = statistics.median
    nbytes = S * P * 16
    line = dict(kind="dispersion_bench", P=P, S=S, layout="u16", reps=a.reps, record_bytes=nbytes, cells_ok=cells[0], cells_few=cells[1], cells_high=cells[2],
                pass_ms=med(t_pass), pass_ms_min=min(t_pass), pass_ms_max=max(t_pass), pass_ms_all=[round(v, 4) for v in t_pass],
                pass_without_samples_ms=med(t_nosamp), finalize_ms=med(t_fin),
                error_estimate_ms=med(t_ee), error_estimate_ms_min=min(t_ee), error_estimate_ms_max=max(t_ee),
                ratio_pass_over_error_estimate=med(t_pass) / med(t_ee),
                pass_GBps=nbytes / med(t_pass) / 1e6, share_of_8_TBps=nbytes / med(t_pass) / 1e6 / 8000.0,
                error_estimate_GBps=nbytes / med(t_ee) / 1e6)
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
