"""Leave-one-out pass (loo_stream_kernel + loo_drain_kernel) against one error_estimate on the same resident records.

Config 3's shape by default: 256 synthetic normals x 100 000 positions, uint16 records, one chunk.  Every repetition is cold for the
timed call's own outputs, bracketed by HIP events, the two kinds alternated.  Also prints what S separate reruns would cost from the
same measured kernels: S x (error_estimate over S-1 normals + poisson_call on 1).  One JSON line on stdout; --out also writes it.
Not a replacement for bench.py.
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import POISSON_PREFILTER

    ctx = Context(0)
    P, S = a.P, a.S
    normals32 = ctx.synth_fill(P, S)
    ref = ctx.synth_ref(P)
    normals, fits = ctx.pack(normals32, "u16")
    assert fits
    del normals32
    ctx.set_record_layout("u16")
    rec = ctx.records(normals, "u16", S)
    acc = ctx.new_acc(P)
    ctx.error_reduce_records(rec, P, acc, 0.002, 100, summary=True)
    callable_pos = torch.zeros((P,), dtype=torch.int32, device=ctx.device)
    callable_sample = torch.zeros((S,), dtype=torch.int32, device=ctx.device)
    flags = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    cap = 1 << 22
    loo = ctx.loo_call(rec, P, acc, ref, 0.002, 100, 100, POISSON_PREFILTER, capacity=cap, callable_pos=callable_pos,
                       callable_sample=callable_sample, flags=flags)
    table = ctx.error_estimate(normals, P, 0.002, 100)
    one = normals[:1]
    pc = ctx.poisson_call(one, P, table.thr, ref, 100, mode=POISSON_PREFILTER, capacity=1 << 16)
    sub = normals[: S - 1]
    torch.cuda.synchronize()
    n_calls = ctx.n_calls_total(loo)
    assert int(flags.item()) == 0 and ctx.flags() & 4 == 0

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_loo, t_ee, t_ee_sub, t_pc = [], [], [], []
    for _ in range(a.reps):
        t_loo.append(timed(lambda: ctx.loo_call(rec, P, acc, ref, 0.002, 100, 100, POISSON_PREFILTER, capacity=cap, call_mask=loo["call_mask"],
                                                calls_buf=loo["calls_buf"], n_calls=loo["n_calls"], callable_pos=callable_pos,
                                                callable_sample=callable_sample, flags=flags)))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        t_ee_sub.append(timed(lambda: ctx.error_estimate(sub, P, 0.002, 100, out=table)))
        t_pc.append(timed(lambda: ctx.poisson_call(one, P, table.thr, ref, 100, mode=POISSON_PREFILTER, capacity=1 << 16,
                                                   call_mask=pc["call_mask"], calls_buf=pc["calls_buf"], n_calls=pc["n_calls"])))
    med = statistics.median
    line = dict(kind="loo_bench", P=P, S=S, layout="u16", reps=a.reps, loo_calls=n_calls,
                loo_ms=med(t_loo), loo_ms_min=min(t_loo), error_estimate_ms=med(t_ee), error_estimate_ms_min=min(t_ee),
                ratio_loo_over_error_estimate=med(t_loo) / med(t_ee), target_ratio=4.0,
                reruns_ms=S * (med(t_ee_sub) + med(t_pc)), error_estimate_s_minus_1_ms=med(t_ee_sub), poisson_call_one_ms=med(t_pc),
                reruns_over_loo=S * (med(t_ee_sub) + med(t_pc)) / med(t_loo))
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
