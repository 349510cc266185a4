"""The panel-of-normals exceedance kernel beside one error_estimate on the normals and a device copy of the same bytes.

96 synthetic tumour rows x 256 synthetic normals x 100 000 positions by default, uint16 records on both sides, the synthetic panel's
reference codes.  Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated
in one process: ampli_exceedance_records, error_estimate on the normals (the parent's kernel, unchanged) and a device-to-device copy
of the normals' record buffer (the box's copy rate, read + written bytes).  The kernel's rate is given as 64-bit comparisons per
second -- n_t x n_n x P x 8 cells, two 32 x 32 -> 64 multiplies each -- and against the bytes it must move: both record sets once and
the two outputs.  Nobody measured a kernel of this form before, so no expectation is asserted.  One JSON line on stdout; --out also
writes it.  Not a replacement for bench.py.
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
    ap.add_argument("--T", type=int, default=96)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import EXCEEDANCE_NA, EXCEEDANCE_ROWS

    ctx = Context(0)
    P, T, S = a.P, a.T, a.S
    normals, fits = ctx.pack(ctx.synth_fill(P, S), "u16")
    assert fits
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, tumour=True), "u16")
    assert fits
    ref = ctx.synth_ref(P)
    rn, rt = ctx.records(normals, "u16", S), ctx.records(tumours, "u16", T)
    elig, ge = ctx.exceedance(rt, rn, P, ref, first_t=S)
    ctx.set_record_layout("u16")
    table = ctx.error_estimate(normals, P, 0.002, 100)
    copy = torch.empty_like(normals)
    torch.cuda.synchronize()
    e, g = elig.cpu().numpy().view(np.uint16), ge.cpu().numpy().view(np.uint16)
    evaluated = g != EXCEEDANCE_NA
    assert evaluated.any() and e.max() <= S and (g[evaluated] <= S).all()

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_ex, t_ee, t_copy = [], [], []
    for _ in range(a.reps):
        t_ex.append(timed(lambda: ctx.exceedance(rt, rn, P, ref, first_t=S, elig=elig, ge=ge)))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        t_copy.append(timed(lambda: copy.copy_(normals)))
    med = statistics.median
    comparisons = T * S * P * 8
    must_move = (T + S) * P * 16 + T * P * 18 + P                       # both record sets once, the two outputs, the reference codes
    groups = (T + EXCEEDANCE_ROWS - 1) // EXCEEDANCE_ROWS
    does_move = (T + groups * S) * P * 16 + T * P * 18 + groups * P     # the normals once per group of tumour rows
    copy_rate = 2 * S * P * 16 / (med(t_copy) * 1e-3)
    line = dict(kind="exceedance_bench", P=P, T=T, S=S, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                evaluated_fraction=float(evaluated.mean()), exceedance_ms=med(t_ex), exceedance_ms_min=min(t_ex), exceedance_ms_max=max(t_ex),
                error_estimate_ms=med(t_ee), error_estimate_ms_min=min(t_ee), error_estimate_ms_max=max(t_ee),
                ratio_exceedance_over_error_estimate=med(t_ex) / med(t_ee), comparisons=comparisons,
                comparisons_per_s=comparisons / (med(t_ex) * 1e-3), multiplies_per_s=2 * comparisons / (med(t_ex) * 1e-3),
                bytes_must_move=must_move, bytes_requested=does_move, must_move_bytes_per_s=must_move / (med(t_ex) * 1e-3),
                requested_bytes_per_s=does_move / (med(t_ex) * 1e-3), copy_ms=med(t_copy), copy_bytes_per_s=copy_rate,
                must_move_fraction_of_copy_rate=must_move / (med(t_ex) * 1e-3) / copy_rate, exceedance_ms_all=[round(v, 4) for v in t_ex],
                error_estimate_ms_all=[round(v, 4) for v in t_ee], copy_ms_all=[round(v, 4) for v in t_copy])
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
