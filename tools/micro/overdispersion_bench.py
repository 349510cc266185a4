"""The three kernels of overdispersion-aware calling beside the parent's comparable passes.

Config 3's shape by default: 256 synthetic normals, 96 synthetic tumours, 100 000 positions, uint16 records.  Every repetition is cold
for the caches (256 MiB written in between), bracketed by HIP events, the kinds alternated in one process:
  * ampli_nb_score_records with omega NULL and with the panel's fitted omega, beside poisson_call in its all-scores mode (POISSON_FULL
    with dense Q) over the same tumours -- the parent's pass that scores every cell;
  * ampli_overdispersion_records beside ampli_dispersion_records over the same normals (both stream the cohort once);
  * ampli_overdispersion_finalize.
The synthetic panel's background is close to Poisson, so few of its cells are HIGH; --omega F plants omega = F in every cell for a
fourth timing of the score (every tail a negative-binomial one).  Nobody measured kernels of this form before, so no expectation is
asserted.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py.
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
    ap.add_argument("--omega", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import POISSON_FULL

    ctx = Context(0)
    P, T, S = a.P, a.T, a.S
    normals, fits = ctx.pack(ctx.synth_fill(P, S), "u16")
    assert fits
    tumours, fits = ctx.pack(ctx.synth_fill(P, T, tumour=True), "u16")
    assert fits
    ref = ctx.synth_ref(P)
    rn, rt = ctx.records(normals, "u16", S), ctx.records(tumours, "u16", T)
    ctx.set_record_layout("u16")
    table = ctx.error_estimate(normals, P, 0.002, 100)
    acc0 = ctx.new_acc(P)
    ctx.error_reduce_records(rn, P, acc0, 0.0, 100, summary=True)
    disp = ctx.panel_dispersion([rn], P, acc0, 100, 4.0, samples=False)
    s2 = ctx.overdispersion_sums(rn, P, acc0, 100)
    omega = ctx.overdispersion_fit(P, acc0, disp["x2"], s2, disp["status"])
    planted = torch.full((2, 4, P), a.omega, dtype=torch.float64, device=ctx.device)
    q = ctx.nb_score(rt, P, table.thr, ref, None, 100)
    full = ctx.poisson_call(tumours, P, table.thr, ref, 100, mode=POISSON_FULL, dense_q=True)
    torch.cuda.synchronize()
    evaluated = float((q[..., 0] != -1).float().mean().item())
    scored = float(((q[..., 0] != -1) & (q[..., 0] != 0)).float().mean().item())
    fitted = int((omega > 0).sum().item())

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    kinds = {
        "nb_score_poisson": lambda: ctx.nb_score(rt, P, table.thr, ref, None, 100, q=q),
        "nb_score_fitted": lambda: ctx.nb_score(rt, P, table.thr, ref, omega, 100, q=q),
        "nb_score_planted": lambda: ctx.nb_score(rt, P, table.thr, ref, planted, 100, q=q),
        "poisson_full": lambda: ctx.poisson_call(tumours, P, table.thr, ref, 100, mode=POISSON_FULL, call_mask=full["call_mask"], q=full["q"]),
        "overdispersion_records": lambda: ctx.overdispersion_sums(rn, P, acc0, 100, s2=s2),
        "dispersion_records": lambda: ctx.dispersion_records(rn, P, acc0, 100, disp["x2"], disp["rinv"]),
        "overdispersion_finalize": lambda: ctx.overdispersion_fit(P, acc0, disp["x2"], s2, disp["status"], omega=omega),
    }
    times = {k: [] for k in kinds}
    for _ in range(a.reps):
        for k, fn in kinds.items():
            times[k].append(timed(fn))
    med = statistics.median
    line = dict(kind="overdispersion_bench", P=P, T=T, S=S, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                evaluated_fraction=evaluated, scored_fraction=scored, cells_fitted=fitted, planted_omega=a.omega)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
    line["ratio_nb_score_poisson_over_poisson_full"] = med(times["nb_score_poisson"]) / med(times["poisson_full"])
    line["ratio_nb_score_fitted_over_poisson_full"] = med(times["nb_score_fitted"]) / med(times["poisson_full"])
    line["ratio_nb_score_planted_over_poisson_full"] = med(times["nb_score_planted"]) / med(times["poisson_full"])
    line["ratio_overdispersion_records_over_dispersion_records"] = med(times["overdispersion_records"]) / med(times["dispersion_records"])
    line["overdispersion_records_bytes_per_s"] = S * P * 16 / (med(times["overdispersion_records"]) * 1e-3)
    line["nb_score_poisson_cells_per_s"] = T * P * 8 / (med(times["nb_score_poisson"]) * 1e-3)
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
