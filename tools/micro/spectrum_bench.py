"""The substitution spectrum kernel against one error_estimate on the same resident records.

Config 3's shape by default: 256 synthetic normals x 100 000 positions, uint16 records resident in one buffer, the synthetic panel's
reference codes, 68 classes drawn uniformly.  Every repetition is cold for the caches (256 MiB written in between), bracketed by HIP
events, the kinds alternated in one process: ampli_spectrum_records, error_estimate (the parent's kernel, unchanged) and a
device-to-device copy of the record buffer (the box's copy rate, read + written bytes).  A second class array with every position in
one class gives the kernel's time under the worst same-address serialisation.  The figure of merit is spectrum_ms /
error_estimate_ms; nobody measured a kernel of this form before, so no expectation is asserted.  One JSON line on stdout; --out also
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
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--classes", type=int, default=68)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import SPEC_SITES

    ctx = Context(0)
    P, S, NC = a.P, a.S, a.classes
    normals32 = ctx.synth_fill(P, S)
    normals, fits = ctx.pack(normals32, "u16")
    assert fits
    del normals32
    ctx.set_record_layout("u16")
    rec = ctx.records(normals, "u16", S)
    ref = ctx.synth_ref(P)
    cls = torch.from_numpy(np.random.default_rng(17).integers(0, NC, P).astype(np.uint8)).to(ctx.device)
    one = torch.zeros((P,), dtype=torch.uint8, device=ctx.device)
    sums = ctx.spectrum(rec, P, ref, cls, NC)
    segments = ctx.last_spectrum_segments()
    sums_one = ctx.spectrum(rec, P, ref, one, NC)
    table = ctx.error_estimate(normals, P, 0.002, 100)
    copy = torch.empty_like(normals)
    torch.cuda.synchronize()
    s, s1 = sums.cpu().numpy(), sums_one.cpu().numpy()
    entering = int(s[:, :, SPEC_SITES].sum())
    assert entering > 0 and (s.sum(1) == s1[:, 0]).all() and not s1[:, 1:].any()  # the same records enter, whatever their classes

    t0, t1 = ctx.event(), ctx.event()
    scratch = torch.empty((256 << 20,), dtype=torch.uint8, device=ctx.device)  # 256 MiB written between reps: no warm L2 / MALL

    def timed(fn):
        scratch.fill_(1)
        ctx.record(t0)
        fn()
        ctx.record(t1)
        return ctx.elapsed_ms(t0, t1)

    t_spec, t_one, t_ee, t_copy = [], [], [], []
    for _ in range(a.reps):
        t_spec.append(timed(lambda: ctx.spectrum(rec, P, ref, cls, NC, out=sums)))
        t_ee.append(timed(lambda: ctx.error_estimate(normals, P, 0.002, 100, out=table)))
        t_copy.append(timed(lambda: copy.copy_(normals)))
        t_one.append(timed(lambda: ctx.spectrum(rec, P, ref, one, NC, out=sums_one)))
    med = statistics.median
    rec_bytes = S * P * 16
    copy_rate = 2 * rec_bytes / (med(t_copy) * 1e-3)
    spec_rate = (rec_bytes + 2 * P * ((S + 3) // 4) + S * NC * 72) / (med(t_spec) * 1e-3)  # records, the two byte arrays per strip, the sums
    line = dict(kind="spectrum_bench", P=P, S=S, classes=NC, layout="u16", reps=a.reps, device=torch.cuda.get_device_properties(0).name,
                segments=segments, entering_fraction=entering / (S * P),
                spectrum_ms=med(t_spec), spectrum_ms_min=min(t_spec), spectrum_ms_max=max(t_spec), error_estimate_ms=med(t_ee),
                error_estimate_ms_min=min(t_ee), error_estimate_ms_max=max(t_ee), ratio_spectrum_over_error_estimate=med(t_spec) / med(t_ee),
                one_class_ms=med(t_one), one_class_ms_min=min(t_one), ratio_one_class_over_error_estimate=med(t_one) / med(t_ee),
                record_bytes=rec_bytes, copy_ms=med(t_copy), copy_bytes_per_s=copy_rate, spectrum_bytes_per_s=spec_rate,
                spectrum_fraction_of_copy_rate=spec_rate / copy_rate, spectrum_ms_all=[round(v, 4) for v in t_spec],
                one_class_ms_all=[round(v, 4) for v in t_one], error_estimate_ms_all=[round(v, 4) for v in t_ee])
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
