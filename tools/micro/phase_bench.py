"""The read-phasing counting kernel beside the read-evidence counting kernel, the walk whose merge it shares, on the same
stream of alignment records and the same list.

The stream is tools/pileup_bench.py's and tools/micro/evidence_bench.py's: 2 M reads of 120 bases on 400 amplicons of one chromosome,
every read of an amplicon starting at its start, one `120M` operation per read, qualities 15 .. 40, both strands (same generator, same
seed).  Kinds of call, alternated in one process, each repetition bracketed by HIP events after a warm-up of every kind; for each list
ampli_pileup_phase and the yardstick ampli_pileup_evidence:
  * one:   one listed position per amplicon -- no pair forms inside a read: the cost of the walk alone;
  * four:  four listed positions per amplicon -- six cells per read, all in the LDS window;
  * dense: every panel position (the global-atomic path: expected to be slow; fewer repetitions);
then the stream of --identical identical reads over two listed keys (every increment in one cell).  The tables are checked against the
invariant of DESIGN 32.1 (row and column sums of every cell whose two keys the same reads cover equal the pileup counts; every other
cell is zero) before anything is timed.  Reported: milliseconds (median, min, max, all), the spread of each kind, and the ratios over the
yardstick with their ranges.  No time is fixed in advance.  One JSON line on stdout; --out also writes it.  Not a replacement for bench.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from indel_bench import records  # noqa: E402  (the generator of the shared stream)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=120)
    ap.add_argument("--identical", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--reps-dense", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    from amplisolve_amd import Context, read_phase
    from amplisolve_amd.api import PHASE_PARTNERS as K
    from amplisolve_amd.api import PHASE_STATES as S

    N, L = a.reads, a.read_len
    rng = np.random.default_rng(1)
    n_amp = 400
    amp_start = 10_000 + np.arange(n_amp) * 2_000
    amp = np.sort(rng.integers(0, n_amp, N))
    flags = (rng.integers(0, 2, N) * 0x10).astype(np.uint16)
    plain = records(np, rng, N, L, [(0, L)], amp_start[amp] - 1, flags)
    raw = plain.tobytes()
    offs = np.arange(N, dtype=np.int64) * plain.dtype.itemsize
    same = np.repeat(plain[:1], a.identical)
    raw_same = same.tobytes()
    offs_same = np.arange(a.identical, dtype=np.int64) * plain.dtype.itemsize
    key_same = int(plain["pos"][0]) + 1 + np.asarray([L // 3, 2 * L // 3], np.int64)
    del plain, same

    ctx = Context(0)
    up = lambda b: torch.frombuffer(bytearray(b + bytes(64)), dtype=torch.uint8).cuda()  # noqa: E731
    d_bam, off = up(raw), torch.from_numpy(offs).cuda()
    d_same, off_same = up(raw_same), torch.from_numpy(offs_same).cuda()
    lists = {"one": (amp_start + L // 2)[:, None], "four": amp_start[:, None] + (L // 5) * np.arange(1, 5)[None, :], "dense": amp_start[:, None] + np.arange(L + 8)[None, :]}
    zeros = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")  # noqa: E731
    keys, table, hist, counts, st = {}, {}, {}, {}, {}
    for name, pos in list(lists.items()) + [("identical", key_same[None, :])]:
        keys[name] = torch.from_numpy(np.ascontiguousarray(pos.reshape(-1).astype(np.int64))).cuda()  # ref id 0 << 32 | pos
        P = keys[name].numel()
        table[name], hist[name], counts[name] = zeros(P, K, S, S), zeros(P, 4, 3, 64), zeros(P, 8)
        st[name] = dict(p=zeros(3, dtype=torch.int64), e=zeros(2, dtype=torch.int64), c=zeros(2, dtype=torch.int64))

    def stream(name):
        return (d_same, off_same) if name == "identical" else (d_bam, off)

    def phase(name):
        read_phase(ctx, *stream(name), keys[name], 20, 20, table=table[name], stats=st[name]["p"])

    def evidence(name):
        ctx.read_evidence(*stream(name), keys[name], 20, 20, hist=hist[name], stats=st[name]["e"])

    def pileup(name):
        bam, o = stream(name)
        ctx._check(ctx.lib.ampli_pileup_count(ctx.h, bam.data_ptr(), o.data_ptr(), int(o.numel()), keys[name].data_ptr(), int(keys[name].numel()), 20, 20,
                                              counts[name].data_ptr(), st[name]["c"].data_ptr()))

    # one call of each, checked: the invariant of every cell whose two keys the same reads cover; every other cell is zero
    cells = {}
    for name in keys:
        phase(name), evidence(name), pileup(name)
        torch.cuda.synchronize()
        pos = keys[name].cpu().numpy()
        P = len(pos)
        first = amp_start[0] if name != "identical" else pos[0]
        a_of = (pos - first) // 2_000
        covered = (pos - first) % 2_000 < L if name != "identical" else np.ones(P, bool)
        i, k = np.meshgrid(np.arange(P), np.arange(K), indexing="ij")
        j = np.minimum(i + 1 + k, P - 1)
        both = (i + 1 + k < P) & (a_of[i] == a_of[j]) & covered[i] & covered[j]
        t = table[name].cpu().numpy().astype(np.int64)
        c = counts[name].cpu().numpy().astype(np.int64)[:, :4]
        assert not t[~both].any(), name
        assert np.array_equal(t[:, :, :4, :].sum(3)[both], c[i[both]]) and np.array_equal(t[:, :, :, :4].sum(2)[both], c[j[both]]), name
        n_reads = a.identical if name == "identical" else N
        assert st[name]["p"].tolist()[0] == st[name]["e"].tolist()[0] == n_reads and st[name]["p"].tolist()[2] == int(t.sum()), (name, st[name]["p"].tolist())
        cells[name] = st[name]["p"].tolist()[2]
    assert cells["one"] == 0 and cells["four"] == 6 * N and cells["identical"] == a.identical

    t0, t1 = ctx.event(), ctx.event()
    times = {}
    for group, reps in ((("one", "four"), a.reps), (("dense",), a.reps_dense), (("identical",), a.reps)):
        kinds = {f"{fn.__name__}_{name}": (lambda fn=fn, name=name: fn(name)) for name in group for fn in (phase, evidence)}
        for _ in range(a.warmup if group != ("dense",) else 1):
            for fn in kinds.values():
                fn()
        torch.cuda.synchronize()
        for k in kinds:
            times[k] = []
        for _ in range(reps):
            for k, fn in kinds.items():
                ctx.record(t0)
                fn()
                ctx.record(t1)
                times[k].append(ctx.elapsed_ms(t0, t1))
    med = statistics.median
    line = dict(kind="phase_bench", reads=N, read_len=L, amplicons=n_amp, positions={k: int(v.numel()) for k, v in keys.items()}, identical_reads=a.identical,
                record_bytes=len(raw), reps=a.reps, reps_dense=a.reps_dense, warmup=a.warmup, device=torch.cuda.get_device_properties(0).name, cells_per_call=cells)
    for k, v in times.items():
        line[k + "_ms"] = med(v)
        line[k + "_ms_min"] = min(v)
        line[k + "_ms_max"] = max(v)
        line[k + "_ms_all"] = [round(x, 4) for x in v]
        line[k + "_spread"] = (max(v) - min(v)) / med(v)
    for name in keys:
        p, e = times[f"phase_{name}"], times[f"evidence_{name}"]
        line[f"ratio_phase_{name}_over_evidence_{name}"] = med(p) / med(e)
        line[f"ratio_phase_{name}_over_evidence_{name}_range"] = [min(p) / max(e), max(p) / min(e)]
    line["ratio_phase_four_over_phase_one"] = med(times["phase_four"]) / med(times["phase_one"])
    line["ratio_phase_four_over_phase_one_range"] = [min(times["phase_four"]) / max(times["phase_one"]), max(times["phase_four"]) / min(times["phase_one"])]
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
