"""The planted cohort of the monitoring command line (tests/test_gpu_monitor_cli.py) -- TEST INFRASTRUCTURE.  Three patients,
each with a tumour (heterozygous variants at 60 % purity: where the list comes from, not a file of sample_dir), a list of 14 somatic variants (one line of patient 0's list is written twice: the cell counts twice) and two
plasma files at tumour fractions 0.3 % and 0.15 % -- below what a single cell shows --, three unrelated samples, a header-only file;
300 positions at 2500-3500 reads per strand, every alternative base at 0.05 % background; an error table written as text with
thresholds between 0.0006 and 0.0012."""
import functools

import numpy as np

SEED = 24
START = 5000
P = 300
N_VAR = 14
FRACTIONS = (0.003, 0.0015)
ASEQ_HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"


@functools.lru_cache(maxsize=None)
def planted(seed=SEED):
    """-> ref uint8 [P], thr [2][4][P], samples {name: int32 [P][8]}, lists {name: [(p, y)]}, assign [(sample, list)], tumours {name: [P][8]}"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, P).astype(np.uint8)
    thr = rng.uniform(0.0006, 0.0012, (2, 4, P))

    def sample(variants=(), fraction=0.0):
        depth = rng.integers(2500, 3501, size=(P, 2))
        frac = np.full((P, 4), 0.0005)
        for p, y in variants:
            frac[p, y] += fraction / 2  # heterozygous in the tumour
        recs = np.zeros((P, 8), np.int64)
        for st in range(2):
            alt = rng.binomial(depth[:, st, None], frac)
            alt[np.arange(P), ref] = 0
            recs[:, st * 4:st * 4 + 4] = alt
            recs[np.arange(P), st * 4 + ref] = depth[:, st] - alt.sum(-1)
        return recs.astype(np.int32)

    order = rng.permutation(P)
    samples, tumours, lists, assign = {}, {}, {}, []
    for k in range(3):
        var = [(int(p), int((ref[p] + 1 + rng.integers(3)) % 4)) for p in order[k * N_VAR:(k + 1) * N_VAR]]
        lists[f"PAT{k}"] = var + ([var[0]] if k == 0 else [])
        tumours[f"TUM{k}"] = sample(var, 0.6)  # where the list came from: not a sample to monitor
        for j, f in enumerate(FRACTIONS):
            samples[f"PLA{k}_{j}"] = sample(var, f)
            assign.append((f"PLA{k}_{j}", f"PAT{k}"))
    for k in range(3):
        samples[f"OTHER{k}"] = sample()
    return ref, thr, samples, lists, assign, tumours


def write_cohort(d):
    """the cohort as files under d (pathlib): table.txt, S/ (every sample and EMPTY, a header-only file), variants.txt, assign.txt"""
    ref, thr, samples, lists, assign, _ = planted()
    text = "chrom\tposition\treference\tduplicate\tThres_A\tThres_C\tThres_G\tThres_T\tGerm_Max_A\tGerm_Max_C\tGerm_Max_G\tGerm_Max_T\n"
    for p in range(P):
        cells = ["-2_-2" if y == ref[p] else f"{thr[0, y, p]:.6f}_{thr[1, y, p]:.6f}" for y in range(4)]
        germ = ["-" if y == ref[p] else "0" for y in range(4)]
        text += f"chr7\t{START + p}\t{'ACGT'[ref[p]]}\tNO\t" + "\t".join(cells) + "\t" + "\t".join(germ) + "\n"
    (d / "table.txt").write_text(text)
    (d / "S").mkdir()
    for name, recs in samples.items():
        out = ASEQ_HEADER
        for p in range(P):
            r = recs[p].astype(np.int64)
            tot = r[:4] + r[4:]
            out += f"chr7\t{START + p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        (d / "S" / f"{name}.PILEUP.ASEQ").write_text(out)
    (d / "S" / "EMPTY.PILEUP.ASEQ").write_text(ASEQ_HEADER)
    (d / "variants.txt").write_text("".join(f"{name}\tchr7\t{START + p}\t{'ACGT'[ref[p]]}\t{'ACGT'[y]}\n" for name, var in lists.items() for p, y in var))
    (d / "assign.txt").write_text("".join(f"{s}\t{l}\n" for s, l in assign))
    return lists, assign
