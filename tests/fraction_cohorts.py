"""The planted cohort of the tumour-fraction command line (tests/test_gpu_fraction_cli.py) -- TEST INFRASTRUCTURE.  The shape of
the monitoring cohort (tests/monitor_cohorts.py: 300 positions at 2500-3500 reads per strand, every alternative base at 0.05 %
background), but the error table's thresholds EQUAL the true background -- the fraction is the one above the table's rates --, every
variant carries a weight in 0.2-0.6, and each of three patients has three draws, at tumour fractions 0.3 %, 0.1 % and 0 %: a listed
variant's allele fraction in a draw is the background plus fraction x weight.  One line of patient 0's list is written twice (the cell
counts twice); three unrelated samples and a header-only file complete the directory.

The seed is chosen on the model (python -m tests.fraction_cohorts tries seeds in order and prints the first that qualifies): every planted
fraction lies inside its interval, the change from 0.3 % to 0.1 % is FALLING in all three patients, and no comparison of F_LO, F_HI or a
verdict is decided by less than 1e-9 relative.  tests/test_gpu_fraction_cli.py asserts all three on the model."""
import functools

import numpy as np

from tests.monitor_cohorts import ASEQ_HEADER

SEED = 1
START = 5000
P = 300
N_VAR = 14
FRACTIONS = (0.003, 0.001, 0.0)
BACKGROUND = 0.0005


@functools.lru_cache(maxsize=None)
def planted(seed=SEED):
    """-> ref uint8 [P], samples {name: int32 [P][8]}, lists {name: [(p, y, weight text)]}, assign [(sample, list)], truth {sample: fraction}"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, P).astype(np.uint8)

    def sample(variants=(), fraction=0.0):
        depth = rng.integers(2500, 3501, size=(P, 2))
        frac = np.full((P, 4), BACKGROUND)
        for p, y, w in variants:
            frac[p, y] += fraction * float(np.float32(w))
        recs = np.zeros((P, 8), np.int64)
        for st in range(2):
            alt = rng.binomial(depth[:, st, None], frac)
            alt[np.arange(P), ref] = 0
            recs[:, st * 4:st * 4 + 4] = alt
            recs[np.arange(P), st * 4 + ref] = depth[:, st] - alt.sum(-1)
        return recs.astype(np.int32)

    order = rng.permutation(P)
    samples, lists, assign, truth = {}, {}, [], {}
    for k in range(3):
        var = [(int(p), int((ref[p] + 1 + rng.integers(3)) % 4), f"{rng.uniform(0.2, 0.6):.4f}") for p in order[k * N_VAR:(k + 1) * N_VAR]]
        lists[f"PAT{k}"] = var + ([var[0]] if k == 0 else [])
        for j, f in enumerate(FRACTIONS):
            samples[f"PLA{k}_{j}"] = sample(var, f)
            assign.append((f"PLA{k}_{j}", f"PAT{k}"))
            truth[f"PLA{k}_{j}"] = f
    for k in range(3):
        samples[f"OTHER{k}"] = sample()
    return ref, samples, lists, assign, truth


def thresholds():
    """float32 [2][4][P] as the table's text gives them: the true background everywhere"""
    return np.full((2, 4, P), np.float32(f"{BACKGROUND:.6f}"), np.float32)


def write_cohort(d, seed=SEED):
    """the cohort as files under d (pathlib): table.txt, S/ (every sample and EMPTY, a header-only file), variants.txt, assign.txt"""
    ref, samples, lists, assign, _ = planted(seed)
    text = "chrom\tposition\treference\tduplicate\tThres_A\tThres_C\tThres_G\tThres_T\tGerm_Max_A\tGerm_Max_C\tGerm_Max_G\tGerm_Max_T\n"
    for p in range(P):
        cells = ["-2_-2" if y == ref[p] else f"{BACKGROUND:.6f}_{BACKGROUND:.6f}" for y in range(4)]
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
    (d / "variants.txt").write_text("".join(f"{name}\tchr7\t{START + p}\t{'ACGT'[ref[p]]}\t{'ACGT'[y]}\t{w}\n" for name, var in lists.items() for p, y, w in var))
    (d / "assign.txt").write_text("".join(f"{s}\t{l}\n" for s, l in assign))
    return lists, assign


def model_of(seed=SEED, cov=100, min_variants=5, z2=None):
    """the model over the planted records themselves (what the command reads back from the text is the same integers): names, list names,
    own pairs, est, count, the CSR"""
    from tests import fraction_model as fm

    ref, samples, lists, assign, truth = planted(seed)
    names, lnames = sorted(samples), list(lists)
    recs = np.stack([samples[n] for n in names])
    off = np.concatenate([[0], np.cumsum([len(lists[n]) for n in lnames])]).astype(np.uint32)
    cell = np.array([4 * p + y for n in lnames for p, y, _ in lists[n]], np.uint32)
    w = np.array([np.float32(t) for n in lnames for _, _, t in lists[n]], np.float32)
    est, count = fm.fraction_model(recs, P, thresholds(), ref, off, cell, w, cov, 1000, fm.Z2_95 if z2 is None else z2)
    own = [(names.index(s), lnames.index(l)) for s, l in assign]
    return names, lnames, own, est, count, (off, cell, w)


MARGIN = 1e-9


def margins_ok(own, est, count, min_variants=5):
    """no comparison that decides a verdict or a change lies within MARGIN relative: F_LO against 0 is exact (a bisection that ran gives a
    value above 2^-61), N_EVAL against min_variants is an integer comparison; the changes compare F_LO_B with F_HI_A and F_HI_B with F_LO_A"""
    from tests import fraction_model as fm

    for k in range(1, len(own)):
        (sa, la), (sb, lb) = own[k - 1], own[k]
        if la != lb:
            continue
        a, b = est[sa, lb], est[sb, lb]
        for x, y in ((b[fm.F_LO], a[fm.F_HI]), (b[fm.F_HI], a[fm.F_LO])):
            if x != y and abs(x - y) <= MARGIN * max(abs(x), abs(y)):
                return False
    return True


def qualifies(seed):
    from tests import fraction_model as fm

    names, lnames, own, est, count, _ = model_of(seed)
    truth = planted(seed)[4]
    inside = all(est[s, l, fm.F_LO] <= truth[names[s]] <= est[s, l, fm.F_HI] for s, l in own)
    verdicts = [fm.verdict(count[s, l, 0], est[s, l, 0], est[s, l, 1], 5) for s, l in own]
    falling = all(fm.change(verdicts[3 * k], est[own[3 * k]], verdicts[3 * k + 1], est[own[3 * k + 1]])[0] == fm.FALLING for k in range(3))
    return inside and falling and margins_ok(own, est, count)


if __name__ == "__main__":
    for seed in range(1, 200):
        if qualifies(seed):
            print("seed", seed)
            break
