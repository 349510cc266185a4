"""The cohorts of the in-silico dilution tests (tests/test_dilution_host.py, tests/test_gpu_dilution*.py) -- TEST
INFRASTRUCTURE.  dispersion_cohorts' record shapes -- absent records, positions listed twice (E > 0), an RD plane -- with counts
placed on the edges of a Philox block (4 reads) and of a round of 64 lanes (256 reads), and mixture lists that use a row several times,
down-sample without a diluent and put the thresholds on 0, 1, 2^32 - 1 and 2^32.  Every case is modelled once and shared, read only."""
import functools

import numpy as np

from tests.dilution_model import ABSENT, BAD_COUNT, BAD_MIXTURE, KEEP_ALL, MAX_COUNT, dilute_model, keep_of
from tests.dispersion_cohorts import cohort

ROWS_A, ROWS_B = 6, 5
EDGE_COUNTS = (0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513)
SHAPES = [(1, 1), (63, 3), (64, 5), (65, 9), (130, 9), (1000, 3)]
FRACTIONS = (0.1, 0.5, 0.02, 0.9, 0.004, 0.25, 0.7, 0.05, 0.33)


def _edged(c, P, rng):
    """the cohort with every edge count written into the primary records: a third of the present cells of the first max(1, P // 8)
    positions of every row"""
    recs = c[0].copy()
    k = max(1, P // 8)
    for s in range(recs.shape[0]):
        for p in range(k):
            if recs[s, p, 0] == ABSENT:
                continue
            for f in range(8):
                if rng.random() < 0.34:
                    recs[s, p, f] = EDGE_COUNTS[int(rng.integers(len(EDGE_COUNTS)))]
    if recs[0, 0, 0] == ABSENT:
        recs[0, 0] = 0
    recs[0, 0, :8] = EDGE_COUNTS[3:11]  # whatever the draw gave: row 0 of position 0 holds eight of them
    return (recs,) + tuple(c[1:])


def mixtures(kind, n_mix, rng):
    """(row_a, row_b, keep_a, keep_b, key): kind same -- both rows of chunk A; different -- a row of A and a row of B.  Every fourth
    mixture down-samples (row_b -1); mixtures 1, 2 and 4 put the thresholds on their edges; with more mixtures than rows a row occurs
    in several"""
    n_b = ROWS_A if kind == "same" else ROWS_B
    out = []
    for i in range(n_mix):
        x = FRACTIONS[i % len(FRACTIONS)]
        keep_a, keep_b = keep_of(x), keep_of(1.0 - x)
        if i == 1:
            keep_a, keep_b = KEEP_ALL - 1, 1
        elif i == 2:
            keep_a, keep_b = 0, KEEP_ALL
        elif i == 4:
            keep_a, keep_b = KEEP_ALL, 0
        row_b = -1 if i % 4 == 3 else (2 * i + 1) % n_b
        out.append((i % ROWS_A, row_b, keep_a, keep_b, int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))))
    return out


@functools.lru_cache(maxsize=None)
def case(P, n_mix, kind):
    """A, B (cohort tuples: recs [S][P+E][8], E, dup_off, ext_pos, rd), the mixtures and the model's (out, flags)"""
    rng = np.random.default_rng(22 * P + n_mix)
    A = _edged(cohort(P, ROWS_A, 3 * P + n_mix, extras=True, own_rd=True, u16=True), P, rng)
    B = _edged(cohort(P, ROWS_B, 5 * P + n_mix + 1, extras=True, own_rd=True, u16=True), P, rng) if kind == "different" else A
    mix = mixtures(kind, n_mix, rng)
    out, flags = dilute_model(A[0], B[0], P, mix)
    assert not flags.any()
    for t in (out, flags):
        t.setflags(write=False)
    return A, B, mix, out, flags


P_SPECIAL = 6
BAD_LIST = [(2, -1), (-1, -1), (0, 2), (0, -2), (-2 ** 31, -1), (0, 2 ** 31 - 1)]  # rows outside their chunk, row_b below -1


@functools.lru_cache(maxsize=None)
def special():
    """an int32 chunk of two rows and six positions.  Row 0: one cell of 2^24 - 2 reads -- the longest loop there is --, edge counts, an
    absent record.  Row 1: a cell of 2^24 - 1, a negative count, a count of 2^31 - 1, a negative count in field 0 that is not ABSENT.
    Mixtures: 0 draws the long cell once; 1 takes all of row 0 (no draw) and thins row 1 -- BAD_COUNT; 2 down-samples row 1; then the
    bad mixtures (BAD_LIST, a keep_a and a keep_b above 2^32).  Returns recs, mixtures, out, flags."""
    recs = np.zeros((2, P_SPECIAL, 8), np.int32)
    recs[0, 0] = [MAX_COUNT, 5, 0, 1, 300, 2, 0, 0]
    recs[0, 1] = [700, 3, 256, 1, 513, 0, 4, 255]
    recs[0, 2] = [1000, 1, 1, 1, 1000, 1, 1, 1]
    recs[0, 3] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
    recs[0, 4] = [40, 0, 0, 0, 41, 0, 0, 0]
    recs[0, 5] = [400, 0, 9, 0, 410, 0, 8, 0]
    recs[1, 0] = [100, 2, 0, 0, 100, 1, 0, 0]
    recs[1, 1] = [500, 0, 0, MAX_COUNT + 1, 500, 0, 0, 0]
    recs[1, 2] = [500, 0, 0, 0, 500, -1, 0, 0]
    recs[1, 3] = [500, 2 ** 31 - 1, 0, 0, 500, 0, 0, 0]  # a's record is absent here: the bad count still raises the flag
    recs[1, 4] = [-7, 0, 0, 0, 100, 0, 0, 0]
    recs[1, 5] = [600, 1, 0, 0, 600, 0, 2, 0]
    key = 0xC0FFEE0DDBA11AD5
    mix = [(0, -1, keep_of(0.3), 0, key), (0, 1, KEEP_ALL, keep_of(0.5), key + 1), (1, -1, keep_of(0.5), KEEP_ALL, key + 2)]
    mix += [(a, b, keep_of(0.5), keep_of(0.5), key) for a, b in BAD_LIST]
    mix += [(0, -1, KEEP_ALL + 1, 0, key), (0, -1, 5, KEEP_ALL + 1, key), (0, 1, 2 ** 64 - 1, 5, key)]
    out, flags = dilute_model(recs, recs, P_SPECIAL, mix)
    assert list(flags[:3]) == [0, BAD_COUNT, BAD_COUNT] and (flags[3:] == BAD_MIXTURE).all() and (out[3:, :, 0] == ABSENT).all()
    assert (out[1, (1, 2, 3, 4), 0] == ABSENT).all() and (out[1, (0, 5), 0] != ABSENT).all() and out[0, 3, 0] == ABSENT
    for t in (out, flags):
        t.setflags(write=False)
    return recs, mix, out, flags


# ---- the planted cohort of the command line (tests/test_gpu_dilution_cli.py) -------------------------------------------------
SERIES_SEED = 22
SERIES_START = 1000
FRACTIONS_CLI = (0.5, 0.2, 0.1, 0.04, 0.02)
ASEQ_HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"


@functools.lru_cache(maxsize=None)
def planted_series(seed=SERIES_SEED, P=200):
    """24 normals for the table, two tumours (TUM0, TUM1) at 4500-7500 reads per strand with six variants each at 5 % on both strands,
    two diluent normals (DIL0, DIL1); every alternative base at 0.1 % background.  Returns normals [24][P][8], samples {name: [P][8]},
    ref uint8 [P], the reference letters as written (N and lower-case among them) and the variants [(tumour, position, base)]."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, P).astype(np.uint8)

    def files(n, variants=()):
        depth = rng.integers(4500, 7501, size=(n, P, 2))
        frac = np.full((n, P, 4), 0.001)
        for t, p, y in variants:
            frac[t, p, y] = 0.05
        recs = np.zeros((n, P, 8), np.int64)
        for st in range(2):
            alt = rng.binomial(depth[:, :, st, None], frac)
            alt[:, np.arange(P), ref] = 0
            recs[:, :, st * 4:st * 4 + 4] = alt
            recs[:, np.arange(P), st * 4 + ref] = depth[:, :, st] - alt.sum(-1)
        return recs.astype(np.int32)

    letters = ["ACGT"[r] for r in ref]
    odd = [int(p) for p in rng.choice(P, 6, replace=False)]
    for p in odd[:3]:
        letters[p] = "N"
    for p in odd[3:]:
        letters[p] = letters[p].lower()
    free = [p for p in rng.permutation(P) if p not in odd]
    variants = [(t, int(free[t * 6 + i]), int((ref[free[t * 6 + i]] + 1 + rng.integers(3)) % 4)) for t in range(2) for i in range(6)]
    normals = files(24)
    tumours = files(2, variants)
    diluents = files(2)
    samples = {"TUM0": tumours[0], "TUM1": tumours[1], "DIL0": diluents[0], "DIL1": diluents[1]}
    return normals, samples, ref, letters, variants


def series_lines():
    """per pair the five fractions and one down-sampling line; one line with a scale; one against the header-only file"""
    out = []
    for k in range(2):
        out += [(f"TUM{k}", f"DIL{k}", f, 1.0) for f in FRACTIONS_CLI] + [(f"TUM{k}", "-", 0.1, 1.0)]
    return out + [("TUM0", "DIL1", 0.5, 0.5), ("TUM0", "EMPTY", 0.5, 1.0)]


def write_series(d, P=200):
    """the cohort as files under d (pathlib): p.bed (two amplicons that share ten positions, so ten positions are listed twice), r.txt,
    N/ (the normals), S/ (the tumours, the diluents and EMPTY, a header-only file), mixtures.txt"""
    normals, samples, ref, letters, variants = planted_series()
    half = P // 2 + 5
    walk = list(range(half)) + list(range(half - 10, P))
    (d / "p.bed").write_text(f"chr7\t{SERIES_START}\t{SERIES_START + half - 1}\ta1\tb1\tg1\nchr7\t{SERIES_START + half - 10}\t{SERIES_START + P - 1}\ta2\tb2\tg2\n")
    (d / "r.txt").write_text("".join(f"chr7\t{SERIES_START + p}\t{letters[p]}\n" for p in walk))

    def aseq(path, recs):
        text = ASEQ_HEADER
        for p in walk:
            r = recs[p].astype(np.int64)
            tot = r[:4] + r[4:]
            text += f"chr7\t{SERIES_START + p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        path.write_text(text)

    (d / "N").mkdir()
    (d / "S").mkdir()
    for s in range(normals.shape[0]):
        aseq(d / "N" / f"NORM{s:02d}.PILEUP.ASEQ", normals[s])
    for name, recs in samples.items():
        aseq(d / "S" / f"{name}.PILEUP.ASEQ", recs)
    (d / "S" / "EMPTY.PILEUP.ASEQ").write_text(ASEQ_HEADER)
    (d / "mixtures.txt").write_text("".join(f"{a}\t{b}\t{f:g}" + ("" if s == 1.0 else f"\t{s:g}") + "\n" for a, b, f, s in series_lines()))
    return variants
