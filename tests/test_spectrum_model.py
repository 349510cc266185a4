"""The definition of the substitution spectrum (tests/spectrum_model.py) on hand-made records, one per clause of the gate; its additivity
over a split of the positions; the class function on every (l, r, t), at a run's first and last position and at a gap; the 96-channel
fold as a two-to-one map of the 64 x 3 (class, alternative) pairs; every branch of the score at its bound, NaNs included; and the
planted cohort (tests/spectrum_cohorts.py) with its measured margins."""
import itertools

import numpy as np

from tests.spectrum_cohorts import N_NORMALS, NAMES, PLANTED, T_CLEAN, T_DEAM, T_NONE, T_OXFW, T_SHALLOW, T_VAR, TY, planted, planted_results
from tests.spectrum_model import (ABSENT, ALL, ASYMMETRIC, CHANNELS, CLASSES, DEFAULTS, ELEVATED, LOW_SITES, NO_REFERENCE, OK, REF_FEW, REF_OK, SKIP, TYPES,
                                  channel_name, channel_of, class_sums, enters, flag_of, fold, panel_classes, rates, score, spectrum_class, z_of)


def _one(rec, ref=0, cls=5, C=68, cutoff=100, pm=30):
    return bool(enters(np.array(rec, np.int64).astype(np.int32), np.uint8(ref), np.uint8(cls), C, cutoff, pm))


def test_every_clause_of_the_gate():
    good = [500, 0, 0, 0, 500, 0, 0, 0]
    assert _one(good)
    assert not _one([ABSENT, 0, 0, 0, 500, 0, 0, 0])                       # absent
    assert not _one(good, ref=255) and not _one(good, ref=4)               # not a reference base
    assert not _one(good, cls=255) and not _one(good, cls=68) and not _one(good, cls=200) and _one(good, cls=67)
    assert _one(good, cls=5, C=6) and not _one(good, cls=5, C=5) and _one(good, cls=0, C=1) and not _one(good, cls=1, C=1)
    # each strand at cutoff - 1 and at the cutoff
    assert not _one([99, 0, 0, 0, 500, 0, 0, 0]) and _one([100, 0, 0, 0, 500, 0, 0, 0])
    assert not _one([500, 0, 0, 0, 99, 0, 0, 0]) and _one([500, 0, 0, 0, 100, 0, 0, 0])
    assert _one([50, 50, 0, 0, 100, 0, 0, 0], pm=1000) and not _one([50, 49, 0, 0, 100, 0, 0, 0], pm=1000)  # FW is the sum of the four
    # the alternative exactly at max_alt_pm d / 1000 and one read above: d = 1000, 30 d = 30000 = 1000 x 30
    assert _one([485, 15, 0, 0, 485, 15, 0, 0]) and not _one([485, 16, 0, 0, 484, 15, 0, 0])
    assert _one([470, 30, 0, 0, 500, 0, 0, 0]) and not _one([469, 31, 0, 0, 500, 0, 0, 0])                   # both strands' reads count together
    # d = 1010: 30 d = 30300 is no multiple of 1000 -- 30 reads pass (30000 <= 30300), 31 do not (31000 > 30300)
    assert _one([480, 30, 0, 0, 500, 0, 0, 0]) and not _one([479, 31, 0, 0, 500, 0, 0, 0])
    # every alternative on its own, and the reference base's count is free
    assert _one([455, 15, 15, 15, 455, 15, 15, 15]) and not _one([455, 15, 15, 15, 454, 15, 15, 16])
    assert _one([0, 0, 500, 0, 0, 0, 500, 0], ref=2) and not _one([0, 0, 500, 0, 0, 0, 500, 0], ref=0)
    # all or nothing: the gate is per position, not per base
    assert not _one([400, 0, 100, 0, 500, 0, 0, 0])
    # d == 0 passes the last clause: only a positive cut-off stops it
    assert _one([0] * 8, cutoff=0) and not _one([0] * 8, cutoff=1) and _one([0] * 8, cutoff=0, pm=0)
    assert _one(good, pm=0) and not _one([499, 1, 0, 0, 500, 0, 0, 0], pm=0) and _one([1, 499, 0, 0, 0, 500, 0, 0], pm=1000)
    # int32 records near 2^31: the products are formed in int64
    top = (1 << 31) - 1
    assert _one([top, 0, 0, 0, top, 0, 0, 0]) and not _one([top, top, 0, 0, top, 0, 0, 0]) and _one([top, top, top, top, top, top, top, top], pm=1000)


def test_sums_are_what_enters_and_add_over_a_split():
    c = planted()
    recs, ref, cls = c["recs"][:5], c["ref_code"], c["cls"]
    P = c["P"]
    whole = class_sums(recs, ref, cls, CLASSES)
    e = enters(recs, ref[None, :], cls[None, :], CLASSES)
    assert whole.shape == (5, CLASSES, 9) and whole[:, :, 0].sum() == e.sum() and 0 < e.sum() < e.size
    assert whole[:, :, 1:].sum() == recs[e].astype(np.int64).sum()
    for cut in (1, 64, 1000, P - 1):
        a, b = class_sums(recs[:, :cut], ref[:cut], cls[:cut], CLASSES), class_sums(recs[:, cut:], ref[cut:], cls[cut:], CLASSES)
        assert np.array_equal(a + b, whole)
    assert np.array_equal(class_sums(recs, ref, cls, 128)[:, :CLASSES], whole) and not class_sums(recs, ref, cls, 128)[:, CLASSES:].any()
    assert np.array_equal(class_sums(recs, ref, cls, 10), whole[:, :10])              # classes at and above C are skipped, not folded
    assert not class_sums(recs, ref, np.full(P, 255, np.uint8), CLASSES).any()
    assert not whole[:, sorted(set(range(CLASSES)) - set(cls.tolist()))].any()


def test_the_class_function():
    seen = set()
    for r, l, t in itertools.product(range(4), repeat=3):
        c = spectrum_class(r, l, t)
        assert c == 16 * r + 4 * l + t and (c >> 4, (c >> 2) & 3, c & 3) == (r, l, t)
        seen.add(c)
    assert seen == set(range(64))
    for r in range(4):
        assert spectrum_class(r, 255, 2) == spectrum_class(r, 1, 255) == spectrum_class(r, 255, 255) == 64 + r
    assert spectrum_class(255, 0, 0) == spectrum_class(4, 1, 2) == SKIP
    # a run of five, a gap, a lone position, another chromosome with the same coordinates
    pos = [("c1", 10), ("c1", 11), ("c1", 12), ("c1", 13), ("c1", 14), ("c1", 16), ("c2", 11), ("c2", 12), ("c2", 13)]
    bases = dict(zip(pos, ["A", "C", "g", "N", "T", "G", "T", "AC", "C"]))
    ref, cls = panel_classes(pos, bases)
    assert ref.tolist() == [0, 1, 255, 255, 3, 2, 3, 255, 1]
    assert cls.tolist() == [64,                 # the chromosome's first panel position: no left neighbour
                            16 + 4 * 0 + 2,     # A [C] g: the lower-case neighbour counts, upper-cased
                            255,                # a lower-case base is not a reference base
                            255, 64 + 3,        # N; N [T] end of the run
                            64 + 2,             # behind the gap at 15: alone
                            64 + 3, 255, 64 + 1]  # c2: first; a two-letter base; last, and its left neighbour is no base
    # a neighbour that is in the panel under another chromosome only is no neighbour
    assert panel_classes([("c1", 5), ("c2", 6), ("c1", 7)], {("c1", 5): "A", ("c2", 6): "C", ("c1", 7): "G"})[1].tolist() == [64, 65, 66]
    c = planted()
    assert (c["cls"] == 255).sum() == 4 and ((c["cls"] >= 64) & (c["cls"] < 68)).sum() >= 48 and len(set(c["cls"][c["cls"] < 64].tolist())) == 64


def test_the_96_fold_is_two_to_one():
    hits = {}
    for c in range(64):
        r = c >> 4
        for y in range(4):
            if y != r:
                hits.setdefault(channel_of(c, y), []).append((c, y))
    assert sorted(hits) == list(range(CHANNELS)) and all(len(v) == 2 for v in hits.values())
    comp = {0: 3, 1: 2, 2: 1, 3: 0}
    for ch, ((c0, y0), (c1, y1)) in hits.items():  # the two are each other's reverse complement, and one of them is the pyrimidine
        r0, l0, t0 = c0 >> 4, (c0 >> 2) & 3, c0 & 3
        assert (c1 >> 4, (c1 >> 2) & 3, c1 & 3, y1) == (comp[r0], comp[t0], comp[l0], comp[y0])
        assert sorted((r0 in (1, 3), (c1 >> 4) in (1, 3))) == [False, True]
    assert [channel_name(0), channel_name(15), channel_name(16), channel_name(47), channel_name(48), channel_name(95)] == [
        "A[C>A]A", "T[C>A]T", "A[C>G]A", "T[C>T]T", "A[T>A]A", "T[T>G]T"]
    # one read in one cell lands in one type and one channel; an edge class in no channel
    s = np.zeros((1, CLASSES, 9), np.int64)
    s[0, 16 * 2 + 4 * 1 + 3] = [1, 0, 0, 90, 7, 0, 0, 100, 3]  # C [G] T: 7 fw and 3 bw reads of T
    f = fold(s)
    ty = 3 * 2 + 2
    assert f["alt"][0, :, ty].tolist() == [7, 3] and f["dep"][0, :, ty].tolist() == [97, 103] and f["sites"][0, ty] == 1
    assert f["alt"][0, :, ALL].tolist() == [7, 3] and f["dep"][0, :, ALL].tolist() == [97, 103] and f["alt"].sum() == 20
    ch = channel_of(16 * 2 + 4 * 1 + 3, 3)  # the reverse complement: A [C>A] G
    assert channel_name(ch) == "A[C>A]G" and f["ctx_alt"][0, ch] == 10 and f["ctx_dep"][0, ch] == 200 and f["ctx_alt"].sum() == 10
    assert f["ctx_dep"].sum() == 600  # the context's depth under each of its three alternatives
    s = np.zeros((1, CLASSES, 9), np.int64)
    s[0, 64 + 1] = [2, 5, 300, 0, 0, 0, 300, 0, 1]
    f = fold(s)
    assert not f["ctx_alt"].any() and not f["ctx_dep"].any() and f["alt"][0, :, 3].tolist() == [5, 0] and f["alt"][0, :, 5].tolist() == [0, 1]
    assert f["sites"][0].tolist() == [0, 0, 0, 2, 2, 2, 0, 0, 0, 0, 0, 0, 2]


def test_score_branches_at_their_bounds():
    kw = dict(min_sites=200, excess_ratio=3.0, z_cutoff=10.0, asym_delta=0.15)
    nan = float("nan")
    assert flag_of(199, False, 9.0, 99.0, 0.9, 0.5, 99.0, **kw) == LOW_SITES and flag_of(199, True, 9.0, 99.0, 0.9, 0.5, 99.0, **kw) == LOW_SITES
    assert flag_of(200, True, 9.0, 99.0, 0.9, 0.5, 99.0, **kw) == NO_REFERENCE
    assert flag_of(200, False, 3.0, 10.0, 0.5, 0.5, 0.0, **kw) == ELEVATED
    assert flag_of(200, False, 2.999, 99.0, 0.5, 0.5, 0.0, **kw) == OK and flag_of(200, False, 9.0, 9.999, 0.5, 0.5, 0.0, **kw) == OK
    assert flag_of(200, False, 9.0, 99.0, 0.9, 0.5, 99.0, **kw) == ELEVATED  # ELEVATED comes first
    assert flag_of(200, False, 1.0, 0.0, 0.65, 0.5, 10.0, **kw) == ASYMMETRIC and flag_of(200, False, 1.0, 0.0, 0.35, 0.5, -10.0, **kw) == ASYMMETRIC
    assert flag_of(200, False, 1.0, 0.0, 0.64, 0.5, 99.0, **kw) == OK and flag_of(200, False, 1.0, 0.0, 0.9, 0.5, 9.99, **kw) == OK
    for bad in ((nan, 99.0, 0.5, 0.5, 0.0), (9.0, nan, 0.5, 0.5, 0.0), (1.0, 0.0, nan, 0.5, 99.0), (1.0, 0.0, 0.9, nan, 99.0), (1.0, 0.0, 0.9, 0.5, nan)):
        assert flag_of(200, False, *bad, **kw) == OK  # a comparison with NaN is false
    # rates: a strand without depth, no depth at all, no reads at all
    a = np.zeros((2, TYPES), np.int64)
    d = np.zeros((2, TYPES), np.int64)
    a[:, 0], d[:, 0] = [3, 1], [100, 100]
    a[:, 1], d[:, 1] = [3, 0], [100, 0]
    d[:, 2] = [100, 100]
    rate, rate2, asym = rates(a, d)
    assert rate[:, 0].tolist() == [0.03, 0.01] and rate2[0] == 4 / 200 and asym[0] == 0.03 / (0.03 + 0.01)
    assert rate[0, 1] == 0.03 and np.isnan(rate[1, 1]) and rate2[1] == 0.03 and np.isnan(asym[1])
    assert rate2[2] == 0.0 and np.isnan(asym[2]) and np.isnan(rate2[3]) and np.isnan(asym[3])
    assert np.isnan(z_of(1.0, 0.5, 0.0)) and np.isnan(z_of(1.0, 0.5, np.nan)) and z_of(1.0, 0.5, 0.25) == 0.5 / (1.4826 * 0.25)


def _folds(rate2, sites, asym_fw_share=0.5):
    """folds of len(rate2) samples whose type 0 has the given pooled rate at depth 10^6 per strand, and the given sites"""
    S = len(rate2)
    f = dict(alt=np.zeros((S, 2, TYPES), np.int64), dep=np.zeros((S, 2, TYPES), np.int64), sites=np.zeros((S, TYPES), np.int64))
    for s in range(S):
        total = int(round(rate2[s] * 2_000_000))
        f["alt"][s, 0, 0] = int(total * asym_fw_share)
        f["alt"][s, 1, 0] = total - f["alt"][s, 0, 0]
        f["dep"][s, :, 0] = 1_000_000
        f["sites"][s, 0] = sites[s]
    return f


def test_reference_and_status():
    f = _folds([1e-3, 2e-3, 3e-3, 4e-3, 100e-3, 9e-3], [500, 500, 500, 500, 10, 500])
    sc = score(f, 5, min_sites=200, min_normals=4)
    assert sc["n_eff"][0] == 4 and sc["status"][0] == REF_OK          # the normal below min_sites is left out of the reference
    assert sc["ref"][0, 0] == (2e-3 + 3e-3) * 0.5 and sc["ref"][0, 1] == (abs(2e-3 - sc["ref"][0, 0]) + abs(4e-3 - sc["ref"][0, 0])) * 0.5
    assert sc["flag"][4, 0] == LOW_SITES and sc["flag"][5, 0] == OK and sc["ratio"][5, 0] == 9e-3 / 2.5e-3
    assert sc["n_eff"][1] == 0 and sc["status"][1] == REF_FEW and np.isnan(sc["ref"][1]).all() and (sc["flag"][:, 1] == LOW_SITES).all()
    sc = score(f, 5, min_sites=200, min_normals=5)
    assert sc["status"][0] == REF_FEW and sc["flag"][:, 0].tolist() == [NO_REFERENCE] * 4 + [LOW_SITES, NO_REFERENCE]
    sc = score(f, 5, min_sites=1, min_normals=5, excess_ratio=2.5, z_cutoff=1.0)
    assert sc["n_eff"][0] == 5 and sc["ref"][0, 0] == 3e-3 and sc["flag"][4, 0] == ELEVATED and sc["flag"][5, 0] == ELEVATED
    # equal normals: mad == 0, z is NaN and nothing is ELEVATED whatever the ratio
    f = _folds([1e-3] * 5 + [50e-3], [500] * 6)
    sc = score(f, 5)
    assert sc["ref"][0, 1] == 0.0 and np.isnan(sc["z"][:, 0]).all() and sc["ratio"][5, 0] == 50.0 and sc["flag"][5, 0] == OK
    # a reference of zeros: med == 0, the ratio is NaN
    f = _folds([0.0] * 5 + [1e-3], [500] * 6)
    sc = score(f, 5)
    assert sc["ref"][0, 0] == 0.0 and np.isnan(sc["ratio"][:, 0]).all() and np.isnan(sc["asym"][:5, 0]).all() and np.isnan(sc["ref"][0, 2])
    assert (sc["flag"][:, 0] == OK).all()
    # no normals at all
    sc = score(f, 0)
    assert (sc["status"] == REF_FEW).all() and (sc["n_eff"] == 0).all() and (sc["flag"][:, 0] == NO_REFERENCE).all()


def test_planted_cohort_and_its_margins():
    """The bounds of this test and the defaults.  Measured on this cohort: over the clean cells (every cell of the normals, of TCLEAN and
    TVAR, and the unplanted types of TDEAM and TOXFW) the ratio lies in [0.625, 1.261], |z| <= 3.49, |za| <= 4.88 and |asym - med_a| <=
    0.0415; the planted cells have C>T 4.52 (z 21.7), G>A 4.82 (z 18.4) and G>T forward-only ratio 2.40, z 11.1, asym 0.802, za 32.3,
    delta 0.302.  The bounds below are about twice the clean worst; the defaults (excess_ratio 3, z_cutoff 10, asym_delta 0.15) lie
    between them and the planted cells.  An excess_ratio of 2 and a z_cutoff of 5 would not: 2 x 1.26 = 2.5 and 2 x 4.88 = 9.8."""
    c, r = planted(), planted_results()
    sc, f = r["score"], r["fold"]
    assert 2800 < c["P"] < 3200 and sc["flag"].shape == (18, TYPES) and (sc["status"] == REF_OK).all() and (sc["n_eff"] == N_NORMALS).all()
    want = np.zeros((18, TYPES), np.uint8)
    want[T_DEAM, [TY["C>T"], TY["G>A"]]] = ELEVATED
    want[T_OXFW, TY["G>T"]] = ASYMMETRIC
    want[T_SHALLOW] = LOW_SITES
    want[T_NONE] = LOW_SITES
    assert np.array_equal(sc["flag"], want), [(NAMES[s], t) for s, t in zip(*np.nonzero(sc["flag"] != want))]
    clean = want == OK
    clean[[T_DEAM, T_OXFW], ALL] = False  # the planted files' pooled rows carry their planted types
    assert clean[:N_NORMALS].all() and clean[T_CLEAN].all() and clean[T_VAR].all() and clean.sum() == 14 * 13 + 11 + 10
    delta = np.abs(sc["asym"] - sc["ref"][:, 2][None, :])
    print("clean: ratio", sc["ratio"][clean].min(), sc["ratio"][clean].max(), "|z|", np.abs(sc["z"][clean]).max(), "|za|", np.abs(sc["za"][clean]).max(),
          "delta", delta[clean].max())
    assert sc["ratio"][clean].max() < 2.5 and np.abs(sc["z"][clean]).max() < 7.0 and np.abs(sc["za"][clean]).max() < 9.8 and delta[clean].max() < 0.083
    for s, types in PLANTED.items():
        for ty in types:
            print(NAMES[s], ty, sc["ratio"][s, ty], sc["z"][s, ty], sc["asym"][s, ty], sc["za"][s, ty], delta[s, ty])
    for ty in (TY["C>T"], TY["G>A"]):
        assert sc["ratio"][T_DEAM, ty] > 4.0 and sc["z"][T_DEAM, ty] > 15.0
    g = TY["G>T"]
    assert sc["za"][T_OXFW, g] > 25.0 and delta[T_OXFW, g] > 0.25 and sc["ratio"][T_OXFW, g] < DEFAULTS["excess_ratio"]
    assert DEFAULTS["excess_ratio"] == 3.0 and DEFAULTS["z_cutoff"] == 10.0 and DEFAULTS["asym_delta"] == 0.15
    # the variant-bearing file: its 40 variant positions are kept out by the gate, and only by it
    v = c["variants"]
    e = enters(c["recs"][T_VAR], c["ref_code"], c["cls"], CLASSES)
    assert not e[v].any() and enters(c["recs"][T_CLEAN], c["ref_code"], c["cls"], CLASSES)[v].sum() >= 38
    open_gate = score(fold(class_sums(c["recs"], c["ref_code"], c["cls"], CLASSES, 100, 1000)), N_NORMALS)
    assert (open_gate["flag"][T_VAR] == ELEVATED).sum() >= 3
    # the shallow file has sites, but too few; the empty file has none
    assert 0 < f["sites"][T_SHALLOW].max() < DEFAULTS["min_sites"] and not f["sites"][T_NONE].any() and np.isnan(sc["rate2"][T_NONE]).all()
