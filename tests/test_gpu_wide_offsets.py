"""Byte offsets of 2^31 and 2^32 and more: record reads through a row stride of 2 GiB, alignment streams 4 GiB long, and outputs of
4.4 GB.

Every record read of the library is `base + (row * row_stride + p) * rec_bytes` (or the same through ext / ext_stride), every output
`out + (row * P + p) * k`.  Read before these tests were run, every one of them widens to size_t before the product: rec_counts and
rec_load_at's callers (ampli_device.h; limits, loo, dispersion and overdispersion go through rec_counts), error_reduce_kernel and
compact_reduce_body (`q = rv.base + ((size_t)min(s0, S - 1) * (size_t)rv.row_stride + (size_t)p) * RB`, then `q += row_step`),
error_sums_inorder, poisson_call_kernel / poisson_full_kernel / poisson_stream_kernel, nb_score_kernel, paired_score_kernel, di_load,
genotype_planes_kernel, contamination_kernel, amplicon_depth_kernel, spectrum_kernel and exceedance_kernel.  Read later, in the same
way:
  monitor_sums_kernel, monitor_control_kernel, fraction_kernel: `stride = (size_t)rv.row_stride * rb`, `q = rv.base + (size_t)row *
    stride`, `rec_load_at(q + (size_t)ent.p * rb)`; the outputs `sums + ((size_t)row0 * (size_t)L + (size_t)l) * AMPLI_MON_SUMS` (and
    the same for lambda, est, count), stepped by `(size_t)L * k`; `thr[(size_t)y * (size_t)P + (size_t)p]`.  Primary records only.
  hetsite_reference_kernel, allelic_site_kernel: `q = rv.base + (size_t)p * rec_bytes`, `row_bytes = (size_t)rv.row_stride *
    rec_bytes`, `rec_load_at(q + (size_t)s * row_bytes)`; `ref + (size_t)c * (size_t)P + (size_t)p` with `plane = (size_t)PAIRS *
    (size_t)P`; `cell = (size_t)s * (size_t)P + (size_t)p`.  Primary records only, by contract.
  the four read walks (ampli_bam.h, ampli_pileup.hip, ampli_indel.hip, ampli_evidence.hip, ampli_amplicon_count.hip): `bam +
    rec_off[read] + 4` with rec_off unsigned long long and `read` long long; bam_window_base the same; the staged kernel's span
    `g0 = rec_off[first] & ~15ull`, `g1 = last + 4ull + block_size`, both unsigned long long, `src = bam + g0`, `stage +
    (rec_off[first + t] - g0)`; inside a record `cig + 4 * (size_t)c`, int query offsets below l_seq.  Counters: `ctr[a * 8 + b4]` with
    `a` int into the LDS window and long long into the global counts; the flushes `counts[(wb + (i >> 3)) * 8 + (i & 7)]`, `counts[(wb +
    (i >> 1)) * 8 + (i & 1) * 4]` with wb long long; `lengths[(a * 2 + (pend - 1)) * AMPLI_INDEL_LEN_BINS + bin]`, a long long; `hist +
    (k * 4 + b4) * (long long)(METRICS * BINS)` and `hist + (wb + w) * (long long)EVIDENCE_CELLS`, k and wb long long; the amplicon
    walk's `w = cell0 + refpos + j`, `counts[w * 8 + nt]`, all long long, `amp_reads[run_a * 2 + run_rev]`.
  amplicon_layers_kernel: `w = amp_off[a] + (long long)(key - lo[a])`, `counts + w * 8`, `layers + ((long long)l * P + p) * 8`,
    `layer_amp[(long long)l * P + p]`, `total + p * 8`, p long long.  evidence_score_kernel: `hist + p * EVIDENCE_CELLS`, `o_int[cell *
    3]`, `o_med[cell * 2]`, `o_z2[cell]`, cell and p long long.
No product of these was found formed in 32 bits.  Nothing holds them to that but these tests.

C. Record reads.  One allocation of 6 GiB, filled with the byte 0x01 (as a record: present, 257 / 65793 / 16843009 reads in every field,
which no row of the cohort holds).  The records' base lies 2 GiB into it; a chunk of 3 rows of 130 positions is written with a row
stride that puts row 1 a row's length past 2^31 bytes and row 2 two rows' lengths past 2^32 bytes from the base
(tests/scale_shapes.wide_stride, per layout).  An offset cut to 32 bits then lands behind row 0, one sign-extended from 32 bits below
the base: both inside the allocation, on the pattern -- a wrong value, not a fault (tests/test_scale_shapes.py works the cases out).
For the kernels that read extra occurrences a second placement does the same with ext / ext_stride (E = 9).  The two-cohort entry
points get the wide chunk on either side in turn; contamination_records takes ONE chunk of records (its sources are planes), so it
has one side.  Per entry point and layout: the outputs on the strided chunk equal, byte for byte, the outputs on a dense copy of the
same rows (which the feature's own tests hold to the model); the rows are unchanged and every other byte of the allocation is still
the pattern.  monitor_sums_records, monitor_control_records, hetsite_reference_records, allelic_site_records and fraction_records take
their lists, thresholds and planes from the features' own case modules (wide_inputs).

D. Outputs.  pair_score, dilute and nb_score at 4 * 65535 + 5 rows of 520 positions write 4.36 GB through their cheap paths -- pairs
that name a row outside the chunk, bad mixtures, absent records -- with real work in four rows: row 0, the first row that starts past
2^31 bytes, the first past 2^32 bytes, and the last.  Those rows equal the model; all other cells are NA / ABSENT, counted in one
reduction on the device; the fence around the output is whole.

E. Alignment streams.  The same allocation, d_bam 2 GiB into it.  808 reads of the pileup table (indels, clips, odd operations, both
strands, filtered and unplaced reads) lie in three places: at d_bam, 1 MiB past 2^31 bytes and 2 MiB past 2^32 bytes from it, rec_off
ascending across them (tests/scale_shapes.bam_layout).  An offset cut to 32 bits, or sign-extended from 32 bits, lands on the pattern
inside the allocation, and the pattern decodes as a FILTERED read (flag 0x0101: secondary): a missing read, not a fault
(tests/test_scale_shapes.py).  Two arrangements: "staged", every group of 256 reads wholly inside one place, so that
pileup_count_staged_kernel stages at wide offsets; "fallback", the cuts 100 reads later, so that two groups straddle a gap, exceed
PILEUP_STAGE and take the wave-per-read walk at wide offsets.  Per walk (pileup_count, pileup_indel_count, pileup_evidence,
pileup_amplicon_count) and arrangement: every output, stats included, equals the output on the dense stream byte for byte, which
equals the model; the records are unchanged and the rest of the allocation is still the pattern.

F. The walks' outputs.  Panels that are a plain arange on one reference (two long amplicons for the amplicon walk), large enough that
the output passes 2^32 bytes: d_hist at 3072 bytes a key (P = 1.4 M; ampli_evidence_score runs over it), d_lengths at 256 (P = 16.8 M),
ampli_pileup_count's d_counts at 32 (P = 134 M), ampli_pileup_amplicon_count's d_counts at 32 (W = 134 M walk entries) and
ampli_amplicon_layers' d_total and one layer at 32 (P = 134 M keys over a walk of four entries).  Four groups of 256 reads on four
cells -- cell 0, the first that starts at or past 2^31 bytes, the first at or past 2^32 bytes, the last --, each group with most of its
reads on its own cell (the LDS window's flush) and one on each of the others (the global counters).  The four cells equal the model on
those four keys; everything else is zero, counted in one reduction on the device; the fence is whole.  Unlike C and E these outputs
have nothing of their own below them: an output offset SIGN-EXTENDED from 32 bits would leave the allocation, which is why every
expression above was read first.

NOT covered, because the case alone needs tens of GB: poisson_call and loo masks beyond 4 GiB; fdr_adjust planes beyond 4 GiB;
P >= 2^28, the first size at which `plane * P + p` passes 2^31; ampli_amplicon_layers with L >= 2 at P = 134 M (8.6 GB of layers, 14 GB
with the totals and keys); ampli_pileup_indel_count's d_counts and ampli_pileup_amplicon_count's d_amp_reads beyond 4 GiB (P = 134 M
keys would put d_lengths at 34 GB; 2^28 amplicons); a single alignment stream of more than 2^32 bytes of RECORDS (E places 150 KB of
them across 4 GiB); monitor / fraction / allelic outputs beyond 4 GiB (n x L = 9 x 10^7 cells)."""
import collections
import functools

import numpy as np
import pytest

from tests import scale_shapes as sh
from tests.helpers import fenced
from tests.scale_device import as_ints, need, release, tile_rows
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min
P, N, E9 = sh.WIDE_P, sh.WIDE_N, sh.WIDE_E
LAYOUTS = ("i32", "u24", "u16")
PATTERN = 0x01
LEVELS = (0.005, 0.02)
COMPACT = {"u16": "error_reduce_u16_kernel", "u24": "error_reduce_u24_kernel"}


# ==== D, F. outputs beyond 2^32 bytes (first in the file: they run before the 6 GiB of C and E are allocated) ==================================

def _na_count(t, na):
    """cells of a float32 tensor that hold exactly `na`, in one reduction"""
    import torch

    return int((t.view(torch.int32) == int(np.float32(na).view(np.int32))).sum())


def test_pair_score_writes_beyond_four_gib(ctx):
    import torch

    from tests.dispersion_cohorts import cohort
    from tests.paired_model import NA, score_model
    from tests.test_gpu_paired import CUTOFF, ROWS_A, ROWS_B, _records, _same

    n, Pb, special = sh.BIG_ROWS, sh.BIG_P, sh.big_special_rows()
    need(ctx, n * sh.BIG_ROW_BYTES + (64 << 20))
    A = cohort(Pb, ROWS_A, 9001, extras=False, u16=True)
    B = cohort(Pb, ROWS_B, 9002, extras=False, u16=True)
    ref = np.random.default_rng(9).integers(0, 4, Pb).astype(np.uint8)
    real = [(1, 4), (0, 0), (5, 2), (3, 3)]
    want, want64 = score_model(A[0], B[0], Pb, real, ref, CUTOFF)
    assert (want != NA).sum() > Pb
    pairs = np.empty((n, 2), np.int32)
    pairs[:] = (ROWS_A, 0)  # a row outside chunk A: NA is stored and no record is loaded
    pairs[1::2] = (0, -1)
    for row, pr in zip(special, real):
        pairs[row] = pr
    s, check = fenced((n, Pb, 4, 2), torch.float32)
    ctx.pair_score(_records(ctx, A, Pb, "u16"), _records(ctx, B, Pb, "u16"), Pb, _t(pairs), _t(ref), CUTOFF, s=s)
    ctx.sync()
    _same(s[list(special)].cpu().numpy(), want, want64)
    assert _na_count(s, NA) == n * Pb * 8 - int((want != NA).sum())
    check()
    del s, check
    release()


def test_dilute_writes_beyond_four_gib(ctx):
    import torch

    from amplisolve_amd.api import DILUTE_BAD_MIXTURE, DILUTE_KEEP_ALL
    from tests.dispersion_cohorts import cohort
    from tests.test_gpu_paired import ROWS_A, _records

    n, Pb, special = sh.BIG_ROWS, sh.BIG_P, sh.big_special_rows()
    need(ctx, n * sh.BIG_ROW_BYTES + (64 << 20))
    A = cohort(Pb, ROWS_A, 9003, extras=False, u16=True)
    rows = (2, 0, 5, 3)
    want = A[0][list(rows), :Pb].copy()  # a keep-all mixture draws nothing: a's primary records as they are
    want[want[:, :, 0] == ABSENT, 1:] = 0
    present = int((want[:, :, 0] != ABSENT).sum())
    assert present > 3 * Pb
    words = np.empty((n, 4), np.uint64)
    words[:] = ((ROWS_A & 0xFFFFFFFF) | (0xFFFFFFFF << 32), 5, 5, 77)  # row_a outside the chunk, no diluent: a bad mixture
    for row, ra in zip(special, rows):
        words[row] = ((ra & 0xFFFFFFFF) | (0xFFFFFFFF << 32), DILUTE_KEEP_ALL, 0, 1000 + ra)
    out, check = fenced((n, Pb, 8), torch.int32)
    flags, fcheck = fenced((n,), torch.int32)
    ctx.dilute(_records(ctx, A, Pb, "u16"), None, Pb, _t(words.view(np.int64)), out=out, flags=flags)
    ctx.sync()
    assert torch.equal(out[list(special)], _t(want))
    assert int((out[:, :, 0] == ABSENT).sum()) == n * Pb - present                          # every other record is ABSENT ...
    assert int((out[:, :, 1:] != 0).sum()) == int((want[:, :, 1:] != 0).sum())              # ... and zero in its other fields
    assert int((flags == DILUTE_BAD_MIXTURE).sum()) == n - 4 and not bool(flags[list(special)].any())
    check()
    fcheck()
    del out, flags, check, fcheck
    release()


def test_nb_score_writes_beyond_four_gib(ctx):
    import torch

    from tests.test_gpu_overdispersion import CUTOFF, NA, Q_TOL, _q_case

    n, Pb, special = sh.BIG_ROWS, sh.BIG_P, sh.big_special_rows()
    need(ctx, n * sh.BIG_ROW_BYTES + n * Pb * 16 + (64 << 20))
    recs, ref, thr, omega, _, want, _ = _q_case(Pb, 4)
    assert (want != NA).sum() > Pb
    absent = np.zeros((1, Pb, 8), np.int32)
    absent[:, :, 0] = ABSENT
    d_recs = tile_rows(_pack(ctx, absent, "u16"), n)
    d_recs[list(special)] = _pack(ctx, recs, "u16")
    q, check = fenced((n, Pb, 4, 2), torch.float32)
    ctx.nb_score(ctx.records(d_recs, "u16", n), Pb, _t(thr), _t(ref), _t(omega), CUTOFF, q=q)
    ctx.sync()
    got = q[list(special)].cpu().numpy()
    exact = (want == NA) | (want == np.float32(-888)) | (want == 0)
    assert np.array_equal(got[exact], want[exact]) and np.array_equal(got == NA, want == NA)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= Q_TOL).all()
    assert _na_count(q, NA) == n * Pb * 8 - int((want != NA).sum())
    check()
    del q, check, d_recs
    release()


# ---- F. the read walks: cells of 32, 256 and 3072 bytes per key (or walk entry), real work on four of them ------------------------------

ONE_COLUMN = ("1M", "3S1M", "1M4S", "2S1=2S", "5H1X", "1M2H")  # a read of these touches one key: the four cells are the whole answer
ONE_JUNCTION = ("2M", "1M2I1M", "1M3D1M", "1=40I1M", "3S1M1D1M", "1M1I1X2S")  # ... observes only the junction behind its first column


def special_stream(where, cigars, seed):
    """Four groups of 256 reads in the order of `where` = [(ref_id, 1-based position)] * 4: 253 reads of a group start on its own
    position -- so the workgroup's LDS window starts at that key and is flushed to that cell -- and one on each of the other three, which
    lie outside the window and go to the global counters directly.  Both strands, MAPQ below, at and above 20, a filtered read, an
    unplaced one, qualities 20 .. 60 around mbq = 30.  Returns (buf, rec_off)."""
    from tests import pileup_model as pm

    rng = np.random.default_rng(seed)
    assert pm.geometry().reads == 256 and len(where) == 4
    reads = []
    for g, (ref_id, pos1) in enumerate(where):
        group = [pm.read(ref_id, pos1 - 1, cigars[int(rng.integers(len(cigars)))], rng, flag=0x10 * int(rng.integers(2)), mapq=int(rng.choice([60, 60, 20, 19])))
                 for _ in range(253)]
        group[7]["flag"] |= 0x400
        group[8]["pos"] = -1
        for k, o in enumerate(x for x in range(4) if x != g):
            group.insert(40 + 70 * k, pm.read(where[o][0], where[o][1] - 1, cigars[k], rng, flag=0x10 * (k & 1)))
        reads += group
    return pm.build_stream(reads, lead=3)


@pytest.fixture(scope="module")
def big_keys(ctx):
    """(reference 0 << 32 | 1 .. n) for the largest panel, built with numpy and uploaded once; the smaller panels are its prefixes"""
    n = sh.special_cells(32)[0]
    need(ctx, n * 8)
    holder = [_t(np.arange(1, n + 1, dtype=np.int64))]
    yield holder[0]
    holder.clear()
    release()


def _only(t, special, want, what):
    """t[special] equals want, and t holds no more non-zero elements than want does (one reduction): every other cell is zero"""
    got = t[list(special)].cpu().numpy().astype(np.int64)
    assert np.array_equal(got.reshape(want.shape), want), f"{what}: the four cells differ from the model"
    assert want.any() and all(want[i].any() for i in range(4)), f"{what}: a special cell is empty in the model"
    assert int((t != 0).sum()) == int((want != 0).sum()), f"{what}: a cell outside the four is not zero"


def test_evidence_histograms_and_their_scores_beyond_four_gib(ctx, big_keys):
    import torch

    from tests import evidence_model as em

    P, special = sh.special_cells(sh.CELL_BYTES["evidence_hist"])
    need(ctx, P * 3072 + P * 128 + (64 << 20))
    src = special_stream([(0, i + 1) for i in special], ONE_COLUMN, 501)
    want = em.count(src, np.asarray([i + 1 for i in special], np.uint64), 30, 20)
    hist, check = fenced((P, 4, em.METRICS, em.BINS), torch.int32)
    hist.zero_()
    stats = torch.zeros((2,), dtype=torch.int64, device=ctx.device)
    ctx.read_evidence(_t(src[0]), _t(src[1].view(np.int64)), big_keys[:P], mbq=30, mrq=20, hist=hist, stats=stats)
    ctx.sync()
    _only(hist, special, want.hist, "d_hist")
    assert tuple(stats.tolist()) == tuple(want.stats) and want.stats[1] > 500
    check()
    # ampli_evidence_score over the same planes: ref A, the alt chosen.  Every row but the four is the score of an empty plane
    ref, alt = np.zeros(P, np.int8), np.full(P, -1, np.int8)
    outs = [fenced(shape, dt) for shape, dt in (((P, 3, 3), torch.int64), ((P, 3, 2), torch.int32), ((P, 3), torch.float64), ((P,), torch.int8))]
    ints, med, z2, used = ctx.evidence_score(hist, _t(ref), _t(alt), *(o[0] for o in outs))
    ctx.sync()
    sp = list(special)
    w4 = em.score(want.hist, ref[:4], alt[:4])
    assert (w4.ints[:, :, 2] >= 0).any()
    found = em.score_differences(em.Score(ints[sp].cpu().numpy(), med[sp].cpu().numpy(), z2[sp].cpu().numpy(), used[sp].cpu().numpy()), w4)
    assert not found, found
    w0 = em.score(np.zeros_like(want.hist[:1]), ref[:1], alt[:1])
    off_rows = ((ints.reshape(P, 9) != _t(np.asarray(w0.ints, np.int64).reshape(1, 9))).any(1) | (med.reshape(P, 6) != _t(np.asarray(w0.med, np.int32).reshape(1, 6))).any(1) |
                (as_ints(z2) != _t(np.asarray(w0.z2, np.float64).view(np.int64).reshape(1, 3))).any(1) | (used != int(np.asarray(w0.alt_used).reshape(-1)[0])))
    assert set(off_rows.nonzero().reshape(-1).tolist()) <= set(special), "a position without reads is not scored as an empty plane"
    for _, c in outs:
        c()
    del hist, check, outs, ints, med, z2, used, off_rows
    release()


def test_indel_length_bins_beyond_four_gib(ctx, big_keys):
    import torch

    from tests import indel_model as im

    P, special = sh.special_cells(sh.CELL_BYTES["indel_lengths"])
    need(ctx, P * (256 + 32) + (64 << 20))
    src = special_stream([(0, i + 1) for i in special], ONE_JUNCTION, 502)
    want = im.count(src, np.asarray([i + 1 for i in special], np.uint64), 30, 20)
    lengths, check = fenced((P, 2, im.BINS), torch.int32)
    lengths.zero_()
    counts, ccheck = fenced((P, 8), torch.int32)
    counts.zero_()
    stats = torch.zeros((2,), dtype=torch.int64, device=ctx.device)
    ctx.indel_count(_t(src[0]), _t(src[1].view(np.int64)), big_keys[:P], mbq=30, mrq=20, counts=counts, lengths=lengths, stats=stats)
    ctx.sync()
    _only(lengths, special, want.lengths, "d_lengths")
    _only(counts, special, want.counts, "d_counts")
    assert tuple(stats.tolist()) == tuple(want.stats) and want.counts[:, 1].min() > 0 and want.counts[:, 2].min() > 0
    check()
    ccheck()
    del lengths, counts, check, ccheck
    release()


def test_pileup_counts_beyond_four_gib(ctx, big_keys):
    import torch

    from tests import pileup_model as pm

    P, special = sh.special_cells(sh.CELL_BYTES["pileup_counts"])
    assert P == big_keys.numel()
    need(ctx, P * 32 + (64 << 20))
    buf, off = special_stream([(0, i + 1) for i in special], ONE_COLUMN, 503)
    w_counts, w_kept, w_added = pm.count((buf, off), np.asarray([i + 1 for i in special], np.uint64), 30, 20)
    counts, check = fenced((P, 8), torch.int32)
    counts.zero_()
    stats = torch.zeros((2,), dtype=torch.int64, device=ctx.device)
    bam, d_off = _t(buf), _t(off.view(np.int64))
    ctx._check(ctx.lib.ampli_pileup_count(ctx.h, bam.data_ptr(), d_off.data_ptr(), d_off.numel(), big_keys.data_ptr(), P, 30, 20, counts.data_ptr(), stats.data_ptr()))
    ctx.sync()
    _only(counts, special, w_counts, "d_counts")
    assert stats.tolist() == [w_kept, w_added] and w_added > 500
    check()
    del counts, check
    release()


def _two_long_amplicons(W, special):
    """[(0, 1, len0), (1, 1, W - len0)]: the walk entries of the first end 100 entries before the first special entry past 2^31 bytes, so
    that three of the four special entries lie in the second; and the (reference, position) of the four entries"""
    len0 = special[1] - 100
    iv = [(0, 1, len0), (1, 1, W - len0)]
    where = [(0, w + 1) if w < len0 else (1, w - len0 + 1) for w in special]
    assert all(1 <= l < 2 ** 31 for _, _, l in iv) and W < 2 ** 31
    return iv, where


def test_amplicon_walk_counts_beyond_four_gib(ctx):
    import torch

    from tests import amplicon_count_model as acm

    W, special = sh.special_cells(sh.CELL_BYTES["amplicon_counts"])
    need(ctx, W * 32 + (64 << 20))
    iv, where = _two_long_amplicons(W, special)
    big = acm.make_amplicons(iv)
    assert int(big.amp_off[-1]) == W and [int(big.amp_off[r]) + x - 1 for r, x in where] == list(special)
    src = special_stream(where, ONE_COLUMN, 504)
    # the model: four amplicons of one position, in the order of the four entries -- a one-column read lies wholly inside either design
    want = acm.count(src, acm.make_amplicons([(r, x, x) for r, x in where]), 30, 20)
    assert want.stats[3] == 0 and want.stats[2] > 500
    counts, check = fenced((W, 8), torch.int32)
    counts.zero_()
    got = ctx.amplicon_count(_t(src[0]), _t(src[1].view(np.int64)), acm._up(big.lo), acm._up(big.hi), acm._up(big.reach), acm._up(big.amp_off), mbq=30, mrq=20,
                             counts=counts)
    ctx.sync()
    _only(counts, special, want.counts, "d_counts")
    assert got[1].tolist() == [want.amp_reads[0].tolist(), want.amp_reads[1:].sum(0).tolist()] and tuple(got[2].tolist()) == tuple(want.stats)
    check()
    del counts, check, got
    release()


def test_amplicon_layers_beyond_four_gib(ctx, big_keys):
    """keys may repeat and lie anywhere, so the walk stays small: four amplicons of one position under the four special keys.  L = 1: the
    one layer and the totals both pass 2^32 bytes (L = 2 would need 14 GB)"""
    import torch

    from tests import amplicon_count_model as acm

    P, special = sh.special_cells(sh.CELL_BYTES["layers_total"])
    assert P == big_keys.numel()
    need(ctx, P * (32 + 32 + 4) + (64 << 20))
    amps = acm.make_amplicons([(0, i + 1, i + 1) for i in special])
    walked = np.random.default_rng(505).integers(1, 1000, (4, 8)).astype(np.int32)
    want = acm.layers(walked.astype(np.int64), amps, np.asarray([i + 1 for i in special], np.uint64), 1)
    (layers, c0), (layer_amp, c1), (total, c2) = (fenced(shape, torch.int32) for shape in ((1, P, 8), (1, P), (P, 8)))
    ctx.amplicon_layers(_t(walked), acm._up(amps.lo), acm._up(amps.hi), acm._up(amps.reach), acm._up(amps.amp_off), big_keys, L=1, layers=layers,
                        layer_amp=layer_amp, total=total)
    ctx.sync()
    sp = list(special)
    _only(total, special, want.total, "d_total")
    assert np.array_equal(layers[0, sp].cpu().numpy(), want.layers[0]) and layer_amp[0, sp].tolist() == want.layer_amp[0].tolist() == [0, 1, 2, 3]
    assert int((layers[0, :, 0] == ABSENT).sum()) == P - 4 and int((layers[0, :, 1:] != 0).sum()) == int((want.layers[0, :, 1:] != 0).sum())
    assert int((layer_amp == -1).sum()) == P - 4
    for c in (c0, c1, c2):
        c()
    del layers, layer_amp, total, c0, c1, c2
    release()


# ==== C. record reads at 2^31 and 2^32 bytes ==============================================================================================

class Arena:
    """the patterned allocation; place() writes a chunk's rows at the wide stride and hands back what ampli_records points at"""

    def __init__(self, buf):
        self.buf, self.placed = buf, []

    def place(self, rows, layout):
        """rows: a packed device tensor [n, R, ...] of `layout`; returns (tensor whose data_ptr is the records' base, stride in records)"""
        rb, stride = sh.REC_BYTES[layout], sh.wide_stride(layout)
        for r in range(rows.shape[0]):
            src = rows[r].contiguous().view(-1).view(self.buf.dtype)
            assert src.numel() == rows.shape[1] * rb
            self.put(sh.WIDE_BASE + r * stride * rb, src)
        return self.buf[sh.WIDE_BASE:], stride

    def put(self, off, src):
        """src (uint8, on the device) at byte `off` of the allocation, remembered for check_and_clear"""
        assert 0 <= off and off + src.numel() <= self.buf.numel()
        self.buf[off:off + src.numel()].copy_(src)
        self.placed.append((off, src.clone()))

    def place_stream(self, arrangement):
        """the records of sh.bam_stream() in their three places; returns (tensor whose data_ptr is d_bam, rec_off of the placed stream)"""
        dense = _t(sh.bam_stream()[0])
        pieces, wide = sh.bam_layout(arrangement)
        for at, lo, hi in pieces:
            self.put(sh.BAM_BASE + at, dense[lo:hi])
        return self.buf[sh.BAM_BASE:], _t(wide.view(np.int64))

    def check_and_clear(self):
        """the rows are what was placed, and with the rows taken out again every byte of the allocation is the pattern"""
        import torch

        for off, src in self.placed:
            assert torch.equal(self.buf[off:off + src.numel()], src), "a kernel wrote to its input records"
            self.buf[off:off + src.numel()] = PATTERN
        self.placed = []
        words = self.buf.view(torch.int64)
        bad = int((words != int.from_bytes(bytes([PATTERN]) * 8, "little")).sum())
        if bad:
            self.buf.fill_(PATTERN)
        assert bad == 0, f"{bad} eight-byte word(s) of the allocation no longer hold the pattern"


_BUNDLES = {}


@pytest.fixture(scope="module")
def arena(ctx):
    import torch

    nbytes = (max([sh.wide_bytes(lay) for lay in LAYOUTS] + [sh.bam_bytes()]) + 4095) // 4096 * 4096
    need(ctx, nbytes)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)
    buf.fill_(PATTERN)
    a = Arena(buf)
    yield a
    _BUNDLES.clear()
    _WALK_DENSE.clear()
    a.buf = None
    del buf
    release()


@functools.lru_cache(maxsize=None)
def _cohort(E):
    """3 rows of 130 positions (tests/test_gpu_loo's normals: edge-case records, absent records, spiked variants), with E extra
    occurrences -- all of them of positions 64 .. 129, so that the compact reduce kernel keeps the first tile --, an RD plane, a table
    of thresholds and amplicon and class lists"""
    from tests.test_gpu_loo import _cohort as loo_cohort

    rng = np.random.default_rng(1000 + E)
    recs, _, _, _, _, ref = loo_cohort(P, N, 31 + E, u16=True)
    dup_off = ext_pos = None
    if E:
        mult = np.zeros(P, np.int64)
        pick = rng.choice(np.arange(64, P), E - 1, replace=False)
        mult[pick] = 1
        mult[pick[0]] = 2
        dup_off = np.concatenate([[0], np.cumsum(mult)]).astype(np.uint32)
        ext_pos = np.repeat(np.arange(P), mult).astype(np.uint32)
        assert len(ext_pos) == E
        ext = recs[:, ext_pos].copy()
        ext = np.where(ext[:, :, :1] == ABSENT, ext, np.minimum(ext + rng.integers(0, 3, ext.shape).astype(np.int32), 65534))
        ext[0, 2] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
        recs = np.concatenate([recs, ext], axis=1)
    rd = np.full((N, P + E), ABSENT, np.int32)
    own = (rng.random((N, P + E)) < 0.1) & (recs[:, :, 0] != ABSENT)
    rd[own] = (recs.sum(-1)[own] + rng.integers(1, 50, own.sum())).astype(np.int32)
    thr = np.array([float(f"{x:f}") for x in np.exp(rng.uniform(np.log(2e-4), np.log(0.02), 8 * P))], np.float32).reshape(2, 4, P)
    thr[:, :, ::17] = np.float32(0.01)
    cls = (np.arange(P) % 5).astype(np.uint8)
    cls[::11] = 255
    assert (recs[:, :, 0] == ABSENT).any() and not (recs[:, :, :] == 257).all(axis=-1).any()
    return dict(recs=recs, ref=ref, dup_off=dup_off, ext_pos=ext_pos, rd=rd, thr=thr, cls=cls, amp_off=np.array([0, 40, 40, 131]),
                amp_pos=np.concatenate([np.arange(40), np.arange(39, 130)]))


class Bundle:
    """the device side of one (layout, E) case: the dense chunk, its Records, and what the entry points need beside records"""

    def __init__(self, ctx, layout, E):
        c = _cohort(E)
        self.layout, self.E, self.c = layout, E, c
        self.packed = _pack(ctx, c["recs"], layout)                      # [N, P + E, ...], the dense interchange layout
        self.prim = self.packed[:, :P].contiguous()
        self.ext = self.packed[:, P:].contiguous() if E else None
        self.thr, self.ref, self.cls = _t(c["thr"]), _t(c["ref"]), _t(c["cls"])
        self.ref4 = _t(np.where(c["ref"] > 3, 0, c["ref"]).astype(np.uint8))
        self.index = dict(dup_off=_t(c["dup_off"]), ext_pos=_t(c["ext_pos"])) if E else {}
        self.rd = dict(rd=_t(c["rd"][:, :P]), rd_ext=_t(c["rd"][:, P:]) if E else None)
        self.dense = ctx.records(self.packed, layout, N, E=E, **self.index)
        self.cache = {}

    def records(self, ctx, arena, placement, with_rd=False):
        """the same chunk with its primaries ("rows") or its extras ("ext") at the wide stride; None: the dense chunk"""
        kw = dict(self.index, **(self.rd if with_rd else {}))
        if placement is None:
            return ctx.records(self.packed, self.layout, N, E=self.E, **kw)
        if placement == "rows":
            base, stride = arena.place(self.prim, self.layout)
            if self.E:
                return ctx.records(base, self.layout, N, E=self.E, row_stride=stride, ext=self.ext, ext_stride=self.E, **kw)
            return ctx.records(base, self.layout, N, row_stride=stride, **kw)
        base, stride = arena.place(self.ext, self.layout)
        return ctx.records(self.prim, self.layout, N, E=self.E, row_stride=P, ext=base, ext_stride=stride, **kw)

    def once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


def _bundle(ctx, layout, E):
    if (layout, E) not in _BUNDLES:
        _BUNDLES[layout, E] = Bundle(ctx, layout, E)
    return _BUNDLES[layout, E]


# ---- the entry points: run(ctx, b, rec[, rec_b]) -> the output tensors --------------------------------------------------------------

def _table(fin):
    import torch

    return [fin.rate, fin.code, fin.thr, fin.germ_present, torch.where(fin.germ_present > 0, fin.germ_val, torch.zeros_like(fin.germ_val))]


def run_reduce_general(ctx, b, rec):
    ctx.set_reduce_compact(False)
    try:
        acc = ctx.new_acc(P)
        acc.buf.zero_()
        fin = ctx.error_reduce_records(rec, P, acc, 0.002, 100, finalize=True)
        assert ctx.last_reduce_kernel() == "error_reduce_kernel"
    finally:
        ctx.set_reduce_compact(True)
    return [acc.snt, acc.srd, acc.cnt, acc.nrec, acc.gm_n] + _table(fin)


def run_reduce_compact(ctx, b, rec):
    ctx.set_tuning(1, groups=1)  # one sample split, one lane group: the shape the compact kernels take
    try:
        acc = ctx.new_acc(P)
        acc.buf.zero_()
        fin = ctx.error_reduce_records(rec, P, acc, 0.002, 100, finalize=True, summary=True)
        assert ctx.last_reduce_kernel() == COMPACT[b.layout]
        assert ctx.flags() == 0
    finally:
        ctx.set_tuning(0)
    return [acc.snt, acc.srd, acc.cnt, acc.nrec] + _table(fin)


def run_inorder(ctx, b, rec):
    acc = ctx.new_acc(P)
    acc.buf.zero_()
    ctx.error_sums_inorder(rec, P, acc, 0.002, 100)
    return [acc.snt]


def run_poisson_prefilter(ctx, b, rec):
    from amplisolve_amd.api import POISSON_PREFILTER

    res = ctx.poisson_call_records(rec, P, b.thr, b.ref, 100, mode=POISSON_PREFILTER)
    assert ctx.flags() & 4 == 0  # AMPLI_FLAG_QUEUE_OVERFLOW
    return [res["call_mask"]]


def run_poisson_full(ctx, b, rec):
    import torch

    from amplisolve_amd.api import POISSON_FULL

    q = torch.zeros((N, P + b.E, 4, 2), dtype=torch.float64, device=ctx.device)
    res = ctx.poisson_call_records(rec, P, b.thr, b.ref, 100, mode=POISSON_FULL, q=q)
    return [res["call_mask"], q]


def _acc(ctx, b, C_value):
    def make():
        acc = ctx.new_acc(P)
        ctx.error_reduce_records(b.dense, P, acc, C_value, 100, summary=True)
        return acc

    return b.once(("acc", C_value), make)


def run_loo(ctx, b, rec):
    from amplisolve_amd.api import POISSON_PREFILTER

    res = ctx.loo_call(rec, P, _acc(ctx, b, 0.002), b.ref, 0.002, 100, 100, mode=POISSON_PREFILTER, capacity=4 * N * (P + b.E) + 64, dense_thr=True)
    assert ctx.flags() & 4 == 0
    return [res["call_mask"], res["callable_pos"], res["callable_sample"], res["thr_loo"], res["flags"], res["n_calls"]]


def run_limit(ctx, b, rec):
    res = ctx.detection_limits(rec, P, b.thr, b.ref, 100, LEVELS)
    return [res["min_reads"], res["status"], res["counts"]]


def run_power(ctx, b, rec):
    lim = b.once("limit", lambda: ctx.detection_limits(b.dense, P, b.thr, b.ref, 100, ()))
    res = ctx.detection_power(rec, P, lim["min_reads"], lim["status"], LEVELS, 0.95)
    return [res["power"], res["lod"], res["counts"]]


def run_dispersion(ctx, b, rec):
    import torch

    x2, rinv = (torch.zeros((2, 4, P), dtype=torch.float64, device=ctx.device) for _ in range(2))
    sx, se = (torch.zeros((N,), dtype=torch.float64, device=ctx.device) for _ in range(2))
    st = torch.zeros((N,), dtype=torch.int64, device=ctx.device)
    ctx.dispersion_records(rec, P, _acc(ctx, b, 0.0), 100, x2, rinv, False, sx, se, st)
    return [x2, rinv, sx, se, st]


def run_overdispersion(ctx, b, rec):
    return [ctx.overdispersion_sums(rec, P, _acc(ctx, b, 0.0), 100)]


def run_nb_score(ctx, b, rec):
    return [ctx.nb_score(rec, P, b.thr, b.ref4, None, 100)]


def run_genotype(ctx, b, rec):
    return [ctx.genotype_planes(rec, P)]


def run_contamination(ctx, b, rec):
    pl = b.once("planes", lambda: ctx.genotype_planes(b.dense, P))
    return [ctx.contamination(rec, P, pl, pl)]


def run_amplicon(ctx, b, rec):
    return [ctx.amplicon_depth(rec, P, b.c["amp_off"], b.c["amp_pos"], 100)]


def run_spectrum(ctx, b, rec):
    return [ctx.spectrum(rec, P, b.ref, b.cls, 5, 100, 1000)]


def run_pair_score(ctx, b, rec_a, rec_b):
    pairs = _t(np.array([(i, j) for i in range(N) for j in range(N)], np.int32))
    return [ctx.pair_score(rec_a, rec_b, P, pairs, b.ref4, 30)]


def run_exceedance(ctx, b, rec_t, rec_n):
    return list(ctx.exceedance(rec_t, rec_n, P, b.ref4, 100, 100))


def run_dilute(ctx, b, rec_a, rec_b):
    from tests.dilution_model import KEEP_ALL, keep_of

    mix = [(0, 1, keep_of(0.3), keep_of(0.7), 11), (1, 2, keep_of(0.5), KEEP_ALL, 12), (2, 0, KEEP_ALL, keep_of(0.1), 13), (2, 2, keep_of(0.9), keep_of(0.9), 14),
           (1, -1, keep_of(0.25), 0, 15)]
    return list(ctx.dilute(rec_a, rec_b, P, mix))


def wide_inputs():
    """What the five later entry points take beside records, from the features' own case modules, cut to the bundle's 3 rows of 130
    positions -- host arrays, computed once; tests/test_scale_shapes.py runs the models over the bundle's records with them and holds
    every output away from all-zero without a GPU.
      monitor: monitor_cases.panel(P) and .lists(P); control_case(P, N, R = 3) for pairs and candidates.
      fraction: fraction_cases.panel() cut to P positions; its lists as they are (an entry at or beyond P is none by the definition).
      allelic: the genotype planes of allelic_cohorts.small(P, N, .) for the chunk's "own" rows, and a germline pool of 12 rows of
      small(P, 12, .) with the model's het-site reference of that pool; min_depth 100, min_normals 3 (tests/test_gpu_allelic.py)."""
    from tests import allelic_cohorts as ac
    from tests import allelic_model as alm
    from tests import fraction_cases as fc
    from tests import monitor_cases as mc
    from tests.concordance_model import classify, pack_planes

    if not _WIDE_INPUTS:
        m_thr, m_ref = mc.panel(P)
        m_off, m_cell = mc.lists(P)
        pairs, cand_off, cand_pos = mc.control_case(P, N, R=3)[:3]
        f_thr, f_ref = fc.panel()
        f_off, f_cell, f_w = fc.lists()
        own = ac.small(P, N, 2500 + P, layout_max=65534)
        pool = ac.small(P, 12, 2600 + P, layout_max=65534)
        bits_own, bits_pool = classify(own), classify(pool)
        _WIDE_INPUTS.update(
            m_thr=m_thr, m_ref=m_ref, m_off=m_off, m_cell=m_cell, pairs=pairs, cand_off=cand_off, cand_pos=cand_pos, cov=mc.COV, seed=mc.CONTROL_SEED,
            f_thr=np.ascontiguousarray(f_thr[:, :, :P]), f_ref=np.ascontiguousarray(f_ref[:P]), f_off=f_off, f_cell=f_cell, f_w=f_w, f_cov=fc.COV,
            bits_own=bits_own, planes_own=pack_planes(bits_own, P), bits_pool=bits_pool, planes_pool=pack_planes(bits_pool, P),
            het_ref=alm.reference(pool, bits_pool, P, 100), row_g=np.array([4, 0, 11], np.int32), min_depth=100, min_normals=3)
    return _WIDE_INPUTS


_WIDE_INPUTS = {}


def _wide(ctx, b):
    """wide_inputs() on the device, once per bundle"""
    def make():
        h = wide_inputs()
        d = {k: _t(h[k]) for k in ("m_thr", "m_ref", "pairs", "f_thr", "f_ref", "het_ref", "row_g")}
        d.update({k: _t(np.ascontiguousarray(h[k]).view(np.int64)) for k in ("planes_own", "planes_pool")})
        d.update(cand_off=_t(h["cand_off"].astype(np.int32)), cand_pos=_t(h["cand_pos"].astype(np.int32)))
        return d

    return b.once("wide", make)


def run_monitor_sums(ctx, b, rec):
    w, h = _wide(ctx, b), wide_inputs()
    sums, lam = ctx.monitor_sums(rec, P, w["m_thr"], w["m_ref"], h["m_off"], h["m_cell"], cov=h["cov"])
    assert bool(sums[:, :, 0].any()) and bool(sums[:, :, 2:4].any())  # entries evaluated (N_EVAL) and alternative reads among them (K_FW, K_BW)
    return [sums, lam]


def run_monitor_controls(ctx, b, rec):
    w, h = _wide(ctx, b), wide_inputs()
    sums, lam = ctx.monitor_controls(rec, P, w["m_thr"], w["m_ref"], h["m_off"], h["m_cell"], w["pairs"], w["cand_off"], w["cand_pos"], 3, first_rep=2,
                                     seed=h["seed"], cov=h["cov"])
    assert bool(sums[:, :, 0].any())
    return [sums, lam]


def run_fraction(ctx, b, rec):
    w, h = _wide(ctx, b), wide_inputs()
    est, count = ctx.tumour_fraction(rec, P, w["f_thr"], w["f_ref"], h["f_off"], h["f_cell"], h["f_w"], cov=h["f_cov"])
    assert bool(count[:, :, 0].any())  # TF_N_EVAL
    return [est, count]


def run_hetsite_reference(ctx, b, rec):
    w, h = _wide(ctx, b), wide_inputs()
    return [ctx.hetsite_reference(rec, P, w["planes_own"], h["min_depth"])]  # a new reference: zero but for what this chunk adds


def run_allelic_sites(ctx, b, rec):
    w, h = _wide(ctx, b), wide_inputs()
    q, km, v, code = ctx.allelic_sites(rec, P, w["planes_pool"], w["row_g"], w["het_ref"], h["min_depth"], h["min_normals"], True)
    assert bool(km.any())  # k_lo and m are stored for tested cells only: `code` alone is non-zero without any record read
    return [q, km, v, code]


Entry = collections.namedtuple("Entry", "run layouts extras with_rd sides")
ENTRIES = {
    "error_reduce_records/general": Entry(run_reduce_general, LAYOUTS, True, False, 1),
    "error_reduce_records/compact": Entry(run_reduce_compact, ("u16", "u24"), True, False, 1),
    "error_sums_inorder": Entry(run_inorder, LAYOUTS, True, False, 1),
    "poisson_call_records/prefilter": Entry(run_poisson_prefilter, LAYOUTS, True, False, 1),
    "poisson_call_records/all_scores": Entry(run_poisson_full, LAYOUTS, True, False, 1),
    "poisson_call_records/irr": Entry(run_poisson_prefilter, ("i32", "u24"), True, True, 1),  # an RD plane goes with these two layouts
    "loo_call_records": Entry(run_loo, LAYOUTS, True, False, 1),
    "limit_records": Entry(run_limit, LAYOUTS, True, False, 1),
    "power_records": Entry(run_power, LAYOUTS, True, False, 1),
    "dispersion_records": Entry(run_dispersion, LAYOUTS, True, False, 1),
    "overdispersion_records": Entry(run_overdispersion, LAYOUTS, True, False, 1),
    "nb_score": Entry(run_nb_score, LAYOUTS, False, False, 1),
    "pair_score": Entry(run_pair_score, LAYOUTS, False, False, 2),
    "genotype_planes": Entry(run_genotype, LAYOUTS, False, False, 1),
    "contamination_records": Entry(run_contamination, LAYOUTS, False, False, 1),
    "amplicon_depth_records": Entry(run_amplicon, LAYOUTS, False, False, 1),
    "spectrum_records": Entry(run_spectrum, LAYOUTS, False, False, 1),
    "exceedance": Entry(run_exceedance, LAYOUTS, False, False, 2),
    "dilute": Entry(run_dilute, LAYOUTS, False, False, 2),
    # the monitoring and fraction gathers read the primary records at the listed positions only; the allelic kernels ignore extras and
    # an RD plane by contract ("only the primary records enter"): no `ext` placement for any of the five
    "monitor_sums_records": Entry(run_monitor_sums, LAYOUTS, False, False, 1),
    "monitor_control_records": Entry(run_monitor_controls, LAYOUTS, False, False, 1),
    "hetsite_reference_records": Entry(run_hetsite_reference, LAYOUTS, False, False, 1),
    "allelic_site_records": Entry(run_allelic_sites, LAYOUTS, False, False, 1),
    "fraction_records": Entry(run_fraction, LAYOUTS, False, False, 1),
}
CASES = [(name, lay, place, side) for name, e in ENTRIES.items() for lay in e.layouts for place in (("rows", "ext") if e.extras else ("rows",))
         for side in range(e.sides)]


@pytest.mark.parametrize("name,layout,placement,side", CASES)
def test_strided_chunk_equals_dense_chunk(ctx, arena, name, layout, placement, side):
    import torch

    e = ENTRIES[name]
    b = _bundle(ctx, layout, E9 if e.extras else 0)
    dense = b.records(ctx, arena, None, e.with_rd)
    want = e.run(ctx, b, dense) if e.sides == 1 else e.run(ctx, b, dense, dense)
    ctx.sync()
    assert any(bool(t.any()) for t in want), "the dense chunk's outputs are all zero: nothing to compare"
    try:
        wide = b.records(ctx, arena, placement, e.with_rd)
        got = e.run(ctx, b, wide) if e.sides == 1 else (e.run(ctx, b, wide, dense) if side == 0 else e.run(ctx, b, dense, wide))
        ctx.sync()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(as_ints(g.contiguous()), as_ints(w.contiguous())), f"{name} ({layout}, {placement}, side {side}): output {i} differs"
    finally:
        arena.check_and_clear()


# ==== E. alignment streams with byte offsets beyond 2^31 and 2^32 (the arena of C) ====================================================================

def walk_pileup(ctx, bam, off, s):
    import torch

    keys = _t(s["keys"].view(np.int64))
    counts, check = fenced((len(s["keys"]), 8), torch.int32)
    counts.zero_()
    stats = torch.zeros((2,), dtype=torch.int64, device=ctx.device)
    ctx._check(ctx.lib.ampli_pileup_count(ctx.h, bam.data_ptr(), off.data_ptr(), off.numel(), keys.data_ptr(), keys.numel(), s["mbq"], s["mrq"], counts.data_ptr(),
                                          stats.data_ptr()))
    ctx.sync()
    check()
    return [counts, stats]


def walk_indel(ctx, bam, off, s):
    return list(ctx.indel_count(bam, off, _t(s["keys"].view(np.int64)), mbq=s["mbq"], mrq=s["mrq"]))


def walk_evidence(ctx, bam, off, s):
    return list(ctx.read_evidence(bam, off, _t(s["keys"].view(np.int64)), mbq=s["mbq"], mrq=s["mrq"]))


def walk_amplicon(ctx, bam, off, s):
    from tests import amplicon_count_model as acm

    a = s["amps"]
    return list(ctx.amplicon_count(bam, off, acm._up(a.lo), acm._up(a.hi), acm._up(a.reach), acm._up(a.amp_off), mbq=s["mbq"], mrq=s["mrq"]))


def model_pileup(s):
    from tests import pileup_model as pm

    counts, kept, added = pm.count(s["src"], s["keys"], s["mbq"], s["mrq"])
    return [counts, np.array([kept, added])]


def model_indel(s):
    from tests import indel_model as im

    r = im.count(s["src"], s["keys"], s["mbq"], s["mrq"])
    return [r.counts, r.lengths, np.array(r.stats)]


def model_evidence(s):
    from tests import evidence_model as em

    r = em.count(s["src"], s["keys"], s["mbq"], s["mrq"])
    return [r.hist, np.array(r.stats)]


def model_amplicon(s):
    from tests import amplicon_count_model as acm

    r = acm.count(s["src"], s["amps"], s["mbq"], s["mrq"])
    return [r.counts, r.amp_reads, np.array(r.stats)]


WALKS = {"pileup_count": (walk_pileup, model_pileup), "pileup_indel_count": (walk_indel, model_indel), "pileup_evidence": (walk_evidence, model_evidence),
         "pileup_amplicon_count": (walk_amplicon, model_amplicon)}
_WALK_DENSE = {}


@functools.lru_cache(maxsize=None)
def _wide_stream():
    from tests import amplicon_count_model as acm

    buf, off, keys, intervals, mbq, mrq = sh.bam_stream()
    return dict(src=(buf, off), keys=keys, amps=acm.make_amplicons(intervals), mbq=mbq, mrq=mrq)


@pytest.mark.parametrize("arrangement", ["staged", "fallback"])
@pytest.mark.parametrize("name", list(WALKS))
def test_a_stream_in_three_places_equals_the_dense_stream_and_the_model(ctx, arena, name, arrangement):
    """the four walks over records 2^31 and 2^32 bytes behind d_bam: "staged" has pileup_count_staged_kernel stage three groups at wide
    offsets, "fallback" has two groups straddle a gap, so that their span exceeds PILEUP_STAGE and the wave-per-read walk runs there"""
    import torch

    from tests import pileup_model as pm

    run, model = WALKS[name]
    s = _wide_stream()
    spans = sh.bam_group_spans(arrangement)
    staged = (spans[:, 1] - spans[:, 0] <= pm.geometry().stage).tolist()
    assert staged == {"staged": [True] * 4, "fallback": [True, False, False, True]}[arrangement]
    if name not in _WALK_DENSE:  # once per walk: the dense stream on the device, and the model
        dense = run(ctx, _t(s["src"][0]), _t(s["src"][1].view(np.int64)), s)
        ctx.sync()
        want = model(s)
        assert len(dense) == len(want) and all(w.any() for w in want)
        for i, (d, w) in enumerate(zip(dense, want)):
            assert np.array_equal(d.cpu().numpy().astype(np.int64).reshape(w.shape), w), f"{name}: output {i} on the dense stream differs from the model"
        _WALK_DENSE[name] = dense
    want = _WALK_DENSE[name]
    try:
        bam, off = arena.place_stream(arrangement)
        assert bam.data_ptr() % 16 == 0 and int(off[-1]) > 1 << 32 and bool((off[1:] > off[:-1]).all())
        got = run(ctx, bam, off, s)
        ctx.sync()
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and torch.equal(as_ints(g.contiguous()), as_ints(w.contiguous())), f"{name} ({arrangement}): output {i} differs from the dense stream's"
    finally:
        arena.check_and_clear()
