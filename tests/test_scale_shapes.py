"""The shapes of tests/test_gpu_launch_splits.py and tests/test_gpu_wide_offsets.py against the constants of the kernel sources
(tests/scale_shapes.py reads them): every shape still crosses the limit it was chosen for.  No GPU."""
import pytest

from tests import scale_shapes as sh


def test_the_constants_are_the_ones_the_shapes_were_written_for():
    c = sh.constants()
    assert c.max_y == c.grid_y == sh.Y
    from amplisolve_amd.api import EXCEEDANCE_ROWS

    assert c.ex_rows == EXCEEDANCE_ROWS


@pytest.mark.parametrize("name", sorted(sh.SPLITS))
def test_split_shapes_reach_a_second_launch_with_a_partial_last_group(name):
    c = sh.constants()
    step = {"fdr_adjust": 1, "dilute": 1, "pair_score": c.pair_rows, "nb_score": c.nb_rows, "exceedance": c.ex_rows}[name]
    s = sh.SPLITS[name]
    assert s["step"] == step
    rows, first = s["rows"], c.max_y * step  # the rows of the first launch
    groups = -(-rows // step)
    assert c.max_y < groups <= 2 * c.max_y, "exactly two launches"
    rem = rows - first  # the rows of the second launch: a few groups at the most, the last one partial
    assert 0 < rem <= max(2 * step, 3)
    assert step == 1 or rem % step != 0, "the last group of the second launch is partial"
    tile = {"fdr_adjust": 256, "dilute": 16, "pair_score": 64, "nb_score": 64, "exceedance": 64}[name]
    assert all(P % tile != 0 for P in s["P"]), "a partial position tile"
    if name == "pair_score":
        assert any(P > tile for P in s["P"]) and any(P < tile for P in s["P"])


def test_genotype_shape_doubles_the_run():
    c = sh.constants()
    n = sh.GENOTYPE["rows"]
    per = c.gp_waves * c.gp_run
    assert -(-n // per) > c.grid_y >= -(-(n - 7) // per), "one partial group past the grid's y extent at the initial run"
    assert -(-n // (2 * per)) <= c.grid_y, "one doubling is enough"
    assert n % (2 * c.gp_run) != 0, "the last wave's run is partial"
    assert sh.GENOTYPE["P"] == (1, 65)  # one word with one bit; a full word and one bit of a second


def test_every_limit_is_the_last_row_count_that_fits_the_grid():
    c = sh.constants()
    per_y = {"limit_records": 1, "power_records": 1, "amplicon_depth_records": c.ad_rows, "concordance_pairs": c.cp_ta,
             "contamination_records": c.ct_tile, "poisson_call": c.pc_samples, "synth_fill": 1}
    assert set(per_y) == set(sh.LIMITS)
    assert c.limit_rows == c.power_rows == c.synth_rows == c.grid_y
    for name, rows in sh.LIMITS.items():
        assert rows == c.grid_y * per_y[name], name
        assert -(-rows // per_y[name]) == c.grid_y and -(-(rows + 1) // per_y[name]) == c.grid_y + 1, name


def test_the_refusal_messages_name_their_limits():
    """the number a message gives is the largest count the call takes"""
    import re

    for f, name in (("ampli_limits.hip", "limit_records"), ("ampli_limits.hip", "power_records"), ("ampli_amplicon.hip", "amplicon_depth_records"),
                    ("ampli_concordance.hip", "concordance_pairs"), ("ampli_contamination.hip", "contamination_records"),
                    ("ampli_kernels.hip", "poisson_call"), ("ampli_aux.hip", "synth_fill")):
        msgs = re.findall(r'AMPLI_E_RANGE,\s*"%s: ([^"]*)"' % name, sh._text(f))
        hit = [m for m in msgs if str(sh.LIMITS[name]) in m]
        assert len(hit) == 1, (name, msgs)
        assert re.search(r"more than %d|at most %d" % (sh.LIMITS[name], sh.LIMITS[name]), hit[0]), hit[0]


@pytest.mark.parametrize("layout", sorted(sh.REC_BYTES))
def test_wide_strides_put_the_rows_past_two_to_the_31_and_32(layout):
    rb, stride = sh.REC_BYTES[layout], sh.wide_stride(layout)
    row1, row2 = stride * rb, 2 * stride * rb
    assert (1 << 31) + sh.WIDE_P * rb < row1 <= (1 << 31) + (sh.WIDE_P + 2) * rb and (1 << 32) < row2 == 2 * row1
    last = row2 + max(sh.WIDE_P, sh.WIDE_E) * rb
    assert sh.wide_bytes(layout) == sh.WIDE_BASE + last
    # an offset cut to 32 bits, or sign-extended from 32 bits, of any record of rows 1 and 2 lands inside the allocation and outside
    # every row: on the pattern
    rows = [(r * stride * rb, r * stride * rb + sh.WIDE_P * rb) for r in range(sh.WIDE_N)]
    for r in (1, 2):
        for p in (0, sh.WIDE_P - 1):
            off = (r * stride + p) * rb
            low = off & 0xFFFFFFFF
            signed = low - (1 << 32) if low >= 1 << 31 else low
            for wrong in {low, signed} - {off}:
                assert -sh.WIDE_BASE <= wrong and wrong + rb <= last, (layout, r, p, wrong)
                assert not any(lo - rb < wrong < hi for lo, hi in rows), (layout, r, p, wrong)
    assert sh.wide_bytes(layout) <= 7 << 30


@pytest.mark.parametrize("layout", sorted(sh.REC_BYTES))
def test_a_32_bit_record_offset_reads_the_pattern(layout):
    """The kernels' record address, `base + (row * row_stride + p) * rec_bytes`, restated on the CPU in three widths over a map of the
    allocation: in 64 bits every record is the row's; with the byte offset kept in an int (sign-extended) every record of rows 1 and 2,
    and with it cut to 32 bits (unsigned) every record of row 2, comes from the pattern fill instead, which decodes to a present
    record no row holds -- so every output that depends on those rows differs from the dense chunk's.  (RecView's strides are long long and p is long long: dropping ONE of
    the three size_t casts of an address leaves the arithmetic 64 bits wide and changes nothing; what the GPU tests catch is a product
    or an offset held in 32 bits.)  Not a wrong value but an access below the allocation: a row STEP kept in an int and added twice
    (compact_reduce_body's `q += row_step`), which reaches 4 GiB below the base -- the base lies only 2 GiB in."""
    import numpy as np

    rb, stride, P = sh.REC_BYTES[layout], sh.wide_stride(layout), sh.WIDE_P
    size = sh.wide_bytes(layout)
    rows = {r: r * stride * rb for r in range(sh.WIDE_N)}

    def at(off):
        """what a record load at byte offset `off` from the base returns: (row, p), "pattern", or None outside the allocation"""
        if off < -sh.WIDE_BASE or off + rb > size - sh.WIDE_BASE:
            return None
        for r, lo in rows.items():
            if lo - rb < off < lo + P * rb:
                return (r, (off - lo) // rb) if (off - lo) % rb == 0 and off >= lo else "row bytes"
        return "pattern"

    def sext(x):
        x &= 0xFFFFFFFF
        return x - (1 << 32) if x >> 31 else x

    for r in range(sh.WIDE_N):
        for p in range(P):
            off = (r * stride + p) * rb
            assert at(off) == (r, p)
            narrow = (at(off & 0xFFFFFFFF), at(sext(off)))
            # row 1 lies between 2^31 and 2^32: only the signed form loses it; row 2 lies past 2^32: both do
            assert narrow == {0: ((0, p), (0, p)), 1: ((1, p), "pattern"), 2: ("pattern", "pattern")}[r], (layout, r, p, narrow)
    assert at(sext(stride * rb)) == "pattern" and at(2 * sext(stride * rb)) is None  # the int step: once on the pattern, twice below it
    # the pattern as a record: present, the same count in every field, above the cohort's 16-bit counts in the wider layouts
    raw = np.full(rb, 0x01, np.uint8)
    if layout == "u24":
        b3 = raw.reshape(8, 3).astype(np.int64)
        fields = b3[:, 0] | b3[:, 1] << 8 | b3[:, 2] << 16
    else:
        fields = raw.view("<i4" if layout == "i32" else "<u2")
    assert len(fields) == 8 and set(int(f) for f in fields) == {{"i32": 0x01010101, "u16": 0x0101, "u24": 0x010101}[layout]}


def test_big_outputs_pass_two_to_the_32_bytes():
    r0, r31, r32, last = sh.big_special_rows()
    assert r0 == 0 and last == sh.BIG_ROWS - 1 and r31 < r32 < last
    assert (r31 - 1) * sh.BIG_ROW_BYTES < (1 << 31) <= r31 * sh.BIG_ROW_BYTES
    assert (r32 - 1) * sh.BIG_ROW_BYTES < (1 << 32) <= r32 * sh.BIG_ROW_BYTES
    assert sh.BIG_ROWS * sh.BIG_ROW_BYTES > 1 << 32 and sh.BIG_ROWS == sh.SPLITS["pair_score"]["rows"]
    assert sh.BIG_ROWS * sh.BIG_ROW_BYTES + (256 << 20) <= 6 << 30  # the output and its inputs stay far below 12 GiB


# ---- alignment streams in three places (tests/test_gpu_wide_offsets.py, part E) -------------------------------------------------------

def test_the_pattern_decodes_as_a_filtered_read():
    """an offset that misses its record lands on bytes of 0x01: as a header, block_size, ref_id and pos 0x01010101 (placed), MAPQ 1 and
    flag 0x0101, whose secondary bit is in BAM_FILTERED -- the read is not kept whatever mrq is: a missing read, not a fault"""
    import struct

    word = struct.unpack("<I", bytes([sh.BAM_PATTERN]) * 4)[0]
    assert word == 0x01010101
    flag, n_cigar = word >> 16, word & 0xFFFF
    mask = sh.bam_filtered_mask()
    assert mask == 0x4 | 0x100 | 0x200 | 0x400 and flag == 0x0101 and flag & mask == 0x100
    from tests import pileup_model as pm

    assert pm.READ_MASK == mask  # the models filter as the header does
    assert struct.unpack("<i", bytes([sh.BAM_PATTERN]) * 4)[0] > 0  # ref_id and pos: a placed read, so it is the FLAG that drops it
    # as a group's last record the pattern gives a block_size of 16 MiB: the group is not staged, and its walk drops every such read
    assert word > pm.geometry().stage and n_cigar > 0


@pytest.mark.parametrize("arrangement", ["staged", "fallback"])
def test_the_three_places_of_the_stream_and_what_a_narrowed_offset_reads(arrangement):
    import numpy as np

    from tests import pileup_model as pm

    buf, off = sh.bam_stream()[:2]
    assert len(off) == sh.BAM_READS == 3 * pm.geometry().reads + 40
    pieces, wide = sh.bam_layout(arrangement)
    wide = wide.astype(np.int64)
    size = pm.headers(buf, off).end - off.astype(np.int64)
    assert np.all(np.diff(wide) > 0), "rec_off ascends across the three places"
    # the places: at the base, just past 2^31 and just past 2^32 bytes from it; each holds records and stays inside its room
    spans = [(at, at + hi - lo) for at, lo, hi in pieces]
    for k, (a, b) in enumerate(spans):
        assert sh.BAM_PLACES[k] <= a < b <= sh.BAM_PLACES[k] + sh.BAM_ROOM - 16, (k, a, b)
    assert spans[0][0] < 16 and (1 << 31) < spans[1][0] < (1 << 31) + 2 * sh.BAM_ROOM and (1 << 32) < spans[2][0] < (1 << 32) + 3 * sh.BAM_ROOM
    assert sh.bam_bytes() == sh.BAM_BASE + sh.BAM_PLACES[2] + sh.BAM_ROOM and sh.bam_bytes() <= 7 << 30
    # every record's bytes are the dense stream's
    for at, lo, hi in pieces:
        inside = (wide >= at) & (wide < at + hi - lo)
        assert np.array_equal(wide[inside] - at, off.astype(np.int64)[inside] - lo)
    cuts = sh.bam_cuts(arrangement)
    assert [int(((wide >= a) & (wide < b)).sum()) for a, b in spans] == [cuts[k + 1] - cuts[k] for k in range(3)]

    def reads_pattern(x, n):
        """bytes [x, x + n) from d_bam lie inside the allocation and on none of the placed records"""
        return -sh.BAM_BASE <= x and x + n <= sh.bam_bytes() - sh.BAM_BASE and not any(x < b and x + n > a for a, b in spans)

    lost_cut = lost_signed = 0
    for o, n in zip(wide.tolist(), size.tolist()):
        low = o & 0xFFFFFFFF
        signed = low - (1 << 32) if low >> 31 else low
        for wrong, is_cut in ((low, True), (signed, False)):
            if wrong != o:
                assert reads_pattern(wrong, 36 + 16), (arrangement, o, wrong)  # the header and the piece a staged copy starts with
                lost_cut += is_cut
                lost_signed += not is_cut
    n1, n2 = cuts[2] - cuts[1], cuts[3] - cuts[2]
    assert lost_cut == n2 and lost_signed == n1 + n2, "place 1 is lost to a signed 32-bit offset, place 2 to either"
    # the 16 bytes behind the last record are the allocation's
    assert int(wide[-1] + size[-1]) + 16 <= sh.bam_bytes() - sh.BAM_BASE


def test_the_arrangements_take_the_staged_path_and_the_fallback():
    from tests import pileup_model as pm

    stage = pm.geometry().stage
    s = sh.bam_group_spans("staged")
    assert len(s) == 4 and (s[:, 1] - s[:, 0] <= stage).all() and (s[1:, 0] > 1 << 31).all() and s[2, 0] > 1 << 32
    f = sh.bam_group_spans("fallback")
    assert (f[:, 1] - f[:, 0] <= stage).tolist() == [True, False, False, True]
    assert f[1, 0] < 1 << 31 < f[1, 1] and f[2, 0] < 1 << 32 < f[2, 1], "the second and third group each straddle a gap"
    # on the dense stream every group is staged (the spans are pileup_model.group_spans' own there)
    d = pm.group_spans(*sh.bam_stream()[:2])
    assert (d[:, 1] - d[:, 0] <= stage).all()
    # the stream holds what the walks tell apart
    buf, off, keys, intervals, mbq, mrq = sh.bam_stream()
    h = pm.headers(buf, off)
    ops = set()
    for c, n in zip(h.cig.tolist(), h.n_cigar.tolist()):
        ops |= {int(buf[c + 4 * k]) & 15 for k in range(n)}
    assert {0, 1, 2, 4} <= ops and ((h.flag & 0x10) != 0).any() and ((h.flag & 0x10) == 0).any() and ((h.flag & pm.READ_MASK) != 0).any()


# ---- the read walks' outputs beyond 2^32 bytes (tests/test_gpu_wide_offsets.py, part F) ---------------------------------------------

@pytest.mark.parametrize("name", sorted(sh.CELL_BYTES))
def test_special_cells_start_at_two_to_the_31_and_32_bytes(name):
    b = sh.CELL_BYTES[name]
    n, (c0, c31, c32, last) = sh.special_cells(b)
    assert c0 == 0 and last == n - 1 and 0 < c31 < c32 < last
    assert (c31 - 1) * b < (1 << 31) <= c31 * b and (c32 - 1) * b < (1 << 32) <= c32 * b
    assert n * b > 1 << 32 and n * b + (2 << 30) <= 12 << 30
    assert n < 1 << 31  # key positions and walk entries are 32-bit
    from amplisolve_amd.api import EVIDENCE_BINS, EVIDENCE_METRICS, INDEL_LEN_BINS

    assert sh.CELL_BYTES == {"evidence_hist": 4 * EVIDENCE_METRICS * EVIDENCE_BINS * 4, "indel_lengths": 2 * INDEL_LEN_BINS * 4, "pileup_counts": 32,
                             "amplicon_counts": 32, "layers_total": 32}


def test_the_special_streams_touch_their_four_keys_only():
    """the big panels are a plain arange; the models run on the four special keys alone.  That is the whole answer only if no read
    counts anything on a neighbouring key: checked here on a panel of the four keys and the five positions behind each"""
    import numpy as np

    from tests import evidence_model as em
    from tests import indel_model as im
    from tests import pileup_model as pm
    from tests.test_gpu_wide_offsets import ONE_COLUMN, ONE_JUNCTION, special_stream

    assert pm.geometry().reads == im.geometry().reads == em.geometry().reads == 256
    where = [(0, 1), (0, 70001), (0, 140001), (0, 141000)]
    four = np.asarray([p for _, p in where], np.uint64)
    near = np.unique(np.concatenate([four + np.uint64(d) for d in range(6)] + [four[1:] - np.uint64(1)]))
    at = np.searchsorted(near, four)
    src = special_stream(where, ONE_COLUMN, 1)
    assert len(src[1]) == 4 * 256
    for counts4, counts in ((pm.count(src, four, 30, 20)[0], pm.count(src, near, 30, 20)[0]), (em.count(src, four, 30, 20).hist, em.count(src, near, 30, 20).hist)):
        assert np.array_equal(counts[at], counts4) and counts.sum() == counts4.sum() and all(counts4[i].any() for i in range(4))
    src = special_stream(where, ONE_JUNCTION, 2)
    r4, r = im.count(src, four, 30, 20), im.count(src, near, 30, 20)
    assert np.array_equal(r.counts[at], r4.counts) and np.array_equal(r.lengths[at], r4.lengths) and r.stats == r4.stats and r.counts.sum() == r4.counts.sum()
    assert (r4.counts[:, :3] > 0).all() and (r4.lengths.sum(2) > 0).all()


# ---- every walk over every table (tests/test_gpu_walks_cross_tables.py) ------------------------------------------------------------

def test_the_design_rule():
    import numpy as np

    from tests import walk_cross as wc
    from tests.pileup_model import make_keys, span_keys

    keys = make_keys([(0, p) for p in range(100, 141)] + [(0, p) for p in range(200, 240)] + [(0, 500)] + [(1, p) for p in range(1, 101)] + [(2, 101)])
    assert wc.runs_of(keys) == [(0, 100, 140), (0, 200, 239), (0, 500, 500), (1, 1, 100), (2, 101, 101)]
    # 41 positions: a second amplicon from the middle of the run to a quarter of its length behind it; 40: none
    assert wc.design_of(keys) == [(0, 100, 140), (0, 120, 150), (0, 200, 239), (0, 500, 500), (1, 1, 100), (1, 51, 125), (2, 101, 101)]
    assert wc.runs_of(np.concatenate([span_keys(0, 2 ** 31 - 3, 2 ** 31 - 2), span_keys(1, 1, 2)])) == [(0, 2 ** 31 - 3, 2 ** 31 - 2), (1, 1, 2)]
    for table in ("pileup", "indel", "evidence"):
        for s in wc.streams(table):
            runs = set(wc.runs_of(s.keys))
            assert np.array_equal(wc.keys_of([iv for iv in s.intervals if iv in runs]), s.keys), s.name  # the runs are the panel
            assert all(1 <= f <= l < 2 ** 31 for _, f, l in s.intervals), s.name
    for s in wc.streams("amplicon"):
        assert np.array_equal(s.keys, wc.keys_of(s.intervals)) and np.all(np.diff(s.keys.astype(np.int64)) > 0)


def test_every_table_is_used_whole_and_no_pair_passes_vacuously():
    from tests import amplicon_count_model as am
    from tests import evidence_model as em
    from tests import indel_model as im
    from tests import pileup_model as pm
    from tests import walk_cross as wc

    tables = {"pileup": pm.cases(), "indel": im.cases(), "evidence": em.cases(), "amplicon": am.cases()}
    for name, cases in tables.items():
        left_out = sorted({c.name for c in cases} - {s.name for s in wc.streams(name)})
        assert left_out == ([wc.LEFT_OUT] if name == "pileup" else []), (name, left_out)
    share, designs = wc.non_vacuity()
    assert sorted(share) == sorted(wc.PAIRS) and len(share) == 12
    for pair, (cases, non_zero) in share.items():
        assert cases == len(wc.streams(pair[1])) and 2 * non_zero >= cases, (pair, cases, non_zero)
    for table, (by_overlap, off_target, both) in designs.items():
        assert both >= 1 and by_overlap >= both and off_target >= both, (table, by_overlap, off_target, both)
    # a pileup-ready stream of every case: ascending offsets and 16 bytes behind the last record
    import numpy as np

    for name in tables:
        for s in wc.streams(name):
            buf, off = wc.staged_stream(s)
            assert np.all(np.diff(off.astype(np.int64)) > 0) and len(buf) - int(pm.headers(buf, off).end.max()) >= 16, s.name


# ---- the five later rows of ENTRIES (tests/test_gpu_wide_offsets.py, part C) ----------------------------------------------------------

def test_the_later_entry_points_have_something_to_compare_on_the_bundles_records():
    """the features' own lists, thresholds and planes, cut to 3 rows of 130 positions, over the bundle's records in the models: entries
    are evaluated and alternative reads counted, control lists evaluate, fractions are estimated, het sites are taken into the
    reference and cells are tested -- so that a strided chunk that read the pattern instead would differ from the dense chunk"""
    import numpy as np

    from tests import allelic_model as alm
    from tests import fraction_model as fm
    from tests import monitor_model as mm
    from tests import test_gpu_wide_offsets as w

    h, recs = w.wide_inputs(), w._cohort(0)["recs"]
    assert recs.shape == (sh.WIDE_N, sh.WIDE_P, 8) and h["f_thr"].shape == (2, 4, sh.WIDE_P) and h["planes_own"].shape[0] == sh.WIDE_N
    sums, _ = mm.sums_model(recs, w.P, h["m_thr"], h["m_ref"], h["m_off"], h["m_cell"], h["cov"], 1000)
    assert (sums[:, :, mm.N_EVAL].sum(1) > 0).all() and sums[:, :, mm.K_FW].any() and sums[:, :, mm.K_BW].any()
    sums, _ = mm.controls_model(recs, w.P, h["m_thr"], h["m_ref"], h["m_off"], h["m_cell"], h["pairs"], h["cand_off"], h["cand_pos"], 3, 2, h["seed"], h["cov"], 1000)
    assert sums[:, :, mm.N_EVAL].any()
    est, count = fm.fraction_model(recs, w.P, h["f_thr"], h["f_ref"], h["f_off"], h["f_cell"], h["f_w"], h["f_cov"])
    assert (count[:, :, 0].sum(1) > 0).all() and (est != fm.NA).any()
    for r in range(sh.WIDE_N):  # every row adds het sites of its own to the reference
        assert alm.reference(recs[r:r + 1], h["bits_own"][r:r + 1], w.P, h["min_depth"])[0].sum() >= 10, r
    code = alm.sites(recs, w.P, h["bits_pool"], h["row_g"], h["het_ref"], h["min_depth"], h["min_normals"], True)[3]
    assert (((code >> 3) >= alm.TESTED_REF).sum(1) >= 10).all()  # ... and has tested cells
    assert all(0 <= g < h["planes_pool"].shape[0] for g in h["row_g"]) and len(h["row_g"]) == sh.WIDE_N
    # rows 1 and 2 -- the rows a narrowed offset loses -- take part in each of them
    assert (np.abs(sums).reshape(len(h["pairs"]), -1).sum(1)[[1, 3, 7]] > 0).any()  # pairs that name rows 2 and 1 (monitor_cases.control_case)
