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
