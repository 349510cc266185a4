"""The shapes of the index-range tests (tests/test_gpu_launch_splits.py, tests/test_gpu_wide_offsets.py) and the constants they rest
on, read from the kernel sources the way tests/pileup_model.py reads PILEUP_* -- TEST INFRASTRUCTURE.  tests/test_scale_shapes.py holds
every shape to its limit without a GPU: a constant that changes fails there rather than silently emptying a GPU test."""
import collections
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "amplisolve_amd", "csrc")
TYPES_H = os.path.join(ROOT, "include", "amplisolve_types.h")


def _text(name):
    return open(name if os.path.isabs(name) else os.path.join(CSRC, name)).read()


def _int(pattern, name, what):
    m = re.search(pattern, _text(name), re.M)
    assert m, f"no `{what}` line in {name}"
    return int(m.group(1))


Constants = collections.namedtuple(
    "Constants", "max_y grid_y gp_waves gp_run ex_rows pair_rows nb_rows cp_ta pc_samples ct_tile ad_rows limit_rows power_rows synth_rows")

SPLIT_FILES = ("ampli_fdr.hip", "ampli_dilution.hip", "ampli_paired.hip", "ampli_overdispersion.hip", "ampli_exceedance.hip")


@functools.lru_cache(None)
def constants():
    """what the launchers state: MAX_Y of the five split loops (one value), the y extent every refusal and the doubling of `run` test
    against, and the rows one y step of each launcher covers"""
    max_y = {f: _int(r"^\s*constexpr\s+(?:long long|int)\s+MAX_Y\s*=\s*(\d+)\s*;", f, "constexpr ... MAX_Y = ...;") for f in SPLIT_FILES}
    assert len(set(max_y.values())) == 1, max_y
    grid_y = {
        "genotype": _int(r"\(GP_WAVES \* run\) > (\d+)\) run <<= 1;", "ampli_concordance.hip", "while (... > 65535) run <<= 1;"),
        "concordance": _int(r"if \(ta > (\d+)\) return fail\(ctx, AMPLI_E_RANGE", "ampli_concordance.hip", "if (ta > 65535) return fail"),
        "contamination": _int(r"if \(tb > (\d+)\) return fail\(ctx, AMPLI_E_RANGE", "ampli_contamination.hip", "if (tb > 65535) return fail"),
        "amplicon": _int(r"if \(strips > (\d+)\) return fail\(ctx, AMPLI_E_RANGE", "ampli_amplicon.hip", "if (strips > 65535) return fail"),
        "poisson": _int(r"/ PC_SAMPLES > (\d+)\) return fail\(ctx, AMPLI_E_RANGE", "ampli_kernels.hip", "(T + PC_SAMPLES - 1) / PC_SAMPLES > 65535"),
    }
    assert set(grid_y.values()) == {max_y[SPLIT_FILES[0]]}, grid_y
    ex_rows = _int(r"^#define\s+AMPLI_EXCEEDANCE_ROWS\s+(\d+)", TYPES_H, "#define AMPLI_EXCEEDANCE_ROWS")
    assert re.search(r"^constexpr int EX_ROWS = AMPLI_EXCEEDANCE_ROWS;", _text("ampli_exceedance.hip"), re.M)
    assert re.search(r"\(int\)\(g0 \* EX_ROWS\)", _text("ampli_exceedance.hip"))
    pair_rows = _int(r"groups = \(\(long long\)n_pairs \+ 3\) / (\d+);", "ampli_paired.hip", "groups = ((long long)n_pairs + 3) / 4;")
    assert _int(r"\(int\)\(g0 \* (\d+)\), d_ref_code", "ampli_paired.hip", "(int)(g0 * 4)") == pair_rows
    nb_rows = _int(r"groups = \(\(long long\)co\.n \+ 3\) / (\d+);", "ampli_overdispersion.hip", "groups = ((long long)co.n + 3) / 4;")
    assert _int(r"co\.n, \(int\)\(g0 \* (\d+)\)", "ampli_overdispersion.hip", "(int)(g0 * 4)") == nb_rows
    ad_waves = _int(r"^constexpr int AD_WAVES = (\d+);", "ampli_amplicon.hip", "constexpr int AD_WAVES = ...;")
    ad_strip = _int(r"^constexpr int AD_STRIP = (\d+);", "ampli_amplicon.hip", "constexpr int AD_STRIP = ...;")
    ct_tile = _int(r"const long long tb = \(\(long long\)n_b \+ \d+\) / (\d+);", "ampli_contamination.hip", "tb = ((long long)n_b + 63) / 64;")
    assert _int(r"const long long b = \(long long\)blockIdx\.y \* (\d+) \+ lane;", "ampli_contamination.hip", "b = blockIdx.y * 64 + lane") == ct_tile
    return Constants(
        max_y=max_y[SPLIT_FILES[0]], grid_y=grid_y["genotype"],
        gp_waves=_int(r"^constexpr int GP_WAVES = (\d+);", "ampli_concordance.hip", "constexpr int GP_WAVES = ...;"),
        gp_run=_int(r"^\s*int run = (\d+);", "ampli_concordance.hip", "int run = 16;"),
        ex_rows=ex_rows, pair_rows=pair_rows, nb_rows=nb_rows,
        cp_ta=_int(r"^constexpr int CP_TA = (\d+),", "ampli_concordance.hip", "constexpr int CP_TA = ...,"),
        pc_samples=_int(r"^constexpr int PC_SAMPLES = (\d+);", "ampli_kernels.hip", "constexpr int PC_SAMPLES = ...;"),
        ct_tile=ct_tile, ad_rows=ad_waves * ad_strip,
        limit_rows=_int(r"if \(co\.n > (\d+)\) return fail\(ctx, AMPLI_E_RANGE, \"limit_records:", "ampli_limits.hip", "limit_records: co.n > 65535"),
        power_rows=_int(r"if \(co\.n > (\d+)\) return fail\(ctx, AMPLI_E_RANGE, \"power_records:", "ampli_limits.hip", "power_records: co.n > 65535"),
        synth_rows=_int(r"if \(n_samples > (\d+)\) return fail\(ctx, AMPLI_E_RANGE, \"synth_fill:", "ampli_aux.hip", "synth_fill: n_samples > 65535"))


# ---- A: the smallest shapes that reach a second launch with a partial last group, over a partial position tile ------------------------
# (rows, P, rows of one y step): written out as the issue states them, held to the constants by tests/test_scale_shapes.py
Y = 65535
SPLITS = {
    "fdr_adjust": dict(rows=Y + 3, P=(5,), step=1),
    "dilute": dict(rows=Y + 2, P=(17,), step=1),
    "pair_score": dict(rows=4 * Y + 5, P=(1, 65), step=4),
    "nb_score": dict(rows=4 * Y + 5, P=(3,), step=4),
    "exceedance": dict(rows=8 * Y + 3, P=(3,), step=8),
}
GENOTYPE = dict(rows=Y * 4 * 16 + 7, P=(1, 65))
EXCEEDANCE_NORMALS = 5

# ---- B: the largest row count each refusing entry point takes ------------------------------------------------------------------------
LIMITS = {"limit_records": Y, "power_records": Y, "amplicon_depth_records": 2097120, "concordance_pairs": 2097120,
          "contamination_records": 4194240, "poisson_call": 262140, "synth_fill": Y}

# ---- C: three rows of P = 130 records whose row stride puts row 1 just past 2^31 and row 2 just past 2^32 bytes from the base, the
# base itself 2 GiB into the allocation; E = 9 extras placed the same way.  A stride is a whole number of records in every layout.
WIDE_P, WIDE_N, WIDE_E = 130, 3, 9
REC_BYTES = {"i32": 32, "u24": 24, "u16": 16}
WIDE_BASE = 1 << 31


def wide_stride(layout):
    """records between two rows: row 1 starts a row's length past 2^31 bytes and row 2 two rows' lengths past 2^32, so that row 2's
    offsets cut to 32 bits fall behind row 0's records, on the pattern, and not onto them"""
    return (1 << 31) // REC_BYTES[layout] + WIDE_P + 1


def wide_bytes(layout):
    """bytes of the allocation: the base offset, two strides and the last row's records"""
    return WIDE_BASE + (2 * wide_stride(layout) + max(WIDE_P, WIDE_E)) * REC_BYTES[layout]


# ---- D: outputs beyond 2^32 bytes: n rows of P positions, eight 4-byte values each --------------------------------------------------
BIG_ROWS, BIG_P = 4 * Y + 5, 520


BIG_ROW_BYTES = BIG_P * 8 * 4


def big_special_rows():
    """row 0, the first row that starts past 2^31 bytes (where a signed 32-bit byte offset, or an unsigned 32-bit count of half-cells,
    wraps), the first that starts past 2^32 bytes, and the last row.  The whole output is 1.09e9 four-byte elements: an offset of 2^31
    ELEMENTS does not exist at this shape."""
    return (0, -(-(1 << 31) // BIG_ROW_BYTES), -(-(1 << 32) // BIG_ROW_BYTES), BIG_ROWS - 1)


# ---- E: alignment streams whose byte offsets pass 2^31 and 2^32.  One allocation filled with the byte 0x01, d_bam 2 GiB into it; the
# records of one stream lie in three places: at d_bam, BAM_ROOM past 2^31 bytes from it and 2 * BAM_ROOM past 2^32.  A place holds less
# than BAM_ROOM bytes, so an offset of place 2 cut to 32 bits lands in [2 * BAM_ROOM, 3 * BAM_ROOM) -- behind place 0's records -- and an
# offset of place 1 sign-extended from 32 bits lands BAM_ROOM bytes into the allocation, 2 GiB below d_bam: on the pattern both times.
BAM_BASE = 1 << 31
BAM_ROOM = 1 << 20
BAM_PLACES = (0, (1 << 31) + BAM_ROOM, (1 << 32) + 2 * BAM_ROOM)
BAM_READS = 3 * 256 + 40
BAM_SHIFT = 100
BAM_SOURCE = "fuzz_12_2048_reads"  # of tests/pileup_model.py: short amplicon reads with indels, clips, odd operations, both strands, a full panel
BAM_PATTERN = 0x01


def bam_bytes():
    """bytes of the allocation: the base offset, the last place and its room"""
    return BAM_BASE + BAM_PLACES[2] + BAM_ROOM


@functools.lru_cache(None)
def bam_filtered_mask():
    """BAM_FILTERED as csrc/ampli_bam.h states it"""
    m = re.search(r"^constexpr unsigned BAM_FILTERED = ([^;]+);", _text("ampli_bam.h"), re.M)
    assert m, "no `constexpr unsigned BAM_FILTERED = ...;` line in ampli_bam.h"
    mask = 0
    for term in m.group(1).split("|"):
        mask |= int(term.strip().rstrip("u"), 16)
    return mask


def bam_cuts(arrangement):
    """the reads [cut[k], cut[k + 1]) lie in place k.  "staged": every group of 256 consecutive reads lies wholly inside one place (the
    last, partial group behind the third); "fallback": the same stream with the cuts BAM_SHIFT reads later, so that the second and the
    third group each straddle a gap"""
    shift = {"staged": 0, "fallback": BAM_SHIFT}[arrangement]
    return (0, 256 + shift, 512 + shift, BAM_READS)


@functools.lru_cache(None)
def bam_stream():
    """(buf, rec_off, keys, intervals, mbq, mrq): the first BAM_READS reads of BAM_SOURCE as a dense stream, its panel, and the design
    tests/walk_cross.design_of derives from the panel for the amplicon walk; mbq = mrq = 20 (the case's own 40 / 21 keep a third of
    the reads and a tenth of their bases)"""
    from tests import pileup_model as pm
    from tests import walk_cross as wc

    case = next(c for c in pm.cases() if c.name == BAM_SOURCE)
    buf, off = pm.build_stream(case.reads[:BAM_READS], lead=5, trail=16)
    for a in (buf, off):
        a.setflags(write=False)
    return buf, off, case.keys, tuple(wc.design_of(case.keys)), 20, 20


def bam_layout(arrangement):
    """([(offset from d_bam, first byte, end byte in the dense buffer)] per place, rec_off of the placed stream): a place's records keep
    their distances and the 16-byte phase of the place's first record"""
    import numpy as np

    from tests import pileup_model as pm

    buf, off = bam_stream()[:2]
    end = pm.headers(buf, off).end
    cuts = bam_cuts(arrangement)
    o = off.astype(np.int64)
    pieces, wide = [], np.empty(len(o), np.int64)
    for k in range(3):
        a, b = cuts[k], cuts[k + 1]
        at = BAM_PLACES[k] + int(o[a] & 15)
        pieces.append((at, int(o[a]), int(end[b - 1])))
        wide[a:b] = at + (o[a:b] - o[a])
    return pieces, wide.astype(np.uint64)


def bam_group_spans(arrangement):
    """int64 [groups][2] of the placed stream, as tests/pileup_model.group_spans computes them: from a group's first offset rounded down
    to 16 to the end of its last record"""
    import numpy as np

    from tests import pileup_model as pm

    buf, off = bam_stream()[:2]
    size = pm.headers(buf, off).end - off.astype(np.int64)
    wide = bam_layout(arrangement)[1].astype(np.int64)
    R = pm.geometry().reads
    first = wide[0::R]
    last = np.minimum(np.arange(len(first)) * R + R, len(wide)) - 1
    return np.stack([first & ~np.int64(15), wide[last] + size[last]], 1)


# ---- F: outputs of the read walks beyond 2^32 bytes: cells of `cell_bytes` bytes per key (or walk entry), real work on four of them
CELL_BYTES = {"evidence_hist": 3072, "indel_lengths": 256, "pileup_counts": 32, "amplicon_counts": 32, "layers_total": 32}
CELL_EXTRA = 1000  # cells behind the first one past 2^32 bytes


def special_cells(cell_bytes):
    """(cells, (0, the first cell that starts at or past 2^31 bytes, the first at or past 2^32 bytes, the last cell))"""
    c31, c32 = -(-(1 << 31) // cell_bytes), -(-(1 << 32) // cell_bytes)
    n = c32 + CELL_EXTRA
    return n, (0, c31, c32, n - 1)
