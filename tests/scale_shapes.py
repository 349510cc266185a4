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
