"""ampli_pileup_count itself, one call per case of the table of tests/pileup_model.py, against the vectorised numpy reference:
exact integer equality of the counts (on top of a non-zero pre-fill, between two guard rows) and of the stats.  The executable
(tests/test_gpu_pileup.py) chooses batch cuts, offsets and padding on its own; here the test does, so the group sizes, the LDS
stage threshold, the 16-byte phases, the byte alignments inside LDS and the window's edges are all met on purpose.  The wave-per-read
build (-DAMPLI_PILEUP_WAVE_PER_READ, the comparison form of tools/pileup_bench.py) runs the same table in a child process."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from amplisolve_amd import build
from tests import pileup_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pm.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_counts_and_stats_equal_the_reference(ctx, case):
    t0 = time.perf_counter()
    found = pm.device_check(ctx.lib, ctx.h, case)
    print(f"{case!r}: {time.perf_counter() - t0:.3f} s incl. upload and reference; groups staged {int(case.staged().sum())}/{len(case.staged())}")
    assert not found, found


def _pick(*names):
    by = {c.name: c for c in CASES}
    return [by[n] for n in names]


def test_two_batches_accumulate_like_one(ctx):
    """a file's batches add up: two different streams counted one after the other into the same buffers = both in one stream"""
    a, b = _pick("walk_across_2000_positions", "one_read_of_100000_bases")
    assert np.array_equal(a.keys, b.keys) and (a.mbq, a.mrq) == (b.mbq, b.mrq)
    d = pm.DeviceBuffers(len(a.keys))
    assert d.call(ctx.lib, ctx.h, a) == 0 and d.call(ctx.lib, ctx.h, b) == 0
    both = pm.Case("both", list(a.reads) + list(b.reads), a.keys, a.mbq, a.mrq)
    one = pm.DeviceBuffers(len(a.keys))
    assert one.call(ctx.lib, ctx.h, both) == 0
    wa, wb = a.want(), b.want()
    want = (wa[0] + wb[0], wa[1] + wb[1], wa[2] + wb[2])
    assert both.want()[1:] == want[1:] and np.array_equal(both.want()[0], want[0])
    assert not d.mismatches(*want) and not one.mismatches(*want)
    assert np.array_equal(d.counts.cpu().numpy(), one.counts.cpu().numpy()) and d.stats.tolist() == one.stats.tolist()


@pytest.mark.parametrize("name", ["group_size_513", "stage_over_phase7", "holes_inside_match_runs", "fuzz_13_3000_reads"])
def test_the_same_call_twice_doubles_the_counts(ctx, name):
    case, = _pick(name)
    d = pm.DeviceBuffers(len(case.keys))
    assert d.call(ctx.lib, ctx.h, case) == 0 and d.call(ctx.lib, ctx.h, case) == 0
    counts, kept, added = case.want()
    assert added > 0 and not d.mismatches(2 * counts, 2 * kept, 2 * added)


@pytest.mark.parametrize("name", ["group_size_257", "only_middle_group_unstaged", "walk_across_2000_positions", "fuzz_16_8000_reads"])
def test_counts_without_a_stats_buffer(ctx, name):
    case, = _pick(name)
    d = pm.DeviceBuffers(len(case.keys))
    assert d.call(ctx.lib, ctx.h, case, stats=False) == 0
    assert not d.mismatches(*case.want(), stats=False)


def test_no_reads_is_accepted_and_writes_nothing(ctx):
    case, = _pick("group_size_64")
    d = pm.DeviceBuffers(len(case.keys))
    assert d.call(ctx.lib, ctx.h, case, n_reads=0) == 0
    assert not d.mismatches(np.zeros((len(case.keys), 8), np.int64), 0, 0)


def test_misaligned_pointers_are_refused_before_anything_is_launched(ctx):
    """d_bam below 16 bytes (the staged kernel copies uint4 pieces from d_bam + (offset & ~15)), d_rec_off, d_keys and d_stats below 8,
    d_counts below 4: AMPLI_E_INVALID, and the fenced counts and stats are untouched"""
    import torch

    from tests.helpers import assert_misaligned_refused, fenced

    case, = _pick("group_size_257")
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
    bam, off, keys = up(case.buf, np.uint8), up(case.rec_off, np.int64), up(case.keys, np.int64)
    counts, stats = fenced((len(case.keys), 8), torch.int32), fenced((2,), torch.int64)
    good = (ctx.h, bam.data_ptr(), off.data_ptr(), case.n_reads, keys.data_ptr(), len(case.keys), case.mbq, case.mrq, counts[0].data_ptr(), stats[0].data_ptr())
    assert_misaligned_refused(ctx, ctx.lib.ampli_pileup_count, good, [(1, 1), (1, 4), (1, 8), (2, 4), (4, 4), (8, 2), (9, 4)], [counts, stats], b"pileup_count: bad argument")


@pytest.fixture(scope="module")
def wave_per_read_library(tmp_path_factory):
    """ampli_pileup.hip built with -DAMPLI_PILEUP_WAVE_PER_READ (+ the runtime it needs) into a temporary directory"""
    try:
        hipcc = build.hipcc_path()
    except RuntimeError:
        pytest.skip("hipcc not found: the wave-per-read form of the kernel cannot be built")
    out = str(tmp_path_factory.mktemp("wave_per_read") / "libamplisolve_pileup_wpr.so")
    cmd = [hipcc, *build.HIPCC_FLAGS, "-DAMPLI_PILEUP_WAVE_PER_READ", "-o", out, os.path.join(build.CSRC, "ampli_pileup.hip"), os.path.join(build.CSRC, "ampli_runtime.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout + r.stderr
    return out


def test_the_wave_per_read_build_passes_the_same_table(wave_per_read_library):
    """one fresh child process binds the comparison build (never a second library in this process) and reports per case; any
    mismatch and any non-zero exit fail, and nothing is started after a failure"""
    r = subprocess.run([sys.executable, "-m", "tests.pileup_model", "--child", wave_per_read_library], cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CASE ")]
    bad = [l for l in lines if not l.endswith(" ok")]
    print("\n".join(bad) or f"{len(lines)} cases ok")
    assert r.returncode == 0 and not bad, f"exit {r.returncode}\n" + "\n".join(bad) + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
    assert [l.split()[1] for l in lines] == [c.name for c in CASES]
