"""Every read walk over every case table: ampli_pileup_count, ampli_pileup_indel_count, ampli_pileup_evidence and
ampli_pileup_amplicon_count (default build) each run over the case tables of the other three and are compared, integer for integer,
with their own model on that stream.  The four kernels share csrc/ampli_bam.h; each was tested only on the table written for its own
geometry, a quarter of the streams the project owns (one_read_of_100000_bases, two_thousand_alternating_1M1I, name_lengths_1_to_255,
all_nine_operations, a_whole_group_unplaced, the adjacent and edge indels, the qualities and MAPQs at the bin edges ...).

tests/walk_cross.py builds the parameters: how a case of one table becomes the input of another kernel, the design derived from a
panel's keys for the amplicon kernel, and the conditions that keep a pair from passing vacuously (at least half the cases of every
(kernel, foreign table) pair give a non-zero model result; per table at least one derived design has reads decided by overlap AND
reads left off-target).  They are asserted on the CPU, where the parameters are built (tests/test_scale_shapes.py runs them without a
GPU), and once more here before the first pair runs.  Every table is used whole, except depth_300000_identical_starts
(walk_cross.LEFT_OUT): its 300 000 reads take the indel and evidence models 8-9 s each."""
import types

import numpy as np
import pytest

from tests import amplicon_count_model as am
from tests import evidence_model as em
from tests import indel_model as im
from tests import pileup_model as pm
from tests import walk_cross as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def params():
    share, designs = wc.non_vacuity()  # asserts its conditions
    assert set(share) == set(wc.PAIRS) and len(wc.PAIRS) == 12 and set(designs) == {"pileup", "indel", "evidence"}
    return share


def _up(a, t):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()


def run_pileup(ctx, s, want):
    buf, off = wc.staged_stream(s)
    case = types.SimpleNamespace(buf=buf, rec_off=off, keys=s.keys, n_reads=len(off), mbq=s.mbq, mrq=s.mrq)
    d = pm.DeviceBuffers(len(s.keys))  # a non-zero pre-fill between two guard rows
    rc = d.call(ctx.lib, ctx.h, case)
    return [f"ampli_pileup_count returned {rc}"] if rc else d.mismatches(*want)


def run_indel(ctx, s, want):
    out = ctx.indel_count(_up(s.buf, np.uint8), _up(s.rec_off, np.int64), _up(s.keys, np.int64), mbq=s.mbq, mrq=s.mrq)
    return im.differences(im.device_result(ctx, *out), want)


def run_evidence(ctx, s, want):
    out = ctx.read_evidence(_up(s.buf, np.uint8), _up(s.rec_off, np.int64), _up(s.keys, np.int64), mbq=s.mbq, mrq=s.mrq)
    return em.differences(em.device_result(ctx, *out), want)


def run_amplicon(ctx, s, want):
    a = am.make_amplicons(s.intervals)
    out = ctx.amplicon_count(_up(s.buf, np.uint8), _up(s.rec_off, np.int64), am._up(a.lo), am._up(a.hi), am._up(a.reach), am._up(a.amp_off), mbq=s.mbq, mrq=s.mrq,
                             min_overlap=s.min_overlap)
    return am.differences(*am.host(ctx, *out), want)


RUN = {"pileup": run_pileup, "indel": run_indel, "evidence": run_evidence, "amplicon": run_amplicon}


@pytest.mark.parametrize("kernel,table", wc.PAIRS, ids=[f"{k}_over_the_{t}_table" for k, t in wc.PAIRS])
def test_a_walk_over_a_foreign_table_equals_its_own_model(ctx, params, kernel, table):
    cases, non_zero = params[kernel, table]
    bad = {}
    for s in wc.streams(table):
        found = RUN[kernel](ctx, s, wc.model(kernel, s)[0])
        if found:
            bad[s.name] = found
    print(f"{kernel} over the {table} table: {cases} cases, {non_zero} with a non-zero model result, {len(bad)} differ")
    assert cases == len(wc.streams(table)) and not bad, bad
