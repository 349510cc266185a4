"""Read-level phasing over the C ABI: read_phase (ampli_pileup_phase) and phase_score (ampli_phase_score).

Two functions that take the Context first, not methods of it: they run under the context's stream through api.py's wrapper like every
method does, and hold its stream contract (tests/test_gpu_phase_stream_order.py).  PHASE_PARTNERS, PHASE_STATES and PHASE_OTHER come
from the headers like every other constant (api.py).
"""
from __future__ import annotations

from .api import PHASE_OTHER, PHASE_PARTNERS, PHASE_STATES, _ok, _on_stream, _ptr  # noqa: F401


@_on_stream
def read_phase(ctx, bam, rec_off, keys, mbq: int = 20, mrq: int = 20, table=None, stats=None):
    """The joint table of a batch of alignment records (ampli_pileup_phase).  bam, rec_off, keys as Context.read_evidence takes them.
    Returns (table, stats): table int32 [P, PHASE_PARTNERS, PHASE_STATES, PHASE_STATES] in the order (key i, partner k, state at key i,
    state at key i + 1 + k) -- per kept read one count for every two keys at most PHASE_PARTNERS apart in the list that it both covers;
    a state is 0 .. 3 = A C G T for a counted column, PHASE_OTHER for a low quality, a non-ACGT base, a deletion or a skip -- and stats
    int64 [3] (reads kept, reads covering at least two keys, cells incremented).  Both are ADDED TO: a given buffer accumulates, None
    starts a new one at zero; stats=False: not computed (NULL) and returned as None."""
    import torch

    assert _ok(bam, torch.uint8, (None,)) and _ok(rec_off, torch.int64, (None,)) and _ok(keys, torch.int64, (None,))
    n_reads, P = int(rec_off.numel()), int(keys.numel())
    table = ctx._out(table, torch.int32, (P, PHASE_PARTNERS, PHASE_STATES, PHASE_STATES), zero=True)
    stats = None if stats is False else ctx._out(stats, torch.int64, (3,), zero=True)
    ctx._check(ctx.lib.ampli_pileup_phase(_ptr(bam), _ptr(rec_off), n_reads, _ptr(keys), P, int(mbq), int(mrq), _ptr(table), _ptr(stats), ctx.h))
    return table, stats


@_on_stream
def phase_score(ctx, table, pair_cell, pair_nt, min_alt: int = 4, min_share: int = 10, ints=None, score=None, cls=None):
    """Are the alts of two listed keys on the same reads (ampli_phase_score)?  table: read_phase's; pair_cell: int64 [Q], each
    i * PHASE_PARTNERS + k; pair_nt: int8 [Q, 4], each ref_i, alt_i, ref_j, alt_j in 0 .. 3.  Returns (ints, score, cls): ints int64
    [Q, 6] (rr, ra, ar, aa, joint, other; the first letter is the state at key i), score float32 [Q] (the signed exact test, > 0: linked
    in cis) and cls int32 [Q] (bit 0: aa, bit 1: ar, bit 2: ra present; -1 with score 0 and counts of -1: untested).  All three are
    overwritten."""
    import torch

    P, Q = int(table.shape[0]), int(pair_cell.numel())
    assert _ok(table, torch.int32, (P, PHASE_PARTNERS, PHASE_STATES, PHASE_STATES)) and _ok(pair_cell, torch.int64, (Q,)) and _ok(pair_nt, torch.int8, (Q, 4))
    ints = ctx._out(ints, torch.int64, (Q, 6))
    score = ctx._out(score, torch.float32, (Q,))
    cls = ctx._out(cls, torch.int32, (Q,))
    ctx._check(ctx.lib.ampli_phase_score(_ptr(table), P, _ptr(pair_cell), _ptr(pair_nt), Q, int(min_alt), int(min_share), _ptr(ints), _ptr(score), _ptr(cls), ctx.h))
    return ints, score, cls
