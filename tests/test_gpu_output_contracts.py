"""Output contracts of every entry point (include/amplisolve_hip.h, "Output contracts", C1-C9): each kernel output is handed over
POISONED and FENCED (tests/helpers.fenced: 4096 guard bytes on either side, every byte 0xFF -- NaN as a float, -1 as an int32, a mask
byte with four impossible bits) and must come back written exactly where the contract says "written" (equal to the oracle, bit for bit;
dense Q within the 1e-5 of test_poisson_call_synthetic), still poisoned, bit for bit, where it says "never written", and with both
guards intact.  Counters a call must reset are prefilled with 1 << 40 (a reset that is missing then writes nothing at all, it cannot
run a list out of bounds); counters and flags a call adds to / ORs into are prefilled with a value that a plain store would lose.
Poison goes into outputs only: never into anything a kernel reads as an index, a count or a bound.

What this guards is the launch geometry: poisson_stream_kernel clears the mask in contiguous shares of the grid's waves (complete only
while grid waves x share >= mask dwords: tiles8, gy, rows per wave, the padding workgroups, the range cuts), error_reduce's clamped
lanes past the last position must never store, and so on -- code whose mistakes leave exactly the expected bytes behind whenever the
buffer held an earlier result of the same shape, as torch.empty's usually does."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests.helpers import edge_case_recs, fenced, synth_recs, synth_ref
from tests.test_gpu_compact_stream import _cohort as _dup_cohort
from tests.test_gpu_compact_stream import _summary_equal
from tests.test_gpu_parity import _t, assert_acc_equal
from tests.test_gpu_records import _pack
from tests.test_gpu_u16 import host_pack

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min
COUNTER_POISON = 1 << 40
SHARDS, STRIDE = 32, 16  # AMPLI_CALL_SHARDS, AMPLI_CALL_COUNTER_STRIDE
CALL_DT = np.dtype([("sample", "<i4"), ("record", "<i4"), ("alt", "<i4"), ("rd", "<i4"), ("q_fw", "<f8"), ("q_bw", "<f8"), ("af", "<f4"),
                    ("af_fw", "<f4"), ("af_bw", "<f4"), ("k_fw", "<i4"), ("k_bw", "<i4"), ("fw", "<i4"), ("bw", "<i4"), ("flags", "<i4")])
LOO_DT = np.dtype([("call", CALL_DT), ("thr_fw", "<f4"), ("thr_bw", "<f4"), ("code", "<i4"), ("pad", "<i4")])
assert CALL_DT.itemsize == 64 and LOO_DT.itemsize == 80


@contextlib.contextmanager
def _layout(ctx, lay):
    ctx.set_record_layout(lay)
    try:
        yield
    finally:
        ctx.set_record_layout("i32")


def _clamp16(recs):
    return np.where(recs == ABSENT, ABSENT, np.minimum(recs, 65534)).astype(np.int32)


def _popcount(mask):
    return int(sum(((mask >> a) & 1).sum() for a in range(4)))


def _bits(a):
    """the array's bytes as unsigned integers of its item size (bit-for-bit comparisons, NaN payloads included)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- call outputs: mask (C1, C2), list (C8), counters (C9) ---------------------------------------------------------------------------
class CallOut:
    """poisoned, fenced outputs of one poisson_call / loo_call: mask [T][R], call list of `capacity` entries, counters at 1 << 40"""

    def __init__(self, T, R, capacity=None, item=64):
        import torch

        self.T, self.R, self.item = T, R, item
        n = T * R
        self.mask_buf, self.mask_chk = fenced(((n + 3) // 4 * 4,), torch.uint8)  # C2: rounded up to 4 bytes, the pad bytes not checked
        self.mask = self.mask_buf[:n].view(T, R)
        self.capacity = (max(8 * n, 2048) if capacity is None else capacity) // SHARDS * SHARDS
        self.calls, self.calls_chk = fenced((self.capacity * item,), torch.uint8)
        self.n_calls, self.n_chk = fenced((SHARDS * STRIDE,), torch.int64)
        self.n_calls.fill_(COUNTER_POISON)

    def repoison(self):
        for c in (self.mask_chk, self.calls_chk, self.n_chk):
            c.repoison()
        self.n_calls.fill_(COUNTER_POISON)

    def kw(self):
        return dict(call_mask=self.mask, capacity=self.capacity, calls_buf=self.calls, n_calls=self.n_calls)

    def check(self, exp_mask, scarce=False, total=None):
        for c in (self.mask_chk, self.calls_chk, self.n_chk):
            c()
        got = self.mask.cpu().numpy()
        assert got.shape == exp_mask.shape
        wrong = got != exp_mask
        assert not wrong.any(), (f"C1: {int(wrong.sum())} mask byte(s) differ from the oracle, {int((got[wrong] == 0xFF).sum())} of them still poison; "
                                 f"first at (row, record) {tuple(np.argwhere(wrong)[0])}")
        # C9: every counter was reset by the call; C8: segment k holds min(count, per) entries, every byte behind them is untouched
        counts = self.n_calls.cpu().numpy()[::STRIDE]
        assert ((counts >= 0) & (counts < COUNTER_POISON)).all(), f"C9: counters not reset: {counts[counts >= COUNTER_POISON][:4]}"
        per = self.capacity // SHARDS
        raw = self.calls.cpu().numpy()
        dt = CALL_DT if self.item == 64 else LOO_DT
        ents = []
        for k in range(SHARDS):
            seg = raw[k * per * self.item:(k + 1) * per * self.item]
            fill = min(int(counts[k]), per)
            if scarce:
                assert counts[k] > per, f"segment {k} was meant to overflow: {counts[k]} <= {per}"
            else:
                assert counts[k] <= per, f"segment {k} overflowed ({counts[k]} > {per}): the test's capacity is too small"
            assert (seg[fill * self.item:] == 0xFF).all(), f"C8: segment {k} written beyond its count {counts[k]}"
            ents.append(np.frombuffer(seg[:fill * self.item].tobytes(), dtype=dt))
        a = np.concatenate(ents)
        c = a["call"] if self.item == 80 else a
        assert ((c["sample"] >= 0) & (c["sample"] < self.T) & (c["record"] >= 0) & (c["record"] < self.R) & (c["alt"] >= 0) & (c["alt"] < 4)).all()
        keys = (c["sample"].astype(np.int64) * self.R + c["record"]) * 4 + c["alt"]
        assert len(np.unique(keys)) == len(keys), "C8: an entry is listed twice"
        in_mask = ((exp_mask[c["sample"], c["record"]] >> c["alt"]) & 1).astype(bool)
        assert in_mask[(c["flags"] & 1) == 0].all(), "C8: an entry that is no call of the oracle (and not flagged borderline)"
        if scarce:
            assert int(counts.sum()) == total
        else:  # the counters count the entries; the entries are the oracle's calls (plus pairs flagged borderline, none on these inputs)
            assert int(counts.sum()) == len(a)
            assert int(in_mask.sum()) == _popcount(exp_mask), (int(in_mask.sum()), _popcount(exp_mask))
        return a


@functools.lru_cache(maxsize=None)
def _call_case(P, E, T):
    """tumour rows (synthetic, edge-case records mixed in as test_error_estimate_compact_state_kernel does, two planted variants, the
    last position among them), thresholds of a synthetic panel of normals, the oracle's outputs.  Counts fit uint16."""
    rng = np.random.default_rng(P * 131 + E * 17 + T)
    R = P + E
    thr = orc.error_finalize(orc.error_reduce(synth_recs(P, 24), P))["thr"]
    ref_code = synth_ref(P)
    trecs = synth_recs(R, T, tumour=True)
    if P >= 63:
        e = edge_case_recs(R, T, rng)
        pick = rng.random((T, R)) < 0.3
        trecs[pick] = e[pick]
        for p in (5, P - 1):
            ref = int(ref_code[p]) & 3
            rec = np.zeros(8, np.int32)
            rec[[ref, 4 + ref]] = 400, 380
            rec[[(ref + 1) % 4, 4 + (ref + 1) % 4]] = 30, 25
            trecs[:, p] = rec
    trecs = _clamp16(trecs)
    ext_pos = rng.integers(0, P, E).astype(np.uint32) if E else None
    exp = orc.poisson_call(trecs, P, thr, ref_code, 100, E=E, ext_pos=ext_pos)
    if P >= 63:  # calls, absent cells and low-depth cells all occur; most records are no call
        m = exp["call_mask"]
        assert m.any() and (m == 0).mean() > 0.5 and m[:, P - 1].all()
        present = trecs[:, :, 0] != ABSENT
        assert (~present).any() and (present & (trecs[:, :, :4].sum(-1) < 100)).any()
    return dict(P=P, E=E, T=T, trecs=trecs, thr=thr, ref_code=ref_code, ext_pos=ext_pos, exp=exp)


def _prefilter(ctx, case, lay="u16", tuning=None, ranges=0, async_drain=False, blocks_of=0, passes=1):
    """poisson_call in prefilter mode (poisson_stream_kernel + poisson_drain_kernel) into poisoned outputs, `passes` times into the same
    buffers, re-poisoned in between"""
    from amplisolve_amd.api import POISSON_PREFILTER

    P, E, T, exp = case["P"], case["E"], case["T"], case["exp"]
    out = CallOut(T, P + E)
    thr = case["thr"]
    if blocks_of:  # the thresholds as the all-gathered blocks of a sliced merge hold them: rate 32 L | thr 32 L | ... per slice (an input: zeros elsewhere)
        L = ctx.slice_len(P, blocks_of)
        blocks = np.zeros((blocks_of, L * 88 + 64), np.uint8)
        for k in range(blocks_of):
            part = np.zeros((8, L), np.float32)
            seg = thr.reshape(8, P)[:, k * L:(k + 1) * L]
            part[:, :seg.shape[1]] = seg
            blocks[k, L * 32:L * 64] = part.view(np.uint8).ravel()
        thr = blocks
    with _layout(ctx, lay):
        d_t, d_thr, d_ref = _pack(ctx, case["trecs"], lay), _t(thr), _t(case["ref_code"])
        d_ext = _t(case["ext_pos"]) if E else None
        try:
            if tuning:
                ctx.set_poisson_tuning(*tuning)
            if ranges:
                ctx.set_ranges(ranges)
            if async_drain:
                ctx.set_async_drain(True)
            for it in range(passes):
                if it:
                    out.repoison()
                ctx.poisson_call(d_t, P, d_thr, d_ref, 100, mode=POISSON_PREFILTER, E=E, ext_pos=d_ext, blocks_of=blocks_of, **out.kw())
                if async_drain:
                    ctx.wait_calls()
                if ranges:
                    ctx.ranges_join()  # the section must be closed before the caller touches the ranges' outputs again (re-poisoning included)
                ctx.sync()
                assert ctx.flags() == 0
                out.check(exp["call_mask"])
        finally:
            ctx.set_async_drain(False)
            ctx.set_ranges(1)
            ctx.set_poisson_tuning()


@pytest.mark.parametrize("P,E,T,lay", [(1, 0, 1, "u16"), (63, 0, 3, "u16"), (65, 3, 5, "u16"), (257, 0, 7, "u16"), (1000, 37, 29, "i32"),
                                       (1000, 37, 29, "u16"), (1000, 37, 29, "u24"), (4099, 0, 13, "u16")])
def test_prefilter_mask_list_and_counters(ctx, P, E, T, lay):
    """a. C1 / C2 / C8 / C9 through poisson_stream_kernel + poisson_drain_kernel at the default launch shape ((4099, 0, 13): R % 4 != 0)"""
    _prefilter(ctx, _call_case(P, E, T), lay)


@pytest.mark.parametrize("rows,blocks", [(0, 0), (1, 1), (3, 32), (24, 7), (1000, 1)])
@pytest.mark.parametrize("P,E,T", [(257, 0, 7), (1000, 37, 29)])
def test_prefilter_under_every_launch_shape(ctx, P, E, T, rows, blocks):
    """a. the clear's shares follow rows_per_wave and the grid: complete and in bounds for each of them"""
    _prefilter(ctx, _call_case(P, E, T), tuning=(rows, blocks))


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("P,T", [(520, 3), (5000, 6)])
def test_prefilter_over_position_ranges(ctx, P, T, n):
    """a. every range clears its own columns of every row and resets its own shards' counters; two passes into the same buffers,
    mask, list and counters re-poisoned in between (behind a join: the caller may not write the outputs of an open section)"""
    _prefilter(ctx, _call_case(P, 0, T), ranges=n, passes=2)


def test_prefilter_with_the_drain_on_its_side_stream(ctx):
    """a. set_async_drain(True) + wait_calls()"""
    _prefilter(ctx, _call_case(1000, 37, 29), async_drain=True)


def test_prefilter_with_thresholds_from_gathered_blocks(ctx):
    """a. ampli_poisson_call_blocks, blocks_of = 3"""
    _prefilter(ctx, _call_case(1000, 37, 29), blocks_of=3)


@pytest.mark.parametrize("route", ["full_q", "full_q_af", "prefilter_af"])
@pytest.mark.parametrize("P,E,T,lay", [(255, 0, 3, "i32"), (257, 5, 5, "u16"), (1000, 37, 6, "u24")])
def test_all_scores_mode_writes_every_dense_element(ctx, P, E, T, lay, route):
    """b. C1 / C3 / C8 / C9 through poisson_full_kernel (dense q only) and poisson_call_kernel (with dense af, both modes): mask, q and
    af poisoned, every element written"""
    import torch

    from amplisolve_amd.api import POISSON_FULL, POISSON_PREFILTER

    case = _call_case(P, E, T)
    exp, R = case["exp"], P + E
    out = CallOut(T, R)
    q, q_chk = fenced((T, R, 4, 2), torch.float64)
    af, af_chk = fenced((T, R, 4, 3), torch.float32)
    with _layout(ctx, lay):
        ctx.poisson_call(_pack(ctx, case["trecs"], lay), P, _t(case["thr"]), _t(case["ref_code"]), 100,
                         mode=POISSON_PREFILTER if route == "prefilter_af" else POISSON_FULL, E=E, ext_pos=_t(case["ext_pos"]) if E else None,
                         q=None if route == "prefilter_af" else q, af=None if route == "full_q" else af, **out.kw())
        ctx.sync()
        assert ctx.flags() == 0
    out.check(exp["call_mask"])
    q_chk()
    af_chk()
    if route != "prefilter_af":
        got, want = q.cpu().numpy(), exp["q"]
        assert not np.isnan(got).any(), f"C3: {int(np.isnan(got).sum())} element(s) of q never written"
        assert np.array_equal(got == -1, want == -1)
        assert np.max(np.abs(got - want)) <= 1e-5
    else:
        assert bool((_bits(q.cpu().numpy()) == np.uint64(0xFFFFFFFFFFFFFFFF)).all())  # not an output of this call
    if route != "full_q":
        assert np.array_equal(_bits(af.cpu().numpy()), _bits(exp["af"])), "C3: af"
    else:
        assert bool((_bits(af.cpu().numpy()) == np.uint32(0xFFFFFFFF)).all())


def test_call_list_segments_that_overflow_stay_inside_their_bounds(ctx):
    """c. scarce capacity: the input of test_prefilter_queue_overflow_is_flagged_and_recoverable at P = 2048, T = 4 (24 576 calls; the
    default queue holds them) with capacity 32 * 64, so that every segment overflows: the counters still count every call, the first 64
    entries of each segment are calls, distinct over the list, nothing is written behind a segment, and the mask is exact"""
    from amplisolve_amd.api import POISSON_PREFILTER

    P, T = 2048, 4
    rng = np.random.default_rng(17)
    trecs = np.zeros((T, P, 8), np.int32)
    trecs[:, :, 0] = 900; trecs[:, :, 4] = 850                      # reference A
    trecs[:, :, 1] = rng.integers(20, 60, (T, P)); trecs[:, :, 5] = rng.integers(20, 60, (T, P))
    trecs[:, :, 2] = rng.integers(15, 50, (T, P)); trecs[:, :, 6] = rng.integers(15, 50, (T, P))
    trecs[:, :, 3] = rng.integers(10, 40, (T, P)); trecs[:, :, 7] = rng.integers(10, 40, (T, P))
    thr = np.full((2, 4, P), 0.002, np.float32)
    ref_code = np.zeros(P, np.uint8)
    exp = orc.poisson_call(trecs, P, thr, ref_code, 100, dense=False)
    assert _popcount(exp["call_mask"]) == 3 * T * P
    out = CallOut(T, P, capacity=SHARDS * 64)
    ctx.poisson_call(_t(trecs), P, _t(thr), _t(ref_code), 100, mode=POISSON_PREFILTER, **out.kw())
    ctx.sync()
    assert ctx.flags() == 0  # the QUEUE did not overflow; the list's segments did, which their counters say
    a = out.check(exp["call_mask"], scarce=True, total=3 * T * P)
    assert len(a) == SHARDS * 64


# ---- error table (C3, C5) ------------------------------------------------------------------------------------------------------------
def _poisoned_table(P, flags0=0):
    import torch

    from amplisolve_amd.api import ErrorTable

    v, checks = {}, []
    for name, shape, dt in (("rate", (2, 4, P), torch.float32), ("code", (4, P), torch.uint8), ("thr", (2, 4, P), torch.float32),
                            ("germ_val", (4, P), torch.float32), ("germ_present", (4, P), torch.uint8), ("flags", (1,), torch.int32)):
        v[name], c = fenced(shape, dt)
        checks.append(c)
    v["flags"].fill_(flags0)  # C5: a flag word is OR-ed into, so it starts from a value of the caller's (never from poison)
    tab = ErrorTable(**v)
    tab.checks = checks
    return tab


def _repoison_table(tab, flags0=0):
    for c in tab.checks:
        c.repoison()
    tab.flags.fill_(flags0)


def _check_table(tab, ref, flags=0):
    for c in tab.checks:
        c()
    got = {k: getattr(tab, k).cpu().numpy() for k in ("rate", "code", "thr", "germ_val", "germ_present")}
    for k in ("code", "germ_present"):
        assert np.array_equal(got[k], ref[k]), f"C3: {k}: {int((got[k] != ref[k]).sum())} differ, {int((got[k] == 0xFF).sum())} still poison"
    for k in ("rate", "thr"):
        bad = _bits(got[k]) != _bits(ref[k])
        assert not bad.any(), f"C3: {k}: {int(bad.sum())} differ, {int((_bits(got[k]) == 0xFFFFFFFF).sum())} still poison"
    m = ref["germ_present"] > 0
    assert np.array_equal(got["germ_val"][m].astype(np.float64), ref["germ_val"][m])
    assert (_bits(got["germ_val"])[~m] != 0xFFFFFFFF).all(), "C3: germ_val is written where germ_present is 0 as well"
    assert int(tab.flags.item()) == flags


@functools.lru_cache(maxsize=None)
def _cohort(P, S, extras=False):
    """normals with edge-case records mixed in (uint16 range), the oracle's accumulator table and error table"""
    rng = np.random.default_rng(P * 1000 + S + (7 if extras else 0))
    if extras:
        recs, E, dup_off = _dup_cohort(P, S, rng)
    else:
        recs, E, dup_off = synth_recs(P, S), 0, None
        if P >= 63:
            e = edge_case_recs(P, S, rng)
            pick = rng.random((S, P)) < 0.3
            recs[pick] = e[pick]
        recs = _clamp16(recs)
    acc = orc.error_reduce(recs, P, 0.002, 100, E=E, dup_off=dup_off)
    assert acc["order_sensitive"] == 0
    return recs, E, dup_off, acc, orc.error_finalize(acc)


TABLE_ROUTES = ["auto", "splits2", "splits3", "groups2", "groups4", "general", "u16", "u24", "finalize", "records", "merged"]


def _table_route(ctx, route, recs, P, E, dup_off, tab):
    """one way to an error table, written into `tab`"""
    import torch

    S = recs.shape[0]
    lay = route[:3] if route[:3] in ("u16", "u24") else "i32"
    with _layout(ctx, lay):
        d = _pack(ctx, recs, lay)
        d_dup = _t(dup_off) if E else None
        try:
            if route in ("auto", "splits2", "splits3", "groups2", "groups4", "general"):
                ctx.set_tuning(int(route[-1]) if route.startswith("splits") else 0, general=route == "general",
                               groups=int(route[-1]) if route.startswith("groups") else 0)
                ctx.error_estimate(d, P, 0.002, 100, E=E, dup_off=d_dup, out=tab)
            elif route in ("u16", "u24", "u16_ranges2", "u16_ranges3"):
                ctx.set_tuning(1, groups=1)  # one sample split, one lane group: the shape the compact kernel takes
                if "ranges" in route:
                    ctx.set_ranges(int(route[-1]))
                ctx.error_estimate(d, P, 0.002, 100, E=E, dup_off=d_dup, out=tab)
                if "ranges" in route:
                    ctx.ranges_join()
                else:
                    assert ctx.last_reduce_kernel() == f"error_reduce_{lay}_kernel"
            elif route == "finalize":
                ctx.error_finalize(ctx.error_reduce(d, P, 0.002, 100, E=E, dup_off=d_dup), 0.002, 100, out=tab)
            elif route == "records":
                rec = ctx.records(d, lay, S, E=E, dup_off=d_dup)
                ctx.error_reduce_records(rec, P, ctx.new_acc(P), 0.002, 100, finalize=True, out=tab)
            elif route == "merged":
                assert E == 0
                cuts = [0, S] if S == 1 else [0, S // 2, S]
                _, gm_off, gm_bytes = ctx.regions(P)
                packed, regions = [], []
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    acc = ctx.new_acc(P)
                    pk = torch.empty(21 * P, dtype=torch.float64, device="cuda")
                    ctx.error_reduce_packed(d[lo:hi].contiguous(), P, acc, pk, first_sample=lo)
                    packed.append(pk)
                    regions.append(acc.buf[gm_off: gm_off + gm_bytes].clone())
                ctx.error_finalize_merged(P, torch.stack(packed).sum(0), torch.cat(regions), len(cuts) - 1, 0.002, 100, out=tab)
            else:
                raise AssertionError(route)
        finally:
            ctx.set_ranges(1)
            ctx.set_tuning(0)
        ctx.sync()
        assert ctx.flags() == 0


@pytest.mark.parametrize("route", TABLE_ROUTES)
@pytest.mark.parametrize("S", [1, 5, 37])
@pytest.mark.parametrize("P", [1, 63, 65, 130, 1000])
def test_error_table_is_fully_written(ctx, P, S, route):
    """d. C3 / C5: every plane of the error table poisoned, flags 0; rate, code, thr, germ_val and germ_present are all written and the
    oracle's -- through the fused epilogue (automatic, 2 and 3 sample splits = merge + finalize kernels, 2 and 4 lane groups, the literal
    kernel, the two compact kernels), error_finalize, error_reduce_records(finalize=True) and error_finalize_merged"""
    recs, E, dup_off, _, fin = _cohort(P, S)
    tab = _poisoned_table(P)
    _table_route(ctx, route, recs, P, E, dup_off, tab)
    _check_table(tab, fin)


@pytest.mark.parametrize("P,S", [(65, 5), (130, 37), (1000, 37)])
def test_error_table_from_compact_and_general_tiles(ctx, P, S):
    """d. uint16 records with positions listed more than once: the compact kernel and the general kernel (over the list of tiles that
    hold such a position) each write their own tiles of ONE poisoned table"""
    recs, E, dup_off, _, fin = _cohort(P, S, extras=True)
    assert E > 0
    tab = _poisoned_table(P)
    _table_route(ctx, "u16", recs, P, E, dup_off, tab)
    _check_table(tab, fin)


@pytest.mark.parametrize("n", [2, 3])
def test_error_table_over_position_ranges(ctx, n):
    """d. uint16 under set_ranges(n) at P = 520: every range writes its own columns of every plane"""
    recs, E, dup_off, _, fin = _cohort(520, 9)
    tab = _poisoned_table(520)
    _table_route(ctx, f"u16_ranges{n}", recs, 520, E, dup_off, tab)
    _check_table(tab, fin)


@pytest.mark.parametrize("route", ["auto", "u16", "finalize", "merged"])
def test_flag_words_are_ored_into(ctx, route):
    """d. C5: a bit the caller's flag word already holds survives the call (inside the exactness envelope the call adds none)"""
    recs, E, dup_off, _, fin = _cohort(130, 5)
    tab = _poisoned_table(130, flags0=0x100)
    _table_route(ctx, route, recs, 130, E, dup_off, tab)
    _check_table(tab, fin, flags=0x100)


# ---- accumulator table (C7) ----------------------------------------------------------------------------------------------------------
def _poisoned_acc(ctx, P):
    import torch

    from amplisolve_amd.api import Acc

    buf, chk = fenced((int(ctx.lib.ampli_acc_bytes(P)),), torch.uint8, 0x5A)
    acc = Acc(ctx, P, buf=buf)
    acc.chk = chk
    return acc


def _check_acc_padding(acc):
    """C7: every byte between the planes and behind the last one, up to ampli_acc_bytes(P), still reads 0x5A; the guards too"""
    acc.chk()
    raw = acc.buf.cpu().numpy()
    covered = np.zeros(len(raw), bool)
    base = acc.buf.data_ptr()
    for name, plane in acc.planes().items():
        off, n = plane.data_ptr() - base, plane.numel() * plane.element_size()
        assert 0 <= off and off + n <= len(raw) and not covered[off:off + n].any(), name
        covered[off:off + n] = True
    assert (~covered).any(), "the shape was meant to leave padding"
    bad = ~covered & (raw != 0x5A)
    assert not bad.any(), f"C7: {int(bad.sum())} padding byte(s) written, the first at offset {int(np.argmax(bad))} of {len(raw)}"


@pytest.mark.parametrize("route", ["fast", "literal", "groups2", "groups4", "splits2", "splits3", "compact_u16", "compact_u24", "records_extras"])
@pytest.mark.parametrize("P", [1, 65, 1000])
def test_accumulator_table_padding_is_never_written(ctx, P, route):
    """e. the whole table buffer poisoned with 0x5A and fenced: the eight planes are the oracle's (assert_acc_equal; _summary_equal for
    a table the compact kernel writes as streaming state), the padding is untouched"""
    S = 37
    recs, E, dup_off, ref, _ = _cohort(P, S, extras=route == "records_extras")
    acc = _poisoned_acc(ctx, P)
    lay = route[-3:] if route.startswith("compact") else "i32"
    with _layout(ctx, lay):
        d = _pack(ctx, recs, lay)
        try:
            if route.startswith("compact"):  # the first chunk of a streamed cohort through the compact kernel
                ctx.set_tuning(1, groups=1)
                ctx.error_reduce_records(ctx.records(d, lay, S), P, acc, 0.002, 100, accumulate=False, summary=True)
                assert ctx.last_reduce_kernel() == f"error_reduce_{lay}_kernel"
            elif route == "records_extras":  # the first chunk, positions listed more than once
                assert E > 0
                ctx.error_reduce_records(ctx.records(d, lay, S, E=E, dup_off=_t(dup_off)), P, acc, 0.002, 100, accumulate=False)
            else:
                ctx.set_tuning(int(route[-1]) if route.startswith("splits") else 0, general=route == "literal",
                               groups=int(route[-1]) if route.startswith("groups") else 0)
                ctx.error_reduce(d, P, 0.002, 100, acc=acc)
        finally:
            ctx.set_tuning(0)
        ctx.sync()
        assert ctx.flags() == 0
    if route.startswith("compact"):
        _summary_equal(acc, ref)
    else:
        assert_acc_equal(acc, ref)
    _check_acc_padding(acc)


# ---- sliced exchange (C6) ------------------------------------------------------------------------------------------------------------
def _pack_slices(acc, P, n, L, slim, G=1, g=0):
    """numpy packer of a shard's (oracle) accumulator table in the documented layout of the sliced exchange: sums f64 [n][G][planes][L]
    -- wide: snt 8 | srd 8 | cnt 4 | nrec 1; slim: snt 8 | srd fw + bw * 2^26 per nucleotide | cnt0 + cnt1 * 2^17 + cnt2 * 2^34 |
    cnt3 + nrec * 2^17 -- and gm f32 [n][G][8][L]: first AF (-1: no qualifying record) | max of the later ones (-inf: none).  Entries
    of positions >= P and of the other batches of the group hold the poison (all bits set)."""
    pl = 14 if slim else 21
    sums = np.full((n, G, pl, L), -1, np.int64).view(np.float64)
    gm = np.full((n, G, 8, L), -1, np.int32).view(np.float32)
    for k in range(n):
        lo, hi = k * L, min((k + 1) * L, P)
        if hi <= lo:
            continue
        w, sl = hi - lo, slice(lo, hi)
        srd = acc["srd"].reshape(8, P)[:, sl].astype(np.float64)
        cnt, nrec = acc["cnt"][:, sl].astype(np.float64), acc["nrec"][sl].astype(np.float64)
        sums[k, g, 0:8, :w] = acc["snt"].reshape(8, P)[:, sl]
        if slim:
            sums[k, g, 8:12, :w] = srd[0:4] + srd[4:8] * 2.0 ** 26
            sums[k, g, 12, :w] = cnt[0] + cnt[1] * 2.0 ** 17 + cnt[2] * 2.0 ** 34
            sums[k, g, 13, :w] = cnt[3] + nrec * 2.0 ** 17
        else:
            sums[k, g, 8:16, :w], sums[k, g, 16:20, :w], sums[k, g, 20, :w] = srd, cnt, nrec
        gn = acc["gm_n"][:, sl]
        gm[k, g, 0:4, :w] = np.where(gn > 0, acc["gm_first_af"][:, sl], np.float32(-1))
        gm[k, g, 4:8, :w] = np.where(gn > 1, acc["gm_rest"][:, sl], np.float32(-np.inf))
    return sums, gm


@functools.lru_cache(maxsize=None)
def _sharded(P, n):
    from amplisolve_amd.dist import shard_range

    S = 24
    recs, _, _, _, fin = _cohort(P, S)
    cuts = [shard_range(S, r, n) for r in range(n)]
    return recs, cuts, [orc.error_reduce(recs[a:b], P, 0.002, 100, first_sample=a) for a, b in cuts], fin


def _sliced_case(ctx, P, n, slim, compact, via_acc=False, G=1, g=0):
    import torch

    from amplisolve_amd.dist import slice_geometry, slice_planes

    recs, cuts, shard_acc, fin = _sharded(P, n)
    L, _, _, bb = slice_geometry(P, n, slim)
    pl = slice_planes(slim)
    poison64, poison32 = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint32(0xFFFFFFFF)
    with _layout(ctx, "u16"):
        ctx.set_slice_format(slim)
        ctx.set_slice_group(G, g)
        ctx.set_tuning(1, groups=1)
        ctx.set_reduce_compact(compact)
        try:
            sums, gms = [], []
            for (a, b), oacc in zip(cuts, shard_acc):
                s, s_chk = fenced((n, G, pl, L), torch.float64)
                m, m_chk = fenced((n, G, 8, L), torch.float32)
                d = _pack(ctx, recs[a:b], "u16")
                if via_acc:
                    acc = ctx.error_reduce(d, P, 0.002, 100, first_sample=a)
                    ctx._check(ctx.lib.ampli_acc_to_slices(ctx.h, C.byref(acc.struct), n, s.data_ptr(), m.data_ptr()))
                else:
                    ctx.error_reduce_sliced(d, P, n, s, m, 0.002, 100, first_sample=a)
                    assert ctx.last_reduce_kernel() == ("error_reduce_u16_kernel" if compact else "error_reduce_kernel")
                ctx.sync()
                s_chk()
                m_chk()
                # C6: entries of positions < P are the packed oracle table, entries of positions >= P are still poison, bit for bit
                es, em = _pack_slices(oacc, P, n, L, slim, G, g)
                gs, gg = s.cpu().numpy(), m.cpu().numpy()
                bad = _bits(gs) != _bits(es)
                assert not bad.any(), (f"C6 sums: {int(bad.sum())} differ; written where poison was due: {int((bad & (_bits(es) == poison64)).sum())}, "
                                       f"still poison where a value was due: {int((bad & (_bits(gs) == poison64)).sum())}; first {tuple(np.argwhere(bad)[0])}")
                bad = _bits(gg) != _bits(em)
                assert not bad.any(), (f"C6 gm: {int(bad.sum())} differ; written where poison was due: {int((bad & (_bits(em) == poison32)).sum())}, "
                                       f"still poison where a value was due: {int((bad & (_bits(gg) == poison32)).sum())}; first {tuple(np.argwhere(bad)[0])}")
                sums.append(s)
                gms.append(m)
            assert ctx.flags() == 0
            # the buffers, poison padding included, through finalize_slice: reduce-scatter = rank k keeps chunk k of the sum, all-to-all = chunk j
            # of the received pairs is rank j's
            total = torch.stack(sums).sum(0).view(n, G * pl * L)
            blocks, b_chk = fenced((n, G, bb), torch.uint8)
            blocks[:, :, L * 88:L * 88 + 4] = 0  # C5: the flag word of every block is OR-ed into
            for k in range(n):
                recv = torch.stack([m.view(n, G * 8 * L)[k] for m in gms]).contiguous()
                ctx.error_finalize_slice(P, n, k, total[k].contiguous(), recv, blocks[k], 0.002, 100)
            ctx.sync()
            b_chk()
            got = blocks.cpu().numpy()
            for k in range(n):
                for gi in range(G):
                    blk = got[k, gi]
                    assert (blk[L * 88:L * 88 + 4] == 0).all() and (blk[L * 88 + 4:] == 0xFF).all(), "C5 / C6: the block's tail"
                    w = max(0, min((k + 1) * L, P) - k * L) if gi == g else 0
                    sl = slice(k * L, k * L + w)
                    for name, at, rows, dt in (("rate", 0, 8, np.float32), ("thr", 32, 8, np.float32), ("germ_val", 64, 4, np.float32),
                                               ("code", 80, 4, np.uint8), ("germ_present", 84, 4, np.uint8)):
                        plane = blk[L * at:L * at + rows * L * np.dtype(dt).itemsize].view(dt).reshape(rows, L)
                        assert (_bits(plane[:, w:]) == _bits(np.full(1, -1, np.int32).view(dt) if dt == np.float32 else np.full(1, 0xFF, dt))[0]).all(), \
                            f"C6: block {k} batch {gi}: {name} written at a position >= P"
                        want = fin[name].reshape(rows, P)[:, sl]
                        if name == "germ_val":
                            pres = fin["germ_present"][:, sl] > 0
                            assert np.array_equal(plane[:, :w][pres].astype(np.float64), want[pres])
                            assert (_bits(plane[:, :w])[~pres] != poison32).all()
                        else:
                            assert np.array_equal(_bits(plane[:, :w]), _bits(want.astype(dt))), f"block {k}: {name}"
            tab = _poisoned_table(P)
            ctx.error_table_unslice(P, n, blocks, out=tab)
            ctx.sync()
            _check_table(tab, fin)
        finally:
            ctx.set_reduce_compact(True)
            ctx.set_tuning(0)
            ctx.set_slice_group(1, 0)
            ctx.set_slice_format(False)


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("slim", [False, True])
@pytest.mark.parametrize("P", [65, 1000, 4097])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_sliced_exchange_never_writes_positions_beyond_the_panel(ctx, n, P, slim, compact):
    """f. C6 through error_reduce_sliced (compact and general kernel, wide and slim sums), error_finalize_slice and
    error_table_unslice: sums, pairs and blocks poisoned"""
    _sliced_case(ctx, P, n, slim, compact)


@pytest.mark.parametrize("slim", [False, True])
def test_sliced_exchange_from_a_table(ctx, slim):
    """f. the same through ampli_acc_to_slices"""
    _sliced_case(ctx, 1000, 3, slim, compact=False, via_acc=True)


def test_sliced_exchange_addresses_one_batch_of_a_group(ctx):
    """f. set_slice_group(2, 1): batch 0 of every buffer stays poison"""
    _sliced_case(ctx, 1000, 3, False, compact=True, G=2, g=1)


# ---- records_pack16 / 24 (C3, C5) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", ["u16", "u24"])
@pytest.mark.parametrize("n_records", [1, 255, 257, 1000])
def test_records_pack_writes_its_records_and_ors_the_overflow_word(ctx, n_records, lay):
    """g. fenced output, the overflow word prefilled 2: it stays 2 without an overflow and becomes 3 with one"""
    import torch

    rng = np.random.default_rng(n_records)
    recs = _clamp16(edge_case_recs(n_records, 1, rng))
    fn, rb, top = (ctx.lib.ampli_records_pack16, 16, 65534) if lay == "u16" else (ctx.lib.ampli_records_pack24, 24, (1 << 24) - 2)
    recs[0, n_records - 1] = [top, 0, 1, 2, 3, top, 5, 6]  # the largest count that fits, in the last record
    for overflow in (False, True):
        if overflow:
            recs[0, n_records // 2] = [10, 1, 2, 3, 4, 5, top + 1, 7]
        d = _t(recs)
        out, o_chk = fenced((n_records * rb,), torch.uint8)
        over, v_chk = fenced((1,), torch.int32)
        over.fill_(2)
        ctx._check(fn(ctx.h, d.data_ptr(), n_records, out.data_ptr(), over.data_ptr()))
        ctx.sync()
        o_chk()
        v_chk()
        assert int(over.item()) == (3 if overflow else 2)
        if not overflow:
            assert np.array_equal(out.cpu().numpy().reshape(1, n_records, rb), host_pack(recs, lay))


# ---- leave-one-out (C1, C3, C4, C5, C8, C9) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(65, 2), (300, 7)])
def test_leave_one_out_outputs(ctx, P, S):
    """h. mask poisoned (cleared by the call), callable_pos / callable_sample prefilled 7 (added to), flags 0 (stays 0), the dense S-1
    thresholds poisoned (fully written), the call list through loo_drain_kernel"""
    import torch

    from amplisolve_amd.api import POISSON_PREFILTER
    from tests.loo_model import loo_model
    from tests.test_gpu_loo import _cohort as loo_cohort

    recs, E, dup_off, ext_pos, rd, ref_code = loo_cohort(P, S, seed=P + S, extras=True)
    assert E > 0 and rd is None
    exp = loo_model(recs, P, ref_code, 0.002, 100, 100, E=E, dup_off=dup_off, ext_pos=ext_pos)
    assert exp["order_sensitive"] == 0
    rec = ctx.records(_t(recs), "i32", S, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos))
    acc = ctx.new_acc(P)
    ctx.error_reduce_records(rec, P, acc, 0.002, 100, summary=True)
    out = CallOut(S, P + E, item=80)
    cpos, cpos_chk = fenced((P,), torch.int32)
    csam, csam_chk = fenced((S,), torch.int32)
    flags, f_chk = fenced((1,), torch.int32)
    thr, t_chk = fenced((S, 2, 4, P), torch.float32)
    cpos.fill_(7)
    csam.fill_(7)
    flags.fill_(0)
    ctx.loo_call(rec, P, acc, _t(ref_code), 0.002, 100, 100, mode=POISSON_PREFILTER, callable_pos=cpos, callable_sample=csam, flags=flags,
                 thr_loo=thr, **out.kw())
    ctx.sync()
    assert ctx.flags() == 0
    for c in (cpos_chk, csam_chk, f_chk, t_chk):
        c()
    out.check(exp["call_mask"])
    assert np.array_equal(cpos.cpu().numpy(), 7 + exp["callable_pos"]) and np.array_equal(csam.cpu().numpy(), 7 + exp["callable_sample"])
    assert int(flags.item()) == 0
    assert np.array_equal(_bits(thr.cpu().numpy()), _bits(exp["thr_loo"])), "C3: thr_loo"
    if S > 2:
        assert exp["call_mask"].any()


# ---- detection limits and power (C3, C4) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("T,P", [(3, 65), (2, 127)])
def test_detection_limit_outputs(ctx, T, P, extras):
    """i. raw ampli_limit_records: min_reads and status poisoned (every cell written, the model's once the open cells are settled),
    counts prefilled 5 (added to)"""
    import torch

    from amplisolve_amd.api import POISSON_PREFILTER
    from tests import limit_model as lm
    from tests.test_gpu_limits import LEVELS, _compare, _inputs

    levels = LEVELS[:3]
    recs, E, ext_pos, rd, ref_code, thr = _inputs("u16", T, P, seed=P + T, extras=extras, own_rd=False, deep=False)
    R = P + E
    assert (E > 0) == extras and (extras or R % 64 in (1, 63))
    exp = lm.limit_model(recs, P, thr, ref_code, 100, E=E, ext_pos=ext_pos, levels=levels, from_one=False)
    d_thr, d_ref = _t(thr), _t(ref_code)
    lv = torch.tensor(levels, dtype=torch.float32, device="cuda")
    mr, mr_chk = fenced((T, R, 4, 2), torch.int32)
    st, st_chk = fenced((T, R, 4), torch.uint8)
    cn, cn_chk = fenced((T, lm.COUNTERS + len(levels)), torch.int64)
    cn.fill_(5)
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", T, E=E, ext_pos=_t(ext_pos) if E else None)
    ctx._check(ctx.lib.ampli_limit_records(ctx.h, C.byref(rec), P, d_thr.data_ptr(), d_ref.data_ptr(), 100, lv.data_ptr(), len(levels),
                                           mr.data_ptr(), st.data_ptr(), cn.data_ptr()))
    call = ctx.poisson_call_records(rec, P, d_thr, d_ref, 100, mode=POISSON_PREFILTER)
    ctx.sync()
    for c in (mr_chk, st_chk, cn_chk):
        c()
    got = dict(min_reads=mr.cpu().numpy().copy(), status=st.cpu().numpy().copy(), counts=cn.cpu().numpy() - 5, mask=call["call_mask"].cpu().numpy())
    assert (got["status"] != 0xFF).all() and (got["min_reads"] != -1).all(), "C3: a cell was never written"
    _compare(got, exp, recs, P, E, ext_pos, None, ref_code, thr, 100, levels)


@pytest.mark.parametrize("extras", [False, True])
@pytest.mark.parametrize("T,P", [(3, 65), (2, 127)])
def test_detection_power_outputs(ctx, T, P, extras):
    """i. raw ampli_power_records: power and lod poisoned (0 in every cell that is not OK, test_gpu_power's bounds against the host's run
    of the same code and against the model in the others), counts prefilled 5 (added to)"""
    import torch

    from tests import power_model as pm
    from tests.test_gpu_limits import LEVELS
    from tests.test_gpu_power import BAND, LOD_TOL, TAIL_TOL, _cohort as power_cohort
    from tests.test_gpu_power import _host, _place

    levels, conf = LEVELS[:3], 0.95
    c32 = float(np.float32(conf))
    recs, E, status0, min_reads0 = power_cohort("u16", T, P, extras, False)
    status, min_reads, kind = _place(recs, status0, min_reads0, levels, seed=1000 * P + T)
    R = P + E
    lv = torch.tensor(levels, dtype=torch.float32, device="cuda")
    pw, pw_chk = fenced((T, R, 4, len(levels)), torch.float32)
    lod, lod_chk = fenced((T, R, 4), torch.float32)
    cn, cn_chk = fenced((T, 1 + len(levels)), torch.int64)
    cn.fill_(5)
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", T, E=E)
    d_mr, d_st = _t(min_reads), _t(status)
    ctx._check(ctx.lib.ampli_power_records(ctx.h, C.byref(rec), P, d_mr.data_ptr(), d_st.data_ptr(), lv.data_ptr(), len(levels),
                                           conf, pw.data_ptr(), lod.data_ptr(), cn.data_ptr()))
    ctx.sync()
    for c in (pw_chk, lod_chk, cn_chk):
        c()
    gp, gl, gc = pw.cpu().numpy(), lod.cpu().numpy(), cn.cpu().numpy() - 5
    FW, BW = recs[:, :, :4].astype(np.int64).sum(-1), recs[:, :, 4:].astype(np.int64).sum(-1)
    ok = pm.is_ok(status, min_reads, FW, BW)
    assert np.array_equal(ok, kind >= 0) and ok.sum() > 0 and (~ok).sum() > 0
    assert not np.isnan(gp).any() and not np.isnan(gl).any(), "C3: a cell was never written"
    assert (gp[~ok] == 0).all() and (gl[~ok] == 0).all()
    cells = [tuple(x) for x in np.argwhere(ok)]
    args = {cell: (int(FW[cell[:2]]), int(min_reads[cell][0]), int(BW[cell[:2]]), int(min_reads[cell][1])) for cell in cells}
    model_p = {cell: pm.powers(*args[cell], levels) for cell in cells}
    rng = np.random.default_rng(P + 31 * T)
    sample = set(cells[i] for i in rng.permutation(len(cells))[:200])
    for cell in cells:
        hp, hl = _host(*args[cell], levels, conf)
        assert float(np.abs(gp[cell] - np.array(hp)).max()) <= TAIL_TOL and 0 < gl[cell] <= 1 and abs(float(gl[cell]) / hl - 1) <= LOD_TOL
        assert float(np.abs(gp[cell] - np.array(model_p[cell])).max()) <= TAIL_TOL
        if cell in sample:
            assert abs(float(gl[cell]) / pm.lod(*args[cell], c32) - 1) <= LOD_TOL
    assert np.array_equal(gc[:, 0], ok.sum(axis=(1, 2)))
    mp_ = np.zeros(status.shape + (len(levels),))
    for cell in cells:
        mp_[cell] = model_p[cell]
    okx = ok[..., None]
    lo, hi = (okx & (mp_ >= c32 + BAND)).sum(axis=(1, 2)), (okx & (mp_ >= c32 - BAND)).sum(axis=(1, 2))
    assert (lo <= gc[:, 1:]).all() and (gc[:, 1:] <= hi).all(), (lo, gc, hi)


# ---- hipGraph replay (last in the file) ----------------------------------------------------------------------------------------------
def test_hipgraph_replay_rewrites_every_output():
    """j. the capture sequence of test_hipgraph_capture_replays_the_same_pass at P = 2000, S = 8, T = 5: mask, error table and counters
    (at 1 << 40) are re-poisoned before each of two replays; both give the eager result, call for call, and raise no flag.  (This case
    found the queue's shard counters not zero at a replay's stream kernel while a memset node reset them: a call listed twice,
    AMPLI_FLAG_QUEUE_OVERFLOW with six items queued.  queue_prepare resets them with a kernel node since.)"""
    import torch

    from amplisolve_amd import Context
    from amplisolve_amd.api import POISSON_PREFILTER

    g_ctx = Context(0, own_stream=True)
    try:
        P, S, T = 2000, 8, 5
        normals = g_ctx.synth_fill(P, S)
        tum = g_ctx.synth_fill(P, T, tumour=True)
        refc = g_ctx.synth_ref(P)
        g_ctx.sync()
        fin = _poisoned_table(P)
        out = CallOut(T, P, capacity=1 << 16)
        torch.cuda.synchronize()

        def one_pass():
            g_ctx.error_estimate(normals, P, out=fin)
            g_ctx.poisson_call(tum, P, fin.thr, refc, 100, mode=POISSON_PREFILTER, **out.kw())

        one_pass()
        g_ctx.sync()
        want = orc.error_finalize(orc.error_reduce(normals.cpu().numpy(), P))
        exp = orc.poisson_call(tum.cpu().numpy(), P, want["thr"], refc.cpu().numpy(), 100, dense=False)
        _check_table(fin, want)
        eager_calls = out.check(exp["call_mask"])
        assert len(eager_calls) > 0
        eager = {k: getattr(fin, k).clone() for k in ("rate", "code", "thr", "germ_val", "germ_present")}
        eager_mask = out.mask.clone()
        key = lambda a: np.sort((a["sample"].astype(np.int64) * P + a["record"]) * 4 + a["alt"])
        torch.cuda.synchronize()
        g_ctx.graph_begin()
        one_pass()
        graph = g_ctx.graph_end()
        try:
            for _ in range(2):
                _repoison_table(fin)
                out.repoison()
                torch.cuda.synchronize()
                g_ctx.graph_launch(graph)
                g_ctx.sync()
                for k, v in eager.items():
                    assert torch.equal(getattr(fin, k).view(torch.uint8), v.view(torch.uint8)), k
                assert torch.equal(out.mask, eager_mask)
                _check_table(fin, want)
                assert np.array_equal(key(out.check(exp["call_mask"])), key(eager_calls))
        finally:
            g_ctx.graph_destroy(graph)
        assert g_ctx.flags() == 0
    finally:
        g_ctx.close()
