"""Byte offsets of 2^31 and 2^32 and more: record reads through a row stride of 2 GiB, and outputs of 4.4 GB.

Every record read of the library is `base + (row * row_stride + p) * rec_bytes` (or the same through ext / ext_stride), every output
`out + (row * P + p) * k`.  Read before these tests were run, every one of them widens to size_t before the product: rec_counts and
rec_load_at's callers (ampli_device.h; limits, loo, dispersion and overdispersion go through rec_counts), error_reduce_kernel and
compact_reduce_body (`q = rv.base + ((size_t)min(s0, S - 1) * (size_t)rv.row_stride + (size_t)p) * RB`, then `q += row_step`),
error_sums_inorder, poisson_call_kernel / poisson_full_kernel / poisson_stream_kernel, nb_score_kernel, paired_score_kernel, di_load,
genotype_planes_kernel, contamination_kernel, amplicon_depth_kernel, spectrum_kernel and exceedance_kernel.  Nothing holds them to
that but these tests.

C. Record reads.  One allocation of 6 GiB, filled with the byte 0x01 (as a record: present, 257 / 65793 / 16843009 reads in every field,
which no row of the cohort holds).  The records' base lies 2 GiB into it; a chunk of 3 rows of 130 positions is written with a row
stride that puts row 1 a row's length past 2^31 bytes and row 2 two rows' lengths past 2^32 bytes from the base
(tests/scale_shapes.wide_stride, per layout).  An offset cut to 32 bits then lands behind row 0, one sign-extended from 32 bits below
the base: both inside the allocation, on the pattern -- a wrong value, not a fault (tests/test_scale_shapes.py works the cases out).
For the kernels that read extra occurrences a second placement does the same with ext / ext_stride (E = 9).  The two-cohort entry
points get the wide chunk on either side in turn; contamination_records takes ONE chunk of records (its sources are planes), so it
has one side.  Per entry point and layout: the outputs on the strided chunk equal, byte for byte, the outputs on a dense copy of the
same rows (which the feature's own tests hold to the model); the rows are unchanged and every other byte of the allocation is still
the pattern.

D. Outputs.  pair_score, dilute and nb_score at 4 * 65535 + 5 rows of 520 positions write 4.36 GB through their cheap paths -- pairs
that name a row outside the chunk, bad mixtures, absent records -- with real work in four rows: row 0, the first row that starts past
2^31 bytes, the first past 2^32 bytes, and the last.  Those rows equal the model; all other cells are NA / ABSENT, counted in one
reduction on the device; the fence around the output is whole.

NOT covered, because the case alone needs tens of GB: poisson_call and loo masks beyond 4 GiB; fdr_adjust planes beyond 4 GiB;
P >= 2^28, the first size at which `plane * P + p` passes 2^31."""
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


# ==== D. outputs beyond 2^32 bytes (first in the file: they run before the 6 GiB of C are allocated) ==================================

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
            off = sh.WIDE_BASE + r * stride * rb
            self.buf[off:off + src.numel()].copy_(src)
            self.placed.append((off, src.clone()))
        return self.buf[sh.WIDE_BASE:], stride

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

    nbytes = (max(sh.wide_bytes(lay) for lay in LAYOUTS) + 4095) // 4096 * 4096
    need(ctx, nbytes)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=ctx.device)
    buf.fill_(PATTERN)
    a = Arena(buf)
    yield a
    _BUNDLES.clear()
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
