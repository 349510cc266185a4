"""Context.dilute (dilute_kernel) against the definition (tests/dilution_model.py): every integer equal, no tolerance.  The cohorts
(tests/dilution_cohorts.py) have dispersion_cohorts' record shapes -- absent records, positions listed twice (E > 0), an RD plane, a
padded row stride -- none of which may change a count, since only the primary record of (row, position) enters."""
import numpy as np
import pytest

from amplisolve_amd.api import DILUTE_BAD_COUNT, DILUTE_BAD_MIXTURE, DILUTE_KEEP_ALL, LIMIT_OK
from tests.dilution_cohorts import BAD_LIST, ROWS_A, SHAPES, case, special
from tests.dilution_model import ABSENT, MAX_COUNT
from tests.test_gpu_overdispersion import _chunks
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu


def _records(ctx, c, P, layout, pad=0):
    recs, E, dup_off, ext_pos, rd = c
    return _chunks(ctx, recs, P, E, dup_off, ext_pos, None if layout == "u16" else rd, layout, (0, recs.shape[0]), pad=pad)[0]


def _run(ctx, ra, rb, P, mix):
    out, flags = ctx.dilute(ra, rb, P, mix)
    return out.cpu().numpy(), flags.cpu().numpy()


LAYOUTS = ("i32", "u24", "u16")
# one chunk has one layout; two chunks have the three layouts independently
KINDS = [("same", a, a) for a in LAYOUTS] + [("different", a, b) for a in LAYOUTS for b in LAYOUTS]


@pytest.mark.parametrize("kind,lay_a,lay_b", KINDS)
@pytest.mark.parametrize("P,n_mix", SHAPES)
def test_every_integer_equals_the_model(ctx, kind, lay_a, lay_b, P, n_mix):
    A, B, mix, want, want_flags = case(P, n_mix, kind)
    ra = _records(ctx, A, P, lay_a, pad=3 if n_mix == 5 else 0)
    rb = _records(ctx, B, P, lay_b) if kind == "different" else ra
    got, flags = _run(ctx, ra, rb, P, mix)
    assert np.array_equal(got, want) and np.array_equal(flags, want_flags)
    again, flags2 = _run(ctx, ra, rb, P, mix)
    assert again.tobytes() == got.tobytes() and flags2.tobytes() == flags.tobytes()  # the same inputs give the same bytes
    if P >= 63:
        present = want[:, :, 0] != ABSENT
        assert (~present).any() and present.sum() > P // 2 and (want[present] > 0).any()


def test_a_mixture_alone_gives_its_bytes_of_the_batch(ctx):
    P = 65
    A, B, mix, want, _ = case(P, 9, "different")
    ra, rb = _records(ctx, A, P, "u16"), _records(ctx, B, P, "u24")
    batch, _ = _run(ctx, ra, rb, P, mix[2:7])  # a batch of five
    for i in (0, 3, 4):
        alone, flags = _run(ctx, ra, rb, P, [mix[2 + i]])
        assert alone[0].tobytes() == batch[i].tobytes() == want[2 + i].tobytes() and flags[0] == 0


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_identity(ctx, layout):
    """keep_a = 2^32 and no diluent: the output is a's primary records as int32"""
    P = 130
    A, _, _, _, _ = case(P, 9, "same")
    ra = _records(ctx, A, P, layout)
    got, flags = _run(ctx, ra, None, P, [(r, -1, DILUTE_KEEP_ALL, 0, 77 + r) for r in range(ROWS_A)])
    want = A[0][:, :P].copy()
    want[want[:, :, 0] == ABSENT, 1:] = 0
    assert np.array_equal(got, want) and not flags.any()


def test_edges_of_the_count_range_and_bad_mixtures(ctx):
    """one cell of 2^24 - 2 reads (the longest loop there is, drawn once), 2^24 - 1, negative counts, rows outside their chunk, keeps
    above 2^32"""
    recs, mix, want, want_flags = special()
    P = recs.shape[1]
    r = ctx.records(_t(recs), "i32", 2)
    got, flags = _run(ctx, r, r, P, mix)
    assert np.array_equal(got, want) and np.array_equal(flags, want_flags)
    assert flags[1] == DILUTE_BAD_COUNT and (flags[3:] == DILUTE_BAD_MIXTURE).all() and len(mix) == 3 + len(BAD_LIST) + 3
    assert 0.29 < got[0, 0, 0] / MAX_COUNT < 0.31
    # row_b >= 0 while recs_b is NULL: a bad mixture; down-sampling beside it is what it was
    got, flags = _run(ctx, r, None, P, [(0, 0, 5, 5, 1), mix[2]])
    assert list(flags) == [DILUTE_BAD_MIXTURE, DILUTE_BAD_COUNT] and (got[0, :, 0] == ABSENT).all() and not got[0, :, 1:].any()
    assert np.array_equal(got[1], want[2])


def test_a_device_tensor_of_descriptors_and_the_callers_buffers(ctx):
    import torch

    P = 63
    A, B, mix, want, _ = case(P, 3, "different")
    ra, rb = _records(ctx, A, P, "u24"), _records(ctx, B, P, "i32")
    words = np.array([[(ra_ & 0xFFFFFFFF) | (rb_ & 0xFFFFFFFF) << 32, ka, kb, key] for ra_, rb_, ka, kb, key in mix], dtype=np.uint64)
    out = torch.full((3, P, 8), -1, dtype=torch.int32, device=ctx.device)
    flags = torch.full((3,), -1, dtype=torch.int32, device=ctx.device)
    o2, f2 = ctx.dilute(ra, rb, P, _t(words.view(np.int64)), out=out, flags=flags)
    assert o2 is out and f2 is flags and np.array_equal(out.cpu().numpy(), want) and not flags.cpu().numpy().any()


def test_chained_into_detection_limits(ctx):
    """the wrapped output goes into detection_limits as it stands, and gives what the model's records give when uploaded"""
    P = 130
    A, B, mix, want, _ = case(P, 9, "different")
    rng = np.random.default_rng(1)
    thr = _t(np.array([float(f"{x:f}") for x in np.exp(rng.uniform(np.log(2e-4), np.log(0.02), 8 * P))], np.float32).reshape(2, 4, P))
    ref = _t(rng.integers(0, 4, P).astype(np.uint8))
    out, _ = ctx.dilute(_records(ctx, A, P, "u16"), _records(ctx, B, P, "u16"), P, mix)
    got = ctx.detection_limits(ctx.dilution_records(out), P, thr, ref, 30)
    exp = ctx.detection_limits(ctx.records(_t(np.array(want)), "i32", len(mix)), P, thr, ref, 30)
    for k in ("min_reads", "status", "counts"):
        assert got[k].cpu().numpy().tobytes() == exp[k].cpu().numpy().tobytes()
    assert (got["status"].cpu().numpy() & 7 == LIMIT_OK).any()  # some pairs are OK: the comparison is not of two empty planes
    packed, fits = ctx.pack(out, "u16")  # and ampli_records_pack16 takes it
    assert fits and np.array_equal(ctx.dilute(ctx.records(packed, "u16", len(mix)), None, P, [(m, -1, DILUTE_KEEP_ALL, 0, 0) for m in range(len(mix))])[0].cpu().numpy(), want)
