"""The host library's in-silico dilution (ampli_host_philox4x32_10, ampli_host_thin, ampli_host_dilute_keep, ampli_host_dilute_records:
csrc/ampli_math.h's text, the text dilute_kernel runs) against the model (tests/dilution_model.py), every integer equal, without a GPU."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd import host_lib
from amplisolve_amd._lib import DiluteMix
from tests import dilution_model as dm
from tests.dilution_cohorts import SHAPES, case, special

KEYS = (0x0123456789ABCDEF, 0xFFFFFFFF00000001)
NS = (0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 20000)
KEEPS = (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_dilute(recs_a, recs_b, P, mix, stride_a=0, stride_b=0):
    arr = (DiluteMix * len(mix))(*[DiluteMix(ra, rb, ka, kb, key) for ra, rb, ka, kb, key in mix])
    out = np.full((len(mix), P, 8), -1, np.int32)
    flags = np.full(len(mix), -1, np.int32)
    rc = host_lib().ampli_host_dilute_records(_p(recs_a), recs_a.shape[0], stride_a, _p(recs_b), recs_b.shape[0] if recs_b is not None else 0, stride_b, P,
                                              C.cast(arr, C.c_void_p), len(mix), _p(out), _p(flags))
    return rc, out, flags


def test_known_answers():
    for ctr, key, want in dm.KNOWN:
        out = (C.c_uint32 * 4)()
        host_lib().ampli_host_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
        assert tuple(out) == want


def test_thin_equals_the_model_on_the_grid():
    L = host_lib()
    grid = [(n, keep, key, 1000003 * (f + 1) + side, f | side << 3) for n in NS for keep in KEEPS for key in KEYS for f in range(8) for side in range(2)]
    n, keep, key, p, fs = (np.array([g[i] for g in grid], dtype=np.uint64 if i in (1, 2) else np.int64) for i in range(5))
    want = dm.thin_cells(n, keep, key, p, fs)
    got = [L.ampli_host_thin(int(a), int(b), int(c), int(d), int(e) & 7, int(e) >> 3) for a, b, c, d, e in zip(n, keep, key, p, fs)]
    assert list(want) == got
    full = keep == 1 << 32
    assert np.array_equal(want[full], n[full]) and not want[keep == 0].any() and (want[(keep == 1 << 31) & (n == 20000)] > 9000).all()
    assert L.ampli_host_thin(-1, 5, 0, 0, 0, 0) == -1 and L.ampli_host_thin(5, (1 << 32) + 1, 0, 0, 0, 0) == -1
    assert L.ampli_host_thin(5, 5, 0, 0, 8, 0) == -1 and L.ampli_host_thin(5, 5, 0, 0, 0, 2) == -1


def test_keep_equals_the_model():
    L = host_lib()
    for x in (0.0, 1.0, 0.5, 0.1, 0.02, 0.004, 1e-9, 2.0 ** -33, 2.0 ** -34, 0.1 * 0.7, (1 - 0.1) * 0.7, 1 - 2.0 ** -40):
        assert L.ampli_host_dilute_keep(x) == dm.keep_of(x)
    for x in (-1e-9, 1.0000001, float("nan"), float("inf")):
        assert L.ampli_host_dilute_keep(x) == 2 ** 64 - 1


@pytest.mark.parametrize("kind", ["same", "different"])
@pytest.mark.parametrize("P,n_mix", SHAPES)
def test_records_equal_the_model(P, n_mix, kind):
    A, B, mix, want, want_flags = case(P, n_mix, kind)
    rc, out, flags = host_dilute(A[0], B[0], P, mix, stride_a=A[0].shape[1], stride_b=B[0].shape[1])  # a row is P + E records
    assert rc == 0 and np.array_equal(out, want) and np.array_equal(flags, want_flags)
    if P >= 63:
        assert (want[:, :, 0] == dm.ABSENT).any() and (want[:, :, 0] != dm.ABSENT).sum() > P // 2


def test_edges_of_the_count_range_and_bad_mixtures():
    recs, mix, want, want_flags = special()
    rc, out, flags = host_dilute(recs, recs, recs.shape[1], mix)
    assert rc == 0 and np.array_equal(out, want) and np.array_equal(flags, want_flags)
    assert 0.29 < out[0, 0, 0] / dm.MAX_COUNT < 0.31
    # without a chunk b a mixture that names a row of it is a bad mixture, and down-sampling is what it was
    rc, out, flags = host_dilute(recs, None, recs.shape[1], [mix[0], (0, 0, 5, 5, 1)])
    assert rc == 0 and np.array_equal(out[0], want[0]) and list(flags) == [0, dm.BAD_MIXTURE] and (out[1, :, 0] == dm.ABSENT).all() and not out[1, :, 1:].any()


def test_refusals_leave_the_outputs():
    recs, mix, _, _ = special()
    L, P = host_lib(), recs.shape[1]
    arr = (DiluteMix * 1)(DiluteMix(*mix[2]))
    out, flags = np.full((1, P, 8), -1, np.int32), np.full(1, -1, np.int32)

    def call(a=recs, n_a=2, sa=0, b=recs, n_b=2, sb=0, P_=P, m=arr, n=1, o=out, f=flags):
        return L.ampli_host_dilute_records(_p(a), n_a, sa, _p(b), n_b, sb, P_, C.cast(m, C.c_void_p) if m is not None else None, n, _p(o), _p(f))

    bad = [call(a=None), call(m=None), call(o=None), call(f=None), call(P_=0), call(P_=-4), call(n=0), call(n_a=0), call(n_b=-1), call(b=None, n_b=2),
           call(sa=P - 1), call(sb=P - 1)]
    assert bad == [-1] * len(bad) and call(P_=2 ** 31 - 1, sa=2 ** 31, sb=2 ** 31) == -6
    assert (out == -1).all() and (flags == -1).all()
    assert call() == 0 and (out != -1).any() and flags[0] == dm.BAD_COUNT
