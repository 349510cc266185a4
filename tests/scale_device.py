"""Device-side helpers of the index-range tests (tests/test_gpu_launch_splits.py, tests/test_gpu_wide_offsets.py) -- TEST
INFRASTRUCTURE: a few base rows repeated along the row dimension on the device, a byte-for-byte comparison of a large output with
its period without downloading it, and the memory gate every large test passes first."""
import ctypes as C

import pytest

GIB = 1 << 30
MAX_TEST_BYTES = 12 * GIB  # what one test may allocate on the device
CHUNK_BYTES = 64 << 20     # the temporaries of a comparison


def free_bytes(ctx):
    """free device memory as the library reports it (ampli_mem_info), torch's cached blocks given back first"""
    import torch

    torch.cuda.empty_cache()
    free, total = C.c_size_t(0), C.c_size_t(0)
    ctx._check(ctx.lib.ampli_mem_info(ctx.h, C.byref(free), C.byref(total)))
    return int(free.value)


def need(ctx, nbytes):
    """skip unless twice `nbytes` are free"""
    assert nbytes <= MAX_TEST_BYTES, f"a test may allocate {MAX_TEST_BYTES >> 30} GiB at the most, not {nbytes / GIB:.1f}"
    free = free_bytes(ctx)
    if free < 2 * nbytes:
        pytest.skip(f"needs {nbytes / GIB:.2f} GiB of device memory with as much again to spare; ampli_mem_info reports {free / GIB:.2f} GiB free")


def release(*tensors):
    """the caller has dropped its own references (del): give the blocks back to the device"""
    import torch

    del tensors
    torch.cuda.empty_cache()


def tile_rows(base, n):
    """base [b, ...] repeated along dim 0 to n rows, on the device, without a second copy of the result"""
    import torch

    b = base.shape[0]
    out = torch.empty((n,) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    k = n // b
    if k:
        out[:k * b].view((k, b) + tuple(base.shape[1:])).copy_(base.unsqueeze(0).expand((k, b) + tuple(base.shape[1:])))
    if n - k * b:
        out[k * b:].copy_(base[:n - k * b])
    return out


def as_ints(t):
    """the tensor's bytes as integers of its element size: NaN equals NaN, -0 differs from +0"""
    import torch

    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def rows_off_period(got, period, lo=0, hi=None):
    """how many of got's rows [lo, hi) differ, in any byte, from period[row % len(period)]; compared on the device in chunks"""
    import torch

    n, b = got.shape[0], period.shape[0]
    hi = n if hi is None else hi
    assert got.is_contiguous() and period.is_contiguous() and got.dtype == period.dtype and tuple(got.shape[1:]) == tuple(period.shape[1:])
    g, p = as_ints(got).reshape(n, -1), as_ints(period).reshape(b, -1)
    step = max(1, CHUNK_BYTES // max(1, g.shape[1] * g.element_size()))
    bad = torch.zeros((), dtype=torch.int64, device=got.device)
    for c0 in range(lo, hi, step):
        c1 = min(hi, c0 + step)
        idx = torch.arange(c0, c1, device=got.device) % b
        bad += (g[c0:c1] != p[idx]).any(dim=1).sum()
    return int(bad)


def assert_tiled(got, period, split=None, what="", second="the second launch"):
    """every row of `got` holds the bytes of its row of the period; with `split`, counted separately for the rows below it (the first
    launch) and from it on (the second launch, its partial last group included), so that a failure names the launch -- both counts
    in one message: a second launch whose base is a group too low shows up in the last rows of the first"""
    n = got.shape[0]
    if split is None:
        bad = rows_off_period(got, period)
        assert bad == 0, f"{what}: {bad} of {n} rows differ from their row of the period"
        return
    assert 0 < split < n
    first, rest = rows_off_period(got, period, 0, split), rows_off_period(got, period, split, n)
    assert first == 0 and rest == 0, (f"{what}: {rest} of the {n - split} rows of {second} (from row {split} on: its base offset) and {first} of the {split} rows "
                                      f"before them differ from their row of the period")
