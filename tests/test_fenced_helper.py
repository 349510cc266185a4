"""tests/helpers.fenced on the host: the fence that tests/test_gpu_output_contracts.py puts around every kernel output must itself
notice a single byte written on either side, and must not mind writes inside."""
import pytest
import torch

from tests.helpers import FENCE_ALIGN, FENCE_GUARD, fenced


@pytest.mark.parametrize("shape,dtype,poison", [((1,), torch.uint8, 0xFF), ((3, 7), torch.int32, 0xFF), ((2, 4, 65), torch.float32, 0xFF),
                                                 ((5, 3), torch.float64, 0xFF), ((1000,), torch.uint8, 0x5A), ((17,), torch.int64, 0x5A)])
def test_layout_and_poison(shape, dtype, poison):
    view, check = fenced(shape, dtype, poison, device="cpu")
    raw = check.raw
    nbytes = view.numel() * view.element_size()
    off = view.data_ptr() - raw.data_ptr()
    assert raw.dtype == torch.uint8 and tuple(view.shape) == shape and view.dtype == dtype
    assert view.data_ptr() % FENCE_ALIGN == 0 and off >= FENCE_GUARD
    assert raw.numel() - off - (nbytes + 15) // 16 * 16 >= FENCE_GUARD
    assert bool((raw == poison).all())
    check()
    if poison == 0xFF:  # what the poison reads as
        if dtype in (torch.float32, torch.float64):
            assert bool(torch.isnan(view).all())
        else:
            assert bool((view == (255 if dtype == torch.uint8 else -1)).all())


@pytest.mark.parametrize("shape,dtype", [((1,), torch.uint8), ((13,), torch.uint8), ((3, 5), torch.float32), ((16,), torch.float64)])
def test_a_write_of_one_byte_on_either_side_fails_and_writes_inside_pass(shape, dtype):
    view, check = fenced(shape, dtype, device="cpu")
    raw = check.raw
    nbytes = view.numel() * view.element_size()
    off = view.data_ptr() - raw.data_ptr()
    view.zero_()  # every byte inside
    check()
    view.fill_(1)
    check()
    for at in (off - 1, off + nbytes, 0, raw.numel() - 1, off - FENCE_GUARD, off + (nbytes + 15) // 16 * 16 + FENCE_GUARD - 1):
        raw[at] = 0xFE
        with pytest.raises(AssertionError):
            check()
        raw[at] = 0xFF
        check()
    # the rounding bytes a contract hands to the call: check(pad=k) lets the first k bytes behind the view go, and no more
    raw[off + nbytes] = 0
    with pytest.raises(AssertionError):
        check()
    check(pad=1)
    raw[off + nbytes + 1] = 0
    with pytest.raises(AssertionError):
        check(pad=1)
    check.repoison()
    check()
    assert bool((raw == 0xFF).all())
