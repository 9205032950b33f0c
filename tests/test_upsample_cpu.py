"""vsrk_upsample2d_fwd / _bwd reject bad arguments on the host, without a
launch (no device needed): VSRK_ERR_INVALID with a vsrk_last_error text."""
import ctypes as C

import pytest

INVALID = 1  # VSRK_ERR_INVALID
F32 = 0


def _call(native, fn, x=0x1000, y=0x2000, dtype=F32, planes=1, h=4, w=4, r=2, mode=0, ac=0, acc=0):
    return getattr(native, fn)(dtype, C.c_void_p(x), planes, h, w, r, mode, ac, acc, C.c_void_p(y), None)


@pytest.mark.parametrize("fn", ["vsrk_upsample2d_fwd", "vsrk_upsample2d_bwd"])
def test_bad_arguments_are_invalid(native, fn):
    assert _call(native, fn, x=None) == INVALID
    assert b"null" in native.vsrk_last_error()
    assert _call(native, fn, y=None) == INVALID
    assert _call(native, fn, r=0) == INVALID
    assert b"scale factor" in native.vsrk_last_error()
    assert _call(native, fn, r=-2) == INVALID
    assert _call(native, fn, h=0) == INVALID
    assert _call(native, fn, w=0) == INVALID
    assert _call(native, fn, planes=0) == INVALID
    assert _call(native, fn, mode=2) == INVALID
    assert _call(native, fn, ac=2) == INVALID
    assert _call(native, fn, acc=-1) == INVALID
    assert _call(native, fn, dtype=7) == INVALID


@pytest.mark.parametrize("fn", ["vsrk_upsample2d_fwd", "vsrk_upsample2d_bwd"])
def test_sizes_past_the_index_range_are_invalid(native, fn):
    # an output row longer than 2^30, and an output of 2^32 elements or more
    assert _call(native, fn, w=1 << 29, r=4) == INVALID
    assert _call(native, fn, planes=1 << 20, h=64, w=64, r=1) == INVALID
    assert _call(native, fn, planes=1 << 40, h=1, w=1, r=1) == INVALID
