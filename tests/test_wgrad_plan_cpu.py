"""vsrk_conv_wgrad_workspace_size walks the weight gradient's candidate chain
(conv_wgrad.hip: pw, roll, roll in sample chunks, row, generic) and returns
the largest candidate's slab bytes.  The query is host-only (test_abi_cpu.py
relies on that too), so the plans behind it are pinned here without a device:
one small shape per candidate, in the default modes and with the rolling-depth
and rolling-row candidates switched off.

The byte counts are those of the library of commit 9756f55 ("Nets: one op
tape and gradient ledger"), the last one before the candidates shared one
chain, built and queried on a host without a device.  Without a device
vsrk_num_cus() answers 256, which is also the MI355X's CU count, so the same
numbers hold on both.
"""
import ctypes as C

import pytest

from vsr_amd._native import VSRK_BF16, VSRK_F32, ConvDesc, Tensor5

# name: (dtype, kernel, pad, (n, d, h, w), cin, cout)
SHAPES = {
    "roll 3x3x3 64->32": (VSRK_BF16, (3, 3, 3), (1, 1, 1), (2, 5, 20, 40), 64, 32),
    "row 3x3 64->64": (VSRK_BF16, (1, 3, 3), (0, 1, 1), (3, 1, 40, 70), 64, 64),
    "ragged 3x3 40->24": (VSRK_BF16, (1, 3, 3), (0, 1, 1), (2, 1, 17, 33), 40, 24),
    "pw 1x1x1 128->256": (VSRK_BF16, (1, 1, 1), (0, 0, 0), (2, 3, 16, 32), 128, 256),
    "thin 3x3 1->64": (VSRK_BF16, (1, 3, 3), (0, 1, 1), (2, 1, 24, 40), 1, 64),
    "fp32 3x3 64->64": (VSRK_F32, (1, 3, 3), (0, 1, 1), (1, 1, 20, 40), 64, 64),
}
# bytes in the default modes, with path "wgrad_roll" at 0, with path "wgrad_row" at 0
EXPECTED = {
    "roll 3x3x3 64->32": (26634240, 13294080, 26634240),
    "row 3x3 64->64": (6647040, 6647040, 6647040),  # (the generic plan's slabs outweigh the row kernel's here)
    "ragged 3x3 40->24": (886272, 886272, 886272),
    "pw 1x1x1 128->256": (6340608, 6340608, 6340608),
    "thin 3x3 1->64": (887808, 887808, 887808),
    "fp32 3x3 64->64": (887808, 887808, 887808),
}
MODES = (None, "wgrad_roll", "wgrad_row")


def _dense(dtype, dims, c):
    n, d, h, w = dims
    return Tensor5(None, n, d, h, w, c, d * h * w * c, h * w * c, w * c, c, 1, dtype)


def _query(native, name):
    dtype, k, pad, dims, cin, cout = SHAPES[name]
    desc = ConvDesc(*k, *pad, 0, 0, 1.0, 0, 1)
    x = _dense(dtype, dims, cin)
    dy = _dense(dtype, dims, cout)
    return native.vsrk_conv_wgrad_workspace_size(C.byref(desc), C.byref(x), C.byref(dy))


@pytest.mark.parametrize("name", list(SHAPES))
def test_wgrad_workspace_bytes(native, name):
    got = []
    try:
        for off in MODES:
            for path in MODES[1:]:
                assert native.vsrk_conv_set_path(path.encode(), 0 if path == off else -1) == 0
            got.append(_query(native, name))
    finally:
        for path in MODES[1:]:
            native.vsrk_conv_set_path(path.encode(), -1)
    assert tuple(got) == EXPECTED[name]
