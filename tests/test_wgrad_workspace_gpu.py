"""vsrk_conv_wgrad never picks its kernel by the size of the workspace: a
workspace too small for the first eligible candidate is an error before any
launch, on the rolling-depth and rolling-row paths as on the pointwise and
generic ones (they used to fall through to another kernel, whose sums have
other bits).  One shape per rolling path, called through the C ABI with one
byte less than vsrk_conv_wgrad_workspace_size answers, then with all of it.
"""
import ctypes as C

import pytest
import torch

from vsr_amd import _native as N
from vsr_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0

CASES = {
    # path: (kernel, pad, (n, d, h, w), cin, cout)
    "roll": ((3, 3, 3), (1, 1, 1), (1, 3, 8, 32), 32, 32),
    "row": ((1, 3, 3), (0, 1, 1), (1, 1, 8, 32), 64, 64),
}


@pytest.mark.parametrize("path", list(CASES))
def test_wgrad_short_workspace_is_an_error(path):
    k, pad, dims, ci, co = CASES[path]
    g = torch.Generator().manual_seed(17)
    x = torch.randn((*dims, ci), generator=g).to(DEV, torch.bfloat16)
    dy = torch.randn((*dims, co), generator=g).to(DEV, torch.bfloat16)
    lib = N.load()
    d = F._desc(k, pad)
    xv, gv = N.t5(x), N.t5(dy)
    need = lib.vsrk_conv_wgrad_workspace_size(C.byref(d), C.byref(xv), C.byref(gv))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dw = torch.full((co, ci, *k), SENTINEL, device=DEV)
    db = torch.full((co,), SENTINEL, device=DEV)

    def call(nbytes):
        return lib.vsrk_conv_wgrad(C.byref(d), C.byref(xv), C.byref(gv), None, None, 1.0, 1, dw.data_ptr(),
                                   db.data_ptr(), 0, ws.data_ptr(), nbytes, N.stream_ptr(x.device))

    rc = call(need - 1)
    msg = lib.vsrk_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0
    assert str(need - 1) in msg and str(need) in msg, msg
    assert torch.all(dw == SENTINEL) and torch.all(db == SENTINEL)
    assert call(need) == 0
    rw, rb = torch.empty_like(dw), torch.empty_like(db)
    F.conv_wgrad(x, dy, k, pad, rw, rb)
    torch.cuda.synchronize()
    assert torch.equal(dw, rw) and torch.equal(db, rb)
