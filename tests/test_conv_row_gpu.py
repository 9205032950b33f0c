"""The row-walking Conv 3x3 64 -> 64 kernel (conv_row.hip: forward and data
gradient of EDSR's body convs, edsr_net.py:108-114,182-190).

The kernel walks the input rows of a band once through a four-slot LDS ring,
computes one output row per stage from the three rows it meets and stores it
during the next stage, so the cases cover what that walk can get wrong: a
single row (both neighbours outside the image), a full / a one-column second
segment, channel-slice views of
wider buffers, bands of uneven height under grid caps, a band longer than the
ring, every epilogue form, both 16-bit types and both weight packings.

1. Parity against fp64 (torch conv2d / conv_transpose2d on the 16-bit-
   quantised operands), per element, no element excluded:
       |y - ref| <= h |ref| + 600 * 2^-24 * A + 2^-24
   h = 2^-8 (bf16) / 2^-11 (fp16): the half-ulp of the single final rounding;
   A = out_scale (conv(|x|, |w|) + |bias|) + |residual| + |old|: 576 fp32
   additions in any order plus the epilogue's few operations, each at most
   2^-24 relative to the magnitudes summed so far.
2. Band / cap invariance: bitwise equal outputs at grid caps 1, 3, 7 and the
   default grid, and on a repeated launch.
3. Against the tile kernel it replaces ("row" 0): at most one 16-bit ulp of the
   output (plus 2^-18 max|ref| for cancelling outputs) on at most 0.1 % of the
   elements.  The kernel accumulates an output element in the tile kernel's
   order (channel chunk, kw, kh; the same MFMA on the same operands), so the
   outputs are also asserted bitwise equal: a train step computes what it
   computed on the tile kernel.
4. Routing, read from the kernel's launch counter (the outputs do not show
   it): "row" 1 launches it, "row" 0 and an explicit roll_wr do not; shapes
   the row kernel does not take fall through to the existing kernels.
"""
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _launches():
    """launches of the row kernel so far"""
    import ctypes
    from vsr_amd import _native
    fn = _native.load().vsrk_conv_row_launches
    fn.restype = ctypes.c_ulonglong
    return int(fn())


EPI = ["plain", "relu", "res", "mask", "res_acc"]
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _row_on(monkeypatch):
    """every eligible form on the row kernel, whatever the default routing"""
    monkeypatch.setattr(F, "FUSE", True)
    F.set_conv_path("row", 1)
    yield
    F.set_conv_path("row", -1)
    F.set_grid_cap(0)


def _q(t, dtype):
    return t.to(dtype).double()


def _make(shape, seed):
    """operands on the CPU in fp32 (quantised by the callers)"""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return dict(
        x=torch.randn((n, 1, h, w, 64), generator=g),
        wt=torch.randn((64, 64, 1, 3, 3), generator=g) / (9 * 64) ** 0.5,
        b=torch.randn(64, generator=g),
        res=torch.randn((n, 1, h, w, 64), generator=g),
        msk=torch.randn((n, 1, h, w, 64), generator=g),
        old=torch.randn((n, 1, h, w, 64), generator=g),
    )


def _scale(epi):
    return 0.1 if epi in ("res", "mask") else 1.0  # EDSR's res_scale


def _conv64(x, w, mode):
    """fp64 conv (mode 0) / transposed conv (mode 1: what the mode-1 packing computes), channels-last in and out"""
    xc = x[:, 0].permute(0, 3, 1, 2)
    y = Fn.conv2d(xc, w[:, :, 0], padding=1) if mode == 0 else Fn.conv_transpose2d(xc, w[:, :, 0], padding=1)
    return y.permute(0, 2, 3, 1).unsqueeze(1)


def _reference(ops, dtype, epi, mode):
    """(ref, A): the fp64 result and the magnitude sum of the bound"""
    s = _scale(epi)
    xq, wq = _q(ops["x"], dtype), _q(ops["wt"], dtype)
    b = ops["b"].double().view(1, 1, 1, 1, -1)
    ref = (_conv64(xq, wq, mode) + b) * s
    mag = (_conv64(xq.abs(), wq.abs(), mode) + b.abs()) * s
    if epi == "relu":
        ref = torch.relu(ref)
    if epi == "mask":
        ref = ref * (_q(ops["msk"], dtype) > 0)
    if epi in ("res", "res_acc"):
        r = _q(ops["res"], dtype)
        ref, mag = ref + r, mag + r.abs()
    if epi == "res_acc":
        o = _q(ops["old"], dtype)
        ref, mag = ref + o, mag + o.abs()
    return ref, mag


def _launch(x, wp, y, b, epi, res=None, msk=None):
    kw = dict(bias=b, out_scale=_scale(epi))
    if epi == "relu":
        kw["act"] = F.ACT_RELU
    if epi == "mask":
        kw["mask"] = msk
    if epi in ("res", "res_acc"):
        kw["residual"] = res
    if epi == "res_acc":
        kw["accumulate"] = True
    F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), **kw)


def _run(ops, dtype, epi, mode=0, cap=0, row=1, sliced=False):
    """one launch on the GPU; sliced: x is channels 64..127 of a 144-channel
    buffer, y channels 8..71 of an 80-channel buffer"""
    x = ops["x"].to(DEV, dtype)
    n, _, h, w, _ = x.shape
    fill = ops["old"].to(DEV, dtype) if epi == "res_acc" else torch.full((n, 1, h, w, 64), 7.0, dtype=dtype, device=DEV)
    if sliced:
        xb = torch.full((n, 1, h, w, 144), 3.0, dtype=dtype, device=DEV)
        xb[..., 64:128] = x
        x = xb[..., 64:128]
        yb = torch.full((n, 1, h, w, 80), 7.0, dtype=dtype, device=DEV)
        yb[..., 8:72] = fill
        y = yb[..., 8:72]
    else:
        y = fill.clone()
    wp = F.pack_weight(ops["wt"].to(DEV), mode, dtype)
    F.set_grid_cap(cap)
    F.set_conv_path("row", row)
    try:
        _launch(x, wp, y, ops["b"].to(DEV), epi, ops["res"].to(DEV, dtype), ops["msk"].to(DEV, dtype))
    finally:
        F.set_grid_cap(0)
        F.set_conv_path("row", 1)
    torch.cuda.synchronize()
    if sliced:  # the channels outside the output slice are untouched
        assert (yb[..., :8].float() == 7.0).all() and (yb[..., 72:].float() == 7.0).all()
    return y.double().cpu()


_CACHE = {}


def _case(shape, dtype, epi, mode):
    """operands and fp64 reference of a case, computed once"""
    key = (shape, dtype, epi, mode)
    if key not in _CACHE:
        ops = _CACHE.setdefault(("ops", shape), _make(shape, seed=sum(shape)))
        _CACHE[key] = (ops,) + _reference(ops, dtype, epi, mode)
    return _CACHE[key]


def _check(y, ref, mag, dtype):
    h = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    bound = h * ref.abs() + 600 * 2.0 ** -24 * mag + 2.0 ** -24
    d = (y - ref).abs()
    print(f"max |d| / bound = {float((d / bound).max()):.3f}")
    bad = (~(d <= bound)).nonzero()  # (a NaN is a violation)
    assert len(bad) == 0, (len(bad), float((d / bound).max()), [(i, float(y[tuple(i)]), float(ref[tuple(i)]))
                                                               for i in bad[:8].tolist()])


# (N, H, W), sliced views, grid caps
PARITY = [
    ((1, 1, 7), False, (0,)),        # one row, partial columns
    ((2, 2, 128), False, (0,)),      # exactly one full segment
    ((1, 3, 129), False, (0,)),      # a second segment one column wide
    ((3, 9, 150), True, (0,)),       # two segments, channel-slice views of wider buffers
    ((2, 33, 70), False, (0, 1, 3, 5)),  # one band per image, uneven bands, more bands
    ((1, 40, 128), False, (1,)),     # a single 40-row band
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epi", EPI)
@pytest.mark.parametrize("shape,sliced,caps", PARITY)
def test_row_parity_fp64(shape, sliced, caps, epi, dtype, mode):
    ops, ref, mag = _case(shape, dtype, epi, mode)
    for cap in caps:
        _check(_run(ops, dtype, epi, mode, cap=cap, sliced=sliced), ref, mag, dtype)


@pytest.mark.parametrize("epi", EPI)
def test_row_band_and_cap_invariant(epi):
    ops = _CACHE.setdefault(("ops", (2, 33, 70)), _make((2, 33, 70), seed=105))
    y0 = _run(ops, torch.bfloat16, epi)
    assert torch.equal(_run(ops, torch.bfloat16, epi), y0)
    for cap in (1, 3, 7):
        y = _run(ops, torch.bfloat16, epi, cap=cap)
        assert torch.equal(y, y0), (cap, (y - y0).abs().max().item())


def _close_to_tile(y1, y0, ref_max):
    d = (y1 - y0).abs()
    ulp = torch.maximum(y0.abs(), y1.abs()) * 2.0 ** -7 + 2.0 ** -18 * ref_max
    ndiff = int((d > 0).sum())
    print(f"max d / ulp = {float((d / ulp).max()):.3f}, {ndiff} of {d.numel()} differ")
    assert (d <= ulp).all(), float((d / ulp).max())
    assert ndiff <= 1e-3 * d.numel(), ndiff
    return ndiff


@pytest.mark.parametrize("epi", EPI)
def test_row_against_tile_kernel_small(epi):
    ops, ref, _ = _case((2, 33, 70), torch.bfloat16, epi, 0)
    y1 = _run(ops, torch.bfloat16, epi, row=1)
    y0 = _run(ops, torch.bfloat16, epi, row=0)
    _close_to_tile(y1, y0, ref.abs().max().item())
    assert torch.equal(y1, y0)


@pytest.mark.parametrize("epi", EPI)
def test_row_against_tile_kernel_layer(epi):
    """the bench's layer: 64 slices of 128 x 128 (operands made on the GPU; no
    fp64 reference at this size: max|ref| >= max|tile output| (1 - 2^-7))"""
    g = torch.Generator(device=DEV).manual_seed(7)
    dt = torch.bfloat16
    shp = (64, 1, 128, 128, 64)
    x, res, msk, old = (torch.randn(shp, generator=g, device=DEV).to(dt) for _ in range(4))
    wt = torch.randn((64, 64, 1, 3, 3), generator=g, device=DEV) / 24.0
    b = torch.randn(64, generator=g, device=DEV)
    wp = F.pack_weight(wt, 0, dt)
    outs = []
    counts = []
    for row in (1, 0):
        n0 = _launches()
        y = old.clone() if epi == "res_acc" else torch.full(shp, 7.0, dtype=dt, device=DEV)
        F.set_conv_path("row", row)
        try:
            _launch(x, wp, y, b, epi, res, msk)
        finally:
            F.set_conv_path("row", 1)
        torch.cuda.synchronize()
        outs.append(y.double())
        counts.append(_launches() - n0)
    assert counts == [1, 0], counts  # the row kernel ran, then the tile kernel
    _close_to_tile(outs[0], outs[1], outs[1].abs().max().item() * (1 - 2.0 ** -7))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("epi", EPI)
def test_row_switch_off_is_tile_kernel(epi):
    """"row" 0 gives the tile kernel's output bitwise (the explicit roll_wr
    request for the tile kernel's default form keeps the row kernel aside)"""
    ops = _CACHE.setdefault(("ops", (2, 33, 70)), _make((2, 33, 70), seed=105))
    n0 = _launches()
    y1 = _run(ops, torch.bfloat16, epi, row=1)
    assert _launches() == n0 + 1
    y0 = _run(ops, torch.bfloat16, epi, row=0)
    assert _launches() == n0 + 1
    assert torch.equal(y0, y1)
    # the tile kernel's router: resident weights except for the prefetched residual / mask forms
    F.set_conv_path("roll_wr", 0 if epi in ("res", "mask") else 2)
    try:
        yt = _run(ops, torch.bfloat16, epi, row=1)
    finally:
        F.set_conv_path("roll_wr", -1)
    assert _launches() == n0 + 1  # an explicit roll_wr keeps the row kernel aside
    assert torch.equal(y0, yt)


def test_row_falls_through():
    """a 32-channel input, a shuffled output and a prologue are not the row
    kernel's: the calls succeed on the existing kernels"""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(3)
    n, h, w = 1, 8, 20
    n0 = _launches()
    b = torch.randn(64, generator=g).to(DEV)
    # 32 input channels
    x32 = torch.randn((n, 1, h, w, 32), generator=g)
    w32 = torch.randn((64, 32, 1, 3, 3), generator=g) / (9 * 32) ** 0.5
    y = torch.full((n, 1, h, w, 64), 7.0, dtype=dt, device=DEV)
    F.conv(x32.to(DEV, dt), F.pack_weight(w32.to(DEV), 0, dt), y, (1, 3, 3), (0, 1, 1), bias=b)
    ref = _conv64(_q(x32, dt), _q(w32, dt), 0) + b.double().cpu().view(1, 1, 1, 1, -1)
    assert (y.double().cpu() - ref).abs().max().item() <= 1.5e-2 * ref.abs().max().item()
    # shuffled output (64 channels = 2 x 2 phases of 16) and the BN-affine + ReLU prologue
    x = torch.randn((n, 1, h, w, 64), generator=g)
    wt = torch.randn((64, 64, 1, 3, 3), generator=g) / 24.0
    ys = torch.full((n, 1, 2 * h, 2 * w, 16), 7.0, dtype=dt, device=DEV)
    F.conv(x.to(DEV, dt), F.pack_weight(wt.to(DEV), 0, dt, perm_r=2), ys, (1, 3, 3), (0, 1, 1), bias=b, y_shuffle=2)
    yp = torch.full((n, 1, h, w, 64), 7.0, dtype=dt, device=DEV)
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    F.conv(x.to(DEV, dt), F.pack_weight(wt.to(DEV), 0, dt), yp, (1, 3, 3), (0, 1, 1), bias=b,
           prologue=F.PRO_AFFINE_RELU, pro_scale=sc.to(DEV), pro_shift=sh.to(DEV))
    torch.cuda.synchronize()
    xin = torch.relu(_q(x, dt) * sc.double() + sh.double()).to(dt).double()
    refp = _conv64(xin, _q(wt, dt), 0) + b.double().cpu().view(1, 1, 1, 1, -1)
    assert (yp.double().cpu() - refp).abs().max().item() <= 1.5e-2 * refp.abs().max().item()
    assert torch.isfinite(ys.float()).all() and not (ys.float() == 7.0).all()
    assert _launches() == n0
