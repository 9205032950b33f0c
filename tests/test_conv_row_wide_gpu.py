"""The wide row-walking Conv 3x3 64 -> 256 kernel that writes through a
shuffle-2 output view (conv_row_wide.hip: forward of EDSR's up-sampler convs,
edsr_net.py:117).

It is the row kernel's walk (test_conv_row_gpu.py) with other wave roles: a
wave owns 32 packed output rows (one half of one sub-pixel phase) and walks
the segment's four 32-voxel quarters per stage.  The cases are that file's:
a single row with a partial quarter, a full / a one-column second segment,
channel-slice views of wider buffers, bands of uneven height under grid caps,
a band longer than the ring, both 16-bit types, with and without bias,
out_scale 1 and 0.1.

1. Parity against fp64 (torch conv2d then pixel_shuffle(2) on the 16-bit-
   quantised operands), per element, no element excluded:
       |y - ref| <= h |ref| + 600 * 2^-24 * A + 2^-24
   h = 2^-8 (bf16) / 2^-11 (fp16); A = out_scale (conv(|x|, |w|) + |bias|):
   K = 576 per output as in the body conv, so that file's bound carries over.
2. Bitwise equality with the tile kernel it replaces ("row_wide" 1 against 0)
   on every shape of 1 and at 8 x 128 x 128 (every CU gets a workgroup), the
   launch counter moving by exactly 1, then 0.
3. Invariance: bitwise equal outputs at grid caps 1, 3, 7 and the default,
   and on a repeated launch.
4. Fall-through: shapes and epilogues that are not the kernel's run on the
   existing kernels and leave its counter alone.
5. Routing: an EDSRNet x4 forward moves the counter by the number of up-convs
   the default routes and is bitwise its output with "row_wide" 0.
"""
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
K3, P1 = (1, 3, 3), (0, 1, 1)


def _launches():
    """launches of the wide row kernel so far"""
    import ctypes
    from vsr_amd import _native
    fn = _native.load().vsrk_conv_row_wide_launches
    fn.restype = ctypes.c_ulonglong
    return int(fn())


@pytest.fixture(autouse=True)
def _wide_on():
    """every eligible shape on the wide kernel, whatever the default routing"""
    F.set_conv_path("row_wide", 1)
    yield
    F.set_conv_path("row_wide", -1)
    F.set_grid_cap(0)


def _q(t, dtype):
    return t.to(dtype).double()


def _make(shape, seed):
    """operands on the CPU in fp32 (quantised by the callers); torch layouts"""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return dict(
        x=torch.randn((n, 1, h, w, 64), generator=g),
        wt=torch.randn((256, 64, 1, 3, 3), generator=g) / (9 * 64) ** 0.5,
        b=torch.randn(256, generator=g),
    )


def _shuffled(x, w, b, r=2):
    """fp64 conv2d + bias then pixel_shuffle(r), channels-last (n, 1, r h, r w, c / r^2)"""
    y = Fn.conv2d(x[:, 0].permute(0, 3, 1, 2), w[:, :, 0], padding=1)
    if b is not None:
        y = y + b.view(1, -1, 1, 1)
    if r > 1:
        y = Fn.pixel_shuffle(y, r)
    return y.permute(0, 2, 3, 1).unsqueeze(1)


_CACHE = {}


def _case(shape, dtype, bias, scale):
    """operands and fp64 reference (ref, A) of a case, computed once"""
    key = (shape, dtype, bias, scale)
    if key not in _CACHE:
        ops = _CACHE.setdefault(("ops", shape), _make(shape, seed=sum(shape)))
        xq, wq = _q(ops["x"], dtype), _q(ops["wt"], dtype)
        b = ops["b"].double() if bias else None
        ref = _shuffled(xq, wq, b) * scale
        mag = _shuffled(xq.abs(), wq.abs(), b.abs() if bias else None) * scale
        _CACHE[key] = (ops, ref, mag)
    return _CACHE[key]


def _run(ops, dtype, bias=True, scale=1.0, cap=0, wide=1, sliced=False):
    """one launch on the GPU; sliced: x is channels 64..127 of a 144-channel
    buffer, y channels 8..71 of an 80-channel HR buffer"""
    x = ops["x"].to(DEV, dtype)
    n, _, h, w, _ = x.shape
    if sliced:
        xb = torch.full((n, 1, h, w, 144), 3.0, dtype=dtype, device=DEV)
        xb[..., 64:128] = x
        x = xb[..., 64:128]
        yb = torch.full((n, 1, 2 * h, 2 * w, 80), 7.0, dtype=dtype, device=DEV)
        y = yb[..., 8:72]
    else:
        y = torch.full((n, 1, 2 * h, 2 * w, 64), 7.0, dtype=dtype, device=DEV)
    wp = F.pack_weight(ops["wt"].to(DEV), 0, dtype, perm_r=2)
    F.set_grid_cap(cap)
    F.set_conv_path("row_wide", wide)
    try:
        F.conv(x, wp, y, K3, P1, bias=ops["b"].to(DEV) if bias else None, out_scale=scale, y_shuffle=2)
    finally:
        F.set_grid_cap(0)
        F.set_conv_path("row_wide", 1)
    torch.cuda.synchronize()
    if sliced:  # the channels outside the output slice are untouched
        assert (yb[..., :8].float() == 7.0).all() and (yb[..., 72:].float() == 7.0).all()
    return y.double().cpu()


def _check(y, ref, mag, dtype):
    h = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    bound = h * ref.abs() + 600 * 2.0 ** -24 * mag + 2.0 ** -24
    d = (y - ref).abs()
    print(f"max |d| / bound = {float((d / bound).max()):.3f}")
    bad = (~(d <= bound)).nonzero()  # (a NaN is a violation)
    assert len(bad) == 0, (len(bad), float((d / bound).max()), [(i, float(y[tuple(i)]), float(ref[tuple(i)]))
                                                               for i in bad[:8].tolist()])


# low-res (N, H, W), sliced views, grid caps
SHAPES = [
    ((1, 1, 7), False, (0,)),        # one row, partial quarter
    ((2, 2, 128), False, (0,)),      # exactly one full segment
    ((1, 3, 129), False, (0,)),      # a second segment one column wide
    ((3, 9, 150), True, (0,)),       # two segments, channel-slice views of wider buffers
    ((2, 33, 70), False, (0, 1, 3, 5)),  # one band per image, uneven bands, more bands
    ((1, 40, 128), False, (1,)),     # a single 40-row band: longer than the ring
]


@pytest.mark.parametrize("scale", [1.0, 0.1])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,sliced,caps", SHAPES)
def test_wide_parity_fp64(shape, sliced, caps, dtype, bias, scale):
    ops, ref, mag = _case(shape, dtype, bias, scale)
    for cap in caps:
        n0 = _launches()
        y = _run(ops, dtype, bias, scale, cap=cap, sliced=sliced)
        assert _launches() == n0 + 1
        _check(y, ref, mag, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,sliced,caps", SHAPES)
def test_wide_bitwise_tile_kernel(shape, sliced, caps, dtype):
    ops = _CACHE.setdefault(("ops", shape), _make(shape, seed=sum(shape)))
    for bias, scale in ((True, 1.0), (False, 0.1)):
        for cap in caps:
            n0 = _launches()
            y1 = _run(ops, dtype, bias, scale, cap=cap, wide=1, sliced=sliced)
            assert _launches() == n0 + 1
            y0 = _run(ops, dtype, bias, scale, cap=cap, wide=0, sliced=sliced)
            assert _launches() == n0 + 1
            assert torch.equal(y1, y0), (bias, scale, cap, int((y1 != y0).sum()), (y1 - y0).abs().max().item())


def test_wide_bitwise_tile_kernel_every_cu():
    """8 slices of 128 x 128 (operands made on the GPU): 256 items, every CU
    gets a workgroup -- the load at which the row kernel's 16-byte store hazard
    showed (conv_row_common.h, cr_store16)"""
    g = torch.Generator(device=DEV).manual_seed(11)
    dt = torch.bfloat16
    x = torch.randn((8, 1, 128, 128, 64), generator=g, device=DEV).to(dt)
    wt = torch.randn((256, 64, 1, 3, 3), generator=g, device=DEV) / 24.0
    b = torch.randn(256, generator=g, device=DEV)
    wp = F.pack_weight(wt, 0, dt, perm_r=2)
    outs, counts = [], []
    for wide in (1, 0):
        n0 = _launches()
        y = torch.full((8, 1, 256, 256, 64), 7.0, dtype=dt, device=DEV)
        F.set_conv_path("row_wide", wide)
        try:
            F.conv(x, wp, y, K3, P1, bias=b, y_shuffle=2)
        finally:
            F.set_conv_path("row_wide", 1)
        torch.cuda.synchronize()
        outs.append(y)
        counts.append(_launches() - n0)
    assert counts == [1, 0], counts  # the wide kernel ran, then the tile kernel
    assert torch.equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())


def test_wide_band_and_cap_invariant():
    ops = _CACHE.setdefault(("ops", (2, 33, 70)), _make((2, 33, 70), seed=105))
    y0 = _run(ops, torch.bfloat16)
    assert torch.equal(_run(ops, torch.bfloat16), y0)
    for cap in (1, 3, 7):
        y = _run(ops, torch.bfloat16, cap=cap)
        assert torch.equal(y, y0), (cap, (y - y0).abs().max().item())


def _fall(cout, r, **kw):
    """a (1, 8, 20) launch with `cout` output channels through a shuffle-r
    view: (y, fp64 reference of the plain conv + bias, shuffled)"""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(3 + cout + r)
    n, h, w = 1, 8, 20
    x = torch.randn((n, 1, h, w, 64), generator=g)
    wt = torch.randn((cout, 64, 1, 3, 3), generator=g) / 24.0
    b = torch.randn(cout, generator=g)
    y = torch.full((n, 1, r * h, r * w, cout // (r * r)), 7.0, dtype=dt, device=DEV)
    F.conv(x.to(DEV, dt), F.pack_weight(wt.to(DEV), 0, dt, perm_r=r), y, K3, P1, bias=b.to(DEV), y_shuffle=r, **kw)
    torch.cuda.synchronize()
    return y.double().cpu(), _shuffled(_q(x, dt), _q(wt, dt), b.double(), r)


def _loosely(y, ref):
    assert (y - ref).abs().max().item() <= 1.5e-2 * ref.abs().max().item()


def test_wide_falls_through():
    """other channel counts and shuffle factors, an unshuffled output, a ReLU,
    a residual and a tap-skip descriptor are not the wide kernel's: the calls
    succeed on the existing kernels"""
    n0 = _launches()
    _loosely(*_fall(128, 2))   # y->c == 128 with shuffle 2
    _loosely(*_fall(256, 4))   # 256 channels with shuffle 4
    _loosely(*_fall(256, 1))   # 256 channels unshuffled
    y, ref = _fall(256, 2, act=F.ACT_RELU)
    _loosely(y, torch.relu(ref))
    res = torch.randn((1, 1, 16, 40, 64), generator=torch.Generator().manual_seed(5))
    y, ref = _fall(256, 2, residual=res.to(DEV, torch.bfloat16))
    _loosely(y, ref + _q(res, torch.bfloat16))
    assert _launches() == n0
    # ConvTranspose2d(64, 64, 6, stride 2, padding 2) as a 3x3 conv on the sub-pixel grid with its zero taps skipped
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(9)
    x = torch.randn((1, 1, 8, 20, 64), generator=g)
    wd, bd = torch.randn((64, 64, 6, 6), generator=g) / 48.0, torch.randn(64, generator=g)
    weq, beq = F.subpixel_conv_weight(wd.to(DEV), bd.to(DEV), 6, 2, 2, True)
    y = torch.full((1, 1, 16, 40, 64), 7.0, dtype=dt, device=DEV)
    F.conv(x.to(DEV, dt), F.pack_weight(weq.unsqueeze(2), 0, dt), y, K3, P1, bias=beq, bias_r=1, y_shuffle=2,
           subpixel=F.subpixel_code(6, 2, 2, True, False))
    torch.cuda.synchronize()
    ref = Fn.conv_transpose2d(_q(x, dt)[:, 0].permute(0, 3, 1, 2), _q(wd, dt), bd.double(), stride=2, padding=2)
    _loosely(y.double().cpu(), ref.permute(0, 2, 3, 1).unsqueeze(1))
    assert _launches() == n0


def test_wide_default_routing_edsr():
    """EDSR x4 at 2 x 1 x 16 x 16: its two up-convs, at 16 x 16 and 32 x 32 low-res
    voxels; the default routes every eligible shape (conv_row_wide.hip, cw_default_on)"""
    from vsr_amd import nets
    torch.manual_seed(0)
    net = nets.EDSRNet(in_channels=1, out_channels=1, num_resblocks=2, num_features=64, upscale_factor=4)
    net = net.to(DEV).set_precision("bf16").eval()
    x = torch.randn((2, 1, 16, 16), generator=torch.Generator().manual_seed(1)).to(DEV)
    F.set_conv_path("row_wide", -1)
    want = 2
    with torch.no_grad():
        n0 = _launches()
        y1 = net(x)
        torch.cuda.synchronize()
        assert _launches() - n0 == want, (_launches() - n0, want)
        F.set_conv_path("row_wide", 0)
        n0 = _launches()
        y0 = net(x)
        torch.cuda.synchronize()
        assert _launches() == n0
    assert torch.equal(y1, y0)
