"""Parity of the rolling-depth Conv3d 3x3x3 kernel (conv_roll.hip: the 16-bit
forward of DUF's dense-unit convs, duf_net.py:203,214, and their input
gradient) against torch fp64 on the CPU.

The kernel walks the input depth slices of a tile once and keeps one
accumulator bank per output depth in flight, so the cases cover what that
walk can get wrong: depth padding 1 (pad-1 units), 0 (depth-valid units,
down to one output depth) and 2 (the data gradient of a depth-valid unit),
partial spatial tiles, output-channel tiles of 32 with a partial last one,
channel-slice views of a wider buffer (the concat layout), the BN-affine+ReLU
prologue, and tiles that cover only part of the depth range (the depth-run
knob) or several tiles per workgroup (the grid cap).  Every depth-run / grid
setting must give BITWISE the same output: the accumulation order of an
output voxel does not depend on the tiling.

Tolerances as tests/test_conv_kernels_gpu.py: inputs and weights rounded to
the 16-bit type before the fp64 reference; max |d| <= 1.5e-2 * max|ref|
(bf16), 2e-3 * max|ref| (fp16).
"""
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fused_on(monkeypatch):
    """the fused entry points are tested whatever VSRK_FUSE says for the nets"""
    monkeypatch.setattr(F, "FUSE", True)


DEV = "cuda"


def _tol(dtype, ref):
    scale = max(ref.abs().max().item(), 1e-3)
    return (2e-3 if dtype == torch.float16 else 1.5e-2) * scale


def _q(t, dtype):
    return t.to(dtype).double()


def _ref(x_cl, w, b, pad):
    y = Fn.conv3d(x_cl.permute(0, 4, 1, 2, 3), w, b, padding=pad)
    return y.permute(0, 2, 3, 4, 1)


CASES = [
    # (N, D, H, W, Cin, Cout, depth pad, channel offset in a wider buffer)
    (2, 5, 9, 35, 32, 32, 1, 0),      # partial row / column tiles
    (1, 7, 16, 32, 64, 32, 1, 8),     # DUF pad-1 unit shape (one full tile), sliced input
    (1, 7, 12, 40, 48, 32, 0, 0),     # depth-valid unit: 7 -> 5
    (2, 3, 17, 33, 16, 40, 0, 16),    # 3 -> 1 output depth, cout 40: a partial 32-channel tile
    (1, 5, 10, 34, 32, 96, 2, 0),     # data gradient of a depth-valid unit: pad 2, 5 -> 7
    (1, 3, 16, 32, 224, 32, 0, 0),    # the last depth-valid unit (F = 224)
    (1, 2, 6, 9, 32, 32, 1, 0),       # fewer slices than kd taps
]


def _run(case, dtype, prologue, depth=0, cap=0, seed=0, roll=1):
    """roll=1 forces the rolling kernel (the default skips single output depths)"""
    n, d, h, w, ci, co, pdp, off = case
    g = torch.Generator().manual_seed(seed)
    big = torch.randn((n, d, h, w, ci + off + 8), generator=g)
    x = big[..., off:off + ci]
    wt = torch.randn((co, ci, 3, 3, 3), generator=g) / (27 * ci) ** 0.5
    b = torch.randn(co, generator=g)
    sc = torch.rand(ci, generator=g) + 0.5
    sh = torch.randn(ci, generator=g) * 0.5
    pad = (pdp, 1, 1)
    do = d + 2 * pdp - 2
    xin = _q(x, dtype)
    if prologue:
        xin = torch.relu(xin * sc.double() + sh.double()).to(dtype).double()
    ref = _ref(xin, _q(wt, dtype), b.double(), pad)
    ybig = torch.full((n, do, h, w, co + 8), 7.0, dtype=dtype, device=DEV)
    y = ybig[..., 4:4 + co]
    kw = dict(prologue=F.PRO_AFFINE_RELU, pro_scale=sc.to(DEV), pro_shift=sh.to(DEV)) if prologue else {}
    F.set_roll_depth(depth)
    F.set_grid_cap(cap)
    F.set_conv_path("roll", roll)
    try:
        F.conv(big.to(DEV, dtype)[..., off:off + ci], F.pack_weight(wt.to(DEV), 0, dtype), y, (3, 3, 3), pad,
               bias=b.to(DEV), **kw)
    finally:
        F.set_roll_depth(0)
        F.set_grid_cap(0)
        F.set_conv_path("roll", -1)
    torch.cuda.synchronize()
    # the channels outside the output slice are untouched
    assert (ybig[..., :4].float() == 7.0).all() and (ybig[..., 4 + co:].float() == 7.0).all()
    return y.double().cpu(), ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("prologue", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_roll_forward(case, prologue, dtype):
    y, ref = _run(case, dtype, prologue)
    err = (y - ref).abs().max().item()
    assert err <= _tol(dtype, ref), err


@pytest.mark.parametrize("case", CASES)
def test_roll_tiling_invariant(case):
    """depth runs of 1, 2, 3 output depths and a capped grid (many tiles per
    workgroup, the cross-tile DMA walk) give bitwise the default output"""
    y0, ref = _run(case, torch.bfloat16, True)
    assert (y0 - ref).abs().max().item() <= _tol(torch.bfloat16, ref)
    for depth, cap in ((1, 0), (2, 0), (3, 0), (0, 3), (2, 5), (1, 1)):
        y, _ = _run(case, torch.bfloat16, True, depth, cap)
        assert torch.equal(y, y0), (depth, cap, (y - y0).abs().max().item())


def test_roll_forward_sample_split():
    """a batch whose view spans more than 2^31 elements (DUF's 256-channel
    concat buffer at cfg 5: 128 windows) runs on the rolling kernel in sample
    chunks (32-bit element offsets): bitwise equal to launches over each half,
    which fit -- the conv_fast fallback it used to take accumulates in another
    order"""
    n, d, h, w, cw, ci, co = 80, 7, 64, 64, 1024, 64, 32
    g = torch.Generator(device=DEV).manual_seed(3)
    big = torch.randn((n, d, h, w, cw), generator=g, device=DEV).to(torch.bfloat16)
    x = big[..., :ci]
    assert (n - 1) * big.stride(0) >= 2 ** 31 > (n // 2 - 1) * big.stride(0)
    wt = torch.randn((co, ci, 3, 3, 3), generator=g, device=DEV) / (27 * ci) ** 0.5
    b = torch.randn(co, generator=g, device=DEV)
    kw = dict(bias=b, prologue=F.PRO_AFFINE_RELU, pro_scale=torch.rand(ci, generator=g, device=DEV) + 0.5,
              pro_shift=torch.randn(ci, generator=g, device=DEV) * 0.5)
    wp = F.pack_weight(wt, 0, torch.bfloat16)
    y = torch.empty((n, d, h, w, co), dtype=torch.bfloat16, device=DEV)
    F.conv(x, wp, y, (3, 3, 3), (1, 1, 1), **kw)
    for lo, hi in ((0, n // 2), (n // 2, n)):
        yp = torch.empty((hi - lo, d, h, w, co), dtype=torch.bfloat16, device=DEV)
        F.conv(x[lo:hi], wp, yp, (3, 3, 3), (1, 1, 1), **kw)
        assert torch.equal(y[lo:hi], yp), (lo, (y[lo:hi].float() - yp.float()).abs().max().item())
    del big


def test_roll_wgrad_sample_split():
    """the rolling weight gradient over a view spanning more than 2^31
    elements runs in sample chunks, each reduced onto dw after the first:
    bitwise the two half-batch calls (the second accumulating)"""
    n, d, h, w, cw, ci, co = 80, 7, 64, 64, 1024, 64, 32
    g = torch.Generator(device=DEV).manual_seed(4)
    big = torch.randn((n, d, h, w, cw), generator=g, device=DEV).to(torch.bfloat16)
    x = big[..., :ci]
    dy = torch.randn((n, d, h, w, co), generator=g, device=DEV).to(torch.bfloat16)
    assert (n - 1) * big.stride(0) >= 2 ** 31 > (n // 2) * big.stride(0)
    kw = dict(prologue=F.PRO_AFFINE_RELU, pro_scale=torch.rand(ci, generator=g, device=DEV) + 0.5,
              pro_shift=torch.randn(ci, generator=g, device=DEV) * 0.5)
    dw = torch.empty((co, ci, 3, 3, 3), device=DEV)
    db = torch.empty(co, device=DEV)
    F.conv_wgrad(x, dy, (3, 3, 3), (1, 1, 1), dw, db, **kw)
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    F.conv_wgrad(x[:n // 2], dy[:n // 2], (3, 3, 3), (1, 1, 1), dw2, db2, **kw)
    F.conv_wgrad(x[n // 2:], dy[n // 2:], (3, 3, 3), (1, 1, 1), dw2, db2, accumulate=True, **kw)
    assert torch.equal(dw, dw2), (dw - dw2).abs().max().item()
    assert torch.equal(db, db2), (db - db2).abs().max().item()
    del big


def test_roll_matches_fast_path():
    """the rolling kernel and the per-kd-stage conv_fast kernel agree within
    16-bit rounding at a DUF unit shape (and the switch really changes path)"""
    case = (2, 7, 16, 64, 64, 32, 1, 0)
    y_roll, ref = _run(case, torch.bfloat16, True)
    y_fast, _ = _run(case, torch.bfloat16, True, roll=0)
    tol = _tol(torch.bfloat16, ref)
    assert (y_roll - ref).abs().max().item() <= tol
    assert (y_fast - ref).abs().max().item() <= tol
    assert not torch.equal(y_roll, y_fast)  # different accumulation order: a different kernel ran


def test_roll_data_gradient_duf_unit():
    """dgrad of a depth-valid DUF unit through the public path: dy is a 32-channel
    slice of the concat gradient, the output the unit's F-channel input gradient"""
    g = torch.Generator().manual_seed(5)
    n, d, h, w, f = 1, 7, 16, 32, 96
    x = torch.randn((n, d, h, w, f), generator=g)
    wt = torch.randn((32, f, 3, 3, 3), generator=g) / (27 * f) ** 0.5
    dC = torch.randn((n, d - 2, h, w, 256), generator=g)
    gy = dC[..., 128:160]
    xr = _q(x, torch.bfloat16).requires_grad_(True)
    _ref(xr, _q(wt, torch.bfloat16), None, (0, 1, 1)).backward(_q(gy, torch.bfloat16))
    dx = torch.empty((n, d, h, w, f), dtype=torch.bfloat16, device=DEV)
    F.conv(dC.to(DEV, torch.bfloat16)[..., 128:160], F.pack_weight(wt.to(DEV), 1, torch.bfloat16), dx, (3, 3, 3),
           (2, 1, 1))
    err = (dx.double().cpu() - xr.grad).abs().max().item()
    assert err <= _tol(torch.bfloat16, xr.grad), err


# ---- the 2-D form: 3x3 over depth-1 slices, 64-channel output blocks ----
# (N, D, H, W, Cin, Cout): EDSR body shapes with partial tiles, several
# samples, a (1,3,3) conv over a 3-slice volume, 128 output channels
CASES2D = [
    (3, 1, 20, 40, 64, 64),
    (2, 1, 16, 32, 32, 64),
    (1, 3, 9, 35, 64, 128),
    (2, 1, 33, 70, 64, 64),
]
EPI = ["plain", "relu", "res", "mask", "res_acc", "pro"]


def _run2d(case, dtype, epi, cap=0, roll=-1, seed=0):
    n, d, h, w, ci, co = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, d, h, w, ci), generator=g)
    wt = torch.randn((co, ci, 1, 3, 3), generator=g) / (9 * ci) ** 0.5
    b = torch.randn(co, generator=g)
    res = torch.randn((n, d, h, w, co), generator=g)
    msk = torch.randn((n, d, h, w, co), generator=g)
    old = torch.randn((n, d, h, w, co), generator=g)
    scale = 0.5 if epi in ("res", "mask") else 1.0
    sc = torch.rand(ci, generator=g) + 0.5
    sh = torch.randn(ci, generator=g)
    xin = _q(x, dtype)
    if epi == "pro":  # DUF's tail: BN-affine + ReLU prologue (duf_net.py:116-118)
        xin = torch.relu(xin * sc.double() + sh.double()).to(dtype).double()
    ref = _ref(xin, _q(wt, dtype), b.double(), (0, 1, 1)) * scale
    if epi == "relu":
        ref = torch.relu(ref)
    if epi == "mask":
        ref = ref * (_q(msk, dtype) > 0)
    if epi in ("res", "res_acc"):
        ref = ref + _q(res, dtype)
    if epi == "res_acc":
        ref = ref + _q(old, dtype)
    y = old.to(DEV, dtype) if epi == "res_acc" else torch.full((n, d, h, w, co), 7.0, dtype=dtype, device=DEV)
    kw = dict(bias=b.to(DEV), out_scale=scale)
    if epi == "relu":
        kw["act"] = F.ACT_RELU
    if epi == "mask":
        kw["mask"] = msk.to(DEV, dtype)
    if epi in ("res", "res_acc"):
        kw["residual"] = res.to(DEV, dtype)
    if epi == "res_acc":
        kw["accumulate"] = True
    if epi == "pro":
        kw.update(prologue=F.PRO_AFFINE_RELU, pro_scale=sc.to(DEV), pro_shift=sh.to(DEV))
    F.set_grid_cap(cap)
    F.set_conv_path("roll", roll)
    try:
        F.conv(x.to(DEV, dtype), F.pack_weight(wt.to(DEV), 0, dtype), y, (1, 3, 3), (0, 1, 1), **kw)
    finally:
        F.set_grid_cap(0)
        F.set_conv_path("roll", -1)
    torch.cuda.synchronize()
    return y.double().cpu(), ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", EPI)
@pytest.mark.parametrize("case", CASES2D)
def test_roll_2d(case, epi, dtype):
    y, ref = _run2d(case, dtype, epi)
    err = (y - ref).abs().max().item()
    assert err <= _tol(dtype, ref), err


@pytest.mark.parametrize("epi", EPI)
def test_roll_2d_tiling_invariant_and_path(epi):
    """a capped grid (many tiles per workgroup: the operand prefetch and the
    DMA walk cross tiles) gives bitwise the default output; the conv_fast
    path agrees within rounding and is a different kernel"""
    case = (2, 1, 33, 70, 64, 64)
    y0, ref = _run2d(case, torch.bfloat16, epi)
    for cap in (1, 3, 7):
        y, _ = _run2d(case, torch.bfloat16, epi, cap=cap)
        assert torch.equal(y, y0), (cap, (y - y0).abs().max().item())
    yf, _ = _run2d(case, torch.bfloat16, epi, roll=0)
    tol = _tol(torch.bfloat16, ref)
    assert (yf - ref).abs().max().item() <= tol
    assert (y0 - ref).abs().max().item() <= tol


# ---- sub-pixel forms: DRF's projections (drf_net.py:70-102) over shuffle-s views ----
PROJ = {2: (6, 2, 2), 4: (8, 4, 2)}


def _run_sub(r, form, epi, skip, cap=0, roll=-1, seed=0):
    """form "up": ConvTranspose2d as a 3x3 conv written through a shuffle-r
    output view (forward; "down_dgrad" is the same form with a flipped
    strided-conv weight); "down": the strided conv reading a shuffle-r input
    view ("up_dgrad" likewise).  epi: plain / prelu / acc."""
    k, s, p = PROJ[r]
    f, n, h, w = 64, 2, 13, 37
    g = torch.Generator().manual_seed(seed + r)
    tr = form in ("up", "up_dgrad")
    flip = form.endswith("dgrad")
    wt = torch.randn((f, f, k, k), generator=g) / (f * k) ** 0.5
    b = torch.randn(f, generator=g)
    weq, beq = F.subpixel_conv_weight(wt.to(DEV), b.to(DEV), k, s, p, transposed=tr)
    dt = torch.bfloat16
    wp = F.pack_weight(weq, 1 if flip else 0, dt)
    ys = form in ("up", "down_dgrad")
    if ys:
        x = torch.randn((n, 1, h, w, f), generator=g)
        y0 = torch.randn((n, 1, h * s, w * s, 2 * f), generator=g)
    else:
        x = torch.randn((n, 1, h * s, w * s, 2 * f), generator=g)
        y0 = torch.randn((n, 1, h, w, 2 * f), generator=g)
    xd = x.to(DEV, dt)[..., :f] if not ys else x.to(DEV, dt)
    yb = y0.to(DEV, dt)
    yv = yb[..., f:]
    slope = torch.tensor([0.25], device=DEV)
    kw = dict(subpixel=F.subpixel_code(k, s, p, tr, flip) if skip else 0)
    if not flip:
        kw.update(bias=beq, bias_r=1)
    if epi == "prelu":
        kw.update(act=F.ACT_PRELU, act_param=slope)
    if epi == "acc":
        kw.update(accumulate=True)
    F.set_grid_cap(cap)
    F.set_conv_path("roll", roll)
    try:
        F.conv(xd, wp, yv, (1, 3, 3), (0, 1, 1), x_shuffle=1 if ys else s, y_shuffle=s if ys else 1, **kw)
    finally:
        F.set_grid_cap(0)
        F.set_conv_path("roll", -1)
    torch.cuda.synchronize()
    return yb.double().cpu(), y0


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("form", ["up", "down", "up_dgrad", "down_dgrad"])
@pytest.mark.parametrize("epi", ["plain", "prelu", "acc"])
def test_roll_subpixel_forms(r, form, epi):
    """the rolling 2-D kernel over a shuffled operand, with and without the
    per-phase tap skip and at capped grids, against the conv_fast path (a
    different kernel, itself checked against fp64 in test_drf_kernels_gpu):
    equal within one bf16 rounding; tap skipping and the grid give BITWISE
    the same output (zero taps add exact zeros); the untouched half of the
    output buffer stays as it was."""
    if form.endswith("dgrad") and epi == "prelu":
        pytest.skip("data gradients carry no activation")
    yref, y0 = _run_sub(r, form, epi, skip=False, roll=0)
    y, _ = _run_sub(r, form, epi, skip=True)
    scale = max(yref.abs().max().item(), 1e-3)
    assert (y - yref).abs().max().item() <= 1.5e-2 * scale
    f = 64
    assert torch.equal(y[..., :f], y0[..., :f].to(torch.bfloat16).double())
    for skip, cap in ((False, 0), (True, 3)):
        y2, _ = _run_sub(r, form, epi, skip=skip, cap=cap)
        assert torch.equal(y2, y), (skip, cap)


@pytest.mark.parametrize("form", ["up_dgrad", "down_dgrad", "plain"])
@pytest.mark.parametrize("acc", [False, True])
def test_roll_prelu_bwd_fused(form, acc):
    """vsrk_conv_fwd_prelu_bwd: the data gradient of a DRF projection with the
    backward of the PReLU before it in the epilogue (drf_net.py:81-102) --
    against the conv followed by the separate prelu_bwd kernel: the output
    within one bf16 rounding (the fused form rounds a*t once, the unfused
    a*round(t)); the slope gradient equals the one recomputed in double from
    the fused output (1e-4 of sum |dx y| / a^2) and the unfused one within one
    output ulp per term (2^-7 sum |dx y| / a^2: sum dx*y cancels ~10^3-fold,
    so bf16 rounding alone moves it by a few %); twice the same launch is
    bitwise equal."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(11 + (form == "plain"))
    f, n, h, w, r = 64, 2, 13, 37, 4
    if form == "plain":
        x = torch.randn((n, 1, h, w, f), generator=g).to(DEV, dt)
        wt = torch.randn((f, f, 1, 3, 3), generator=g) / (9 * f) ** 0.5
        wp, kw, yshape = F.pack_weight(wt.to(DEV), 1, dt), {}, (n, 1, h, w, f)
    else:
        k, s, p = PROJ[r]
        tr = form == "up_dgrad"
        wt = torch.randn((f, f, k, k), generator=g) / (f * k) ** 0.5
        weq, _ = F.subpixel_conv_weight(wt.to(DEV), None, k, s, p, transposed=tr)
        wp = F.pack_weight(weq, 1, dt)
        code = F.subpixel_code(k, s, p, tr, True)
        if tr:  # x: high-res gradient through a shuffle-r view -> low-res
            x = torch.randn((n, 1, h * s, w * s, f), generator=g).to(DEV, dt)
            kw, yshape = dict(x_shuffle=s, subpixel=code), (n, 1, h, w, f)
        else:   # low-res gradient -> high-res through the output view
            x = torch.randn((n, 1, h, w, f), generator=g).to(DEV, dt)
            kw, yshape = dict(y_shuffle=s, subpixel=code), (n, 1, h * s, w * s, f)
    y_fwd = torch.randn(yshape, generator=g).to(DEV, dt)
    a = torch.tensor([0.2], device=DEV)
    da0 = torch.tensor([0.5], device=DEV)
    y_ref = torch.empty(yshape, dtype=dt, device=DEV)
    F.conv(x, wp, y_ref, (1, 3, 3), (0, 1, 1), **kw)
    da_ref = da0.clone()
    F.prelu_bwd(y_fwd, y_ref, a, y_ref, da_ref, acc)
    outs = []
    for _ in range(2):
        y = torch.empty(yshape, dtype=dt, device=DEV)
        da = da0.clone()
        assert F.conv_prelu_bwd(x, wp, y, (1, 3, 3), (0, 1, 1), y_fwd, a, da, acc, **kw)
        outs.append((y, da))
    y, da = outs[0]
    assert torch.equal(outs[1][0], y) and torch.equal(outs[1][1], da)
    scale = y_ref.float().abs().max().item()
    assert (y.float() - y_ref.float()).abs().max().item() <= 1e-2 * scale
    m = y_fwd.double()
    neg = m < 0
    base = da0.item() if acc else 0.0
    cond = (y_ref.double() * m)[neg].abs().sum().item() / 0.04
    own = base + (y.double() * m)[neg].sum().item() / 0.04
    assert abs(da.item() - own) <= 1e-4 * cond + 1e-3, (da.item(), own)
    assert abs(da.item() - da_ref.item()) <= 2 ** -7 * cond, (da.item(), da_ref.item(), cond)


@pytest.mark.parametrize("case", [(2, 7, 20, 40, 32, 64, 1), (1, 5, 16, 33, 32, 96, 2), (2, 3, 9, 35, 32, 224, 2)])
def test_roll_bn_backward_reduce_fused(case):
    """vsrk_conv_fwd_reduce on the rolling 3x3x3 data gradient: DUF's conv2
    dgrad (32 -> F channels, depth pad 1, or 2 for a depth-valid unit) with
    bn2's BN+ReLU backward reduce in the epilogue (duf_net.py:198-203) --
    the output bitwise equal to the unfused kernel, the sums within fp32
    summation noise of the separate reduce, bitwise run to run, and
    bitwise under a different grid (per-tile partials)."""
    n, d, h, w, ci, co, pdp = case
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(co + pdp)
    dy = torch.randn((n, d, h, w, ci + 16), generator=g).to(DEV, dt)[..., 8:8 + ci]  # a concat-buffer slice
    wt = (torch.randn((ci, co, 3, 3, 3), generator=g) / (27 * co) ** 0.5).to(DEV)
    wp = F.pack_weight(wt, 1, dt)
    do = d + 2 * pdp - 2
    t1 = torch.randn((n, do, h, w, co), generator=g).to(DEV, dt)
    st = torch.stack([(torch.rand(co, generator=g) + 0.5), torch.randn(co, generator=g),
                      torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) + 0.5]).to(DEV)
    y_ref = torch.empty_like(t1)
    F.conv(dy, wp, y_ref, (3, 3, 3), (pdp, 1, 1))
    ref = F.bn_relu_bwd_reduce(t1, y_ref, st)
    outs = []
    for cap in (0, 0, 5):
        F.set_grid_cap(cap)
        try:
            y = torch.empty_like(t1)
            red = F.conv_reduce(dy, wp, y, bnx=t1, st=st, k=(3, 3, 3), pad=(pdp, 1, 1))
        finally:
            F.set_grid_cap(0)
        assert red is not None
        assert torch.equal(y, y_ref)
        outs.append(red)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    err = (outs[0] - ref).abs().max().item()
    assert err <= 1e-5 * (1 + ref.abs().max().item()), err


@pytest.mark.parametrize("r", [2, 4])
def test_roll_pixel_shuffle_output_bias(r):
    """EDSR's upsampler conv (edsr_net.py Upsampler: Conv2d(F, r*r*F, 3) + PixelShuffle(r)):
    perm-packed weights, a y_shuffle output view and the bias in torch's
    pixel-shuffle order; the rolling kernel (2-D form, SP_Y) and the tile
    kernel both match the fp64 conv + pixel shuffle"""
    g = torch.Generator().manual_seed(11)
    n, h, w, f = 2, 20, 36, 64
    co = f * r * r
    x = torch.randn((n, 1, h, w, f), generator=g)
    wt = torch.randn((co, f, 3, 3), generator=g) / (9 * f) ** 0.5
    b = torch.randn(co, generator=g)
    dt = torch.bfloat16
    ref = Fn.pixel_shuffle(Fn.conv2d(_q(x, dt)[:, 0].permute(0, 3, 1, 2), _q(wt, dt), b.double(), padding=1), r)
    ref = ref.permute(0, 2, 3, 1).unsqueeze(1)
    outs = []
    for roll in (1, 0):
        y = torch.full((n, 1, h * r, w * r, f), 7.0, dtype=dt, device=DEV)
        F.set_conv_path("roll", roll)
        try:
            F.conv(x.to(DEV, dt), F.pack_weight(wt.to(DEV), 0, dt, perm_r=r), y, (1, 3, 3), (0, 1, 1),
                   bias=b.to(DEV), y_shuffle=r)
        finally:
            F.set_conv_path("roll", -1)
        torch.cuda.synchronize()
        outs.append(y.double().cpu())
    for y in outs:
        assert (y - ref).abs().max().item() <= _tol(dt, ref)
    assert not torch.equal(outs[0], outs[1])  # different accumulation order: the rolling kernel ran


@pytest.mark.parametrize("epi", ["res", "mask", "relu", "res_acc", "plain"])
@pytest.mark.parametrize("case", [(3, 1, 20, 40, 64, 64), (2, 1, 33, 70, 64, 64)])
def test_roll_2d_resident_weights_forced(case, epi):
    """The resident-weight (WR) 2-D form forced on every epilogue (VERDICT r4
    weak item 4): the prefetched residual / mask forms park their rows in two
    halves of the wave's own DMA pieces of a 24 KB slot.  The router keeps
    those two forms on streamed weights (slower with WR, not wrong).  Forced:
    within the fp64 tolerance, bitwise invariant under grid caps that walk
    many tiles per workgroup, and equal to the streamed-weight kernel except
    where its different fp32 summation order flips a bf16 rounding tie (one
    output ulp, on < 0.1 % of the elements: r5 tools/diag/wr_check.py found
    5-20 of 1.5-3e5, each with the fp64 value halfway between the two).  A
    stale or misplaced operand would be neither."""
    outs = {}
    try:
        for wr in (0, 2):
            F.set_conv_path("roll_wr", wr)
            for cap in (0, 3):
                outs[(wr, cap)], ref = _run2d(case, torch.bfloat16, epi, cap=cap)
    finally:
        F.set_conv_path("roll_wr", -1)
    tol = _tol(torch.bfloat16, ref)
    for key, y in outs.items():
        assert (y - ref).abs().max().item() <= tol, key
    for wr in (0, 2):
        assert torch.equal(outs[(wr, 3)], outs[(wr, 0)]), wr
    y0, y2 = outs[(0, 0)], outs[(2, 0)]
    d = (y2 - y0).abs()
    # one bf16 ulp of the output, plus a few fp32 ulps of the operands for
    # outputs that cancel (conv + residual ~ 0: 1.6e-6 vs 1.8e-6 seen)
    ulp = torch.maximum(y0.abs(), y2.abs()) * 2.0 ** -7 + 2.0 ** -18 * ref.abs().max().item()
    assert (d <= ulp).all(), float((d / ulp).max())
    assert int((d > 0).sum()) <= 1e-3 * d.numel(), int((d > 0).sum())


FOLD_CASES = [
    # (N, D=3, H, W, Cin, Cout, depth pad 0, channel offset): one output depth
    (1, 3, 16, 32, 224, 32, 0, 0),    # DUF's last unit (F = 224), one 32-row tile
    (2, 3, 40, 70, 48, 64, 0, 8),     # partial row / column tiles, two output blocks, sliced input
    (1, 3, 33, 32, 16, 32, 0, 0),     # one chunk per depth tap, a 1-row second tile
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", FOLD_CASES)
def test_roll_depth_fold(case, dtype):
    """the depth-folded form (conv_roll_fold.hip, conv_roll_impl.h's kernel
    built with 32-row tiles: 3 slices -> 1 output depth as a 3x3 conv over
    (kd, channel) chunks) against fp64 with
    and without the BN prologue, bitwise invariant under the grid cap, and
    bitwise equal to the 3-D rolling form it replaces (both accumulate an
    output voxel slice by slice, chunk by chunk, tap by tap)"""
    for prologue in (False, True):
        y, ref = _run(case, dtype, prologue)
        assert (y - ref).abs().max().item() <= _tol(dtype, ref)
        for cap in (1, 3):
            yc, _ = _run(case, dtype, prologue, cap=cap)
            assert torch.equal(yc, y), cap
    F.set_conv_path("roll_fold", 0)
    try:
        y3, _ = _run(case, dtype, True)
    finally:
        F.set_conv_path("roll_fold", -1)
    assert torch.equal(y3, y), (y3 - y).abs().max().item()
