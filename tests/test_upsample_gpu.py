"""vsrk_upsample2d_fwd / _bwd (csrc/upsample.hip) against F.interpolate on the
CPU in fp64, through vsr_amd.functional, torch.ops.vsrk.upsample2d and
modules.HipUpsample.

Bounds are DESIGN section 4's kernel-against-fp64 figures, relative to
max|ref|: fp32 2e-5, fp16 2e-3, bf16 1.5e-2 (the 16-bit inputs are rounded
first, so the bound covers the fp32 arithmetic and one output rounding).

Shapes: one-pixel axes (align_corners=True divides by zero there if
mishandled), images smaller than the four bicubic taps, and an output row
(67 r) that is neither a multiple of 64 nor of the per-lane 16-byte run.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from vsr_amd import functional as F
from vsr_amd import modules

pytestmark = pytest.mark.gpu
DEV = "cuda"

MODES = ["bilinear", "bicubic"]
SCALES = [2, 3, 4, 8]
PLANES = [(1, 1), (2, 3)]
SIZES = [(1, 1), (1, 5), (2, 3), (5, 7), (9, 67)]
BOUND = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
DTYPES = list(BOUND)


def _data(planes, h, w, r, dtype, seed):
    """x (planes, h, w) with distinct content per plane, g and y0 of the output
    shape, all rounded to dtype (kept on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((*planes, h, w), generator=g) + torch.arange(planes[0] * planes[1]).view(*planes, 1, 1) * 0.25
    gy = torch.randn((*planes, h * r, w * r), generator=g)
    y0 = torch.randn((*planes, h * r, w * r), generator=g)
    return x.to(dtype), gy.to(dtype), y0.to(dtype)


def _ref(x, r, mode, ac):
    return Fn.interpolate(x.double(), scale_factor=r, mode=mode, align_corners=ac)


def _ref_bwd(gy, h, w, r, mode, ac):
    x = torch.zeros((*gy.shape[:2], h, w), dtype=torch.float64, requires_grad=True)
    Fn.interpolate(x, scale_factor=r, mode=mode, align_corners=ac).backward(gy.double())
    return x.grad


def _close(got, exp, dtype, what):
    err = (got.detach().cpu().double() - exp).abs().max().item()
    tol = BOUND[dtype] * exp.abs().max().item()
    print(f"{what}: max|d| {err:.3e} bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _cases():
    for planes in PLANES:
        for h, w in SIZES:
            for dtype in DTYPES:
                yield planes, h, w, dtype


@pytest.mark.parametrize("r", SCALES)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_forward_matches_interpolate(mode, ac, r):
    for i, (planes, h, w, dtype) in enumerate(_cases()):
        x, _, y0 = _data(planes, h, w, r, dtype, 100 + i)
        ref = _ref(x, r, mode, ac)
        what = f"{mode} ac={ac} r={r} {planes} {h}x{w} {dtype}"
        # accumulate = 0 overwrites whatever y held
        y = torch.full(ref.shape, float("nan"), dtype=dtype, device=DEV)
        assert F.upsample2d(x.to(DEV), y, mode, ac, r) is y
        assert not torch.isnan(y).any(), what
        _close(y, ref, dtype, "fwd " + what)
        # accumulate = 1 adds onto y
        y = y0.to(DEV)
        F.upsample2d(x.to(DEV), y, mode, ac, r, accumulate=True)
        _close(y, y0.double() + ref, dtype, "fwd+acc " + what)


@pytest.mark.parametrize("r", SCALES)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_backward_matches_autograd(mode, ac, r):
    for i, (planes, h, w, dtype) in enumerate(_cases()):
        x, gy, _ = _data(planes, h, w, r, dtype, 200 + i)
        ref = _ref_bwd(gy, h, w, r, mode, ac)
        what = f"{mode} ac={ac} r={r} {planes} {h}x{w} {dtype}"
        gx = torch.full(x.shape, float("nan"), dtype=dtype, device=DEV)
        assert F.upsample2d_bwd(gy.to(DEV), gx, mode, ac, r) is gx
        _close(gx, ref, dtype, "bwd " + what)
        # deterministic: a second launch is bitwise equal
        gx2 = torch.empty_like(gx)
        F.upsample2d_bwd(gy.to(DEV), gx2, mode, ac, r)
        assert torch.equal(gx, gx2), what
        # accumulate = 1
        acc = x.to(DEV)
        F.upsample2d_bwd(gy.to(DEV), acc, mode, ac, r, accumulate=True)
        _close(acc, x.double() + ref, dtype, "bwd+acc " + what)


@pytest.mark.parametrize("r", SCALES)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_backward_is_the_adjoint_of_forward(mode, ac, r):
    """<Up x, g> = <x, Up^T g>, both sides in fp64 from the fp32 kernels' own
    outputs.  Each kernel output carries a few fp32 roundings (<= 1e-6 of the
    magnitudes summed), so the two sides agree far inside 2e-5 |Up x| |g|; a
    border rule that differs between the two kernels shows at >= 1e-3."""
    for i, (planes, h, w, _) in enumerate(_cases()):
        x, gy, _ = _data(planes, h, w, r, torch.float32, 300 + i)
        y = F.upsample2d(x.to(DEV), torch.empty(gy.shape, device=DEV), mode, ac, r)
        gx = F.upsample2d_bwd(gy.to(DEV), torch.empty(x.shape, device=DEV), mode, ac, r)
        lhs = (y.cpu().double() * gy.double()).sum().item()
        rhs = (x.double() * gx.cpu().double()).sum().item()
        scale = y.cpu().double().norm().item() * gy.double().norm().item()
        assert abs(lhs - rhs) <= 2e-5 * scale, (mode, ac, r, planes, h, w, lhs, rhs)


def test_offsets_past_2_to_31():
    """An output of more than 2^31 elements (bf16, 4.3 GB): the last plane's
    flat offsets do not fit 32 bits."""
    planes, h, w, r = 129, 1024, 1024, 4
    assert planes * h * r * w * r > 2 ** 31
    g = torch.Generator().manual_seed(7)
    x = torch.randn((planes, h, w), generator=g).to(torch.bfloat16)
    y = torch.empty((planes, h * r, w * r), dtype=torch.bfloat16, device=DEV)
    F.upsample2d(x.to(DEV), y, "bilinear", False, r)
    for p in (0, planes - 1):
        ref = _ref(x[p][None, None], r, "bilinear", False)[0, 0]
        _close(y[p], ref, torch.bfloat16, f"plane {p}")
    gx = torch.empty((planes, h, w), dtype=torch.bfloat16, device=DEV)
    F.upsample2d_bwd(y, gx, "bilinear", False, r)
    yl = y[planes - 1].cpu()[None, None]
    _close(gx[planes - 1], _ref_bwd(yl, h, w, r, "bilinear", False)[0, 0], torch.bfloat16, "bwd last plane")


def test_functional_rejects_bad_arguments():
    x = torch.zeros((1, 1, 4, 4), device=DEV)
    with pytest.raises(ValueError):
        F.upsample2d(x, torch.zeros((1, 1, 8, 9), device=DEV), "bilinear", False, 2)
    with pytest.raises(TypeError):
        F.upsample2d(x, torch.zeros((1, 1, 8, 8), device=DEV, dtype=torch.bfloat16), "bilinear", False, 2)
    with pytest.raises(ValueError):
        F.upsample2d(x.transpose(2, 3)[..., :2], torch.zeros((1, 1, 8, 4), device=DEV), "bilinear", False, 2)
    with pytest.raises(KeyError):
        F.upsample2d(x, torch.zeros((1, 1, 8, 8), device=DEV), "nearest", False, 2)
    with pytest.raises(RuntimeError, match=r"upsample2d_fwd failed \(code 1\)"):  # VSRK_ERR_INVALID, nothing launched
        F.upsample2d(x, torch.zeros((1, 1, 0, 0), device=DEV), "bilinear", False, 0)


@pytest.mark.parametrize("mode,ac", [("bilinear", False), ("bicubic", True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_matches_functional(mode, ac, dtype):
    """torch.ops.vsrk.upsample2d: forward and .backward() are the functional
    calls (bitwise), on NCHW tensors."""
    r = 3
    x, gy, _ = _data((2, 3), 5, 7, r, dtype, 400)
    xd = x.to(DEV).requires_grad_(True)
    y = torch.ops.vsrk.upsample2d(xd, r, mode, ac)
    assert y.shape == (2, 3, 15, 21) and y.dtype == dtype
    assert torch.equal(y.detach(), F.upsample2d(x.to(DEV), torch.empty_like(y), mode, ac, r))
    y.backward(gy.to(DEV))
    assert torch.equal(xd.grad, F.upsample2d_bwd(gy.to(DEV), torch.empty_like(xd), mode, ac, r))
    _close(y, _ref(x, r, mode, ac), dtype, "op fwd")
    _close(xd.grad, _ref_bwd(gy, 5, 7, r, mode, ac), dtype, "op bwd")


def test_op_fake_and_opcheck():
    x = torch.randn((1, 2, 3, 4), device=DEV, requires_grad=True)
    torch.library.opcheck(torch.ops.vsrk.upsample2d.default, (x, 2, "bilinear", False),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


def test_swap_modules_converts_supported_upsample():
    net = nn.Sequential()
    net.add_module("bl", nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
    net.add_module("bc", nn.Upsample(scale_factor=(3, 3), mode="bicubic", align_corners=True))
    net.add_module("nearest", nn.Upsample(scale_factor=2, mode="nearest"))
    net.add_module("tri", nn.Upsample(scale_factor=2, mode="trilinear"))
    net.add_module("size", nn.Upsample(size=(8, 8), mode="bilinear"))
    net.add_module("frac", nn.Upsample(scale_factor=2.5, mode="bilinear"))
    net.add_module("uneven", nn.Upsample(scale_factor=(2, 3), mode="bicubic"))
    modules.swap_modules(net)
    assert type(net.bl) is modules.HipUpsample and type(net.bc) is modules.HipUpsample
    for name in ("nearest", "tri", "size", "frac", "uneven"):
        assert type(getattr(net, name)) is nn.Upsample, name
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 5, 7), generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = net.bc(net.bl(xd))
    ref = _ref(_ref(x, 2, "bilinear", False).float(), 3, "bicubic", True)
    _close(y, ref, torch.float32, "bl -> bc")
    y.sum().backward()
    x64 = x.double().requires_grad_(True)
    Fn.interpolate(Fn.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=False), scale_factor=3,
                   mode="bicubic", align_corners=True).sum().backward()
    _close(xd.grad, x64.grad, torch.float32, "bl -> bc grad")
    # a 3-D or 5-D input is nn.Upsample's own business
    assert type(modules.swap_modules(nn.Upsample(scale_factor=2, mode="bilinear"))) is modules.HipUpsample
