"""The channels-last pooling / resampling kernels (csrc/resample_cl.hip), tanh
(csrc/elementwise.hip) and the modules built on them, against torch on the
CPU.

A max-pool only selects, so its values and its routed gradients are compared
bitwise, for random inputs and for small integers with many exact ties (the
first maximum in row-major window order wins, as in torch's CPU kernel).
The bilinear kernels and tanh are held to test_upsample_gpu.py's bounds
against fp64, relative to max|ref|: fp32 2e-5, fp16 2e-3, bf16 1.5e-2 (the
16-bit inputs are rounded first).

Channel counts: 2 (one element per lane), 32 and 256 (16-byte chunks), 48
(chunks, not a power of two); 6 x 130 makes more than one workgroup; slices
of a wider buffer cover strided views with and without 16-byte alignment.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from vsr_amd import functional as F
from vsr_amd import modules

pytestmark = pytest.mark.gpu
DEV = "cuda"

BOUND = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
DTYPES = list(BOUND)
CHANNELS = [2, 32, 48, 256]
POOL_SIZES = [(2, 2), (5, 7), (8, 16), (6, 130)]


def _cl(x, dtype=None):
    """(N, C, H, W) CPU -> channels-last (N, 1, H, W, C) on the device."""
    x = x if dtype is None else x.to(dtype)
    v = x.permute(0, 2, 3, 1).unsqueeze(1)
    return torch.empty(v.shape, dtype=v.dtype).copy_(v).to(DEV)  # (.contiguous() keeps odd strides on 1-sized axes)


def _nchw(v):
    return v[:, 0].permute(0, 3, 1, 2).cpu()


def _close(got, exp, dtype, what):
    err = (got.double() - exp).abs().max().item()
    tol = BOUND[dtype] * exp.abs().max().item()
    print(f"{what}: max|d| {err:.3e} bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _pool_ref(x, gy):
    """torch's CPU max-pool of the (already rounded) values, in fp32: (y, gx)."""
    xr = x.detach().float().clone().requires_grad_(True)
    y = Fn.max_pool2d(xr, 2)
    y.backward(gy.float())
    return y.detach(), xr.grad


def _pool_check(x, gy, dtype, what, view=None):
    y_ref, gx_ref = _pool_ref(x, gy)
    n, c, h, w = x.shape
    xv, gv = _cl(x), _cl(gy)
    if view is not None:
        xv, gv = view(xv), view(gv)
    y = torch.full((n, 1, h // 2, w // 2, c), float("nan"), dtype=dtype, device=DEV)
    assert F.max_pool2x2(xv, y) is y
    assert torch.equal(_nchw(y).float(), y_ref), what
    gx = torch.full((n, 1, h, w, c), float("nan"), dtype=dtype, device=DEV)
    assert F.max_pool2x2_bwd(xv, gv, gx) is gx
    assert torch.equal(_nchw(gx).float(), gx_ref), what


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_max_pool_matches_torch_bitwise(dtype, c):
    for i, (h, w) in enumerate(POOL_SIZES):
        g = torch.Generator().manual_seed(10 * c + i)
        x = torch.randn((2, c, h, w), generator=g).to(dtype)
        gy = torch.randn((2, c, h // 2, w // 2), generator=g).to(dtype)
        _pool_check(x, gy, dtype, f"random {dtype} c={c} {h}x{w}")
        # small integers, many exact ties: the first maximum wins, forward and backward
        t = torch.randint(-1, 2, (2, c, h, w), generator=g).to(dtype)
        _pool_check(t, gy, dtype, f"ties {dtype} c={c} {h}x{w}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_pool_on_channel_slices(dtype):
    """Views into a wider buffer: an offset that keeps 16-byte alignment (the
    chunk path on strided pixels) and one that breaks it (one element per lane)."""
    g = torch.Generator().manual_seed(5)
    c, h, w = 32, 5, 7
    x = torch.randn((2, c, h, w), generator=g).to(dtype)
    gy = torch.randn((2, c, h // 2, w // 2), generator=g).to(dtype)
    for off in (8, 3):
        def view(t, off=off):
            wide = torch.full((*t.shape[:-1], off + c + 5), 9.0, dtype=t.dtype, device=DEV)
            wide[..., off:off + c] = t
            return wide[..., off:off + c]
        _pool_check(x, gy, dtype, f"slice at {off} {dtype}", view)


def _up_ref(x, r, ac):
    return Fn.interpolate(x.double(), scale_factor=r, mode="bilinear", align_corners=ac)


def _up_ref_bwd(gy, h, w, r, ac):
    x = torch.zeros((*gy.shape[:2], h, w), dtype=torch.float64, requires_grad=True)
    Fn.interpolate(x, scale_factor=r, mode="bilinear", align_corners=ac).backward(gy.double())
    return x.grad


UP_SIZES = [(1, 1), (2, 3), (5, 7), (8, 16)]


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("c", [2, 32, 48, 256])
def test_upsample_cl_forward_and_adjoint(c, r, ac):
    for i, (h, w) in enumerate(UP_SIZES):
        for dtype in DTYPES:
            g = torch.Generator().manual_seed(100 * c + i)
            x = torch.randn((2, c, h, w), generator=g).to(dtype)
            gy = torch.randn((2, c, h * r, w * r), generator=g).to(dtype)
            y0 = torch.randn((2, c, h * r, w * r), generator=g).to(dtype)
            what = f"c={c} r={r} ac={ac} {h}x{w} {dtype}"
            ref = _up_ref(x, r, ac)
            y = torch.full((2, 1, h * r, w * r, c), float("nan"), dtype=dtype, device=DEV)
            assert F.upsample_cl(_cl(x), y, r, ac) is y
            _close(_nchw(y), ref, dtype, "fwd " + what)
            acc = _cl(y0)
            F.upsample_cl(_cl(x), acc, r, ac, accumulate=True)
            _close(_nchw(acc), y0.double() + ref, dtype, "fwd+acc " + what)
            ref_b = _up_ref_bwd(gy, h, w, r, ac)
            gx = torch.full((2, 1, h, w, c), float("nan"), dtype=dtype, device=DEV)
            assert F.upsample_cl_bwd(_cl(gy), gx, r, ac) is gx
            _close(_nchw(gx), ref_b, dtype, "bwd " + what)
            gx2 = torch.empty_like(gx)
            F.upsample_cl_bwd(_cl(gy), gx2, r, ac)
            assert torch.equal(gx, gx2), what  # a fixed-order gather
            accb = _cl(x)
            F.upsample_cl_bwd(_cl(gy), accb, r, ac, accumulate=True)
            _close(_nchw(accb), x.double() + ref_b, dtype, "bwd+acc " + what)
            if dtype == torch.float32:
                # <Up x, g> = <x, Up^T g> from the kernels' own outputs, in fp64
                lhs = (_nchw(y).double() * gy.double()).sum().item()
                rhs = (x.double() * _nchw(gx).double()).sum().item()
                scale = _nchw(y).double().norm().item() * gy.double().norm().item()
                assert abs(lhs - rhs) <= 2e-5 * scale, (what, lhs, rhs)


def test_upsample_cl_agrees_with_the_plane_kernel():
    """One tap routine serves both layouts: same taps and weights, so the fp32
    results differ by the rounding of the blend alone (a few ulp of max|y|)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 32, 5, 7), generator=g)
    for r, ac in ((2, False), (4, True)):
        y = F.upsample_cl(_cl(x), torch.empty((2, 1, 5 * r, 7 * r, 32), device=DEV), r, ac)
        p = F.upsample2d(x.to(DEV), torch.empty((2, 32, 5 * r, 7 * r), device=DEV), "bilinear", ac, r)
        assert (_nchw(y) - p.cpu()).abs().max().item() <= 4 * 2.0 ** -24 * p.abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tanh_forward_and_backward(dtype):
    g = torch.Generator().manual_seed(1)
    for shape in ((2, 2, 5, 7), (1, 32, 3, 4)):
        x = (torch.randn(shape, generator=g) * 2).to(dtype)
        dy = torch.randn(shape, generator=g).to(dtype)
        y = F.tanh(_cl(x), torch.empty_like(_cl(x)))
        _close(_nchw(y), torch.tanh(x.double()), dtype, f"tanh {dtype}")
        yr = _nchw(y)  # the backward takes the rounded forward output
        dx = F.tanh_bwd(y, _cl(dy), torch.empty_like(y))
        _close(_nchw(dx), dy.double() * (1 - yr.double() ** 2), dtype, f"tanh_bwd {dtype}")
    # in place, on a 2-channel slice of 8-channel storage (FNet's flow head)
    wide = torch.full((1, 1, 4, 4, 8), 5.0, device=DEV)
    v = wide[..., :2]
    v.copy_(torch.linspace(-3, 3, 32, device=DEV).view(1, 1, 4, 4, 2))
    want = torch.tanh(v.double())
    F.tanh(v, v)
    assert (v.double() - want).abs().max().item() <= 2e-5 and (wide[..., 2:] == 5.0).all()


def test_bad_arguments():
    x = torch.zeros((1, 1, 4, 6, 8), device=DEV)
    with pytest.raises(RuntimeError, match=r"max_pool2x2_fwd failed \(code 1\).*factor 2"):
        F.max_pool2x2(x, torch.zeros((1, 1, 2, 2, 8), device=DEV))
    with pytest.raises(RuntimeError, match=r"max_pool2x2_fwd failed \(code 1\).*channel mismatch"):
        F.max_pool2x2(x, torch.zeros((1, 1, 2, 3, 16), device=DEV))
    with pytest.raises(RuntimeError, match=r"max_pool2x2_bwd failed \(code 1\).*does not match"):
        F.max_pool2x2_bwd(x, torch.zeros((1, 1, 2, 3, 8), device=DEV), torch.zeros((1, 1, 4, 5, 8), device=DEV))
    with pytest.raises(RuntimeError, match=r"upsample_cl_fwd failed \(code 1\).*factor 2"):
        F.upsample_cl(x, torch.zeros((1, 1, 8, 13, 8), device=DEV), 2, False)
    with pytest.raises(RuntimeError, match=r"upsample_cl_bwd failed \(code 1\).*scale factor"):
        F.upsample_cl_bwd(x, x, 0, False)
    with pytest.raises(RuntimeError, match=r"tanh_fwd failed \(code 1\).*shape or dtype"):
        F.tanh(x, torch.zeros((1, 1, 4, 6, 4), device=DEV))


@pytest.mark.parametrize("dtype", DTYPES)
def test_max_pool_op_and_module(dtype):
    """torch.ops.vsrk.max_pool2x2 and HipMaxPool2d (through swap_modules) on
    NCHW tensors: torch's values and gradients, bitwise."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 5, 6), generator=g).to(dtype)
    gy = torch.randn((2, 3, 2, 3), generator=g).to(dtype)
    y_ref, gx_ref = _pool_ref(x, gy)
    net = modules.swap_modules(nn.Sequential(nn.MaxPool2d(2), nn.MaxPool2d(2, ceil_mode=True)))
    assert type(net[0]) is modules.HipMaxPool2d and type(net[1]) is nn.MaxPool2d
    xd = x.to(DEV).requires_grad_(True)
    y = net[0](xd)
    assert y.dtype == dtype and torch.equal(y.detach().cpu().float(), y_ref)
    y.backward(gy.to(DEV))
    assert torch.equal(xd.grad.cpu().float(), gx_ref)
    torch.library.opcheck(torch.ops.vsrk.max_pool2x2.default, (torch.randn((1, 2, 4, 4), device=DEV,
                                                                           requires_grad=True),),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


def test_deconv_with_output_padding_matches_torch():
    """nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1)
    (frvsr_net.py:84,86) as the 3x3 sub-pixel conv: 2h x 2w, fp64 torch's output
    and gradients at the op tests' 1e-4 relative L2."""
    torch.manual_seed(6)
    ref = nn.ConvTranspose2d(16, 16, 3, stride=2, padding=1, output_padding=1)
    hip = modules.swap_modules(copy.deepcopy(ref)).to(DEV)
    assert type(hip) is modules.HipConvTranspose2d
    ref = ref.double()
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2, 16, 5, 7), generator=g)
    G = torch.randn((2, 16, 10, 14), generator=g)

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double()
        return ((a - b).norm() / b.norm()).item()

    x64 = x.double().requires_grad_(True)
    o64 = ref(x64)
    (o64 * G.double()).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    o = hip(xd)
    assert o.shape == o64.shape
    (o * G.to(DEV)).sum().backward()
    assert rel(o, o64) <= 1e-4 and rel(xd.grad, x64.grad) <= 1e-4
    assert rel(hip.weight.grad, ref.weight.grad) <= 1e-4 and rel(hip.bias.grad, ref.bias.grad) <= 1e-4
