"""vsrk_flow_warp_fwd / _bwd (csrc/warp.hip) against F.grid_sample on the CPU
in fp64, on the reference STN's mesh (float32 of np.linspace(-1, 1, size),
frvsr_net.py:212-213,228-240), through vsr_amd.functional,
torch.ops.vsrk.flow_warp and modules.STN.

Bounds, relative to max|ref|: fp32 2e-5 (the project's kernel-against-fp64
figure, as for Bicubic); a 16-bit image adds half an ulp of its type at
max|ref| for the one output rounding (the inputs are rounded first).  The
flow gradient is held to rel-L2 1e-5 in fp32 on positions drawn at least
0.1 px from every kink of the bilinear surface, which the test asserts on
the CPU for every sample.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F
from vsr_amd import modules

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 1, 6), (1, 1, 6, 1), (2, 3, 5, 7), (1, 1, 8, 16), (1, 2, 33, 70)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
PADS = ["zeros", "border"]
FLOWS = ["zero", "subpixel", "leaving"]


def _mesh(h, w):
    """The reference's mesh (h, w, 2), x first, as its float32 tensor."""
    my, mx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    return torch.tensor(np.stack([mx, my], -1), dtype=torch.float32)


def _grid64(u, v):
    h, w = u.shape[-2:]
    return _mesh(h, w).double()[None] + torch.stack([u, v], -1).double()


def _ref(img, u, v, pad, ac):
    return Fn.grid_sample(img.double(), _grid64(u, v), mode="bilinear", padding_mode=pad, align_corners=ac)


def _tol(ref, dtype):
    m = ref.abs().max().item()
    tol = 2e-5 * m
    if dtype != torch.float32 and m > 0:
        tol += 0.5 * torch.finfo(dtype).eps * 2.0 ** math.floor(math.log2(m))
    return tol


def _cl(x, dtype):
    """(N, C, H, W) CPU -> channels-last (N, 1, H, W, C) device tensor of dtype."""
    v = x.to(dtype).permute(0, 2, 3, 1).unsqueeze(1)
    return torch.empty(v.shape, dtype=v.dtype).copy_(v).to(DEV)  # (.contiguous() keeps odd strides on 1-sized axes)


def _nchw(v):
    return v[:, 0].permute(0, 3, 1, 2).cpu()


def _flow(kind, n, h, w, g):
    if kind == "zero":
        return torch.zeros((n, h, w)), torch.zeros((n, h, w))
    if kind == "subpixel":  # within +-0.8 px (align_corners=False: 2 / size per pixel)
        return ((torch.rand((n, h, w), generator=g) - 0.5) * 1.6 * 2 / w,
                (torch.rand((n, h, w), generator=g) - 0.5) * 1.6 * 2 / h)
    # normalised targets spread over [-1 - 6/size, 1 + 6/size]: 3.5 px past either edge with
    # align_corners=False; the first samples are pinned to the four extremes
    m = _mesh(h, w)
    tx = (torch.rand((n, h, w), generator=g) * 2 - 1) * (1 + 6 / w)
    ty = (torch.rand((n, h, w), generator=g) * 2 - 1) * (1 + 6 / h)
    fx, fy = tx.view(n, -1), ty.view(n, -1)
    fx[:, 0], fx[:, 1] = -(1 + 6 / w), 1 + 6 / w
    fy[:, 2], fy[:, 3] = -(1 + 6 / h), 1 + 6 / h
    return tx - m[..., 0], ty - m[..., 1]


def _pixels(u, v, ac):
    """fp64 pixel coordinates (x, y) the kernel is asked to sample."""
    g = _grid64(u, v)
    h, w = u.shape[-2:]
    if ac:
        return (g[..., 0] + 1) / 2 * (w - 1), (g[..., 1] + 1) / 2 * (h - 1)
    return ((g[..., 0] + 1) * w - 1) / 2, ((g[..., 1] + 1) * h - 1) / 2


def _warp(img, u, v, pad, ac, dtype):
    iv = _cl(img, dtype)
    flow = torch.stack([u, v], 1).contiguous().to(DEV)
    out = torch.full(iv.shape, float("nan"), dtype=dtype, device=DEV)
    assert F.flow_warp(iv, flow, out, pad, ac) is out
    return _nchw(out)


@pytest.mark.parametrize("kind", FLOWS)
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("pad", PADS)
def test_forward_matches_grid_sample(pad, ac, kind):
    for i, (n, c, h, w) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(100 + i)
        img0 = torch.randn((n, c, h, w), generator=g)
        u, v = _flow(kind, n, h, w, g)
        if kind == "leaving":
            px, py = _pixels(u, v, False)
            assert px.min() < -2 and px.max() > w + 1 and py.min() < -2 and py.max() > h + 1
        for dtype in DTYPES:
            img = img0.to(dtype)
            ref = _ref(img, u, v, pad, ac)
            got = _warp(img, u, v, pad, ac, dtype)
            assert not torch.isnan(got).any()
            err = (got.double() - ref).abs().max().item()
            tol = _tol(ref, dtype)
            print(f"{pad} ac={ac} {kind} {(n, c, h, w)} {dtype}: max|d| {err:.3e} bound {tol:.3e}")
            assert err <= tol, (pad, ac, kind, (n, c, h, w), dtype, err, tol)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("r", [2, 3, 4])
def test_space_to_depth_store(r, c):
    """s2d = r into a channel slice of a wider buffer: bitwise the unfused
    output rearranged on the host, neighbours untouched; for one channel the
    order is the reference's SpaceToDepth (= pixel_unshuffle)."""
    n, h, w, off, tail = 2, 3 * r, 2 * r, 3, 5
    g = torch.Generator().manual_seed(7 * r + c)
    img = torch.randn((n, c, h, w), generator=g)
    u, v = _flow("subpixel", n, h, w, g)
    for dtype in DTYPES:
        iv = _cl(img, dtype)
        flow = torch.stack([u, v], 1).contiguous().to(DEV)
        plain = F.flow_warp(iv, flow, torch.empty_like(iv), "border", False)
        buf = torch.full((n, 1, h // r, w // r, off + r * r * c + tail), 7.0, dtype=dtype, device=DEV)
        F.flow_warp(iv, flow, buf[..., off:off + r * r * c], "border", False, s2d=r)
        want = plain.view(n, h // r, r, w // r, r, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 1, h // r, w // r, r * r * c)
        assert torch.equal(buf[..., off:off + r * r * c], want), (r, c, dtype)
        assert (buf[..., :off] == 7.0).all() and (buf[..., off + r * r * c:] == 7.0).all()
        if c == 1:
            ref_order = Fn.pixel_unshuffle(plain[:, 0].permute(0, 3, 1, 2).float(), r)
            assert torch.equal(_nchw(buf[..., off:off + r * r]).float(), ref_order.cpu())


def _targets(size, shape, g, outside):
    """Pixel coordinates with a fractional part in [0.1, 0.9]: inside the
    image, or -- where `outside` -- 0.1 to 2.5 px past either edge."""
    frac = 0.1 + 0.8 * torch.rand(shape, generator=g, dtype=torch.float64)
    inside = torch.floor(torch.rand(shape, generator=g, dtype=torch.float64) * max(size - 1, 1)) + frac
    k = torch.floor(torch.rand(shape, generator=g, dtype=torch.float64) * 3)
    off = k + torch.where(k == 2, 0.1 + 0.4 * torch.rand(shape, generator=g, dtype=torch.float64), frac)
    low = torch.rand(shape, generator=g) < 0.5
    out = torch.where(low, -off, size - 1 + off)
    return torch.where(outside | (size == 1), out, inside)


def _grad_case(n, c, h, w, ac, seed, share=0.25):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn((n, c, h, w), generator=g)
    gout = torch.randn((n, c, h, w), generator=g)
    px = _targets(w, (n, h, w), g, torch.rand((n, h, w), generator=g) < share)
    py = _targets(h, (n, h, w), g, torch.rand((n, h, w), generator=g) < share)
    m = _mesh(h, w).double()
    # align_corners=True puts every sample of a one-pixel axis at coordinate 0 whatever the flow (the
    # un-normalisation multiplies by size - 1 = 0): the flow there is arbitrary and its gradient exactly 0
    pinned = [ac and size == 1 for size in (w, h)]
    gx = px if pinned[0] else (2 * px / (w - 1) - 1 if ac else (2 * px + 1) / w - 1)
    gy = py if pinned[1] else (2 * py / (h - 1) - 1 if ac else (2 * py + 1) / h - 1)
    u, v = (gx - m[..., 0]).float(), (gy - m[..., 1]).float()
    # every sample, as the kernel will see it, keeps its distance from every
    # kink: the integers of [0, size-1], and -1 and size for 'zeros'
    ax, ay = _pixels(u, v, ac)
    for a, size, pin in ((ax, w, pinned[0]), (ay, h, pinned[1])):
        if pin:
            assert (a == 0).all()
            continue
        dist = (a - a.round().clamp(-1, size)).abs()
        assert (dist >= 1e-3).all(), (size, dist.min().item())
        assert a.numel() < 24 or ((a < 0) | (a > size - 1)).any()  # (a quarter of the targets, given enough)
    return img, gout, u, v


def _ref_grad(img, gout, u, v, pad, ac):
    grid = _grid64(u, v).requires_grad_(True)
    Fn.grid_sample(img.double(), grid, mode="bilinear", padding_mode=pad, align_corners=ac).backward(gout.double())
    return grid.grad.permute(0, 3, 1, 2)  # (n, 2, h, w): d/du, d/dv


GRAD_SHAPES = [(2, 3, 5, 7), (1, 1, 8, 16), (1, 2, 33, 70), (1, 1, 1, 6), (1, 2, 6, 1)]


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("pad", PADS)
def test_flow_gradient_matches_autograd(pad, ac):
    for i, (n, c, h, w) in enumerate(GRAD_SHAPES):
        img, gout, u, v = _grad_case(n, c, h, w, ac, 300 + i)
        ref = _ref_grad(img, gout, u, v, pad, ac)
        iv, gv = _cl(img, torch.float32), _cl(gout, torch.float32)
        flow = torch.stack([u, v], 1).contiguous().to(DEV)
        gf = torch.full((n, 2, h, w), float("nan"), device=DEV)
        assert F.flow_warp_bwd(iv, flow, gv, gf, pad, ac) is gf
        rel = ((gf.cpu().double() - ref).norm() / ref.norm()).item()
        print(f"{pad} ac={ac} {(n, c, h, w)}: rel-L2 {rel:.3e}")
        assert rel <= 1e-5, (pad, ac, (n, c, h, w), rel)
        for axis, size in ((0, w), (1, h)):  # a one-pixel axis under align_corners=True: exactly 0, as torch's
            if ac and size == 1:
                assert (gf[:, axis] == 0).all() and (ref[:, axis] == 0).all()
        if pad == "border":  # clipped positions carry an exact zero, as torch's do
            ax, ay = _pixels(u, v, ac)
            assert (gf[:, 0].cpu()[(ax <= 0) | (ax >= w - 1)] == 0).all()
            assert (gf[:, 1].cpu()[(ay <= 0) | (ay >= h - 1)] == 0).all()
        # bitwise reproducible
        gf2 = torch.empty_like(gf)
        F.flow_warp_bwd(iv, flow, gv, gf2, pad, ac)
        assert torch.equal(gf, gf2)
        # accumulate = 1 adds onto gflow
        base = torch.randn((n, 2, h, w), generator=torch.Generator().manual_seed(9))
        acc = base.to(DEV)
        F.flow_warp_bwd(iv, flow, gv, acc, pad, ac, accumulate=True)
        rel = ((acc.cpu().double() - (base.double() + ref)).norm() / (base.double() + ref).norm()).item()
        assert rel <= 1e-5, ("accumulate", rel)


def test_flow_gradient_through_space_to_depth():
    """gout in the s2d layout gives the gradient of the plain layout (bitwise)."""
    n, c, r = 2, 2, 2
    h, w = 3 * r, 4 * r
    img, gout, u, v = _grad_case(n, c, h, w, False, 500)
    iv, gv = _cl(img, torch.bfloat16), _cl(gout, torch.bfloat16)
    flow = torch.stack([u, v], 1).contiguous().to(DEV)
    plain = F.flow_warp_bwd(iv, flow, gv, torch.empty((n, 2, h, w), device=DEV), "border", False)
    gs = gv.view(n, h // r, r, w // r, r, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 1, h // r, w // r, r * r * c)
    fused = F.flow_warp_bwd(iv, flow, gs.contiguous(), torch.empty((n, 2, h, w), device=DEV), "border", False, s2d=r)
    assert torch.equal(plain, fused)


def _coarse_flow(n, h, w, r, seed):
    """A coarse flow (n, 2, h/r, w/r) of a few HR pixels whose fp64
    interpolation puts every HR sample at least 1e-4 px from every integer of
    [0, size-1] (the kernel interpolates in fp32: positions move by ~1e-6 px,
    which then crosses no cell border); the first seed from `seed` that does."""
    for s in range(seed, seed + 200):
        g = torch.Generator().manual_seed(s)
        lo = torch.stack(_flow("subpixel", n, h // r, w // r, g), 1) / r * 3
        hi64 = Fn.interpolate(lo.double(), scale_factor=r, mode="bilinear", align_corners=True)
        ax, ay = _pixels(hi64[:, 0], hi64[:, 1], False)
        if all(((a - a.round().clamp(0, size - 1)).abs() >= 1e-4).all() for a, size in ((ax, w), (ay, h))):
            return lo, hi64, g
    raise AssertionError("no seed keeps the samples off the cell borders")


@pytest.mark.parametrize("r", [2, 4])
def test_coarse_flow_is_interpolated_in_the_kernel(r):
    """flow_up = r: the positions come from the flow's bilinear x r,
    align_corners=True interpolation, done per pixel in the kernel.  Forward
    against fp64 interpolate -> grid_sample at the forward bounds; the flow
    gradient (of the interpolated flow) against fp64 autograd at rel-L2 1e-5."""
    for i, (n, c, h, w) in enumerate([(2, 3, 3 * r, 2 * r), (1, 1, r, r), (1, 2, 8 * r, 18 * r)]):
        lo, hi64, g = _coarse_flow(n, h, w, r, 700 + 1000 * r + 200 * i)
        img0 = torch.randn((n, c, h, w), generator=g)
        gout = torch.randn((n, c, h, w), generator=g)
        lod = lo.contiguous().to(DEV)
        for dtype in DTYPES:
            img = img0.to(dtype)
            iv = _cl(img, dtype)
            fused = F.flow_warp(iv, lod, torch.empty_like(iv), "border", False, flow_up=r)
            grid = (_mesh(h, w).double()[None] + hi64.permute(0, 2, 3, 1)).requires_grad_(True)
            ref = Fn.grid_sample(img.double(), grid, mode="bilinear", padding_mode="border", align_corners=False)
            err = (_nchw(fused).double() - ref.detach()).abs().max().item()
            print(f"flow_up={r} {(n, c, h, w)} {dtype}: max|d| {err:.3e} bound {_tol(ref.detach(), dtype):.3e}")
            assert err <= _tol(ref.detach(), dtype), (r, (n, c, h, w), dtype, err)
            if dtype == torch.float32:
                ref.backward(gout.double())
                want = grid.grad.permute(0, 3, 1, 2)
                gf = F.flow_warp_bwd(iv, lod, _cl(gout, dtype), torch.empty((n, 2, h, w), device=DEV), "border", False,
                                     flow_up=r)
                rel = ((gf.cpu().double() - want).norm() / want.norm()).item()
                print(f"flow_up={r} {(n, c, h, w)}: flow gradient rel-L2 {rel:.3e}")
                assert rel <= 1e-5, (r, (n, c, h, w), rel)
    with pytest.raises(ValueError, match="flow_up"):
        F.flow_warp(iv, lod, torch.empty_like(iv), "border", False, flow_up=r + 1)


def test_two_launches_are_bitwise_equal():
    n, c, h, w = 1, 2, 33, 70
    g = torch.Generator().manual_seed(11)
    img = torch.randn((n, c, h, w), generator=g)
    u, v = _flow("leaving", n, h, w, g)
    for dtype in DTYPES:
        a = _warp(img, u, v, "zeros", False, dtype)
        b = _warp(img, u, v, "zeros", False, dtype)
        assert torch.equal(a, b)


def test_bad_arguments():
    iv = torch.zeros((1, 1, 4, 6, 8), device=DEV)
    flow = torch.zeros((1, 2, 4, 6), device=DEV)
    with pytest.raises(RuntimeError, match=r"flow_warp_fwd failed \(code 1\).*shape mismatch"):  # VSRK_ERR_INVALID
        F.flow_warp(iv, flow, torch.zeros((1, 1, 4, 5, 8), device=DEV), "border", False)
    with pytest.raises(RuntimeError, match=r"flow_warp_fwd failed \(code 1\).*multiple of s2d"):
        F.flow_warp(iv, flow, torch.zeros((1, 1, 4, 6, 8), device=DEV), "border", False, s2d=4)
    with pytest.raises(RuntimeError, match=r"flow_warp_fwd failed \(code 1\).*dtype mismatch"):
        F.flow_warp(iv, flow, torch.zeros((1, 1, 4, 6, 8), device=DEV, dtype=torch.bfloat16), "border", False)
    with pytest.raises(RuntimeError, match=r"flow_warp_bwd failed \(code 1\).*shape mismatch"):
        F.flow_warp_bwd(iv, flow, torch.zeros((1, 1, 2, 3, 8), device=DEV), torch.zeros_like(flow), "zeros", True)
    with pytest.raises(ValueError, match="flow must be"):
        F.flow_warp(iv, torch.zeros((1, 2, 4, 5), device=DEV), torch.zeros_like(iv), "border", False)
    with pytest.raises(TypeError, match="fp32"):
        F.flow_warp(iv, flow.half(), torch.zeros_like(iv), "border", False)
    with pytest.raises(KeyError):
        F.flow_warp(iv, flow, torch.zeros_like(iv), "reflection", False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_op_and_stn_match_functional(dtype):
    """torch.ops.vsrk.flow_warp on NCHW tensors is the functional call
    (bitwise), its backward the flow-gradient kernel; modules.STN is the op
    with the reference's defaults."""
    n, c, h, w = 2, 3, 5, 7
    img, gout, u, v = _grad_case(n, c, h, w, False, 600)
    img, gout = img.to(dtype), gout.to(dtype)
    ud, vd = u.to(DEV).requires_grad_(True), v.to(DEV).requires_grad_(True)
    y = torch.ops.vsrk.flow_warp(img.to(DEV), ud, vd, "border", False)
    assert y.shape == (n, c, h, w) and y.dtype == dtype
    assert torch.equal(y.detach().cpu(), _warp(img, u, v, "border", False, dtype))
    y.backward(gout.to(DEV))
    gf = F.flow_warp_bwd(_cl(img, dtype), torch.stack([u, v], 1).contiguous().to(DEV), _cl(gout, dtype),
                         torch.empty((n, 2, h, w), device=DEV), "border", False)
    assert torch.equal(ud.grad, gf[:, 0]) and torch.equal(vd.grad, gf[:, 1])
    if dtype == torch.float32:
        ref = _ref_grad(img, gout, u, v, "border", False)
        assert ((gf.cpu().double() - ref).norm() / ref.norm()).item() <= 1e-5
    stn = modules.STN(padding_mode="border")
    assert torch.equal(stn(img.to(DEV), ud.detach(), vd.detach()), y.detach())
    # normalize=True takes the flow in pixels
    pix = modules.STN(padding_mode="border", normalize=True)
    assert torch.equal(pix(img.to(DEV), ud.detach() * w / 2, vd.detach() * h / 2),
                       torch.ops.vsrk.flow_warp(img.to(DEV), ud.detach() * w / 2 / w * 2, vd.detach() * h / 2 / h * 2,
                                                "border", False))
    with pytest.raises(NotImplementedError, match="bilinear"):
        modules.STN(mode="nearest")(img.to(DEV), ud, vd)


def test_image_gradient_is_refused():
    img = torch.randn((1, 1, 4, 4), device=DEV, requires_grad=True)
    u = torch.zeros((1, 4, 4), device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="image"):
        torch.ops.vsrk.flow_warp(img, u, u, "border", False)


def test_op_fake_and_opcheck():
    img = torch.randn((1, 2, 3, 4), device=DEV)
    u = (torch.rand((1, 3, 4), device=DEV) - 0.5).requires_grad_(True)
    v = (torch.rand((1, 3, 4), device=DEV) - 0.5).requires_grad_(True)
    torch.library.opcheck(torch.ops.vsrk.flow_warp.default, (img, u, v, "border", False),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
