"""The DCN sampling kernels on channels-last views (vsrk_dcn_view_* in
csrc/dcn.hip): columns, the gradient of the raw conv_offset_mask output `om`
(offsets and mask logits) and the input scatter, against fp64 autograd through
oracle/dcn_ref.py fed the decoded planes (chunk(3), cat(o1, o2), sigmoid:
deform_conv.py:261-300).

Bounds, relative to max|ref|: fp32 2e-5, fp16 2e-3, bf16
1.5e-2; x and the column gradient are rounded to the storage type first, om
stays fp32.  For fp32 the kernels are also compared, at the same bound, with
the NCHW-plane kernels vsrk_dcn_im2col / _coord_grad / _col2im.

Offsets: all zero (the integer-position branch; no offset gradient is checked
there, the interpolation's derivative jumps at integers), sub-pixel, and wide
enough to leave the image on every side and to land between -1 and 0 and
between H - 1 and H.  Where gradients are checked every sampling position keeps
0.1 px from every integer (the -1, H and W validity edges are integers too), and
that margin is asserted per sample.

Shapes cover C / G of 1 and 2 (one element per lane in every dtype), 4 (16-byte
chunks in fp32 only), 8 and more (chunks in every dtype), and more than one
workgroup.
"""
import ctypes as C

import pytest
import torch

from oracle.dcn_ref import modulated_deform_conv_ref
from vsr_amd import _native as N
from vsr_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 9
BOUND = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
MARGIN = 0.1

# (N, C, G, H, W)
SHAPES = [(1, 8, 1, 2, 3), (2, 16, 2, 5, 7), (3, 64, 8, 9, 10), (2, 8, 8, 4, 5), (1, 16, 8, 3, 4), (2, 64, 1, 6, 5),
          (1, 8, 2, 9, 10)]
KINDS = ["zero", "subpixel", "leaving"]


def _close(got, exp, dtype, what):
    err = (got.double().cpu() - exp).abs().max().item()
    tol = BOUND[dtype] * exp.abs().max().item()
    print(f"{what}: max|d| {err:.3e} bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _make_om(g, n, G, h, w, kind):
    """The raw conv_offset_mask output (n, h, w, 3 G K) fp32: offsets with every
    fraction in [0.1, 0.9], mask logits of a few units."""
    if kind == "zero":
        off = torch.zeros((n, h, w, 2 * G * K))
    else:
        off = torch.randn((n, h, w, 2 * G * K), generator=g) * (0.6 if kind == "subpixel" else 4.0)
        fl = off.floor()
        off = fl + MARGIN + (1 - 2 * MARGIN) * (off - fl)
    logit = torch.randn((n, h, w, G * K), generator=g) * 2
    return torch.cat((off, logit), -1).float()


def _decode(om, G):
    """om (n, h, w, 3GK) -> the reference's NCHW offset (n, 2GK, h, w) and mask (n, GK, h, w)."""
    o1, o2, m = torch.chunk(om.permute(0, 3, 1, 2), 3, dim=1)
    return torch.cat((o1, o2), 1), torch.sigmoid(m)


def _positions(om, G, h, w):
    """Sampling positions (hs, ws), each (n, G, K, h, w), of a 3x3 / stride 1 / pad 1 geometry."""
    n = om.shape[0]
    off = om[..., :2 * G * K].double().view(n, h, w, G, K, 2).permute(0, 3, 4, 5, 1, 2)
    ki, kj = torch.arange(K) // 3, torch.arange(K) % 3
    hs = (torch.arange(h).view(1, 1, 1, h, 1) - 1 + ki.view(1, 1, K, 1, 1)) + off[:, :, :, 0]
    ws = (torch.arange(w).view(1, 1, 1, 1, w) - 1 + kj.view(1, 1, K, 1, 1)) + off[:, :, :, 1]
    return hs, ws


def _reference(x, om, gcols, G):
    """fp64: columns (n, 1, h, w, K*C), and the gradients of <columns, gcols>
    with respect to x (n, 1, h, w, C) and om."""
    n, _, h, w, c = x.shape
    x64 = x[:, 0].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    om64 = om.double().requires_grad_(True)
    offset, mask = _decode(om64, G)
    eye = torch.eye(c * K, dtype=torch.float64).view(c * K, c, 3, 3)  # output channel c*K + k = that column
    out = modulated_deform_conv_ref(x64, offset.contiguous(), mask.contiguous(), eye, None, 1, 1, 1, G)
    cols = out.view(n, c, K, h, w).permute(0, 3, 4, 2, 1).reshape(n, 1, h, w, K * c)
    (cols * gcols.double()).sum().backward()
    return cols.detach(), x64.grad.permute(0, 2, 3, 1).unsqueeze(1), om64.grad.unsqueeze(1)


def _run(x, om, gcols, G, dtype):
    n, _, h, w, c = x.shape
    xd, od, gd = x.to(DEV), om.unsqueeze(1).to(DEV), gcols.to(DEV)
    geo, ho, wo = F.dcn_geometry(xd, deformable_groups=G)
    assert (ho, wo) == (h, w)
    cols = torch.full((n, 1, h, w, K * c), float("nan"), dtype=dtype, device=DEV)
    assert F.dcn_view_im2col(geo, xd, od, cols) is cols
    gom = torch.full((n, 1, h, w, 3 * G * K), float("nan"), device=DEV)
    F.dcn_view_coord_grad(geo, xd, gd, od, gom)
    gom2 = torch.empty_like(gom)
    F.dcn_view_coord_grad(geo, xd, gd, od, gom2)
    assert torch.equal(gom, gom2)  # fixed order
    gx = torch.zeros((n, 1, h, w, c), device=DEV)
    F.dcn_view_col2im(geo, gd, od, gx)
    return geo, cols, gom, gx


def _plane_kernels(geo, x, om, gcols, G, modulated=True):
    """The fp32 NCHW-plane entry points on the decoded planes, in the view kernels' layouts; without
    `modulated` as DCNv1 (mask and grad_mask NULL), the gradient then that of the offsets alone."""
    lib = N.load()
    n, _, h, w, c = x.shape
    offset, mask = (t.contiguous().to(DEV) for t in _decode(om, G))
    if not modulated:
        mask = None
    xd, gd = x.to(DEV), gcols.to(DEV)
    sp = N.stream_ptr(xd.device)
    cols = torch.empty((n, 1, h, w, K * c), device=DEV)
    N.check(lib.vsrk_dcn_im2col(geo, xd.data_ptr(), offset.data_ptr(), N.ptr(mask), cols.data_ptr(), sp), "im2col")
    goff, gmask = torch.empty_like(offset), torch.empty_like(mask) if modulated else None
    N.check(lib.vsrk_dcn_coord_grad(geo, xd.data_ptr(), gd.data_ptr(), offset.data_ptr(), N.ptr(mask),
                                    goff.data_ptr(), N.ptr(gmask), sp), "coord_grad")
    gx = torch.zeros_like(xd)
    N.check(lib.vsrk_dcn_col2im(geo, gd.data_ptr(), offset.data_ptr(), N.ptr(mask), gx.data_ptr(), sp), "col2im")
    gom = torch.cat((goff, gmask * mask * (1 - mask)), 1) if modulated else goff
    return cols, gom.permute(0, 2, 3, 1).unsqueeze(1), gx


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_view_kernels_match_fp64(shape, kind):
    n, c, G, h, w = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 10, 100, 1000, 10000))) + KINDS.index(kind))
    om = _make_om(g, n, G, h, w, kind)
    hs, ws = _positions(om, G, h, w)
    if kind != "zero":
        for p in (hs, ws):  # the margin, per sample, on the fp32 values the kernels read
            assert ((p - p.round()).abs() >= MARGIN - 1e-5).all()
    if kind == "leaving" and h * w >= 20:
        # off the image on every side, and between the last corner and the validity edge on both ends
        assert (hs <= -1).any() and (hs >= h).any() and (ws <= -1).any() and (ws >= w).any()
        assert ((hs > -1) & (hs < 0)).any() and ((hs > h - 1) & (hs < h)).any()
        assert ((ws > -1) & (ws < 0)).any() and ((ws > w - 1) & (ws < w)).any()
    x0 = torch.randn((n, 1, h, w, c), generator=g)
    g0 = torch.randn((n, 1, h, w, K * c), generator=g)
    for dtype in BOUND:
        x, gcols = x0.to(dtype), g0.to(dtype)
        cols_r, gx_r, gom_r = _reference(x, om, gcols, G)
        geo, cols, gom, gx = _run(x, om, gcols, G, dtype)
        what = f"{dtype} {shape} {kind}"
        _close(cols, cols_r, dtype, "cols " + what)
        _close(gx, gx_r, dtype, "gx " + what)
        if kind == "zero":
            _close(gom[..., 2 * G * K:], gom_r[..., 2 * G * K:], dtype, "gom logits " + what)
        else:
            _close(gom, gom_r, dtype, "gom " + what)
            # each part against its own scale too
            _close(gom[..., :2 * G * K], gom_r[..., :2 * G * K], dtype, "gom offsets " + what)
            _close(gom[..., 2 * G * K:], gom_r[..., 2 * G * K:], dtype, "gom logits " + what)
        if dtype == torch.float32 and (c // G) % 4 == 0:  # the plane kernels need C / G % 4 == 0
            pc, pg, px = _plane_kernels(geo, x, om, gcols, G)
            _close(cols, pc.double().cpu(), dtype, "cols vs planes " + what)
            _close(gx, px.double().cpu(), dtype, "gx vs planes " + what)
            part = slice(2 * G * K, None) if kind == "zero" else slice(None)
            _close(gom[..., part], pg[..., part].double().cpu(), dtype, "gom vs planes " + what)


@pytest.mark.parametrize("shape", [(2, 8, 2, 4, 5), (1, 16, 1, 2, 3)], ids=lambda s: "x".join(map(str, s)))
def test_plane_and_view_entry_points_run_one_core(shape):
    """One sampling core behind two sample sources.  Mask logits of +20 make the view path's modulation
    exactly 1 in fp32 (1 + expf(-20) rounds to 1), which is what the plane path takes for a NULL mask (DCNv1):
    both then do the same arithmetic on the same numbers, so the columns and the offset gradient are equal bit
    for bit and the logit gradient, vm * (1 * (1 - 1)), is exactly zero.  The atomic input scatter is compared
    at the fp32 bound.  C / G = 4 puts one fp32 chunk in each deformable group (and 720 lanes in more than one
    workgroup); 2 x 3 is the smallest map on which all nine taps leave the image."""
    n, c, G, h, w = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 10, 100, 1000, 10000))))
    om = _make_om(g, n, G, h, w, "leaving")
    om[..., 2 * G * K:] = 20.0
    for p in _positions(om, G, h, w):  # the margin, per sample, on the fp32 values the kernels read
        assert ((p - p.round()).abs() >= MARGIN - 1e-5).all()
    x = torch.randn((n, 1, h, w, c), generator=g)
    gcols = torch.randn((n, 1, h, w, K * c), generator=g)
    geo, cols, gom, gx = _run(x, om, gcols, G, torch.float32)
    pc, pg, px = _plane_kernels(geo, x, om, gcols, G, modulated=False)
    assert torch.equal(cols, pc)
    assert torch.equal(gom[..., :2 * G * K], pg)
    assert (gom[..., 2 * G * K:] == 0).all()
    _close(gx, px.double().cpu(), torch.float32, f"gx vs planes {shape}")


@pytest.mark.parametrize("off", [8, 3])
@pytest.mark.parametrize("dtype", list(BOUND))
def test_view_kernels_on_channel_slices(dtype, off):
    """x, the columns and their gradient as channel slices of wider buffers, 16-byte aligned or not:
    same results, the columns' neighbours untouched."""
    n, c, G, h, w = 2, 16, 2, 4, 5
    g = torch.Generator().manual_seed(11)
    om = _make_om(g, n, G, h, w, "leaving")
    x = torch.randn((n, 1, h, w, c), generator=g).to(dtype)
    gcols = torch.randn((n, 1, h, w, K * c), generator=g).to(dtype)
    cols_r, gx_r, gom_r = _reference(x, om, gcols, G)

    def sliced(t, fill=9.0):
        wide = torch.full((*t.shape[:-1], off + t.shape[-1] + 5), fill, dtype=t.dtype, device=DEV)
        v = wide[..., off:off + t.shape[-1]]
        v.copy_(t)
        return wide, v

    (_, xv), (_, gv), (_, ov) = sliced(x), sliced(gcols), sliced(om.unsqueeze(1))
    wide_c, cols = sliced(torch.zeros((n, 1, h, w, K * c), dtype=dtype))
    wide_g, gom = sliced(torch.zeros((n, 1, h, w, 3 * G * K)))
    geo, _, _ = F.dcn_geometry(xv, deformable_groups=G)
    F.dcn_view_im2col(geo, xv, ov, cols)
    F.dcn_view_coord_grad(geo, xv, gv, ov, gom)
    gx = F.dcn_view_col2im(geo, gv, ov, torch.zeros((n, 1, h, w, c), device=DEV))
    _close(cols, cols_r, dtype, "cols")
    _close(gom, gom_r, dtype, "gom")
    _close(gx, gx_r, dtype, "gx")
    for wide, width in ((wide_c, K * c), (wide_g, 3 * G * K)):
        assert (wide[..., :off] == 9.0).all() and (wide[..., off + width:] == 9.0).all()


def test_bad_arguments():
    x = torch.zeros((1, 1, 4, 5, 8), device=DEV)
    om = torch.zeros((1, 1, 4, 5, 27), device=DEV)
    cols = torch.zeros((1, 1, 4, 5, 72), device=DEV)
    geo, _, _ = F.dcn_geometry(x)
    with pytest.raises(RuntimeError, match=r"dcn_view_im2col failed \(code 1\).*om is"):
        F.dcn_view_im2col(geo, x, om[..., :18], cols)
    with pytest.raises(RuntimeError, match=r"dcn_view_im2col failed \(code 1\).*om has dtype"):
        F.dcn_view_im2col(geo, x, om.half(), cols)
    with pytest.raises(RuntimeError, match=r"dcn_view_im2col failed \(code 1\).*x has dtype"):
        F.dcn_view_im2col(geo, x.half(), om, cols)
    bad = (C.c_int32 * 15)(*geo)
    bad[4] = 3  # Ho
    with pytest.raises(RuntimeError, match=r"dcn_view_im2col failed \(code 1\).*does not follow"):
        F.dcn_view_im2col(bad, x, om, cols)
    with pytest.raises(ValueError, match="grad_x"):
        F.dcn_view_col2im(geo, cols, om, torch.zeros((1, 1, 4, 5, 8), dtype=torch.float16, device=DEV))
