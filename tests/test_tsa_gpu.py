"""EDVR's TSA fusion kernels (csrc/tsa.hip) against torch on the CPU.

Temporal attention and the gated merge are held to the kernel bounds of
DESIGN.md section 4 against fp64, relative to max|ref|: fp32 2e-5, fp16 2e-3,
bf16 1.5e-2 (the 16-bit inputs are rounded first).  None of these kernels has
an atomic, so two launches agree bitwise.

The 3x3 stride-2 pool pair only selects (max) or sums nine fp32 terms in
row-major order and divides by 9 (avg), so its values are compared bitwise with
F.max_pool2d / F.avg_pool2d (3, 2, 1) run by torch on the CPU in the same
dtype, and so are the routed max gradients (torch sums them in the storage
type).  The avg gradient is summed in fp32 here and in the storage type by
torch: it is held to the bounds above against fp64.

Channel counts: 2 (one element per lane), 8 / 16 / 48 / 64 (16-byte chunks; 8
is one chunk of a 16-bit type, 48 not a power of two); 6 x 130 makes more than
one workgroup; slices of a wider buffer cover strided destinations with and
without 16-byte alignment.
"""
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

BOUND = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 1.5e-2}
DTYPES = list(BOUND)


def _close(got, exp, dtype, what):
    err = (got.double().cpu() - exp).abs().max().item()
    tol = BOUND[dtype] * exp.abs().max().item()
    print(f"{what}: max|d| {err:.3e} bound {tol:.3e}")
    assert err <= tol, (what, err, tol)


def _dev(t):
    """A CPU tensor on the device, contiguous whatever its 1-sized axes."""
    return torch.empty(t.shape, dtype=t.dtype).copy_(t).to(DEV)


def _slice_of(shape, dtype, off, fill=9.0):
    """A (..., c) view at channel `off` of a wider buffer filled with `fill`."""
    wide = torch.full((*shape[:-1], off + shape[-1] + 5), fill, dtype=dtype, device=DEV)
    return wide, wide[..., off:off + shape[-1]]


def _untouched(wide, off, c, fill=9.0):
    return bool((wide[..., :off] == fill).all() and (wide[..., off + c:] == fill).all())


# ---- temporal attention ----
def _tatt_ref(emb, ref, al, gout, b, n):
    """fp64 autograd of EDVR_arch.py:284-294 on channels-last tensors."""
    e, r, a = (t.double().clone().requires_grad_(True) for t in (emb, ref, al))
    h, w, c = emb.shape[2:]
    cor = (e.view(b, n, h, w, c) * r.view(b, 1, h, w, c)).sum(-1)
    prob = torch.sigmoid(cor)
    out = (a.view(b, n, h, w, c) * prob.unsqueeze(-1)).permute(0, 2, 3, 1, 4).reshape(b, 1, h, w, n * c)
    out.backward(gout.double())
    return out.detach(), prob.detach(), e.grad, r.grad, a.grad


TATT_CASES = [(1, 1, 1, 1), (2, 3, 2, 3), (2, 5, 5, 7), (1, 3, 5, 7)]  # (B, N, h, w)


@pytest.mark.parametrize("c", [8, 16, 24, 48, 64])  # 24 and 48: chunks per pixel no power of two, idle lanes in a group
@pytest.mark.parametrize("dtype", DTYPES)
def test_tatt_forward_and_backward(dtype, c):
    for i, (b, n, h, w) in enumerate(TATT_CASES):
        g = torch.Generator().manual_seed(100 * c + i)
        emb = (torch.randn((b * n, 1, h, w, c), generator=g) * 0.5).to(dtype)
        ref = (torch.randn((b, 1, h, w, c), generator=g) * 0.5).to(dtype)
        al = torch.randn((b * n, 1, h, w, c), generator=g).to(dtype)
        gout = torch.randn((b, 1, h, w, n * c), generator=g).to(dtype)
        out_r, prob_r, ge_r, gr_r, ga_r = _tatt_ref(emb, ref, al, gout, b, n)
        what = f"{dtype} c={c} B={b} N={n} {h}x{w}"

        ed, rd, ad, gd = _dev(emb), _dev(ref), _dev(al), _dev(gout)
        out = torch.full((b, 1, h, w, n * c), float("nan"), dtype=dtype, device=DEV)
        prob = torch.full((b, n, h, w), float("nan"), device=DEV)
        assert F.tsa_tatt(ed, rd, ad, out, prob) is out
        _close(out, out_r, dtype, "out " + what)
        _close(prob, prob_r, dtype, "prob " + what)
        ge, gr, ga = (torch.full(t.shape, float("nan"), dtype=dtype, device=DEV) for t in (ed, rd, ad))
        F.tsa_tatt_bwd(ed, rd, ad, prob, gd, ge, gr, ga)
        _close(ge, ge_r, dtype, "g_emb " + what)
        _close(gr, gr_r, dtype, "g_emb_ref " + what)
        _close(ga, ga_r, dtype, "g_aligned " + what)

        out2, prob2 = torch.empty_like(out), torch.empty_like(prob)
        F.tsa_tatt(ed, rd, ad, out2, prob2)
        ge2, gr2, ga2 = torch.empty_like(ge), torch.empty_like(gr), torch.empty_like(ga)
        F.tsa_tatt_bwd(ed, rd, ad, prob, gd, ge2, gr2, ga2)
        for p, q in ((out, out2), (prob, prob2), (ge, ge2), (gr, gr2), (ga, ga2)):
            assert torch.equal(p, q), what


@pytest.mark.parametrize("off", [8, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tatt_into_channel_slices(dtype, off):
    """Destinations that are channel slices of wider buffers, at an offset that
    keeps 16-byte alignment and at one that breaks it: same values, neighbours
    untouched."""
    b, n, h, w, c = 2, 3, 3, 5, 16
    g = torch.Generator().manual_seed(7)
    emb = (torch.randn((b * n, 1, h, w, c), generator=g) * 0.5).to(dtype)
    ref = (torch.randn((b, 1, h, w, c), generator=g) * 0.5).to(dtype)
    al = torch.randn((b * n, 1, h, w, c), generator=g).to(dtype)
    gout = torch.randn((b, 1, h, w, n * c), generator=g).to(dtype)
    out_r, _, ge_r, gr_r, ga_r = _tatt_ref(emb, ref, al, gout, b, n)
    ed, rd, ad = _dev(emb), _dev(ref), _dev(al)
    wide_o, out = _slice_of((b, 1, h, w, n * c), dtype, off)
    prob = torch.empty((b, n, h, w), device=DEV)
    F.tsa_tatt(ed, rd, ad, out, prob)
    _close(out, out_r, dtype, "out slice")
    assert _untouched(wide_o, off, n * c)
    wide_g, gd = _slice_of(gout.shape, dtype, off)
    gd.copy_(gout)
    (we, ge), (wr, gr), (wa, ga) = (_slice_of(t.shape, dtype, off) for t in (emb, ref, al))
    F.tsa_tatt_bwd(ed, rd, ad, prob, gd, ge, gr, ga)
    for got, exp, wide, name in ((ge, ge_r, we, "g_emb"), (gr, gr_r, wr, "g_emb_ref"), (ga, ga_r, wa, "g_aligned")):
        _close(got, exp, dtype, name + " slice")
        assert _untouched(wide, off, c), name


# ---- the pool pair ----
def _cl(x):
    """(N, C, H, W) CPU -> channels-last (N, 1, H, W, C) on the device."""
    return _dev(x.permute(0, 2, 3, 1).unsqueeze(1))


def _nchw(v):
    return v[:, 0].permute(0, 3, 1, 2).cpu()


def _pool_check(x, gm, ga, dtype, what, view=None):
    n, c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xr = x.clone().requires_grad_(True)  # torch's CPU kernels in the storage dtype
    ym = Fn.max_pool2d(xr, 3, 2, 1)
    ym.backward(gm)
    gxm = xr.grad.clone()
    ya = Fn.avg_pool2d(xr, 3, 2, 1)
    assert ym.shape == (n, c, ho, wo) and ya.shape == ym.shape
    x64 = x.double().requires_grad_(True)
    Fn.avg_pool2d(x64, 3, 2, 1).backward(ga.double())

    xv = _cl(x)
    if view is not None:
        xv = view(xv)
    y = torch.full((n, 1, ho, wo, 2 * c), float("nan"), dtype=dtype, device=DEV)
    assert F.pool3s2(xv, y) is y
    assert torch.equal(_nchw(y[..., :c]), ym.detach()), "max " + what
    assert torch.equal(_nchw(y[..., c:]), ya.detach()), "avg " + what
    zero = torch.zeros_like(gm)
    gx = torch.full((n, 1, h, w, c), float("nan"), dtype=dtype, device=DEV)
    gy = _cl(torch.cat((gm, zero), 1))
    if view is not None:
        gy = view(gy)
    assert F.pool3s2_bwd(xv, gy, gx) is gx
    assert torch.equal(_nchw(gx), gxm), "routed " + what
    F.pool3s2_bwd(xv, _cl(torch.cat((zero, ga), 1)), gx)
    _close(_nchw(gx), x64.grad, dtype, "avg bwd " + what)
    F.pool3s2_bwd(xv, _cl(torch.cat((gm, ga), 1)), gx)
    _close(_nchw(gx), gxm.double() + x64.grad, dtype, "both bwd " + what)
    gx2 = torch.empty_like(gx)
    F.pool3s2_bwd(xv, _cl(torch.cat((gm, ga), 1)), gx2)
    assert torch.equal(gx, gx2), what


POOL_SIZES = [(1, 1), (2, 2), (5, 7), (6, 130)]


@pytest.mark.parametrize("c", [2, 16, 48])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_pair_matches_torch_bitwise(dtype, c):
    for i, (h, w) in enumerate(POOL_SIZES):
        g = torch.Generator().manual_seed(10 * c + i)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        x = torch.randn((2, c, h, w), generator=g).to(dtype)
        gm = torch.randn((2, c, ho, wo), generator=g).to(dtype)
        ga = torch.randn((2, c, ho, wo), generator=g).to(dtype)
        _pool_check(x, gm, ga, dtype, f"random {dtype} c={c} {h}x{w}")
        # small integers, many exact ties: the first maximum wins, forward and backward
        t = torch.randint(-1, 2, (2, c, h, w), generator=g).to(dtype)
        _pool_check(t, gm, ga, dtype, f"ties {dtype} c={c} {h}x{w}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_pair_on_channel_slices(dtype):
    g = torch.Generator().manual_seed(5)
    c, h, w = 16, 5, 7
    x = torch.randn((2, c, h, w), generator=g).to(dtype)
    gm = torch.randn((2, c, 3, 4), generator=g).to(dtype)
    ga = torch.randn((2, c, 3, 4), generator=g).to(dtype)
    for off in (8, 3):
        def view(t, off=off):
            wide, v = _slice_of(t.shape, t.dtype, off)
            v.copy_(t)
            return v
        _pool_check(x, gm, ga, dtype, f"slice at {off} {dtype}", view)


def test_pool_pair_nan_and_infinities():
    """A NaN wins over what precedes it; a window of -inf keeps its first position."""
    x = torch.randn((1, 2, 4, 5), generator=torch.Generator().manual_seed(1))
    x[0, 0, 1, 1] = float("nan")
    x[0, 1] = float("-inf")
    xr = x.clone().requires_grad_(True)
    ym = Fn.max_pool2d(xr, 3, 2, 1)
    gm = torch.arange(1.0, 1.0 + ym.numel()).view(ym.shape)
    ym.backward(gm)
    y = F.pool3s2(_cl(x), torch.empty((1, 1, 2, 3, 4), device=DEV))
    assert torch.equal(_nchw(y[..., :2]).nan_to_num(7.0), ym.detach().nan_to_num(7.0))
    gx = F.pool3s2_bwd(_cl(x), _cl(torch.cat((gm, torch.zeros_like(gm)), 1)), torch.empty((1, 1, 4, 5, 2), device=DEV))
    assert torch.equal(_nchw(gx), xr.grad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_pair_op(dtype):
    """torch.ops.vsrk.pool3s2 on NCHW tensors: torch's two pools concatenated,
    values and routed gradients bitwise, with autograd and a fake implementation."""
    import vsr_amd.ops  # noqa: F401  (registers torch.ops.vsrk)
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 5, 6), generator=g).to(dtype)
    gm = torch.randn((2, 3, 3, 3), generator=g).to(dtype)
    xr = x.clone().requires_grad_(True)
    ref = torch.cat((Fn.max_pool2d(xr, 3, 2, 1), Fn.avg_pool2d(xr, 3, 2, 1)), 1)
    ref[:, :3].backward(gm)
    xd = x.to(DEV).requires_grad_(True)
    y = torch.ops.vsrk.pool3s2(xd)
    assert y.dtype == dtype and torch.equal(y.detach().cpu(), ref.detach())
    y.backward(torch.cat((gm, torch.zeros_like(gm)), 1).to(DEV))
    assert torch.equal(xd.grad.cpu(), xr.grad)
    torch.library.opcheck(torch.ops.vsrk.pool3s2.default, (torch.randn((1, 2, 4, 4), device=DEV, requires_grad=True),),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))


# ---- the gated merge ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_modulate_forward_and_backward(dtype):
    for i, shape in enumerate(((2, 1, 5, 7, 2), (1, 1, 3, 4, 16), (2, 1, 6, 70, 64))):
        g = torch.Generator().manual_seed(i)
        fea, att, add, d = (torch.randn(shape, generator=g).to(dtype) for _ in range(4))
        att = (att.float() * 3).to(dtype)
        f64, a64, b64 = (t.double().requires_grad_(True) for t in (fea, att, add))
        ref = f64 * torch.sigmoid(a64) * 2 + b64
        ref.backward(d.double())
        fd, ad, bd, dd = _dev(fea), _dev(att), _dev(add), _dev(d)
        out = F.tsa_modulate(fd, ad, bd, torch.full(shape, float("nan"), dtype=dtype, device=DEV))
        _close(out, ref.detach(), dtype, f"modulate {dtype} {shape}")
        gf, ga, gb = (torch.full(shape, float("nan"), dtype=dtype, device=DEV) for _ in range(3))
        F.tsa_modulate_bwd(fd, ad, dd, gf, ga, gb)
        _close(gf, f64.grad, dtype, "gfea")
        _close(ga, a64.grad, dtype, "gatt")
        assert torch.equal(gb, dd)
        gf2, ga2 = torch.empty_like(gf), torch.empty_like(ga)
        F.tsa_modulate_bwd(fd, ad, dd, gf2, ga2)  # without the copy of g
        assert torch.equal(gf, gf2) and torch.equal(ga, ga2)
    # in place on an unaligned channel slice: out over fea
    wide, v = _slice_of((1, 1, 4, 4, 6), torch.float32, 3)
    v.copy_(torch.linspace(-2, 2, 96, device=DEV).view(1, 1, 4, 4, 6))
    want = v.double() * torch.sigmoid(v.double()) * 2 + v.double()
    F.tsa_modulate(v, v, v, v)
    assert (v.double() - want).abs().max().item() <= 2e-5 * want.abs().max().item() and _untouched(wide, 3, 6)


def test_bad_arguments():
    x = torch.zeros((2, 1, 4, 6, 8), device=DEV)
    with pytest.raises(RuntimeError, match=r"pool3s2_fwd failed \(code 1\).*max \| avg"):
        F.pool3s2(x, torch.zeros((2, 1, 2, 3, 8), device=DEV))
    with pytest.raises(RuntimeError, match=r"pool3s2_bwd failed \(code 1\).*gx"):
        F.pool3s2_bwd(x, torch.zeros((2, 1, 2, 3, 16), device=DEV), torch.zeros((2, 1, 4, 5, 8), device=DEV))
    with pytest.raises(RuntimeError, match=r"tsa_tatt_fwd failed \(code 1\).*out"):
        F.tsa_tatt(x, x[:1], x, torch.zeros((1, 1, 4, 6, 8), device=DEV), torch.zeros((1, 2, 4, 6), device=DEV))
    with pytest.raises(ValueError, match="prob"):
        F.tsa_tatt(x, x[:1], x, torch.zeros((1, 1, 4, 6, 16), device=DEV), torch.zeros((2, 1, 4, 6), device=DEV))
    wide = torch.zeros((1, 1, 2, 2, 80), device=DEV)[..., 1:73]  # 72 channels, one element per lane
    with pytest.raises(RuntimeError, match=r"tsa_tatt_fwd failed \(code 1\).*64 lanes"):
        F.tsa_tatt(wide, wide, wide, torch.zeros((1, 1, 2, 2, 72), device=DEV), torch.zeros((1, 1, 2, 2), device=DEV))
    with pytest.raises(RuntimeError, match=r"tsa_modulate_fwd failed \(code 1\).*att"):
        F.tsa_modulate(x, x[..., :4], x, x)
