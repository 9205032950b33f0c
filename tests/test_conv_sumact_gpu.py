"""The PReLU-of-the-sum conv epilogue (VSRK_ACT_PRELU_SUM):
    out = prelu(out_scale * (bias + conv) + residual), slope *act_param
-- the tail of RBPN's ResnetBlock -- on the two kernels that implement it
(the tile kernel, every dtype; the 2-D rolling form, 16-bit, cout % 64 == 0)
and on shapes every other family would take for another activation: those
must decline, and whichever kernel runs a silent "no activation" fails here.

Parity against fp64 on the dtype-rounded operands, per element, no element
excluded, in the form of tests/test_conv_row_gpu.py::_check:
    |y - ref| <= h |ref| + (9 Cin + 24) * 2^-24 * max(1, |a|) * mag + 2^-24
h = 2^-8 (bf16) / 2^-11 (fp16) / 0 (fp32): the one output rounding;
mag = conv(|x|, |w|) + |bias| + |residual|: the fp32 accumulation of at most
9 Cin terms plus the epilogue's few operations, each at most 2^-24 relative
to the magnitudes summed so far; PReLU is Lipschitz with constant max(1, |a|).

Also: the argument checks (no residual / a mask -> VSRK_ERR_INVALID), two
identical launches bitwise equal, and F.sub against torch (exact up to the
output rounding) on contiguous and channel-sliced views in all three dtypes.
"""
import pytest
import torch
import torch.nn.functional as Fn

from vsr_amd import functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
SENTINEL = 7.0


def _store(t, dtype, lo=0, width=None):
    """t (.., C) on the device as channels [lo, lo + C) of a `width`-channel
    buffer filled with SENTINEL (whole 16-byte chunks by default) -> (view, buffer)."""
    c = t.shape[-1]
    width = width or -(-c // 8) * 8
    buf = torch.full((*t.shape[:-1], width), SENTINEL, dtype=dtype, device=DEV)
    buf[..., lo:lo + c] = t.to(dtype).to(DEV)
    return buf[..., lo:lo + c], buf


def _untouched(buf, lo, c):
    return bool((buf[..., :lo] == SENTINEL).all()) and bool((buf[..., lo + c:] == SENTINEL).all())


def _shuffle_phys(t, r):
    """logical (N, 1, H, W, r r c') in view channel order -> physical (N, 1, r H, r W, c')"""
    n, _, h, w, c = t.shape
    cp = c // (r * r)
    return t.view(n, 1, h, w, r, r, cp).permute(0, 1, 2, 4, 3, 5, 6).reshape(n, 1, h * r, w * r, cp)


def _run(shape, cin, cout, k, dtype, slope, seed, *, sliced=False, y_shuffle=1):
    """One launch against its fp64 reference -> (worst |y - ref| / bound, the output)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, 1, h, w, cin), generator=g)
    wt = torch.randn((cout, cin, 1, k, k), generator=g) / (k * k * cin) ** 0.5
    b = torch.randn(cout, generator=g)
    res = torch.randn((n, 1, h, w, cout), generator=g)
    xq, wq, rq = x.to(dtype).double(), wt.to(dtype).double(), res.to(dtype).double()

    def conv64(a, ww):
        return Fn.conv2d(a[:, 0].permute(0, 3, 1, 2), ww[:, :, 0], padding=k // 2).permute(0, 2, 3, 1).unsqueeze(1)

    bd = b.double().view(1, 1, 1, 1, -1)
    s = conv64(xq, wq) + bd + rq
    ref = torch.where(s > 0, s, slope * s)
    mag = conv64(xq.abs(), wq.abs()) + bd.abs() + rq.abs()
    bound = HALF_ULP[dtype] * ref.abs() + (9 * cin + 24) * 2.0 ** -24 * max(1.0, abs(slope)) * mag + 2.0 ** -24

    if sliced:
        xv, _ = _store(x, dtype, 64, 144 if cin == 64 else cin + 80)
        rv, _ = _store(res, dtype, 16, cout + 24)
        ylo = 8
        yv, ybuf = _store(torch.zeros_like(res), dtype, ylo, cout + 24)
        ybuf[..., ylo:ylo + cout] = SENTINEL
    elif y_shuffle > 1:
        xv, _ = _store(x, dtype)
        rv, _ = _store(_shuffle_phys(res, y_shuffle), dtype)
        ylo = 0
        yv, ybuf = _store(torch.zeros_like(rv, device="cpu"), dtype)
    else:
        xv, _ = _store(x, dtype)
        rv, _ = _store(res, dtype)
        ylo = 0
        yv, ybuf = _store(torch.zeros_like(res), dtype)
    wp = F.pack_weight(wt.to(DEV), 0, dtype)
    a = torch.tensor([slope], dtype=torch.float32, device=DEV)
    bias = b.to(DEV)
    kk, pp = ((1, 3, 3), (0, 1, 1)) if k == 3 else ((1, 1, 1), (0, 0, 0))

    def launch(out):
        return F.conv(xv, wp, out, kk, pp, bias=bias, bias_r=1, residual=rv, act=F.ACT_PRELU_SUM, act_param=a,
                      y_shuffle=y_shuffle)

    launch(yv)
    again = launch(torch.empty_like(ybuf)[..., ylo:ylo + yv.shape[-1]])
    torch.cuda.synchronize()
    assert torch.equal(yv, again), "two identical launches differ"
    if sliced:
        assert _untouched(ybuf, ylo, cout), "channels outside the output slice were written"
    got = yv.cpu().double()
    if y_shuffle > 1:
        ref, bound = _shuffle_phys(ref, y_shuffle), _shuffle_phys(bound, y_shuffle)
    assert got.shape == ref.shape
    ratio = ((got - ref).abs() / bound).max().item()
    return ratio, got


def _check(ratio, what):
    print(f"{what}: worst |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("sliced", [False, True], ids=["plain", "sliced"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,c", [((2, 19, 37), 64), ((1, 17, 33), 256)], ids=["c64", "c256"])
def test_rolling_form(shape, c, dtype, sliced):
    ratio, _ = _run(shape, c, c, 3, dtype, 0.25, 1, sliced=sliced)
    _check(ratio, f"roll {shape} c{c} {dtype} sliced={sliced}")


@pytest.mark.parametrize("shape,c,dtype", [((2, 9, 11), 16, torch.float32), ((1, 9, 11), 96, torch.bfloat16)],
                         ids=["fp32_c16", "bf16_c96"])
def test_tile_kernel(shape, c, dtype):
    ratio, _ = _run(shape, c, c, 3, dtype, 0.25, 2)
    _check(ratio, f"tile {shape} c{c} {dtype}")


DECLINE = {  # cin, cout, k, y_shuffle: shapes another family takes for the activations it implements
    "pw_1x1_64": (64, 64, 1, 1),
    "thin_in_2_64": (2, 64, 3, 1),
    "thin_out_64_1": (64, 1, 3, 1),
    "fast_yshuffle2": (64, 64, 3, 2),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(DECLINE))
def test_other_families_decline(name, dtype):
    cin, cout, k, ys = DECLINE[name]
    ratio, _ = _run((2, 9, 13), cin, cout, k, dtype, -0.5, 3, y_shuffle=ys)
    _check(ratio, f"{name} {dtype}")


@pytest.mark.parametrize("slope", [0.25, -0.1, 0.0, 1.5])
def test_slopes(slope):
    ratio, got = _run((2, 19, 37), 64, 64, 3, torch.bfloat16, slope, 4)
    _check(ratio, f"slope {slope}")
    if slope == 0.0:
        assert (got >= 0).all() and (got == 0).any()


def _args(dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 1, 8, 8, 64), generator=g).to(dtype).to(DEV)
    wp = F.pack_weight(torch.randn((64, 64, 1, 3, 3), generator=g).to(DEV), 0, dtype)
    return x, wp, torch.empty_like(x), torch.tensor([0.25], device=DEV)


def test_needs_a_residual():
    x, wp, y, a = _args()
    with pytest.raises(RuntimeError, match=r"code 1\)"):  # VSRK_ERR_INVALID
        F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), act=F.ACT_PRELU_SUM, act_param=a)


def test_takes_no_mask():
    x, wp, y, a = _args()
    with pytest.raises(RuntimeError, match=r"code 1\)"):
        F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), residual=x, mask=x, act=F.ACT_PRELU_SUM, act_param=a)


def test_takes_no_accumulate():
    x, wp, y, a = _args()
    with pytest.raises(RuntimeError, match=r"code 1\)"):
        F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), residual=x, accumulate=True, act=F.ACT_PRELU_SUM, act_param=a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
def test_sub_matches_torch(dtype, sliced):
    g = torch.Generator().manual_seed(6)
    a, b = (torch.randn((2, 1, 5, 7, 24), generator=g) for _ in range(2))
    if sliced:
        av, _ = _store(a, dtype, 8, 40)
        bv, _ = _store(b, dtype, 16, 48)
        ov, obuf = _store(torch.zeros_like(a), dtype, 8, 40)
        obuf[..., 8:32] = SENTINEL
    else:
        (av, _), (bv, _), (ov, obuf) = _store(a, dtype), _store(b, dtype), _store(torch.zeros_like(a), dtype)
    F.sub(av, bv, ov)
    torch.cuda.synchronize()
    want = (av.float() - bv.float()).to(dtype)  # fp32 arithmetic, one output rounding
    assert torch.equal(ov, want)
    if sliced:
        assert _untouched(obuf, 8, 24)
    with pytest.raises(RuntimeError, match=r"code 1\)"):
        F.sub(av, bv[..., :16], ov)
