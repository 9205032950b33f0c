"""fp64 references, input builders and bounds for the loss, PSNR and SSIM
kernels, shared by the GPU tests (test_losses_gpu, test_metrics_gpu,
test_metrics3d_gpu) and by the CPU self-check of their sharpness
(test_metrics_sharpness_cpu).  Plain helper module: no fixtures, no hooks.

Every reference is torch fp64 on the CPU over the fp32 values the kernel is
given; parameters that cross the C ABI as ``float`` (delta, epsilon, mean,
std, max_value) are rounded to fp32 first.  References are computed once per
case (lru_cache) and must not be modified by their users.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import cpu_nets

EPS32 = 2.0 ** -24  # half an ulp of fp32, relative
# half an ulp of the gradient's storage type, relative (test_conv_row_gpu.py's convention)
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# fp16 is subnormal below 2^-14 with a fixed spacing of 2^-24: half an ulp there is 2^-25 absolute
FP16_SUBNORMAL_HALF_ULP = 2.0 ** -25

ACDC = cpu_nets.DATASET_STATS["acdc"]
DSB15 = cpu_nets.DATASET_STATS["dsb15"]


def f32(x: float) -> float:
    """The value a C ``float`` parameter holds."""
    return float(np.float32(x))


def ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------ losses --
# (name, kind code of the ABI, parameter as the ABI sees it)
LOSS_SPECS = [
    ("l1", 0, 0.0),
    ("mse", 1, 0.0),
    ("huber_0.75", 2, 0.75),
    ("huber_f32(0.7)", 2, f32(0.7)),
    ("charbonnier_1e-3", 3, f32(1e-3)),
]
LOSS_SPEC_IDS = [s[0] for s in LOSS_SPECS]
# 2^21 + 3 is past the forward's cap of 1024 blocks (reached at 1024 x 256 x 8
# = 2^21 elements), which hands loss_final 1024 partials (four laps of its 256
# lanes), and past the backward's 4096 x 256 = 2^20, so its lanes lap too
LOSS_COUNTS = [1, 255, 256, 257, 2047, 2049, 2 ** 21 + 3]
LOSS_LOCALISED_COUNTS = [2049, 2 ** 21 + 3]
LOSS_GSCALES = [None, 1.0, 0.25, -3.0, 0.0]


def loss_terms(kind: int, p: float, d: torch.Tensor) -> torch.Tensor:
    """Per-element loss in the reference's own formulation (nn.L1Loss,
    nn.MSELoss, HuberLoss with torch.min(|d|, delta), CharbonnierLoss)."""
    a = d.abs()
    if kind == 0:
        return a
    if kind == 1:
        return d * d
    if kind == 2:
        q = torch.min(a, torch.full_like(a, p))  # a tie sends half the gradient each way: d/da sums to delta
        return 0.5 * q * q + p * (a - q)
    return torch.sqrt(d * d + p)


def loss_ref(kind: int, p: float, o: torch.Tensor, t: torch.Tensor):
    """(mean loss as a Python float, fp64 gradient w.r.t. ``o`` by autograd)."""
    o64 = o.detach().double().requires_grad_(True)
    loss = loss_terms(kind, f32(p), o64 - t.double()).mean()
    (g,) = torch.autograd.grad(loss, o64)
    return loss.item(), g


def loss_bound(ref: float) -> float:
    """Each term is <= ~6 fp32 roundings of positive quantities, partial sums
    are double, one final cast: 8 * 2^-24 relative."""
    return 8 * EPS32 * abs(ref)


def grad_bound(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Per element 8 * 2^-24 |ref| for the fp32 arithmetic plus half an ulp of
    the storage type: h |ref| with h = 0 / 2^-8 / 2^-11 (fp32 / bf16 / fp16).
    fp16 alone can be subnormal here (gradients of a mean are O(1/count)):
    below 2^-14 its half ulp is the absolute 2^-25, not h |ref|."""
    a = ref.abs()
    store = HALF_ULP[dtype] * a
    if dtype == torch.float16:
        store = store.clamp_min(FP16_SUBNORMAL_HALF_ULP)
    return 8 * EPS32 * a + store


def grad_violations(g: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype) -> int:
    """Elements outside grad_bound; a NaN counts as one."""
    err = (g.detach().cpu().double().reshape(-1) - ref.reshape(-1)).abs()
    return int((~(err <= grad_bound(ref.reshape(-1), dtype))).sum())


def loss_dense(count: int):
    g = torch.Generator().manual_seed(1000 + count % 9973)
    return torch.randn(count, generator=g), torch.randn(count, generator=g)


def loss_localised_indices(count: int):
    idx = []
    for i in (0, 255, 256, 2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21, count - 1):
        if 0 <= i < count and i not in idx:
            idx.append(i)
    return idx


def loss_localised(count: int):
    """out == target (small integers, so every sum below is exact) except at
    the block / lap / tail indices, each off by its own power of two
    (2^-3, 2^-2, ... alternating in sign; the tail gets the largest)."""
    g = torch.Generator().manual_seed(2000 + count % 9973)
    t = torch.randint(-8, 9, (count,), generator=g).float()
    o = t.clone()
    idx = loss_localised_indices(count)
    for k, i in enumerate(idx):
        o[i] = t[i] + (-1.0) ** k * 2.0 ** (k - 3)
    return o, t, idx


@functools.lru_cache(maxsize=None)
def loss_case(spec: int, count: int, localised: bool = False):
    _, kind, p = LOSS_SPECS[spec]
    if localised:
        o, t, idx = loss_localised(count)
    else:
        (o, t), idx = loss_dense(count), None
    loss, grad = loss_ref(kind, p, o, t)
    return SimpleNamespace(kind=kind, p=p, o=o, t=t, idx=idx, loss=loss, grad=grad)


def loss_kink_points():
    """d = 0 and |d| = delta exactly, and one fp32 step to either side of
    delta, for both deltas (target is 0, so d = out)."""
    pts = [0.0]
    for delta in (np.float32(0.75), np.float32(0.7)):
        up, down = np.nextafter(delta, np.float32(2)), np.nextafter(delta, np.float32(0))
        for v in (delta, up, down):
            pts += [float(v), -float(v)]
    o = torch.tensor(pts, dtype=torch.float32)
    return o, torch.zeros_like(o)


# -------------------------------------------------------------------- PSNR --
PSNR_CHUNKS = 64  # psnr_partial's fixed grid.x
PSNR_PER_SAMPLE = [1, 63, 64, 65, 4097, 64 * 256 + 1]
PSNR_LOCALISED_PER = [4097, 64 * 256 + 1]
PSNR_TOL_DB = 1e-4  # <= 4 * 2^-24 on log10's argument is ~1e-6 dB; log10f within 2 ulp of a value < 16, x 10: ~2e-5 dB
PSNR_EXACT_TOL_DB = 3e-5  # d^2 and its sum exact; the 2e-5 dB of log10f, 2e-6 of the result's own rounding, 1e-6 of the mse cast and division


def denorm64(x: torch.Tensor, mean: float, std: float) -> torch.Tensor:
    """utils.py denormalize in fp64 with the fp32 statistics the kernel gets."""
    return (x.double() * f32(std) + f32(mean)).round().clamp(0, 255)


def screen_off_ties(x: torch.Tensor, mean: float, std: float, margin: float = 1e-3) -> torch.Tensor:
    """Nudge every element whose fp64 x * std + mean lies within ``margin`` of
    a half-integer.  Device code is built with the compiler's default
    contraction, so a fused multiply-add may round such a near-tie to the other
    grey level than torch's separate multiply and add (about 1e-5 of randn
    pixels): an accepted difference, kept out of the comparison here the way
    test_dcn_gpu keeps samples off grid lines."""
    x = x.clone()
    for _ in range(16):
        v = x.double() * f32(std) + f32(mean)
        near = ((v - torch.floor(v)) - 0.5).abs() < margin
        if not bool(near.any()):
            return x
        x[near] += f32(4 * margin / std)
    raise AssertionError("screen_off_ties did not converge")


def psnr_ref(o: torch.Tensor, t: torch.Tensor, max_value: float = 255.0) -> torch.Tensor:
    """metrics.py:20-36 per sample in fp64 (the 1e-10 and max_value as fp32 hold them)."""
    d = o.double() - t.double()
    mse = (d * d).flatten(1).mean(1)
    return 10 * torch.log10(f32(max_value) ** 2 / (mse + f32(1e-10)))


def psnr_dense(batch: int, per: int, max_value: float):
    """Different content and a different noise level per sample."""
    g = torch.Generator().manual_seed(3000 + 7 * batch + per % 9973 + int(max_value))
    o = torch.rand((batch, per), generator=g) * max_value
    lvl = 0.02 * max_value * torch.arange(1, batch + 1, dtype=torch.float32).view(batch, 1)
    return o, o + lvl * torch.randn((batch, per), generator=g)


def psnr_boundary_indices(per: int):
    pc = -(-per // PSNR_CHUNKS)
    idx = {0, per - 1}
    for k in range(1, PSNR_CHUNKS):
        if k * pc < per:
            idx |= {k * pc - 1, k * pc}
    return sorted(idx), pc


def psnr_localised(per: int):
    """Integer images equal except at the first and last element and on either
    side of each of the 63 chunk boundaries.  Those ~128 places are dealt to
    samples in runs of 8 and differ by 2^0 .. 2^7 within a sample, so d^2 and
    every sample's sum are exact in fp32/fp64 and each place has its own
    weight.  Dropping or doubling the d = 1 place of a sample moves its PSNR
    by 10 log10(1 + 1/21845) = 2e-4 dB, the others by 4x more each, up to 6 dB."""
    idx, _ = psnr_boundary_indices(per)
    groups = [idx[i:i + 8] for i in range(0, len(idx), 8)]
    g = torch.Generator().manual_seed(4000 + per % 9973)
    t = torch.randint(0, 128, (len(groups), per), generator=g).float()
    o = t.clone()
    for b, grp in enumerate(groups):
        for k, i in enumerate(grp):
            o[b, i] = t[b, i] + 2.0 ** k
    return o, t, groups


def psnr_ties():
    """mean 0.5, std 2, x = k/2: x * std + mean = k + 0.5 exactly, fused or
    not, for k in [-4, 260] -- every value a tie, both clamps included.  The
    target is the same ramp one step on (k + 1), so neighbours of opposite
    parity meet: inside the clamps half-to-even gives d in {0, 2} (mse ~2),
    half-away d = 1 everywhere (mse ~1, 3 dB off)."""
    k = torch.arange(-4, 261, dtype=torch.float32)
    o = (k / 2).view(1, -1)
    return o, o + 0.5, 0.5, 2.0


def psnr_stats_case(dataset: str):
    mean, std = cpu_nets.DATASET_STATS[dataset]
    g = torch.Generator().manual_seed(5000 + len(dataset))
    o = torch.randn((3, 1, 37, 41), generator=g) * 1.5
    t = o + 0.3 * torch.randn((3, 1, 37, 41), generator=g)
    return screen_off_ties(o, mean, std), screen_off_ties(t, mean, std), mean, std


# -------------------------------------------------------------------- SSIM --
SSIM_WIN, SSIM_TX, SSIM_TY = 11, 32, 16  # window; output tile of ssim_partial
SSIM2D_SHAPES = [
    (2, 1, 11, 11), (2, 1, 11, 43), (2, 1, 27, 11), (2, 1, 27, 43),
    (2, 1, 26, 42),  # exactly one full tile
    (2, 3, 43, 75),
    (1, 1, 17611, 11),  # 1101 tiles: ssim_final's strided loop takes a second lap
    (5, 2, 30, 50),
]
SSIM3D_SHAPES = [
    (1, 1, 11, 11, 11),  # one output voxel
    (2, 2, 12, 28, 44),  # dout = 2, 2 x 2 in-plane tiles
    (1, 3, 13, 27, 43),
    (2, 1, 11, 26, 42),
]
SSIM_FLOOR = 2.0 ** -22  # the fp32 result's own rounding near 1


def ssim_shapes(dim: int):
    return SSIM2D_SHAPES if dim == 2 else SSIM3D_SHAPES


def ramp_pair(shape, seed: int = 0):
    """Normalised-space pair whose per-pixel SSIM varies strongly: o is noise,
    t = ramp * o + (1 - ramp) * other noise, ramp 0 -> 1 along W, 1 -> 0.2
    along H (and 1 -> 0.5 along D); its own seed per (sample, channel)."""
    n, c, *sp = shape
    ramp = torch.linspace(0, 1, sp[-1]) * torch.linspace(1, 0.2, sp[-2]).view(-1, 1)
    if len(sp) == 3:
        ramp = ramp * torch.linspace(1, 0.5, sp[0]).view(-1, 1, 1)
    o, t = torch.empty(shape), torch.empty(shape)
    for i in range(n):
        for j in range(c):
            g = torch.Generator().manual_seed(7000 + 100 * seed + i * c + j)
            a, b = torch.randn(sp, generator=g), torch.randn(sp, generator=g)
            o[i, j], t[i, j] = a, ramp * a + (1 - ramp) * b
    return o, t


def ssim_map(o: torch.Tensor, t: torch.Tensor, value_range: float) -> torch.Tensor:
    """cpu_nets.ssim's per-pixel map (same fp32-built window, same formula) --
    the sharpness check mutates this; ssim_case asserts its means equal
    cpu_nets.ssim's."""
    dim, ch = o.dim() - 2, o.shape[1]
    conv = torch.nn.functional.conv2d if dim == 2 else torch.nn.functional.conv3d
    g1 = torch.arange(11, dtype=torch.float32)
    g1 = 1 / (1.5 * math.sqrt(2 * math.pi)) * torch.exp(-((g1 - 5) / (2 * 1.5)) ** 2)
    k = g1
    for _ in range(dim - 1):
        k = k.unsqueeze(-1) * g1
    k = (k / k.sum()).view(1, 1, *k.shape).repeat(ch, *[1] * (dim + 1)).to(o.dtype)
    c1, c2 = (0.01 * value_range) ** 2, (0.03 * value_range) ** 2
    mu1, mu2 = conv(o, k, groups=ch), conv(t, k, groups=ch)
    s1 = conv(o * o, k, groups=ch) - mu1.pow(2)
    s2 = conv(t * t, k, groups=ch) - mu2.pow(2)
    s12 = conv(o * t, k, groups=ch) - mu1 * mu2
    return ((2 * mu1 * mu2 + c1) * (2.0 * s12 + c2)) / ((mu1.pow(2) + mu2.pow(2) + c1) * (s1 + s2 + c2))


def per_sample(m: torch.Tensor) -> torch.Tensor:
    return m.flatten(1).mean(1)


def ssim_ref_and_gap(o: torch.Tensor, t: torch.Tensor, value_range: float):
    """(fp64 per-sample SSIM, |fp32 evaluation - fp64 evaluation| per sample)
    of cpu_nets.ssim on the fp32 images o, t."""
    dim, ch = o.dim() - 2, o.shape[1]
    ref = cpu_nets.ssim(o.double(), t.double(), dim, ch, False, value_range)
    low = cpu_nets.ssim(o, t, dim, ch, False, value_range)
    return ref, (low.double() - ref).abs()


@functools.lru_cache(maxsize=None)
def ssim_case(shape):
    """One shape's inputs and references in the three ranges:
      x_o, x_t     normalised (ACDC statistics), screened off rounding ties --
                   the fused denormalize=True path
      o255, t255   their denormalisation: integer images, value_range 255
      o1, t1       float images in [0, 1], value_range 1
    ref255 serves both of the first two."""
    x_o, x_t = ramp_pair(shape)
    x_o, x_t = screen_off_ties(x_o, *ACDC), screen_off_ties(x_t, *ACDC)
    o255, t255 = denorm64(x_o, *ACDC).float(), denorm64(x_t, *ACDC).float()
    o1, t1 = (x_o * 0.188 + 0.212).clamp(0, 1), (x_t * 0.188 + 0.212).clamp(0, 1)
    ref255, gap255 = ssim_ref_and_gap(o255, t255, 255.0)
    ref1, gap1 = ssim_ref_and_gap(o1, t1, 1.0)
    assert torch.equal(per_sample(ssim_map(o255.double(), t255.double(), 255.0)), ref255)
    return SimpleNamespace(shape=shape, x_o=x_o, x_t=x_t, o255=o255, t255=t255, o1=o1, t1=t1,
                           ref255=ref255, gap255=gap255, ref1=ref1, gap1=gap1)


def ssim_gap(dim: int, value_range: int) -> float:
    """g_max: the largest fp32-vs-fp64 gap of the reference itself over the
    module's ramp cases of this window dimension and value range."""
    key = "gap255" if value_range == 255 else "gap1"
    return max(float(getattr(ssim_case(s), key).max()) for s in ssim_shapes(dim))


def check_ssim(tag: str, m: torch.Tensor, per: torch.Tensor, ref: torch.Tensor, tol: float) -> None:
    """A kernel's (batch mean, per-sample) result: per-sample and mean within
    tol of fp64 (a NaN fails); the mean equals the mean of the returned
    per-sample values within 2 fp32 ulp.  Prints each figure first."""
    per = per.cpu().double()
    err = (per - ref).abs().max().item()
    print(f"{tag}: max per-sample err {err:.3e}, mean err {abs(m.item() - ref.mean().item()):.3e}, tol {tol:.3e}")
    assert per.shape == ref.shape
    assert err <= tol, (tag, err, tol)
    assert abs(m.item() - ref.mean().item()) <= tol, (tag, m.item(), ref.mean().item())
    assert abs(m.item() - per.mean().item()) <= 2 * ulp32(per.mean().item()), (tag, m.item(), per.mean().item())


def ssim_tol(dim: int, value_range: int, extra_gap: float = 0.0) -> float:
    """What the kernel is allowed against fp64: max(8 g_max, 2^-22).  g_max is
    what fp32 evaluation costs the reference alone; 8 covers the kernel's
    separable summation order and contraction."""
    return max(8 * max(ssim_gap(dim, value_range), extra_gap), SSIM_FLOOR)
