"""Metrics on HIP (PSNR, SSIM, with the trainer's denormalize fused) against
the reference's own values (tests/golden/metrics.pt, made by importing
src/model/metrics.py; 1e-4 SSIM / 1e-3 dB there because the fixture values are
fp32 numbers) and against fp64 on the CPU (tests/metrics_ref.py).

PSNR bounds.  Per sample and batch mean within 1e-4 dB of fp64: the kernel's
d^2, the mse cast and the division are <= 4 * 2^-24 relative on log10's
argument (~1e-6 dB); log10f within 2 ulp of a value below 16, times 10, is
~2e-5 dB.  On the localised integer images d^2 and the sums are exact, which
leaves log10f and the result's rounding: 3e-5 dB.  The batch mean equals the
mean of the returned per-sample values within 2 fp32 ulp (it is their fp32
running sum over the batch, divided once).  Identical images give
10 log10(max^2 / 1e-10): within 5e-5 dB of the fp32 CPU formula (2 ulp of
log10f at 14.8, x 10, is 1.9e-5; each side's rounding of 148 is 0.8e-5; the
CPU's own log10 1 ulp is 1e-5).

SSIM tolerance, measured, not assumed.  For every ramp case the reference
itself is evaluated in fp32 and in fp64 on the CPU (oracle.cpu_nets.ssim, same
fp32-built window); g is the per-sample gap between the two, i.e. what fp32
evaluation costs the reference alone.  The kernel is allowed
max(8 * g_max, 2^-22) against fp64, g_max over this module's ramp cases of the
value range (8: a different, separable summation order and contraction;
2^-22: the fp32 result's own rounding near 1).  The gap is recomputed where
the test runs (metrics_ref.ssim_tol); measured on the development host:
  (N, C, H, W)        g, range 255   g, range 1
  (2, 1, 11, 11)      5.1e-7         3.8e-7
  (2, 1, 11, 43)      7.0e-8         5.1e-8
  (2, 1, 27, 11)      1.2e-7         1.5e-7
  (2, 1, 27, 43)      6.0e-8         1.9e-8
  (2, 1, 26, 42)      9.1e-8         6.1e-8
  (2, 3, 43, 75)      2.5e-8         4.2e-8
  (1, 1, 17611, 11)   3.1e-8         2.0e-8
  (5, 2, 30, 50)      5.9e-8         3.5e-8
  tolerance           4.1e-6         3.0e-6
The kernel itself measured 1.5e-7 .. 3.1e-7 from fp64 on these cases on an
MI355X, nearly the same at every shape: it normalises the fp32 1-D window
where the reference normalises the 2-D product, so the taps differ in their
last bit (an fp64 evaluation with the kernel's window is 1.7e-7 .. 1.8e-7 from
the reference's).  The ramp inputs make the per-pixel SSIM vary (standard deviation 0.2-0.27
against 0.01 for target = output + noise), so a misplaced pixel moves the
mean; tests/test_metrics_sharpness_cpu.py proves that on the same inputs.
The older randn + 0.3 noise cases keep their shapes and are held to the same
rule (their own g, 3e-8 .. 6e-8, joins the maximum).
"""
import json

import pytest
import torch

from oracle import cpu_nets
from tests import metrics_ref as R
from tests.conftest import load_golden
from vsr_amd import functional as F
from vsr_amd import metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.mark.parametrize("ds", ["acdc", "dsb15"])
def test_ssim_psnr_match_reference_fixture(ds):
    fx = load_golden("metrics")
    o, t = fx["out"].to(DEV), fx["target"].to(DEV)
    s = metrics.ssim_denorm(o, t, ds).item()
    assert abs(s - fx[f"ssim_{ds}"]) <= 1e-4, (s, fx[f"ssim_{ds}"])
    p = metrics.psnr_denorm(o, t, ds).item()
    assert abs(p - fx[f"psnr_{ds}"]) <= 1e-3, (p, fx[f"psnr_{ds}"])
    per = metrics.psnr_denorm(o, t, ds, size_average=False).cpu()
    assert torch.allclose(per, fx[f"psnr_{ds}_per_sample"], atol=1e-3)


_check_ssim = R.check_ssim


@pytest.mark.parametrize("shape", [(4, 1, 64, 96), (2, 3, 45, 77), (1, 1, 11, 11), (3, 1, 512, 512)])
def test_ssim_matches_oracle(shape):
    g = torch.Generator().manual_seed(sum(shape))
    o = torch.randn(shape, generator=g)
    t = (o + 0.3 * torch.randn(shape, generator=g))
    o, t = R.screen_off_ties(o, *R.ACDC), R.screen_off_ties(t, *R.ACDC)
    od, td = R.denorm64(o, *R.ACDC).float(), R.denorm64(t, *R.ACDC).float()
    ref_per, gap = R.ssim_ref_and_gap(od, td, 255.0)
    tol = R.ssim_tol(2, 255, extra_gap=gap.max().item())
    m, per = F.ssim(o.to(DEV), t.to(DEV), *metrics.DATASET_STATS["acdc"], 255.0, denormalize=True)
    _check_ssim("fused", m, per, ref_per, tol)
    # SSIM module on already-denormalized images (size_average False/True)
    mod = metrics.SSIM(channels=shape[1], size_average=False)
    assert (mod(od.to(DEV), td.to(DEV)).cpu().double() - ref_per).abs().max().item() <= tol
    assert abs(metrics.SSIM(channels=shape[1])(od.to(DEV), td.to(DEV)).item() - ref_per.mean().item()) <= tol


@pytest.mark.parametrize("shape", R.SSIM2D_SHAPES, ids=_ids(R.SSIM2D_SHAPES))
def test_ssim_ramp_fp64(shape):
    """Ramp inputs at the tile edges (tile 16 x 32 outputs, window 11), in the
    three ranges: integer images with value_range 255 through the SSIM module,
    [0, 1] floats with value_range 1, and the fused denormalize=True path on
    the screened normalised inputs (same reference as the first)."""
    c, ch = R.ssim_case(shape), shape[1]
    tol255, tol1 = R.ssim_tol(2, 255), R.ssim_tol(2, 1)
    print(f"{shape}: g255 {c.gap255.max():.2e} g1 {c.gap1.max():.2e}")
    o255, t255 = c.o255.to(DEV), c.t255.to(DEV)
    per = metrics.SSIM(channels=ch, size_average=False)(o255, t255)
    _check_ssim("255 module", metrics.SSIM(channels=ch)(o255, t255), per, c.ref255, tol255)
    o1, t1 = c.o1.to(DEV), c.t1.to(DEV)
    m, per1 = F.ssim(o1, t1, value_range=1.0)
    _check_ssim("[0,1]", m, per1, c.ref1, tol1)
    assert torch.equal(metrics.SSIM(channels=ch, size_average=False, value_range=1)(o1, t1), per1)
    xo, xt = c.x_o.to(DEV), c.x_t.to(DEV)
    m, perf = F.ssim(xo, xt, *metrics.DATASET_STATS["acdc"], 255.0, denormalize=True)
    _check_ssim("fused", m, perf, c.ref255, tol255)
    assert torch.equal(metrics.ssim_denorm(xo, xt, "acdc", size_average=False), perf)
    assert metrics.ssim_denorm(xo, xt, "acdc").item() == m.item()
    # an image against itself
    for img, kw in ((o255, {}), (o1, {"value_range": 1.0}),
                    (xo, dict(zip(("mean", "std"), R.ACDC), denormalize=True))):
        m, same = F.ssim(img, img, **kw)
        assert (1 - same.cpu().double()).abs().max().item() <= 2.0 ** -22
        assert abs(1 - m.item()) <= 2.0 ** -22


@pytest.mark.parametrize("shape", [(5, 2, 30, 50), (2, 3, 43, 75)], ids=["5x2x30x50", "2x3x43x75"])
def test_ssim_batch_permutation(shape):
    """Samples are independent: permuting the batch permutes the per-sample output bitwise."""
    c = R.ssim_case(shape)
    perm = torch.tensor([3, 0, 4, 1, 2][:shape[0]] if shape[0] == 5 else [1, 0])
    for o, t, kw in ((c.o255, c.t255, {}), (c.o1, c.t1, {"value_range": 1.0}),
                     (c.x_o, c.x_t, dict(zip(("mean", "std"), R.ACDC), denormalize=True))):
        _, per = F.ssim(o.to(DEV), t.to(DEV), **kw)
        _, per_p = F.ssim(o[perm].to(DEV), t[perm].to(DEV), **kw)
        assert torch.equal(per_p.cpu(), per.cpu()[perm])


@pytest.mark.parametrize("ds", ["acdc", "dsb15"])
def test_ssim_psnr_denorm_dataset_stats_fp64(ds):
    """The fused denormalize with each dataset's statistics, on inputs screened
    off rounding ties (metrics_ref.screen_off_ties says why): device code is
    built with the compiler's default contraction, and a fused multiply-add may
    round a near-tie to the other grey level than torch's two operations --
    about one grey level on ~1e-5 of pixels, an accepted difference."""
    o, t, mean, std = R.psnr_stats_case(ds)
    od, td = R.denorm64(o, mean, std).float(), R.denorm64(t, mean, std).float()
    ref = R.psnr_ref(od, td)
    per = metrics.psnr_denorm(o.to(DEV), t.to(DEV), ds, size_average=False).cpu().double()
    print(f"{ds}: psnr err {(per - ref).abs().max():.3e} dB")
    assert (per - ref).abs().max().item() <= R.PSNR_TOL_DB
    assert abs(metrics.psnr_denorm(o.to(DEV), t.to(DEV), ds).item() - ref.mean().item()) <= R.PSNR_TOL_DB
    sref, gap = R.ssim_ref_and_gap(od, td, 255.0)
    m, sper = F.ssim(o.to(DEV), t.to(DEV), mean, std, 255.0, denormalize=True)
    _check_ssim(f"{ds} fused", m, sper, sref, R.ssim_tol(2, 255, extra_gap=gap.max().item()))
    assert torch.equal(metrics.ssim_denorm(o.to(DEV), t.to(DEV), ds, size_average=False), sper)


def test_ssim_too_small_raises():
    for shape in ((1, 1, 10, 16), (1, 1, 16, 10)):
        x = torch.zeros(shape, device=DEV)
        with pytest.raises(RuntimeError, match="at least 11x11"):
            F.ssim(x, x)
        with pytest.raises(RuntimeError, match="at least 11x11"):
            metrics.SSIM()(x, x)


def test_cardiac_ssim_crop_is_a_view(tmp_path):
    """The cardiac box is a non-contiguous view: same value as the crop made contiguous."""
    c = R.ssim_case((2, 3, 43, 75))
    box = (3, 40, 7, 66)
    path = tmp_path / "coords.json"
    path.write_text(json.dumps({"p0": list(box)}))
    o, t = c.o255.to(DEV), c.t255.to(DEV)
    crop = lambda x: x[..., box[0]:box[1], box[2]:box[3]]  # noqa: E731
    assert not crop(o).is_contiguous()
    cs = metrics.CardiacSSIM(str(path), channels=3, size_average=False)
    got = cs(o, t, "p0")
    dense = metrics.SSIM(channels=3, size_average=False)(crop(o).contiguous(), crop(t).contiguous())
    assert torch.equal(got, dense)
    ref, gap = R.ssim_ref_and_gap(crop(c.o255).contiguous(), crop(c.t255).contiguous(), 255.0)
    tol = R.ssim_tol(2, 255, extra_gap=gap.max().item())
    assert (got.cpu().double() - ref).abs().max().item() <= tol
    cp = metrics.CardiacPSNR(str(path), size_average=False)
    pref = R.psnr_ref(crop(c.o255), crop(c.t255))
    assert (cp(o, t, "p0").cpu().double() - pref).abs().max().item() <= R.PSNR_TOL_DB


# -------------------------------------------------------------------- PSNR --
def _check_psnr(tag, m, per, ref, tol):
    per = per.cpu().double()
    err = (per - ref).abs().max().item()
    print(f"{tag}: per-sample err {err:.3e} dB, mean err {abs(m.item() - ref.mean().item()):.3e} dB, tol {tol:.1e}")
    assert per.shape == ref.shape
    assert not err > tol and err == err, (tag, per, ref)
    assert abs(m.item() - ref.mean().item()) <= tol, (tag, m.item(), ref.mean().item())
    assert abs(m.item() - per.mean().item()) <= 2 * R.ulp32(per.mean().item()), (tag, m.item(), per.mean().item())


@pytest.mark.parametrize("per_sample", R.PSNR_PER_SAMPLE)
def test_psnr_geometry_fp64(per_sample):
    """per_sample below, at and off multiples of the 64 fixed chunks; batch 1
    and 5 with different content per sample; max_value 255 and 1."""
    for batch in (1, 5):
        for max_value in (255.0, 1.0):
            o, t = R.psnr_dense(batch, per_sample, max_value)
            ref = R.psnr_ref(o, t, max_value)
            od, td = o.to(DEV), t.to(DEV)
            m, per = F.psnr(od, td, max_value=max_value, denormalize=False)
            _check_psnr(f"per={per_sample} b={batch} max={max_value}", m, per, ref, R.PSNR_TOL_DB)
            assert torch.equal(metrics.PSNR(size_average=False, max_value=max_value)(od, td), per)
            assert metrics.PSNR(max_value=max_value)(od, td).item() == m.item()


def test_psnr_5d_input():
    g = torch.Generator().manual_seed(21)
    o = torch.rand((2, 1, 3, 5, 7), generator=g) * 255
    t = o + 9 * torch.randn(o.shape, generator=g)
    ref = R.psnr_ref(o, t)
    m, per = F.psnr(o.to(DEV), t.to(DEV), denormalize=False)
    _check_psnr("5-D", m, per, ref, R.PSNR_TOL_DB)
    assert torch.equal(metrics.PSNR(size_average=False)(o.to(DEV), t.to(DEV)), per)


@pytest.mark.parametrize("per_sample", R.PSNR_LOCALISED_PER)
def test_psnr_localised_fp64(per_sample):
    """Integer images equal except at the first and last element and either
    side of every chunk boundary i0 = k * ceil(per / 64), each place with its
    own power of two inside its sample (metrics_ref.psnr_localised): exact
    sums, 3e-5 dB; a dropped or doubled place moves its sample by >= 2e-4 dB."""
    o, t, _ = R.psnr_localised(per_sample)
    ref = R.psnr_ref(o, t)
    m, per = F.psnr(o.to(DEV), t.to(DEV), denormalize=False)
    _check_psnr(f"localised per={per_sample}", m, per, ref, R.PSNR_EXACT_TOL_DB)


@pytest.mark.parametrize("max_value", [255.0, 1.0])
def test_psnr_identical_images(max_value):
    """mse = 0: 10 log10(max^2 / 1e-10), as the fp32 reference formula gives it."""
    g = torch.Generator().manual_seed(22)
    o = torch.rand((3, 1, 17, 29), generator=g) * max_value
    want32 = cpu_nets.psnr(o, o.clone(), max_value, size_average=False).double()
    m, per = F.psnr(o.to(DEV), o.to(DEV), max_value=max_value, denormalize=False)
    assert (per.cpu().double() - want32).abs().max().item() <= 5e-5, (per, want32)
    _check_psnr(f"identical max={max_value}", m, per, R.psnr_ref(o, o, max_value), R.PSNR_TOL_DB)
    # the fused path too: both sides denormalise to the same integers
    m, per = F.psnr(o.to(DEV), o.to(DEV), 0.5, 2.0, max_value, denormalize=True)
    assert (per.cpu().double() - want32).abs().max().item() <= 5e-5


def test_psnr_denormalize_exact_ties():
    """mean 0.5, std 2, x = k / 2 for k in [-4, 260]: every x * std + mean is
    exactly k + 0.5 (fused or not), so the kernel's rounding must be
    half-to-even like torch.round, and both clamps are hit.  Half-away would
    be 3 dB off (test_metrics_sharpness_cpu)."""
    o, t, mean, std = R.psnr_ties()
    ref = R.psnr_ref(R.denorm64(o, mean, std), R.denorm64(t, mean, std))
    m, per = F.psnr(o.to(DEV), t.to(DEV), mean, std, 255.0, denormalize=True)
    _check_psnr("ties", m, per, ref, R.PSNR_EXACT_TOL_DB)
    # the same ties through SSIM's denormalize: 3 x 265 values as a 15 x 53 image
    o2 = o.repeat(1, 3).view(1, 1, 15, 53)
    t2 = t.repeat(1, 3).view(1, 1, 15, 53)
    od, td = R.denorm64(o2, mean, std).float(), R.denorm64(t2, mean, std).float()
    sref, gap = R.ssim_ref_and_gap(od, td, 255.0)
    m, sper = F.ssim(o2.to(DEV), t2.to(DEV), mean, std, 255.0, denormalize=True)
    _check_ssim("ties ssim", m, sper, sref, R.ssim_tol(2, 255, extra_gap=gap.max().item()))
