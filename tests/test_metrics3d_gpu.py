"""SSIM(dim=3) and the Cardiac bounding-box metrics against the reference's own
values (tests/golden/metrics3d.pt, written by oracle/make_golden.py from
src/model/metrics.py:39-165 on fixed data; fp32 kernels with fp64 partial
sums: within 1e-5 relative of the reference), and SSIM(dim=3) against fp64 on
the CPU (tests/metrics_ref.py) on volumes with more than one in-plane tile,
more than one channel, dout = 1 and dout > 1.

Tolerance against fp64, by the rule of test_metrics_gpu.py: g is the gap
between oracle.cpu_nets.ssim(dim=3) evaluated in fp32 and in fp64 on the same
ramp volumes (what fp32 costs the reference alone); the kernel is allowed
max(8 * g_max, 2^-22), g_max over this module's ramp cases of the value
range.  Recomputed where the test runs; measured on the development host:
  (N, C, D, H, W)       g, range 255   g, range 1
  (1, 1, 11, 11, 11)    7.9e-7         1.4e-6
  (2, 2, 12, 28, 44)    7.5e-7         9.1e-8
  (1, 3, 13, 27, 43)    6.9e-7         3.2e-8
  (2, 1, 11, 26, 42)    7.9e-7         2.1e-7
  tolerance             6.3e-6         1.1e-5
The kernel itself measured 3.4e-7 .. 5.2e-7 from fp64 on these cases on an
MI355X; 3.7e-7 of that is its window, three normalised fp32 1-D factors where
the reference normalises the 3-D product (an fp64 evaluation with the kernel's
window is that far from the reference's).  Per-voxel SSIM of the ramp volumes
has a standard deviation of 0.16-0.17.
"""
import pickle

import pytest
import torch

from tests import metrics_ref as R
from tests.conftest import load_golden
from vsr_amd import _native as N
from vsr_amd import functional as F
from vsr_amd import metrics
from vsr_amd.utils import DATASET_STATS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SSIM3D_SHAPES]


def test_ssim3d_denormalized_matches_reference():
    fx = load_golden("metrics3d")
    mean, std = DATASET_STATS["acdc"]
    m, per = F.ssim(fx["out"].to(DEV), fx["target"].to(DEV), mean, std, 255.0, denormalize=True)
    assert abs(m.item() - fx["ssim3d_acdc"]) <= 1e-5 * abs(fx["ssim3d_acdc"]), (m.item(), fx["ssim3d_acdc"])
    assert (per.cpu().double() - fx["ssim3d_acdc_per_sample"].double()).abs().max().item() <= 1e-5


def test_ssim3d_module_on_volumes():
    fx = load_golden("metrics3d")
    from oracle import cpu_nets
    od = cpu_nets.denormalize(fx["out"], "acdc")
    td = cpu_nets.denormalize(fx["target"], "acdc")
    got = metrics.SSIM(dim=3)(od.to(DEV), td.to(DEV)).item()
    assert abs(got - fx["ssim3d_acdc"]) <= 1e-5 * abs(fx["ssim3d_acdc"])
    with pytest.raises(ValueError):
        metrics.SSIM(dim=3)(od[:, :, 0].to(DEV), td[:, :, 0].to(DEV))


@pytest.mark.parametrize("fmt", ["pickle", "json"])
def test_cardiac_metrics(tmp_path, fmt):
    fx = load_golden("metrics3d")
    coords = fx["cardiac_coords"]
    path = tmp_path / f"coords.{fmt}"
    if fmt == "pickle":  # the reference's own format (metrics.py:123-125)
        with open(path, "wb") as fh:
            pickle.dump(dict(coords), fh)
    else:
        import json
        path.write_text(json.dumps({k: list(v) for k, v in coords.items()}))
    o, t = fx["cardiac_out"].to(DEV), fx["cardiac_target"].to(DEV)
    cp, cs = metrics.CardiacPSNR(str(path)), metrics.CardiacSSIM(str(path))
    for name, ref in fx["cardiac"].items():
        assert abs(cp(o, t, name).item() - ref["psnr"]) <= 1e-5 * abs(ref["psnr"]), name
        assert abs(cs(o, t, name).item() - ref["ssim"]) <= 1e-5 * abs(ref["ssim"]), name


_check_ssim = R.check_ssim
_FUSED = dict(zip(("mean", "std"), R.ACDC), denormalize=True)


@pytest.mark.parametrize("shape", R.SSIM3D_SHAPES, ids=SHAPE_IDS)
def test_ssim3d_ramp_fp64(shape):
    """Ramp volumes (varying along D, H and W; their own seed per sample and
    channel) in the three ranges: integer volumes with value_range 255 through
    SSIM(dim=3), [0, 1] floats with value_range 1, and the fused
    denormalize=True path on the screened normalised inputs."""
    c, ch = R.ssim_case(shape), shape[1]
    tol255, tol1 = R.ssim_tol(3, 255), R.ssim_tol(3, 1)
    print(f"{shape}: g255 {c.gap255.max():.2e} g1 {c.gap1.max():.2e}")
    o255, t255 = c.o255.to(DEV), c.t255.to(DEV)
    per = metrics.SSIM(dim=3, channels=ch, size_average=False)(o255, t255)
    _check_ssim("255 module", metrics.SSIM(dim=3, channels=ch)(o255, t255), per, c.ref255, tol255)
    o1, t1 = c.o1.to(DEV), c.t1.to(DEV)
    m, per1 = F.ssim(o1, t1, value_range=1.0)
    _check_ssim("[0,1]", m, per1, c.ref1, tol1)
    assert torch.equal(metrics.SSIM(dim=3, channels=ch, size_average=False, value_range=1)(o1, t1), per1)
    xo, xt = c.x_o.to(DEV), c.x_t.to(DEV)
    m, perf = F.ssim(xo, xt, value_range=255.0, **_FUSED)
    _check_ssim("fused", m, perf, c.ref255, tol255)
    for img, kw in ((o255, {}), (o1, {"value_range": 1.0}), (xo, _FUSED)):
        m, same = F.ssim(img, img, **kw)
        assert (1 - same.cpu().double()).abs().max().item() <= 2.0 ** -22
        assert abs(1 - m.item()) <= 2.0 ** -22


@pytest.mark.parametrize("shape", [(2, 2, 12, 28, 44), (2, 1, 11, 26, 42)], ids=["2x2x12x28x44", "2x1x11x26x42"])
def test_ssim3d_batch_permutation(shape):
    """Samples are independent: swapping the two volumes swaps the per-sample output bitwise."""
    c = R.ssim_case(shape)
    perm = torch.tensor([1, 0])
    for o, t, kw in ((c.o255, c.t255, {}), (c.o1, c.t1, {"value_range": 1.0}), (c.x_o, c.x_t, _FUSED)):
        _, per = F.ssim(o.to(DEV), t.to(DEV), **kw)
        _, per_p = F.ssim(o[perm].to(DEV), t[perm].to(DEV), **kw)
        assert torch.equal(per_p.cpu(), per.cpu()[perm])
        assert per[0].item() != per[1].item()


def test_ssim3d_too_small_raises():
    for shape in ((1, 1, 10, 12, 12), (1, 1, 12, 10, 12), (1, 1, 12, 12, 10)):
        x = torch.zeros(shape, device=DEV)
        with pytest.raises(RuntimeError, match="at least 11"):
            F.ssim(x, x)
        with pytest.raises(RuntimeError, match="at least 11"):
            metrics.SSIM(dim=3)(x, x)


def _ssim3d_abi(o, t, ws, ws_bytes):
    b, c, d, h, w = o.shape
    per = torch.empty(b, dtype=torch.float32, device=o.device)
    m = torch.empty((), dtype=torch.float32, device=o.device)
    rc = N.load().vsrk_ssim3d(o.data_ptr(), t.data_ptr(), b, c, d, h, w, 0, 0.0, 1.0, 255.0, per.data_ptr(),
                              m.data_ptr(), ws.data_ptr(), ws_bytes, N.stream_ptr(o.device))
    return rc, m, per


@pytest.mark.parametrize("shape", R.SSIM3D_SHAPES, ids=SHAPE_IDS)
def test_ssim3d_workspace(shape, monkeypatch):
    """vsrk_ssim3d_workspace_size is the depth-filtered moments (5 fp32 planes
    per output depth, padded to 256 bytes) plus one double per tile; it is what
    F.ssim allocates; exactly that much is enough, and one byte less is
    rejected through the ABI with an error text before anything is launched."""
    lib = N.load()
    b, c, d, h, w = shape
    dout = d - 10
    tiles = -(-(w - 10) // R.SSIM_TX) * -(-(h - 10) // R.SSIM_TY)
    want = -(-(b * c * dout * 5 * h * w * 4) // 256) * 256 + b * c * dout * tiles * 8
    need = lib.vsrk_ssim3d_workspace_size(b, c, d, h, w)
    assert need == want
    case = R.ssim_case(shape)
    o, t = case.o255.to(DEV), case.t255.to(DEV)
    sizes = []
    real_empty = torch.empty

    def spy(*a, **kw):
        if kw.get("dtype") == torch.uint8:
            sizes.append(a[0])
        return real_empty(*a, **kw)

    monkeypatch.setattr(F.torch, "empty", spy)
    m_ref, per_ref = F.ssim(o, t)
    monkeypatch.undo()
    assert sizes == [need]
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc, m, per = _ssim3d_abi(o, t, ws, need)
    assert rc == 0
    assert torch.equal(per, per_ref) and m.item() == m_ref.item()
    rc, m, per = _ssim3d_abi(o, t, ws, need - 1)  # the buffer itself stays full-sized
    assert rc != 0
    msg = lib.vsrk_last_error().decode()
    assert "workspace" in msg and str(need) in msg and str(need - 1) in msg, msg
    with pytest.raises(RuntimeError, match="workspace"):
        N.check(rc, "ssim3d")
