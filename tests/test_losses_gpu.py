"""Loss kernels (vsrk_loss_fwd / vsrk_loss_bwd) two ways.

Against the reference's own values: tests/golden/metrics.pt holds
torch.nn.L1Loss / MSELoss and the reference's HuberLoss(delta=0.7) /
CharbonnierLoss(1e-3) (src/model/losses.py:5-34) evaluated on fixed data, with
their input gradients (oracle/make_golden.py run_metrics).  fp32 kernels with
double-precision partial sums: loss within 1e-6 relative, gradient within
1e-6 relative of its max (the gradient of a mean is O(1/count)).

Against fp64 (tests/metrics_ref.py) through F.loss_fwd / F.loss_bwd, at the
counts where the launch changes shape: one lane, either side of a 256-lane
block, either side of one block's 2048 elements, and 2^21 + 3, which is past
the forward's cap of 1024 blocks (1024 partials: four laps of loss_final) and
past the backward's 4096 x 256 lanes.  Bounds:
  loss      |loss - ref| <= 8 * 2^-24 * ref.  Every term is at most ~6 fp32
            roundings (each 2^-24 relative) of positive quantities, the sums
            are double, and there is one cast to fp32 at the end.
  gradient  per element |g - ref| <= 8 * 2^-24 |ref| + h |ref|, h = 0 / 2^-8 /
            2^-11 for an fp32 / bf16 / fp16 result: the arithmetic (d, d^2,
            + eps, sqrt, divide, gscale / count, the product: <= 7 roundings)
            plus half an ulp of the storage type.  For fp16 the storage term
            is max(2^-11 |ref|, 2^-25): gradients of a mean are O(1/count) and
            fall below fp16's smallest normal 2^-14, where the spacing is the
            fixed 2^-24 and half an ulp is 2^-25 absolute, whatever |ref| is.
            No element is excluded; a NaN is a violation.
The dense cases cannot see one dropped element in a mean of 2^21, so the
localised cases have out == target except at block, lap and tail indices:
for L1 / MSE / Huber only those terms contribute and the gradient must be
exactly 0 elsewhere.  Kinks (d = 0, |d| = delta and one fp32 step to either
side) are compared with fp64 autograd of the reference formulation.
Measured on an MI355X the loss used at most 0.18 of its bound.
"""
import pytest
import torch

from tests import metrics_ref as R
from tests.conftest import load_golden
from vsr_amd import functional as F
from vsr_amd import losses

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPECS = range(len(R.LOSS_SPECS))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _make(name, params):
    if name == "HuberLoss":
        return losses.HuberLoss(delta=params[name])
    if name == "CharbonnierLoss":
        return losses.CharbonnierLoss(epsilon=params[name])
    return getattr(losses, name)()


@pytest.mark.parametrize("name", ["L1Loss", "MSELoss", "HuberLoss", "CharbonnierLoss"])
def test_loss_matches_reference(name):
    fx = load_golden("metrics")
    fn = _make(name, fx["loss_params"])
    o = fx["out"].to(DEV).requires_grad_(True)
    t = fx["target"].to(DEV)
    val = fn(o, t)
    val.backward()
    ref = fx["loss"][name]
    assert abs(val.item() - ref) <= 1e-6 * max(1.0, abs(ref)), (name, val.item(), ref)
    g, gr = o.grad.cpu(), fx["grad"][name]
    assert (g - gr).abs().max().item() <= 1e-6 * gr.abs().max().item() + 1e-12, name


@pytest.mark.parametrize("name", ["L1Loss", "MSELoss"])
def test_loss_upstream_gradient_scale(name):
    """backward multiplies by the upstream gradient (weighted loss sums, base_trainer.py:126)."""
    fx = load_golden("metrics")
    fn = _make(name, fx["loss_params"])
    o = fx["out"].to(DEV).requires_grad_(True)
    (0.25 * fn(o, fx["target"].to(DEV))).backward()
    assert torch.allclose(o.grad.cpu(), 0.25 * fx["grad"][name], rtol=1e-5, atol=1e-12)


def _check_loss(case, o, t, tag):
    got = F.loss_fwd(case.kind, case.p, o, t).item()
    print(f"{tag}: loss {got!r} ref {case.loss!r} err/bound "
          f"{abs(got - case.loss) / max(R.loss_bound(case.loss), 1e-300):.3f}")
    assert abs(got - case.loss) <= R.loss_bound(case.loss), (tag, got, case.loss)


def _check_grad(case, o, t, gscale, dtype, tag):
    gs = None if gscale is None else torch.tensor(gscale, device=DEV)
    g = F.loss_bwd(case.kind, case.p, o, t, gs, dtype)
    assert g.dtype == dtype and g.shape == o.shape
    ref = case.grad * (1.0 if gscale is None else R.f32(gscale))
    bad = R.grad_violations(g, ref, dtype)
    assert bad == 0, (tag, gscale, dtype, bad)
    return g


@pytest.mark.parametrize("count", R.LOSS_COUNTS)
@pytest.mark.parametrize("spec", SPECS, ids=R.LOSS_SPEC_IDS)
def test_loss_dense_fp64(spec, count):
    """randn inputs: loss and the fp32 gradient (no gscale pointer) at every count."""
    case = R.loss_case(spec, count)
    o, t = case.o.to(DEV), case.t.to(DEV)
    _check_loss(case, o, t, f"dense {R.LOSS_SPEC_IDS[spec]} n={count}")
    _check_grad(case, o, t, None, torch.float32, "dense")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("spec", SPECS, ids=R.LOSS_SPEC_IDS)
def test_loss_bwd_gscale_and_dtype(spec, dtype):
    """Every kind x result dtype x upstream scale (None at the ABI, 1, 0.25,
    -3, 0) at every count; gscale 0 has bound 0, i.e. the gradient is 0."""
    for count in R.LOSS_COUNTS:
        case = R.loss_case(spec, count)
        o, t = case.o.to(DEV), case.t.to(DEV)
        for gscale in R.LOSS_GSCALES:
            g = _check_grad(case, o, t, gscale, dtype, f"n={count}")
            if gscale == 0.0:
                assert not bool(g.any()), (count, dtype)


@pytest.mark.parametrize("count", R.LOSS_LOCALISED_COUNTS)
@pytest.mark.parametrize("spec", SPECS, ids=R.LOSS_SPEC_IDS)
def test_loss_localised_fp64(spec, count):
    """out == target except at indices 0, 255, 256, 2^20 - 1, 2^20, 2^21 - 1,
    2^21, count - 1 (those that exist), each off by its own power of two.
    A dropped or doubled element is at least 2^-3 / 32 of the L1 / MSE / Huber
    sum.  Charbonnier keeps its sqrt(eps) floor per element (gradient 0 / sqrt(eps)
    = 0 there), so it is checked against the reference like the dense case."""
    case = R.loss_case(spec, count, True)
    o, t = case.o.to(DEV), case.t.to(DEV)
    _check_loss(case, o, t, f"localised {R.LOSS_SPEC_IDS[spec]} n={count}")
    for dtype in DTYPES:
        g = _check_grad(case, o, t, None, dtype, "localised").cpu()
        if case.kind != 3:
            g[case.idx] = 0
            assert bool((g == 0).all()), (dtype, int((g != 0).sum()))
            assert bool((case.grad[case.idx] != 0).all())


@pytest.mark.parametrize("spec", SPECS, ids=R.LOSS_SPEC_IDS)
def test_loss_kinks_fp64(spec):
    """target 0 and out in {0, +-delta, +-one fp32 step either side of delta}
    for delta 0.75 and float32(0.7): fp64 autograd of the reference
    formulation (torch.min(|d|, delta), whose tie gradient sums to delta);
    the gradient at d = 0 is exactly 0 for every kind."""
    o, t = R.loss_kink_points()
    _, kind, p = R.LOSS_SPECS[spec]
    loss, grad = R.loss_ref(kind, p, o, t)
    case = R.SimpleNamespace(kind=kind, p=p, loss=loss, grad=grad)
    od, td = o.to(DEV), t.to(DEV)
    _check_loss(case, od, td, f"kinks {R.LOSS_SPEC_IDS[spec]}")
    for dtype in DTYPES:
        g = _check_grad(case, od, td, None, dtype, "kinks")
        assert g[0].item() == 0.0 and grad[0].item() == 0.0
    # every point on its own (count 1): no neighbour to borrow a value from
    for i in range(len(o)):
        one = R.SimpleNamespace(kind=kind, p=p, grad=grad[i:i + 1] * len(o))
        _check_grad(one, od[i:i + 1].clone(), td[i:i + 1].clone(), None, torch.float32, f"kink {i}")


@pytest.mark.parametrize("name", ["L1Loss", "MSELoss", "HuberLoss", "CharbonnierLoss"])
def test_loss_module_bf16_output(name):
    """A bf16 output that requires grad gets a bf16 gradient: the fp32 gradient cast once."""
    fn = _make(name, {"HuberLoss": 0.7, "CharbonnierLoss": 1e-3})
    g = torch.Generator().manual_seed(11)
    o = torch.randn((2, 1, 19, 23), generator=g).to(DEV, torch.bfloat16).requires_grad_(True)
    t = torch.randn((2, 1, 19, 23), generator=g).to(DEV)
    val = fn(o, t)
    assert val.dtype == torch.float32
    (0.5 * val).backward()
    assert o.grad.dtype == torch.bfloat16
    g32 = F.loss_bwd(fn.kind, fn._param(), o.detach().float(), t, torch.tensor(0.5, device=DEV), torch.float32)
    assert torch.equal(o.grad, g32.to(torch.bfloat16))
    ref_loss, ref = R.loss_ref(fn.kind, fn._param(), o.detach().float().cpu(), t.cpu())
    assert abs(val.item() - ref_loss) <= R.loss_bound(ref_loss)
    assert R.grad_violations(o.grad, 0.5 * ref, torch.bfloat16) == 0


@pytest.mark.parametrize("view", ["crop", "permute"])
@pytest.mark.parametrize("name", ["L1Loss", "MSELoss", "HuberLoss", "CharbonnierLoss"])
def test_loss_module_noncontiguous_output(name, view):
    """A cropped or permuted output gives the same loss and gradient as its contiguous copy."""
    fn = _make(name, {"HuberLoss": 0.7, "CharbonnierLoss": 1e-3})
    g = torch.Generator().manual_seed(12)
    base = torch.randn((2, 3, 20, 30), generator=g).to(DEV).requires_grad_(True)
    cut = (lambda x: x[..., 1:-1, 2:-3]) if view == "crop" else (lambda x: x.permute(0, 2, 3, 1))
    v = cut(base)
    assert not v.is_contiguous()
    t = torch.randn(v.shape, generator=g).to(DEV)
    val = fn(v, t)
    val.backward()
    dense = v.detach().contiguous().requires_grad_(True)
    val_c = fn(dense, t)
    val_c.backward()
    assert val.item() == val_c.item()
    assert torch.equal(cut(base.grad), dense.grad)
    outside = base.grad.clone()
    cut(outside).zero_()
    assert not bool(outside.any())
    ref_loss, ref = R.loss_ref(fn.kind, fn._param(), dense.detach().cpu(), t.cpu())
    assert abs(val.item() - ref_loss) <= R.loss_bound(ref_loss)
    assert R.grad_violations(dense.grad, ref, torch.float32) == 0


def test_loss_shape_mismatch_raises():
    o = torch.zeros((2, 1, 8, 8), device=DEV)
    for fn in (losses.L1Loss(), losses.MSELoss(), losses.HuberLoss(0.7), losses.CharbonnierLoss(1e-3)):
        with pytest.raises(ValueError):
            fn(o, torch.zeros((2, 1, 8, 9), device=DEV))
