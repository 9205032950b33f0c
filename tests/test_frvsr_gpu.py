"""FRVSRNet on the GPU.

Golden runs: the frvsr_* fixtures (tools/make_golden_frvsr.py: the reference's
own FRVSRNet, with the restatement pinned to it bit for bit) in fp32 / bf16 /
fp16 under test_nets_gpu.test_net_matches_golden's rules -- both output lists
against the fp64 run, PSNR, every parameter gradient against fp64 (in full or
by its 16 projections) at max(1e-4, 3 ref32_err) in fp32, max(5e-2, 2 bf16_env)
in bf16, max(3e-2, 3 fp16_env) in fp16 -- one Adam step against
adam_update_*, and the no_grad / is_prediction outputs against output_eval.

Variants: against the stock-torch restatement tests/frvsr_ref.py run in
fp64: both output lists and every parameter gradient of the FRVSR trainers'
loss, mean_t L1(lr'_t, lr_t) + mean_t L1(sr_t, hr_t).

Bound, as for the SRFB variants (test_srfb_gpu.py): max(1e-4, 3 x the
restatement's own fp32 error against its fp64 run) -- on the outputs as
max|d|, per parameter as rel-L2.  The cases have no searched seed: a ReLU
input, a pool tie or a warp position within fp32 rounding of a kink shows in
the restatement's own fp32 error too, which is why the bound follows it.
"""
import pytest
import torch

from tests import frvsr_ref
from tests import test_nets_gpu as tn
from tests.conftest import load_golden
from tests.frvsr_ref import FRVSRRef
from vsr_amd import nets

pytestmark = pytest.mark.gpu
DEV = "cuda"

BASE = dict(in_channels=1, out_channels=1, upscale_factor=4, num_resblocks=2)
VARIANTS = {  # kwargs, (N, T, C, H, W)
    "small": (BASE, (2, 3, 1, 8, 16)),
    "pad": (dict(BASE, num_resblocks=1), (1, 2, 1, 6, 10)),  # H, W no multiples of 8: pad with the minimum, crop
    "two_channels": (dict(BASE, in_channels=2, out_channels=2, num_resblocks=1), (1, 2, 2, 8, 8)),
    "one_frame": (dict(BASE, num_resblocks=1), (2, 1, 1, 8, 8)),
    "batch3": (dict(BASE, num_resblocks=1), (3, 2, 1, 8, 8)),
}


def _data(shape, seed):
    n, t, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    lr = [torch.randn((n, c, h, w), generator=g) for _ in range(t)]
    hr = [torch.randn((n, c, 4 * h, 4 * w), generator=g) for _ in range(t)]
    return lr, hr


def _flat(out):
    return torch.cat([t.flatten() for part in out for t in part])


def _reference(kw, shape, seed):
    """(fp64 outputs, fp64 gradients, the restatement's fp32 output error and per-parameter gradient error)."""
    lr, hr = _data(shape, seed + 1)
    runs = {}
    for dt in (torch.float64, torch.float32):
        torch.manual_seed(seed)
        m = FRVSRRef(**kw).to(dt).train()
        x, y = [t.to(dt) for t in lr], [t.to(dt) for t in hr]
        out = m(x)
        frvsr_ref.loss(out, x, y).backward()
        runs[dt] = (_flat(out).detach().double(), {k: p.grad.double() for k, p in m.named_parameters()})
    o64, g64 = runs[torch.float64]
    o32, g32 = runs[torch.float32]
    err = {k: ((g32[k] - v).norm() / v.norm()).item() for k, v in g64.items()}
    return o64, g64, (o32 - o64).abs().max().item(), err


def _hip(kw, shape, seed, precision="fp32"):
    lr, hr = _data(shape, seed + 1)
    torch.manual_seed(seed)
    net = nets.FRVSRNet(**kw).to(DEV).set_precision(precision).train()
    x, y = [t.to(DEV) for t in lr], [t.to(DEV) for t in hr]
    out = net(x)
    frvsr_ref.loss(out, x, y).backward()
    torch.cuda.synchronize()
    return net, out


GOLDEN = ["frvsr_x4_small", "frvsr_x4_pad"]


def _golden_step(fx, precision):
    net = tn._build(fx, precision)  # seeded: the fixture's param_sum is checked there
    assert list(net.state_dict()) == list(fx["param_sum"])
    lr, hr = tn._to(fx["lr"]), tn._to(fx["hr"])
    out = net(lr)
    loss = frvsr_ref.loss(out, lr, hr)
    loss.backward()
    torch.cuda.synchronize()
    return net, out, loss, hr


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", GOLDEN)
def test_net_matches_golden(name, precision):
    fx = load_golden(name)
    net, out, loss, hr = _golden_step(fx, precision)
    got, exp = _flat(out).detach().cpu().double(), _flat(fx["output64"]).double()
    d = (got - exp).abs()
    print(f"{name} {precision}: out max|d| {d.max().item():.2e} mean {d.mean().item():.2e} "
          f"(reference fp32 {fx['out_err32']:.2e})")
    if precision == "fp32":
        assert d.max().item() <= max(1e-4, 3 * fx["out_err32"]), d.max().item()
        assert abs(loss.item() - fx["loss"]) <= 1e-5 * (1 + abs(fx["loss"]))
    elif precision == "fp16":
        assert d.max().item() <= 5e-3 and d.mean().item() <= 5e-4, (d.max().item(), d.mean().item())
    else:
        assert d.max().item() <= 3e-2 and d.mean().item() <= 3e-3, (d.max().item(), d.mean().item())
    assert abs(tn._psnr([o.detach() for o in out[0]], hr).item() - fx["psnr_acdc"]) <= 0.01
    gmax = fx["grad_max64"]
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach().cpu().double()
        r32 = fx["ref32_err"][k]
        if r32 is None:  # exact gradient is zero
            assert g.norm().item() <= {"fp32": 1e-4, "fp16": 3e-3}.get(precision, 2e-2) * gmax, (k, g.norm().item())
            continue
        rel = tn._rel(g, fx, k)
        if precision == "fp32":
            tol = max(1e-4, 3 * r32)
        elif precision == "fp16":
            tol = max(3e-2, 3 * fx["fp16_env"][k])
        else:
            tol = max(5e-2, 2 * fx["bf16_env"][k])
        print(f"  {k}: rel {rel:.2e} tol {tol:.2e}")
        assert rel <= tol, (k, rel, tol)
    if precision == "fp16":
        assert net.step_ok()


@pytest.mark.parametrize("name", GOLDEN)
def test_adam_step_on_hip_gradients(name):
    """test_nets_gpu.test_adam_step_on_hip_gradients' check: one Adam step on the
    fp32 HIP gradients reproduces the reference's update, rel-L2 <= 1e-3."""
    fx = load_golden(name)
    net, _, _, _ = _golden_step(fx, "fp32")
    a = fx["adam"]
    opt = torch.optim.Adam(net.parameters(), lr=a["lr"], betas=tuple(a["betas"]), eps=a["eps"])
    p0 = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    for k, p in net.named_parameters():
        if fx["ref32_err"][k] is None:
            continue
        upd = (p.detach() - p0[k]).cpu().double()
        if k in fx["adam_update_full"] and k in fx["grad_full64"]:
            gref, uref = fx["grad_full64"][k].double(), fx["adam_update_full"][k].double()
            keep = gref.abs() > 1e-6 * gref.abs().max()
            assert (upd.abs() <= a["lr"] * 1.001).all(), k
            rel = ((upd - uref)[keep].norm() / uref[keep].norm()).item()
        else:
            rel = tn._rel(upd, fx, k, "adam_update_full", "adam_update_proj", "adam_update_norm")
        print(f"  {k}: update rel {rel:.2e}")
        assert rel <= 1e-3, (k, rel)


@pytest.mark.parametrize("name", GOLDEN)
def test_eval_outputs_match_golden(name):
    """no_grad in eval mode gives the fixture's output_eval (the reference's fp32
    outputs: the fp32 output bound); is_prediction returns the SR frames alone."""
    fx = load_golden(name)
    net = tn._build(fx, "fp32").eval()
    lr = tn._to(fx["lr"])
    with torch.no_grad():
        out = net(lr)
        net.is_prediction = True
        pred = net(lr)
    exp = _flat(fx["output_eval"]).double()
    d = (_flat(out).cpu().double() - exp).abs().max().item()
    assert d <= max(1e-4, 3 * fx["out_err32"]), d
    assert isinstance(pred, list) and len(pred) == len(fx["output_eval"][0])
    assert all(torch.equal(a, b) for a, b in zip(pred, out[0]))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_matches_restatement_fp32(variant):
    kw, shape = VARIANTS[variant]
    o64, g64, out_err32, ref32_err = _reference(kw, shape, 11)
    net, out = _hip(kw, shape, 11)
    assert len(out) == 2 and len(out[0]) == len(out[1]) == shape[1]
    assert out[0][0].shape == (shape[0], shape[2], 4 * shape[3], 4 * shape[4]) and out[1][0].shape[-2:] == shape[3:]
    d = (_flat(out).detach().cpu().double() - o64).abs().max().item()
    print(f"{variant}: out max|d| {d:.2e} (restatement fp32 {out_err32:.2e})")
    assert d <= max(1e-4, 3 * out_err32), d
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        rel = ((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm()).item()
        print(f"  {k}: rel {rel:.2e} (restatement fp32 {ref32_err[k]:.2e})")
        assert rel <= max(1e-4, 3 * ref32_err[k]), (k, rel, ref32_err[k])


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_sixteen_bit_runs_close_to_fp64(precision):
    """16-bit storage: finite gradients for every parameter, outputs within the
    golden tests' 16-bit output figures of the fp64 run (test_nets_gpu.py's
    test_net_matches_golden: max 3e-2 / mean 3e-3 bf16, max 5e-3 / mean 5e-4 fp16)."""
    kw, shape = VARIANTS["small"]
    o64, g64, _, _ = _reference(kw, shape, 11)
    net, out = _hip(kw, shape, 11, precision)
    d = (_flat(out).detach().cpu().double() - o64).abs()
    mx, mean = (3e-2, 3e-3) if precision == "bf16" else (5e-3, 5e-4)
    print(f"{precision}: out max|d| {d.max().item():.2e} mean {d.mean().item():.2e}")
    assert d.max().item() <= mx and d.mean().item() <= mean, (d.max().item(), d.mean().item())
    assert net.step_ok()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


def test_no_grad_and_prediction_outputs():
    kw, shape = VARIANTS["small"]
    net, out = _hip(kw, shape, 11)
    lr, _ = _data(shape, 12)
    x = [t.to(DEV) for t in lr]
    with torch.no_grad():
        sr, lrw = net(x)
    assert all(torch.equal(a, b.detach()) for a, b in zip(sr + lrw, out[0] + out[1]))
    net.is_prediction = True
    net.eval()
    with torch.no_grad():
        pred = net(x)
    assert isinstance(pred, list) and all(torch.equal(a, b) for a, b in zip(pred, sr))


def test_seeded_bf16_training_is_reproducible():
    kw, shape = VARIANTS["small"]
    lr, hr = _data(shape, 5)
    x, y = [t.to(DEV) for t in lr], [t.to(DEV) for t in hr]
    ends = []
    for _ in range(2):
        torch.manual_seed(3)
        net = nets.FRVSRNet(**kw).to(DEV).set_precision("bf16").train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        for _ in range(3):
            opt.zero_grad()
            frvsr_ref.loss(net(x), x, y).backward()
            opt.step()
        ends.append(torch.cat([p.detach().flatten() for p in net.parameters()]))
    assert torch.equal(ends[0], ends[1])


def test_other_upscale_factors_raise():
    net = nets.FRVSRNet(in_channels=1, out_channels=1, upscale_factor=2, num_resblocks=1).to(DEV)
    with pytest.raises(ValueError, match="x4"):
        net([torch.zeros((1, 1, 8, 8), device=DEV)])
