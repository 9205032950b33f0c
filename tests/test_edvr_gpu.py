"""EDVRNet on the GPU.

Golden runs: the edvr_* fixtures (tools/make_golden_edvr.py: the reference's
own EDVRNet around a DCN pinned to its source, with the restatement equal to
it bit for bit) in fp32 / bf16 / fp16 under test_nets_gpu.test_net_matches_golden's
rules -- the output against the fp64 run (fp32 max(1e-4, 3 x the reference's
fp32 error); bf16 max 3e-2 / mean 3e-3; fp16 max 5e-3 / mean 5e-4), PSNR
within 0.01 dB, every parameter gradient against fp64 (in full or by its 16
projections) at max(1e-4, 3 ref32_err) in fp32, max(5e-2, 2 bf16_env) in bf16,
max(3e-2, 3 fp16_env) in fp16 -- one Adam step against adam_update_* at 1e-3,
and the no_grad output against output_eval.  No parameter is skipped:
edvr_x4_offsets is the case where deformable sampling and the offset and mask
gradients carry signal.

Variants: against the stock-torch restatement tests/edvr_ref.py run in fp64,
each with perturbed offset convs, at max(1e-4, 3 x the restatement's own fp32
error against its fp64 run) -- the output as max|d|, per parameter as rel-L2.

The forward is bitwise equal between two calls.  Gradients are not asserted
bitwise equal: the DCN input gradient is a float-atomic scatter.
"""
import pytest
import torch

from tests import test_nets_gpu as tn
from tests.conftest import load_golden
from tests.edvr_ref import EDVRRef, perturb_offset_convs
from vsr_amd import nets

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = ["edvr_x4_small", "edvr_x4_offsets", "edvr_x4_pad"]

BASE = dict(in_channels=1, out_channels=1, nf=16, nframes=3, groups=2, front_RBs=1, back_RBs=1)
VARIANTS = {  # kwargs, (B, N, C, H, W)
    "no_tsa": (dict(BASE, w_TSA=False), (2, 3, 1, 8, 12)),
    "two_channels": (dict(BASE, in_channels=2, out_channels=2), (1, 3, 2, 8, 8)),
    "five_frames_center1": (dict(BASE, nframes=5, center=1), (1, 5, 1, 8, 8)),
    "batch3": (BASE, (3, 3, 1, 8, 8)),
}
SCALE = 0.5  # perturb_offset_convs' scale for the variants (the fixtures store their own)


def _build(fx, precision):
    torch.manual_seed(fx["seed"])
    net = nets.EDVRNet(**fx["kwargs"])
    if fx["perturbed"]:
        perturb_offset_convs(net, fx["seed"], fx["perturb_scale"])
    for k, v in net.state_dict().items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k
    return net.to(DEV).set_precision(precision).train()


def _golden_step(fx, precision):
    net = _build(fx, precision)
    lr, hr = tn._to(fx["lr"]), tn._to(fx["hr"])
    out = net(lr)
    loss = torch.nn.functional.l1_loss(out, hr)
    loss.backward()
    torch.cuda.synchronize()
    return net, out, loss, hr


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", GOLDEN)
def test_net_matches_golden(name, precision):
    fx = load_golden(name)
    net, out, loss, hr = _golden_step(fx, precision)
    assert out.shape == fx["output64"].shape
    d = (out.detach().cpu().double() - fx["output64"].double()).abs()
    print(f"{name} {precision}: out max|d| {d.max().item():.2e} mean {d.mean().item():.2e} "
          f"(reference fp32 {fx['out_err32']:.2e})")
    if precision == "fp32":
        assert d.max().item() <= max(1e-4, 3 * fx["out_err32"]), d.max().item()
        assert abs(loss.item() - fx["loss"]) <= 1e-5 * (1 + abs(fx["loss"]))
    elif precision == "fp16":
        assert d.max().item() <= 5e-3 and d.mean().item() <= 5e-4, (d.max().item(), d.mean().item())
    else:
        assert d.max().item() <= 3e-2 and d.mean().item() <= 3e-3, (d.max().item(), d.mean().item())
    assert abs(tn._psnr(out.detach(), hr).item() - fx["psnr_acdc"]) <= 0.01
    bad = []
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach().cpu().double()
        r32 = fx["ref32_err"][k]
        if r32 is None:  # exact gradient zero: the offset branch behind a zeroed conv_offset_mask (initial weights only)
            assert not fx["perturbed"] and "offset_conv" in k, k  # no parameter of the perturbed cases is skipped
            assert g.norm().item() <= {"fp32": 1e-4, "fp16": 3e-3}.get(precision, 2e-2) * fx["grad_max64"], k
            continue
        rel = tn._rel(g, fx, k)
        if precision == "fp32":
            tol = max(1e-4, 3 * r32)
        elif precision == "fp16":
            tol = max(3e-2, 3 * fx["fp16_env"][k])
        else:
            tol = max(5e-2, 2 * fx["bf16_env"][k])
        print(f"  {k}: rel {rel:.2e} tol {tol:.2e}")
        if not rel <= tol:
            bad.append((k, rel, tol))
    assert not bad, bad
    if precision == "fp16":
        assert net.step_ok()


@pytest.mark.parametrize("name", GOLDEN)
def test_adam_step_on_hip_gradients(name):
    """One Adam step on the fp32 HIP gradients reproduces the reference's update, rel-L2 <= 1e-3."""
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
def test_eval_output_matches_golden_and_forward_is_bitwise(name):
    fx = load_golden(name)
    net = _build(fx, "fp32").eval()
    lr = tn._to(fx["lr"])
    with torch.no_grad():
        out, again = net(lr), net(lr)
    d = (out.cpu().double() - fx["output_eval"].double()).abs().max().item()
    assert d <= max(1e-4, 3 * fx["out_err32"]), d
    assert torch.equal(out, again)
    net.train()
    assert torch.equal(net(lr).detach(), out)  # the taped forward is the same computation


def _data(shape, seed):
    b, n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((b, c, h, w), generator=g) for _ in range(n)], torch.randn((b, c, 4 * h, 4 * w), generator=g)


def _make(cls, kw, seed):
    torch.manual_seed(seed)
    return perturb_offset_convs(cls(**kw), seed, SCALE)


def _reference(kw, shape, seed):
    lr, hr = _data(shape, seed + 1)
    runs = {}
    for dt in (torch.float64, torch.float32):
        m = _make(EDVRRef, kw, seed).to(dt).train()
        out = m([t.to(dt) for t in lr])
        torch.nn.functional.l1_loss(out, hr.to(dt)).backward()
        runs[dt] = (out.detach().double(), {k: p.grad.double() for k, p in m.named_parameters()})
    o64, g64 = runs[torch.float64]
    o32, g32 = runs[torch.float32]
    err = {k: ((g32[k] - v).norm() / v.norm()).item() for k, v in g64.items()}
    return o64, g64, (o32 - o64).abs().max().item(), err


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_matches_restatement_fp32(variant):
    kw, shape = VARIANTS[variant]
    o64, g64, out_err32, ref32_err = _reference(kw, shape, 11)
    lr, hr = _data(shape, 12)
    net = _make(nets.EDVRNet, kw, 11).to(DEV).set_precision("fp32").train()
    out = net([t.to(DEV) for t in lr])
    torch.nn.functional.l1_loss(out, hr.to(DEV)).backward()
    torch.cuda.synchronize()
    assert out.shape == o64.shape
    d = (out.detach().cpu().double() - o64).abs().max().item()
    print(f"{variant}: out max|d| {d:.2e} (restatement fp32 {out_err32:.2e})")
    assert d <= max(1e-4, 3 * out_err32), d
    bad = []
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        rel = ((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm()).item()
        print(f"  {k}: rel {rel:.2e} (restatement fp32 {ref32_err[k]:.2e})")
        if not rel <= max(1e-4, 3 * ref32_err[k]):
            bad.append((k, rel, ref32_err[k]))
    assert not bad, bad
