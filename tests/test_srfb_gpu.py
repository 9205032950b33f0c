"""SRFBNet and Bicubic on the HIP path.

* The srfb_* fixtures (the reference's own SRFBNet, tools/make_golden_srfb.py)
  in fp32 / bf16 / fp16 through test_nets_gpu.test_net_matches_golden itself:
  output, PSNR within 0.01 dB and every gradient (grad_full64 / projections),
  at that test's bounds.
* Shapes of the constructor the fixtures do not cover, and PReLU slopes <= 0,
  in fp32 against tests/srfb_ref.SRFBRef in fp64 on the CPU.  Bounds: the golden
  fp32 rule -- output max|d| <= max(1e-4, 3 out_err32), gradient rel-L2 <=
  max(1e-4, 3 ref32_err) per parameter, with out_err32 / ref32_err the
  restatement's own fp32 CPU error against the same fp64 run; the slope case is
  held to test_drf_prelu_gpu's bound instead (outputs 1e-4, gradients rel-L2
  1e-4, slope gradients 1e-4 of the largest slope gradient).
* Bicubic against tests/golden/bicubic.pt (the reference's Bicubic and an fp64
  evaluation) at 2e-5 of max|ref| in every set_precision mode.
"""
import pytest
import torch
import torch.nn.functional as Fn

import tests.test_nets_gpu as tn
from tests.conftest import load_golden
from tests.srfb_ref import SRFBRef
from vsr_amd import nets

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["srfb_x2_small", "srfb_x3_small", "srfb_x4_canon"]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", CASES)
def test_srfb_matches_golden(name, precision):
    tn.test_net_matches_golden(name, precision)


@pytest.mark.parametrize("name", CASES)
def test_nograd_forward_equals_output_eval(name):
    fx = load_golden(name)
    net = tn._build(fx, "fp32").eval()
    with torch.no_grad():
        out = net(tn._to(fx["lr"]))
    assert isinstance(out, list) and len(out) == fx["kwargs"]["num_steps"]
    d = (tn._flat(out).cpu().double() - tn._flat(fx["output_eval"]).double()).abs().max().item()
    assert d <= max(1e-4, 3 * fx["out_err32"]), d


@pytest.mark.parametrize("name", CASES)
def test_srfb_adam_step(name):
    tn.test_adam_step_on_hip_gradients(name)


def _step(net, x, hr):
    out = net(x)
    torch.stack([Fn.l1_loss(o, hr) for o in out]).mean().backward()
    return [o.detach() for o in out], {k: p.grad.detach() for k, p in net.named_parameters()}


def _against_ref(kw, shape, slopes=None, seed=11):
    """One fp32 HIP train step and the restatement's fp64 / fp32 CPU steps from
    the same weights -> (out, grads, out64, grads64, out_err32, ref32_err)."""
    torch.manual_seed(seed)
    net = nets.SRFBNet(**kw)
    if slopes:
        with torch.no_grad():
            for name, a in slopes.items():
                net.get_submodule(name).weight.fill_(a)
    g = torch.Generator().manual_seed(seed + 1)
    r = kw["upscale_factor"]
    x = torch.randn(shape, generator=g)
    hr = torch.randn((shape[0], kw["out_channels"], shape[2] * r, shape[3] * r), generator=g)
    ref64 = SRFBRef(**kw).double().train()
    ref64.load_state_dict(net.state_dict())
    out64, g64 = _step(ref64, x.double(), hr.double())
    ref32 = SRFBRef(**kw).train()
    ref32.load_state_dict(net.state_dict())
    out32, g32 = _step(ref32, x, hr)
    out_err32 = (tn._flat(out32).double() - tn._flat(out64)).abs().max().item()
    ref32_err = {k: (g32[k].double() - v).norm().item() / v.norm().item() for k, v in g64.items()}
    net = net.to(DEV).set_precision("fp32").train()
    out, gm = _step(net, x.to(DEV), hr.to(DEV))
    torch.cuda.synchronize()
    assert len(out) == kw["num_steps"] and all(o.shape == hr.shape for o in out)
    return out, gm, out64, g64, out_err32, ref32_err


VARIANTS = {
    "one_step": (dict(in_channels=1, out_channels=1, num_steps=1, num_features=16, num_groups=2, upscale_factor=2),
                 (2, 1, 8, 8)),
    "one_group": (dict(in_channels=1, out_channels=1, num_steps=2, num_features=16, num_groups=1, upscale_factor=4),
                  (1, 1, 5, 7)),
    "two_channels": (dict(in_channels=2, out_channels=2, num_steps=2, num_features=16, num_groups=2,
                          upscale_factor=3), (2, 2, 5, 6)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_srfb_variants_match_restatement(variant):
    kw, shape = VARIANTS[variant]
    out, gm, out64, g64, out_err32, ref32_err = _against_ref(kw, shape)
    d = (tn._flat(out).cpu().double() - tn._flat(out64)).abs().max().item()
    print(f"{variant}: out max|d| {d:.2e} (reference fp32 {out_err32:.2e})")
    assert d <= max(1e-4, 3 * out_err32), d
    for k, v in g64.items():
        rel = (gm[k].cpu().double() - v).norm().item() / v.norm().item()
        print(f"  {k}: rel {rel:.2e} (reference fp32 {ref32_err[k]:.2e})")
        assert rel <= max(1e-4, 3 * ref32_err[k]), (k, rel, ref32_err[k])


def test_srfb_nonpositive_slopes():
    """r_block.prelu1 with slope -0.1 and lrf_block.prelu2 with slope 0: both
    take the pre-activation backward (test_drf_prelu_gpu's bound)."""
    kw = dict(in_channels=1, out_channels=1, num_steps=2, num_features=16, num_groups=2, upscale_factor=4)
    out, gm, out64, g64, _, _ = _against_ref(kw, (2, 1, 6, 8),
                                             slopes={"r_block.prelu1": -0.1, "lrf_block.prelu2": 0.0})
    d = (tn._flat(out).cpu().double() - tn._flat(out64)).abs().max().item()
    assert d <= 1e-4, d
    smax = max(v.abs().item() for v in g64.values() if v.numel() == 1)
    for k, v in g64.items():
        got = gm[k].cpu().double()
        assert torch.isfinite(got).all(), k
        if v.numel() == 1:  # PReLU slope gradients
            print(f"  {k}: |d| {(got - v).abs().item():.2e} of {smax:.2e}")
            assert (got - v).abs().item() <= 1e-4 * smax, (k, got.item(), v.item())
        else:
            rel = (got - v).norm().item() / max(v.norm().item(), 1e-30)
            print(f"  {k}: rel {rel:.2e}")
            assert rel <= 1e-4, (k, rel)


def test_srfb_skip_modes_agree():
    """The two ways of folding the bilinear skip in (per-step accumulate, or
    materialised once and added in the last conv's epilogue) give the same
    outputs to fp32 rounding and the same gradients bitwise."""
    kw, shape = VARIANTS["one_group"]
    res = []
    for mode in ("accumulate", "residual"):
        torch.manual_seed(3)
        net = nets.SRFBNet(**kw).to(DEV).set_precision("fp32").train()
        net.SKIP_MODE = mode
        g = torch.Generator().manual_seed(4)
        x = torch.randn(shape, generator=g).to(DEV)
        hr = torch.randn((1, 1, shape[2] * 4, shape[3] * 4), generator=g).to(DEV)
        res.append(_step(net, x, hr))
    (oa, ga), (ob, gb) = res
    for a, b in zip(oa, ob):
        assert (a - b).abs().max().item() <= 1e-6 * (1 + a.abs().max().item())
    for k in ga:
        assert (ga[k] - gb[k]).norm().item() <= 1e-5 * (gb[k].norm().item() + 1e-30), k


def test_srfb_training_is_reproducible():
    """Two seeded three-step Adam runs give bitwise-equal parameters."""
    kw = dict(in_channels=1, out_channels=1, num_steps=2, num_features=16, num_groups=2, upscale_factor=2)
    runs = []
    for _ in range(2):
        torch.manual_seed(21)
        net = nets.SRFBNet(**kw).to(DEV).set_precision("bf16").train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        g = torch.Generator().manual_seed(22)
        for _ in range(3):
            x = torch.randn((2, 1, 12, 10), generator=g).to(DEV)
            hr = torch.randn((2, 1, 24, 20), generator=g).to(DEV)
            opt.zero_grad(set_to_none=True)
            torch.stack([Fn.l1_loss(o, hr) for o in net(x)]).mean().backward()
            opt.step()
        torch.cuda.synchronize()
        runs.append({k: v.detach().clone() for k, v in net.state_dict().items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_srfb_channel_mismatch_raises():
    net = nets.SRFBNet(in_channels=2, out_channels=1, num_steps=1, num_features=16, num_groups=1,
                       upscale_factor=2).to(DEV).set_precision("fp32")
    with pytest.raises(ValueError, match="in_channels"), torch.no_grad():
        net(torch.zeros((1, 2, 4, 4), device=DEV))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_bicubic_matches_reference(precision):
    fx = load_golden("bicubic")
    for r in fx["scales"]:
        net = nets.Bicubic(r).to(DEV).set_precision(precision)
        for x, ref32, ref64 in zip(fx["inputs"], fx["output"][r], fx["output64"][r]):
            y = net(x.to(DEV))
            assert y.dtype == torch.float32 and y.shape == ref64.shape
            for ref in (ref32.double(), ref64):
                err = (y.cpu().double() - ref).abs().max().item()
                assert err <= 2e-5 * ref64.abs().max().item(), (r, tuple(x.shape), err)
