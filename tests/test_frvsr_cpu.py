"""FRVSRNet without a device.

* The restatement tests/frvsr_ref.py reproduces both frvsr_* fixtures, which
  tools/make_golden_frvsr.py wrote from the reference's own FRVSRNet after
  asserting the restatement equal to it bit for bit (initial weights, both
  output lists, every gradient): seeded initial weights (param_sum, keys),
  both output lists bitwise in fp32, every gradient within the fixture's
  ref32_err of the fp64 gradient.
* vsr_amd.nets.FRVSRNet has the fixture's state_dict keys and seeded
  param_sum, and state_dicts load both ways.
* The net and both trainers resolve by name; the trainers' two losses and log
  keys.
That both cfg7 files build is checked by tests/test_configs_cpu.py, which
globs configs/; the new C entry points and the swap_modules rules by
tests/test_warp_pool_cpu.py."""
import inspect

import pytest
import torch

from tests import frvsr_ref
from tests.conftest import load_golden
from tests.frvsr_ref import FRVSRRef
from tests.test_nets_gpu import _proj
from vsr_amd import nets
from vsr_amd.runner import trainers

KW = dict(in_channels=1, out_channels=1, upscale_factor=4, num_resblocks=2)


def test_net_and_trainers_resolve():
    assert "FRVSRNet" in nets.__all__ and issubclass(nets.FRVSRNet, nets.BaseNet)
    assert list(inspect.signature(nets.FRVSRNet.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "upscale_factor", "is_prediction", "num_resblocks"]
    assert inspect.signature(nets.FRVSRNet.__init__).parameters["num_resblocks"].default == 10
    for name, ds in (("AcdcFRVSRTrainer", "acdc"), ("Dsb15FRVSRTrainer", "dsb15")):
        cls = getattr(trainers, name)
        assert issubclass(cls, trainers.BaseTrainer) and cls.dataset == ds
    assert "not mirrored" not in trainers.__doc__


def test_same_seed_gives_the_restatement_weights():
    torch.manual_seed(1234)
    net = nets.FRVSRNet(**KW)
    torch.manual_seed(1234)
    ref = FRVSRRef(**KW)
    sd, rd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(torch.equal(sd[k], rd[k]) for k in sd)
    want = (["srnet.head.conv"] + [f"srnet.body.{i}.body.conv{j}" for i in range(2) for j in (1, 2)]
            + ["srnet.tail.deconv1", "srnet.tail.deconv2", "srnet.tail.conv"]
            + [f"fnet.body.conv{k}_{j}" for k in range(1, 7) for j in (1, 2)] + ["fnet.tail.conv1", "fnet.tail.conv2"])
    assert list(sd) == [f"{m}.{p}" for m in want for p in ("weight", "bias")]
    n = sum(p.numel() for p in net.parameters())
    assert 1.97e6 < n < 1.99e6  # 1.98 M at two resblocks, FNet 1.74 M of them
    ref.load_state_dict(sd)
    net.load_state_dict(rd)


def test_trainer_losses_and_log_keys():
    """The two loss functions of the FRVSR trainers: warped previous frame
    against the frame, estimate against the target; both under 'L1Loss'."""
    from vsr_amd.losses import L1Loss
    tr = trainers.AcdcFRVSRTrainer.__new__(trainers.AcdcFRVSRTrainer)
    tr.loss_fns, tr.metric_fns = [torch.nn.L1Loss(), torch.nn.L1Loss()], []
    assert list(tr._init_log()) == ["Loss", "L1Loss"]
    lr = [torch.zeros(1, 1, 2, 2), torch.ones(1, 1, 2, 2)]
    hr = [torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8)]
    out = ([h + 3 for h in hr], [x + 1 for x in lr])
    flow_loss, sr_loss = tr._losses(out, lr, hr)
    assert flow_loss.item() == 1.0 and sr_loss.item() == 3.0
    assert tr._logged_outputs(out) is out[0] and tr._frames(lr) == 2
    assert L1Loss.__name__ == "L1Loss"


GOLDEN = ["frvsr_x4_small", "frvsr_x4_pad"]


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_fixture(name):
    """Outputs bitwise (the fixture holds this restatement's own fp32 outputs,
    asserted equal to the reference's); gradients against the fixture's fp64
    gradients at ref32_err, which is the worst of this very computation over
    thread counts and of the noise envelope.  A gradient kept as 16 projections
    only is held to 2 ref32_err: the rms over 16 Gaussian projections
    estimates the rel-L2 error with a chi-square(16) spread, below 1.7 x at
    the 1e-4 quantile."""
    fx = load_golden(name)
    assert fx["class"] == "FRVSRNet" and fx["margin_mult"] == 3.0
    assert min(fx["act_ratio"], fx["pool_ratio"], fx["coord_ratio"]) >= fx["margin_mult"]
    torch.manual_seed(fx["seed"])
    net = FRVSRRef(**fx["kwargs"]).train()
    sd = net.state_dict()
    assert list(sd) == list(fx["param_sum"])
    for k, v in sd.items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k
    out = net(fx["lr"])
    loss = frvsr_ref.loss(out, fx["lr"], fx["hr"])
    loss.backward()
    for got, exp in zip(out, fx["output"]):
        assert len(got) == len(exp)
        for a, b in zip(got, exp):
            assert torch.equal(a.detach(), b)
    assert abs(loss.item() - fx["loss"]) <= 1e-6 * (1 + abs(fx["loss"]))
    for k, p in net.named_parameters():
        r32 = fx["ref32_err"][k]
        assert r32 is not None, k
        g = p.grad.double()
        if k in fx["grad_full64"]:
            ref = fx["grad_full64"][k].double()
            rel, tol = ((g - ref).norm() / ref.norm()).item(), r32
        else:
            e = _proj(g, k, fx["proj_n"]) - fx["grad_proj64"][k]
            rel, tol = e.pow(2).mean().sqrt().item() / fx["grad_norm64"][k], 2 * r32
        assert rel <= tol, (k, rel, tol)


@pytest.mark.parametrize("name", GOLDEN)
def test_same_seed_gives_the_fixture_weights(name):
    fx = load_golden(name)
    torch.manual_seed(fx["seed"])
    net = nets.FRVSRNet(**fx["kwargs"])
    sd = net.state_dict()
    assert list(sd) == list(fx["param_sum"])
    for k, v in sd.items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k
