"""RBPNet without a device.

* The restatement tests/rbp_ref.py, run in fp64, reproduces the rbp_* fixtures'
  output64 and fp64 gradients (tools/make_golden_rbp.py wrote them after
  asserting the restatement equal to the reference's own RBPNet bit for bit in
  fp32: initial weights, output, loss, every gradient).  fp64 sums differ by
  their order only: 1e-9 relative.
* No fixture holds a zero gradient or a reference fp32 error above 1e-3, and
  rbp_x3_slopes has non-positive slopes on a block tail and on a projection.
* vsr_amd.nets.RBPNet has the restatement's state_dict keys, shapes and seeded
  values, and state_dicts load both ways.
* num_stages != 3 and an unsupported upscale_factor raise at construction; the
  centre index; the caller's list is not mutated (checked on the argument
  handling alone: the forward needs a device).
"""
import inspect

import pytest
import torch
import torch.nn as nn

from tests.conftest import load_golden
from tests.rbp_ref import RBPRef, set_slopes
from tests.test_nets_gpu import _proj
from vsr_amd import nets

GOLDEN = ["rbp_x4_small", "rbp_x2_roll", "rbp_x3_slopes"]
KW = dict(in_channels=1, out_channels=1, base_filter=32, feat=16, num_stages=3, num_resblocks=1, num_frames=3,
          upscale_factor=4)


def _seeded(cls, fx):
    torch.manual_seed(fx["seed"])
    net = cls(**fx["kwargs"]).train()
    if fx["perturbed"]:
        set_slopes(net, fx["slopes"])
    return net


def _check_sums(net, fx):
    sd = net.state_dict()
    assert list(sd) == list(fx["param_sum"])
    for k, v in sd.items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_fixture_fp64(name):
    fx = load_golden(name)
    assert fx["class"] == "RBPNet"
    net = _seeded(RBPRef, fx)
    _check_sums(net, fx)
    net = net.double()
    lr = [x.double() for x in fx["lr"]]
    out = net(lr)
    assert len(lr) == fx["kwargs"]["num_frames"]  # the list is not mutated
    o64 = fx["output64"].double()
    assert out.shape == o64.shape
    assert (out.detach() - o64).abs().max().item() <= 1e-9 * (1 + o64.abs().max().item())
    torch.nn.functional.l1_loss(out, fx["hr"].double()).backward()
    for k, p in net.named_parameters():
        assert fx["grad_norm64"][k] > 0 and fx["ref32_err"][k] is not None and fx["ref32_err"][k] <= 1e-3, k
        g = p.grad
        if k in fx["grad_full64"]:
            ref = fx["grad_full64"][k].double()
            rel = ((g - ref).norm() / ref.norm()).item()
        else:
            e = _proj(g, k, fx["proj_n"]) - fx["grad_proj64"][k]
            rel = e.pow(2).mean().sqrt().item() / fx["grad_norm64"][k]
        assert rel <= 1e-9, (k, rel)


def test_slopes_fixture_has_nonpositive_tail_and_projection_slopes():
    fx = load_golden("rbp_x3_slopes")
    net = _seeded(RBPRef, fx)
    slopes = {k[:-len(".act.weight")]: float(v) for k, v in net.state_dict().items() if k.endswith(".act.weight")}
    assert set(fx["slopes"]) == {0.25, -0.1, 0.0, 1.5}
    assert any(a <= 0 for k, a in slopes.items() if k.startswith("res_feat") and k.split(".")[-1] == "0")
    assert any(a <= 0 for k, a in slopes.items() if "up_conv" in k or "down_conv" in k)


@pytest.mark.parametrize("name", GOLDEN)
def test_same_seed_gives_the_fixture_weights(name):
    fx = load_golden(name)
    _check_sums(_seeded(nets.RBPNet, fx), fx)


def test_constructor_keys_and_state_dicts():
    assert "RBPNet" in nets.__all__ and issubclass(nets.RBPNet, nets.BaseNet)
    assert list(inspect.signature(nets.RBPNet.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "base_filter", "feat", "num_stages", "num_resblocks", "num_frames",
        "upscale_factor"]
    for over in (dict(), dict(upscale_factor=8, num_frames=4, num_resblocks=2), dict(in_channels=2, out_channels=2,
                                                                                    upscale_factor=3)):
        kw = dict(KW, **over)
        torch.manual_seed(7)
        net = nets.RBPNet(**kw)
        torch.manual_seed(7)
        ref = RBPRef(**kw)
        sd, rd = net.state_dict(), ref.state_dict()
        assert list(sd) == list(rd)
        assert all(sd[k].shape == rd[k].shape and torch.equal(sd[k], rd[k]) for k in sd)
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in ref.named_parameters()]
        ref.load_state_dict(sd)
        net.load_state_dict(rd)
    assert {"feat0.conv.weight", "feat1.act.weight", "dbp_net.feat1.conv.bias", "dbp_net.up1.up_conv1.deconv.weight",
            "dbp_net.down2.down_conv3.act.weight", "dbp_net.output.conv.weight", "res_feat1.0.conv2.bias",
            "res_feat1.1.deconv.weight", "res_feat2.0.act.weight", "res_feat2.1.conv.weight",
            "res_feat3.1.conv.weight", "output.conv.bias"} <= set(sd)
    assert all(float(m.weight) == 0.25 for m in net.modules() if isinstance(m, nn.PReLU))


@pytest.mark.parametrize("over,match", [(dict(num_stages=2), "num_stages"), (dict(upscale_factor=5), "upscale")])
def test_constructor_errors(over, match):
    with pytest.raises(ValueError, match=match):
        nets.RBPNet(**dict(KW, **over))


@pytest.mark.parametrize("n,t", [(3, 1), (4, 1), (7, 3)])
def test_centre_index(n, t):
    assert nets.RBPNet(**dict(KW, num_frames=n)).t == t
    assert RBPRef(**dict(KW, num_frames=n)).t == t


def test_callers_list_is_not_mutated():
    """_run copies the list before it takes the centre frame out; a wrong
    frame count is refused before anything is launched."""
    net = nets.RBPNet(**KW)
    frames = [torch.zeros(1, 1, 4, 4) for _ in range(2)]
    with pytest.raises(ValueError, match="3 frames"):
        net._run(frames, None)
    assert len(frames) == 2  # (tests/test_rbp_gpu.py checks the same after a real forward)
