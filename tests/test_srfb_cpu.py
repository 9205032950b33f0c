"""SRFBNet / Bicubic without a device: module tree, state_dict keys and initial
weights of the srfb_* fixtures (made from the reference's own SRFBNet by
tools/make_golden_srfb.py), and the constructor's argument check."""
import pytest
import torch

from tests.conftest import load_golden
from tests.srfb_ref import SRFBRef
from vsr_amd import nets

CASES = ["srfb_x2_small", "srfb_x3_small", "srfb_x4_canon"]


@pytest.mark.parametrize("name", CASES)
def test_same_seed_gives_the_fixture_weights(name):
    fx = load_golden(name)
    assert fx["class"] == "SRFBNet" and fx["kind"] == "sisr_list"
    torch.manual_seed(fx["seed"])
    net = nets.SRFBNet(**fx["kwargs"])
    sd = net.state_dict()
    assert list(sd) == list(fx["param_sum"])  # keys, in creation order
    for k, v in sd.items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k
    assert [k.split(".")[0] for k in sd][::len(sd) - 1] == ["lrf_block", "r_block"]
    assert {"r_block.deconv1.weight", "r_block.prelu1.weight", "r_block.conv2.bias"} <= set(sd)
    # state_dicts load both ways with the stock-torch restatement
    ref = SRFBRef(**fx["kwargs"])
    ref.load_state_dict(sd)
    net.load_state_dict(ref.state_dict())


def test_bad_upscale_factor_raises():
    with pytest.raises(ValueError, match="The upscale factor should be 2, 3, 4 or 8. Got 5."):
        nets.SRFBNet(in_channels=1, out_channels=1, num_steps=2, num_features=8, num_groups=1, upscale_factor=5)


def test_bicubic_has_no_parameters():
    net = nets.Bicubic(4)
    assert not list(net.parameters()) and not net.state_dict()
    assert net.set_precision("bf16") is net
    with pytest.raises(ValueError):
        nets.Bicubic(2.5)
    assert {"SRFBNet", "Bicubic"} <= set(nets.__all__)
