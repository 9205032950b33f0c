"""EDVRNet without a device.

* The restatement tests/edvr_ref.py reproduces the three edvr_* fixtures, which
  tools/make_golden_edvr.py wrote from the reference's own EDVRNet after
  asserting the restatement equal to it bit for bit (initial weights, output,
  loss, every gradient): seeded (and, where the fixture says so, perturbed)
  weights by param_sum and keys, the output bitwise at one thread and at the
  default thread count, every gradient within the fixture's ref32_err of the
  fp64 gradient.
* vsr_amd.nets.EDVRNet has the fixtures' state_dict keys and seeded param_sum,
  state_dicts load both ways, predeblur and HR_in raise.
* Both cfg8 files parse and build the net.
"""
import inspect
from pathlib import Path

import pytest
import torch
import yaml

from tests.conftest import load_golden
from tests.edvr_ref import EDVRRef, perturb_offset_convs
from tests.test_nets_gpu import _proj
from vsr_amd import nets

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ["edvr_x4_small", "edvr_x4_offsets", "edvr_x4_pad"]


def _seeded(cls, fx):
    torch.manual_seed(fx["seed"])
    net = cls(**fx["kwargs"]).train()
    if fx["perturbed"]:
        perturb_offset_convs(net, fx["seed"], fx["perturb_scale"])
    return net


def _check_sums(net, fx):
    sd = net.state_dict()
    assert list(sd) == list(fx["param_sum"])
    for k, v in sd.items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_fixture(name):
    """The output bitwise at one thread and at the default thread count.  torch's
    own 1x1 conv (fea_fusion) sums in another order on one thread than on
    several -- in the reference's net as in the restatement, an ulp (9e-8) in
    places -- so no single tensor can be both: the fixture holds the
    reference's output at one thread (output_t1) beside its output at several
    (output), each asserted equal to the restatement's when it was written.
    Like test_frvsr_cpu.py's, the bitwise comparison holds on the kind of host
    the fixtures were written on: torch's CPU convs pick their kernels by
    instruction set.
    A gradient kept as 16 projections only is held to 2 ref32_err, as in
    test_frvsr_cpu.py (the chi-square(16) spread of the estimate)."""
    fx = load_golden(name)
    assert fx["class"] == "EDVRNet" and fx["margin_mult"] == 3.0
    assert min(fx["act_ratio"], fx["pool_ratio"], fx.get("coord_ratio", 3.0)) >= fx["margin_mult"]
    if fx["perturbed"]:
        assert 0.4 <= fx["offset_rms"] <= 0.6 and fx["offset_max"] > 1.0
    else:
        assert fx["offset_rms"] == 0.0
    nthreads = torch.get_num_threads()
    try:
        for nt in (1, nthreads):
            torch.set_num_threads(nt)
            net = _seeded(EDVRRef, fx)
            _check_sums(net, fx)
            out = net(fx["lr"])
            assert torch.equal(out.detach(), fx["output_t1" if nt == 1 else "output"]), nt
    finally:
        torch.set_num_threads(nthreads)
    loss = torch.nn.functional.l1_loss(out, fx["hr"])
    loss.backward()
    assert abs(loss.item() - fx["loss"]) <= 1e-6 * (1 + abs(fx["loss"]))
    for k, p in net.named_parameters():
        r32 = fx["ref32_err"][k]
        g = p.grad.double()
        if r32 is None:  # exact gradient zero: the offset branch behind a zeroed conv_offset_mask (initial weights only)
            assert not fx["perturbed"] and "offset_conv" in k and g.norm().item() <= 1e-9 * fx["grad_max64"], k
            continue
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
    _check_sums(_seeded(nets.EDVRNet, fx), fx)


def test_constructor_keys_and_state_dicts():
    assert "EDVRNet" in nets.__all__ and issubclass(nets.EDVRNet, nets.BaseNet)
    assert list(inspect.signature(nets.EDVRNet.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "nf", "nframes", "groups", "front_RBs", "back_RBs", "center", "predeblur",
        "HR_in", "w_TSA"]
    kw = dict(in_channels=1, out_channels=1, nf=16, nframes=3, groups=2, front_RBs=1, back_RBs=2)
    for extra in (dict(), dict(w_TSA=False)):
        torch.manual_seed(7)
        net = nets.EDVRNet(**kw, **extra)
        torch.manual_seed(7)
        ref = EDVRRef(**kw, **extra)
        sd, rd = net.state_dict(), ref.state_dict()
        assert list(sd) == list(rd)
        assert all(torch.equal(sd[k], rd[k]) for k in sd)
        ref.load_state_dict(sd)
        net.load_state_dict(rd)
    assert {"conv_first.weight", "feature_extraction.0.conv2.bias", "pcd_align.L3_dcnpack.conv_offset_mask.weight",
            "pcd_align.cas_dcnpack.weight", "tsa_fusion.sAtt_add_2.bias", "recon_trunk.1.conv1.weight",
            "conv_last.bias"} <= set(nets.EDVRNet(**kw).state_dict())
    assert all(v.abs().sum() == 0 for k, v in sd.items() if "conv_offset_mask" in k)


def test_reference_defaults_parameter_count():
    n = sum(p.numel() for p in nets.EDVRNet(1, 1).parameters())
    assert 3.2e6 < n < 3.4e6  # nf 64, 8 groups, 5 + 10 blocks, one channel: 3.3 M


@pytest.mark.parametrize("kw", [dict(predeblur=True), dict(HR_in=True)])
def test_unsupported_modes_raise(kw):
    with pytest.raises(NotImplementedError, match=list(kw)[0]):
        nets.EDVRNet(1, 1, nf=16, **kw)


@pytest.mark.parametrize("folder", ["train", "test"])
def test_cfg8_parses_and_builds_the_net(folder):
    cfg = yaml.safe_load((ROOT / "configs" / folder / "cfg8_acdc_misr_edvr_x4.yaml").read_text())
    assert cfg["net"]["name"] == "EDVRNet" and cfg["precision"] == "bf16"
    assert cfg["dataset"]["name"] == "AcdcMISRDataset" and cfg["dataset"]["kwargs"]["num_frames"] == 5
    if folder == "train":
        assert cfg["trainer"]["name"] == "AcdcMISRTrainer" and cfg["dataset"]["kwargs"]["temporal_order"] == "middle"
    else:
        assert cfg["predictor"]["name"] == "AcdcMISRPredictor"
    kw = cfg["net"]["kwargs"]
    assert (kw["nf"], kw["groups"], kw["front_RBs"], kw["back_RBs"], kw["nframes"]) == (64, 8, 5, 10, 5)
    net = getattr(nets, cfg["net"]["name"])(**kw)
    assert isinstance(net, nets.EDVRNet) and net.center == 2 and net.w_TSA
