"""EDVRNet and RBPNet under the unchanged MISR trainer and predictor, through
the config surface, on the synthetic NIfTI tree (the reference's on-disk
layout).  Per net (a row of NETS):

* configs/train/<cfg>.yaml (AcdcMISRTrainer + the net + AcdcMISRLogger),
  shrunk through its kwargs (a small crop, 3 frames; EDVR: nf 16, 2 groups,
  one block each; RBP: base_filter 32, feat 16, one block each), trains one
  epoch with finite, ordered logs and writes a checkpoint that loads into a
  fresh net;
* configs/test/<cfg>.yaml (AcdcMISRPredictor) loads that checkpoint, predicts
  and exports."""
import csv
import math
from pathlib import Path

import pytest
import torch
import yaml

from nifti_tree import make_tree
from vsr_amd import config as C
from vsr_amd import nets
from vsr_amd.runner import trainers

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _edvr_grads_arrived(net):
    # the offset convs start at zero and must have moved: their gradients arrived
    return all(p.abs().sum() > 0 for k, p in net.named_parameters() if "conv_offset_mask" in k)


def _rbp_grads_arrived(net):
    # every PReLU starts at 0.25 and must have moved: the slope gradients arrived
    return all(float(p) != 0.25 for k, p in net.named_parameters() if k.endswith("act.weight"))


# (config, net class name, the small kwargs, "gradients arrived", state-dict keys a checkpoint must hold)
NETS = {
    "edvr": ("cfg8_acdc_misr_edvr_x4.yaml", "EDVRNet", dict(nf=16, groups=2, front_RBs=1, back_RBs=1, nframes=3),
             _edvr_grads_arrived,
             {"conv_first.weight", "pcd_align.cas_dcnpack.conv_offset_mask.bias", "tsa_fusion.sAtt_L3.weight",
              "conv_last.bias"}),
    "rbp": ("cfg9_acdc_misr_rbp_x4.yaml", "RBPNet", dict(base_filter=32, feat=16, num_resblocks=1, num_frames=3),
            _rbp_grads_arrived,
            {"feat0.conv.weight", "dbp_net.up1.up_conv1.deconv.weight", "res_feat2.0.act.weight",
             "res_feat3.1.conv.bias", "output.conv.bias"}),
}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("data"), T=4, H=32, W=32, patients=2)


@pytest.mark.parametrize("which", list(NETS))
def test_trains_an_epoch_and_predicts(which, tree, tmp_path):
    cfg_name, net_name, small, grads_arrived, keys = NETS[which]
    net_cls = getattr(nets, net_name)
    cfg = yaml.safe_load((ROOT / "configs" / "train" / cfg_name).read_text())
    assert cfg["net"]["name"] == net_name and cfg["trainer"]["name"] == "AcdcMISRTrainer"
    assert cfg["logger"]["name"] == "AcdcMISRLogger" and cfg["dataset"]["name"] == "AcdcMISRDataset"
    cfg["dataset"]["kwargs"].update(data_dir=str(tree / "videos"), num_frames=3)
    for a in cfg["dataset"]["kwargs"]["augments"]:
        if a["name"] == "RandomCropPatch":
            a["kwargs"]["size"] = [8, 8]
    cfg["main"]["saved_dir"] = str(tmp_path / "out")
    cfg["dataloader"]["kwargs"].update(num_workers=0, train_batch_size=2)
    cfg["net"]["kwargs"].update(small)
    cfg["logger"]["kwargs"]["dummy_input"] = [1, 1, 8, 8]
    cfg["monitor"]["kwargs"]["saved_freq"] = 1
    cfg["trainer"]["kwargs"]["num_epochs"] = 1
    trainer = C.build_train(C.Box(cfg), device="cuda:0")
    assert isinstance(trainer, trainers.AcdcMISRTrainer) and isinstance(trainer.net, net_cls)
    assert trainer.net.compute_dtype == torch.bfloat16
    seen = {}
    write = trainer.logger.write

    def record(epoch, train_log, train_batch, train_outputs, valid_log, valid_batch, valid_outputs):
        seen.update(train=train_log, valid=valid_log, outputs=valid_outputs, batch=valid_batch)
        return write(epoch, train_log, train_batch, train_outputs, valid_log, valid_batch, valid_outputs)

    trainer.logger.write = record
    trainer.train()
    assert list(seen["train"]) == ["Loss", "L1Loss", "PSNR", "SSIM"]
    for log in (seen["train"], seen["valid"]):
        assert all(math.isfinite(v) for v in log.values()) and log["Loss"] > 0, log
    for p in trainer.net.parameters():
        assert torch.isfinite(p).all()
    assert grads_arrived(trainer.net)
    cks = sorted((tmp_path / "out" / "checkpoints").glob("*.pth"))
    assert cks, "no checkpoint written"
    from vsr_amd.callbacks.monitor import safe_globals
    with torch.serialization.safe_globals(safe_globals()):
        ck = torch.load(cks[0], map_location="cpu", weights_only=True)
    fresh = net_cls(**cfg["net"]["kwargs"])
    fresh.load_state_dict(ck["net"])
    assert keys <= set(ck["net"])

    # ---- the test config on that checkpoint
    tcfg = yaml.safe_load((ROOT / "configs" / "test" / cfg_name).read_text())
    assert tcfg["predictor"]["name"] == "AcdcMISRPredictor" and tcfg["net"]["name"] == net_name
    tcfg["dataset"]["kwargs"].update(data_dir=str(tree / "videos"), num_frames=3)
    tcfg["main"].update(saved_dir=str(tmp_path / "pred"), loaded_path=str(cks[0]))
    tcfg["predictor"]["kwargs"].update(saved_dir=str(tmp_path / "pred"))
    tcfg["dataloader"]["kwargs"]["num_workers"] = 0
    tcfg["net"]["kwargs"].update(small)
    pred = C.build_test(C.Box(tcfg), device="cuda:0")
    assert isinstance(pred.net, net_cls)
    log = pred.predict()
    assert all(math.isfinite(v) for v in log.values()), log
    rows = list(csv.reader(open(tmp_path / "pred" / "results.csv")))
    assert rows[0][0] == "name" and len(rows) > 1
