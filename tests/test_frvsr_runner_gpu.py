"""The FRVSR trainer and predictor through the config surface, on the synthetic
NIfTI tree (the reference's on-disk layout):

* configs/train/cfg7_acdc_vsr_frvsr_x4.yaml (AcdcFRVSRTrainer + FRVSRNet +
  AcdcVSRLogger, a small crop, one resblock, one epoch) trains with finite
  logs under the reference's keys (its two L1Loss functions add into the one
  'L1Loss' key), hands the SR frames to the logger and writes a checkpoint
  that loads into a fresh FRVSRNet;
* configs/test/cfg7_acdc_vsr_frvsr_x4.yaml (AcdcVSRPredictor, is_prediction)
  loads that checkpoint, predicts and exports."""
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


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("data"), T=4, H=32, W=32, patients=2)


def test_frvsr_trains_an_epoch_and_predicts(tree, tmp_path):
    cfg = yaml.safe_load((ROOT / "configs" / "train" / "cfg7_acdc_vsr_frvsr_x4.yaml").read_text())
    assert cfg["net"]["name"] == "FRVSRNet" and cfg["trainer"]["name"] == "AcdcFRVSRTrainer"
    assert cfg["logger"]["name"] == "AcdcVSRLogger" and cfg["dataset"]["name"] == "AcdcVSRDataset"
    assert [l["name"] for l in cfg["losses"]] == ["L1Loss", "L1Loss"]
    cfg["dataset"]["kwargs"].update(data_dir=str(tree / "videos"), num_frames=3)
    for a in cfg["dataset"]["kwargs"]["augments"]:
        if a["name"] == "RandomCropPatch":
            a["kwargs"]["size"] = [8, 8]
    cfg["main"]["saved_dir"] = str(tmp_path / "out")
    cfg["dataloader"]["kwargs"].update(num_workers=0, train_batch_size=2)
    cfg["net"]["kwargs"].update(num_resblocks=1)
    cfg["logger"]["kwargs"]["dummy_input"] = [1, 1, 8, 8]
    cfg["monitor"]["kwargs"]["saved_freq"] = 1
    cfg["trainer"]["kwargs"]["num_epochs"] = 1
    trainer = C.build_train(C.Box(cfg), device="cuda:0")
    assert isinstance(trainer, trainers.AcdcFRVSRTrainer) and isinstance(trainer.net, nets.FRVSRNet)
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
        assert abs(log["L1Loss"] - log["Loss"]) <= 1e-6 * log["Loss"]  # both terms, weights 1 and 1
    # outputs[0], the SR frames, went to the logger
    assert len(seen["outputs"]) == len(seen["batch"]["hr_imgs"]) >= 3  # (validation takes whole sequences)
    assert seen["outputs"][0].shape == seen["batch"]["hr_imgs"][0].shape
    for p in trainer.net.parameters():
        assert torch.isfinite(p).all()
    cks = sorted((tmp_path / "out" / "checkpoints").glob("*.pth"))
    assert cks, "no checkpoint written"
    from vsr_amd.callbacks.monitor import safe_globals
    with torch.serialization.safe_globals(safe_globals()):
        ck = torch.load(cks[0], map_location="cpu", weights_only=True)
    fresh = nets.FRVSRNet(**cfg["net"]["kwargs"])
    fresh.load_state_dict(ck["net"])
    assert {"srnet.head.conv.weight", "srnet.tail.deconv2.bias", "fnet.body.conv6_2.weight",
            "fnet.tail.conv2.bias"} <= set(ck["net"])

    # ---- the test config on that checkpoint
    tcfg = yaml.safe_load((ROOT / "configs" / "test" / "cfg7_acdc_vsr_frvsr_x4.yaml").read_text())
    assert tcfg["predictor"]["name"] == "AcdcVSRPredictor" and tcfg["net"]["kwargs"]["is_prediction"] is True
    tcfg["dataset"]["kwargs"].update(data_dir=str(tree / "videos"), num_frames=3)
    tcfg["main"].update(saved_dir=str(tmp_path / "pred"), loaded_path=str(cks[0]))
    tcfg["predictor"]["kwargs"].update(saved_dir=str(tmp_path / "pred"))
    tcfg["dataloader"]["kwargs"]["num_workers"] = 0
    tcfg["net"]["kwargs"].update(num_resblocks=1)
    pred = C.build_test(C.Box(tcfg), device="cuda:0")
    assert isinstance(pred.net, nets.FRVSRNet) and pred.net.is_prediction
    log = pred.predict()
    assert all(math.isfinite(v) for v in log.values()), log
    rows = list(csv.reader(open(tmp_path / "pred" / "results.csv")))
    assert rows[0][0] == "name" and len(rows) > 1
