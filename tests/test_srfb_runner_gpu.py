"""The SRFB trainer and the Bicubic baseline through the config surface, on the
synthetic NIfTI tree (the reference's on-disk layout):

* configs/train/cfg6_acdc_sisr_srfb_x4.yaml (AcdcSISRSRFBTrainer + SRFBNet +
  AcdcSISRSRFBLogger, a smaller net and one epoch) trains with a finite loss
  and writes a checkpoint that loads back into the net;
* configs/test/cfg6_acdc_sisr_bicubic_x4.yaml (AcdcSISRPredictor + Bicubic(4))
  exports, and its PSNR is within 0.01 dB of torch's bicubic on the CPU."""
import csv
import math
from pathlib import Path

import pytest
import torch
import yaml

from nifti_tree import make_tree
from oracle import cpu_nets
from vsr_amd import config as C
from vsr_amd import nets

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp("data"), T=4, H=32, W=32, patients=2)


def test_srfb_trainer_runs_an_epoch(tree, tmp_path):
    cfg = yaml.safe_load((ROOT / "configs" / "train" / "cfg6_acdc_sisr_srfb_x4.yaml").read_text())
    assert cfg["net"]["name"] == "SRFBNet" and cfg["trainer"]["name"] == "AcdcSISRSRFBTrainer"
    assert cfg["logger"]["name"] == "AcdcSISRSRFBLogger" and cfg["precision"] == "bf16"
    cfg["dataset"]["kwargs"]["data_dir"] = str(tree / "imgs")
    for a in cfg["dataset"]["kwargs"]["augments"]:
        if a["name"] == "RandomCropPatch":
            a["kwargs"]["size"] = [8, 8]
    cfg["main"]["saved_dir"] = str(tmp_path / "out")
    cfg["dataloader"]["kwargs"].update(num_workers=0, train_batch_size=4)
    cfg["net"]["kwargs"].update(num_steps=2, num_features=16, num_groups=2)
    cfg["logger"]["kwargs"]["dummy_input"] = [1, 1, 8, 8]
    cfg["monitor"]["kwargs"]["saved_freq"] = 1
    cfg["trainer"]["kwargs"]["num_epochs"] = 1
    trainer = C.build_train(C.Box(cfg), device="cuda:0")
    assert isinstance(trainer.net, nets.SRFBNet) and trainer.net.compute_dtype == torch.bfloat16
    seen = {}
    write = trainer.logger.write

    def record(epoch, train_log, train_batch, train_outputs, valid_log, valid_batch, valid_outputs):
        seen.update(train=train_log, valid=valid_log, steps=len(valid_outputs))
        return write(epoch, train_log, train_batch, train_outputs, valid_log, valid_batch, valid_outputs)

    trainer.logger.write = record
    trainer.train()
    assert seen["steps"] == 2 and list(seen["train"]) == ["Loss", "L1Loss", "PSNR", "SSIM"]
    for log in (seen["train"], seen["valid"]):
        assert all(math.isfinite(v) for v in log.values()) and log["Loss"] > 0, log
    for p in trainer.net.parameters():
        assert torch.isfinite(p).all()
    cks = sorted((tmp_path / "out" / "checkpoints").glob("*.pth"))
    assert cks, "no checkpoint written"
    from vsr_amd.callbacks.monitor import safe_globals
    with torch.serialization.safe_globals(safe_globals()):
        ck = torch.load(cks[0], map_location="cpu", weights_only=True)
    fresh = nets.SRFBNet(**cfg["net"]["kwargs"])
    fresh.load_state_dict(ck["net"])
    assert "r_block.deconv1.weight" in ck["net"] and "lrf_block.conv1.weight" in ck["net"]


def test_bicubic_predictor_exports(tree, tmp_path):
    cfg = yaml.safe_load((ROOT / "configs" / "test" / "cfg6_acdc_sisr_bicubic_x4.yaml").read_text())
    assert cfg["net"]["name"] == "Bicubic" and cfg["predictor"]["name"] == "AcdcSISRPredictor"
    cfg["dataset"]["kwargs"]["data_dir"] = str(tree / "imgs")
    cfg["main"]["saved_dir"] = str(tmp_path / "pred")
    cfg["main"]["loaded_path"] = str(tmp_path / "no_such_checkpoint.pth")  # never read for Bicubic
    cfg["predictor"]["kwargs"].update(saved_dir=str(tmp_path / "pred"))
    cfg["dataloader"]["kwargs"]["num_workers"] = 0
    pred = C.build_test(C.Box(cfg), device="cuda:0")
    assert isinstance(pred.net, nets.Bicubic)
    log = pred.predict()
    # torch's bicubic on the CPU, the reference's metric on the denormalized images
    ps = []
    for b in pred.test_dataloader:
        out = torch.nn.functional.interpolate(b["lr_img"], scale_factor=4, mode="bicubic", align_corners=True)
        ps.append(cpu_nets.psnr(cpu_nets.denormalize(out, "acdc"), cpu_nets.denormalize(b["hr_img"], "acdc")).item())
    assert abs(log["PSNR"] - sum(ps) / len(ps)) <= 0.01, (log["PSNR"], sum(ps) / len(ps))
    rows = list(csv.reader(open(tmp_path / "pred" / "results.csv")))
    assert len(rows) == 1 + len(ps) and rows[0][0] == "name"
    assert len(list((tmp_path / "pred" / "imgs").rglob("*.png"))) == len(ps)
