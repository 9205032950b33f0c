"""TEST INFRASTRUCTURE ONLY -- golden fixtures of SRFBNet and Bicubic, made
from the reference itself.  Drives oracle.make_golden from outside (nothing
under oracle/ changes); needs the reference tree (build container only):

    python tools/make_golden_srfb.py

* srfb_*: oracle.make_golden.run_case per case with tests/srfb_ref.SRFBRef as
  the restatement: it asserts identical initial weights, outputs and
  gradients against the reference's SRFBNet bit for bit, then writes
  tests/golden/<case>.pt; oracle.add_fp16_env.main() adds the fp16 envelope.
  Full gradient tensors are kept up to FULL_GRAD_MAX[case] elements, chosen so
  that every fixture stays under 1 MiB; larger gradients are pinned by
  run_case's 16 random projections, as in every fixture.
* bicubic.pt: the reference Bicubic(r) outputs (fp32) and an fp64 evaluation
  of the same nn.Upsample for r = 2, 3, 4 on two inputs.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import add_fp16_env, make_golden as mg, ref_loader  # noqa: E402
from tests.srfb_ref import SRFBRef  # noqa: E402

_MOD = "src.model.nets.srfb_net"
CASES = {
    "srfb_x2_small": (_MOD, "SRFBNet", SRFBRef,
                      dict(in_channels=1, out_channels=1, num_steps=2, num_features=16, num_groups=2,
                           upscale_factor=2), "sisr_list", (2, 1, 8, 8)),
    "srfb_x3_small": (_MOD, "SRFBNet", SRFBRef,
                      dict(in_channels=1, out_channels=1, num_steps=3, num_features=16, num_groups=2,
                           upscale_factor=3), "sisr_list", (1, 1, 5, 7)),
    "srfb_x4_canon": (_MOD, "SRFBNet", SRFBRef,
                      dict(in_channels=1, out_channels=1, num_steps=2, num_features=64, num_groups=4,
                           upscale_factor=4), "sisr_list", (1, 1, 6, 8)),
}
# elements up to which a gradient is stored in full (make_golden's default is 20000)
FULL_GRAD_MAX = {"srfb_x2_small": 20000, "srfb_x3_small": 12000, "srfb_x4_canon": 10000}
MAX_BYTES = 1 << 20

BICUBIC_INPUTS = [(2, 1, 5, 7), (1, 1, 1, 6)]
BICUBIC_SCALES = [2, 3, 4]


def run_bicubic():
    ref_cls = ref_loader.load("src.model.nets.bicubic").Bicubic
    g = torch.Generator().manual_seed(mg.SEED + 2)
    fx = {"inputs": [torch.randn(s, generator=g) for s in BICUBIC_INPUTS], "scales": BICUBIC_SCALES,
          "output": {}, "output64": {}}
    for r in BICUBIC_SCALES:
        net = ref_cls(r)
        assert not list(net.parameters())
        with torch.no_grad():
            fx["output"][r] = [net(x) for x in fx["inputs"]]
            fx["output64"][r] = [torch.nn.functional.interpolate(x.double(), scale_factor=r, mode="bicubic",
                                                                 align_corners=True) for x in fx["inputs"]]
        for a, b in zip(fx["output"][r], fx["output64"][r]):
            assert (a.double() - b).abs().max().item() <= 1e-5 * (1 + b.abs().max().item())
    torch.save(fx, mg.OUT / "bicubic.pt")
    print(f"bicubic: {os.path.getsize(mg.OUT / 'bicubic.pt') / 1024:.0f} KiB")


def main():
    if not ref_loader.available():
        raise SystemExit("reference not available (build container only)")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_loader._FILES[_MOD] = "src/model/nets/srfb_net.py"
    ref_loader._FILES["src.model.nets.bicubic"] = "src/model/nets/bicubic.py"
    only = os.environ.get("GOLDEN_ONLY")
    done = {}
    for name, spec in CASES.items():
        if only and name not in only.split(","):
            continue
        mg.FULL_GRAD_MAX = FULL_GRAD_MAX[name]
        mg.run_case(name, spec)
        done[name] = spec
    mg.CASES = done  # add_fp16_env walks make_golden.CASES
    add_fp16_env.main()
    for name in done:
        size = os.path.getsize(mg.OUT / f"{name}.pt")
        assert size <= MAX_BYTES, f"{name}: fixture {size} bytes > {MAX_BYTES}; lower FULL_GRAD_MAX[{name!r}]"
        print(f"{name}: {size / 1024:.0f} KiB")
    if not only or "bicubic" in only.split(","):
        run_bicubic()


if __name__ == "__main__":
    main()
