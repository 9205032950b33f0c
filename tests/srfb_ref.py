"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference SRFBNet
(src/model/nets/srfb_net.py:8-151) in stock torch.nn ops, on the blocks of
oracle.cpu_nets: the reference's parameter names (state_dicts load both ways)
and module construction order (one seed gives the same initial weights).
tools/make_golden_srfb.py pins it to the reference bit for bit (initial
weights, outputs, every gradient) when it writes the srfb_* fixtures."""
from __future__ import annotations

import torch.nn as nn
import torch.nn.functional as Fn

from oracle.cpu_nets import _DRFFeedback, _DRFIn, _PROJ, _prelu


class SRFBRef(nn.Module):
    """(B, C, h, w) -> list of num_steps (B, C, rh, rw) (srfb_net.py:38-50)."""

    def __init__(self, in_channels, out_channels, num_steps, num_features, num_groups, upscale_factor):
        super().__init__()
        if upscale_factor not in _PROJ:
            raise ValueError(f"The upscale factor should be 2, 3, 4 or 8. Got {upscale_factor}.")
        self.num_steps = num_steps
        self.upscale_factor = upscale_factor
        k, s, p = _PROJ[upscale_factor]
        self.lrf_block = _DRFIn(in_channels, num_features)
        self.f_block = _DRFFeedback(num_features, num_groups, upscale_factor)
        self.r_block = nn.Sequential()
        self.r_block.add_module("deconv1", nn.ConvTranspose2d(num_features, num_features, k, stride=s, padding=p))
        self.r_block.add_module("prelu1", _prelu())
        self.r_block.add_module("conv2", nn.Conv2d(num_features, out_channels, 3, padding=1))

    def forward(self, x):
        outs = []
        for i in range(self.num_steps):
            feat = self.lrf_block(x)
            if i == 0:
                self.f_block.hidden_state = feat
            feat = self.f_block(feat)
            self.f_block.hidden_state = feat
            up = Fn.interpolate(x, scale_factor=self.upscale_factor, mode="bilinear", align_corners=False)
            outs.append(up + self.r_block(feat))
        return outs
