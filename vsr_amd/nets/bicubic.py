"""The bicubic-interpolation baseline (src/model/nets/bicubic.py:8-19):
nn.Upsample(scale_factor=r, mode='bicubic', align_corners=True), the floor of
every SR table.  No parameters; one vsrk_upsample2d_fwd launch on the fp32
input."""
from __future__ import annotations

import torch

from .. import functional as F
from .base_net import BaseNet


class Bicubic(BaseNet):
    """(B, C, h, w) -> (B, C, rh, rw).  The image path is fp32 in every
    set_precision mode (there is nothing to train and no activation to keep)."""

    def __init__(self, upscale_factor):
        super().__init__()
        r = int(upscale_factor)
        if r != upscale_factor or r < 1:
            raise ValueError(f"The upscale factor should be a positive integer. Got {upscale_factor}.")
        self.upscale_factor = r

    def _run(self, inputs, tape: dict | None):
        x = inputs if (inputs.dtype == torch.float32 and inputs.is_contiguous()) else inputs.float().contiguous()
        b, c, h, w = x.shape
        r = self.upscale_factor
        y = torch.empty((b, c, h * r, w * r), dtype=torch.float32, device=x.device)
        return F.upsample2d(x, y, "bicubic", True, r)

    def _backward(self, tape: dict, grads) -> dict:
        return {}
