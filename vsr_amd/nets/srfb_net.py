"""SRFBN (super-resolution feedback network) on the DRF machinery.

Same constructor, module tree, state_dict keys and creation order as the
reference SRFBNet (src/model/nets/srfb_net.py:8-151), so one seed gives its
initial weights and its checkpoints load:

    lrf_block.{conv1, prelu1, conv2, prelu2}     (:53-59, DRF's in_block)
    f_block.*                                    (:62-134, DRF's f_block layer for layer)
    r_block.{deconv1, prelu1, conv2}             (:137-151)

DRFN is SRFBN with two changes (drf_sisr_net.py:9-13), so SRFBNet runs
_DRFBase's forward and hand-written backward (sequence buffers, deferred slope
slots, weight-gradient runs on the side stream) and overrides the three places
where the two differ:

  * the reconstruction reads f_features alone (srfb_net.py:44-46), not
    in_features + f_features: lrf_block.prelu2's gradient comes from the
    feedback block only;
  * the reconstruction is ConvTranspose2d(k, s, p) + PReLU + conv 3x3: the
    sub-pixel deconv through a shuffle-s view with the PReLU epilogue (the form
    of the feedback block's up projections), then the conv writing the fp32
    output;
  * the global skip adds F.interpolate(input, scale_factor=r, 'bilinear',
    align_corners=False) (srfb_net.py:47-48) to every step's output
    (vsrk_upsample2d_fwd).  It has no parameters and the input needs no
    gradient, so the backward passes the output gradient through unchanged.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import functional as F
from .drf_net import _DRFBase, _FBlock, _InBlock, _prelu
from .tape import K3, P1, PROJ


class _RBlock(nn.Sequential):
    def __init__(self, in_channels, out_channels, upscale_factor):
        super().__init__()
        k, s, p = PROJ[upscale_factor]
        self.add_module("deconv1", nn.ConvTranspose2d(in_channels, in_channels, kernel_size=k, stride=s, padding=p))
        self.add_module("prelu1", _prelu())
        self.add_module("conv2", nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1))


class SRFBNet(_DRFBase):
    """SRFBN (srfb_net.py:8-50): (B,C,h,w) -> list of num_steps (B,C,rh,rw)."""

    _FEATURE_SKIP = False
    # The bilinear skip: "accumulate" runs upsample2d(..., accumulate=True) on
    # each step's output; "residual" materialises the upsampled input once per
    # forward and the last conv adds it in its epilogue (one output channel
    # only: there the NCHW image is the conv's channels-last view).
    # VSR_SRFB_SKIP selects; the measured figures are in DESIGN.md section 7.
    SKIP_MODE = os.environ.get("VSR_SRFB_SKIP", "accumulate")

    def __init__(self, in_channels, out_channels, num_steps, num_features, num_groups, upscale_factor):
        super().__init__(in_channels, out_channels, num_features, num_groups, upscale_factor)
        self.num_steps = num_steps
        self._skip_img = None

    def _build_blocks(self):
        self.lrf_block = _InBlock(self.in_channels, self.num_features)
        self.f_block = _FBlock(self.num_features, self.num_groups, self.upscale_factor)
        self.r_block = _RBlock(self.num_features, self.out_channels, self.upscale_factor)

    def _feature_block(self):
        return self.lrf_block

    def _frames(self, inputs):
        return [inputs] * self.num_steps

    # ------------------------------------------------------------------
    def _reconstruct(self, t, x, infeat, ffeat, buf, pw, sp):
        f, co = self.num_features, self.out_channels
        k, s, p = PROJ[self.upscale_factor]
        b, _, h, w, _ = ffeat.shape
        H, W = h * s, w * s
        rb = self.r_block
        hr = buf("rhr", t, H, W, f)
        wq, bq = sp(rb.deconv1, True)
        F.conv(ffeat, wq, hr, K3, P1, bias=bq, bias_r=1, y_shuffle=s, act=F.ACT_PRELU, act_param=rb.prelu1.weight,
               subpixel=F.subpixel_code(k, s, p, True, False))
        xs = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.float().contiguous()
        if xs.shape[1] != co:
            raise ValueError(f"SRFBNet adds the upsampled input to the output: in_channels {xs.shape[1]} != "
                             f"out_channels {co}")
        if self.SKIP_MODE == "residual" and co == 1:
            if t == 0:  # the input is the same at every step
                self._skip_img = F.upsample2d(xs, torch.empty((b, 1, H, W), dtype=torch.float32, device=xs.device),
                                              "bilinear", False, s)
            y = torch.empty((b, 1, H, W), dtype=torch.float32, device=xs.device)
            F.conv(hr, pw(rb.conv2), y.view(b, 1, H, W, 1), K3, P1, bias=rb.conv2.bias,
                   residual=self._skip_img.view(b, 1, H, W, 1))
            if t == self.num_steps - 1:
                self._skip_img = None
        else:
            y = self._tail(rb.conv2, hr, pw)
            F.upsample2d(xs, y, "bilinear", False, s, accumulate=True)
        return y, dict(tail_in=hr)

    def _recon_seq_elems(self, HH, WW, h, w) -> int:
        return (HH * WW + h * w) * self.num_features  # drhr, gff

    def _reconstruct_backward(self, bk, t, rc, g):
        f = self.num_features
        k, s, p = PROJ[self.upscale_factor]
        rb = self.r_block
        hr, ffeat = rc["tail_in"], rc["ffeat"]
        b, _, H, W, _ = hr.shape
        h, w = H // s, W // s
        bk.wgrad(rb.conv2, hr, g, K3, P1, t)
        # conv2's data gradient with prelu1's backward: fused where eligible;
        # for a slope <= 0 from the recomputed pre-activation (the deconv
        # without its activation), as nn.PReLU does
        dhr = bk.sbuf("drhr", t, H, W, f)
        w2 = bk.pw(rb.conv2, 1)
        pr = rb.prelu1
        da, acc, sl = bk.slot(pr)
        if id(pr) in bk.nonpos:
            F.conv(g, w2, dhr, K3, P1)
            wq, bq = bk.sp(rb.deconv1, True)
            pre = F.conv(ffeat, wq, bk.new(H, W, f), K3, P1, bias=bq, bias_r=1, y_shuffle=s,
                         subpixel=F.subpixel_code(k, s, p, True, False))
            F.prelu_bwd(pre, dhr, pr.weight, dhr, da, acc, pre=True, slot=sl)
        elif not F.conv_prelu_bwd(g, w2, dhr, K3, P1, hr, pr.weight, da, acc, slot=sl):
            F.conv(g, w2, dhr, K3, P1)
            F.prelu_bwd(hr, dhr, pr.weight, dhr, da, acc, slot=sl)
        bk.sp_wgrad(rb.deconv1, ffeat, dhr, True, t)
        # the sub-pixel data gradient down to LR: the gradient of f_features
        return F.conv(dhr, bk.sp(rb.deconv1, True, 1)[0], bk.sbuf("gff", t, h, w, f), K3, P1, x_shuffle=s,
                      subpixel=F.subpixel_code(k, s, p, True, True))
