"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference FRVSRNet
(src/model/nets/frvsr_net.py:11-240; Sajjadi et al., "Frame-Recurrent Video
Super-Resolution", arXiv 1801.04590) in stock torch ops, written from the
paper and from the reference's observed behaviour.  It keeps the reference's
parameter names (state_dicts load both ways), its module construction order
and its Xavier pass over every module whose class name contains "Conv" (one
seed gives the same initial weights).  tools/make_golden_frvsr.py pins it to
the reference bit for bit in fp32 (initial weights, both output lists, every
gradient) when it writes the frvsr_* fixtures.

Where it differs on purpose: the reference fixes float32 for the first
estimate and for the mesh, so its .double() fails inside grid_sample.  Here
both follow the input's dtype, which makes the fp64 yardstick run.  The mesh
keeps the reference's VALUES in every dtype (np.linspace rounded to float32,
then cast), so the fp32 and fp64 runs sample the same nominal positions.

Behaviour reproduced as found:
  * only upscale_factor = 4 works (the tail is two stride-2 deconvs);
  * grid_sample runs with align_corners=False on a mesh of linspace(-1, 1,
    size) and a flow added in normalised units, padding 'border';
  * neither warped image carries a gradient (the estimate is detached, the
    previous frame is data): the flow is the only path into the flow net;
  * the flow net pads H and W to multiples of 8 with the batch minimum, runs
    and crops.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn


def mesh(h: int, w: int, dtype, device=None) -> torch.Tensor:
    """(h, w, 2) sampling mesh, x first: linspace(-1, 1, size) per axis with the
    reference's float32 values, in `dtype`."""
    my, mx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    return torch.tensor(np.stack([mx, my], -1), dtype=torch.float32, device=device).to(dtype)


def warp(img: torch.Tensor, u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Bilinear sample of img (N, C, H, W) at mesh + (u, v), border padding."""
    grid = mesh(img.shape[-2], img.shape[-1], img.dtype, img.device)[None] + torch.stack([u, v], dim=-1)
    return Fn.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)


def space_to_depth(x: torch.Tensor, r: int) -> torch.Tensor:
    """(N, C, rh, rw) -> (N, C r r, h, w), channel c r r + i r + j (= pixel_unshuffle)."""
    n, c, hh, ww = x.shape
    return x.reshape(n, c, hh // r, r, ww // r, r).permute(0, 1, 3, 5, 2, 4).reshape(n, c * r * r, hh // r, ww // r)


class _Residual(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.body = nn.Sequential()
        self.body.add_module("conv1", nn.Conv2d(f, f, 3, padding=1))
        self.body.add_module("relu1", nn.ReLU())
        self.body.add_module("conv2", nn.Conv2d(f, f, 3, padding=1))

    def forward(self, x):
        return x + self.body(x)


class _SR(nn.Module):
    """cat(space_to_depth(warped estimate), frame) -> x4 image."""

    def __init__(self, in_channels, out_channels, r, num_resblocks):
        super().__init__()
        self.head = nn.Sequential()
        self.head.add_module("conv", nn.Conv2d(in_channels * (r * r + 1), 64, 3, padding=1))
        self.head.add_module("relu", nn.ReLU())
        self.body = nn.Sequential(*[_Residual(64) for _ in range(num_resblocks)])
        self.tail = nn.Sequential()
        for i in (1, 2):
            self.tail.add_module(f"deconv{i}", nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1))
            self.tail.add_module(f"relu{i}", nn.ReLU())
        self.tail.add_module("conv", nn.Conv2d(64, out_channels, 3, padding=1))

    def forward(self, estimate, frame):
        return self.tail(self.body(self.head(torch.cat([estimate, frame], dim=1))))


class _Up2(nn.Module):
    def forward(self, x):
        return Fn.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


class _Flow(nn.Module):
    """cat(previous frame, frame) -> (u, v) in (-1, 1): three conv-conv-pool
    stages 32, 64, 128, three conv-conv-upsample stages 256, 128, 64, a 32-wide
    conv and the two-channel tanh head; LeakyReLU(0.2) throughout."""

    def __init__(self, in_channels):
        super().__init__()
        self.body = nn.Sequential()
        cin = 2 * in_channels
        for i, (f, down) in enumerate([(32, True), (64, True), (128, True), (256, False), (128, False), (64, False)]):
            self.body.add_module(f"conv{i + 1}_1", nn.Conv2d(cin, f, 3, padding=1))
            self.body.add_module(f"leaky_relu{i + 1}_1", nn.LeakyReLU(0.2))
            self.body.add_module(f"conv{i + 1}_2", nn.Conv2d(f, f, 3, padding=1))
            self.body.add_module(f"leaky_relu{i + 1}_2", nn.LeakyReLU(0.2))
            if down:
                self.body.add_module(f"pooling_{i}", nn.MaxPool2d(2))
            else:
                self.body.add_module(f"upsample_{i - 3}", _Up2())
            cin = f
        self.tail = nn.Sequential()
        self.tail.add_module("conv1", nn.Conv2d(cin, 32, 3, padding=1))
        self.tail.add_module("leaky_relu", nn.LeakyReLU(0.2))
        self.tail.add_module("conv2", nn.Conv2d(32, 2, 3, padding=1))
        self.tail.add_module("tanh", nn.Tanh())

    def forward(self, previous, frame):
        x = torch.cat([previous, frame], dim=1)
        h, w = x.shape[-2:]
        ph, pw = -h % 8, -w % 8
        if ph or pw:
            x = Fn.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), value=float(x.min()))
        x = self.tail(self.body(x))
        return x[..., ph // 2:ph // 2 + h, pw // 2:pw // 2 + w]


class FRVSRRef(nn.Module):
    """list of T frames (N, C, h, w) -> (T estimates (N, C, 4h, 4w), T warped
    previous frames (N, C, h, w)); the estimates alone when is_prediction."""

    def __init__(self, in_channels, out_channels, upscale_factor, is_prediction=False, num_resblocks=10):
        super().__init__()
        self.upscale_factor = upscale_factor
        self.is_prediction = is_prediction
        self.srnet = _SR(in_channels, out_channels, upscale_factor, num_resblocks)
        self.fnet = _Flow(in_channels)
        for m in self.modules():
            if "Conv" in type(m).__name__:
                nn.init.xavier_uniform_(m.weight)

    def forward(self, inputs):
        r = self.upscale_factor
        if r != 4:
            raise ValueError(f"FRVSRNet's tail is two stride-2 deconvs, a fixed x4: upscale_factor {r}")
        first = inputs[0]
        n, c, h, w = first.shape
        previous = first
        estimate = torch.zeros((n, c, h * r, w * r), dtype=first.dtype, device=first.device)
        sr, lr = [], []
        for frame in inputs:
            flow = self.fnet(previous, frame)
            flow_hr = Fn.interpolate(flow, scale_factor=r, mode="bilinear", align_corners=True)
            warped = warp(estimate.detach(), flow_hr[:, 0], flow_hr[:, 1])
            estimate = self.srnet(space_to_depth(warped, r), frame)
            sr.append(estimate)
            lr.append(warp(previous, flow[:, 0], flow[:, 1]))
            previous = frame
        return sr if self.is_prediction else (sr, lr)


def loss(out, frames, targets) -> torch.Tensor:
    """The FRVSR trainers' objective: mean_t L1(warped previous frame_t,
    frame_t) + mean_t L1(estimate_t, target_t)."""
    sr, lr = out
    flow_term = torch.stack([Fn.l1_loss(a, b) for a, b in zip(lr, frames)]).mean()
    sr_term = torch.stack([Fn.l1_loss(a, b) for a, b in zip(sr, targets)]).mean()
    return flow_term + sr_term
