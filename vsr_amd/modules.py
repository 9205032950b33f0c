"""Op-level drop-in modules over ``torch.ops.vsrk`` (vsr_amd.ops).

Each class subclasses the torch.nn layer it replaces, so parameters, buffers,
``state_dict`` keys and constructor arguments are unchanged; only forward()
runs the HIP kernels.  ``swap_modules(net)`` replaces every supported layer
of an existing network in place -- e.g. a reference generator built from its
own source (src/model/nets/*.py) keeps its forward code and weights and runs
its convolutions / batch norms on MI355X:

  nn.Conv2d / nn.Conv3d (kernel 1 or 3 in h, w; stride 1; zero padding)  -> HipConv2d / HipConv3d
  nn.Conv2d(k, stride s, padding p), k <= p + 2s, p <= s (DRF's down
      projections, drf_net.py:93,100)                                   -> HipConv2d (sub-pixel form)
  nn.ConvTranspose2d(k, s, p) (DRF's up projections, drf_net.py:81,86),
      output_padding 0 or s - k + 2p (FRVSR's tail, frvsr_net.py:84,86)   -> HipConvTranspose2d
  nn.MaxPool2d(2) (FRVSR's FNet, frvsr_net.py:127)                      -> HipMaxPool2d
  nn.BatchNorm3d (duf_net.py:116,198,201)                               -> HipBatchNorm3d
  nn.Upsample(scale_factor=r, mode='bilinear' | 'bicubic'), integer r (or a
      pair of equal integers), 4-D input (bicubic.py:15)                -> HipUpsample

``STN`` is the reference's flow-warp module (frvsr_net.py:196-226) by name and
signature, on vsrk::flow_warp; it has no torch.nn counterpart to swap.

Other nn.Upsample forms (nearest, trilinear, size=, a non-integer scale) are
left as they are.  Activations, PixelShuffle and tensor plumbing stay torch ops.  The fused
generators in vsr_amd.nets are the fast path; these modules trade a layout
conversion per op for drop-in generality.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops  # noqa: F401  (registers torch.ops.vsrk)


def _supported_conv(m: nn.Module) -> bool:
    k = m.kernel_size
    return (m.groups == 1 and m.dilation == (1,) * len(k) and m.padding_mode == "zeros"
            and all(s == 1 for s in m.stride) and k[-1] == k[-2] and k[-1] in (1, 3)
            and isinstance(m.padding, tuple))


def _subpixel_ok(k: int, s: int, p: int) -> bool:
    return s > 1 and k <= p + 2 * s and p <= s


class HipConv2d(nn.Conv2d):
    """nn.Conv2d on vsrk::conv (stride 1, kernel 1/3), or -- for a strided
    kernel k with stride s -- a 3x3 conv over the s x s sub-pixel view."""

    def forward(self, x):
        s = self.stride[0]
        if s > 1:
            weq, beq = torch.ops.vsrk.subpixel_weight(self.weight, self.bias, self.kernel_size[0], s,
                                                      self.padding[0], False)
            return torch.ops.vsrk.conv(x, weq, beq if self.bias is not None else None, [1, 1], "none", s, 1)
        return torch.ops.vsrk.conv(x, self.weight, self.bias, list(self.padding), "none", 1, 1)


class HipConv3d(nn.Conv3d):
    def forward(self, x):
        return torch.ops.vsrk.conv(x, self.weight, self.bias, list(self.padding), "none", 1, 1)


class HipConvTranspose2d(nn.ConvTranspose2d):
    """nn.ConvTranspose2d(k, stride s, padding p) as a 3x3 conv storing through
    an s x s sub-pixel output view (exact: every output sub-pixel is one 3x3
    window of the low-resolution input)."""

    def forward(self, x, output_size=None):
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        weq, beq = torch.ops.vsrk.subpixel_weight(self.weight, self.bias, k, s, p, True)
        return torch.ops.vsrk.conv(x, weq, beq if self.bias is not None else None, [1, 1], "none", 1, s, True)


class HipBatchNorm3d(nn.BatchNorm3d):
    def forward(self, x):
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        use_batch = self.training or not self.track_running_stats
        rm = self.running_mean if self.running_mean is not None else torch.zeros(self.num_features, device=x.device)
        rv = self.running_var if self.running_var is not None else torch.ones(self.num_features, device=x.device)
        st = torch.ops.vsrk.batch_norm_stats(x.detach(), self.weight.detach() if self.weight is not None else None,
                                             self.bias.detach() if self.bias is not None else None, rm, rv,
                                             use_batch, self.momentum if self.momentum is not None else 0.1,
                                             self.eps)
        return torch.ops.vsrk.batch_norm(x, self.weight, self.bias, st, use_batch, False)


def _int_scale(sf) -> int | None:
    """The integer factor of an nn.Upsample scale_factor (a number or a pair of
    equal numbers), or None."""
    if isinstance(sf, (tuple, list)):
        if len(sf) != 2 or sf[0] != sf[1]:
            return None
        sf = sf[0]
    if sf is None or float(sf) != int(sf) or int(sf) < 1:
        return None
    return int(sf)


class HipUpsample(nn.Upsample):
    """nn.Upsample(scale_factor=r, mode='bilinear' | 'bicubic') on
    vsrk::upsample2d for 4-D inputs; anything else runs nn.Upsample's own forward."""

    def forward(self, input):
        r = _int_scale(self.scale_factor)
        if (input.dim() != 4 or r is None or self.size is not None or self.mode not in ("bilinear", "bicubic")
                or getattr(self, "recompute_scale_factor", None)):
            return super().forward(input)
        return torch.ops.vsrk.upsample2d(input, r, self.mode, bool(self.align_corners))


def _pair(v) -> tuple:
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _pool2x2(m: nn.MaxPool2d) -> bool:
    """nn.MaxPool2d(2): kernel 2, stride 2 (or the default: the kernel), no
    padding, dilation, ceil_mode or indices."""
    stride = m.kernel_size if m.stride is None else m.stride
    return (_pair(m.kernel_size) == (2, 2) and _pair(stride) == (2, 2) and _pair(m.padding) == (0, 0)
            and _pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices)


class HipMaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d(2) on vsrk::max_pool2x2 for 4-D inputs (frvsr_net.py:127);
    any other configuration or rank runs nn.MaxPool2d's own forward."""

    def forward(self, input):
        if input.dim() != 4 or not _pool2x2(self):
            return super().forward(input)
        return torch.ops.vsrk.max_pool2x2(input)


class STN(nn.Module):
    """The reference's spatial transformer (frvsr_net.py:196-240) on
    vsrk::flow_warp: ``forward(inputs, u, v)`` samples ``inputs`` (N, C, H, W)
    bilinearly at mesh + (u, v), the mesh being linspace(-1, 1) per axis and
    the flow in normalised units; ``normalize=True`` takes a flow in pixels
    and divides it by half the image size as the reference does.  grid_sample
    runs with its default align_corners=False, as in the reference.  The
    gradient goes to u and v only."""

    def __init__(self, mode="bilinear", padding_mode="zeros", normalize=False):
        super().__init__()
        self.mode = mode
        self.padding_mode = padding_mode
        self.norm = normalize

    def forward(self, inputs, u, v):
        if self.mode != "bilinear":
            raise NotImplementedError(f"STN: sampling mode {self.mode!r} (the warp kernel is bilinear)")
        if self.padding_mode not in ("zeros", "border"):
            raise NotImplementedError(f"STN: padding_mode {self.padding_mode!r} ('zeros' or 'border')")
        if self.norm:
            h, w = inputs.shape[-2:]
            u = u / w * 2
            v = v / h * 2
        return torch.ops.vsrk.flow_warp(inputs, u, v, self.padding_mode, False)


def _deconv_output_padding_ok(m: nn.ConvTranspose2d) -> bool:
    """The sub-pixel form writes exactly s*h rows: torch's size when
    output_padding = s - k + 2p (frvsr_net.py:84,86: (3, 2, 1) with 1).
    output_padding = 0 is accepted for every (k, s, p) too, as it always was:
    that is right where s - k + 2p = 0 (every DRF deconv) and a KNOWN WRONG
    SIZE otherwise -- (3, 2, 1) with 0 is 2h - 1 rows in torch, 2h here.  Kept
    so that every module converted so far converts the same way; a later
    change can accept s - k + 2p alone."""
    k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
    return m.output_padding in ((0, 0), (s - k + 2 * p,) * 2)


def _convert(m: nn.Module) -> nn.Module | None:
    if type(m) is nn.Conv2d:
        if _supported_conv(m):
            new = HipConv2d.__new__(HipConv2d)
        elif (m.groups == 1 and m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1]
              and m.padding[0] == m.padding[1] and _subpixel_ok(m.kernel_size[0], m.stride[0], m.padding[0])):
            new = HipConv2d.__new__(HipConv2d)
        else:
            return None
    elif type(m) is nn.Conv3d and _supported_conv(m):
        new = HipConv3d.__new__(HipConv3d)
    elif (type(m) is nn.ConvTranspose2d and m.groups == 1 and _deconv_output_padding_ok(m)
          and m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1]
          and _subpixel_ok(m.kernel_size[0], m.stride[0], m.padding[0])):
        new = HipConvTranspose2d.__new__(HipConvTranspose2d)
    elif type(m) is nn.MaxPool2d and _pool2x2(m):
        new = HipMaxPool2d.__new__(HipMaxPool2d)
    elif type(m) is nn.BatchNorm3d:
        new = HipBatchNorm3d.__new__(HipBatchNorm3d)
    elif (type(m) is nn.Upsample and m.mode in ("bilinear", "bicubic") and m.size is None
          and _int_scale(m.scale_factor) is not None):
        new = HipUpsample.__new__(HipUpsample)
    else:
        return None
    new.__dict__ = m.__dict__  # same parameters, buffers and hyper-parameters
    return new


def swap_modules(net: nn.Module) -> nn.Module:
    """Replace every supported layer of `net` (recursively, in place) by its
    Hip* counterpart; returns net (or its replacement when net itself is a
    supported layer).  Unsupported layers are left as they are."""
    new = _convert(net)
    if new is not None:
        return new
    for name, child in list(net.named_children()):
        new = _convert(child)
        if new is not None:
            setattr(net, name, new)
        else:
            swap_modules(child)
    return net
