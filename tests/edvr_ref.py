"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference EDVRNet
(src/model/nets/edvr_net/EDVR_arch.py:13-321 over arch_util.py:7-52; Wang et
al., "EDVR: Video Restoration with Enhanced Deformable Convolutional
Networks", arXiv 1905.02716) in stock torch ops, written from the paper and
from the reference's observed behaviour.  It keeps the reference's parameter
names (state_dicts load both ways), its module construction order and its
initialisation (residual-block convs Kaiming normal x 0.1 with zero bias, the
DCN weight uniform in +-1/sqrt(fan_in) with zero bias, conv_offset_mask
zeroed, everything else torch's default), so one seed gives the same initial
weights.  tools/make_golden_edvr.py pins it to the reference bit for bit in
fp32 (initial weights, output, L1 loss, every gradient) when it writes the
edvr_* fixtures.

The DCN pack is built on oracle.dcn_ref.modulated_deform_conv_ref: the
reference's own pack loads a CUDA extension, so the DCN arithmetic is pinned
to the reference's SOURCE only, as oracle/dcn_ref.py states.

Everything follows the input's dtype, so the fp64 yardstick runs.  Only what
the reference's configs use is restated: predeblur and HR_in raise.

Behaviour reproduced as found:
  * H, W off multiples of 4 are padded with the global minimum of the stacked
    input and the output is cropped (:73-80, 141-144);
  * the alignment loop runs frame by frame over shared weights, the centre
    frame aligned to itself included;
  * `L3_offset * 2` / `L2_offset * 2` after the bilinear x2 (:231-241);
  * no activation after L1_fea_conv, LeakyReLU after the L3 and cascade DCNs.
Not reproduced: the pack's `offset_mean > 100` warning (a log line).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as Fn

from oracle.dcn_ref import modulated_deform_conv_ref

# when a list: every pack appends (h positions, w positions, H, W) of its samples (tools/make_golden_edvr.py)
COORD_LOG = None


def sampling_coords(offset, h, w, k=3, stride=1, pad=1, dil=1, dg=1):
    """Sampling positions (n, dg, K, ho, wo) of a DCN, rows and columns, as
    oracle.dcn_ref computes them from the (n, dg*2*K, ho, wo) offsets."""
    n, _, ho, wo = offset.shape
    K = k * k
    off = offset.view(n, dg, K, 2, ho, wo)
    ki, kj = torch.arange(K) // k, torch.arange(K) % k
    bh = (torch.arange(ho) * stride - pad).view(1, 1, 1, ho, 1) + (ki * dil).view(1, 1, K, 1, 1)
    bw = (torch.arange(wo) * stride - pad).view(1, 1, 1, 1, wo) + (kj * dil).view(1, 1, K, 1, 1)
    return bh.to(offset.dtype) + off[:, :, :, 0], bw.to(offset.dtype) + off[:, :, :, 1]


class DCNPackRef(nn.Module):
    """The reference's ModulatedDeformConvPack (deform_conv.py:221-291) with
    extra_offset_mask: forward([input, features])."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=True, extra_offset_mask=False):
        super().__init__()
        assert groups == 1 and bias and extra_offset_mask
        self.k, self.stride, self.padding, self.dilation = kernel_size, stride, padding, dilation
        self.deformable_groups = deformable_groups
        self.weight = nn.Parameter(torch.Tensor(out_channels, in_channels, kernel_size, kernel_size))
        self.bias = nn.Parameter(torch.Tensor(out_channels))
        self.weight.data.uniform_(-1. / math.sqrt(in_channels * kernel_size ** 2),
                                  1. / math.sqrt(in_channels * kernel_size ** 2))
        self.bias.data.zero_()
        self.conv_offset_mask = nn.Conv2d(in_channels, deformable_groups * 3 * kernel_size ** 2, kernel_size,
                                          stride=stride, padding=padding, bias=True)
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def forward(self, x):
        x, fea = x
        out = self.conv_offset_mask(fea)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        mask = torch.sigmoid(mask)
        if COORD_LOG is not None:
            hs, ws = sampling_coords(offset.detach(), x.shape[2], x.shape[3], self.k, self.stride, self.padding,
                                     self.dilation, self.deformable_groups)
            COORD_LOG.append((hs, ws, x.shape[2], x.shape[3]))
        return modulated_deform_conv_ref(x, offset, mask, self.weight, self.bias, self.stride, self.padding,
                                         self.dilation, self.deformable_groups)


class ResBlockRef(nn.Module):
    def __init__(self, nf):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        for c in (self.conv1, self.conv2):
            nn.init.kaiming_normal_(c.weight, a=0, mode="fan_in")
            c.weight.data *= 0.1
            c.bias.data.zero_()
        self.relu = nn.ReLU()

    def forward(self, x):
        return x + self.conv2(self.relu(self.conv1(x)))


def _up2(x):
    return Fn.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


class PCDAlignRef(nn.Module):
    def __init__(self, nf, groups):
        super().__init__()

        def dcn():
            return DCNPackRef(nf, nf, 3, stride=1, padding=1, dilation=1, deformable_groups=groups,
                              extra_offset_mask=True)

        self.L3_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L3_offset_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L3_dcnpack = dcn()
        self.L2_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L2_offset_conv2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L2_offset_conv3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L2_dcnpack = dcn()
        self.L2_fea_conv = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L1_dcnpack = dcn()
        self.L1_fea_conv = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.cas_dcnpack = dcn()
        self.lrelu = nn.LeakyReLU(0.1)

    def forward(self, nbr, ref):
        a = self.lrelu
        o3 = a(self.L3_offset_conv1(torch.cat([nbr[2], ref[2]], dim=1)))
        o3 = a(self.L3_offset_conv2(o3))
        f3 = a(self.L3_dcnpack([nbr[2], o3]))
        o2 = a(self.L2_offset_conv1(torch.cat([nbr[1], ref[1]], dim=1)))
        o3 = _up2(o3)
        o2 = a(self.L2_offset_conv2(torch.cat([o2, o3 * 2], dim=1)))
        o2 = a(self.L2_offset_conv3(o2))
        f2 = self.L2_dcnpack([nbr[1], o2])
        f3 = _up2(f3)
        f2 = a(self.L2_fea_conv(torch.cat([f2, f3], dim=1)))
        o1 = a(self.L1_offset_conv1(torch.cat([nbr[0], ref[0]], dim=1)))
        o2 = _up2(o2)
        o1 = a(self.L1_offset_conv2(torch.cat([o1, o2 * 2], dim=1)))
        o1 = a(self.L1_offset_conv3(o1))
        f1 = self.L1_dcnpack([nbr[0], o1])
        f2 = _up2(f2)
        f1 = self.L1_fea_conv(torch.cat([f1, f2], dim=1))
        off = a(self.cas_offset_conv1(torch.cat([f1, ref[0]], dim=1)))
        off = a(self.cas_offset_conv2(off))
        return a(self.cas_dcnpack([f1, off]))


class TSAFusionRef(nn.Module):
    def __init__(self, nf, nframes, center):
        super().__init__()
        self.center = center
        self.tAtt_1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.tAtt_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.fea_fusion = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.sAtt_1 = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        self.avgpool = nn.AvgPool2d(3, stride=2, padding=1)
        self.sAtt_2 = nn.Conv2d(nf * 2, nf, 1, 1)
        self.sAtt_3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_4 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_5 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_L1 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_L2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.sAtt_L3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_add_1 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_add_2 = nn.Conv2d(nf, nf, 1, 1)
        self.lrelu = nn.LeakyReLU(0.1)

    def forward(self, aligned):
        B, N, C, H, W = aligned.size()
        a = self.lrelu
        emb_ref = self.tAtt_2(aligned[:, self.center].clone())
        emb = self.tAtt_1(aligned.view(-1, C, H, W)).view(B, N, -1, H, W)
        cor = [torch.sum(emb[:, i] * emb_ref, 1).unsqueeze(1) for i in range(N)]
        prob = torch.sigmoid(torch.cat(cor, dim=1))
        prob = prob.unsqueeze(2).repeat(1, 1, C, 1, 1).view(B, -1, H, W)
        aligned = aligned.view(B, -1, H, W) * prob
        fea = a(self.fea_fusion(aligned))
        att = a(self.sAtt_1(aligned))
        att = a(self.sAtt_2(torch.cat([self.maxpool(att), self.avgpool(att)], dim=1)))
        att_L = a(self.sAtt_L1(att))
        att_L = a(self.sAtt_L2(torch.cat([self.maxpool(att_L), self.avgpool(att_L)], dim=1)))
        att_L = _up2(a(self.sAtt_L3(att_L)))
        att = a(self.sAtt_3(att))
        att = att + att_L
        att = _up2(a(self.sAtt_4(att)))
        att = self.sAtt_5(att)
        att_add = self.sAtt_add_2(a(self.sAtt_add_1(att)))
        att = torch.sigmoid(att)
        return fea * att * 2 + att_add


class EDVRRef(nn.Module):
    def __init__(self, in_channels, out_channels, nf=64, nframes=5, groups=8, front_RBs=5, back_RBs=10, center=None,
                 predeblur=False, HR_in=False, w_TSA=True):
        super().__init__()
        if predeblur or HR_in:
            raise NotImplementedError("the restatement covers the reference's configs: no predeblur, no HR_in")
        self.center = nframes // 2 if center is None else center
        self.w_TSA = w_TSA
        self.conv_first = nn.Conv2d(in_channels, nf, 3, 1, 1)
        self.feature_extraction = nn.Sequential(*[ResBlockRef(nf) for _ in range(front_RBs)])
        self.fea_L2_conv1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.fea_L2_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.fea_L3_conv1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.fea_L3_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.pcd_align = PCDAlignRef(nf, groups)
        if w_TSA:
            self.tsa_fusion = TSAFusionRef(nf, nframes, self.center)
        else:
            self.tsa_fusion = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.recon_trunk = nn.Sequential(*[ResBlockRef(nf) for _ in range(back_RBs)])
        self.upconv1 = nn.Conv2d(nf, nf * 4, 3, 1, 1)
        self.upconv2 = nn.Conv2d(nf, 64 * 4, 3, 1, 1)
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.HRconv = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, out_channels, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(0.1)

    def forward(self, inputs):
        x = torch.stack(inputs, dim=1)
        B, N, C, H, W = x.size()
        pad = None
        if H % 4 or W % 4:
            hd, wd = -H % 4, -W % 4
            pad = (wd // 2, wd - wd // 2, hd // 2, hd - hd // 2)
            x = Fn.pad(x, pad, value=x.min())
            B, N, C, H, W = x.size()
        xc = x[:, self.center].contiguous()
        a = self.lrelu
        f1 = self.feature_extraction(a(self.conv_first(x.view(-1, C, H, W))))
        f2 = a(self.fea_L2_conv2(a(self.fea_L2_conv1(f1))))
        f3 = a(self.fea_L3_conv2(a(self.fea_L3_conv1(f2))))
        f1 = f1.view(B, N, -1, H, W)
        f2 = f2.view(B, N, -1, H // 2, W // 2)
        f3 = f3.view(B, N, -1, H // 4, W // 4)
        ref = [f[:, self.center].clone() for f in (f1, f2, f3)]
        aligned = []
        for i in range(N):
            aligned.append(self.pcd_align([f[:, i].clone() for f in (f1, f2, f3)], ref))
        aligned = torch.stack(aligned, dim=1)
        if not self.w_TSA:
            aligned = aligned.view(B, -1, H, W)
        out = self.recon_trunk(self.tsa_fusion(aligned))
        out = a(self.pixel_shuffle(self.upconv1(out)))
        out = a(self.pixel_shuffle(self.upconv2(out)))
        out = self.conv_last(a(self.HRconv(out)))
        out = out + Fn.interpolate(xc, scale_factor=4, mode="bilinear", align_corners=False)
        if pad is not None:
            out = out[..., pad[2] * 4:out.size(-2) - pad[3] * 4, pad[0] * 4:out.size(-1) - pad[1] * 4]
        return out


def perturb_offset_convs(net, seed, scale=0.5):
    """Seeded normal noise on every conv_offset_mask weight and bias, in
    named_parameters order, from a CPU Generator(seed + 2): weights with std
    scale / sqrt(fan_in), biases with std scale.  tools/make_golden_edvr.py
    sizes `scale` so that the offsets' rms is about half a pixel and stores it
    (with the rms and maximum that came out) in the fixture."""
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "conv_offset_mask" not in k:
                continue
            std = scale / math.sqrt(p[0].numel()) if p.dim() == 4 else scale
            p.add_(torch.randn(p.shape, generator=g, dtype=torch.float32).to(p.dtype) * std)
    return net
