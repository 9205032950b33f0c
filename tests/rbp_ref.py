"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference RBPNet
(src/model/nets/rbp_net.py:8-285; Haris et al., "Recurrent Back-Projection
Network for Video Super-Resolution", arXiv 1903.10128) in stock torch ops,
written from the paper and from the reference's observed behaviour.  It keeps
the reference's parameter names (state_dicts load both ways) and its module
construction order (one seed gives the same initial weights: torch's default
initialisation, nn.PReLU() at 0.25).  tools/make_golden_rbp.py pins it to the
reference bit for bit in fp32 (initial weights, output, every gradient) when
it writes the rbp_* fixtures.

Structure, from the paper: the centre frame's features go through a DBPN
(three up / two down back-projection stages, concatenated) to an HR estimate
h0; each neighbour, stacked with the centre frame, goes through residual
blocks and a deconvolution to an HR estimate h1; the residual h0 - h1 is
refined by residual blocks and added back to h0, which gives H_t; H_t is
projected down again (residual blocks, strided conv) to feed the next
neighbour's DBPN.  The H_t are concatenated and reduced by one 3x3 conv.

Behaviour reproduced as found:
  * the centre index is num_frames // 2 for odd counts, num_frames // 2 - 1
    for even ones;
  * a residual block has ONE PReLU, used after conv1 and after the skip add;
  * every PReLU and every sub-network is shared by the neighbours;
  * the last neighbour's down projection is computed and dropped.
Where it differs on purpose: the caller's list is not mutated (the reference
pops the centre frame out of it).
"""
from __future__ import annotations

import torch
import torch.nn as nn

PROJ = {2: (6, 2, 2), 3: (7, 3, 2), 4: (8, 4, 2), 8: (12, 8, 2)}
SLOPE_MIX = (0.25, -0.1, 0.0, 1.5)


class Stored(nn.Identity):
    """Marks a sum or difference that a conv reads: an implementation with
    16-bit activations has to store it, i.e. round it (the fixtures' 16-bit
    envelopes round here too).  No parameters: the state_dict is the reference's."""


class ConvBlock(nn.Module):
    def __init__(self, cin, cout, k=3, s=1, p=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, s, p)
        if act:
            self.act = nn.PReLU()

    def forward(self, x):
        y = self.conv(x)
        return self.act(y) if hasattr(self, "act") else y


class DeconvBlock(nn.Module):
    def __init__(self, cin, cout, k, s, p):
        super().__init__()
        self.deconv = nn.ConvTranspose2d(cin, cout, k, s, p)
        self.act = nn.PReLU()

    def forward(self, x):
        return self.act(self.deconv(x))


class ResnetBlock(nn.Module):
    def __init__(self, nf):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.act = nn.PReLU()

    def forward(self, x):
        return self.act(torch.add(self.conv2(self.act(self.conv1(x))), x))


class UpBlock(nn.Module):
    def __init__(self, nf, k, s, p):
        super().__init__()
        self.up_conv1 = DeconvBlock(nf, nf, k, s, p)
        self.up_conv2 = ConvBlock(nf, nf, k, s, p)
        self.up_conv3 = DeconvBlock(nf, nf, k, s, p)
        self.diff, self.out = Stored(), Stored()

    def forward(self, x):
        h0 = self.up_conv1(x)
        return self.out(self.up_conv3(self.diff(self.up_conv2(h0) - x)) + h0)


class DownBlock(nn.Module):
    def __init__(self, nf, k, s, p):
        super().__init__()
        self.down_conv1 = ConvBlock(nf, nf, k, s, p)
        self.down_conv2 = DeconvBlock(nf, nf, k, s, p)
        self.down_conv3 = ConvBlock(nf, nf, k, s, p)
        self.diff, self.out = Stored(), Stored()

    def forward(self, x):
        l0 = self.down_conv1(x)
        return self.out(self.down_conv3(self.diff(self.down_conv2(l0) - x)) + l0)


class DBPNet(nn.Module):
    def __init__(self, base_filter, feat, num_stages, k, s, p):
        super().__init__()
        self.feat1 = ConvBlock(base_filter, feat, 1, 1, 0)
        self.up1 = UpBlock(feat, k, s, p)
        self.down1 = DownBlock(feat, k, s, p)
        self.up2 = UpBlock(feat, k, s, p)
        self.down2 = DownBlock(feat, k, s, p)
        self.up3 = UpBlock(feat, k, s, p)
        self.output = ConvBlock(num_stages * feat, feat, 1, 1, 0, act=False)

    def forward(self, x):
        x = self.feat1(x)
        h1 = self.up1(x)
        h2 = self.up2(self.down1(h1))
        h3 = self.up3(self.down2(h2))
        return self.output(torch.cat((h3, h2, h1), 1))


class RBPRef(nn.Module):
    def __init__(self, in_channels, out_channels, base_filter, feat, num_stages, num_resblocks, num_frames,
                 upscale_factor):
        super().__init__()
        self.t = num_frames // 2 if num_frames % 2 == 1 else num_frames // 2 - 1
        k, s, p = PROJ[upscale_factor]
        self.feat0 = ConvBlock(in_channels, base_filter)
        self.feat1 = ConvBlock(in_channels * 2, base_filter)
        self.dbp_net = DBPNet(base_filter, feat, num_stages, k, s, p)
        self.res_feat1 = nn.Sequential(*[ResnetBlock(base_filter) for _ in range(num_resblocks)],
                                       DeconvBlock(base_filter, feat, k, s, p))
        self.res_feat2 = nn.Sequential(*[ResnetBlock(feat) for _ in range(num_resblocks)], ConvBlock(feat, feat))
        self.res_feat3 = nn.Sequential(*[ResnetBlock(feat) for _ in range(num_resblocks)],
                                       ConvBlock(feat, base_filter, k, s, p))
        self.output = ConvBlock((num_frames - 1) * feat, out_channels, act=False)
        self.diff, self.sum = Stored(), Stored()

    def forward(self, inputs):
        frames = list(inputs)
        x = frames.pop(self.t)
        feat_input = self.feat0(x)
        feat_frame = [self.feat1(torch.cat([x, nb], dim=1)) for nb in frames]
        ht = []
        for ff in feat_frame:
            h0 = self.dbp_net(feat_input)
            h1 = self.res_feat1(ff)
            h = self.sum(h0 + self.res_feat2(self.diff(h0 - h1)))
            ht.append(h)
            feat_input = self.res_feat3(h)
        return self.output(torch.cat(ht, dim=1))


def perturb_slopes(net: nn.Module) -> list:
    """Set the PReLU slopes, in module order, to the cycle SLOPE_MIX (0.25,
    -0.1, 0.0, 1.5) -> the slopes set, for a fixture to store."""
    out = []
    with torch.no_grad():
        for i, m in enumerate(mm for mm in net.modules() if isinstance(mm, nn.PReLU)):
            m.weight.fill_(SLOPE_MIX[i % len(SLOPE_MIX)])
            out.append(SLOPE_MIX[i % len(SLOPE_MIX)])
    return out


def set_slopes(net: nn.Module, slopes) -> nn.Module:
    prelus = [m for m in net.modules() if isinstance(m, nn.PReLU)]
    assert len(prelus) == len(slopes)
    with torch.no_grad():
        for m, a in zip(prelus, slopes):
            m.weight.fill_(float(a))
    return net
