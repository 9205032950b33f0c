"""EDVR (Wang et al., arXiv 1905.02716) on the HIP kernels: PCD alignment with
modulated deformable convolutions and TSA fusion.

Same constructor, module tree, state_dict keys, construction order and
initialisation as the reference EDVRNet (src/model/nets/edvr_net/
EDVR_arch.py:13-321 over arch_util.py:7-52 and dcn/deform_conv.py:221-291),
so one seed gives its initial weights and its checkpoints load: the
residual-block convs are Kaiming normal x 0.1 with zero bias, a DCN weight is
uniform in +-1/sqrt(fan_in) with zero bias, every conv_offset_mask is zeroed,
everything else is torch's default.  predeblur=True and HR_in=True raise
NotImplementedError: no config of the reference uses them.  w_TSA=False (one
1x1 fusion conv) is supported.

How the step runs (the structure the reference allows):

  * Feature extraction and the whole PCD alignment run ONCE over a batch of
    B N frames: the reference's per-frame loop (:117-122) shares all weights,
    so the centre frame's features are broadcast into the second half of each
    concat input and every weight gradient is one launch.
  * Concat inputs are never assembled: producers store into channel slices of
    one buffer; a consumer's data gradient is read back by slices.
  * Activations are channels-last views from the first conv to the last.
    LeakyReLU(0.1) is the conv epilogue VSRK_ACT_PRELU on a constant device
    slope; the stride-2 convs are sub-pixel 3x3 convs over shuffle-2 input
    views; PixelShuffle(2) is a shuffle-2 output view (the LeakyReLU after it
    commutes into the epilogue); bilinear x2 is vsrk_upsample_cl; the x4
    bilinear base image is vsrk_upsample2d accumulated onto the fp32 output.
  * A DCN pack: conv_offset_mask writes an fp32 view that vsrk_dcn_view_im2col
    reads raw (chunk, cat and sigmoid are folded in), the columns go through
    the library's 1x1 conv (bias, and the LeakyReLU where the reference
    applies one right after the DCN, in its epilogue).  Backward: the 1x1 data
    and weight gradients, vsrk_dcn_view_coord_grad into the output gradient of
    conv_offset_mask, vsrk_dcn_view_col2im for the input.  Offsets, masks and
    their gradients stay fp32 in every compute precision; the backward of
    conv_offset_mask itself rounds that gradient to bf16, and under fp16, where
    rounding it missed the fixtures' gradient bound, runs in fp32.  The pack's
    weight, permuted to (Cout, 9 C) in a persistent buffer, is packed with all
    the other weights.
  * TSA: vsrk_tsa_tatt, vsrk_pool3s2 (max | avg in one pass) and
    vsrk_tsa_modulate, forward and backward.
  * `L3_offset * 2` / `L2_offset * 2` (:232, 241) are an in-place multiply of
    the upsampled slice (exact in every precision).
  * H, W off multiples of 4: padded with the global minimum of the stacked
    input (computed on the device, no host read) and the output is cropped,
    in torch plumbing, as the reference does (:73-80, 141-144).

The backward pass is an op-level tape (tape.py); the gradients of a tensor
with several consumers are summed as they arrive (_Bwd.acc), so that only one
is held at a time.

Deliberately not reproduced: the pack's `offset_mean > 100` warning
(deform_conv.py:285-287) costs a host read per DCN per step.

The forward is bitwise reproducible.  Gradients are not: the DCN input
gradient is a float-atomic scatter (vsrk_dcn_view_col2im), the library's one
sum that is not in a fixed order.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import functional as F
from .base_net import BaseNet
from .tape import K1, K3, P0, P1, Bwd, cp, empty_view, recorder, subpixel_cache

_S2 = (3, 2, 1)  # kernel, stride, padding of the stride-2 feature convs
LEAKY, RELU = "leaky", "relu"


class _ResBlock(nn.Module):
    """arch_util.ResidualBlock_noBN: x + conv2(relu(conv1(x)))."""

    def __init__(self, nf):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        for c in (self.conv1, self.conv2):
            nn.init.kaiming_normal_(c.weight, a=0, mode="fan_in")
            c.weight.data *= 0.1
            c.bias.data.zero_()


class _DCNPack(nn.Module):
    """The parameters of ModulatedDeformConvPack(nf, nf, 3, 1, 1, extra_offset_mask=True)."""

    def __init__(self, nf, groups):
        super().__init__()
        self.deformable_groups = groups
        self.weight = nn.Parameter(torch.Tensor(nf, nf, 3, 3))
        self.bias = nn.Parameter(torch.Tensor(nf))
        stdv = 1. / math.sqrt(nf * 9)
        self.weight.data.uniform_(-stdv, stdv)
        self.bias.data.zero_()
        self.conv_offset_mask = nn.Conv2d(nf, groups * 27, 3, 1, 1)
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()


class PCDAlign(nn.Module):
    def __init__(self, nf=64, groups=8):
        super().__init__()
        self.L3_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L3_offset_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L3_dcnpack = _DCNPack(nf, groups)
        self.L2_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L2_offset_conv2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L2_offset_conv3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L2_dcnpack = _DCNPack(nf, groups)
        self.L2_fea_conv = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.L1_offset_conv3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.L1_dcnpack = _DCNPack(nf, groups)
        self.L1_fea_conv = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv1 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.cas_offset_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.cas_dcnpack = _DCNPack(nf, groups)


class TSAFusion(nn.Module):
    def __init__(self, nf=64, nframes=5, center=2):
        super().__init__()
        self.center = center
        self.tAtt_1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.tAtt_2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.fea_fusion = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.sAtt_1 = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.sAtt_2 = nn.Conv2d(nf * 2, nf, 1, 1)
        self.sAtt_3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_4 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_5 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_L1 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_L2 = nn.Conv2d(nf * 2, nf, 3, 1, 1)
        self.sAtt_L3 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.sAtt_add_1 = nn.Conv2d(nf, nf, 1, 1)
        self.sAtt_add_2 = nn.Conv2d(nf, nf, 1, 1)


class _Bwd(Bwd):
    """The reverse pass with the packed data-gradient weights pk; a tensor's
    gradient contributions are summed on arrival, left to right, which frees
    both operands there (the peak at 5 x 128 x 128 x 64 depends on it)."""

    def __init__(self, net, dev, pk, sp):
        super().__init__(net)
        self.pk, self.sp = pk, sp
        self.cd = net.compute_dtype
        self.slope = net._const(dev, 0.1)
        self.dummy = torch.empty(1, dtype=torch.float32, device=dev)

    def acc(self, t, g):
        old = self.G.get(id(t))
        self.G[id(t)] = [g] if old is None else [F.add(old[0], g, self.new_like(g))]

    def act_bwd(self, act, y, g):
        if g.dtype != self.cd:  # the fp32 gradient of an fp32 view (offsets and masks), rounded for the conv's backward
            t = self.new_like(g, self.cd, zero=True)
            t.copy_(g)
            g = t
        if act == LEAKY:
            return F.prelu_bwd(y, g, self.slope, self.new_like(g), self.dummy, False)
        if act == RELU:
            return F.relu_bwd(y, g, self.new_like(g))
        return g


class EDVRNet(BaseNet):
    """list of N frames (B, C, h, w) -> the centre frame's estimate (B, C, 4h, 4w)."""

    def __init__(self, in_channels, out_channels, nf=64, nframes=5, groups=8, front_RBs=5, back_RBs=10, center=None,
                 predeblur=False, HR_in=False, w_TSA=True):
        super().__init__()
        if predeblur:
            raise NotImplementedError("EDVRNet: predeblur=True (the pre-deblur pyramid) is not implemented; no config "
                                      "of the reference uses it")
        if HR_in:
            raise NotImplementedError("EDVRNet: HR_in=True (high-resolution input) is not implemented; no config of "
                                      "the reference uses it")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.nf = nf
        self.nframes = nframes
        self.center = nframes // 2 if center is None else center
        self.is_predeblur = False
        self.HR_in = False
        self.w_TSA = w_TSA
        self.conv_first = nn.Conv2d(in_channels, nf, 3, 1, 1)
        self.feature_extraction = nn.Sequential(*[_ResBlock(nf) for _ in range(front_RBs)])
        self.fea_L2_conv1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.fea_L2_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.fea_L3_conv1 = nn.Conv2d(nf, nf, 3, 2, 1)
        self.fea_L3_conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.pcd_align = PCDAlign(nf=nf, groups=groups)
        if w_TSA:
            self.tsa_fusion = TSAFusion(nf=nf, nframes=nframes, center=self.center)
        else:
            self.tsa_fusion = nn.Conv2d(nframes * nf, nf, 1, 1)
        self.recon_trunk = nn.Sequential(*[_ResBlock(nf) for _ in range(back_RBs)])
        self.upconv1 = nn.Conv2d(nf, nf * 4, 3, 1, 1)
        self.upconv2 = nn.Conv2d(nf, 64 * 4, 3, 1, 1)
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.HRconv = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, out_channels, 3, 1, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.1, inplace=True)
        self._w1: dict = {}

    # ------------------------------------------------------------------
    def _packs(self):
        p = self.pcd_align
        return [p.L3_dcnpack, p.L2_dcnpack, p.L1_dcnpack, p.cas_dcnpack]

    def _columns_weight(self, pack) -> torch.Tensor:
        """The pack's weight as the 1x1 conv (Cout, 9 C, 1, 1) over columns k C + c,
        refreshed in a persistent buffer so that it is packed with all the others."""
        w = pack.weight
        key = (id(w), w.device)
        buf = self._w1.get(key)
        if buf is None:
            buf = self._w1[key] = torch.empty((w.shape[0], 9 * w.shape[1], 1, 1), dtype=torch.float32, device=w.device)
        buf.view(w.shape[0], 3, 3, w.shape[1]).copy_(w.detach().permute(0, 2, 3, 1))
        return buf

    def _specs(self, mode):
        """[(weight, mode, perm_r)] of every conv packed in the one launch: the
        plain convs, the two pixel-shuffle convs and the DCN column weights
        (the stride-2 convs go through their sub-pixel images)."""
        strided = (self.fea_L2_conv1, self.fea_L3_conv1)
        ups = (self.upconv1, self.upconv2)
        out = []
        for m in self.modules():
            if isinstance(m, nn.Conv2d) and m not in strided and not (mode == 1 and m is self.conv_first):
                out.append((m.weight, mode, 2 if m in ups else 1))
        return out + [(self._columns_weight(p), mode, 1) for p in self._packs()]

    # ------------------------------------------------------------------
    def _run(self, inputs, tape: dict | None):
        cd, nf, cen = self.compute_dtype, self.nf, self.center
        X = torch.stack([x.float() for x in inputs], dim=1)                 # (B, N, C, H, W)
        B, N, C, H0, W0 = X.shape
        if N != self.nframes and self.w_TSA:
            raise ValueError(f"EDVRNet was built for {self.nframes} frames, got {N}")
        dev = X.device
        hd, wd = -H0 % 4, -W0 % 4
        top, left = hd // 2, wd // 2
        H, W = H0 + hd, W0 + wd
        if hd or wd:  # F.pad(x, value=x.min()), the minimum staying on the device
            padded = X.amin().expand(B, N, C, H, W).clone()
            padded[..., top:top + H0, left:left + W0] = X
            X = padded
        BN = B * N
        slope = self._const(dev, 0.1)
        pk = self._pack_weights(self._specs(0))
        sp = subpixel_cache(cd)
        ops, push = recorder(tape is not None)
        pa, ts = self.pcd_align, self.tsa_fusion

        def new(b, hh, ww, ch, dtype=cd, zero=False):
            return empty_view((b, 1, hh, ww), ch, dtype, dev, zero)

        def conv(x, m, y, act=None, residual=None, parts=None, need_dx=True, shuffle=1):
            """y = act(conv(x) + bias [+ residual]); parts: the channel slices of x that are tensors of their own."""
            k, p = (K3, P1) if m.kernel_size[0] == 3 else (K1, P0)
            F.conv(x, pk[(id(m.weight), 0, shuffle)], y, k, p, bias=m.bias, residual=residual, y_shuffle=shuffle,
                   act={LEAKY: F.ACT_PRELU, RELU: F.ACT_RELU, None: F.ACT_NONE}[act],
                   act_param=slope if act == LEAKY else None)

            def bwd(bk):
                g = bk.take(y)
                if g.dtype == torch.float32 and cd == torch.float16:
                    # conv_offset_mask under fp16: with the offset and mask gradients rounded to fp16 the L3 weight
                    # gradient missed its bound (edvr_x4_pad), so this conv's backward runs in fp32
                    x32 = bk.new_like(x, torch.float32, zero=True)
                    x32.copy_(x)
                    bk.conv_wgrad(m, x32, g, k, p)
                    gx = F.conv(g, F.pack_weight(m.weight, 1, torch.float32), bk.new_like(x, torch.float32), k, p)
                    g16 = bk.new_like(x)
                    g16.copy_(gx)
                    bk.route(x, parts, g16)
                    return
                g = bk.act_bwd(act, y, g)
                if residual is not None:
                    bk.acc(residual, g)
                bk.conv_wgrad(m, x, g, k, p, perm_r=shuffle, dy_shuffle=shuffle)
                if need_dx:
                    gx = F.conv(g, bk.pk[(id(m.weight), 1, shuffle)], bk.new_like(x), k, p, x_shuffle=shuffle)
                    bk.route(x, parts, gx)

            push(bwd)
            return y

        def sconv(x, m, y):
            """LeakyReLU(Conv2d(3, stride 2, pad 1)): a sub-pixel 3x3 conv over the shuffle-2 view of x."""
            s_ = _S2[1]
            wq, beq = sp(m, _S2, False)
            F.conv(x, wq, y, K3, P1, bias=beq, x_shuffle=s_, act=F.ACT_PRELU, act_param=slope)

            def bwd(bk):
                g = bk.act_bwd(LEAKY, y, bk.take(y))
                bk.subpixel_wgrad(m, x, g, _S2, False, tap_skip=False)
                bk.acc(x, F.conv(g, bk.sp(m, _S2, False, 1)[0], bk.new_like(x), K3, P1, y_shuffle=s_))

            push(bwd)
            return y

        def resblocks(seq, x, last=None):
            """The residual blocks; the last one stores into `last` when given."""
            for i, blk in enumerate(seq):
                b_, _, hh, ww, _ = x.shape
                a = conv(x, blk.conv1, new(b_, hh, ww, nf), RELU)
                dst = last if (last is not None and i == len(seq) - 1) else new(b_, hh, ww, nf)
                x = conv(a, blk.conv2, dst, residual=x)
            return x

        def cat2(b, hh, ww):
            buf = new(b, hh, ww, 2 * nf)
            lo, hi = buf[..., :nf], buf[..., nf:]
            return buf, lo, hi, [(lo, 0, nf), (hi, nf, 2 * nf)]

        def put_ref(src, dst):
            """dst of every frame = src of its clip's centre frame."""
            dst.unflatten(0, (B, N)).copy_(src.unflatten(0, (B, N))[:, cen:cen + 1])

            def bwd(bk):
                g = bk.take(dst).unflatten(0, (B, N)).sum(dim=1)
                z = torch.zeros((B, N, *g.shape[1:]), dtype=g.dtype, device=dev)
                z[:, cen] = g
                bk.acc(src, z.flatten(0, 1))

            push(bwd)

        def up2(x, y, scale=None):
            F.upsample_cl(x, y, 2, False)
            if scale:
                y.mul_(scale)

            def bwd(bk):
                g = bk.take(y)
                if scale:
                    g = g * scale
                bk.acc(x, F.upsample_cl_bwd(g, bk.new_like(x), 2, False))

            push(bwd)
            return y

        def dcn(x, fea, pack, y, act=None):
            """One DCN pack: x sampled at the offsets that conv_offset_mask derives from fea."""
            b_, _, hh, ww, _ = x.shape
            G_ = pack.deformable_groups
            om = conv(fea, pack.conv_offset_mask, new(b_, hh, ww, 27 * G_, torch.float32, zero=True))
            geo, _, _ = F.dcn_geometry(x, deformable_groups=G_)
            cols = torch.empty((b_, 1, hh, ww, 9 * nf), dtype=cd, device=dev)
            F.dcn_view_im2col(geo, x, om, cols)
            w1 = self._w1[(id(pack.weight), pack.weight.device)]
            F.conv(cols, pk[(id(w1), 0, 1)], y, K1, P0, bias=pack.bias,
                   act=F.ACT_PRELU if act == LEAKY else F.ACT_NONE, act_param=slope if act == LEAKY else None)

            def bwd(bk):
                g = bk.act_bwd(act, y, bk.take(y))
                gcols = F.conv(g, bk.pk[(id(w1), 1, 1)], bk.new_like(cols), K1, P0)
                dw1 = torch.empty((nf, 9 * nf, 1, 1, 1), dtype=torch.float32, device=dev)
                F.conv_wgrad(cols, g, K1, P0, dw1, bk.buf(pack.bias)[0])
                bk.buf(pack.weight)[0].copy_(dw1.view(nf, 3, 3, nf).permute(0, 3, 1, 2))
                bk.acc(om, F.dcn_view_coord_grad(geo, x, gcols, om, bk.new_like(om, zero=True)))
                gx = torch.zeros(x.shape, dtype=torch.float32, device=dev)
                F.dcn_view_col2im(geo, gcols, om, gx)
                bk.acc(x, gx if cd == torch.float32 else gx.to(cd))

            push(bwd)
            return y

        h2, w2, h3, w3 = H // 2, W // 2, H // 4, W // 4
        # ---- features of all B N frames; each level's result is the first half of its concat buffer
        x0 = F.to_view(X.reshape(BN, C, H, W), cd, cpad=cp(C))[..., :C]
        c1, l1, r1, p1 = cat2(BN, H, W)
        c2, l2, r2, p2 = cat2(BN, h2, w2)
        c3, l3, r3, p3 = cat2(BN, h3, w3)
        nrb = len(self.feature_extraction)
        f = conv(x0, self.conv_first, l1 if nrb == 0 else new(BN, H, W, nf), LEAKY, need_dx=False)
        resblocks(self.feature_extraction, f, l1)
        put_ref(l1, r1)
        conv(sconv(l1, self.fea_L2_conv1, new(BN, h2, w2, nf)), self.fea_L2_conv2, l2, LEAKY)
        put_ref(l2, r2)
        conv(sconv(l2, self.fea_L3_conv1, new(BN, h3, w3, nf)), self.fea_L3_conv2, l3, LEAKY)
        put_ref(l3, r3)
        # ---- PCD alignment, all frames at once
        o3 = conv(c3, pa.L3_offset_conv1, new(BN, h3, w3, nf), LEAKY, parts=p3)
        o3 = conv(o3, pa.L3_offset_conv2, new(BN, h3, w3, nf), LEAKY)
        f3 = dcn(l3, o3, pa.L3_dcnpack, new(BN, h3, w3, nf), LEAKY)
        co2, o2a, o3u, po2 = cat2(BN, h2, w2)
        conv(c2, pa.L2_offset_conv1, o2a, LEAKY, parts=p2)
        up2(o3, o3u, 2.0)
        o2 = conv(co2, pa.L2_offset_conv2, new(BN, h2, w2, nf), LEAKY, parts=po2)
        o2 = conv(o2, pa.L2_offset_conv3, new(BN, h2, w2, nf), LEAKY)
        cf2, f2a, f3u, pf2 = cat2(BN, h2, w2)
        dcn(l2, o2, pa.L2_dcnpack, f2a)
        up2(f3, f3u)
        f2 = conv(cf2, pa.L2_fea_conv, new(BN, h2, w2, nf), LEAKY, parts=pf2)
        co1, o1a, o2u, po1 = cat2(BN, H, W)
        conv(c1, pa.L1_offset_conv1, o1a, LEAKY, parts=p1)
        up2(o2, o2u, 2.0)
        o1 = conv(co1, pa.L1_offset_conv2, new(BN, H, W, nf), LEAKY, parts=po1)
        o1 = conv(o1, pa.L1_offset_conv3, new(BN, H, W, nf), LEAKY)
        cf1, f1a, f2u, pf1 = cat2(BN, H, W)
        dcn(l1, o1, pa.L1_dcnpack, f1a)
        up2(f2, f2u)
        cc, f1, rc, pc = cat2(BN, H, W)
        conv(cf1, pa.L1_fea_conv, f1, parts=pf1)
        put_ref(l1, rc)
        off = conv(cc, pa.cas_offset_conv1, new(BN, H, W, nf), LEAKY, parts=pc)
        off = conv(off, pa.cas_offset_conv2, new(BN, H, W, nf), LEAKY)
        aligned = dcn(f1, off, pa.cas_dcnpack, new(BN, H, W, nf), LEAKY)
        # ---- fusion
        if self.w_TSA:
            ac = aligned.unflatten(0, (B, N))[:, cen].contiguous()

            def ac_bwd(bk):
                g = bk.take(ac)
                z = torch.zeros((B, N, *g.shape[1:]), dtype=g.dtype, device=dev)
                z[:, cen] = g
                bk.acc(aligned, z.flatten(0, 1))

            push(ac_bwd)
            emb_ref = conv(ac, ts.tAtt_2, new(B, H, W, nf))
            emb = conv(aligned, ts.tAtt_1, new(BN, H, W, nf))
            wal = new(B, H, W, N * nf)
            prob = torch.empty((B, N, H, W), dtype=torch.float32, device=dev)
            F.tsa_tatt(emb, emb_ref, aligned, wal, prob)

            def tatt_bwd(bk):
                ge, gr, ga = bk.new_like(emb), bk.new_like(emb_ref), bk.new_like(aligned)
                F.tsa_tatt_bwd(emb, emb_ref, aligned, prob, bk.take(wal), ge, gr, ga)
                bk.acc(emb, ge)
                bk.acc(emb_ref, gr)
                bk.acc(aligned, ga)

            push(tatt_bwd)
            fea = conv(wal, ts.fea_fusion, new(B, H, W, nf), LEAKY)
            att = conv(wal, ts.sAtt_1, new(B, H, W, nf), LEAKY)

            def pool(x):
                b_, _, hh, ww, ch = x.shape
                y = F.pool3s2(x, new(b_, (hh - 1) // 2 + 1, (ww - 1) // 2 + 1, 2 * ch))
                push(lambda bk: bk.acc(x, F.pool3s2_bwd(x, bk.take(y), bk.new_like(x))))
                return y

            att = conv(pool(att), ts.sAtt_2, new(B, h2, w2, nf), LEAKY)
            att_l = conv(att, ts.sAtt_L1, new(B, h2, w2, nf), LEAKY)
            att_l = conv(pool(att_l), ts.sAtt_L2, new(B, h3, w3, nf), LEAKY)
            att_l = conv(att_l, ts.sAtt_L3, new(B, h3, w3, nf), LEAKY)
            att_lu = up2(att_l, new(B, h2, w2, nf))
            att3 = conv(att, ts.sAtt_3, new(B, h2, w2, nf), LEAKY)
            asum = F.add(att3, att_lu, new(B, h2, w2, nf))

            def add_bwd(bk):
                g = bk.take(asum)
                bk.acc(att3, g)
                bk.acc(att_lu, g)

            push(add_bwd)
            att4 = conv(asum, ts.sAtt_4, new(B, h2, w2, nf), LEAKY)
            att4u = up2(att4, new(B, H, W, nf))
            att5 = conv(att4u, ts.sAtt_5, new(B, H, W, nf))
            add1 = conv(att5, ts.sAtt_add_1, new(B, H, W, nf), LEAKY)
            att_add = conv(add1, ts.sAtt_add_2, new(B, H, W, nf))
            fused = F.tsa_modulate(fea, att5, att_add, new(B, H, W, nf))

            def mod_bwd(bk):
                gf, ga, gadd = bk.new_like(fea), bk.new_like(att5), bk.new_like(att_add)
                F.tsa_modulate_bwd(fea, att5, bk.take(fused), gf, ga, gadd)
                bk.acc(fea, gf)
                bk.acc(att5, ga)
                bk.acc(att_add, gadd)

            push(mod_bwd)
        else:
            wide = aligned.unflatten(0, (B, N)).permute(0, 2, 3, 4, 1, 5).reshape(B, 1, H, W, N * nf)

            def wide_bwd(bk):
                g = bk.take(wide).view(B, 1, H, W, N, nf).permute(0, 4, 1, 2, 3, 5).reshape(BN, 1, H, W, nf)
                bk.acc(aligned, g)

            push(wide_bwd)
            fused = conv(wide, ts, new(B, H, W, nf))
        # ---- reconstruction
        out = resblocks(self.recon_trunk, fused)
        out = conv(out, self.upconv1, new(B, 2 * H, 2 * W, nf), LEAKY, shuffle=2)
        out = conv(out, self.upconv2, new(B, 4 * H, 4 * W, 64), LEAKY, shuffle=2)
        out = conv(out, self.HRconv, new(B, 4 * H, 4 * W, 64), LEAKY)
        yv = conv(out, self.conv_last, new(B, 4 * H, 4 * W, self.out_channels, torch.float32))
        y = F.from_view(yv)                                                 # (B, C, 4H, 4W) fp32
        if self.in_channels != self.out_channels:
            raise ValueError("EDVRNet adds the upsampled centre frame to its output: in_channels must equal "
                             "out_channels")
        F.upsample2d(X[:, cen].contiguous(), y, "bilinear", False, 4, accumulate=True)
        if tape is not None:
            tape.update(ops=ops, yv=yv, sp=sp, geom=(B, H, W, H0, W0, top, left))
        if hd or wd:
            y = y[..., top * 4:(top + H0) * 4, left * 4:(left + W0) * 4].contiguous()
        return y

    # ------------------------------------------------------------------
    def _backward(self, tape: dict, grads) -> dict:
        B, H, W, H0, W0, top, left = tape["geom"]
        g = grads.float()
        dev = g.device
        if (H, W) != (H0, W0):
            full = torch.zeros((B, g.shape[1], 4 * H, 4 * W), dtype=torch.float32, device=dev)
            full[..., top * 4:(top + H0) * 4, left * 4:(left + W0) * 4] = g
            g = full
        co = self.out_channels
        bk = _Bwd(self, dev, self._pack_weights(self._specs(1)), tape["sp"])
        return bk.run(tape["ops"], tape["yv"], F.to_view(g, self.compute_dtype, cpad=cp(co))[..., :co])
