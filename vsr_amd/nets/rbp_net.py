"""RBPN (Recurrent Back-Projection Network, Haris et al., arXiv 1903.10128) on
the HIP kernels.

Same constructor, module tree, parameter names and creation order as the
reference RBPNet (src/model/nets/rbp_net.py:8-285), so one seed gives its
initial weights and state_dicts load both ways:

    feat0, feat1                                   ConvBlock: {conv, act}
    dbp_net.{feat1, up1, down1, up2, down2, up3, output}
        up<i>.{up_conv1: deconv, up_conv2: conv, up_conv3: deconv} (+ act each)
        down<i>.{down_conv1: conv, down_conv2: deconv, down_conv3: conv}
    res_feat1/2/3.<i>.{conv1, conv2, act}, then a DeconvBlock / ConvBlock / strided ConvBlock
    output                                         ConvBlock without activation

How the step runs:

  * Every conv is one launch with its PReLU in the epilogue.  A ResnetBlock is
    two launches: conv1 + PReLU, then conv2 with the block input as residual
    and the block's PReLU applied to the sum (VSRK_ACT_PRELU_SUM) -- the block
    tail never makes a separate pass over the tensor.
  * The strided Conv2d / ConvTranspose2d(k, s, p) projections (6/2, 7/3, 8/4,
    12/8) are 3x3 sub-pixel convs through shuffle-s views, as in drf_net.py.
  * DBPNet's concat (h3, h2, h1) and the final concat of the H_t are channel
    slices of one channels-last buffer: the producing add writes its slice,
    the consuming conv's data gradient is read back by slices.
  * dbp_net, res_feat1/2/3 and every PReLU are shared by the neighbours: each
    weight is packed once per step (once more, flipped, for the backward), and
    the weight, bias and slope gradients accumulate over the neighbours in a
    fixed order.  A ResnetBlock's one PReLU collects two contributions per
    block and neighbour.
  * The back-projection differences l0 - x, h0 - x and h0 - h1 are vsrk_sub;
    in the backward the subtrahend receives the negated gradient (0 - g, exact).
  * The backward pass is an op-level tape (tape.py).  The gradient
    contributions of a tensor with several consumers stay apart until its
    producer takes them; a PReLU backward then adds two of them in its own
    pass (vsrk_prelu_bwd's second gradient operand), so the sum and the
    derivative cost one rounding.  A PReLU output with one consumer has its
    backward, slope gradient included, in that consumer's data gradient
    (vsrk_conv_fwd_prelu_bwd, or the mask epilogue and vsrk_prelu_wgrad).
    Each rounding saved matters at 16 bits: the net is about 40 convs deep
    per neighbour.
  * A PReLU with a slope > 0 is differentiated from its output; with a slope
    <= 0 the sign of the output no longer tells the sign of the
    pre-activation, which is then recomputed by the producing conv without
    its activation (a block tail: the same conv with the plain residual
    epilogue), as nn.PReLU does.
  * res_feat3 of the last neighbour feeds nothing (rbp_net.py:86) and is not
    computed; its gradient contribution in the reference is exactly zero.

Deliberate differences from the reference:

  * The caller's list is not mutated (the reference pops the centre frame out
    of it, rbp_net.py:67).
  * num_stages != 3 raises ValueError at construction: DBPNet always
    concatenates three stages (rbp_net.py:137), so the reference fails at its
    first forward with a channel mismatch.  An upscale_factor outside
    {2, 3, 4, 8} raises likewise (the reference: UnboundLocalError).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import functional as F
from .base_net import BaseNet
from .tape import K1, K3, P0, P1, PROJ, Bwd, cp, empty_view, recorder, subpixel_cache


class _ConvBlock(nn.Module):
    def __init__(self, cin, cout, k=3, s=1, p=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, s, p)
        if act:
            self.act = nn.PReLU()


class _DeconvBlock(nn.Module):
    def __init__(self, cin, cout, k, s, p):
        super().__init__()
        self.deconv = nn.ConvTranspose2d(cin, cout, k, s, p)
        self.act = nn.PReLU()


class _ResnetBlock(nn.Module):
    """act(conv2(act(conv1(x))) + x) with ONE PReLU (rbp_net.py:212-257)."""

    def __init__(self, nf):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf, nf, 3, 1, 1)
        self.act = nn.PReLU()


class _UpBlock(nn.Module):
    def __init__(self, nf, k, s, p):
        super().__init__()
        self.up_conv1 = _DeconvBlock(nf, nf, k, s, p)
        self.up_conv2 = _ConvBlock(nf, nf, k, s, p)
        self.up_conv3 = _DeconvBlock(nf, nf, k, s, p)


class _DownBlock(nn.Module):
    def __init__(self, nf, k, s, p):
        super().__init__()
        self.down_conv1 = _ConvBlock(nf, nf, k, s, p)
        self.down_conv2 = _DeconvBlock(nf, nf, k, s, p)
        self.down_conv3 = _ConvBlock(nf, nf, k, s, p)


class _DBPNet(nn.Module):
    def __init__(self, base_filter, feat, num_stages, k, s, p):
        super().__init__()
        self.feat1 = _ConvBlock(base_filter, feat, 1, 1, 0)
        self.up1 = _UpBlock(feat, k, s, p)
        self.down1 = _DownBlock(feat, k, s, p)
        self.up2 = _UpBlock(feat, k, s, p)
        self.down2 = _DownBlock(feat, k, s, p)
        self.up3 = _UpBlock(feat, k, s, p)
        self.output = _ConvBlock(num_stages * feat, feat, 1, 1, 0, act=False)


class _Bwd(Bwd):
    """The reverse pass with the packed data-gradient weights pk and the
    sub-pixel weight cache sp.  A PReLU backward adds two of its output's
    gradient contributions in fp32 (one rounding for the sum and the
    derivative together), and a subtrahend's contribution arrives negated
    (exact), so that every merge is a sum."""

    def __init__(self, net, pk, sp, nonpos, uses, act_of):
        super().__init__(net)
        self.pk, self.sp, self.nonpos = pk, sp, nonpos
        self.uses, self.act_of = uses, act_of
        self.fused: set = set()  # PReLU outputs whose backward ran inside their one consumer's data gradient
        self._zeros: dict = {}

    def neg(self, g):
        key = (tuple(g.shape), g.dtype)
        if key not in self._zeros:
            self._zeros[key] = self.new_like(g).zero_()
        return F.sub(self._zeros[key], g, self.new_like(g))

    def prelu(self, pr, y, pre):
        """The gradient at the input of the PReLU that gave y, and its slope
        gradient, from the output y -- or, for a slope <= 0, from the
        pre-activation pre() recomputes.  Already there when y's one consumer
        fused it into its data gradient (dgrad)."""
        if id(y) in self.fused:
            return self.take(y)
        gs = self.take_list(y, 2)
        g, g2 = gs[0], (gs[1] if len(gs) > 1 else None)
        da, seen = self.buf(pr.weight)
        out = self.new_like(g)
        if id(pr) in self.nonpos:
            return F.prelu_bwd(pre(), g, pr.weight, out, da, seen, dy2=g2, pre=True)
        return F.prelu_bwd(y, g, pr.weight, out, da, seen, dy2=g2)

    def dgrad(self, xx, g, wp, k, p, **kw):
        """The data gradient of a conv with input xx.  Where xx is a PReLU
        output (slope > 0) that nothing else consumes, that PReLU's backward
        and slope gradient ride in the epilogue: vsrk_conv_fwd_prelu_bwd where
        eligible, else the PReLU mask epilogue and vsrk_prelu_wgrad."""
        out = self.new_like(xx)
        pr = self.act_of.get(id(xx))
        if pr is None or self.uses.get(id(xx)) != 1 or id(pr) in self.nonpos:
            return F.conv(g, wp, out, k, p, **kw)
        da, seen = self.buf(pr.weight)
        if not F.conv_prelu_bwd(g, wp, out, k, p, xx, pr.weight, da, seen, **kw):
            F.conv(g, wp, out, k, p, mask=xx, mask_slope=pr.weight, **kw)
            F.prelu_wgrad(xx, out, pr.weight, da, seen)
        self.fused.add(id(xx))
        return out


class RBPNet(BaseNet):
    """list of num_frames (B, C, h, w) -> the centre frame's estimate (B, C_out, r h, r w)."""

    def __init__(self, in_channels, out_channels, base_filter, feat, num_stages, num_resblocks, num_frames,
                 upscale_factor):
        super().__init__()
        if upscale_factor not in PROJ:
            raise ValueError(f"The upscale factor should be 2, 3, 4 or 8. Got {upscale_factor}.")
        if num_stages != 3:
            raise ValueError(f"RBPNet's DBPNet concatenates three back-projection stages: num_stages must be 3, "
                             f"got {num_stages}.")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.base_filter, self.feat = base_filter, feat
        self.num_frames = num_frames
        self.upscale_factor = upscale_factor
        self.t = num_frames // 2 if num_frames % 2 == 1 else num_frames // 2 - 1
        k, s, p = PROJ[upscale_factor]
        self.feat0 = _ConvBlock(in_channels, base_filter)
        self.feat1 = _ConvBlock(in_channels * 2, base_filter)
        self.dbp_net = _DBPNet(base_filter, feat, num_stages, k, s, p)
        self.res_feat1 = nn.Sequential(*[_ResnetBlock(base_filter) for _ in range(num_resblocks)],
                                       _DeconvBlock(base_filter, feat, k, s, p))
        self.res_feat2 = nn.Sequential(*[_ResnetBlock(feat) for _ in range(num_resblocks)], _ConvBlock(feat, feat))
        self.res_feat3 = nn.Sequential(*[_ResnetBlock(feat) for _ in range(num_resblocks)],
                                       _ConvBlock(feat, base_filter, k, s, p))
        self.output = _ConvBlock((num_frames - 1) * feat, out_channels, act=False)

    # ------------------------------------------------------------------
    def _specs(self, mode):
        """[(weight, mode, perm_r)] of the stride-1 convs, packed in one launch
        (the projections go through their sub-pixel images); the two input
        convs need no data gradient."""
        skip = (self.feat0.conv, self.feat1.conv) if mode == 1 else ()
        return [(m.weight, mode, 1) for m in self.modules()
                if isinstance(m, nn.Conv2d) and m.stride == (1, 1) and m not in skip]

    def _slopes_async(self):
        """The PReLU slopes on their way to the host (no sync): the backward
        reads them to choose each PReLU's form (see the module docstring)."""
        prelus = [m for m in self.modules() if isinstance(m, nn.PReLU)]
        sl = torch.cat([m.weight.detach().reshape(-1) for m in prelus])
        host = torch.empty(sl.shape, dtype=sl.dtype, pin_memory=True)
        host.copy_(sl, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(sl.device))
        return host, ev, prelus

    # ------------------------------------------------------------------
    def _run(self, inputs, tape: dict | None):
        frames = list(inputs)  # the caller's list stays as it is
        if len(frames) != self.num_frames:
            raise ValueError(f"RBPNet was built for {self.num_frames} frames, got {len(frames)}")
        cd, f, bf = self.compute_dtype, self.feat, self.base_filter
        proj = PROJ[self.upscale_factor]
        k, s, p = proj
        x = frames[self.t]
        nbs = frames[:self.t] + frames[self.t + 1:]
        B, C, h, w = x.shape
        H, W = h * s, w * s
        dev = x.device
        PR = F.ACT_PRELU
        pk = self._pack_weights(self._specs(0))
        ops, push = recorder(tape is not None)
        sp = subpixel_cache(cd)
        uses: dict = {}    # id(tensor) -> consumers (a concat consumer counts for its slices)
        act_of: dict = {}  # id(tensor) -> the PReLU that produced it

        def use(*ts):
            for t_ in ts:
                uses[id(t_)] = uses.get(id(t_), 0) + 1

        def new(hh, ww, ch, dtype=cd):
            return empty_view((B, 1, hh, ww), ch, dtype, dev)

        def conv(xx, m, y, pr=None, parts=None, need_dx=True):
            """y = [prelu](conv(xx) + bias); parts: the channel slices of xx that are tensors of their own."""
            kk, pp = (K3, P1) if m.kernel_size[0] == 3 else (K1, P0)
            w0 = pk[(id(m.weight), 0, 1)]
            F.conv(xx, w0, y, kk, pp, bias=m.bias, act=PR if pr is not None else F.ACT_NONE,
                   act_param=pr.weight if pr is not None else None)
            use(*([t_ for t_, _, _ in parts] if parts is not None else [xx]))
            if pr is not None:
                act_of[id(y)] = pr

            def bwd(bk):
                if pr is not None:
                    g = bk.prelu(pr, y, lambda: F.conv(xx, w0, bk.new_like(y), kk, pp, bias=m.bias))
                else:
                    g = bk.take(y)
                bk.conv_wgrad(m, xx, g, kk, pp)
                if need_dx:
                    bk.route(xx, parts, bk.dgrad(xx, g, bk.pk[(id(m.weight), 1, 1)], kk, pp))

            push(bwd)
            return y

        def deconv(xx, blk, y):
            """y = prelu(ConvTranspose2d(k, s, p)(xx)): a 3x3 conv written through the shuffle-s view of y."""
            m, pr = blk.deconv, blk.act
            wq, bq = sp(m, proj, True)
            code = F.subpixel_code(k, s, p, True, False)
            F.conv(xx, wq, y, K3, P1, bias=bq, bias_r=1, y_shuffle=s, act=PR, act_param=pr.weight, subpixel=code)
            use(xx)
            act_of[id(y)] = pr

            def bwd(bk):
                g = bk.prelu(pr, y, lambda: F.conv(xx, wq, bk.new_like(y), K3, P1, bias=bq, bias_r=1, y_shuffle=s,
                                                   subpixel=code))
                bk.subpixel_wgrad(m, xx, g, proj, True, tap_skip=True)
                bk.acc(xx, bk.dgrad(xx, g, bk.sp(m, proj, True, 1)[0], K3, P1, x_shuffle=s,
                                    subpixel=F.subpixel_code(k, s, p, True, True)))

            push(bwd)
            return y

        def sconv(xx, blk, y):
            """y = prelu(Conv2d(k, stride s, p)(xx)): a 3x3 conv over the shuffle-s view of xx."""
            m, pr = blk.conv, blk.act
            wq, bq = sp(m, proj, False)
            code = F.subpixel_code(k, s, p, False, False)
            F.conv(xx, wq, y, K3, P1, bias=bq, x_shuffle=s, act=PR, act_param=pr.weight, subpixel=code)
            use(xx)
            act_of[id(y)] = pr

            def bwd(bk):
                g = bk.prelu(pr, y, lambda: F.conv(xx, wq, bk.new_like(y), K3, P1, bias=bq, x_shuffle=s,
                                                   subpixel=code))
                bk.subpixel_wgrad(m, xx, g, proj, False, tap_skip=True)
                bk.acc(xx, bk.dgrad(xx, g, bk.sp(m, proj, False, 1)[0], K3, P1, y_shuffle=s,
                                    subpixel=F.subpixel_code(k, s, p, False, True)))

            push(bwd)
            return y

        def resblock(xx, blk):
            """prelu(conv2(prelu(conv1(xx))) + xx): the tail is one launch, the PReLU applied to the sum."""
            _, _, hh, ww, ch = xx.shape
            t1 = conv(xx, blk.conv1, new(hh, ww, ch), blk.act)
            m, pr = blk.conv2, blk.act
            w2 = pk[(id(m.weight), 0, 1)]
            y = F.conv(t1, w2, new(hh, ww, ch), K3, P1, bias=m.bias, residual=xx, act=F.ACT_PRELU_SUM,
                       act_param=pr.weight)
            use(t1, xx)
            act_of[id(y)] = pr

            def bwd(bk):
                g = bk.prelu(pr, y, lambda: F.conv(t1, w2, bk.new_like(y), K3, P1, bias=m.bias, residual=xx))
                bk.acc(xx, g)
                bk.conv_wgrad(m, t1, g, K3, P1)
                bk.acc(t1, bk.dgrad(t1, g, bk.pk[(id(m.weight), 1, 1)], K3, P1))

            push(bwd)
            return y

        def sub(a, b, y):
            F.sub(a, b, y)
            use(a, b)

            def bwd(bk):
                g = bk.take(y)
                bk.acc(a, g)
                bk.acc(b, bk.neg(g))

            push(bwd)
            return y

        def add(a, b, y):
            F.add(a, b, y)
            use(a, b)

            def bwd(bk):
                for g in bk.take_list(y, 2):  # (a PReLU backward downstream adds two in one pass)
                    bk.acc(a, g)
                    bk.acc(b, g)

            push(bwd)
            return y

        def up(xx, blk, y):
            """UpBlock (rbp_net.py:260-271): LR xx -> HR y = up_conv3(up_conv2(h0) - xx) + h0."""
            h0 = deconv(xx, blk.up_conv1, new(H, W, f))
            l0 = sconv(h0, blk.up_conv2, new(h, w, f))
            h1 = deconv(sub(l0, xx, new(h, w, f)), blk.up_conv3, new(H, W, f))
            return add(h1, h0, y)

        def down(xx, blk):
            """DownBlock (rbp_net.py:274-285): HR xx -> LR down_conv3(down_conv2(l0) - xx) + l0."""
            l0 = sconv(xx, blk.down_conv1, new(h, w, f))
            h0 = deconv(l0, blk.down_conv2, new(H, W, f))
            l1 = sconv(sub(h0, xx, new(H, W, f)), blk.down_conv3, new(h, w, f))
            return add(l1, l0, new(h, w, f))

        def dbp(xx):
            """DBPNet (rbp_net.py:129-139): the concat (h3, h2, h1) is one buffer."""
            d = self.dbp_net
            x1 = conv(xx, d.feat1.conv, new(h, w, f), d.feat1.act)
            cat = new(H, W, 3 * f)
            h3, h2, h1 = cat[..., :f], cat[..., f:2 * f], cat[..., 2 * f:]
            up(x1, d.up1, h1)
            up(down(h1, d.down1), d.up2, h2)
            up(down(h2, d.down2), d.up3, h3)
            return conv(cat, d.output.conv, new(H, W, f), parts=[(h3, 0, f), (h2, f, 2 * f), (h1, 2 * f, 3 * f)])

        def blocks(seq, xx):
            for blk in list(seq)[:-1]:
                xx = resblock(xx, blk)
            return xx

        xf = x.float()
        xv = F.to_view(xf, cd, cpad=cp(C))[..., :C]
        feat_input = conv(xv, self.feat0.conv, new(h, w, bf), self.feat0.act, need_dx=False)
        feat_frame = []
        for nb in nbs:
            pair = F.to_view(torch.cat([xf, nb.float()], dim=1), cd, cpad=cp(2 * C))[..., :2 * C]
            feat_frame.append(conv(pair, self.feat1.conv, new(h, w, bf), self.feat1.act, need_dx=False))
        nn_ = len(nbs)
        HT = new(H, W, nn_ * f)
        parts = []
        for j in range(nn_):
            h0 = dbp(feat_input)
            h1 = deconv(blocks(self.res_feat1, feat_frame[j]), self.res_feat1[-1], new(H, W, f))
            e = sub(h0, h1, new(H, W, f))
            last = self.res_feat2[-1]
            e = conv(blocks(self.res_feat2, e), last.conv, new(H, W, f), last.act)
            hj = HT[..., j * f:(j + 1) * f]
            add(h0, e, hj)
            parts.append((hj, j * f, (j + 1) * f))
            if j + 1 < nn_:  # (the last neighbour's res_feat3 feeds nothing)
                feat_input = sconv(blocks(self.res_feat3, hj), self.res_feat3[-1], new(h, w, bf))
        co = self.out_channels
        yv = conv(HT, self.output.conv, new(H, W, co, torch.float32), parts=parts)
        y = F.from_view(yv)
        if tape is not None:
            tape.update(ops=ops, yv=yv, sp=sp, uses=uses, act_of=act_of, slopes=self._slopes_async())
        return y

    # ------------------------------------------------------------------
    def _backward(self, tape: dict, grads) -> dict:
        g = grads.float()
        host, ev, prelus = tape["slopes"]
        ev.synchronize()
        nonpos = {id(m) for m, a in zip(prelus, host.tolist()) if not a > 0}
        co = self.out_channels
        bk = _Bwd(self, self._pack_weights(self._specs(1)), tape["sp"], nonpos, tape["uses"], tape["act_of"])
        return bk.run(tape["ops"], tape["yv"], F.to_view(g, self.compute_dtype, cpad=cp(co))[..., :co])
