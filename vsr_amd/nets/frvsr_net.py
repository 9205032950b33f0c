"""Frame-recurrent video super-resolution (FRVSR) on the HIP kernels.

Same constructor, module tree, state_dict keys, construction order and Xavier
pass as the reference FRVSRNet (src/model/nets/frvsr_net.py:11-240), so one
seed gives its initial weights and its checkpoints load:

    srnet.head.conv                   conv3x3 C (r^2 + 1) -> 64, ReLU   (:80-81)
    srnet.body.{i}.body.conv1 / conv2 resblock conv3x3 64 -> 64         (:98-107)
    srnet.tail.deconv1 / deconv2      ConvTranspose2d(3, 2, 1, 1), ReLU (:84-87)
    srnet.tail.conv                   conv3x3 64 -> out                 (:88)
    fnet.body.conv{k}_1 / conv{k}_2   conv3x3 + LeakyReLU(0.2), k = 1..6 (:120-137)
    fnet.tail.conv1 / conv2           conv3x3 + LeakyReLU, conv3x3 + tanh (:139-143)

How the step runs (the structure the reference allows: neither warped image
carries a gradient, frvsr_net.py:49,55, so there is no backpropagation
through time):

  * FNet runs ONCE over all T frame pairs as a batch of N T, forward and
    backward: convs with the LeakyReLU in the epilogue (VSRK_ACT_PRELU with a
    constant device slope 0.2), vsrk_max_pool2x2, vsrk_upsample_cl.  Its last
    conv writes an fp32 view and the flow stays fp32 through vsrk_tanh and
    both warps, whatever the compute dtype.
  * The T low-resolution warps are one vsrk_flow_warp launch.
  * Only the SR net's forward is sequential: per frame, the previous estimate
    is warped from the LOW-resolution flow (flow_up = r interpolates it inside
    the kernel) and stored through SpaceToDepth(r) straight into the head's
    concat input (s2d = r); the deconvs are 3x3 sub-pixel convs written through
    shuffle-2 views.  Its backward runs frame by frame, in ascending t: the
    shared weights' gradients accumulate over the frames in that order, which
    is why the two backward loops are written out and are not a reverse tape
    (tape.py supplies the gradient ledger, the sub-pixel weight cache and the
    view allocation only).
  * The warp's space-to-depth channel order is (i r + j) C + c', the
    reference's c' r^2 + i r + j: equal for C = 1; for C > 1 the head weight's
    input channels are permuted when packed and its gradient permuted back.
  * H, W that are no multiples of 8: the frame pairs are padded with the
    per-pair batch minimum (computed on the device, no host read) and the flow
    is cropped, in torch plumbing, as the reference does (:149-166).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import functional as F
from .base_net import BaseNet
from .tape import K3, P1, ParamGrads, cp, empty_view, subpixel_cache

_DECONV = (3, 2, 1)  # kernel, stride, padding of the tail's deconvs (output_padding 1 = s - k + 2p)


class _ResBlock(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.body = nn.Sequential()
        self.body.add_module("conv1", nn.Conv2d(f, f, 3, padding=1))
        self.body.add_module("relu1", nn.ReLU(True))
        self.body.add_module("conv2", nn.Conv2d(f, f, 3, padding=1))


class SRNet(nn.Module):
    def __init__(self, in_channels, out_channels, upscale_factor, num_resblocks=10):
        super().__init__()
        self.head = nn.Sequential()
        self.head.add_module("conv", nn.Conv2d(in_channels * (upscale_factor ** 2 + 1), 64, 3, padding=1))
        self.head.add_module("relu", nn.ReLU(True))
        self.body = nn.Sequential(*[_ResBlock(64) for _ in range(num_resblocks)])
        self.tail = nn.Sequential()
        self.tail.add_module("deconv1", nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1))
        self.tail.add_module("relu1", nn.ReLU(True))
        self.tail.add_module("deconv2", nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1))
        self.tail.add_module("relu2", nn.ReLU(True))
        self.tail.add_module("conv", nn.Conv2d(64, out_channels, 3, padding=1))


class FNet(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.body = nn.Sequential()
        cin, f = in_channels * 2, 32
        for i in range(6):
            self.body.add_module(f"conv{i + 1}_1", nn.Conv2d(cin, f, 3, padding=1))
            self.body.add_module(f"leaky_relu{i + 1}_1", nn.LeakyReLU(0.2, inplace=True))
            self.body.add_module(f"conv{i + 1}_2", nn.Conv2d(f, f, 3, padding=1))
            self.body.add_module(f"leaky_relu{i + 1}_2", nn.LeakyReLU(0.2, inplace=True))
            if i < 3:
                self.body.add_module(f"pooling_{i}", nn.MaxPool2d(2))
            else:
                self.body.add_module(f"upsample_{i - 3}", nn.Upsample(scale_factor=2, mode="bilinear",
                                                                      align_corners=False))
            cin = f
            f = f * 2 if i < 3 else f // 2
        self.tail = nn.Sequential()
        self.tail.add_module("conv1", nn.Conv2d(cin, 32, 3, padding=1))
        self.tail.add_module("leaky_relu", nn.LeakyReLU(0.2, inplace=True))
        self.tail.add_module("conv2", nn.Conv2d(32, out_channels, 3, padding=1))
        self.tail.add_module("tanh", nn.Tanh())

    def ops(self):
        """[(kind, module)]: 'leaky' convs, 'pool', 'up', then the plain last conv."""
        out = []
        for m in self.body:
            if isinstance(m, nn.Conv2d):
                out.append(("leaky", m))
            elif isinstance(m, nn.MaxPool2d):
                out.append(("pool", m))
            elif isinstance(m, nn.Upsample):
                out.append(("up", m))
        return out + [("leaky", self.tail.conv1), ("plain", self.tail.conv2)]


class FRVSRNet(BaseNet):
    """list of T frames (N, C, h, w) -> (T estimates (N, C, 4h, 4w), T warped
    previous frames (N, C, h, w)); the estimates alone when is_prediction."""

    def __init__(self, in_channels, out_channels, upscale_factor, is_prediction=False, num_resblocks=10):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.upscale_factor = upscale_factor
        self.is_prediction = is_prediction
        self.srnet = SRNet(in_channels, out_channels, upscale_factor, num_resblocks)
        self.fnet = FNet(in_channels, 2)
        for m in self.modules():
            if m.__class__.__name__.find("Conv") != -1:
                nn.init.xavier_uniform_(m.weight)

    # ------------------------------------------------------------------
    def forward(self, inputs):
        if self.upscale_factor != 4:
            raise ValueError(f"FRVSRNet's tail is two stride-2 deconvs, a fixed x4: upscale_factor "
                             f"{self.upscale_factor} is not supported")
        if self.in_channels != self.out_channels:
            raise ValueError("FRVSRNet warps its own estimate into its input: in_channels must equal out_channels")
        flat = super().forward(list(inputs))
        t = len(inputs)
        sr, lr = list(flat[:t]), list(flat[t:])
        return sr if self.is_prediction else (sr, lr)

    def _returns_list(self) -> bool:
        return True

    def _head_perm(self, dev):
        """Input-channel index of the reference's head weight for each channel of
        the head's input as the warp stores it; None when they agree (C = 1)."""
        c, rr = self.in_channels, self.upscale_factor ** 2
        if c == 1:
            return None
        idx = [cc * rr + s for s in range(rr) for cc in range(c)] + [rr * c + cc for cc in range(c)]
        return torch.tensor(idx, dtype=torch.long, device=dev)

    def _sr_convs(self):
        sr = self.srnet
        return [c for blk in sr.body for c in (blk.body.conv1, blk.body.conv2)] + [sr.tail.conv]

    # ------------------------------------------------------------------
    def _run(self, inputs, tape: dict | None):
        cd, r, c = self.compute_dtype, self.upscale_factor, self.in_channels
        T = len(inputs)
        n, _, h, w = inputs[0].shape
        dev = inputs[0].device
        H, W, NT, rr = h * r, w * r, n * T, r * r
        slope = self._const(dev, 0.2)
        sr, fn = self.srnet, self.fnet

        def new(b, hh, ww, ch, dtype=cd, zero=False):
            return empty_view((b, 1, hh, ww), ch, dtype, dev, zero)

        X = torch.stack([x.float() for x in inputs])                       # (T, n, c, h, w)
        prev = torch.cat([X[:1], X[:-1]])
        pair = torch.cat([prev, X], dim=2)                                 # (T, n, 2c, h, w)
        ph, pw = -h % 8, -w % 8
        top, left, hp, wp = ph // 2, pw // 2, h + ph, w + pw
        if ph or pw:  # F.pad(x, value=x.min()) per frame pair, the minimum staying on the device
            padded = pair.amin(dim=(1, 2, 3, 4)).view(T, 1, 1, 1, 1).expand(T, n, 2 * c, hp, wp).clone()
            padded[..., top:top + h, left:left + w] = pair
            pair = padded
        # ---- FNet over all frame pairs
        fops = fn.ops()
        pk = self._pack_weights([(m.weight, 0, 1) for k, m in fops if k in ("leaky", "plain")]
                                + [(m.weight, 0, 1) for m in self._sr_convs()])

        def P(conv):
            return pk[(id(conv.weight), 0, 1)]

        cur = F.to_view(pair.reshape(NT, 2 * c, hp, wp), cd, cpad=cp(2 * c))[..., :2 * c]
        ftape = []
        for kind, m in fops:
            b_, _, hh, ww, ch = cur.shape
            if kind == "leaky":
                y = F.conv(cur, P(m), new(b_, hh, ww, m.out_channels), K3, P1, bias=m.bias, act=F.ACT_PRELU,
                           act_param=slope)
            elif kind == "plain":  # the flow head: an fp32 view
                y = F.conv(cur, P(m), new(b_, hh, ww, m.out_channels, torch.float32, zero=True), K3, P1, bias=m.bias)
            elif kind == "pool":
                y = F.max_pool2x2(cur, new(b_, hh // 2, ww // 2, ch))
            else:
                y = F.upsample_cl(cur, new(b_, hh * 2, ww * 2, ch), 2, False)
            ftape.append((kind, m, cur, y))
            cur = y
        flow_cl = F.tanh(cur, cur)                                          # (NT, 1, hp, wp, 2) fp32, in place
        flow = flow_cl[:, 0, top:top + h, left:left + w].permute(0, 3, 1, 2).contiguous()   # (NT, 2, h, w)
        # ---- the T low-resolution warps, one launch (fp32 images)
        prev_v = F.to_view(prev.reshape(NT, c, h, w), torch.float32, cpad=cp(c))[..., :c]
        lrw = F.flow_warp(prev_v, flow, new(NT, h, w, c, torch.float32), "border", False)
        lr_out = list(F.from_view(lrw).view(T, n, c, h, w).unbind(0))
        # ---- SR net, frame by frame
        Xv = F.to_view(X.reshape(NT, c, h, w), cd, cpad=cp(c))[..., :c]
        perm = self._head_perm(dev)
        hw_ = sr.head.conv.weight if perm is None else sr.head.conv.weight.detach()[:, perm].contiguous()
        head_p = F.pack_weight(hw_, 0, cd)
        sp = subpixel_cache(cd)
        dec = [sp(d, _DECONV, True) for d in (sr.tail.deconv1, sr.tail.deconv2)]
        cin = c * (rr + 1)
        est = new(n, H, W, c, zero=True)                                    # the first estimate: zeros
        sr_out, stape = [], []
        for t in range(T):
            fl = flow[t * n:(t + 1) * n]
            hin = new(n, h, w, cin, zero=True)
            F.flow_warp(est, fl, hin[..., :rr * c], "border", False, s2d=r, flow_up=r)
            hin[..., rr * c:].copy_(Xv[t * n:(t + 1) * n])
            h0 = F.conv(hin, head_p, new(n, h, w, 64), K3, P1, bias=sr.head.conv.bias, act=F.ACT_RELU)
            x_, saved = h0, []
            for blk in sr.body:
                c1, c2 = blk.body.conv1, blk.body.conv2
                a = F.conv(x_, P(c1), new(n, h, w, 64), K3, P1, bias=c1.bias, act=F.ACT_RELU)
                nxt = F.conv(a, P(c2), new(n, h, w, 64), K3, P1, bias=c2.bias, residual=x_)
                saved.append((x_, a))
                x_ = nxt
            u1 = F.conv(x_, dec[0][0], new(n, 2 * h, 2 * w, 64), K3, P1, bias=dec[0][1], bias_r=1, y_shuffle=2,
                        act=F.ACT_RELU)
            u2 = F.conv(u1, dec[1][0], new(n, H, W, 64), K3, P1, bias=dec[1][1], bias_r=1, y_shuffle=2,
                        act=F.ACT_RELU)
            tc = sr.tail.conv
            yv = F.conv(u2, P(tc), new(n, H, W, c, torch.float32), K3, P1, bias=tc.bias)
            y = F.from_view(yv)                                             # (n, c, H, W) fp32
            sr_out.append(y)
            if tape is not None:
                stape.append(dict(est=est, hin=hin, h0=h0, saved=saved, body=x_, u1=u1, u2=u2))
            est = F.to_view(y, cd, cpad=cp(c))[..., :c]
        if tape is not None:
            tape.update(ftape=ftape, flow_cl=flow_cl, flow=flow, prev_v=prev_v, stape=stape, sp=sp, perm=perm,
                        geom=(T, n, h, w, top, left, hp, wp))
        return sr_out + lr_out

    # ------------------------------------------------------------------
    def _backward(self, tape: dict, grads) -> dict:
        cd, r, c = self.compute_dtype, self.upscale_factor, self.in_channels
        T, n, h, w, top, left, hp, wp = tape["geom"]
        H, W, NT, rr = h * r, w * r, n * T, r * r
        grads = list(grads) if isinstance(grads, (tuple, list)) else [grads]
        gsr, glr = grads[:T], grads[T:]
        flow = tape["flow"]
        dev = flow.device
        slope = self._const(dev, 0.2)
        sr, fn = self.srnet, self.fnet
        pg = ParamGrads(self)

        def new(b, hh, ww, ch, dtype=cd, zero=False):
            return empty_view((b, 1, hh, ww), ch, dtype, dev, zero)

        pk = self._pack_weights([(m.weight, 1, 1) for k, m in fn.ops() if k in ("leaky", "plain")][1:]
                                + [(m.weight, 1, 1) for m in self._sr_convs()])

        def D(conv):
            return pk[(id(conv.weight), 1, 1)]

        def relu_bwd(y, g):
            return F.relu_bwd(y, g, torch.empty_like(g))

        # ---- SR net, frame by frame (independent: the estimate and the frames carry no gradient)
        s_ = _DECONV[1]
        dec_d = [tape["sp"](d, _DECONV, True, 1)[0] for d in (sr.tail.deconv1, sr.tail.deconv2)]
        perm = tape["perm"]
        hconv = sr.head.conv
        hw_ = hconv.weight if perm is None else hconv.weight.detach()[:, perm].contiguous()
        head_d = F.pack_weight(hw_, 1, cd)
        cin = c * (rr + 1)
        gflow = torch.zeros((NT, 2, h, w), dtype=torch.float32, device=dev)
        ghr = torch.empty((n, 2, H, W), dtype=torch.float32, device=dev)
        for t in range(T):
            if gsr[t] is None:
                continue
            rec = tape["stape"][t]
            g = F.to_view(gsr[t].float(), cd, cpad=cp(c))[..., :c]
            tc = sr.tail.conv
            pg.conv_wgrad(tc, rec["u2"], g, K3, P1)
            g = relu_bwd(rec["u2"], F.conv(g, D(tc), new(n, H, W, 64), K3, P1))
            for d, x_in, dd in ((sr.tail.deconv2, rec["u1"], dec_d[1]), (sr.tail.deconv1, rec["body"], dec_d[0])):
                pg.subpixel_wgrad(d, x_in, g, _DECONV, True, tap_skip=False)
                hh, ww = x_in.shape[2], x_in.shape[3]
                g = F.conv(g, dd, new(n, hh, ww, 64), K3, P1, x_shuffle=s_)
                if d is sr.tail.deconv2:
                    g = relu_bwd(x_in, g)
            for blk, (x_in, a) in reversed(list(zip(sr.body, rec["saved"]))):
                c1, c2 = blk.body.conv1, blk.body.conv2
                pg.conv_wgrad(c2, a, g, K3, P1)
                ga = relu_bwd(a, F.conv(g, D(c2), new(n, h, w, 64), K3, P1))
                pg.conv_wgrad(c1, x_in, ga, K3, P1)
                g = F.conv(ga, D(c1), new(n, h, w, 64), K3, P1, residual=g)
            g = relu_bwd(rec["h0"], g)
            if perm is None:
                pg.conv_wgrad(hconv, rec["hin"], g, K3, P1)
            else:  # in the warp's channel order, permuted back onto the reference's
                # (one accumulate flag serves weight and bias: the scratch starts at zero)
                tmp = torch.zeros_like(hconv.weight, dtype=torch.float32)
                db, accb = pg.buf(hconv.bias)
                F.conv_wgrad(rec["hin"], g, K3, P1, tmp.view(*tmp.shape[:2], 1, *tmp.shape[2:]), db, accumulate=accb)
                dw, acc = pg.buf(hconv.weight)
                if acc:
                    dw.index_add_(1, perm, tmp)
                else:
                    dw.zero_().index_add_(1, perm, tmp)
            if t > 0:  # the first estimate is zeros: no flow gradient through it
                ghin = F.conv(g, head_d, new(n, h, w, cin), K3, P1)
                F.flow_warp_bwd(rec["est"], flow[t * n:(t + 1) * n], ghin[..., :rr * c], ghr, "border", False, s2d=r,
                                flow_up=r)
                F.upsample2d_bwd(ghr, gflow[t * n:(t + 1) * n], "bilinear", True, r)
        # ---- the low-resolution warps, one launch, onto the same flow gradient
        if any(g_ is not None for g_ in glr):
            gl = torch.stack([g_.float() if g_ is not None else torch.zeros((n, c, h, w), device=dev) for g_ in glr])
            glv = F.to_view(gl.reshape(NT, c, h, w), torch.float32, cpad=cp(c))[..., :c]
            F.flow_warp_bwd(tape["prev_v"], flow, glv, gflow, "border", False, accumulate=True)
        # ---- tanh and FNet over all frame pairs
        flow_cl = tape["flow_cl"]
        g32 = new(NT, hp, wp, 2, torch.float32, zero=True)
        g32[:, 0, top:top + h, left:left + w].copy_(gflow.permute(0, 2, 3, 1))
        F.tanh_bwd(flow_cl, g32, g32)
        g = new(NT, hp, wp, 2, zero=True)
        g.copy_(g32)
        dummy = torch.empty(1, dtype=torch.float32, device=dev)
        ftape = tape["ftape"]
        for i in range(len(ftape) - 1, -1, -1):
            kind, m, x_in, y = ftape[i]
            if kind == "pool":
                g = F.max_pool2x2_bwd(x_in, g, torch.empty_like(x_in))
            elif kind == "up":
                g = F.upsample_cl_bwd(g, torch.empty_like(x_in), 2, False)
            else:
                if kind == "leaky":
                    g = F.prelu_bwd(y, g, slope, torch.empty_like(g), dummy, False)
                pg.conv_wgrad(m, x_in, g, K3, P1)
                if i > 0:  # the frames need no gradient
                    b_, _, hh, ww, ch = x_in.shape
                    g = F.conv(g, D(m), new(b_, hh, ww, ch), K3, P1)
        return pg.done()
