"""What the hand-written backward passes of the nets share: the conv geometry
constants, channels-last view allocation, the parameter-gradient ledger, the
per-step sub-pixel weight cache and the reverse pass of an op-level tape.

An op-level tape: a net's forward calls push(bwd) after every op, where
bwd(bk) takes the gradient of the op's output from bk (a Bwd), launches the
op's weight and data gradients and hands the input's gradient back with
bk.acc / bk.route.  Bwd.run seeds the output's gradient, runs the reverses
last to first and returns the finished parameter gradients.  Two things are
part of a net's results and are decided here, once:

  * The order in which the gradient contributions of a tensor with several
    consumers are summed: F.add rounds at 16 bits.  Bwd keeps them apart, in
    arrival order, until the tensor's producer takes them, and folds from the
    tail: take_list(t, 2) of arrivals a, b, c is [a, b + c], take(t) is
    a + (b + c).  A subclass that overrides acc may sum on arrival instead
    (EDVRNet: (a + b) + c, one tensor held at a time).
  * The order in which parameters are first touched: ParamGrads.done hands
    them to BaseNet._grad_done in that order (data-parallel: the order in
    which a bucket's all-reduce can start), and a parameter touched again
    accumulates onto what the earlier launch wrote (shared weights: a fixed
    order, the order of the calls).
"""
from __future__ import annotations

import torch

from .. import functional as F

K3, P1 = (1, 3, 3), (0, 1, 1)
K1, P0 = (1, 1, 1), (0, 0, 0)
# kernel, stride, padding of the x2 / x3 / x4 / x8 projections (reference drf_net.py:70-77)
PROJ = {2: (6, 2, 2), 3: (7, 3, 2), 4: (8, 4, 2), 8: (12, 8, 2)}


def cp(c: int) -> int:
    """Channels of the storage a c-channel view lives in (whole 16-byte chunks)."""
    return -(-c // 8) * 8


def empty_view(lead4, ch: int, dtype, device, zero: bool = False) -> torch.Tensor:
    """A new channels-last view (*lead4, ch) in cp(ch)-channel storage."""
    mk = torch.zeros if zero else torch.empty
    return mk((*lead4, cp(ch)), dtype=dtype, device=device)[..., :ch]


def recorder(on: bool):
    """(ops, push) of a forward: push(bwd) appends to ops; both idle when not on."""
    ops: list | None = [] if on else None

    def push(fn):
        if ops is not None:
            ops.append(fn)

    return ops, push


def subpixel_cache(cd):
    """sp(conv, (k, s, p), transposed, mode) -> (the packed 3x3 sub-pixel image
    of conv's weight, its bias): the image once per weight and step, packed
    once per mode (0 forward, 1 data gradient) in compute dtype cd."""
    cache: dict = {}

    def sp(conv, proj, transposed, mode=0):
        key = id(conv.weight)
        if key not in cache:
            cache[key] = F.subpixel_conv_weight(conv.weight, conv.bias, *proj, transposed)
        weq, beq = cache[key]
        if (key, mode) not in cache:
            cache[(key, mode)] = F.pack_weight(weq, mode, cd)
        return cache[(key, mode)], beq

    return sp


class ParamGrads:
    """The parameter gradients of one backward pass of net, in first-touch order."""

    def __init__(self, net):
        self.net = net
        self._bufs: dict = {}  # id(p) -> (p, buffer), in first-touch order

    def buf(self, p):
        """(fp32 gradient buffer of p, whether an earlier launch already wrote it)."""
        ent = self._bufs.get(id(p))
        if ent is None:
            ent = self._bufs[id(p)] = (p, self.net._grad_buffer(p))
            return ent[1], False
        return ent[1], True

    def conv_wgrad(self, m, x, g, k, pad, **kw):
        """Weight and bias gradient of the conv m with input x and output gradient g."""
        dw, seen = self.buf(m.weight)
        db, _ = self.buf(m.bias)
        F.conv_wgrad(x, g, k, pad, dw.view(*dw.shape[:2], 1, *dw.shape[2:]), db, accumulate=seen, **kw)

    def subpixel_wgrad(self, m, x, g, proj, transposed, tap_skip):
        """Likewise for a Conv2d / ConvTranspose2d(k, s, p) run as a 3x3 sub-pixel
        conv: the 3x3 image's gradient through the shuffle-s view, folded onto
        m's own layout.  tap_skip: compute only the taps the image carries."""
        k, s, p = proj
        cop, cip = (s * s * m.out_channels, m.in_channels) if transposed else (m.out_channels, s * s * m.in_channels)
        dw, seen = self.buf(m.weight)
        db, _ = self.buf(m.bias)
        dweq = torch.empty((cop, cip, 1, 3, 3), dtype=torch.float32, device=x.device)
        dbeq = torch.empty(cop, dtype=torch.float32, device=x.device)
        kw = {"dy_shuffle" if transposed else "x_shuffle": s}
        if tap_skip:
            kw["subpixel"] = F.subpixel_code(k, s, p, transposed, False)
        F.conv_wgrad(x, g, K3, P1, dweq, dbeq, **kw)
        F.subpixel_wgrad_fold(dweq, dbeq, dw, db, k, s, p, transposed, accumulate=seen)

    def done(self) -> dict:
        """Hand every touched parameter to the net -> {id(p): gradient}."""
        out: dict = {}
        for p, g in self._bufs.values():
            self.net._grad_done(out, p, g)
        return out


class Bwd(ParamGrads):
    """The reverse pass of an op tape: G holds, per tensor, the gradient
    contributions that have arrived, apart and in arrival order."""

    def __init__(self, net):
        super().__init__(net)
        self.G: dict = {}

    def new_like(self, t, dtype=None, zero=False):
        return empty_view(t.shape[:4], t.shape[4], dtype or t.dtype, t.device, zero)

    def acc(self, t, g):
        self.G.setdefault(id(t), []).append(g)

    def take_list(self, t, n):
        """The contributions to t's gradient, summed from the tail down to at most n tensors."""
        lst = self.G.pop(id(t))
        while len(lst) > n:
            b, a = lst.pop(), lst.pop()
            lst.append(F.add(a, b, self.new_like(a)))
        return lst

    def take(self, t):
        return self.take_list(t, 1)[0]

    def route(self, x, parts, gx):
        """gx is x's gradient; parts: the channel slices [(tensor, lo, hi)] of x
        that are tensors of their own (x is then a concat buffer and gets nothing)."""
        if parts is None:
            self.acc(x, gx)
        else:
            for t, lo, hi in parts:
                self.acc(t, gx[..., lo:hi])

    def run(self, ops, yv, g) -> dict:
        """g is the gradient of the forward's last view yv -> {id(p): gradient}."""
        self.acc(yv, g)
        for op in reversed(ops):
            op(self)
        return self.done()
