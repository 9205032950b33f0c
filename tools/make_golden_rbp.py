"""TEST INFRASTRUCTURE ONLY -- golden fixtures of RBPNet, made from the
reference itself.  Needs the reference tree (build container only):

    python tools/make_golden_rbp.py

Per case it builds the reference's RBPNet (rbp_net.py, registered with
oracle.ref_loader from here) and the restatement tests/rbp_ref.RBPRef from one
seed, asserts identical initial weights, output, L1 loss and every gradient
bit for bit in fp32, and writes tests/golden/<case>.pt with the keys of
oracle.make_golden.run_case that tests/test_rbp_gpu.py reads.

rbp_x3_slopes sets the PReLU slopes, in module order, to the cycle 0.25, -0.1,
0.0, 1.5 (rbp_ref.perturb_slopes) in the reference and the restatement alike,
and stores them: block-tail and projection PReLUs with a slope <= 0 take the
pre-activation backward.

The 16-bit envelopes (bf16_env, fp16_env) are make_golden._bf16_envelope's
model of an ideal 16-bit-storage implementation -- fp64 math with 16-bit conv
weights and every conv output, its input gradient and the network input
rounded (dithered) -- with the one change this net's structure forces: the
back-projection sums and differences (rbp_ref.Stored: l0 - x, h1 + h0, h0 - x,
l1 + l0, h0 - h1, h0 + e) are conv INPUTS, so any implementation with 16-bit
activations stores them; they and the gradients arriving at them are rounded
like a conv's output.  make_golden's model has no such tensor: in the nets it
was written for every conv reads a conv's (or BatchNorm's) output.

A fixture whose fp64 gradient is zero for some parameter would have that
parameter skipped, and one whose reference fp32 error is large (a scalar that
nearly cancels) would pass at a vacuous tolerance.  So a case is refused when
any parameter's fp64 gradient norm is zero or its ref32_err exceeds
REF32_MAX; the seeds are walked in order from make_golden.SEED until a case
qualifies, and the seed is stored.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as Fn

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import cpu_nets, make_golden as mg, ref_loader  # noqa: E402
from tests.rbp_ref import RBPRef, Stored, perturb_slopes  # noqa: E402

_MOD = "src.model.nets.rbp_net"


def _kw(**over):
    return dict(dict(in_channels=1, out_channels=1, base_filter=32, feat=16, num_stages=3, num_resblocks=1,
                     num_frames=3, upscale_factor=4), **over)


CASES = {
    # name: (kwargs, (B, N, C, h, w), perturbed slopes)
    "rbp_x4_small": (_kw(), (2, 3, 1, 8, 12), False),
    "rbp_x2_roll": (_kw(base_filter=64, feat=64, num_resblocks=2, num_frames=4, upscale_factor=2),
                    (1, 4, 1, 10, 18), False),
    "rbp_x3_slopes": (_kw(in_channels=2, out_channels=2, upscale_factor=3), (1, 3, 2, 6, 10), True),
}
FULL_GRAD_MAX = 3000  # elements up to which a gradient is stored in full; the rest by 16 projections
MAX_BYTES = 1 << 20
REF32_MAX = 1e-3
ENV_DRAWS = 16
TRIES = 50


def _data(shape, seed, r):
    return mg._inputs("misr", shape, r, torch.Generator().manual_seed(seed + 1))


def _factory(perturbed):
    def make(**kwargs):
        net = RBPRef(**kwargs)
        if perturbed:
            perturb_slopes(net)
        return net
    return make


def _net(kwargs, seed, perturbed, dtype=torch.float32):
    torch.manual_seed(seed)
    net = _factory(perturbed)(**kwargs).train()
    return net.double() if dtype == torch.float64 else net


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _measure(kwargs, shape, seed, perturbed):
    """The fp64 run and the reference's own fp32 error against it (worst over
    thread counts and make_golden's noise envelope), or None when the case
    does not qualify."""
    r = kwargs["upscale_factor"]
    lr, hr = _data(shape, seed, r)
    lr64, hr64 = [x.double() for x in lr], hr.double()
    m64 = _net(kwargs, seed, perturbed, torch.float64)
    out64 = m64(lr64)
    Fn.l1_loss(out64, hr64).backward()
    g64 = _grads(m64)
    zero = [k for k, v in g64.items() if v.norm().item() == 0.0]
    if zero:
        print(f"    seed {seed}: zero fp64 gradient for {zero}", flush=True)
        return None
    out_err32 = 0.0
    ref32_err = {k: 0.0 for k in g64}
    nthreads = torch.get_num_threads()
    for nt in (1, 2, 4, nthreads):
        torch.set_num_threads(nt)
        m32 = _net(kwargs, seed, perturbed)
        o32 = m32(lr)
        Fn.l1_loss(o32, hr).backward()
        out_err32 = max(out_err32, (o32.double() - out64.detach()).abs().max().item())
        for k, p in m32.named_parameters():
            ref32_err[k] = max(ref32_err[k], (p.grad.double() - g64[k]).norm().item() / g64[k].norm().item())
    torch.set_num_threads(nthreads)
    noise_err = {k: 0.0 for k in g64}
    gn = torch.Generator().manual_seed(seed + 7)

    def jitter(t):
        return t + mg.NOISE_EPS_COND * t.detach().pow(2).mean().sqrt() * torch.randn(t.shape, generator=gn,
                                                                                      dtype=t.dtype)

    def hook(mod, inp, o):
        o = jitter(o)
        if o.requires_grad:
            o.register_hook(jitter)
        return o

    for _ in range(mg.NOISE_DRAWS):
        mn = _net(kwargs, seed, perturbed, torch.float64)
        for mod in mn.modules():
            if isinstance(mod, nn.modules.conv._ConvNd):
                mod.register_forward_hook(hook)
        Fn.l1_loss(mn(lr64), hr64).backward()
        for k, p in mn.named_parameters():
            noise_err[k] = max(noise_err[k], (p.grad - g64[k]).norm().item() / g64[k].norm().item())
    ref32_err = {k: max(v, noise_err[k]) for k, v in ref32_err.items()}
    worst = max(ref32_err, key=ref32_err.get)
    if ref32_err[worst] > REF32_MAX:
        print(f"    seed {seed}: ref32_err {ref32_err[worst]:.2e} for {worst} > {REF32_MAX}", flush=True)
        return None
    return lr, hr, lr64, hr64, out64.detach(), g64, out_err32, ref32_err, noise_err


def _envelope(make, kwargs, lr64, hr64, g64, seed, dtype, draws=ENV_DRAWS):
    """make_golden._bf16_envelope with the Stored sums and differences rounded
    too (see the module docstring)."""
    dither = 2.0 ** -12 if dtype == torch.bfloat16 else 2.0 ** -15
    gscale = float(2 ** (hr64.numel().bit_length() - 1)) if dtype == torch.float16 else 1.0
    env = {k: 0.0 for k in g64}
    for draw in range(draws):
        g = torch.Generator().manual_seed(seed + 100 + draw)

        def q(t):
            return (t + t.abs() * dither * torch.randn(t.shape, generator=g, dtype=t.dtype)).to(dtype).to(t.dtype)

        def qg(t):
            return q(t * gscale) / gscale

        def hook(mod, inp, out):
            out = out + (q(out.detach()) - out.detach())  # straight-through rounding
            if out.requires_grad:
                out.register_hook(qg)
            return out

        torch.manual_seed(seed)
        m = make(**kwargs).double().train()
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.modules.conv._ConvNd):
                    mod.weight.copy_(mod.weight.to(dtype).double())
        for mod in m.modules():
            if isinstance(mod, (nn.modules.conv._ConvNd, Stored)):
                mod.register_forward_hook(hook)
        Fn.l1_loss(m([q(t) for t in lr64]), hr64).backward()
        for k, p in m.named_parameters():
            env[k] = max(env[k], (p.grad - g64[k]).norm().item() / g64[k].norm().item())
    return env


def run_case(name, kwargs, shape, perturbed):
    for seed in range(mg.SEED, mg.SEED + TRIES):
        got = _measure(kwargs, shape, seed, perturbed)
        if got is not None:
            break
    else:
        raise SystemExit(f"{name}: no seed in [{mg.SEED}, {mg.SEED + TRIES}) qualifies")
    lr, hr, lr64, hr64, out64, g64, out_err32, ref32_err, noise_err = got
    ref_cls = ref_loader.load(_MOD).RBPNet
    torch.manual_seed(seed)
    ref = ref_cls(**kwargs).train()
    mine = _net(kwargs, seed, False)
    rsd, msd = ref.state_dict(), mine.state_dict()
    assert list(rsd) == list(msd), f"{name}: state_dict keys differ"
    for k in rsd:
        assert torch.equal(rsd[k], msd[k]), f"{name}: init of {k} differs"
    slopes = None
    if perturbed:
        slopes = perturb_slopes(ref)
        assert perturb_slopes(mine) == slopes
    init_sum = {k: float(v.double().sum()) for k, v in mine.state_dict().items()}
    outs, grads, losses = [], [], []
    for net in (ref, mine):
        net.zero_grad(set_to_none=True)
        out = net(list(lr))  # (the reference pops the centre frame out of the list it is given)
        ls = Fn.l1_loss(out, hr)
        ls.backward()
        outs.append(out.detach())
        losses.append(ls.detach())
        grads.append(_grads(net))
    assert torch.equal(outs[0], outs[1]), f"{name}: outputs differ"
    assert torch.equal(losses[0], losses[1])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), f"{name}: grad {k} differs"
    out = outs[1]
    gmax = max(v.norm().item() for v in g64.values())
    make = _factory(perturbed)
    bf16_env = _envelope(make, kwargs, lr64, hr64, g64, seed, torch.bfloat16)
    fp16_env = _envelope(make, kwargs, lr64, hr64, g64, seed, torch.float16)
    ma = _net(kwargs, seed, perturbed)
    Fn.l1_loss(ma(lr), hr).backward()
    opt = torch.optim.Adam(ma.parameters(), **mg.ADAM)
    p0 = {k: p.detach().clone() for k, p in ma.named_parameters()}
    opt.step()
    adam_update = {k: (p.detach() - p0[k]) for k, p in ma.named_parameters()}
    mine.eval()
    with torch.no_grad():
        out_eval = mine(lr)
    psnr = cpu_nets.psnr(cpu_nets.denormalize(out, "acdc"), cpu_nets.denormalize(hr, "acdc"))
    worst = max(ref32_err.values())
    fx = {
        "name": name, "class": "RBPNet", "kwargs": kwargs, "seed": seed, "kind": "misr", "perturbed": perturbed,
        "slopes": slopes, "param_sum": init_sum, "lr": lr, "hr": hr, "output": out, "output64": out64,
        "loss": float(losses[1]), "psnr_acdc": float(psnr), "out_err32": out_err32,
        "grad_norm64": {k: v.norm().item() for k, v in g64.items()},
        "grad_full64": {k: v for k, v in g64.items() if v.numel() <= FULL_GRAD_MAX},
        "grad_proj64": {k: mg.proj(v, k, mg.PROJ) for k, v in g64.items()}, "proj_n": mg.PROJ,
        "grad_max64": gmax,
        "ref32_err": ref32_err, "noise_err": noise_err, "bf16_env": bf16_env, "fp16_env": fp16_env,
        "adam": {**mg.ADAM, "betas": list(mg.ADAM["betas"])},
        "adam_update_full": {k: v for k, v in adam_update.items() if v.numel() <= FULL_GRAD_MAX},
        "adam_update_proj": {k: mg.proj(v.double(), k, mg.PROJ) for k, v in adam_update.items()},
        "adam_update_norm": {k: v.double().norm().item() for k, v in adam_update.items()},
        "output_eval": out_eval, "cond_worst": worst,
    }
    mg.OUT.mkdir(parents=True, exist_ok=True)
    path = mg.OUT / f"{name}.pt"
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: fixture {size} bytes > {MAX_BYTES}; lower FULL_GRAD_MAX"
    print(f"{name}: seed {seed}, restatement == reference (bitwise), loss={fx['loss']:.6f} "
          f"psnr={fx['psnr_acdc']:.4f}; fp32-vs-fp64: out {out_err32:.1e}, worst grad {worst:.1e}; bf16_env max "
          f"{max(bf16_env.values()):.2e}, fp16_env max {max(fp16_env.values()):.2e}; fixture {size / 1024:.0f} KiB",
          flush=True)


def main():
    if not ref_loader.available():
        raise SystemExit("reference not available (build container only)")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_loader._FILES[_MOD] = "src/model/nets/rbp_net.py"
    only = os.environ.get("GOLDEN_ONLY")
    for name, (kwargs, shape, perturbed) in CASES.items():
        if not only or name in only.split(","):
            run_case(name, kwargs, shape, perturbed)


if __name__ == "__main__":
    main()
