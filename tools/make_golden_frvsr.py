"""TEST INFRASTRUCTURE ONLY -- golden fixtures of FRVSRNet, made from the
reference itself.  Needs the reference tree (build container only):

    python tools/make_golden_frvsr.py

Per case it builds the reference's FRVSRNet (imported by path through
oracle.ref_loader) and the restatement tests/frvsr_ref.FRVSRRef from one
seed, asserts identical initial weights, both output lists and every
gradient bit for bit in fp32, and writes tests/golden/<case>.pt with the keys
of oracle.make_golden.run_case (which cannot take the net's tuple output, so
this script writes the fixture itself).  Loss: mean_t L1(lr'_t, lr_t) +
mean_t L1(sr_t, hr_t), the FRVSR trainers' two L1 terms.

The seed (net init; inputs from seed + 1) is searched as make_golden.find_seed
does.  The margins are RESTATED from the first plan (make_golden.MARGIN = 1e-5
rms for activations and pools, 100 x the fp32-fp64 coordinate difference for
the warps): at 2 x 3 frames of 8x16 those cannot be met -- about 1.3 M
activation inputs put ten inside 1e-5 rms on every seed, and the HR warp's
26 112 coordinates put 2-14 inside 1e-4 px against a 3-6e-4 px margin.  Each
margin is now per element: MULT = 3 times that element's own difference
between the restatement's fp32 and fp64 runs, measured per seed, so that in
the fp64 run
  * every ReLU / LeakyReLU input is at least MULT x its own fp32-fp64
    difference from zero (both in units of its tensor's rms),
  * every 2x2 pool window's two largest values are at least MULT x the
    fp32-fp64 difference of their gap apart (same units) -- or tie EXACTLY in
    both runs: the pad-and-crop case pads with a constant, so neighbouring
    pixels inside the pad see identical 3x3 inputs and give identical values
    in any precision (about a hundred windows in frvsr_x4_pad, n_pool_ties);
    there the first-maximum rule decides, in torch and in the pool kernel,
  * every sampling coordinate of either warp, in pixels, is at least MULT x its
    own fp32-fp64 difference from every integer in [0, size - 1]:
the restatement's own fp32 rounding then flips no activation mask, arg-max or
bilinear cell, with a factor 3 to spare.  An implementation that rounds
differently may still flip one; the fixture's ref32_err carries make_golden's
noise envelope for that, and every margin and measured difference is stored
in the fixture (*_ratio: the smallest distance / difference; *_err32: the\nlargest difference; *_min: the smallest distance).
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import cpu_nets, make_golden as mg, ref_loader  # noqa: E402
from tests import frvsr_ref  # noqa: E402
from tests.frvsr_ref import FRVSRRef  # noqa: E402

_MOD = "src.model.nets.frvsr_net"
CASES = {
    # name: (kwargs, (N, T, C, H, W))
    "frvsr_x4_small": (dict(in_channels=1, out_channels=1, upscale_factor=4, num_resblocks=2), (2, 3, 1, 8, 16)),
    "frvsr_x4_pad": (dict(in_channels=1, out_channels=1, upscale_factor=4, num_resblocks=1), (1, 2, 1, 6, 10)),
}
# elements up to which a gradient is stored in full; the rest is pinned by 16 projections
FULL_GRAD_MAX = {"frvsr_x4_small": 5000, "frvsr_x4_pad": 5000}
MAX_BYTES = 1 << 20
MULT = 3.0
TRIES = 4000


def _data(shape, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return mg._inputs("vsr", shape, 4, g)


def _net(kwargs, seed, dtype=torch.float32):
    torch.manual_seed(seed)
    net = FRVSRRef(**kwargs).train()
    return net.double() if dtype == torch.float64 else net


def _probe(kwargs, shape, seed, dtype):
    """One forward of the restatement: every ReLU / LeakyReLU input and every
    pool window's top-two gap, each over its tensor's rms, and the warps'
    pixel coordinates with their axis sizes, as flat fp64 tensors."""
    lr, _ = _data(shape, seed)
    net = _net(kwargs, seed, dtype)
    act, pool, coords, sizes = [], [], [], []

    def act_hook(mod, inp, out):
        x = inp[0].detach().double()
        act.append((x / x.pow(2).mean().sqrt()).flatten())

    def pool_hook(mod, inp, out):
        x = inp[0].detach().double()
        win = nn.functional.unfold(x.reshape(-1, 1, *x.shape[-2:]), 2, stride=2)  # (planes, 4, windows)
        top = win.topk(2, dim=1).values
        pool.append(((top[:, 0] - top[:, 1]) / x.pow(2).mean().sqrt()).flatten())

    for mod in net.modules():
        if isinstance(mod, (nn.ReLU, nn.LeakyReLU)):
            mod.register_forward_hook(act_hook)
        elif isinstance(mod, nn.MaxPool2d):
            mod.register_forward_hook(pool_hook)

    real_warp = frvsr_ref.warp

    def spy(img, u, v):
        h, w = img.shape[-2:]
        m = frvsr_ref.mesh(h, w, img.dtype)
        for flow, base, size in ((u, m[..., 0], w), (v, m[..., 1], h)):
            coords.append((((base[None] + flow.detach() + 1) * size - 1) / 2).double().flatten())
            sizes.append(torch.full((flow.numel(),), float(size), dtype=torch.float64))
        return real_warp(img, u, v)

    frvsr_ref.warp = spy
    try:
        with torch.no_grad():
            net([x.to(dtype) for x in lr])
    finally:
        frvsr_ref.warp = real_warp
    return torch.cat(act), torch.cat(pool), torch.cat(coords), torch.cat(sizes)


def _ratio(dist, err):
    """min over the elements of (distance to the kink) / (own fp32-fp64 difference)."""
    return (dist / err.clamp_min(1e-300)).min().item()


def conditions(kwargs, shape, seed):
    a64, p64, c64, sizes = _probe(kwargs, shape, seed, torch.float64)
    a32, p32, c32, _ = _probe(kwargs, shape, seed, torch.float32)
    nearest = torch.minimum(torch.maximum(c64.round(), torch.zeros_like(c64)), sizes - 1)
    cdist = (c64 - nearest).abs()
    tie = (p64 == 0) & (p32 == 0)  # exact in both runs: see the module docstring
    ratios = dict(act_ratio=_ratio(a64.abs(), (a32 - a64).abs()),
                  pool_ratio=_ratio(p64[~tie], (p32 - p64).abs()[~tie]),
                  coord_ratio=_ratio(cdist, (c32 - c64).abs()))
    if min(ratios.values()) < MULT:
        return None
    return dict(margin_mult=MULT, **ratios,
                act_err32=(a32 - a64).abs().max().item(), act_min=a64.abs().min().item(),
                pool_err32=(p32 - p64).abs().max().item(), pool_min=p64[~tie].min().item(),
                n_pool_ties=int(tie.sum()),
                coord_err32=(c32 - c64).abs().max().item(), coord_min_dist=cdist.min().item(),
                n_act=a64.numel(), n_pool=p64.numel(), n_coord=c64.numel())


def find_seed(name, kwargs, shape):
    for seed in range(mg.SEED, mg.SEED + TRIES):
        c = conditions(kwargs, shape, seed)
        if c is not None:
            print(f"  {name}: seed {seed}, " + ", ".join(f"{k} {v:.2e}" for k, v in c.items() if not k.startswith("n_")), flush=True)
            return seed, c
    raise SystemExit(f"{name}: no seed in [{mg.SEED}, {mg.SEED + TRIES}) meets the margins")


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _flat(out):
    return torch.cat([t.flatten() for part in out for t in part])


def run_case(name, kwargs, shape):
    seed, cond = find_seed(name, kwargs, shape)
    full_max = FULL_GRAD_MAX[name]
    ref_cls = ref_loader.load(_MOD).FRVSRNet
    torch.manual_seed(seed)
    ref = ref_cls(**kwargs).train()
    mine = _net(kwargs, seed)
    rsd, msd = ref.state_dict(), mine.state_dict()
    assert list(rsd) == list(msd), f"{name}: state_dict keys differ"
    for k in rsd:
        assert torch.equal(rsd[k], msd[k]), f"{name}: init of {k} differs"
    init_sum = {k: float(v.double().sum()) for k, v in msd.items()}
    lr, hr = _data(shape, seed)
    outs, grads, losses = [], [], []
    for net in (ref, mine):
        net.zero_grad(set_to_none=True)
        out = net(lr)
        ls = frvsr_ref.loss(out, lr, hr)
        ls.backward()
        outs.append(out)
        losses.append(ls.detach())
        grads.append(_grads(net))
    for pr, pm in zip(outs[0], outs[1]):
        assert len(pr) == len(pm) == shape[1]
        for a, b in zip(pr, pm):
            assert torch.equal(a, b), f"{name}: outputs differ"
    assert torch.equal(losses[0], losses[1])
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), f"{name}: grad {k} differs"
    out = outs[1]
    # fp64 evaluation of the restatement: the accuracy yardstick
    m64 = _net(kwargs, seed, torch.float64)
    lr64, hr64 = [x.double() for x in lr], [x.double() for x in hr]
    out64 = m64(lr64)
    frvsr_ref.loss(out64, lr64, hr64).backward()
    g64 = _grads(m64)
    gmax = max(v.norm().item() for v in g64.values())
    # the reference's own fp32 error against it, worst over summation orders (thread counts) ...
    out_err32 = 0.0
    ref32_err = {k: (0.0 if v.norm().item() > 1e-9 * gmax else None) for k, v in g64.items()}
    nthreads = torch.get_num_threads()
    for nt in (1, 2, 4, nthreads):
        torch.set_num_threads(nt)
        m32 = _net(kwargs, seed)
        o32 = m32(lr)
        frvsr_ref.loss(o32, lr, hr).backward()
        out_err32 = max(out_err32, (_flat(o32).double() - _flat(out64).detach()).abs().max().item())
        for k, p in m32.named_parameters():
            if ref32_err[k] is not None:
                ref32_err[k] = max(ref32_err[k], (p.grad.double() - g64[k]).norm().item() / g64[k].norm().item())
    torch.set_num_threads(nthreads)
    # ... and the fp32 rounding envelope: fp64 runs with fp32-scale noise at every conv output and the
    # gradient flowing into it (make_golden.run_case, at NOISE_EPS_COND: the level of its searched cases)
    noise_err = {k: (0.0 if v is not None else None) for k, v in ref32_err.items()}
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
        mn = _net(kwargs, seed, torch.float64)
        for mod in mn.modules():
            if isinstance(mod, nn.modules.conv._ConvNd):
                mod.register_forward_hook(hook)
        frvsr_ref.loss(mn(lr64), lr64, hr64).backward()
        for k, p in mn.named_parameters():
            if noise_err[k] is not None:
                noise_err[k] = max(noise_err[k], (p.grad - g64[k]).norm().item() / g64[k].norm().item())
    ref32_err = {k: (None if v is None else max(v, noise_err[k])) for k, v in ref32_err.items()}
    worst = max(v for v in ref32_err.values() if v is not None)
    # 16-bit storage envelopes: make_golden's, with this net's loss in place of its own
    keep = mg._loss
    mg._loss = lambda o, target: frvsr_ref.loss(o, lr64, target)
    try:
        bf16_env = mg._bf16_envelope(FRVSRRef, kwargs, lr64, hr64, g64, ref32_err, seed)
        fp16_env = mg._bf16_envelope(FRVSRRef, kwargs, lr64, hr64, g64, ref32_err, seed, dtype=torch.float16)
    finally:
        mg._loss = keep
    # one Adam step from the reference's fp32 gradients
    ma = _net(kwargs, seed)
    frvsr_ref.loss(ma(lr), lr, hr).backward()
    opt = torch.optim.Adam(ma.parameters(), **mg.ADAM)
    p0 = {k: p.detach().clone() for k, p in ma.named_parameters()}
    opt.step()
    adam_update = {k: (p.detach() - p0[k]) for k, p in ma.named_parameters()}
    mine.eval()
    with torch.no_grad():
        out_eval = mine(lr)
    mine.train()
    sr = [o.detach() for o in out[0]]
    psnr = torch.stack([cpu_nets.psnr(cpu_nets.denormalize(o, "acdc"), cpu_nets.denormalize(t, "acdc"))
                        for o, t in zip(sr, hr)]).mean()
    fx = {
        "name": name, "class": "FRVSRNet", "kwargs": kwargs, "seed": seed, "kind": "frvsr",
        "param_sum": init_sum, "lr": lr, "hr": hr,
        "output": [sr, [o.detach() for o in out[1]]],
        "output64": [[o.detach() for o in part] for part in out64],
        "loss": float(losses[1]), "psnr_acdc": float(psnr),
        "out_err32": out_err32,
        "grad_norm64": {k: v.norm().item() for k, v in g64.items()},
        "grad_full64": {k: v for k, v in g64.items() if v.numel() <= full_max},
        "grad_proj64": {k: mg.proj(v, k, mg.PROJ) for k, v in g64.items()}, "proj_n": mg.PROJ,
        "grad_max64": gmax,
        "ref32_err": ref32_err, "noise_err": noise_err, "bf16_env": bf16_env, "fp16_env": fp16_env,
        "adam": {**mg.ADAM, "betas": list(mg.ADAM["betas"])},
        "adam_update_full": {k: v for k, v in adam_update.items() if v.numel() <= full_max},
        "adam_update_proj": {k: mg.proj(v.double(), k, mg.PROJ) for k, v in adam_update.items()},
        "adam_update_norm": {k: v.double().norm().item() for k, v in adam_update.items()},
        "output_eval": [[o.detach() for o in part] for part in out_eval],
        "cond_worst": worst, **cond,
    }
    mg.OUT.mkdir(parents=True, exist_ok=True)
    path = mg.OUT / f"{name}.pt"
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: fixture {size} bytes > {MAX_BYTES}; lower FULL_GRAD_MAX[{name!r}]"
    print(f"{name}: restatement == reference (bitwise), loss={fx['loss']:.6f} psnr={fx['psnr_acdc']:.4f} "
          f"fp32-vs-fp64: out {out_err32:.1e}, worst grad {worst:.1e}; bf16_env max "
          f"{max(v for v in bf16_env.values() if v is not None):.2e}; fixture {size / 1024:.0f} KiB", flush=True)


def main():
    if not ref_loader.available():
        raise SystemExit("reference not available (build container only)")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_loader._FILES[_MOD] = "src/model/nets/frvsr_net.py"
    only = os.environ.get("GOLDEN_ONLY")
    for name, (kwargs, shape) in CASES.items():
        if not only or name in only.split(","):
            run_case(name, kwargs, shape)


if __name__ == "__main__":
    main()
