"""TEST INFRASTRUCTURE ONLY -- golden fixtures of EDVRNet, made from the
reference itself.  Needs the reference tree (build container only):

    python tools/make_golden_edvr.py

Per case it builds the reference's EDVRNet (EDVR_arch.py and arch_util.py,
registered with oracle.ref_loader from here) and the restatement
tests/edvr_ref.EDVRRef from one seed, asserts identical initial weights,
output, L1 loss and every gradient bit for bit in fp32, and writes
tests/golden/<case>.pt with the keys of oracle.make_golden.run_case.

The reference's own `dcn` package cannot be imported: it loads a CUDA
extension.  A stub module src.model.nets.edvr_net.dcn is installed whose
ModulatedDeformConvPack is tests/edvr_ref.DCNPackRef, built on
oracle.dcn_ref.modulated_deform_conv_ref.  So the bitwise assertion pins
everything AROUND the DCN to the reference's execution, and the DCN
arithmetic itself stays pinned to the reference's SOURCE only, as
oracle/dcn_ref.py states.

Cases: edvr_x4_small runs the initial weights (conv_offset_mask zeroed: the
offsets are exactly zero in any precision, the sampler's integer-position
branch).  edvr_x4_offsets and edvr_x4_pad add seeded normal noise to every
conv_offset_mask weight and bias (edvr_ref.perturb_offset_convs: CPU
Generator(seed + 2), named_parameters order).  Its scale is set per seed from
one fp64 forward at scale 1 so that the offsets' rms is about half a pixel
(the offsets are close to linear in it); scale, the perturbed param_sum and the
offsets' rms and maximum are stored.

The seed (net init; inputs from seed + 1) is searched with
make_golden_frvsr.py's per-element margins: MULT = 3 times the element's own
difference between the restatement's fp32 and fp64 runs, so that in the fp64
run
  * every ReLU / LeakyReLU input is at least MULT x its own fp32-fp64
    difference from zero (in units of its tensor's rms),
  * every 3x3 stride-2 pool window's two largest values (padding -inf) are at
    least MULT x the fp32-fp64 difference of their gap apart -- or tie EXACTLY
    in both runs (n_pool_ties; the pad-and-crop case pads with a constant),
  * in the perturbed cases every DCN sampling coordinate is at least MULT x
    its own fp32-fp64 difference from the nearest integer in [-1, size], which
    covers the bilinear cell edges and the -1 / H / W validity edges
    (edvr_x4_small's coordinates are integers in both runs and exempt).
Every ratio, measured difference and count is stored in the fixture.

The 16-bit envelopes are make_golden._bf16_envelope's model with the two
changes this net's precision plan makes: conv_offset_mask's output and the
gradient flowing into it stay unrounded (offsets, masks and their gradients
are fp32 in every compute precision) and each DCN pack's output is rounded
like a conv's.
"""
from __future__ import annotations

import os
import sys
import types
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as Fn

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from oracle import cpu_nets, make_golden as mg, ref_loader  # noqa: E402
from tests import edvr_ref  # noqa: E402
from tests.edvr_ref import DCNPackRef, EDVRRef, perturb_offset_convs  # noqa: E402

_MOD = "src.model.nets.edvr_net.EDVR_arch"
_BASE = dict(in_channels=1, out_channels=1, nf=16, nframes=3, groups=2, front_RBs=1, back_RBs=1)
CASES = {
    # name: (kwargs, (B, N, C, H, W), perturbed)
    "edvr_x4_small": (_BASE, (2, 3, 1, 8, 12), False),
    "edvr_x4_offsets": (_BASE, (2, 3, 1, 8, 12), True),
    "edvr_x4_pad": (_BASE, (1, 3, 1, 6, 10), True),
}
FULL_GRAD_MAX = 3000  # elements up to which a gradient is stored in full; the rest by 16 projections
MAX_BYTES = 1 << 20
MULT = 3.0
TRIES = 2000
OFFSET_RMS = 0.5


def _data(shape, seed):
    return mg._inputs("misr", shape, 4, torch.Generator().manual_seed(seed + 1))


def _offsets(net, lr):
    edvr_ref.COORD_LOG = []
    try:
        with torch.no_grad():
            net(lr)
        log = edvr_ref.COORD_LOG
    finally:
        edvr_ref.COORD_LOG = None
    return log


def _scale(kwargs, shape, seed):
    """Perturbation scale that puts the offsets' rms near OFFSET_RMS (see the module docstring)."""
    lr, _ = _data(shape, seed)
    rms = _offset_stats(_net(kwargs, seed, 1.0, torch.float64), [x.double() for x in lr])[0]
    return float(f"{OFFSET_RMS / rms:.3g}")


def _offset_stats(net, lr):
    vals = []
    hooks = [m.conv_offset_mask.register_forward_hook(lambda mod, i, o: vals.append(o.detach()[:, :2 * o.shape[1] // 3]))
             for m in net.modules() if isinstance(m, DCNPackRef)]
    with torch.no_grad():
        net(lr)
    for h in hooks:
        h.remove()
    v = torch.cat([t.flatten() for t in vals]).double()
    return v.pow(2).mean().sqrt().item(), v.abs().max().item()


def _net(kwargs, seed, scale, dtype=torch.float32):
    torch.manual_seed(seed)
    net = EDVRRef(**kwargs).train()
    if scale:
        perturb_offset_convs(net, seed, scale)
    return net.double() if dtype == torch.float64 else net


def _probe(kwargs, shape, seed, scale, dtype):
    lr, _ = _data(shape, seed)
    net = _net(kwargs, seed, scale, dtype)
    act, pool = [], []

    def act_hook(mod, inp, out):
        x = inp[0].detach().double()
        act.append((x / x.pow(2).mean().sqrt()).flatten())

    def pool_hook(mod, inp, out):
        x = inp[0].detach().double()
        xp = Fn.pad(x.reshape(-1, 1, *x.shape[-2:]), (1, 1, 1, 1), value=float("-inf"))
        top = Fn.unfold(xp, 3, stride=2).topk(2, dim=1).values
        pool.append(((top[:, 0] - top[:, 1]) / x.pow(2).mean().sqrt()).flatten())

    for mod in net.modules():
        if isinstance(mod, (nn.ReLU, nn.LeakyReLU)):
            mod.register_forward_hook(act_hook)
        elif isinstance(mod, nn.MaxPool2d):
            mod.register_forward_hook(pool_hook)
    log = _offsets(net, [x.to(dtype) for x in lr])
    coords = torch.cat([c.double().flatten() for hs, ws, _, _ in log for c in (hs, ws)])
    sizes = torch.cat([torch.full((c.numel(),), float(s), dtype=torch.float64)
                       for hs, ws, h, w in log for c, s in ((hs, h), (ws, w))])
    return torch.cat(act), torch.cat(pool), coords, sizes


def _ratio(dist, err):
    return (dist / err.clamp_min(1e-300)).min().item()


def conditions(kwargs, shape, seed, perturbed):
    scale = _scale(kwargs, shape, seed) if perturbed else 0.0
    a64, p64, c64, sizes = _probe(kwargs, shape, seed, scale, torch.float64)
    a32, p32, c32, _ = _probe(kwargs, shape, seed, scale, torch.float32)
    tie = (p64 == 0) & (p32 == 0)
    ratios = dict(act_ratio=_ratio(a64.abs(), (a32 - a64).abs()),
                  pool_ratio=_ratio(p64[~tie], (p32 - p64).abs()[~tie]))
    extra = {}
    if perturbed:
        nearest = torch.minimum(torch.maximum(c64.round(), -torch.ones_like(c64)), sizes)
        cdist = (c64 - nearest).abs()
        ratios["coord_ratio"] = _ratio(cdist, (c32 - c64).abs())
        extra = dict(coord_err32=(c32 - c64).abs().max().item(), coord_min_dist=cdist.min().item(),
                     n_coord=c64.numel(), n_coord_outside=int(((c64 <= -1) | (c64 >= sizes)).sum()))
    else:
        assert torch.equal(c64, c64.round()) and torch.equal(c32, c64), "initial offsets are not exactly zero"
    if min(ratios.values()) < MULT:
        return None
    return dict(margin_mult=MULT, perturb_scale=scale, **ratios, **extra,
                act_err32=(a32 - a64).abs().max().item(), act_min=a64.abs().min().item(),
                pool_err32=(p32 - p64).abs().max().item(), pool_min=p64[~tie].min().item(),
                n_pool_ties=int(tie.sum()), n_act=a64.numel(), n_pool=p64.numel())


def find_seed(name, kwargs, shape, perturbed):
    for seed in range(mg.SEED, mg.SEED + TRIES):
        c = conditions(kwargs, shape, seed, perturbed)
        if c is not None:
            print(f"  {name}: seed {seed}, " + ", ".join(f"{k} {v:.2e}" for k, v in c.items() if not k.startswith("n_")),
                  flush=True)
            return seed, c
    raise SystemExit(f"{name}: no seed in [{mg.SEED}, {mg.SEED + TRIES}) meets the margins")


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def _envelope(kwargs, scale, lr64, hr64, g64, ref32_err, seed, dtype, draws=4):
    """make_golden._bf16_envelope with conv_offset_mask kept unrounded and the
    DCN packs' outputs rounded (see the module docstring)."""
    dither = 2.0 ** -12 if dtype == torch.bfloat16 else 2.0 ** -15
    gscale = float(2 ** (hr64.numel().bit_length() - 1)) if dtype == torch.float16 else 1.0
    env = {k: (0.0 if v is not None else None) for k, v in ref32_err.items()}
    for draw in range(draws):
        g = torch.Generator().manual_seed(seed + 100 + draw)

        def q(t):
            return (t + t.abs() * dither * torch.randn(t.shape, generator=g, dtype=t.dtype)).to(dtype).to(t.dtype)

        def qg(t):
            return q(t * gscale) / gscale

        def hook(mod, inp, out):
            out = out + (q(out.detach()) - out.detach())
            if out.requires_grad:
                out.register_hook(qg)
            return out

        m = _net(kwargs, seed, scale, torch.float64)
        om = {id(p.conv_offset_mask) for p in m.modules() if isinstance(p, DCNPackRef)}
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, (nn.Conv2d, DCNPackRef)):
                    mod.weight.copy_(mod.weight.to(dtype).double())
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, DCNPackRef)) and id(mod) not in om:
                mod.register_forward_hook(hook)
        Fn.l1_loss(m([q(t) for t in lr64]), hr64).backward()
        for k, p in m.named_parameters():
            if env[k] is not None:
                env[k] = max(env[k], (p.grad - g64[k]).norm().item() / g64[k].norm().item())
    return env


def run_case(name, kwargs, shape, perturbed):
    seed, cond = find_seed(name, kwargs, shape, perturbed)
    scale = cond["perturb_scale"]
    ref_cls = ref_loader.load(_MOD).EDVRNet
    torch.manual_seed(seed)
    ref = ref_cls(**kwargs).train()
    mine = _net(kwargs, seed, 0.0)
    rsd, msd = ref.state_dict(), mine.state_dict()
    assert list(rsd) == list(msd), f"{name}: state_dict keys differ"
    for k in rsd:
        assert torch.equal(rsd[k], msd[k]), f"{name}: init of {k} differs"
    if perturbed:
        perturb_offset_convs(ref, seed, scale)
        perturb_offset_convs(mine, seed, scale)
    init_sum = {k: float(v.double().sum()) for k, v in mine.state_dict().items()}
    lr, hr = _data(shape, seed)
    outs, grads, losses = [], [], []
    for net in (ref, mine):
        net.zero_grad(set_to_none=True)
        out = net(lr)
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
    # torch's own 1x1 conv (fea_fusion, N nf -> nf) sums in another order on one thread than on several, in
    # the reference as in the restatement (2 and 8 threads agree; 1 differs by an ulp in places): the
    # one-thread output is pinned to the reference too and stored beside the other
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)
    with torch.no_grad():
        out_t1 = mine(lr)
        assert torch.equal(ref(lr), out_t1), f"{name}: one-thread outputs differ"
    torch.set_num_threads(nthreads)
    lr64, hr64 = [x.double() for x in lr], hr.double()
    m64 = _net(kwargs, seed, scale, torch.float64)
    out64 = m64(lr64)
    Fn.l1_loss(out64, hr64).backward()
    g64 = _grads(m64)
    off_rms, off_max = _offset_stats(m64, lr64)
    gmax = max(v.norm().item() for v in g64.values())
    out_err32 = 0.0
    ref32_err = {k: (0.0 if v.norm().item() > 1e-9 * gmax else None) for k, v in g64.items()}
    nthreads = torch.get_num_threads()
    for nt in (1, 2, 4, nthreads):
        torch.set_num_threads(nt)
        m32 = _net(kwargs, seed, scale)
        o32 = m32(lr)
        Fn.l1_loss(o32, hr).backward()
        out_err32 = max(out_err32, (o32.double() - out64.detach()).abs().max().item())
        for k, p in m32.named_parameters():
            if ref32_err[k] is not None:
                ref32_err[k] = max(ref32_err[k], (p.grad.double() - g64[k]).norm().item() / g64[k].norm().item())
    torch.set_num_threads(nthreads)
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
        mn = _net(kwargs, seed, scale, torch.float64)
        for mod in mn.modules():
            if isinstance(mod, (nn.Conv2d, DCNPackRef)):
                mod.register_forward_hook(hook)
        Fn.l1_loss(mn(lr64), hr64).backward()
        for k, p in mn.named_parameters():
            if noise_err[k] is not None:
                noise_err[k] = max(noise_err[k], (p.grad - g64[k]).norm().item() / g64[k].norm().item())
    ref32_err = {k: (None if v is None else max(v, noise_err[k])) for k, v in ref32_err.items()}
    worst = max(v for v in ref32_err.values() if v is not None)
    bf16_env = _envelope(kwargs, scale, lr64, hr64, g64, ref32_err, seed, torch.bfloat16)
    fp16_env = _envelope(kwargs, scale, lr64, hr64, g64, ref32_err, seed, torch.float16)
    ma = _net(kwargs, seed, scale)
    Fn.l1_loss(ma(lr), hr).backward()
    opt = torch.optim.Adam(ma.parameters(), **mg.ADAM)
    p0 = {k: p.detach().clone() for k, p in ma.named_parameters()}
    opt.step()
    adam_update = {k: (p.detach() - p0[k]) for k, p in ma.named_parameters()}
    mine.eval()
    with torch.no_grad():
        out_eval = mine(lr)
    psnr = cpu_nets.psnr(cpu_nets.denormalize(out, "acdc"), cpu_nets.denormalize(hr, "acdc"))
    fx = {
        "name": name, "class": "EDVRNet", "kwargs": kwargs, "seed": seed, "kind": "misr", "perturbed": perturbed,
        "param_sum": init_sum, "lr": lr, "hr": hr, "output": out, "output_t1": out_t1, "output64": out64.detach(),
        "loss": float(losses[1]), "psnr_acdc": float(psnr), "out_err32": out_err32,
        "offset_rms": off_rms, "offset_max": off_max,
        "grad_norm64": {k: v.norm().item() for k, v in g64.items()},
        "grad_full64": {k: v for k, v in g64.items() if v.numel() <= FULL_GRAD_MAX},
        "grad_proj64": {k: mg.proj(v, k, mg.PROJ) for k, v in g64.items()}, "proj_n": mg.PROJ,
        "grad_max64": gmax,
        "ref32_err": ref32_err, "noise_err": noise_err, "bf16_env": bf16_env, "fp16_env": fp16_env,
        "adam": {**mg.ADAM, "betas": list(mg.ADAM["betas"])},
        "adam_update_full": {k: v for k, v in adam_update.items() if v.numel() <= FULL_GRAD_MAX},
        "adam_update_proj": {k: mg.proj(v.double(), k, mg.PROJ) for k, v in adam_update.items()},
        "adam_update_norm": {k: v.double().norm().item() for k, v in adam_update.items()},
        "output_eval": out_eval, "cond_worst": worst, **cond,
    }
    mg.OUT.mkdir(parents=True, exist_ok=True)
    path = mg.OUT / f"{name}.pt"
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: fixture {size} bytes > {MAX_BYTES}; lower FULL_GRAD_MAX"
    print(f"{name}: restatement == reference (bitwise), loss={fx['loss']:.6f} psnr={fx['psnr_acdc']:.4f} "
          f"offsets rms {off_rms:.3f} max {off_max:.2f}; fp32-vs-fp64: out {out_err32:.1e}, worst grad {worst:.1e}; "
          f"bf16_env max {max(v for v in bf16_env.values() if v is not None):.2e}; fixture {size / 1024:.0f} KiB",
          flush=True)


def main():
    if not ref_loader.available():
        raise SystemExit("reference not available (build container only)")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_loader._FILES["src.model.nets.edvr_net.arch_util"] = "src/model/nets/edvr_net/arch_util.py"
    ref_loader._FILES[_MOD] = "src/model/nets/edvr_net/EDVR_arch.py"
    for pkg in ("src", "src.model", "src.model.nets", "src.model.nets.edvr_net"):
        if pkg not in sys.modules:
            sys.modules[pkg] = types.ModuleType(pkg)
            sys.modules[pkg].__path__ = []
    stub = types.ModuleType("src.model.nets.edvr_net.dcn")
    stub.ModulatedDeformConvPack = DCNPackRef
    sys.modules["src.model.nets.edvr_net.dcn"] = stub
    ref_loader.load("src.model.nets.edvr_net.arch_util")
    only = os.environ.get("GOLDEN_ONLY")
    for name, (kwargs, shape, perturbed) in CASES.items():
        if not only or name in only.split(","):
            run_case(name, kwargs, shape, perturbed)


if __name__ == "__main__":
    main()
