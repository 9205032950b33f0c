"""Timing of SRFBNet and of the interpolating upsample kernel (DESIGN.md
section 7, profiles/r8_srfb_*.txt).

  --what upsample   vsrk_upsample2d_fwd at 64 x 1 x 128 x 128 -> 512^2: bilinear
                    (align_corners=False) and bicubic (align_corners=True), with
                    and without accumulate, fp32 / bf16: us per launch and GB/s
                    against the algorithmic bytes (y written, + y read when
                    accumulating; x is 1/16 of y and stays cached)
  --what step       ms per train step (forward + L1 over the steps + backward +
                    Adam) of SRFBNet with each way of folding the bilinear skip
                    in, and of DRFSISRNet with the same hyper-parameters as
                    context: 64 x 1 x 128 x 128, x4, F 64, G 4, 4 steps, bf16.
                    The nets alternate round by round in one process; median
                    and min over the rounds.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vsr_amd import _native, nets  # noqa: E402
from vsr_amd import functional as F  # noqa: E402
from vsr_amd.losses import L1Loss  # noqa: E402

DEV = "cuda"


def _time(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


def upsample(args):
    b, h, w, r = args.batch, args.size, args.size, args.scale
    g = torch.Generator().manual_seed(0)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn((b, 1, h, w), generator=g).to(DEV, dt)
        y = torch.randn((b, 1, h * r, w * r), generator=g).to(DEV, dt)
        ybytes = y.numel() * y.element_size()
        for mode, ac in (("bilinear", False), ("bicubic", True)):
            for acc in (False, True):
                fn = lambda: F.upsample2d(x, y, mode, ac, r, accumulate=acc)  # noqa: E731
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                ms = [_time(fn, args.iters) for _ in range(args.rounds)]
                med, nbytes = statistics.median(ms), ybytes * (2 if acc else 1)
                print(f"upsample2d {mode:8s} ac={int(ac)} acc={int(acc)} {str(dt)[6:]:8s} {b}x1x{h}x{w} x{r}: "
                      f"median {med * 1e3:7.1f} us  min {min(ms) * 1e3:7.1f} us  {nbytes / med / 1e6:7.1f} GB/s "
                      f"({nbytes / 2 ** 20:.0f} MiB)", flush=True)


def step(args):
    kw = dict(in_channels=1, out_channels=1, num_steps=args.steps, num_features=64, num_groups=4,
              upscale_factor=args.scale)
    b, h, r = args.batch, args.size, args.scale
    g = torch.Generator().manual_seed(0)
    x = torch.randn((b, 1, h, h), generator=g).to(DEV)
    hr = torch.randn((b, 1, h * r, h * r), generator=g).to(DEV)
    loss_fn = L1Loss()
    arms = {}
    for name in args.arms.split(","):
        torch.manual_seed(1)
        if name == "drf_sisr":
            net = nets.DRFSISRNet(**kw)
        else:
            net = nets.SRFBNet(**kw)
            net.SKIP_MODE = name.split(":")[1]
        net = net.to(DEV).set_precision("bf16").train()
        arms[name] = (net, torch.optim.Adam(net.parameters(), lr=1e-4))

    def one(name):
        net, opt = arms[name]
        opt.zero_grad(set_to_none=True)
        torch.stack([loss_fn(o, hr) for o in net(x)]).mean().backward()
        opt.step()

    for name in arms:
        for _ in range(args.warmup):
            one(name)
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name in arms:
            times[name].append(_time(lambda: one(name), args.iters))
    for name, ms in times.items():
        print(f"step {name:16s} {b}x1x{h}x{h} x{r} F64 G4 steps {args.steps} bf16: median {statistics.median(ms):8.2f} "
              f"ms  min {min(ms):8.2f} ms  max {max(ms):8.2f} ms  ({args.rounds} rounds x {args.iters})", flush=True)
    print(f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="upsample,step")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="srfb:accumulate,srfb:residual,drf_sisr")
    args = ap.parse_args()
    _native.load()
    for what in args.what.split(","):
        {"upsample": upsample, "step": step}[what](args)


if __name__ == "__main__":
    main()
