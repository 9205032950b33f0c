"""Train-step time of FRVSRNet (profiles/r9_frvsr_step.txt).

ms per step (forward + the FRVSR trainers' two L1 terms + backward + Adam) at
cfg 3's shape, 4 x T = 30 frames of 1 x 128 x 128 LR, x4, 10 resblocks: the HIP
path in bf16 and fp32, beside the stock-torch restatement tests/frvsr_ref.py run
by PyTorch-ROCm on the same GPU in fp32 and under bf16 autocast (it builds its
mesh on the host per warp, as the reference's STN does).  The arms alternate
round by round in one process; median and min over the rounds.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import frvsr_ref  # noqa: E402
from vsr_amd import _native, nets  # noqa: E402

DEV = "cuda"


def _time(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--resblocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default="hip:bf16,hip:fp32,torch:fp32,torch:bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frvsr_microbench needs an MI355X: timings come from device events (no CPU fallback)")
    _native.load()
    kw = dict(in_channels=1, out_channels=1, upscale_factor=4, num_resblocks=args.resblocks)
    g = torch.Generator().manual_seed(0)
    b, t, s = args.batch, args.frames, args.size
    lr = [torch.randn((b, 1, s, s), generator=g).to(DEV) for _ in range(t)]
    hr = [torch.randn((b, 1, 4 * s, 4 * s), generator=g).to(DEV) for _ in range(t)]
    arms = {}
    for name in args.arms.split(","):
        kind, prec = name.split(":")
        torch.manual_seed(1)
        if kind == "hip":
            net = nets.FRVSRNet(**kw).to(DEV).set_precision(prec).train()
        else:
            net = frvsr_ref.FRVSRRef(**kw).to(DEV).train()
        arms[name] = (kind, prec, net, torch.optim.Adam(net.parameters(), lr=1e-4))

    def one(name):
        kind, prec, net, opt = arms[name]
        opt.zero_grad(set_to_none=True)
        if kind == "torch" and prec == "bf16":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = net(lr)
            out = ([o.float() for o in out[0]], [o.float() for o in out[1]])
        else:
            out = net(lr)
        frvsr_ref.loss(out, lr, hr).backward()
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
        print(f"step {name:12s} {b} x T={t} x 1x{s}x{s} x4, {args.resblocks} resblocks: median "
              f"{statistics.median(ms):9.2f} ms  min {min(ms):9.2f} ms  max {max(ms):9.2f} ms  "
              f"({args.rounds} rounds x {args.iters})", flush=True)
    print(f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)


if __name__ == "__main__":
    main()
