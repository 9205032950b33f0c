"""Timing of RBPNet's training step and of the PReLU-of-the-sum conv epilogue
alone (profiles/r13_rbp_step.txt and r13_rbp_sumact.txt).

  --what step    forward + L1 + backward + Adam of cfg9's RBPNet (base_filter
                 256, feat 64, 5 blocks, 7 frames, x4) in bf16 and fp32 against
                 tests/rbp_ref.py run by stock PyTorch in fp32 and under bf16
                 autocast; 3 steps per round.
  --what sumact  the 3x3 conv with act = VSRK_ACT_PRELU_SUM at B x 64 x 128 x 128
                 and B x 256 x 32 x 32 (RBPNet's HR and LR block tails) in bf16
                 against the same conv with the plain residual epilogue on the
                 same kernel (the rolling form): the same launch geometry,
                 bytes and FLOPs, the PReLU of the sum apart.  The plain arm
                 runs twice (first and last in every round): the difference
                 between its two figures is the spread the new epilogue is
                 judged against.  At 64 -> 64 the library's default routing
                 sends the plain residual form to the row-walking kernel
                 (conv_row.hip), which has no PReLU form: the three arms run
                 with that path off, and the default routing is timed after
                 them for reference.

Method: the arms of one comparison alternate inside one process, round by
round; each figure is the median over the rounds of the mean of `iters` calls
between two device events.  Beside the time, the share of 8 TB/s that the bytes
a call must move (every operand once) amount to.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vsr_amd import _native as N  # noqa: E402
from vsr_amd import functional as F  # noqa: E402

DEV = "cuda"
HBM = 8e12  # bytes / s, the vendor peak the shares are quoted against


def _time(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


def _compare(title, arms, args):
    """arms: [(name, fn, bytes)], timed alternately -> the medians (ms)."""
    print(title, flush=True)
    for _, fn, _ in arms:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in arms]
    for _ in range(args.rounds):
        for i, (_, fn, _) in enumerate(arms):
            ms[i].append(_time(fn, args.iters))
    meds = []
    for (name, _, nbytes), m in zip(arms, ms):
        med = statistics.median(m)
        meds.append(med)
        if not nbytes:  # a whole step: milliseconds, no byte count
            print(f"  {name:44s} median {med:9.2f} ms  min {min(m):9.2f} ms", flush=True)
            continue
        print(f"  {name:44s} median {med * 1e3:9.1f} us  min {min(m) * 1e3:9.1f} us  "
              f"{nbytes / HBM / (med * 1e-3):6.1%} of 8 TB/s ({nbytes / 2 ** 20:.0f} MiB)", flush=True)
    return meds


def sumact(args):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    a = torch.tensor([0.25], device=DEV)
    for c, size in ((64, 128), (256, 32)):
        b = args.batch
        x = torch.randn((b, 1, size, size, c), generator=g).to(DEV, dt)
        res = torch.randn((b, 1, size, size, c), generator=g).to(DEV, dt)
        y = torch.empty_like(x)
        wp = F.pack_weight((torch.randn((c, c, 1, 3, 3), generator=g) / (9 * c) ** 0.5).to(DEV), 0, dt)
        bias = torch.randn(c, generator=g).to(DEV)
        nbytes = 3 * x.numel() * 2 + wp.numel() * 2

        def plain():
            F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), bias=bias, residual=res)

        def fused():
            F.conv(x, wp, y, (1, 3, 3), (0, 1, 1), bias=bias, residual=res, act=F.ACT_PRELU_SUM, act_param=a)

        F.set_conv_path("row", 0)
        try:
            m = _compare(f"conv 3x3 {c} -> {c} + residual, B={b} {size}x{size} bf16, rolling kernel", [
                ("plain residual epilogue (run 1)", plain, nbytes),
                ("PReLU of the sum (VSRK_ACT_PRELU_SUM)", fused, nbytes),
                ("plain residual epilogue (run 2)", plain, nbytes),
            ], args)
        finally:
            F.set_conv_path("row", -1)
        spread = abs(m[0] - m[2])
        over = m[1] - min(m[0], m[2])
        print(f"  spread between the plain arm's two runs {spread * 1e3:.1f} us; PReLU of the sum minus the faster "
              f"plain run {over * 1e3:+.1f} us ({'within' if over <= spread else 'BEYOND'} the spread)", flush=True)
        _compare("  default routing, for reference", [("plain residual epilogue", plain, nbytes)], args)


def _step_arms(args):
    """name -> a function running one training step (forward, L1, backward, Adam) on B windows."""
    from tests.rbp_ref import RBPRef
    from vsr_amd import nets

    kw = dict(in_channels=1, out_channels=1, base_filter=args.base_filter, feat=args.feat, num_stages=3,
              num_resblocks=args.resblocks, num_frames=args.frames, upscale_factor=4)
    g = torch.Generator().manual_seed(0)
    lr = [torch.randn((args.batch, 1, args.size, args.size), generator=g).to(DEV) for _ in range(args.frames)]
    hr = torch.randn((args.batch, 1, 4 * args.size, 4 * args.size), generator=g).to(DEV)

    def arm(cls, precision, autocast):
        torch.manual_seed(0)
        net = cls(**kw).to(DEV).train()
        if precision is not None:
            net.set_precision(precision)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def fn():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                out = net(list(lr))
            torch.nn.functional.l1_loss(out.float(), hr).backward()
            opt.step()

        return fn

    return {"RBPNet bf16 (HIP)": lambda: arm(nets.RBPNet, "bf16", False),
            "RBPNet fp32 (HIP)": lambda: arm(nets.RBPNet, "fp32", False),
            "stock torch fp32": lambda: arm(RBPRef, None, False),
            "stock torch autocast bf16": lambda: arm(RBPRef, None, True)}


def step(args):
    arms = [(name, make(), 0) for name, make in _step_arms(args).items()]
    args = argparse.Namespace(**{**vars(args), "iters": 3})
    _compare(f"step B={args.batch} windows of {args.frames} x 1x{args.size}x{args.size}, base_filter "
             f"{args.base_filter}, feat {args.feat}, {args.resblocks} blocks, x4", arms, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="sumact", help="sumact, step (comma separated)")
    ap.add_argument("--batch", type=int, default=16, help="windows B (cfg9: 16)")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--size", type=int, default=32, help="LR size of the step (cfg9: 128 / 4)")
    ap.add_argument("--base-filter", dest="base_filter", type=int, default=256)
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--resblocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rbp_microbench needs an MI355X: timings come from device events (no CPU fallback)")
    N.load()
    for what in args.what.split(","):
        {"sumact": sumact, "step": step}[what](args)


if __name__ == "__main__":
    main()
