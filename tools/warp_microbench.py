"""Timing of the flow-warp, max-pool and channels-last bilinear kernels
(profiles/r9_warp_*.txt).

  --what warp      vsrk_flow_warp_fwd + vsrk_flow_warp_bwd at 120 x 1 x 512 x 512
                   ('border', align_corners=False: FRVSR's HR warp of 4 x 30
                   frames at 128^2 x4), fp32 and bf16 images, plain and with the
                   space-to-depth store, the SR warp from the LR flow with the x4
                   interpolation inside the kernel (flow_up) against upsample2d
                   followed by the warp, beside F.grid_sample forward + backward
                   (gradient to the grid only) of stock PyTorch on the same
                   GPU.  us per call and the share of 8 TB/s that the bytes
                   each call must move (image, flow, output / output gradient,
                   flow gradient, once each) amount to.
  --what fnet      vsrk_max_pool2x2_fwd / _bwd and vsrk_upsample_cl_fwd / _bwd at
                   FNet's shapes for 120 frame pairs of 128^2 (32 / 64 / 128
                   channels down, 256 / 128 / 64 channels up), bf16, beside
                   F.max_pool2d / F.interpolate on channels_last tensors.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as Fn

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vsr_amd import _native  # noqa: E402
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


def _report(name, fn, nbytes, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = [_time(fn, args.iters) for _ in range(args.rounds)]
    med = statistics.median(ms)
    share = f"{nbytes / HBM / (med * 1e-3):6.1%} of 8 TB/s ({nbytes / 2 ** 20:.0f} MiB)" if nbytes else ""
    print(f"{name:58s} median {med * 1e3:8.1f} us  min {min(ms) * 1e3:8.1f} us  {share}", flush=True)


def warp(args):
    n, h, w, r = args.batch, args.size, args.size, args.scale
    g = torch.Generator().manual_seed(0)
    flow = ((torch.rand((n, 2, h, w), generator=g) - 0.5) * 8 / h).to(DEV)  # +- 2 px
    my, mx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    mesh = torch.stack([mx, my], -1)[None].to(DEV)
    for dt in (torch.float32, torch.bfloat16):
        es = torch.empty((), dtype=dt).element_size()
        img = torch.randn((n, 1, h, w, 1), generator=g).to(DEV, dt)
        gout = torch.randn((n, 1, h, w, 1), generator=g).to(DEV, dt)
        out, gflow = torch.empty_like(img), torch.empty_like(flow)
        pix = n * h * w
        fwd_bytes, bwd_bytes = pix * (2 * es + 8), pix * (2 * es + 16)
        tag = f"{str(dt)[6:]:8s} {n}x1x{h}x{w}"
        _report(f"flow_warp fwd {tag}", lambda: F.flow_warp(img, flow, out, "border", False), fwd_bytes, args)
        _report(f"flow_warp bwd {tag}", lambda: F.flow_warp_bwd(img, flow, gout, gflow, "border", False), bwd_bytes,
                args)
        wide = torch.empty((n, 1, h // r, w // r, r * r + 1), dtype=dt, device=DEV)
        _report(f"flow_warp fwd s2d={r} into {r * r + 1} ch {tag}",
                lambda: F.flow_warp(img, flow, wide[..., :r * r], "border", False, s2d=r), fwd_bytes, args)
        # the SR warp from the LR flow, A/B: interpolated inside the warp (flow_up = r), or by upsample2d into
        # two fp32 HR planes that the warp then reads (the planes: 8 B written + 8 B read per pixel)
        lo = ((torch.rand((n, 2, h // r, w // r), generator=g) - 0.5) * 8 / h).to(DEV)
        hi = torch.empty_like(flow)

        def unfused():
            F.upsample2d(lo, hi, "bilinear", True, r)
            F.flow_warp(img, hi, wide[..., :r * r], "border", False, s2d=r)

        _report(f"SR warp fused: flow_up={r} s2d={r} {tag}",
                lambda: F.flow_warp(img, lo, wide[..., :r * r], "border", False, s2d=r, flow_up=r),
                pix * (2 * es) + pix * 8 // (r * r), args)
        _report(f"SR warp unfused: upsample2d + warp s2d={r} {tag}", unfused, pix * (2 * es + 16) + pix * 8 // (r * r),
                args)
        _report(f"flow_warp bwd flow_up={r} {tag}",
                lambda: F.flow_warp_bwd(img, lo, gout, gflow, "border", False, flow_up=r),
                pix * (2 * es + 8) + pix * 8 // (r * r), args)
        # stock PyTorch: the grid is built outside the timed region
        im = img.view(n, 1, h, w)
        grid = (mesh + flow.permute(0, 2, 3, 1)).to(dt).requires_grad_(True)
        go = gout.view(n, 1, h, w)

        def torch_fwd():
            with torch.no_grad():
                Fn.grid_sample(im, grid, mode="bilinear", padding_mode="border", align_corners=False)

        def torch_both():
            grid.grad = None
            Fn.grid_sample(im, grid, mode="bilinear", padding_mode="border", align_corners=False).backward(go)

        _report(f"F.grid_sample fwd {tag} (grid in {str(dt)[6:]})", torch_fwd, 0, args)
        _report(f"F.grid_sample fwd + bwd {tag}", torch_both, 0, args)


def fnet(args):
    n, s, dt = args.batch, args.size // args.scale, torch.bfloat16
    g = torch.Generator().manual_seed(0)
    for c, hw in ((32, s), (64, s // 2), (128, s // 4)):
        x = torch.randn((n, 1, hw, hw, c), generator=g).to(DEV, dt)
        y = torch.empty((n, 1, hw // 2, hw // 2, c), dtype=dt, device=DEV)
        gy, gx = torch.randn_like(y), torch.empty_like(x)
        nb = x.numel() * 2
        tag = f"bf16 {n}x{hw}x{hw}x{c}"
        _report(f"max_pool2x2 fwd {tag}", lambda: F.max_pool2x2(x, y), nb + nb // 4, args)
        _report(f"max_pool2x2 bwd {tag}", lambda: F.max_pool2x2_bwd(x, gy, gx), 2 * nb + nb // 4, args)
        xt = x[:, 0].permute(0, 3, 1, 2).requires_grad_(True)  # channels_last NCHW

        def torch_both():
            xt.grad = None
            Fn.max_pool2d(xt, 2).backward(gy[:, 0].permute(0, 3, 1, 2))

        _report(f"F.max_pool2d fwd + bwd {tag} channels_last", torch_both, 0, args)
    for c, hw in ((256, s // 8), (128, s // 4), (64, s // 2)):
        x = torch.randn((n, 1, hw, hw, c), generator=g).to(DEV, dt)
        y = torch.empty((n, 1, 2 * hw, 2 * hw, c), dtype=dt, device=DEV)
        gy, gx = torch.randn_like(y), torch.empty_like(x)
        nb = x.numel() * 2
        tag = f"bf16 {n}x{hw}x{hw}x{c} x2"
        _report(f"upsample_cl fwd {tag}", lambda: F.upsample_cl(x, y, 2, False), 5 * nb, args)
        _report(f"upsample_cl bwd {tag}", lambda: F.upsample_cl_bwd(gy, gx, 2, False), 5 * nb, args)
        xt = x[:, 0].permute(0, 3, 1, 2).requires_grad_(True)

        def torch_both():
            xt.grad = None
            Fn.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False).backward(
                gy[:, 0].permute(0, 3, 1, 2))

        _report(f"F.interpolate fwd + bwd {tag} channels_last", torch_both, 0, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="warp,fnet")
    ap.add_argument("--batch", type=int, default=120)
    ap.add_argument("--size", type=int, default=512, help="HR size; FNet runs at size / scale")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("warp_microbench needs an MI355X: timings come from device events (no CPU fallback)")
    _native.load()
    for what in args.what.split(","):
        {"warp": warp, "fnet": fnet}[what](args)


if __name__ == "__main__":
    main()
