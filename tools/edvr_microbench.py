"""Timing of EDVRNet's training step and of its kernels alone (DESIGN.md
section 7, profiles/r10_edvr_step.txt and r10_edvr_microbench.txt).

  --what step  forward + L1 + backward + Adam of EDVRNet in bf16 and fp32
               against tests/edvr_ref.py run by stock PyTorch with the fp32
               NCHW layer op vsr_amd.dcn in its packs, in fp32 and under bf16
               autocast; 3 steps per round.  --what one_step: three bf16 steps
               alone, for a kernel trace.
  --what dcn   the DCN sampling kernels on views (vsrk_dcn_view_im2col /
               _coord_grad / _col2im) at EDVR's level-1 alignment shape, B*N x
               64 x 128^2 with 8 deformable groups: fp32 views against the
               NCHW-plane fp32 kernels (vsrk_dcn_im2col / _coord_grad / _col2im
               fed the decoded offset and mask planes; the chunk / cat / sigmoid
               that produce those planes in torch are NOT in their time), and
               bf16 views against fp32 views.
  --what tsa   vsrk_tsa_tatt, vsrk_pool3s2 and vsrk_tsa_modulate, forward and
               backward, at B x N x 64 x 128^2 in bf16 and fp32.

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
K = 9


def _time(fn, iters):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(iters):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / iters


def _compare(title, arms, args):
    """arms: [(name, fn, bytes)], timed alternately."""
    print(title, flush=True)
    for _, fn, _ in arms:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in arms]
    for _ in range(args.rounds):
        for i, (_, fn, _) in enumerate(arms):
            ms[i].append(_time(fn, args.iters))
    for (name, _, nbytes), m in zip(arms, ms):
        med = statistics.median(m)
        if not nbytes:  # a whole step: milliseconds, no byte count
            print(f"  {name:44s} median {med:9.2f} ms  min {min(m):9.2f} ms", flush=True)
            continue
        print(f"  {name:44s} median {med * 1e3:9.1f} us  min {min(m) * 1e3:9.1f} us  "
              f"{nbytes / HBM / (med * 1e-3):6.1%} of 8 TB/s ({nbytes / 2 ** 20:.0f} MiB)", flush=True)


def _es(dt):
    return torch.empty((), dtype=dt).element_size()


def dcn(args):
    n, h, w, c, G = args.batch * args.frames, args.size, args.size, args.channels, args.groups
    g = torch.Generator().manual_seed(0)
    om = torch.randn((n, 1, h, w, 3 * G * K), generator=g)
    om[..., :2 * G * K] *= 2  # offsets of +- a few pixels, mask logits of order one
    om = om.to(DEV)
    gom = torch.empty_like(om)
    o1, o2, m = torch.chunk(om[:, 0].permute(0, 3, 1, 2), 3, dim=1)
    offset, mask = torch.cat((o1, o2), 1).contiguous(), torch.sigmoid(m).contiguous()
    goff, gmask = torch.empty_like(offset), torch.empty_like(mask)
    lib = N.load()
    sp = N.stream_ptr(om.device)
    pix = n * h * w
    t = {}
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn((n, 1, h, w, c), generator=g).to(DEV, dt)
        cols = torch.empty((n, 1, h, w, K * c), dtype=dt, device=DEV)
        t[dt] = (x, cols, torch.randn_like(cols), torch.zeros((n, 1, h, w, c), device=DEV))
    geo, _, _ = F.dcn_geometry(t[torch.float32][0], deformable_groups=G)
    x32, cols32, gcols32, gx32 = t[torch.float32]

    def nbytes(dt, has_x, has_cols=1, extra=0):
        return pix * (has_x * c * _es(dt) + has_cols * K * c * _es(dt) + 3 * G * K * 4 + extra)

    def view(fn, dt):
        x, cols, gcols, gx = t[dt]
        return {"im2col": lambda: F.dcn_view_im2col(geo, x, om, cols),
                "coord_grad": lambda: F.dcn_view_coord_grad(geo, x, gcols, om, gom),
                "col2im": lambda: F.dcn_view_col2im(geo, gcols, om, gx)}[fn]

    plane = {
        "im2col": lambda: lib.vsrk_dcn_im2col(geo, x32.data_ptr(), offset.data_ptr(), mask.data_ptr(),
                                              cols32.data_ptr(), sp),
        "coord_grad": lambda: lib.vsrk_dcn_coord_grad(geo, x32.data_ptr(), gcols32.data_ptr(), offset.data_ptr(),
                                                      mask.data_ptr(), goff.data_ptr(), gmask.data_ptr(), sp),
        "col2im": lambda: lib.vsrk_dcn_col2im(geo, gcols32.data_ptr(), offset.data_ptr(), mask.data_ptr(),
                                              gx32.data_ptr(), sp),
    }
    # bytes: x, om, cols | x, gcols, om, gom | gcols, om, fp32 gx (the scatter keeps adding into gx: timing only)
    shape = {"im2col": (1, 1, 0), "coord_grad": (1, 1, 3 * G * K * 4), "col2im": (0, 1, c * 4)}
    for fn, (hx, hc, extra) in shape.items():
        _compare(f"dcn {fn} {n}x{h}x{w}x{c} G={G}", [
            (f"view fp32 (vsrk_dcn_view_{fn})", view(fn, torch.float32), nbytes(torch.float32, hx, hc, extra)),
            (f"planes fp32 (vsrk_dcn_{fn})", plane[fn], nbytes(torch.float32, hx, hc, extra)),
            (f"view bf16 (vsrk_dcn_view_{fn})", view(fn, torch.bfloat16), nbytes(torch.bfloat16, hx, hc, extra)),
        ], args)


def tsa(args):
    b, nf, h, w, c = args.batch, args.frames, args.size, args.size, args.channels
    g = torch.Generator().manual_seed(0)
    arms = {k: [] for k in ("tatt fwd", "tatt bwd", "pool3s2 fwd", "pool3s2 bwd", "modulate fwd", "modulate bwd")}
    for dt in (torch.bfloat16, torch.float32):
        es, tag = _es(dt), str(dt)[6:]
        emb = (torch.randn((b * nf, 1, h, w, c), generator=g) * 0.3).to(DEV, dt)
        ref, al = emb[:b].clone(), torch.randn_like(emb)
        out = torch.empty((b, 1, h, w, nf * c), dtype=dt, device=DEV)
        prob = torch.empty((b, nf, h, w), device=DEV)
        gout, ge, gr, ga = torch.randn_like(out), torch.empty_like(emb), torch.empty_like(ref), torch.empty_like(al)
        F.tsa_tatt(emb, ref, al, out, prob)
        frame, pb = b * nf * h * w * c * es, b * nf * h * w * 4
        arms["tatt fwd"].append((tag, lambda emb=emb, ref=ref, al=al, out=out, prob=prob:
                                 F.tsa_tatt(emb, ref, al, out, prob), 3 * frame + frame // nf + pb))
        arms["tatt bwd"].append((tag, lambda emb=emb, ref=ref, al=al, prob=prob, gout=gout, ge=ge, gr=gr, ga=ga:
                                 F.tsa_tatt_bwd(emb, ref, al, prob, gout, ge, gr, ga),
                                 5 * frame + 2 * (frame // nf) + pb))
        x = torch.randn((b, 1, h, w, c), generator=g).to(DEV, dt)
        y = torch.empty((b, 1, h // 2, w // 2, 2 * c), dtype=dt, device=DEV)
        gy, gx = torch.randn_like(y), torch.empty_like(x)
        one = x.numel() * es
        arms["pool3s2 fwd"].append((tag, lambda x=x, y=y: F.pool3s2(x, y), one + one // 2))
        arms["pool3s2 bwd"].append((tag, lambda x=x, gy=gy, gx=gx: F.pool3s2_bwd(x, gy, gx), 2 * one + one // 2))
        att, add, o2 = torch.randn_like(x), torch.randn_like(x), torch.empty_like(x)
        gf, gt = torch.empty_like(x), torch.empty_like(x)
        arms["modulate fwd"].append((tag, lambda x=x, att=att, add=add, o2=o2: F.tsa_modulate(x, att, add, o2),
                                     4 * one))
        arms["modulate bwd"].append((tag, lambda x=x, att=att, add=add, gf=gf, gt=gt:
                                     F.tsa_modulate_bwd(x, att, add, gf, gt), 5 * one))
    for name, a in arms.items():
        _compare(f"tsa {name} B={b} N={nf} {h}x{w}x{c}", a, args)


def _step_arms(args):
    """name -> a function running one training step (forward, L1, backward, Adam) on B windows."""
    import types

    from tests.edvr_ref import DCNPackRef, EDVRRef, perturb_offset_convs
    from vsr_amd import dcn as hip_dcn
    from vsr_amd import nets

    kw = dict(in_channels=1, out_channels=1, nf=args.channels, nframes=args.frames, groups=args.groups)
    g = torch.Generator().manual_seed(0)
    lr = [torch.randn((args.batch, 1, args.size, args.size), generator=g).to(DEV) for _ in range(args.frames)]
    hr = torch.randn((args.batch, 1, 4 * args.size, 4 * args.size), generator=g).to(DEV)

    def pack_forward(self, x):  # the restatement's pack on the library's fp32 NCHW DCN layer op
        x, fea = x
        o1, o2, mask = torch.chunk(self.conv_offset_mask(fea), 3, dim=1)
        return hip_dcn.modulated_deform_conv(x.float(), torch.cat((o1, o2), 1).float(), torch.sigmoid(mask).float(),
                                             self.weight, self.bias, 1, 1, 1, 1, self.deformable_groups).to(x.dtype)

    def arm(cls, precision, autocast):
        torch.manual_seed(0)
        net = perturb_offset_convs(cls(**kw), 0, 0.5).to(DEV).train()  # offsets of about half a pixel
        if cls is EDVRRef:
            for m in net.modules():
                if isinstance(m, DCNPackRef):
                    m.forward = types.MethodType(pack_forward, m)
        else:
            net.set_precision(precision)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def fn():
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                out = net(lr)
            torch.nn.functional.l1_loss(out.float(), hr).backward()
            opt.step()

        return fn

    return {"EDVRNet bf16 (HIP)": lambda: arm(nets.EDVRNet, "bf16", False),
            "EDVRNet fp32 (HIP)": lambda: arm(nets.EDVRNet, "fp32", False),
            "stock torch fp32 + vsr_amd.dcn": lambda: arm(EDVRRef, None, False),
            "stock torch autocast bf16 + vsr_amd.dcn": lambda: arm(EDVRRef, None, True)}


def step(args):
    """The training step against the restatement run by stock PyTorch with the
    library's fp32 DCN layer op in its packs (the only DCN that ran on the GPU
    before EDVRNet): median of `rounds` rounds x 3 steps, arms alternating."""
    arms = [(name, make(), 0) for name, make in _step_arms(args).items()]
    args = argparse.Namespace(**{**vars(args), "iters": 3})
    _compare(f"step B={args.batch} windows of {args.frames} x 1x{args.size}x{args.size}, nf {args.channels}, "
             f"G {args.groups}", arms, args)


def one_step(args):
    """Three bf16 steps of EDVRNet and nothing else: the workload of a kernel-trace run."""
    fn = _step_arms(args)["EDVRNet bf16 (HIP)"]()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="dcn,tsa", help="dcn, tsa, step, one_step (comma separated)")
    ap.add_argument("--batch", type=int, default=4, help="windows B")
    ap.add_argument("--frames", type=int, default=5, help="frames per window N")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edvr_microbench needs an MI355X: timings come from device events (no CPU fallback)")
    N.load()
    for what in args.what.split(","):
        {"dcn": dcn, "tsa": tsa, "step": step, "one_step": one_step}[what](args)


if __name__ == "__main__":
    main()
