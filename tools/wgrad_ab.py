"""Bitwise A/B of the weight gradient between two builds of the library.

  python tools/wgrad_ab.py --out a.pt                     this tree's libvsrk.so
  VSRK_LIB=/path/libvsrk.so python tools/wgrad_ab.py --out b.pt   another build
  python tools/wgrad_ab.py --compare a.pt b.pt            torch.equal of every tensor

A fixed, seeded table of small cases (the shapes of the tests) through
F.conv_wgrad, at least one per path x reduce kernel of vsrk_conv_wgrad:
pointwise; rolling-depth with both reduce kernels, grid caps and the sample
chunks; rolling-row plain, through a shuffled dy with perm_r, and the tap-skip
form; pipelined; the sub-pixel forms of the generic plan; thin; generic fp32,
ragged and 16-bit; the row-order reduce.  Each case runs with and without
dbias, plain and accumulating with dy_scale 0.5, in bf16 and fp16 (or fp32),
and every dw / db lands in one .pt file.  Run once per library in separate
processes (under rocprofv3 --kernel-trace --stats the kernel names and call
counts of the two runs pin the routing as well).
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vsr_amd import functional as F  # noqa: E402

DEV = "cuda"
K3, P1 = (1, 3, 3), (0, 1, 1)
K27 = (3, 3, 3)
H16 = (torch.bfloat16, torch.float16)
F32 = (torch.float32,)
PROJ = (6, 2, 2)  # DRF's x2 projection: ConvTranspose2d / Conv2d (k, s, p)

# name, (n, d, h, w), cin, cout, k, pad, options:
#   bn: BN-affine + ReLU prologue; caps: grid caps; paths: conv path modes;
#   dts: element types; cst / dy_cst: channels of the buffer x / dy is a slice of;
#   dy_r / x_r: the operand is a shuffle-r view (dims are the low-res grid);
#   perm_r; sub: "t" / "c" = the sub-pixel code of the transposed / strided projection
CASES = [
    ("pw_128_256", (2, 3, 20, 40), 128, 256, (1, 1, 1), (0, 0, 0), dict(bn=True)),
    ("roll_64_32", (1, 7, 16, 32), 64, 32, K27, (1, 1, 1), dict(caps=(0, 3), paths={"wgrad_roll": 1})),
    ("roll_64_32_bn", (1, 7, 16, 32), 64, 32, K27, (1, 1, 1), dict(bn=True, caps=(0, 3), paths={"wgrad_roll": 1})),
    ("roll_192_32", (1, 5, 16, 32), 192, 32, K27, (1, 1, 1), dict(caps=(0, 3), paths={"wgrad_roll": 1})),
    ("roll_192_32_bn", (1, 5, 16, 32), 192, 32, K27, (1, 1, 1), dict(bn=True, caps=(0, 3), paths={"wgrad_roll": 1})),
    # test_roll_gpu.py::test_roll_wgrad_sample_split: a view spanning more than 2^31 elements.  bf16 only, on
    # purpose: the buffer is 47 GB, and the chunk rule looks at strides and sizes, the same for both 16-bit types
    ("roll_chunks", (80, 7, 64, 64), 64, 32, K27, (1, 1, 1), dict(bn=True, cst=1024, dts=(torch.bfloat16,))),
    ("row_64_64", (2, 1, 19, 45), 64, 64, K3, P1, dict(caps=(0, 5), paths={"wgrad_row": 1})),
    ("row_upsampler", (2, 1, 11, 37), 64, 256, K3, P1, dict(dy_r=2, perm_r=2, paths={"wgrad_row": 1})),
    ("row_tapskip_t", (2, 1, 7, 23), 64, 256, K3, P1, dict(dy_r=2, sub="t", paths={"wgrad_row": 2})),
    ("row_tapskip_c", (2, 1, 7, 23), 256, 64, K3, P1, dict(x_r=2, sub="c", paths={"wgrad_row": 2})),
    ("pipe_96_32", (2, 5, 20, 40), 96, 32, K27, (0, 1, 1), dict(bn=True, caps=(0, 3), paths={"wgrad_roll": 0})),
    ("pipe_224_32", (2, 4, 12, 50), 224, 32, K27, (0, 1, 1), dict(bn=True, caps=(0, 3), paths={"wgrad_roll": 0})),
    ("sp_by1", (2, 1, 7, 23), 64, 256, K3, P1, dict(dy_r=2, sub="t", paths={"wgrad_row": 1})),
    ("sp_by2", (2, 1, 7, 23), 256, 64, K3, P1, dict(x_r=2, sub="c", paths={"wgrad_row": 1})),
    ("thin_1_64", (3, 1, 40, 70), 1, 64, K3, P1, dict(cst=8)),
    ("thin_64_1", (2, 1, 20, 70), 64, 1, K3, P1, dict(dy_cst=8)),
    ("generic_f32_64_64", (3, 1, 40, 70), 64, 64, K3, P1, dict(dts=F32, caps=(0, 3))),
    ("generic_ragged_40_24", (2, 3, 13, 37), 40, 24, K27, (1, 1, 1), dict(bn=True, dts=F32 + H16)),
    ("generic16_64_64", (3, 1, 40, 70), 64, 64, K3, P1, dict(caps=(0, 3), paths={"wgrad_row": 0, "wgrad_pipe": 0})),
    ("generic16_64_32_3d", (2, 5, 20, 40), 64, 32, K27, (1, 1, 1),
     dict(bn=True, paths={"wgrad_roll": 0, "wgrad_pipe": 0})),
    ("rows_64_256", (2, 1, 24, 40), 64, 256, K3, P1, dict()),
    ("rows_48_320", (1, 1, 20, 36), 48, 320, K3, P1, dict()),
]


def _operand(g, dims, c, r, cst, dt):
    """A (n, d, h, w, c) view; with r > 1 the physical image of a shuffle-r view of c logical channels."""
    n, d, h, w = dims
    if cst:  # a channel slice of a wider buffer
        big = torch.zeros((n, d, h, w, cst), dtype=dt, device=DEV)
        big[..., :c] = torch.randn((n, d, h, w, c), generator=g, device=DEV).to(dt)
        return big[..., :c]
    return torch.randn((n, d, h * r, w * r, c // (r * r)), generator=g, device=DEV).to(dt)


def run_case(case, out):
    name, dims, ci, co, k, pad, o = case
    xr, yr = o.get("x_r", 1), o.get("dy_r", 1)
    kw = dict(perm_r=o.get("perm_r", 1), x_shuffle=xr, dy_shuffle=yr)
    if "sub" in o:
        kw["subpixel"] = F.subpixel_code(*PROJ, o["sub"] == "t", False)
    do = dims[1] + 2 * pad[0] - (k[0] - 1)
    for dt in o.get("dts", H16):
        g = torch.Generator(device=DEV).manual_seed(len(name) * 131 + ci + co)
        x = _operand(g, dims, ci, xr, o.get("cst", 0), dt)
        dy = _operand(g, (dims[0], do) + dims[2:], co, yr, o.get("dy_cst", 0), dt)
        if o.get("bn"):
            kw.update(prologue=F.PRO_AFFINE_RELU, pro_scale=torch.rand(ci, generator=g, device=DEV) + 0.5,
                      pro_shift=torch.randn(ci, generator=g, device=DEV) * 0.5)
        dw0 = torch.randn((co, ci) + k, generator=g, device=DEV)
        db0 = torch.randn(co, generator=g, device=DEV)
        for path, mode in o.get("paths", {}).items():
            F.set_conv_path(path, mode)
        try:
            for cap in o.get("caps", (0,)):
                F.set_grid_cap(cap)
                for bias in (True, False):
                    for acc in (False, True):
                        dw = dw0.clone() if acc else torch.empty_like(dw0)
                        db = (db0.clone() if acc else torch.empty_like(db0)) if bias else None
                        F.conv_wgrad(x, dy, k, pad, dw, db, dy_scale=0.5 if acc else 1.0, accumulate=acc, **kw)
                        key = f"{name}/{str(dt).split('.')[-1]}/cap{cap}/bias{int(bias)}/acc{int(acc)}"
                        out[key + "/dw"] = dw.cpu()
                        if bias:
                            out[key + "/db"] = db.cpu()
        finally:
            F.set_grid_cap(0)
            for path in o.get("paths", {}):
                F.set_conv_path(path, -1)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="run the table and write every dw / db to this .pt file")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two such files bitwise")
    ap.add_argument("--only", help="substring of the case names to run")
    args = ap.parse_args()
    if args.compare:
        a, b = (torch.load(p, weights_only=True) for p in args.compare)
        bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or not torch.equal(a[k], b[k])]
        print(f"{len(a)} / {len(b)} tensors, {len(bad)} differ")
        for k in bad:
            print("  differs:", k)
        return 1 if bad or not a else 0
    out = {}
    for case in CASES:
        if not args.only or args.only in case[0]:
            run_case(case, out)
            print(f"{case[0]}: {len(out)} tensors so far", flush=True)
    torch.save(out, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
