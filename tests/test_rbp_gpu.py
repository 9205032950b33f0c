"""RBPNet on the GPU.

Golden runs: the rbp_* fixtures (tools/make_golden_rbp.py: the reference's own
RBPNet, with the restatement equal to it bit for bit) in fp32 / bf16 / fp16
under tests/test_edvr_gpu.py's rules -- the output against the fp64 run (fp32
max(1e-4, 3 x the reference's fp32 error); bf16 max 3e-2 / mean 3e-3; fp16 max
5e-3 / mean 5e-4), PSNR within 0.01 dB, every parameter gradient against fp64
(in full or by its 16 projections) at max(1e-4, 3 ref32_err) in fp32,
max(5e-2, 2 bf16_env) in bf16, max(3e-2, 3 fp16_env) in fp16 -- one Adam step
against adam_update_* at 1e-3, and the no_grad output against output_eval.
No parameter is skipped.  rbp_x4_small: tile / fast kernels, batch 2.
rbp_x2_roll: an even frame count, 64-channel blocks and sub-pixel projections
on the rolling kernels, HR 20 x 36 across the rolling tile.  rbp_x3_slopes:
slopes 0.25, -0.1, 0.0 and 1.5 (stored), non-positive on block tails and
projections: the pre-activation backward.

Variants against the stock-torch restatement tests/rbp_ref.py run in fp64, at
max(1e-4, 3 x the restatement's own fp32 error against its fp64 run, the worst
over 1, 2, 4 and the default number of threads as in the fixtures): x8 at LR
4 x 4, five frames, batch 3.

The forward is bitwise equal between two calls, the caller's list is left as
it was, and, read from the dispatch log of a child process (the log switch is
read when the library loads), the block-tail convs of rbp_x2_roll at bf16 run
on the rolling form and not on the tile kernel.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import test_nets_gpu as tn
from tests.conftest import load_golden
from tests.rbp_ref import RBPRef, set_slopes
from vsr_amd import nets

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ["rbp_x4_small", "rbp_x2_roll", "rbp_x3_slopes"]

BASE = dict(in_channels=1, out_channels=1, base_filter=32, feat=16, num_stages=3, num_resblocks=1, num_frames=3,
            upscale_factor=4)
VARIANTS = {  # kwargs, (B, N, C, h, w)
    "x8": (dict(BASE, upscale_factor=8), (1, 3, 1, 4, 4)),
    "five_frames": (dict(BASE, num_frames=5), (1, 5, 1, 6, 8)),
    "batch3": (BASE, (3, 3, 1, 6, 8)),
}


def _build(fx, precision):
    torch.manual_seed(fx["seed"])
    net = nets.RBPNet(**fx["kwargs"])
    if fx["perturbed"]:
        set_slopes(net, fx["slopes"])
    for k, v in net.state_dict().items():
        assert abs(float(v.double().sum()) - fx["param_sum"][k]) <= 1e-9 * (1 + abs(fx["param_sum"][k])), k
    return net.to(DEV).set_precision(precision).train()


def _golden_step(fx, precision):
    net = _build(fx, precision)
    lr, hr = tn._to(fx["lr"]), tn._to(fx["hr"])
    out = net(lr)
    assert len(lr) == fx["kwargs"]["num_frames"]  # the caller's list is not mutated
    loss = torch.nn.functional.l1_loss(out, hr)
    loss.backward()
    torch.cuda.synchronize()
    return net, out, loss, hr


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", GOLDEN)
def test_net_matches_golden(name, precision):
    fx = load_golden(name)
    net, out, loss, hr = _golden_step(fx, precision)
    assert out.shape == fx["output64"].shape and out.dtype == torch.float32
    d = (out.detach().cpu().double() - fx["output64"].double()).abs()
    print(f"{name} {precision}: out max|d| {d.max().item():.2e} mean {d.mean().item():.2e} "
          f"(reference fp32 {fx['out_err32']:.2e})")
    if precision == "fp32":
        assert d.max().item() <= max(1e-4, 3 * fx["out_err32"]), d.max().item()
        assert abs(loss.item() - fx["loss"]) <= 1e-5 * (1 + abs(fx["loss"]))
    elif precision == "fp16":
        assert d.max().item() <= 5e-3 and d.mean().item() <= 5e-4, (d.max().item(), d.mean().item())
    else:
        assert d.max().item() <= 3e-2 and d.mean().item() <= 3e-3, (d.max().item(), d.mean().item())
    assert abs(tn._psnr(out.detach(), hr).item() - fx["psnr_acdc"]) <= 0.01
    bad = []
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        g = p.grad.detach().cpu().double()
        r32 = fx["ref32_err"][k]
        assert r32 is not None, k  # no parameter of these fixtures is skipped
        rel = tn._rel(g, fx, k)
        if precision == "fp32":
            tol = max(1e-4, 3 * r32)
        elif precision == "fp16":
            tol = max(3e-2, 3 * fx["fp16_env"][k])
        else:
            tol = max(5e-2, 2 * fx["bf16_env"][k])
        print(f"  {k}: rel {rel:.2e} tol {tol:.2e}")
        if not rel <= tol:
            bad.append((k, rel, tol))
    assert not bad, bad
    if precision == "fp16":
        assert net.step_ok()


@pytest.mark.parametrize("name", GOLDEN)
def test_adam_step_on_hip_gradients(name):
    """One Adam step on the fp32 HIP gradients reproduces the reference's update, rel-L2 <= 1e-3."""
    fx = load_golden(name)
    net, _, _, _ = _golden_step(fx, "fp32")
    a = fx["adam"]
    opt = torch.optim.Adam(net.parameters(), lr=a["lr"], betas=tuple(a["betas"]), eps=a["eps"])
    p0 = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt.step()
    for k, p in net.named_parameters():
        upd = (p.detach() - p0[k]).cpu().double()
        if k in fx["adam_update_full"] and k in fx["grad_full64"]:
            gref, uref = fx["grad_full64"][k].double(), fx["adam_update_full"][k].double()
            keep = gref.abs() > 1e-6 * gref.abs().max()
            assert (upd.abs() <= a["lr"] * 1.001).all(), k
            rel = ((upd - uref)[keep].norm() / uref[keep].norm()).item()
        else:
            rel = tn._rel(upd, fx, k, "adam_update_full", "adam_update_proj", "adam_update_norm")
        print(f"  {k}: update rel {rel:.2e}")
        assert rel <= 1e-3, (k, rel)


@pytest.mark.parametrize("name", GOLDEN)
def test_eval_output_matches_golden_and_forward_is_bitwise(name):
    fx = load_golden(name)
    net = _build(fx, "fp32").eval()
    lr = tn._to(fx["lr"])
    with torch.no_grad():
        out, again = net(lr), net(lr)
    d = (out.cpu().double() - fx["output_eval"].double()).abs().max().item()
    assert d <= max(1e-4, 3 * fx["out_err32"]), d
    assert torch.equal(out, again)
    net.train()
    assert torch.equal(net(lr).detach(), out)  # the taped forward is the same computation


def _data(shape, r, seed):
    b, n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((b, c, h, w), generator=g) for _ in range(n)], torch.randn((b, c, r * h, r * w), generator=g)


def _make(cls, kw, seed):
    torch.manual_seed(seed)
    return cls(**kw)


def _run_ref(kw, lr, hr, seed, dt):
    m = _make(RBPRef, kw, seed).to(dt).train()
    out = m([t.to(dt) for t in lr])
    torch.nn.functional.l1_loss(out, hr.to(dt)).backward()
    return out.detach().double(), {k: p.grad.double() for k, p in m.named_parameters()}


def _reference(kw, shape, seed):
    """The fp64 run and the restatement's own fp32 error against it: the worst
    over the thread counts 1, 2, 4 and the default, as the fixtures' ref32_err
    (torch's CPU sums change order with the thread count, and a near-cancelling
    slope gradient shows it: one run alone would make the bound depend on the
    host's core count)."""
    lr, hr = _data(shape, kw["upscale_factor"], seed + 1)
    o64, g64 = _run_ref(kw, lr, hr, seed, torch.float64)
    out_err, err = 0.0, {k: 0.0 for k in g64}
    nthreads = torch.get_num_threads()
    try:
        for nt in (1, 2, 4, nthreads):
            torch.set_num_threads(nt)
            o32, g32 = _run_ref(kw, lr, hr, seed, torch.float32)
            out_err = max(out_err, (o32 - o64).abs().max().item())
            for k, v in g64.items():
                err[k] = max(err[k], ((g32[k] - v).norm() / v.norm()).item())
    finally:
        torch.set_num_threads(nthreads)
    return o64, g64, out_err, err


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_matches_restatement_fp32(variant):
    kw, shape = VARIANTS[variant]
    o64, g64, out_err32, ref32_err = _reference(kw, shape, 11)
    lr, hr = _data(shape, kw["upscale_factor"], 12)
    net = _make(nets.RBPNet, kw, 11).to(DEV).set_precision("fp32").train()
    out = net([t.to(DEV) for t in lr])
    torch.nn.functional.l1_loss(out, hr.to(DEV)).backward()
    torch.cuda.synchronize()
    assert out.shape == o64.shape
    d = (out.detach().cpu().double() - o64).abs().max().item()
    print(f"{variant}: out max|d| {d:.2e} (restatement fp32 {out_err32:.2e})")
    assert d <= max(1e-4, 3 * out_err32), d
    bad = []
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        rel = ((p.grad.cpu().double() - g64[k]).norm() / g64[k].norm()).item()
        print(f"  {k}: rel {rel:.2e} (restatement fp32 {ref32_err[k]:.2e})")
        if not rel <= max(1e-4, 3 * ref32_err[k]):
            bad.append((k, rel, ref32_err[k]))
    assert not bad, bad


_LOG_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.conftest import load_golden
from vsr_amd import nets
fx = load_golden("rbp_x2_roll")
torch.manual_seed(fx["seed"])
net = nets.RBPNet(**fx["kwargs"]).to("cuda").set_precision("bf16").eval()
with torch.no_grad():
    net([t.to("cuda") for t in fx["lr"]])
torch.cuda.synchronize()
"""


def test_block_tails_run_on_the_rolling_form():
    """VSRK_LOG_DISPATCH=1 prints one line per conv launch with the path taken
    ("roll": the rolling family) and act=<code>; the block tails are the
    act=3 launches."""
    env = dict(os.environ, VSRK_LOG_DISPATCH="1")
    r = subprocess.run([sys.executable, "-c", _LOG_CHILD.format(root=str(ROOT))], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    tails = [ln for ln in r.stderr.splitlines() if ln.startswith("vsrk_conv_fwd ") and " act=3 " in ln]
    fx = load_golden("rbp_x2_roll")
    kw = fx["kwargs"]
    # res_feat1 and res_feat2 for every neighbour, res_feat3 for all but the last
    want = kw["num_resblocks"] * (3 * (kw["num_frames"] - 1) - 1)
    assert len(tails) == want, (len(tails), want)
    assert all(ln.split()[1] == "roll" for ln in tails), [ln for ln in tails if ln.split()[1] != "roll"]
