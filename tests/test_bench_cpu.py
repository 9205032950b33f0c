"""bench.py's host-side plumbing (no GPU): the BASELINE configs, their
propagation to spawned ranks, the roofline matchers and the traffic files."""
import argparse
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_configs_cover_the_one_node_baseline_configs():
    assert set(bench.CONFIGS) == {"cfg2", "cfg3", "cfg4", "cfg5"}
    assert bench.CONFIGS["cfg2"]["B"] * bench.CONFIGS["cfg2"]["T"] * 128 * 128 == 1048576
    assert bench.CONFIGS["cfg5"]["precision"] == "fp16" and bench.CONFIGS["cfg5"]["B"] == 8
    assert bench.CONFIGS["cfg3"]["T"] == 30 and bench.CONFIGS["cfg3"]["models"] == "drf"
    # cfg 4: DUF on whole (uncropped) ACDC cine volumes: 256 x 256 HR at 4x
    c4 = bench.CONFIGS["cfg4"]
    assert c4["models"] == "duf" and c4["H"] * 4 == 256 and c4["W"] * 4 == 256 and c4["T"] == 30


def test_apply_config_sets_the_workload():
    args = argparse.Namespace(config="cfg3")
    bench.apply_config(args)
    assert (bench.B, bench.T, bench.DATASET) == (4, 30, "dsb15")
    bench.apply_config(argparse.Namespace(config="cfg4"))
    assert (bench.B, bench.T, bench.H, bench.W) == (2, 30, 64, 64)
    bench.apply_config(argparse.Namespace(config="cfg2"))
    assert (bench.B, bench.T, bench.DATASET, bench.H, bench.W) == (4, 16, "acdc", 128, 128)


class _V:
    def __init__(self, n, d, h, w, c, shuffle=1):
        self.n, self.d, self.h, self.w, self.c, self.shuffle = n, d, h, w, c, shuffle


def test_roofline_matchers_count_the_named_convs():
    m, _ = bench.dominant("edsr")
    assert m(("conv_fwd", (1, 3, 3)), _V(64, 1, 128, 128, 64), _V(64, 1, 128, 128, 64)) == 2 * 64 * 64 * 9 * 64 * 128 * 128
    assert m(("conv_fwd", (1, 3, 3)), _V(64, 1, 128, 128, 64), _V(64, 1, 128, 128, 256)) == 0
    m, _ = bench.dominant("duf")
    x, y = _V(64, 7, 128, 128, 96), _V(64, 7, 128, 128, 32)
    f = m(("conv_fwd", (3, 3, 3)), x, y)
    assert f == 2 * 27 * 96 * 32 * 64 * 7 * 128 * 128
    assert m(("conv_wgrad", (3, 3, 3)), x, y) == f
    assert m(("conv_fwd", (3, 3, 3)), y, x) == f  # data gradient: x = dy (32 channels)


def test_traffic_files_are_per_launch_bytes():
    for model in ("edsr", "duf"):
        t, k = bench._traffic(model, "bf16")
        # the forward roofline kernel: the rolling conv (round 3) or the tile kernel
        assert t is None or (t > 1e8 and k.startswith(("conv_roll_kernel", "conv_fast_kernel")))


def test_every_conv_entry_point_is_timed():
    """The north-star roofline counts the fused data gradients too: every conv
    entry point that can run a roofline kernel launches through timer.wrap
    (conv_reduce / conv_prelu_bwd were not, so the DUF line
    counted 12 of its 18 Conv3d 3x3x3 launches)."""
    import inspect

    from vsr_amd import functional as F
    for fn in (F.conv, F.conv_reduce, F.conv_prelu_bwd, F.conv_wgrad):
        assert "timer.wrap(" in inspect.getsource(fn), fn.__name__


def test_plain_run_times_the_headline_model_only(monkeypatch):
    """Without --full a run sets up and times the config's first model alone;
    --full brings the config's other models back; named models run as named."""
    monkeypatch.delenv("VSR_BENCH_MODELS", raising=False)
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (plain.models, plain.full, plain.steps, plain.warmup, plain.dump_outputs) == ("edsr", False, 7, 2, None)
    assert bench.parse_args(["--full"]).models == "edsr,duf"
    assert bench.parse_args(["--config", "cfg3"]).models == "drf"
    assert bench.parse_args(["--config", "cfg5", "--full"]).models == "edsr,duf"
    assert bench.parse_args(["--models", "edsr,duf"]).models == "edsr,duf"
    assert bench.parse_args(["--model", "duf", "--dump-outputs", "d"]).models == "duf"


def test_dump_array_is_whole_or_a_fixed_sample(tmp_path):
    import numpy as np
    import torch
    t = torch.arange(1000, dtype=torch.bfloat16).reshape(10, 100) / 8
    bench._dump_array(tmp_path / "whole.npy", t, 1000)
    whole = np.load(tmp_path / "whole.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, t.float().reshape(-1).numpy())
    bench._dump_array(tmp_path / "a.npy", t, 64)
    bench._dump_array(tmp_path / "b.npy", t + 0, 64)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == np.float32 and a.shape == (64,) and np.array_equal(a, b)
    assert set(a.tolist()) <= set(whole.tolist())
    # the sample has no index twice, keeps the array's order and reaches over the whole of it
    f = torch.arange(1000, dtype=torch.float32)
    bench._dump_array(tmp_path / "f.npy", f, 64)
    picked = np.load(tmp_path / "f.npy")
    assert len(set(picked.tolist())) == 64 and np.array_equal(picked, np.sort(picked)) and picked.max() > 500


def test_dump_outputs_names_and_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    net = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))
    frozen = torch.nn.Parameter(torch.zeros(3))  # no gradient: left out of grads / params
    net.register_parameter("frozen", frozen)
    out = net(torch.ones(5, 8))
    loss = out.abs().mean()
    loss.backward()
    bench.dump_outputs(tmp_path / "d", "edsr", 1, loss, out, net)
    got = {p.name: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["edsr_grads.npy", "edsr_loss.npy", "edsr_out.npy", "edsr_params.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["edsr_loss.npy"].shape == (1,) and got["edsr_out.npy"].shape == (20,)
    n = sum(p.numel() for p in net.parameters()) - 3
    assert got["edsr_grads.npy"].shape == (n,) and got["edsr_params.npy"].shape == (n,)
    assert np.array_equal(got["edsr_params.npy"][:64], net[0].weight.detach().reshape(-1).numpy())
    # a frame list (DRF) under a budget smaller than the arrays: every file is a sample, the sum stays inside
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 64)
    bench.dump_outputs(tmp_path / "l", "drf", 2, loss, [out, out * 2], net)
    files = sorted((tmp_path / "l").iterdir())
    assert [p.name for p in files] == ["drf_grads.npy", "drf_loss.npy", "drf_out_00.npy", "drf_out_01.npy",
                                      "drf_params.npy"]
    assert sum(np.load(p).size for p in files) * 4 <= 4 * 64 // 2
