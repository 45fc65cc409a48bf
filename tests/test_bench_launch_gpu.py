"""bench.py's own multi-rank launcher: a plain `python bench.py --gpus N` (no WORLD_SIZE in the
environment, the driver's command form) starts the N ranks itself through torch.distributed.run
and relays rank 0's JSON line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launcher_command_without_world_size(monkeypatch):
    """CPU: with WORLD_SIZE unset and --gpus 2 the parent only spawns the launcher child (it never
    reaches a torch.cuda call) and exits with the child's return code."""
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return R()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "2", "--steps", "3"]
    assert cmd[-5].endswith("bench.py")


@pytest.mark.gpu
def test_bench_self_launches_two_ranks(cuda):
    """GPU: `python bench.py --gpus 2 --dist-backend gloo --one-device` (both ranks on this GPU)
    prints one JSON line with n_gpus 2, dp2 and a finite loss."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--dist-backend", "gloo", "--one-device", "--no-cpu-baseline",
           "--no-config5", "--no-sliding", "--no-grouped", "--no-bf16", "--no-dropin", "--no-data", "--no-exchange"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["config"]["global_batch"] == 8
    assert out["value"] > 0 and out["final_loss"] == out["final_loss"]


SIDE_KEYS = ("fwd_ms_per_patch", "sliding_window_256", "config5", "grouped_1gpu", "bf16", "dropin",
             "lesion_256", "patches", "launches_per_step", "exchange", "roofline", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_outputs(cuda, tmp_path, monkeypatch, capsys):
    """GPU: a plain `bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` (in this process)
    prints the headline keys without the --full legs and writes the last step's loss, flat
    parameters and flat gradient as float32 .npy."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                      "--dump-outputs", str(tmp_path / "o")])
    out = bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == out
    assert out["metric"] == bench.METRIC and out["unit"] == "patches/s" and out["dtype"] == "fp32"
    assert out["higher_is_better"] is True and out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / (1000 * 4) - 1) < 1e-3   # bs 4 patches per step
    assert not set(SIDE_KEYS) & set(out)
    got = {f: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(got) == ["grads.npy", "loss.npy", "params.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["loss.npy"].shape == () and abs(float(got["loss.npy"]) - out["final_loss"]) <= 1e-6
    assert got["params.npy"].shape == got["grads.npy"].shape == (217228,)   # the 16->128 model
    assert np.abs(got["grads.npy"]).max() > 0


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    """CPU: dump_outputs writes float32 .npy; an array over its share of the byte budget becomes a
    fixed sample of its elements (the same indices in every call), a smaller one is whole."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 4 * 100)   # 100 elements per array
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    small = torch.arange(6, dtype=torch.bfloat16).reshape(2, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a.max() < 1000   # distinct elements of `big`, in order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3) and np.array_equal(s.ravel(), np.arange(6))


def test_bench_options(monkeypatch, capsys):
    """CPU: --full and --dump-outputs parse; --dump-calls without --full and --steps 0 are
    usage errors."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 5, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--dump-calls", "c.json"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.dump_calls == "c.json"
    for bad in (["--dump-calls", "c.json"], ["--steps", "0"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit) as e:
            bench.parse()
        assert e.value.code == 2
    capsys.readouterr()


def test_paired_call_bytes_are_the_two_calls():
    """CPU: the in-step byte model of a paired GEMM backward launch (l3u_pw_bwd2,
    l3u_pw_bwd_tail_pair) is the sum of the two calls it replaces, so pairing does not move the
    GEMM family's algorithmic bytes."""
    sys.path.insert(0, ROOT)
    import bench
    N, J, S, Ka, Kb = 4, 64, 1728, 64, 32
    p = 1   # any non-null pointer
    one = lambda K, acc: bench.call_bytes(  # noqa: E731
        "l3u_pw_bwd", (p, J * S, None, 0, None, None, 0, p, K * S, p, p, K * S, acc, p, N, J, K, S, p))[2]
    pair = bench.call_bytes("l3u_pw_bwd2", (p, J * S, p, Ka * S, p, p, Ka * S, 0, p, Ka,
                                            p, J * S, p, Kb * S, p, p, Kb * S, 0, p, Kb, N, J, S, p))
    assert pair[0] == "gemm" and pair[2] == one(Ka, 0) + one(Kb, 0)
    J, S, Ka, Kb = 16, 110592, 16, 32
    tail = lambda yr, sel, K, acc: bench.call_bytes(  # noqa: E731
        "l3u_pw_bwd_tail", (p, J * S, p, J * S, yr, J * S, p, p, 4, sel, p, K * S, p, p, K * S, acc, p,
                            N, J, K, S, p))[2]
    args = (p, J * S, None, None, 0, None, 0, 0, p, J * S, p, 4,
            p, J * S, p, p, Ka * S, p, p, Ka * S, 0, p, Ka, 1,
            p, J * S, p, p, Kb * S, p, p, Kb * S, 0, p, Kb, 2, N, J, S, p)
    tp = bench.call_bytes("l3u_pw_bwd_tail_pair", args)
    assert tp[0] == "gemm" and tp[2] == tail(p, 1, Ka, 0) + tail(p, 2, Kb, 0)


def test_reduce_call_bytes(monkeypatch):
    """CPU: the byte model of the weight-gradient reduction launch reads every partial once (fp32,
    fp64 for the InstanceNorm affine partials) and the item table, and per output writes the
    gradient and (the fused AdamW form) reads and writes the parameter and both moments."""
    sys.path.insert(0, ROOT)
    import bench
    items = [[0, 1728, 512, 1, 32, 0, 0, 0], [64, 4, 3, 12, 16, 32, 0, 1]]
    monkeypatch.setattr(bench, "SEG_ITEMS", {99: items})
    f, label, b = bench.call_bytes("l3u_reduce_segments_adamw", (1, 99, 2))
    assert f == "reduce" and "2 items" in label
    assert b == 1728 * 32 * 4 + 4 * 16 * 8 + 2 * 64 + 28 * 48
    assert bench.call_bytes("l3u_reduce_segments", (1, 99, 2))[2] == 1728 * 32 * 4 + 4 * 16 * 8 + 2 * 64 + 4 * 48
    assert bench.call_bytes("l3u_reduce_segments", (1, 98, 2)) is None   # items not recorded
