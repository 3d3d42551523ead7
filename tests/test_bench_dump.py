"""bench.py --dump-outputs: the last timed step's costs and gradients land in DIR as f32 .npy files within the 64 MB
budget (a fixed sample of lattice cells when the gradients are larger), and they are what the op computes on the bench's
seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_fits_the_budget_and_samples_the_same_cells_every_time(tmp_path):
    B, T, U, V = 2, 300, 150, 200  # 72 MB of gradients: over the budget
    g = torch.randn(B, T, U, V)
    c = torch.randn(B)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), c, g)
    files = _files(tmp_path / "a")
    assert list(files) == ["costs.npy", "grads_sample.npy"] and sum(files.values()) <= bench.DUMP_BUDGET_BYTES
    s = np.load(tmp_path / "a" / "grads_sample.npy")
    assert s.dtype == np.float32 and s.shape[1] == V and s.shape[0] > 0
    assert np.array_equal(s, np.load(tmp_path / "b" / "grads_sample.npy"))
    pick = np.sort(np.random.default_rng(0).choice(B * T * U, s.shape[0], replace=False))
    assert np.array_equal(s, g.reshape(-1, V).numpy()[pick])
    assert np.array_equal(np.load(tmp_path / "a" / "costs.npy"), c.numpy())


def test_dump_writes_small_gradients_whole(tmp_path):
    g = torch.randn(2, 5, 4, 28)
    bench.dump_outputs(str(tmp_path), torch.randn(2), g)
    assert list(_files(tmp_path)) == ["costs.npy", "grads.npy"]
    assert np.array_equal(np.load(tmp_path / "grads.npy"), g.numpy())


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "x", "--engine", "stub"],
                                  ["--dump-outputs", "x", "--fused-only", "16,1500,300,1024"]])
def test_bench_refuses_arguments_it_cannot_honour(argv):
    with pytest.raises(SystemExit):
        bench.parse(argv)


@pytest.mark.gpu
def test_dumped_outputs_are_the_last_timed_step_of_the_op(tmp_path):
    from oracle import rnnt_oracle as orc

    B, T, U, V, rotate, steps = 2, 40, 12, 28, 2, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shape", f"{B},{T},{U},{V}", "--rotate", str(rotate),
                        "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline", "--no-fused", "--no-ragged", "--no-e2e",
                        "--no-config5", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == steps
    # bench.py's inputs: a ring of `rotate` logits tensors, then the labels, from one CPU generator seeded 1234 (rank 0)
    g = torch.Generator().manual_seed(1234)
    ring = [torch.randn(B, T, U, V, generator=g) for _ in range(rotate)]
    labels = torch.randint(1, V, (B, U - 1), generator=g, dtype=torch.int32).numpy()
    c_ref, g_ref = orc.rnnt_loss_and_grad(ring[(steps - 1) % rotate].numpy(), labels, [T] * B, [U - 1] * B)
    costs, grads = np.load(tmp_path / "costs.npy"), np.load(tmp_path / "grads.npy")
    assert costs.dtype == grads.dtype == np.float32 and grads.shape == (B, T, U, V)
    assert np.abs(costs - c_ref).max() <= 1e-4 * np.abs(c_ref).max()
    assert np.abs(grads - g_ref / B).max() <= 1e-4  # cost_scale = 1 / global batch
