"""Time forced alignment: the engine (compute_rnnt_align / align_joint over the library) against the same function on its torch
route (alignment._torch_cells / _torch_path on device tensors) on the same GPU in the same process, with compute_rnnt_loss_fwd
at the same shape as a yardstick.

    python scripts/probes/align_probe.py [--iters 20] [--warmup 3] [--shapes c1,c4,fused] [--engine-only]

Shapes: c1 = BASELINE configs[1] (B32 T600 U150 V28), c4 = configs[4]'s lattice on materialised logits (B16 T1500 U300 V1024),
fused = the slab route at the reference's default vocabulary (B16 T300 U100 V4096, H = J = 640).  HIP events around every call,
medians after warm-up, the routes alternating call by call, the inputs rotated through several buffers.  --engine-only runs the
engine alone (for a `rocprofv3 --kernel-trace --stats` run of its own: the cell kernel and the sweep / back-trace separately).
Prints one JSON line per shape; `cell_algo_bytes` is what the cell pass must move (4 V bytes in, 8 out per lattice cell)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import alignment  # noqa: E402

SHAPES = {"c1": (32, 600, 150, 28), "c4": (16, 1500, 300, 1024), "fused": (16, 300, 100, 4096)}


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def summary(name, xs, out):
    xs = sorted(xs)
    out[name + "_ms_median"] = round(statistics.median(xs), 4)
    out[name + "_ms_min"] = round(xs[0], 4)
    out[name + "_ms_max"] = round(xs[-1], 4)


def torch_align(acts, labels, il, ll):
    lpb, lpl = alignment._torch_cells(acts, labels, 0)
    return alignment._torch_path(lpb, lpl, il, ll)


def torch_align_joint(joint, enc, pred, labels, il, ll, S):
    parts = [alignment._torch_cells(joint.logits(enc[:, t0:t0 + S], pred), labels, 0) for t0 in range(0, enc.shape[1], S)]
    return alignment._torch_path(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), il, ll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="c1,c4,fused")
    ap.add_argument("--engine-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    pkg.build()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    for name in a.shapes.split(","):
        B, T, U, V = SHAPES[name]
        labels = torch.randint(1, V, (B, U - 1), generator=g, device=dev, dtype=torch.int32)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        ll = torch.full((B,), U - 1, dtype=torch.int32, device=dev)
        out = {"shape": name, "B": B, "T": T, "U": U, "V": V, "iters": a.iters,
               "cell_algo_bytes": B * T * U * (4 * V + 8)}
        if name == "fused":
            joint = pkg.JointLoss(640, 640, V).to(dev)
            bufs = [(torch.randn(B, T, 640, generator=g, device=dev), torch.randn(B, U, 640, generator=g, device=dev))
                    for _ in range(4)]
            S = alignment.slab_frames_for(B, T, U, V)
            out["slab_frames"] = S
            routes = {"engine": lambda x: pkg.align_joint(joint, x[0], x[1], labels, il, ll),
                      "torch": lambda x: torch_align_joint(joint, x[0], x[1], labels, il, ll, S),
                      "loss_fwd": lambda x: joint(x[0], x[1], labels, il, ll)}
        else:
            nbuf = 2 if B * T * U * V * 4 > (8 << 30) else 4
            bufs = [torch.randn(B, T, U, V, generator=g, device=dev) for _ in range(nbuf)]
            routes = {"engine": lambda x: pkg.rnnt_align(x, labels, il, ll),
                      "torch": lambda x: torch_align(x, labels, il, ll),
                      "loss_fwd": lambda x: pkg.rnnt_loss(x, labels, il, ll)}
        if a.engine_only:
            routes = {"engine": routes["engine"]}
        times = {r: [] for r in routes}
        with torch.no_grad():
            for i in range(a.warmup + a.iters):
                for r, fn in routes.items():
                    ms = timed(lambda: fn(bufs[i % len(bufs)]))
                    if i >= a.warmup:
                        times[r].append(ms)
        for r in routes:
            summary(r, times[r], out)
        if not a.engine_only:
            out["speedup_vs_torch"] = round(out["torch_ms_median"] / out["engine_ms_median"], 2)
            out["ratio_to_loss_fwd"] = round(out["engine_ms_median"] / out["loss_fwd_ms_median"], 2)
            spread = (out["engine_ms_max"] - out["engine_ms_min"]) + (out["torch_ms_max"] - out["torch_ms_min"])
            out["bar_met"] = bool(out["torch_ms_median"] - out["engine_ms_median"] > spread)
        print(json.dumps(out), flush=True)
        del bufs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
