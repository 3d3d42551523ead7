"""Time forced alignment on the modified (one symbol per frame) lattice: the engine (compute_rnnt_modified_align) against the
standard-lattice engine of the same build (compute_rnnt_align) and against the modified route's torch mirror
(alignment._torch_cells / _torch_path_modified on device tensors), on the same GPU in the same process.

    python scripts/probes/modified_align_probe.py [--iters 20] [--warmup 3] [--shapes c1,c4] [--engine-only]

Shapes: c1 = BASELINE configs[1] (B32 T600 U150 V28), c4 = configs[4]'s lattice on materialised logits (B16 T1500 U300 V1024).
HIP events around every call, medians after warm-up, the routes alternating call by call, the inputs rotated through several
buffers (the method of scripts/probes/align_probe.py).  --engine-only runs the two engines alone (for a
`rocprofv3 --kernel-trace --stats` run of its own).  Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import alignment  # noqa: E402

SHAPES = {"c1": (32, 600, 150, 28), "c4": (16, 1500, 300, 1024)}


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


def torch_align_modified(acts, labels, il, ll):
    lpb, lpl = alignment._torch_cells(acts, labels, 0)
    return alignment._torch_path_modified(lpb, lpl, il, ll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-iters", type=int, default=5)
    ap.add_argument("--shapes", default="c1,c4")
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
        out = {"shape": name, "B": B, "T": T, "U": U, "V": V, "iters": a.iters, "cell_algo_bytes": B * T * U * (4 * V + 8)}
        nbuf = 2 if B * T * U * V * 4 > (8 << 30) else 4
        bufs = [torch.randn(B, T, U, V, generator=g, device=dev) for _ in range(nbuf)]
        routes = {"modified": lambda x: pkg.rnnt_align(x, labels, il, ll, topology="modified"),
                  "standard": lambda x: pkg.rnnt_align(x, labels, il, ll)}
        if not a.engine_only:
            routes["torch_modified"] = lambda x: torch_align_modified(x, labels, il, ll)
        times = {r: [] for r in routes}
        with torch.no_grad():
            for i in range(a.warmup + a.iters):
                for r, fn in routes.items():
                    if r == "torch_modified" and i >= a.warmup + a.torch_iters:
                        continue  # (hundreds of milliseconds a call: fewer of them)
                    ms = timed(lambda: fn(bufs[i % len(bufs)]))
                    if i >= a.warmup:
                        times[r].append(ms)
        for r in routes:
            summary(r, times[r], out)
        out["modified_over_standard"] = round(out["modified_ms_median"] / out["standard_ms_median"], 3)
        if not a.engine_only:
            out["speedup_vs_torch"] = round(out["torch_modified_ms_median"] / out["modified_ms_median"], 2)
        print(json.dumps(out), flush=True)
        del bufs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
