"""Timings of the CTC loss op (include/rnnt_ctc.h compute_rnnt_ctc_loss, forward + gradients) against what a caller has without
it: torch.nn.functional.ctc_loss forward + backward on the same device in the same session.  The method of
profiles/modified_topology_notes.md: device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call.
The per-kernel split of the op comes from the torch profiler's device activities (kernel names holding "ctc_"), in a pass of its own.

    python -m tests.tools.time_ctc [--shape small|wide|long|all] [--out FILE]"""
import argparse
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import ctc_cases as cc

DEV = "cuda:0"
SHAPES = {"small": dict(B=32, T=600, L=150, V=28, rounds=7, calls=10), "wide": dict(B=32, T=300, L=100, V=4096, rounds=7, calls=10),
          "long": dict(B=16, T=1500, L=300, V=1024, rounds=5, calls=4)}


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _kernel_split(fn, calls):
    """{kernel name: mean device milliseconds per call} of the op's own kernels, or None where the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            if "ctc_" in e.key:
                us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                name = e.key.split("(")[0].split("::")[-1]
                rows[name] = rows.get(name, 0.0) + us / 1000.0 / calls
        return rows or None
    except Exception as e:  # noqa: BLE001 -- a tool: report and go on
        print("kernel split not available:", e)
        return None


def run_shape(name, cfg):
    B, T, L, V = cfg["B"], cfg["T"], cfg["L"], cfg["V"]
    rng = np.random.default_rng(0)
    il = rng.integers(3 * T // 4, T + 1, size=B).astype(np.int32)
    ll = rng.integers(L // 2, L + 1, size=B).astype(np.int32)
    il[0], ll[0] = T, L
    labels_np = np.stack([cc.random_labels(rng, L, V, repeat_prob=0.1) for _ in range(B)])
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(labels_np, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.randn((B, T, V), device=DEV, generator=g)
    grads = torch.empty_like(acts)
    costs = torch.empty(B, device=DEV)
    lib = _lib.load_ctc()
    ws = torch.empty(_lib.ctc_workspace_bytes(T, L + 1, B), dtype=torch.uint8, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, L + 1)

    def call(gp, cp):
        assert lib.compute_rnnt_ctc_loss(acts.data_ptr(), gp, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), None, V, B, cp,
                                         ws.data_ptr(), opts) == 0

    x = acts.clone().requires_grad_(True)
    il64, ll64, lab64 = t_il.long(), t_ll.long(), labels.long()

    def torch_both():
        x.grad = None
        lp = torch.log_softmax(x, dim=2).transpose(0, 1)
        torch.nn.functional.ctc_loss(lp, lab64, il64, ll64, blank=0, reduction="sum", zero_infinity=True).backward()

    def torch_fwd():
        with torch.no_grad():
            torch.nn.functional.ctc_loss(torch.log_softmax(acts, dim=2).transpose(0, 1), lab64, il64, ll64, blank=0, reduction="sum")

    variants = {"ctc forward": lambda: call(None, costs.data_ptr()), "ctc gradient pass": lambda: call(grads.data_ptr(), None),
                "ctc both": lambda: call(grads.data_ptr(), costs.data_ptr()),
                "torch ctc_loss forward": torch_fwd, "torch ctc_loss forward + backward": torch_both}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(costs).all()
    times = {k: [] for k in variants}
    for _ in range(cfg["rounds"]):
        for k, fn in variants.items():
            times[k].append(_window(fn, cfg["calls"]))
    rows = {}
    for k, v in times.items():
        rows[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{name} B{B} T{T} L{L} V{V} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    rows["ratio torch / ctc, forward + backward"] = rows["torch ctc_loss forward + backward"]["median"] / rows["ctc both"]["median"]
    print(f"{name} | torch / ctc (both): {rows['ratio torch / ctc, forward + backward']:.2f}", flush=True)
    split = _kernel_split(variants["ctc both"], cfg["calls"])
    if split:
        rows["kernels"] = split
        for k, v in sorted(split.items()):
            print(f"{name} | kernel {k}: {v:.4f} ms per call", flush=True)
        sweep = sum(v for k, v in split.items() if "sweep" in k)
        if sweep:
            rows["sweep microseconds per frame"] = 1000.0 * sweep / T
            print(f"{name} | sweeps: {rows['sweep microseconds per frame']:.3f} us per frame (T = {T} serial steps)", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg.build()
    out = {}
    for name, cfg in SHAPES.items():
        if a.shape in (name, "all"):
            out[name] = run_shape(name, cfg)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
