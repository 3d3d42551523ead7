"""Timings of the TDT loss op (include/rnnt_tdt.h) at B32 T600 U150 V28, durations [0, 1, 2, 3, 4], against two routes measured in
the same session: compute_rnnt_loss_modified at B32 T600 U150 V33 (the same bytes of logits) and the float64 torch mirror of
rnnt_speech_recognition_amd.tdt run on the device.  The method of profiles/modified_topology_notes.md: device events, warm-up,
alternating rounds, median [min .. max] in milliseconds per call.

    python -m tests.tools.time_tdt [--out FILE] [--no-mirror]
    python -m tests.tools.time_tdt --calls 5          # no timing: a few calls of each library route, to run under a kernel trace

Per kernel: the forward call is the cell pass and the sweeps, the gradient-only call the gradient pass; a kernel trace of --calls
splits the forward."""
import argparse
import ctypes
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, tdt

DEV = "cuda:0"
B, T, U, V = 32, 600, 150, 28
DUR = [0, 1, 2, 3, 4]
ROUNDS, CALLS = 7, 10


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _routes(with_mirror):
    D = len(DUR)
    rng = np.random.default_rng(0)
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.randn((B, T, U, V + D), device=DEV, generator=g)
    grads = torch.empty_like(acts)
    costs, costs_mod = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    lib, mod = _lib.load_tdt(), _lib.load_mod()
    ws = torch.empty(_lib.tdt_workspace_bytes(T, U, B, D), dtype=torch.uint8, device=DEV)
    ws_mod = torch.empty(_lib.modified_workspace_bytes(T, U, B), dtype=torch.uint8, device=DEV)
    dur = (ctypes.c_int * D)(*DUR)

    def call_tdt(gr, cst):
        assert lib.compute_rnnt_loss_tdt(acts.data_ptr(), gr, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), None, V, dur, D, 0.0,
                                         B, cst, ws.data_ptr(), opts) == 0

    def call_mod(gr, cst):  # the same tensor read as V + D = 33 symbols
        assert mod.compute_rnnt_loss_modified(acts.data_ptr(), gr, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), None, V + D, B,
                                              cst, ws_mod.data_ptr(), opts, 0.0) == 0

    routes = {
        "tdt forward (cell pass + sweeps)": lambda: call_tdt(None, costs.data_ptr()),
        "tdt gradient pass": lambda: call_tdt(grads.data_ptr(), None),
        "tdt both": lambda: call_tdt(grads.data_ptr(), costs.data_ptr()),
        "modified V33 forward (cell pass + sweeps)": lambda: call_mod(None, costs_mod.data_ptr()),
        "modified V33 gradient pass": lambda: call_mod(grads.data_ptr(), None),
        "modified V33 both": lambda: call_mod(grads.data_ptr(), costs_mod.data_ptr()),
    }
    slow = {}
    if with_mirror:
        x = acts.clone().requires_grad_(True)

        def mirror():
            x.grad = None
            tdt._mirror(x, labels, t_il, t_ll, tuple(DUR), 0, 0.0).sum().backward()
        slow["float64 torch mirror on the device, both"] = mirror
    return routes, slow, (costs, costs_mod)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-mirror", action="store_true")
    ap.add_argument("--calls", type=int, default=0, help="no timing: this many calls of each library route (for a kernel trace)")
    a = ap.parse_args()
    pkg.build()
    routes, slow, (costs, costs_mod) = _routes(not a.no_mirror and not a.calls)
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(costs).all() and torch.isfinite(costs_mod).all()
    if a.calls:
        for fn in routes.values():
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        return
    times = {k: [] for k in list(routes) + list(slow)}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            times[k].append(_window(fn, CALLS))
    for k, fn in slow.items():
        fn()
        for _ in range(3):
            times[k].append(_window(fn, 1))
    rows = {}
    for k, v in times.items():
        rows[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"B{B} T{T} U{U} V{V} D{len(DUR)} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
