"""Timings of forced alignment on the TDT lattice (include/rnnt_tdt_align.h) at B32 T600 U150 V28, durations [0, 1, 2, 3, 4], ragged
lengths, against the forward-only call of compute_rnnt_loss_tdt on the same tensor, measured in the same process.  The method of
tests/tools/time_tdt.py: device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call.

    python -m tests.tools.time_tdt_align [--out FILE]
    python -m tests.tools.time_tdt_align --calls 5      # no timing: a few calls of each route, to run under a kernel trace

The aligner's two halves are timed alone as well: the cell pass (compute_rnnt_tdt_align_cells on all frames) and the sweep with the
back-trace (compute_rnnt_tdt_align_path)."""
import argparse
import ctypes
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib

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


def _routes():
    D = len(DUR)
    rng = np.random.default_rng(0)
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.randn((B, T, U, V + D), device=DEV, generator=g)
    costs, scores = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    frames = torch.empty((B, U - 1), dtype=torch.int32, device=DEV)
    durs = torch.empty((B, U - 1), dtype=torch.int32, device=DEV)
    logp = torch.empty((B, U - 1), device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    loss, al = _lib.load_tdt(), _lib.load_tdtalign()
    ws_loss = torch.empty(_lib.tdt_workspace_bytes(T, U, B, D), dtype=torch.uint8, device=DEV)
    ws = torch.empty(_lib.tdt_align_workspace_bytes(T, U, B, D), dtype=torch.uint8, device=DEV)
    dur = (ctypes.c_int * D)(*DUR)
    out = (frames.data_ptr(), durs.data_ptr(), logp.data_ptr(), scores.data_ptr())
    keep = (acts, labels, t_il, t_ll, ws_loss, ws, frames, durs, logp)

    def loss_forward():
        assert loss.compute_rnnt_loss_tdt(acts.data_ptr(), None, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), None, V, dur, D,
                                          0.0, B, costs.data_ptr(), ws_loss.data_ptr(), opts) == 0

    def align():
        assert al.compute_rnnt_tdt_align(acts.data_ptr(), labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), V, dur, D, 0.0, B, *out,
                                         ws.data_ptr(), opts) == 0

    def cells():
        assert al.compute_rnnt_tdt_align_cells(acts.data_ptr(), T, 0, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), V, dur, D,
                                               0.0, B, ws.data_ptr(), opts) == 0

    def path():
        assert al.compute_rnnt_tdt_align_path(*out, t_ll.data_ptr(), t_il.data_ptr(), dur, D, B, ws.data_ptr(), opts) == 0

    # the sweep without its back-trace: a second workspace from the same logits with every blank at -inf.  No path reaches the
    # terminal (the last edge is a blank), the sweep does the same loads, adds and compares, and the walk back is skipped
    ws_dead = torch.empty_like(ws)
    dead = acts.clone()
    dead[..., 0] = float("-inf")
    assert al.compute_rnnt_tdt_align_cells(dead.data_ptr(), T, 0, labels.data_ptr(), t_ll.data_ptr(), t_il.data_ptr(), V, dur, D, 0.0,
                                           B, ws_dead.data_ptr(), opts) == 0
    torch.cuda.synchronize()
    del dead
    dead_out = [torch.empty_like(x) for x in (frames, durs, logp, scores)]

    def sweep_alone():
        assert al.compute_rnnt_tdt_align_path(*(x.data_ptr() for x in dead_out), t_ll.data_ptr(), t_il.data_ptr(), dur, D, B,
                                              ws_dead.data_ptr(), opts) == 0

    routes = {
        "tdt loss forward (cell pass + sweeps)": loss_forward,
        "tdt align (cell pass + sweep + back-trace)": align,
        "tdt align cell pass": cells,
        "tdt align sweep + back-trace": path,
        "tdt align sweep alone (no path: every blank at -inf, no back-trace)": sweep_alone,
    }
    return routes, (costs, scores, dead_out[3]), keep + (ws_dead,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=0, help="no timing: this many calls of each route (for a kernel trace)")
    a = ap.parse_args()
    pkg.build()
    routes, (costs, scores, dead_scores), _keep = _routes()
    for fn in routes.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    assert torch.isfinite(costs).all() and torch.isfinite(scores).all() and bool((scores <= -costs + 1e-4 * costs.abs()).all())
    assert bool((dead_scores == float("-inf")).all())
    if a.calls:
        for fn in routes.values():
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        return
    times = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, fn in routes.items():
            times[k].append(_window(fn, CALLS))
    rows = {}
    for k, v in times.items():
        rows[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"B{B} T{T} U{U} V{V} D{len(DUR)} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
