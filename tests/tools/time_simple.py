"""Timings of the simple loss op (include/rnnt_simple.h) against the route a caller has without it: am[:, :, None] + lm[:, None]
materialised in torch, then rnnt_loss of the same topology with its autograd.  The method of profiles/modified_topology_notes.md:
device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call.

    python -m tests.tools.time_simple [--shape small|mid|large|all] [--out FILE]

The comparison route is skipped (and reported as such) where its [B, T, U, V] tensors do not fit in the device's free memory."""
import argparse
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib

DEV = "cuda:0"
SHAPES = {"small": dict(B=32, T=600, U=150, V=28, rounds=7, calls=20), "mid": dict(B=32, T=600, U=150, V=512, rounds=5, calls=4),
          "large": dict(B=16, T=1500, U=300, V=1024, rounds=5, calls=2)}


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run_shape(name, cfg):
    B, T, U, V = cfg["B"], cfg["T"], cfg["U"], cfg["V"]
    rng = np.random.default_rng(0)
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    am = torch.randn((B, T, V), device=DEV, generator=g)
    lm = torch.randn((B, U, V), device=DEV, generator=g)
    g_am, g_lm = torch.empty_like(am), torch.empty_like(lm)
    occ = torch.empty((B, T, U), device=DEV)
    costs = torch.empty(B, device=DEV)
    lib = _lib.load_simple()
    ws = torch.empty(_lib.simple_workspace_bytes(T, U, B), dtype=torch.uint8, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    variants = {}
    for topo, tid in (("standard", 0), ("modified", 1)):
        def call(ga, gl, cst, tid=tid):
            st = lib.compute_rnnt_loss_simple(am.data_ptr(), lm.data_ptr(), ga, gl, occ.data_ptr() if cst else None, labels.data_ptr(),
                                              t_ll.data_ptr(), t_il.data_ptr(), None, V, B, tid, 0.0, 0.0, cst, ws.data_ptr(), opts)
            assert st == 0
        variants[f"simple {topo} forward"] = lambda call=call: call(None, None, costs.data_ptr())
        variants[f"simple {topo} gradient pass"] = lambda call=call: call(g_am.data_ptr(), g_lm.data_ptr(), None)
        variants[f"simple {topo} both"] = lambda call=call: call(g_am.data_ptr(), g_lm.data_ptr(), costs.data_ptr())
    # the materialised route: the sum, its gradient and the op's workspace, about 3.5 tensors of [B, T, U, V] float32
    need = int(3.5 * 4 * B * T * U * V)
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    skipped = need > free
    if not skipped:
        x, y = am.clone().requires_grad_(True), lm.clone().requires_grad_(True)
        for topo in ("standard", "modified"):
            def fwd(topo=topo):
                with torch.no_grad():
                    pkg.rnnt_loss(am[:, :, None, :] + lm[:, None, :, :], labels, t_il, t_ll, topology=topo)

            def both(topo=topo):
                x.grad = y.grad = None
                pkg.rnnt_loss(x[:, :, None, :] + y[:, None, :, :], labels, t_il, t_ll, topology=topo).sum().backward()
            variants[f"materialised sum + rnnt_loss {topo} forward"] = fwd
            variants[f"materialised sum + rnnt_loss {topo} both"] = both
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
        print(f"{name} B{B} T{T} U{U} V{V} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    if skipped:
        print(f"{name} B{B} T{T} U{U} V{V} | materialised sum + rnnt_loss: does not fit ({need / 2**30:.1f} GiB needed, {free / 2**30:.1f} free)", flush=True)
        rows["materialised sum + rnnt_loss"] = "does not fit in memory"
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
