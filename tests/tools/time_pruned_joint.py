"""Timings and peak memory of the fused joint on the pruned band (include/rnnt_pruned_joint.h) against the route a caller has
without it: prune_joint_inputs -> torch.tanh(a + p) @ W2 + b2 -> rnnt_loss_pruned, forward and forward + backward.  The method of
tests/tools/time_simple.py: device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call; both routes in
the same process and the same rounds.  torch.cuda.max_memory_allocated is taken per route in a pass of its own, after the timings.

    python -m tests.tools.time_pruned_joint [--shape small|mid|large|all] [--out FILE]

Both routes' costs and gradients are compared once per shape and lattice at the sizes timed (printed as max differences)."""
import argparse
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg

DEV = "cuda:0"
SHAPES = {"small": dict(B=32, T=600, U=150, S=5, J=640, V=28, rounds=7, calls=10),
          "mid": dict(B=32, T=600, U=150, S=5, J=512, V=500, rounds=5, calls=4),
          "large": dict(B=16, T=1500, U=300, S=5, J=640, V=1024, rounds=5, calls=2)}


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run_shape(name, cfg):
    B, T, U, S, J, V = (cfg[k] for k in "BTUSJV")
    rng = np.random.default_rng(0)
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    # a straight-line band from (0, 0) to (T_b - 1, L_b + 1 - S): steps of 0 and 1, connected on both lattices
    sb = np.zeros((B, T), np.int32)
    for b in range(B):
        hi = max(0, int(ll[b]) + 1 - S)
        sb[b] = np.minimum((np.arange(T) * hi) // max(int(il[b]) - 1, 1), hi)
    t_il, t_ll, t_sb = (torch.as_tensor(a, device=DEV) for a in (il, ll, sb))
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    lim = float(np.sqrt(6.0 / (J + V)))
    data = [torch.randn((B, T, J), device=DEV, generator=g), torch.randn((B, U, J), device=DEV, generator=g),
            (torch.rand((J, V), device=DEV, generator=g) * 2 - 1) * lim, 0.1 * torch.randn((V,), device=DEV, generator=g)]
    leaves = [x.clone().requires_grad_(True) for x in data]

    def fused(topo):
        return pkg.rnnt_joint_loss_pruned(*leaves, t_sb, labels, t_il, t_ll, topology=topo, s_range=S)

    def composed(topo):
        e, p, W, bias = leaves
        a, q = pkg.prune_joint_inputs(e, p, t_sb, S)
        return pkg.rnnt_loss_pruned(torch.tanh(a + q) @ W + bias, t_sb, labels, t_il, t_ll, topology=topo)

    def forward(route, topo):
        with torch.no_grad():
            return route(topo)

    def both(route, topo):
        for x in leaves:
            x.grad = None
        costs = route(topo)
        costs.sum().backward()
        return costs

    variants = {}
    for topo in ("standard", "modified"):
        for rname, route in (("fused", fused), ("composed (prune_joint_inputs + torch joint + rnnt_loss_pruned)", composed)):
            variants[f"{rname} {topo} forward"] = lambda route=route, topo=topo: forward(route, topo)
            variants[f"{rname} {topo} forward + backward"] = lambda route=route, topo=topo: both(route, topo)
    rows = {}
    for topo in ("standard", "modified"):  # the two routes compute the same thing, at the sizes timed
        res = {}
        for rname, route in (("fused", fused), ("composed", composed)):
            costs = both(route, topo)
            torch.cuda.synchronize()
            assert torch.isfinite(costs).all()
            res[rname] = [costs.detach().clone()] + [x.grad.clone() for x in leaves]
        diff = [float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(res["fused"], res["composed"])]
        rows[f"agreement {topo}"] = dict(zip(("costs", "d_enc", "d_pred", "dW2", "db2"), diff))
        print(f"{name} | fused against composed, {topo}: max |difference| / max(1, max |composed|) = {rows[f'agreement {topo}']}", flush=True)
        del res
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(cfg["rounds"]):
        for k, fn in variants.items():
            times[k].append(_window(fn, cfg["calls"]))
    for k, v in times.items():
        rows[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{name} B{B} T{T} U{U} S{S} J{J} V{V} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    for x in leaves:
        x.grad = None
    for k, fn in variants.items():  # peak memory of one call above what the inputs occupy
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        rows[k]["peak_MiB_above_inputs"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for x in leaves:
            x.grad = None
        print(f"{name} | {k}: peak {rows[k]['peak_MiB_above_inputs']:.1f} MiB above the inputs", flush=True)
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
