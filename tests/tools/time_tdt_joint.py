"""Timings and peak memory of the fused TDT joint (include/rnnt_tdt_joint.h) against the route a caller has without it: the joint in
torch producing the logits [B, T, U, V + D], then rnnt_loss_tdt, forward and forward + backward through both.  The method of
tests/tools/time_pruned_joint.py: device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call; both
routes in the same process and the same rounds.  Every call takes the next of a ring of input sets, so no call finds the previous
call's inputs in cache.  torch.cuda.max_memory_allocated is taken per route in a pass of its own, after the timings.

    python -m tests.tools.time_tdt_joint [--shape headline|wordpiece|all] [--kernels] [--out FILE]

Both routes' costs and gradients are compared once per shape at the sizes timed (printed as max differences).  --kernels: the
device time of every kernel of one fused forward + backward, from torch.profiler."""
import argparse
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg

DEV = "cuda:0"
DUR = [0, 1, 2, 3, 4]
SHAPES = {"headline": dict(B=32, T=600, U=150, J=640, V=28, rounds=5, calls=3, sets=3),
          "wordpiece": dict(B=16, T=300, U=75, J=640, V=1024, rounds=5, calls=3, sets=3)}


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def run_shape(name, cfg, kernels=False):
    B, T, U, J, V = (cfg[k] for k in "BTUJV")
    R = V + len(DUR)
    rng = np.random.default_rng(0)
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    lim = float(np.sqrt(6.0 / (J + R)))
    ring = []
    for _ in range(cfg["sets"]):
        data = [torch.randn((B, T, J), device=DEV, generator=g), torch.randn((B, U, J), device=DEV, generator=g),
                (torch.rand((J, R), device=DEV, generator=g) * 2 - 1) * lim, 0.1 * torch.randn((R,), device=DEV, generator=g)]
        ring.append([x.requires_grad_(True) for x in data])
    turn = [0]

    def leaves():
        turn[0] = (turn[0] + 1) % len(ring)
        return ring[turn[0]]

    def fused(x):
        return pkg.rnnt_joint_loss_tdt(*x, labels, t_il, t_ll, DUR)

    def composed(x):
        e, p, W, bias = x
        return pkg.rnnt_loss_tdt(torch.tanh(e[:, :, None, :] + p[:, None, :, :]) @ W + bias, labels, t_il, t_ll, DUR)

    def forward(route):
        with torch.no_grad():
            return route(leaves())

    def both(route, x=None):
        x = leaves() if x is None else x
        for v in x:
            v.grad = None
        costs = route(x)
        costs.sum().backward()
        return costs

    variants = {}
    for rname, route in (("fused", fused), ("composed (torch joint + rnnt_loss_tdt)", composed)):
        variants[f"{rname} forward"] = lambda route=route: forward(route)
        variants[f"{rname} forward + backward"] = lambda route=route: both(route)
    rows, res = {}, {}
    for rname, route in (("fused", fused), ("composed", composed)):  # the two routes compute the same thing, at the sizes timed
        costs = both(route, ring[0])
        torch.cuda.synchronize()
        assert torch.isfinite(costs).all()
        res[rname] = [costs.detach().clone()] + [x.grad.clone() for x in ring[0]]
    diff = [float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(res["fused"], res["composed"])]
    rows["agreement"] = dict(zip(("costs", "d_enc", "d_pred", "dW2", "db2"), diff))
    print(f"{name} | fused against composed: max |difference| / max(1, max |composed|) = {rows['agreement']}", flush=True)
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
        print(f"{name} B{B} T{T} U{U} J{J} V{V} D{len(DUR)} | {k}: {rows[k]['median']:.4f} [{rows[k]['min']:.4f} .. {rows[k]['max']:.4f}]", flush=True)
    for x in ring:
        for v in x:
            v.grad = None
    for k, fn in variants.items():  # peak memory of one call above what the inputs occupy
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        rows[k]["peak_MiB_above_inputs"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for x in ring:
            for v in x:
                v.grad = None
        print(f"{name} | {k}: peak {rows[k]['peak_MiB_above_inputs']:.1f} MiB above the inputs", flush=True)
    if kernels:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            both(fused)
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
            if t > 0:
                split[ev.key] = dict(ms=t / 1e3, calls=ev.count)
        rows["fused forward + backward kernels"] = split
        for k, v in sorted(split.items(), key=lambda kv: -kv[1]["ms"]):
            print(f"{name} | kernel {k[:90]}: {v['ms']:.4f} ms in {v['calls']} launch(es)", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg.build()
    out = {}
    for name, cfg in SHAPES.items():
        if a.shape in (name, "all"):
            out[name] = run_shape(name, cfg, a.kernels)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
