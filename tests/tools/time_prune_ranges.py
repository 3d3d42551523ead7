"""Timings of the band positions (include/rnnt_prune_ranges.h) and of the pruned training objective built on them.  The method of
tests/tools/time_pruned_joint.py: device events, warm-up, alternating rounds, median [min .. max] in milliseconds per call; the
routes of one comparison in the same process and the same rounds.

    python -m tests.tools.time_prune_ranges [--part ranges|objective|all] [--out FILE]

ranges     prune_ranges(ordered=False) -- the torch route, the same on every commit -- against prune_ranges(ordered=True), the
           library's two launches, on the device occupancies of rnnt_loss_simple (3 N(0,1) inputs, V = 28, ragged lengths), and the
           number of live frames on which the two rules give another band position.
objective  PrunedJointLoss (heads + first pass + ranges + fused band joint) forward + backward against JointLoss forward +
           backward on the same enc / pred (N(0,1), freshly initialised weights), with torch.cuda.max_memory_allocated per route in
           a pass of its own.  The number of utterances whose cost is +inf is reported with each route."""
import argparse
import json
import statistics

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg

DEV = "cuda:0"
RANGE_SHAPES = [dict(B=32, T=600, U=150), dict(B=16, T=1500, U=300)]
OBJECTIVE_SHAPES = [dict(B=32, T=600, U=150, J=640, V=28, calls=4), dict(B=16, T=1500, U=300, J=640, V=1024, calls=2),
                    dict(B=16, T=300, U=100, J=640, V=4096, calls=2)]
HIDDEN = 640


def _window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def _time(variants, rounds, calls):
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(_window(fn, calls))
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}


def _lengths(B, T, U, rng):
    il = rng.integers(T // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers(U // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    return il, ll


def run_ranges(cfg):
    B, T, U = cfg["B"], cfg["T"], cfg["U"]
    V = 28
    rng = np.random.default_rng(0)
    il, ll = _lengths(B, T, U, rng)
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    am, lm = 3.0 * torch.randn((B, T, V), device=DEV, generator=g), 3.0 * torch.randn((B, U, V), device=DEV, generator=g)
    rows = {}
    for topo in ("standard", "modified"):
        _, occ = pkg.rnnt_loss_simple(am, lm, labels, t_il, t_ll, topology=topo)
        live = (torch.arange(T, device=DEV)[None, :] < t_il[:, None])
        for S in (5, 64):
            a = pkg.prune_ranges(occ, t_il, t_ll, S, ordered=False)
            b = pkg.prune_ranges(occ, t_il, t_ll, S, ordered=True)
            name = f"B{B} T{T} U{U} S{S} {topo}"
            rows[name] = dict(frames_differ=int(((a != b) & live).sum()), live_frames=int(live.sum()))
            if topo == "standard":
                rows[name].update(_time({"torch (ordered=False)": lambda S=S: pkg.prune_ranges(occ, t_il, t_ll, S, ordered=False),
                                         "library (ordered=True)": lambda S=S: pkg.prune_ranges(occ, t_il, t_ll, S, ordered=True)},
                                        rounds=7, calls=10))
            print(f"ranges {name}: {json.dumps(rows[name])}", flush=True)
    return rows


def run_objective(cfg):
    B, T, U, J, V, calls = (cfg[k] for k in ("B", "T", "U", "J", "V", "calls"))
    rng = np.random.default_rng(0)
    il, ll = _lengths(B, T, U, rng)
    t_il, t_ll = torch.as_tensor(il, device=DEV), torch.as_tensor(ll, device=DEV)
    labels = torch.as_tensor(rng.integers(1, V, size=(B, U - 1)).astype(np.int32), device=DEV)
    torch.manual_seed(0)
    joint = pkg.JointLoss(HIDDEN, J, V).to(DEV)
    pruned = pkg.PrunedJointLoss(HIDDEN, J, V).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    enc = torch.randn((B, T, HIDDEN), device=DEV, generator=g).requires_grad_(True)
    pred = torch.randn((B, U, HIDDEN), device=DEV, generator=g).requires_grad_(True)
    leaves = [enc, pred] + list(joint.parameters()) + list(pruned.parameters())

    def both(route):
        for x in leaves:
            x.grad = None
        costs = route()
        costs.sum().backward()
        return costs

    variants = {"pruned objective forward + backward": lambda: both(lambda: pruned(joint, enc, pred, labels, t_il, t_ll)),
                "full JointLoss forward + backward": lambda: both(lambda: joint(enc, pred, labels, t_il, t_ll))}
    name = f"B{B} T{T} U{U} J{J} V{V}"
    health = {}
    for k, fn in variants.items():  # a band that does not connect (0, 0) to the end costs +inf, legitimately; NaN would be a fault
        costs = fn()
        torch.cuda.synchronize()
        assert not torch.isnan(costs).any(), k
        health[k] = dict(utterances=B, inf_costs=int(torch.isinf(costs).sum()))
    if not torch.isfinite(pruned.last_pruned_costs).all():  # which frame breaks the band: the step out of frame 0 is not limited
        sb = pruned.last_s_begin
        health["pruned objective forward + backward"].update(
            inf_simple=int(torch.isinf(pruned.last_simple_costs).sum()), inf_pruned=int(torch.isinf(pruned.last_pruned_costs).sum()),
            first_step_beyond_band=int((sb[:, 1] > pruned.s_range - 1).sum()))
    rows = _time(variants, rounds=5, calls=calls)
    for k in rows:
        rows[k].update(health[k])
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
        print(f"objective {name} | {k}: {json.dumps(rows[k])}", flush=True)
    return {name: rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["ranges", "objective", "all"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg.build()
    out = {"ranges": {}, "objective": {}}
    if a.part in ("ranges", "all"):
        for cfg in RANGE_SHAPES:
            out["ranges"].update(run_ranges(cfg))
    if a.part in ("objective", "all"):
        for cfg in OBJECTIVE_SHAPES:
            out["objective"].update(run_objective(cfg))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
