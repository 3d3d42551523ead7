"""What FastEmit costs per step: lambda = 0 against lambda = 0.01 through the C ABI, device-event times, for
  * the loss op at BASELINE.json configs[1] (B32 T600 U150 V28, N(0,1) logits, full lengths): compute_rnnt_loss_fastemit;
  * the f32-grade fused joint at the same lattice (joint size 640): compute_rnnt_joint_loss_fwd + _bwd_fastemit;
  * the f16 fused joint at B16 T300 U100 J640 V4096: the same pair of calls with joint_dtype 1.
lambda = 0 launches the plain instantiations of the kernels, lambda > 0 the FastEmit ones: the difference is expected to be one
multiply-add per lattice cell.  A report, not a gate.  Needs an MI355X.

    python tests/tools/time_fastemit.py [--steps 20] [--warmup 5] [--out time_fastemit.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import _lib  # noqa: E402

DEV = "cuda:0"


def timed(fn, steps, warmup):
    """Median / min / max over `steps` calls of fn(), milliseconds, one event pair per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def op_case(lib, B, T, U, V, steps, warmup):
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.randn(B, T, U, V, device=DEV, generator=g)
    labels = torch.randint(1, V, (B, U - 1), device=DEV, generator=g, dtype=torch.int32)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ll = torch.full((B,), U - 1, dtype=torch.int32, device=DEV)
    grads, costs = torch.empty_like(acts), torch.empty(B, device=DEV)
    ws = torch.empty(_lib.workspace_bytes(T, U, B), dtype=torch.uint8, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)

    def call(lam):
        st = lib.compute_rnnt_loss_fastemit(acts.data_ptr(), grads.data_ptr(), labels.data_ptr(), ll.data_ptr(), il.data_ptr(), None,
                                            V, B, costs.data_ptr(), ws.data_ptr(), opts, 0, lam)
        assert st == 0, st

    return {f"lambda_{lam:g}": timed(lambda: call(lam), steps, warmup) for lam in (0.0, 0.01)} | \
           {f"lambda_{lam:g}_again": timed(lambda: call(lam), steps, warmup) for lam in (0.0, 0.01)}


def joint_case(lib, B, T, U, J, V, dtype, steps, warmup):
    g = torch.Generator(device=DEV).manual_seed(1)
    ep = torch.randn(B, T, J, device=DEV, generator=g)
    pp = torch.randn(B, U, J, device=DEV, generator=g)
    lim = float(np.sqrt(6.0 / (J + V)))
    W2 = (torch.rand(J, V, device=DEV, generator=g) * 2 - 1) * lim
    b2 = torch.zeros(V, device=DEV)
    labels = torch.randint(1, V, (B, U - 1), device=DEV, generator=g, dtype=torch.int32)
    il = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ll = torch.full((B,), U - 1, dtype=torch.int32, device=DEV)
    outs = [torch.empty_like(x) for x in (ep, pp, W2, b2)]
    costs = torch.empty(B, device=DEV)
    ws = torch.empty(_lib.joint_workspace_bytes(T, U, B, J, V), dtype=torch.uint8, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    head = [x.data_ptr() for x in (ep, pp, W2, b2, labels, ll, il)]

    def call(lam):
        st = lib.compute_rnnt_joint_loss_fwd(*head, J, V, B, costs.data_ptr(), dtype, ws.data_ptr(), opts)
        assert st == 0, st
        st = lib.compute_rnnt_joint_loss_bwd_fastemit(*head, None, J, V, B, *[o.data_ptr() for o in outs], dtype, ws.data_ptr(), opts, lam)
        assert st == 0, st

    return {f"lambda_{lam:g}": timed(lambda: call(lam), steps, warmup) for lam in (0.0, 0.01)} | \
           {f"lambda_{lam:g}_again": timed(lambda: call(lam), steps, warmup) for lam in (0.0, 0.01)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fastemit: needs an MI355X (no CPU fallback)")
    pkg.build()
    lib = _lib.load()
    res = {
        "op_B32_T600_U150_V28": op_case(lib, 32, 600, 150, 28, a.steps, a.warmup),
        "joint_f32_B32_T600_U150_J640_V28": joint_case(lib, 32, 600, 150, 640, 28, 0, max(3, a.steps // 2), max(2, a.warmup // 2)),
        "joint_f16_B16_T300_U100_J640_V4096": joint_case(lib, 16, 300, 100, 640, 4096, 1, max(3, a.steps // 2), max(2, a.warmup // 2)),
    }
    for k, v in res.items():
        print(k, json.dumps(v))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
