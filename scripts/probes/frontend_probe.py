"""Time one feed of the streaming log-mel front end: the engine route (compute_rnnt_frontend_feed, two launches) against the
same class on its torch route, on the same GPU in the same process.

    python scripts/probes/frontend_probe.py [--slots 256] [--feeds 60] [--warmup 10]

Per size (1024 and 16000 samples per slot and feed): HIP events around each feed, the median over --feeds feeds after --warmup,
the two routes alternating feed by feed, the audio rotated through several buffers.  The launches per feed are counted with
torch's profiler over one extra feed.  Prints one JSON line per size."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import features  # noqa: E402


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--feeds", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU only"
    pkg.build()
    dev, S = torch.device("cuda:0"), a.slots
    hp = pkg.HParams()
    for n in (1024, 16000):
        routes = {"engine": features.StreamingFrontEnd(hp, 16000, S, n, 2, device=dev, engine=True),
                  "torch": features.StreamingFrontEnd(hp, 16000, S, n, 2, device=dev, engine=False)}
        bufs = [torch.randn(S, n, device=dev) * 0.2 for _ in range(4)]
        k, fin = [n] * S, [False] * S
        times = {r: [] for r in routes}
        for fe in routes.values():
            fe.start(list(range(S)))
        for i in range(a.warmup + a.feeds):
            for r, fe in routes.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fe.feed(bufs[i % len(bufs)], k, fin)
                t1.record()
                t1.synchronize()
                if i >= a.warmup:
                    times[r].append(t0.elapsed_time(t1))
        out = {"slots": S, "samples": n, "feeds": a.feeds}
        for r, fe in routes.items():
            out[r + "_ms_median"] = round(statistics.median(times[r]), 4)
            out[r + "_ms_min"] = round(min(times[r]), 4)
            out[r + "_launches"] = launches(lambda fe=fe: fe.feed(bufs[0], k, fin))
        out["speedup"] = round(out["torch_ms_median"] / out["engine_ms_median"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
