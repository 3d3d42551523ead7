"""Wall time of training through the LSTM layers on an MI355X: lstm="torch" (nn.LSTM) against lstm="engine" (the library's
forward and BPTT step kernels, lstm.LSTMLayerFunction), on the same tree and the same box.  Device-synchronised seconds, warmed
up, the two routes alternated; the median and the spread (min ... max) of --reps runs.  One JSON line per case.

    python tests/tools/time_train_lstm.py [--cases layer,step] [--reps 7]
  layer   one layer forward + backward (every gradient): 240/320/320 at R = 64, T = 600; 640/2048/640 at R = 16 and 64 for
          T = 150 and 300
  step    the whole train step (forward, fused joint + loss, backward, SGD) of bench.py's bench_e2e model: configs[2], 2 x 320
          encoder, 1 x 320 prediction network, B = 64, T = 600, 100 labels
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/tools/time_train_lstm.py --trace
  trace   a run of its own for the profiler: every layer shape once per route after one warm-up, no timing (per-launch times of
          lstm_train_step_kernel<role, rows per workgroup, k groups>: roles 0 forward gates, 1 forward projection, 2 backward
          dr, 3 backward cell)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import lstm as lmod  # noqa: E402

# (I, H, P, R, T)
LAYERS = [(240, 320, 320, 64, 600), (640, 2048, 640, 16, 150), (640, 2048, 640, 64, 150), (640, 2048, 640, 16, 300),
          (640, 2048, 640, 64, 300)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns, reps, warmup=2):
    """fns {name: callable}: warm every one up, then time them in turn, reps times -> {name: (median, min, max)} in ms."""
    for _ in range(warmup):
        for fn in fns.values():
            timed(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timed(fn) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def layer_fns(I, H, P, R, T, dev):
    torch.manual_seed(0)
    m = torch.nn.LSTM(I, H, proj_size=P if P < H else 0, batch_first=True)
    pkg.model.init_lstm_like_tf1_(m)
    m = m.to(dev)
    x = torch.randn(R, T, I, device=dev, requires_grad=True)
    dy = torch.randn(R, T, P, device=dev)

    def run(engine):
        m.zero_grad(set_to_none=True)
        x.grad = None
        y = lmod.lstm_layer(m, x) if engine else m(x)[0]
        y.backward(dy)

    return {"torch": lambda: run(False), "engine": lambda: run(True)}


def report(case, res, **shape):
    t, e = res["torch"], res["engine"]
    print(json.dumps({"case": case, **shape, "torch_ms": round(t[0], 3), "torch_min_max": [round(t[1], 3), round(t[2], 3)],
                      "engine_ms": round(e[0], 3), "engine_min_max": [round(e[1], 3), round(e[2], 3)],
                      "speedup": round(t[0] / e[0], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="layer,step")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_lstm.py needs an MI355X: a timing taken elsewhere says nothing")
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    dev = torch.device("cuda:0")
    pkg.build()
    if args.trace:
        for I, H, P, R, T in LAYERS:
            for fn in layer_fns(I, H, P, R, T, dev).values():
                fn(), fn()
            torch.cuda.synchronize()
        return
    cases = args.cases.split(",")
    if "layer" in cases:
        for I, H, P, R, T in LAYERS:
            report("layer", alternate(layer_fns(I, H, P, R, T, dev), args.reps), I=I, H=H, P=P, R=R, T=T)
    if "step" in cases:
        hp = pkg.HParams(vocab_size=28, embedding_size=320, encoder_layers=2, encoder_size=320, projection_size=320,
                         time_reduction_index=0, pred_net_layers=1, pred_net_size=320, joint_net_size=320)  # bench.py bench_e2e
        batch = pkg.synthetic_batch(hp, batch=64, frames=600, max_labels=100, device=dev, seed=1234)
        steps = {}
        for route in ("torch", "engine"):
            torch.manual_seed(0)
            steps[route] = pkg.TrainStep(pkg.Transducer(hp, lstm=route).to(dev), global_batch=64)
        res = alternate({k: (lambda s=s: s(*batch)) for k, s in steps.items()}, args.reps, warmup=3)
        report("train_step", res, model="configs[2]", B=64, T=600, U=101)


if __name__ == "__main__":
    main()
