"""Wall time of the encoder on an MI355X: torch's (model.encoder: nn.LSTM with proj_size per block) against the library's
(joint.EncoderStream, compute_rnnt_encoder_run), and of whole greedy decodes with each route.  Device-synchronised seconds,
warmed up, the two routes alternated; the median of --reps runs.  One JSON line per case.

    python tests/tools/time_encoder.py [--cases enc,decode] [--reps 5]
  enc     the reference-default encoder (240 features, 8 x 2048 / 640, reduction 2 at block 1) at B = 1, 16, 64 for T = 300 and
          1000 spectrogram frames, and the configs[2] encoder (2 x 320) at B = 64, T = 600
  decode  greedy_decode_batch at B = 16, T = 300, V = 4096, J = 640 with the reference defaults, in three configurations:
          torch encoder + torch prediction network, torch + engine, engine + engine"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import decoding  # noqa: E402
from rnnt_speech_recognition_amd.joint import EncoderStream  # noqa: E402

ENCODERS = {"ref": dict(encoder_layers=8, encoder_size=2048, projection_size=640, time_reduction_index=1),
            "configs2": dict(encoder_layers=2, encoder_size=320, projection_size=320, time_reduction_index=0,
                             pred_net_size=320, joint_net_size=320)}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts)


def alternate(runs, reps):
    """runs: {name: fn}; warm-up each, then reps rounds in which every route runs once -> {name: (out, median s)}."""
    outs, ts = {}, {k: [] for k in runs}
    for k, fn in runs.items():
        fn()
    for _ in range(reps):
        for k, fn in runs.items():
            outs[k], t = timed(fn, 1)
            ts[k].append(t)
    return {k: (outs[k], statistics.median(v)) for k, v in ts.items()}


def enc_cases(reps):
    for name, B, T in [("ref", 1, 300), ("ref", 16, 300), ("ref", 64, 300), ("ref", 1, 1000), ("ref", 16, 1000), ("ref", 64, 1000),
                       ("configs2", 64, 600)]:
        torch.manual_seed(0)
        model = pkg.Transducer(pkg.HParams(**ENCODERS[name])).cuda().eval()
        x = torch.randn(B, T, model.encoder.input_norm.num_features, device="cuda")
        es = EncoderStream(model.encoder)
        assert es.engine

        def engine():
            es.begin(B, T)
            return es.run(x)

        def torch_route():
            with torch.no_grad():
                return model.encoder(x)

        r = alternate({"torch": torch_route, "engine": engine}, reps)
        rec = {"case": "encoder", "encoder": name, "B": B, "T": T, "torch_ms": round(1e3 * r["torch"][1], 3),
               "engine_ms": round(1e3 * r["engine"][1], 3)}
        rec["speedup"] = round(rec["torch_ms"] / rec["engine_ms"], 2)
        d = (r["torch"][0] - r["engine"][0]).abs().max().item()
        rec["max_abs_diff"] = d
        print(json.dumps(rec), flush=True)
        del model, es


def decode_cases(reps):
    torch.manual_seed(11)
    B, T, V = 16, 300, 4096
    model = pkg.Transducer(pkg.HParams(vocab_size=V, **ENCODERS["ref"]))
    with torch.no_grad():  # blank-leaning, as a trained joint is: a few symbols per utterance
        model.joint.b2[0] += 15.0
        model.joint.W2 *= 8.0
    model = model.cuda().eval()
    mel = torch.randn(B, T, model.encoder.input_norm.num_features, device="cuda")
    runs = {f"{e}+{p}": (lambda e=e, p=p: decoding.greedy_decode_batch(model, mel, max_length=60, encoder=e, prediction=p))
            for e, p in [("torch", "torch"), ("torch", "engine"), ("engine", "engine")]}
    r = alternate(runs, reps)
    base = r["torch+torch"][0]
    for k, (out, t) in r.items():
        rec = {"case": "greedy_decode", "B": B, "T": T, "V": V, "routes": k, "ms": round(1e3 * t, 3),
               "ids_agree": bool(torch.equal(out[0], base[0]) and torch.equal(out[1], base[1]))}
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="enc,decode")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg.build()
    cases = a.cases.split(",")
    if "enc" in cases:
        enc_cases(a.reps)
    if "decode" in cases:
        decode_cases(a.reps)


if __name__ == "__main__":
    main()
