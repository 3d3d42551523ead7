"""Cost of token_times=True on an MI355X: the timed against the untimed route of greedy_decode_batch, beam_decode_batch,
StreamingGreedyDecoder and StreamingBeamDecoder at the shapes of time_beam_batch.py / time_streaming_beam.py (H = J = 640, V = 4096
and V = 28, ~300 encoder frames), and against today's workaround for the same information: an untimed greedy decode followed by
alignment.align_joint on its hypothesis, the lattice at the fused-route shape of DESIGN 8i (B16 T300 U100 V4096 for the default
first case: the hypothesis padded to --align-u - 1 labels).  The parent commit's build is not a route here: the tool loads one
library per process.  HIP events; the routes alternate call by call in one process; medians after warm-up,
spreads as min ... max.  One JSON line per case.

    python tests/tools/time_token_times.py [--cases 16x4096,16x28] [--beam 4] [--frames 300] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from rnnt_speech_recognition_amd import alignment, decoding  # noqa: E402
from rnnt_speech_recognition_amd.decoding import StreamingBeamDecoder, StreamingGreedyDecoder  # noqa: E402
from tests.tools.time_greedy_batch import model_for  # noqa: E402


def alternate(routes, reps, warmup=2):
    """routes: {name: fn}.  Every round runs each route once, in turn -> {name: (median ms, min ms, max ms)}."""
    ms = {k: [] for k in routes}
    for r in range(warmup + reps):
        for name, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return {k: (round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)) for k, v in ms.items()}


def stream_route(make, mel, chunk):
    dec = make()
    S, T = mel.shape[0], mel.shape[1]

    def run():
        dec.start(list(range(S)))
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            dec.feed(mel[:, t0: t0 + n], [n] * S, [t0 + n == T] * S)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="16x4096,16x28")
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=16, help="spectrogram rows per streaming feed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--align-u", type=int, default=100, help="lattice rows of the workaround's alignment")
    a = ap.parse_args()
    K = a.beam
    for case in a.cases.split(","):
        B, V = (int(x) for x in case.split("x"))
        model = model_for(V)
        mel = torch.randn(B, 2 * a.frames, 8, device="cuda")

        def workaround():
            ids, n, _ = decoding.greedy_decode_batch(model, mel, max_length=60)
            U = a.align_u
            labels = torch.nn.functional.pad(ids, (0, max(0, U - 1 - ids.shape[1])))[:, : U - 1].contiguous()
            with torch.no_grad():
                enc = model.encoder(mel)
                pred = model.prediction(torch.nn.functional.pad(labels.long(), (1, 0)))
            T = torch.full((B,), enc.shape[1], dtype=torch.int32, device=mel.device)
            return alignment.align_joint(model.joint, enc, pred, labels, T, n.clamp(max=U - 1))

        batch = alternate({
            "greedy": lambda: decoding.greedy_decode_batch(model, mel, max_length=60),
            "greedy_timed": lambda: decoding.greedy_decode_batch(model, mel, max_length=60, token_times=True),
            "greedy_then_align": workaround,
            "beam": lambda: decoding.beam_decode_batch(model, mel, beam=K),
            "beam_timed": lambda: decoding.beam_decode_batch(model, mel, beam=K, token_times=True),
        }, a.reps)
        stream = alternate({
            "stream_greedy": stream_route(lambda: StreamingGreedyDecoder(model, B, a.chunk, max_length=60), mel, a.chunk),
            "stream_greedy_timed": stream_route(lambda: StreamingGreedyDecoder(model, B, a.chunk, max_length=60, token_times=True),
                                                mel, a.chunk),
            "stream_beam": stream_route(lambda: StreamingBeamDecoder(model, B, a.chunk, beam=K), mel, a.chunk),
            "stream_beam_timed": stream_route(lambda: StreamingBeamDecoder(model, B, a.chunk, beam=K, token_times=True), mel, a.chunk),
        }, a.reps)
        print(json.dumps({"B": B, "V": V, "J": 640, "frames": a.frames, "beam": K, "chunk": a.chunk, "reps": a.reps,
                          "ms_median_min_max": {**batch, **stream}}), flush=True)


if __name__ == "__main__":
    main()
