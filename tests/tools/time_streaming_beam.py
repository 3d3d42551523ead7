"""Wall time of streaming beam search on an MI355X (decoding.StreamingBeamDecoder) with the set-up of time_streaming.py: the
reference defaults (240 features, the 8 x 2048 / 640 encoder, H = J = 640, V = 4096, a blank-leaning joint), every slot fed
chunks of 16 spectrogram frames = 8 encoder frames (480 ms of audio).  Per (S, K) with S K <= 1024, beside each other:
  beam_feed_ms       a StreamingBeamDecoder feed;
  greedy_feed_ms     a StreamingGreedyDecoder feed at the same S (check_every = 8): what the beam costs a live service;
  offline_ms_per_480ms  beam_decode_batch of the same audio (encoder and prediction on the engine) per 480 ms: what chunking costs.
Device-synchronised wall time; warm-up feeds discarded; the two streaming routes alternate feed by feed in one session; median
and min ... max of `--chunks` (>= 12) feeds, and of as many offline decodes.  One JSON line per (S, K).

    python tests/tools/time_streaming_beam.py [--slots 1,16,64] [--beams 1,4,8] [--chunks 12] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from rnnt_speech_recognition_amd import decoding  # noqa: E402
from tests.tools.time_streaming import AUDIO_S, CHUNK, model_at_defaults  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def spread(ts):
    return {"median": round(statistics.median(ts) * 1e3, 3), "min": round(min(ts) * 1e3, 3), "max": round(max(ts) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,16,64")
    ap.add_argument("--beams", default="1,4,8")
    ap.add_argument("--chunks", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-length", type=int, default=512)
    args = ap.parse_args()
    assert args.chunks >= 12
    model = model_at_defaults()
    n = args.warmup + args.chunks
    for S in (int(s) for s in args.slots.split(",")):
        for K in (int(k) for k in args.beams.split(",")):
            if S * K > 1024:
                continue
            torch.manual_seed(S)
            mel = torch.randn(S, n * CHUNK, 240, device="cuda")
            beam = decoding.StreamingBeamDecoder(model, S, CHUNK, beam=K, max_length=args.max_length)
            greedy = decoding.StreamingGreedyDecoder(model, S, CHUNK, max_length=1000, check_every=8)
            beam.start(list(range(S)))
            greedy.start(list(range(S)))
            tb, tg = [], []
            for k in range(n):
                chunk, fr, fi = mel[:, CHUNK * k: CHUNK * (k + 1)], [CHUNK] * S, [k == n - 1] * S
                b = timed(lambda: beam.feed(chunk, fr, fi))
                g = timed(lambda: greedy.feed(chunk, fr, fi))
                if k >= args.warmup:
                    tb.append(b)
                    tg.append(g)
            decoding.beam_decode_batch(model, mel, None, beam=K, prediction="engine", encoder="engine")  # (allocations)
            offs = [timed(lambda: decoding.beam_decode_batch(model, mel, None, beam=K, prediction="engine", encoder="engine")) / n
                    for _ in range(args.chunks)]
            print(json.dumps({"slots": S, "beam": K, "chunk_frames": CHUNK, "max_length": args.max_length, "feeds": len(tb),
                              "beam_feed_ms": spread(tb), "greedy_feed_ms": spread(tg), "offline_ms_per_480ms": spread(offs),
                              "beam_rtf": round(statistics.median(tb) / AUDIO_S, 4)}), flush=True)


if __name__ == "__main__":
    main()
