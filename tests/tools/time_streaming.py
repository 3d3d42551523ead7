"""Wall time of streaming greedy decoding on an MI355X (decoding.StreamingGreedyDecoder) at the reference defaults: 240 features
(80 mel bins x downsample 3), the 8 x 2048 / 640 encoder with reduction 2 at block 1, H = J = 640, V = 4096, a blank-leaning
joint.  Every slot is fed chunks of 16 spectrogram frames (480 ms of audio at a 10 ms step and downsample 3).  Reported per
S = 1, 16, 64: the median wall time of a feed (device-synchronised, after warm-up feeds), the real-time factor (feed time /
480 ms), and for comparison one offline greedy_decode_batch of the same audio (every chunk at once, encoder="engine",
prediction="engine"), per 480 ms of audio.  One JSON line per S.

    python tests/tools/time_streaming.py [--slots 1,16,64] [--chunks 12] [--warmup 3] [--check-every 32]"""
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

CHUNK, AUDIO_S = 16, 0.48


def model_at_defaults():
    torch.manual_seed(11)
    hp = pkg.HParams()  # (the reference defaults)
    model = pkg.Transducer(hp)
    with torch.no_grad():
        model.joint.b2[0] += 15.0  # a blank-leaning joint, as a trained one is
        model.joint.W2 *= 8.0
    return model.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,16,64")
    ap.add_argument("--chunks", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-every", type=int, default=decoding.CHECK_EVERY)
    args = ap.parse_args()
    model = model_at_defaults()
    for S in (int(s) for s in args.slots.split(",")):
        torch.manual_seed(S)
        K = args.warmup + args.chunks
        mel = torch.randn(S, K * CHUNK, 240, device="cuda")
        dec = decoding.StreamingGreedyDecoder(model, S, CHUNK, max_length=1000, check_every=args.check_every)
        dec.start(list(range(S)))
        ts, steps = [], []
        for k in range(K):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.feed(mel[:, CHUNK * k: CHUNK * (k + 1)], [CHUNK] * S, [k == K - 1] * S)
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts.append(time.perf_counter() - t0)
                steps.append(decoding.LAST_STEPS)
        feed = statistics.median(ts)
        offs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decoding.greedy_decode_batch(model, mel, None, 1000, encoder="engine", prediction="engine")
            torch.cuda.synchronize()
            offs.append(time.perf_counter() - t0)
        off = statistics.median(offs) / K
        print(json.dumps({"slots": S, "chunk_frames": CHUNK, "check_every": args.check_every, "feed_ms": round(feed * 1e3, 3), "rtf": round(feed / AUDIO_S, 4),
                          "steps_per_feed": statistics.median(steps), "offline_ms_per_480ms": round(off * 1e3, 3),
                          "offline_rtf": round(off / AUDIO_S, 4)}), flush=True)


if __name__ == "__main__":
    main()
