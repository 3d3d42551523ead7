"""Wall time of greedy decoding on an MI355X: the one-utterance decoder (decoding.greedy_decode) looped over a batch against
decoding.greedy_decode_batch, at the reference's defaults (H = J = 640, V = 4096) and at a character vocabulary (V = 28), ~300
encoder frames.  One JSON line per case: device-synchronised seconds of both, decode steps of the batched one, ids agree.

    python tests/tools/time_greedy_batch.py [--cases 16x4096,64x4096,16x28] [--frames 300]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import decoding  # noqa: E402


def model_for(V, seed=11):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=2, encoder_size=640,
                     projection_size=640, time_reduction_index=0, pred_net_layers=1, pred_net_size=640, joint_net_size=640)
    m = pkg.Transducer(hp)
    with torch.no_grad():  # blank-leaning, as a trained joint is: a few symbols per utterance
        m.joint.b2[0] += 15.0 if V > 32 else 3.0
        m.joint.W2 *= 8.0
    return m.cuda().eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="16x4096,64x4096,16x28")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--max-length", type=int, default=60)
    ap.add_argument("--skip-old", action="store_true", help="time the batched decoder only")
    a = ap.parse_args()
    pkg.build()
    for case in a.cases.split(","):
        B, V = (int(x) for x in case.split("x"))
        model = model_for(V)
        mel = torch.randn(B, 2 * a.frames, 8, device="cuda")
        decoding.greedy_decode_batch(model, mel[:2], max_length=a.max_length)  # warm-up (allocations, code objects)
        (ids, lengths, _), t_new = timed(lambda: decoding.greedy_decode_batch(model, mel, max_length=a.max_length))
        steps = decoding.LAST_STEPS
        rec = {"B": B, "V": V, "J": 640, "frames": a.frames, "steps": steps, "new_s": round(t_new, 4),
               "symbols": int(lengths.sum())}
        if not a.skip_old:
            old, t_old = timed(lambda: [decoding.greedy_decode(model, mel[b : b + 1], a.max_length).tolist()[0] for b in range(B)])
            rec["old_s"] = round(t_old, 4)
            rec["speedup"] = round(t_old / t_new, 2)
            rec["ids_agree"] = all(ids[b, : int(lengths[b])].tolist() == old[b] for b in range(B))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
