"""Wall time of beam search on an MI355X: decoding.beam_decode_batch at beam 1 / 4 / 8 against decoding.greedy_decode_batch with
max_symbols_per_frame = 1, at the reference's defaults (H = J = 640, V = 4096) and at a character vocabulary (V = 28), ~300
encoder frames.  One JSON line per case: device-synchronised seconds, per-step milliseconds, agreement of beam 1 with greedy.

    python tests/tools/time_beam_batch.py [--cases 16x4096,64x4096,16x28] [--beams 1,4,8] [--frames 300]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from rnnt_speech_recognition_amd import decoding  # noqa: E402
from tests.tools.time_greedy_batch import model_for, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="16x4096,64x4096,16x28")
    ap.add_argument("--beams", default="1,4,8")
    ap.add_argument("--frames", type=int, default=300)
    a = ap.parse_args()
    for case in a.cases.split(","):
        B, V = (int(x) for x in case.split("x"))
        model = model_for(V)
        mel = torch.randn(B, 2 * a.frames, 8, device="cuda")
        decoding.greedy_decode_batch(model, mel[:2], max_symbols_per_frame=1)  # warm-up (allocations, code objects)
        (gids, glen, _), t_greedy = timed(lambda: decoding.greedy_decode_batch(model, mel, max_symbols_per_frame=1))
        for K in (int(k) for k in a.beams.split(",")):
            decoding.beam_decode_batch(model, mel[:2], beam=K)
            (ids, lengths, _), t_beam = timed(lambda: decoding.beam_decode_batch(model, mel, beam=K))
            rec = {"B": B, "V": V, "J": 640, "frames": a.frames, "beam": K, "beam_s": round(t_beam, 4),
                   "beam_ms_per_step": round(1e3 * t_beam / a.frames, 3), "greedy_s": round(t_greedy, 4),
                   "symbols": int(lengths.sum())}
            if K == 1:
                rec["ids_agree_greedy"] = bool(torch.equal(lengths, glen)) and all(
                    ids[b, : int(lengths[b])].tolist() == gids[b, : int(glen[b])].tolist() for b in range(B))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
