"""Wall time of batched decoding on an MI355X with the prediction network stepped by torch (prediction="torch", the default)
against the library's prediction-network step (prediction="engine"), on encoder outputs of ~300 frames.  Two prediction
networks: time_greedy_batch.py's model (E 64, H 640 unprojected, L 1) and the reference defaults (E 500, H 2048, P 640, L 2);
J = 640.  One JSON line per case: device-synchronised seconds of both routes, decode steps, per-step milliseconds, ids agree.

    python tests/tools/time_prednet_decode.py [--cases greedy:16x4096,beam4:64x28,...] [--nets small,ref] [--frames 300]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import decoding  # noqa: E402

NETS = {"small": dict(embedding_size=64, pred_net_layers=1, pred_net_size=640),
        "ref": dict(embedding_size=500, pred_net_layers=2, pred_net_size=2048)}
CASES = ",".join(f"{m}:{b}x{v}" for m in ("greedy", "beam4") for b in (16, 64) for v in (4096, 28))


def model_for(net, V, seed=11):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, encoder_layers=2, encoder_size=640, projection_size=640,
                     time_reduction_index=0, joint_net_size=640, **NETS[net])
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
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--nets", default="small,ref")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--max-length", type=int, default=60)
    a = ap.parse_args()
    pkg.build()
    for net in a.nets.split(","):
        for case in a.cases.split(","):
            mode, shape = case.split(":")
            B, V = (int(x) for x in shape.split("x"))
            model = model_for(net, V)
            torch.manual_seed(1)
            enc = torch.randn(B, a.frames, 640, device="cuda")
            frames = torch.full((B,), a.frames, dtype=torch.int32, device="cuda")
            if mode == "greedy":
                run = lambda p: decoding.greedy_search_batch(model, enc, frames, a.max_length, prediction=p)  # noqa: E731
            else:
                K = int(mode[4:])
                run = lambda p: decoding.beam_search_batch(model, enc, frames, beam=K, prediction=p)  # noqa: E731
            rec = {"net": net, "mode": mode, "B": B, "V": V, "frames": a.frames}
            out = {}
            for p in ("torch", "engine"):
                run(p)  # warm-up (allocations, code objects, workspaces)
                out[p], rec[f"{p}_s"] = timed(lambda: run(p))
                steps = decoding.LAST_STEPS if mode == "greedy" else a.frames
                rec["steps"] = steps
                rec[f"{p}_ms_per_step"] = round(1e3 * rec[f"{p}_s"] / max(1, steps), 4)
                rec[f"{p}_s"] = round(rec[f"{p}_s"], 4)
            rec["speedup"] = round(rec["torch_s"] / rec["engine_s"], 2)
            rec["ids_agree"] = bool(torch.equal(out["torch"][0], out["engine"][0]) and torch.equal(out["torch"][1], out["engine"][1]))
            best = lambda o: o[2].reshape(B, -1)[:, 0].double()  # noqa: E731  (the best hypothesis' score of each utterance)
            rec["max_best_score_diff"] = float((best(out["torch"]) - best(out["engine"])).abs().max())
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
