"""Timings of the streaming beam search with several symbols per frame (include/rnnt_beam_multi_stream.h), by the method of
tests/tools/time_multibeam.py: device events, warm-up, alternating rounds in one process, median [min .. max] in milliseconds.

    python -m tests.tools.time_multibeam_stream [--out FILE] [--quick]
    python -m tests.tools.time_multibeam_stream --trace     # no timing: a short decode of each kind, to run under a kernel trace

S = 16, V = 4096, H = J = 640, beam 4, the prediction network on the engine route; 300 encoder frames per stream.  In alternating
rounds, for E = 1, 2, 3:
    decoding.beam_search_batch(symbols_per_frame=E)      the baseline: the offline search on the same frames, 300 (E + 1) steps
    MultiBeamStreamJoint in chunks of 10 frames          30 feeds, each followed by 10 (E + 1) steps of decoding._beam_loop(carry=True)
    MultiBeamStreamJoint in chunks of 1 frame            300 feeds, each followed by E + 1 steps
Reported: wall time of the whole stream, ms per step, and the ratio to the baseline's median.  The stream steps the prediction
network after every joint step (the offline search skips the last one), and adds per chunk the projection of the chunk and one feed
kernel.  The weights are random: how often a frame really needs a second symbol says nothing about a trained model."""
import argparse
import json
import statistics

import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd import joint as jmod
from tests.tools.time_multibeam import B as S
from tests.tools.time_multibeam import DEV, K, T, _events, _setup


def _stream(model, enc, E, chunk, token_times=False):
    """One pass of all S streams over enc [S, frames, H] in chunks of `chunk` frames; the joint, its workspace and the prediction
    stepper are made once (a live decoder keeps them)."""
    jx = jmod.MultiBeamStreamJoint(model.joint, K, E, token_times=token_times)
    frames_n = enc.shape[1]
    jx.begin(S, chunk, frames_n * E)
    assert jx.engine
    ps, x0 = decoding._prediction_step(model.prediction, decoding._joint_W1(jx), S * 2 * K)
    ones = torch.ones(S, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(S, dtype=torch.int32, device=DEV)
    full = torch.full((S,), chunk, dtype=torch.int32, device=DEV)
    chunks = [enc[:, lo: lo + chunk].contiguous() for lo in range(0, frames_n, chunk)]
    state = {"x": x0}

    def run():
        x = ps.reset([True] * (S * 2 * K))
        for i, c in enumerate(chunks):
            n = c.shape[1]
            jx.feed(c, full if n == chunk else torch.full((S,), n, dtype=torch.int32, device=DEV), reset=ones if i == 0 else zeros,
                    final=ones if i + 1 == len(chunks) else zeros)
            x = decoding._beam_loop(jx, ps, x, n * (E + 1), carry=True)
        state["x"] = x
        return jx.results()

    return run


def _kinds(model, enc, frames):
    out = {}
    for E in (1, 2, 3):
        out[f"E={E} | offline beam_search_batch(symbols_per_frame={E})"] = (
            lambda E=E: decoding.beam_search_batch(model, enc, frames, beam=K, prediction="engine", symbols_per_frame=E), E, None)
        for chunk in (10, 1):
            out[f"E={E} | stream, chunks of {chunk}"] = (_stream(model, enc, E, chunk), E, chunk)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="3 rounds instead of 5")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    pkg.build()
    model, enc, frames = _setup(20 if a.trace else T)
    kinds = _kinds(model, enc, frames)
    for fn, _, _ in kinds.values():  # warm-up: allocations, workspaces, code objects
        fn()
    torch.cuda.synchronize()
    if a.trace:
        for fn, _, _ in kinds.values():
            fn()
        torch.cuda.synchronize()
        return
    # the stream and the offline search give the same ids here only up to the projection's summation order: not asserted
    rounds = 3 if a.quick else 5
    times = {k: [] for k in kinds}
    for _ in range(rounds):
        for k, (fn, _, _) in kinds.items():
            times[k].append(_events(fn))
    rows, base = {}, {}
    tag = f"S{S} T'{T} V4096 H640 J640 beam{K} (engine prediction)"
    for k, v in times.items():
        _, E, chunk = kinds[k]
        steps = T * (E + 1)
        med = statistics.median(v)
        if chunk is None:
            base[E] = (med, min(v), max(v))
        b = base[E]
        rows[f"{tag} | {k}"] = dict(median=med, min=min(v), max=max(v), steps=steps, ms_per_step=med / steps, ratio=med / b[0],
                                    baseline_spread=[b[1] / b[0], b[2] / b[0]])
        print(f"{tag} | {k}: {med:.2f} [{min(v):.2f} .. {max(v):.2f}] ms  steps={steps}  {med / steps:.4f} ms/step  "
              f"x{med / b[0]:.3f} of the baseline [{b[1] / b[0]:.3f} .. {b[2] / b[0]:.3f}]", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
