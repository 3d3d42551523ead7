"""Timings of the batched TDT beam search (include/rnnt_tdt_beam.h), by the method of tests/tools/time_tdt_decode.py: device events,
warm-up, alternating rounds in one process, median [min .. max] in milliseconds.

    python -m tests.tools.time_tdt_beam [--out FILE] [--quick]
    python -m tests.tools.time_tdt_beam --trace      # no timing: one short decode of each route, to run under a kernel trace

H = J = 640, 300 encoder frames, B in {16, 64}, V in {28, 1024}, D = 5 (durations [0, 1, 2, 3, 4]), beam in {1, 4, 8}.  Per
configuration, in the same process and in alternating rounds:
    tdt_beam_search_batch                                     the decoder under test
    tdt_greedy_search_batch(max_symbols_per_frame=1)          what beam = 1 must equal
    decoding.beam_search_batch on the same joint read as V + D symbols   the token-only beam search: every occupied row, every frame
Reported: wall time of a decode, ms per step (300 steps for the two beam searches), and the joint rows the TDT beam search
evaluated per utterance (its ACTIVE rows; the token-only search evaluates every occupied slot at every frame: about beam x 300)
-- what the duration jumps save.  The active rows are counted in a separate, untimed decode.  The weights are random: what they
skip says nothing about a trained model.

--trace: B = 64, V = 1024, beam = 4, 40 frames, durations [1] (every hypothesis is active at every frame, so the step kernel runs
on as many live rows as beam_step_kernel does at alphabet_size = V + 1) and then durations [0, 1, 2, 3, 4]."""
import argparse
import json
import statistics
import types

import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding, tdt

DEV = "cuda:0"
DUR = [0, 1, 2, 3, 4]
H = J = 640
T = 300
BLANK_BIAS = 3.0  # added to the blank's b2, so that blanks and tokens both occur with random weights


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _setup(B, V, frames_n=T, durations=DUR, seed=0):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=1, encoder_size=H,
                     projection_size=H, time_reduction_index=0, pred_net_layers=1, pred_net_size=H, joint_net_size=J)
    pred = pkg.model.PredictionNetwork(hp).eval().to(DEV)
    jt = pkg.JointLoss(H, J, V + len(durations)).to(DEV)
    with torch.no_grad():
        jt.W2.mul_(6.0)
        jt.b2[0] += BLANK_BIAS
    enc = torch.randn(B, frames_n, H, device=DEV)
    frames = torch.full((B,), frames_n, dtype=torch.int32, device=DEV)
    return pred, jt, enc, frames


def _routes(pred, jt, enc, frames, K, route, durations=DUR):
    as_symbols = types.SimpleNamespace(joint=jt, prediction=pred)  # the same joint, its V + D columns read as symbols
    return {
        "tdt_beam_search_batch": lambda: tdt.tdt_beam_search_batch(pred, jt, enc, frames, durations, beam=K, prediction_route=route),
        "tdt_greedy_search_batch(max_symbols_per_frame=1)":
            lambda: tdt.tdt_greedy_search_batch(pred, jt, enc, frames, durations, max_symbols_per_frame=1, prediction_route=route),
        "beam_search_batch at V + D symbols": lambda: decoding.beam_search_batch(as_symbols, enc, frames, beam=K, prediction=route),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="3 rounds instead of 5")
    ap.add_argument("--route", default="engine", choices=["torch", "engine"], help="the prediction network's route, the same for all")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    pkg.build()
    if a.trace:
        for durations in ([1], DUR):
            pred, jt, enc, frames = _setup(64, 1024, 40, durations)
            routes = _routes(pred, jt, enc, frames, 4, a.route, durations)
            for _ in range(2):
                for fn in routes.values():
                    fn()
        torch.cuda.synchronize()
        return
    rows = {}
    rounds = 3 if a.quick else 5
    for B in (16, 64):
        for V in (28, 1024):
            pred, jt, enc, frames = _setup(B, V)
            for K in (1, 4, 8):
                tag = f"B{B} V{V} D{len(DUR)} beam{K} T'{T} H{H} J{J} ({a.route} prediction)"
                routes = _routes(pred, jt, enc, frames, K, a.route)
                for fn in routes.values():  # warm-up: allocations, workspaces, code objects
                    fn()
                times = {k: [] for k in routes}
                for _ in range(rounds):
                    for k, fn in routes.items():
                        times[k].append(_events(fn))
                steps = {k: T for k in routes}
                steps["tdt_greedy_search_batch(max_symbols_per_frame=1)"] = tdt.LAST_STEPS
                tdt.tdt_beam_search_batch(pred, jt, enc, frames, DUR, beam=K, prediction_route=a.route, count_active=True)  # (untimed)
                active = tdt.LAST_ACTIVE_ROWS.double().mean().item()
                for k, v in times.items():
                    med = statistics.median(v)
                    rows[f"{tag} | {k}"] = dict(median=med, min=min(v), max=max(v), steps=steps[k], ms_per_step=med / steps[k])
                rows[f"{tag} | joint rows per utterance"] = dict(tdt_beam_active_rows=active, token_only_beam_rows_at_most=K * T,
                                                                 greedy_steps=tdt.LAST_STEPS)
                for k, r in rows.items():
                    if k.startswith(tag):
                        if "median" in r:
                            print(f"{k}: {r['median']:.2f} [{r['min']:.2f} .. {r['max']:.2f}] ms  steps={r['steps']}  "
                                  f"{r['ms_per_step']:.4f} ms/step", flush=True)
                        else:
                            print(f"{k}: {r}", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
