"""Timings of the beam search with several symbols per frame (include/rnnt_beam_multi.h), by the method of
tests/tools/time_tdt_beam.py: device events, warm-up, alternating rounds in one process, median [min .. max] in milliseconds.

    python -m tests.tools.time_multibeam [--out FILE] [--quick] [--route engine|torch]
    python -m tests.tools.time_multibeam --trace     # no timing: a short decode of each search, to run under a kernel trace

B = 16, T' = 300, V = 4096, H = J = 640, beam 4.  In alternating rounds:
    decoding.beam_search_batch(symbols_per_frame=E), E = 1, 2, 3    the search under test: T' (E + 1) steps on B 2 beam rows
    decoding.beam_search_batch()                                    the modified search: T' steps on B beam rows
Reported: wall time of a whole search and ms per step.  Then, on begun decodes and without the prediction network, the joint step
alone (the step and select kernels of one call, pred_proj fixed): compute_rnnt_multibeam_step against compute_rnnt_beam_step, per
call.  The two kernels of a call are told apart by a kernel trace of --trace, not here.  The weights are random: how often a
frame really needs a second symbol says nothing about a trained model."""
import argparse
import json
import statistics
import types

import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import decoding
from rnnt_speech_recognition_amd import joint as jmod

DEV = "cuda:0"
H = J = 640
B, T, V, K = 16, 300, 4096, 4
BLANK_BIAS = 3.0  # added to the blank's b2, so that blanks and tokens both occur with random weights


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _setup(frames_n=T, seed=0):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=1, encoder_size=H,
                     projection_size=H, time_reduction_index=0, pred_net_layers=1, pred_net_size=H, joint_net_size=J)
    pred = pkg.model.PredictionNetwork(hp).eval().to(DEV)
    jt = pkg.JointLoss(H, J, V).to(DEV)
    with torch.no_grad():
        jt.W2.mul_(6.0)
        jt.b2[0] += BLANK_BIAS
    enc = torch.randn(B, frames_n, H, device=DEV)
    frames = torch.full((B,), frames_n, dtype=torch.int32, device=DEV)
    return types.SimpleNamespace(joint=jt, prediction=pred), enc, frames


def _searches(model, enc, frames, route):
    out = {"beam_search_batch() [modified]": (lambda: decoding.beam_search_batch(model, enc, frames, beam=K, prediction=route), 1)}
    for E in (1, 2, 3):
        out[f"beam_search_batch(symbols_per_frame={E})"] = (
            lambda E=E: decoding.beam_search_batch(model, enc, frames, beam=K, prediction=route, symbols_per_frame=E), E + 1)
    return out


def _joint_steps(model, enc, frames, calls):
    """ms per call of the joint step alone on begun decodes: every call is a live round (calls <= T)."""
    out = {}
    for name, jx, rows in (("compute_rnnt_beam_step", jmod.BeamJoint(model.joint, K), B * K),
                           ("compute_rnnt_multibeam_step (E=3)", jmod.MultiBeamJoint(model.joint, K, 3), B * 2 * K)):
        jx.begin(enc, frames)
        pp = 0.5 * torch.randn(rows, jx.Jp, device=DEV)
        for _ in range(8):
            jx.step(pred_proj=pp)
        ms = _events(lambda: [jx.step(pred_proj=pp) for _ in range(calls)])
        out[name] = ms / calls
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="3 rounds instead of 5")
    ap.add_argument("--route", default="engine", choices=["torch", "engine"], help="the prediction network's route, the same for all")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    pkg.build()
    if a.trace:
        model, enc, frames = _setup(20)
        for fn, _ in _searches(model, enc, frames, a.route).values():
            fn()
            fn()
        torch.cuda.synchronize()
        return
    model, enc, frames = _setup()
    searches = _searches(model, enc, frames, a.route)
    for fn, _ in searches.values():  # warm-up: allocations, workspaces, code objects
        fn()
    rounds = 3 if a.quick else 5
    times = {k: [] for k in searches}
    for _ in range(rounds):
        for k, (fn, _) in searches.items():
            times[k].append(_events(fn))
    rows = {}
    tag = f"B{B} T'{T} V{V} H{H} J{J} beam{K} ({a.route} prediction)"
    for k, v in times.items():
        steps = T * searches[k][1]
        med = statistics.median(v)
        rows[f"{tag} | {k}"] = dict(median=med, min=min(v), max=max(v), steps=steps, ms_per_step=med / steps)
        print(f"{tag} | {k}: {med:.2f} [{min(v):.2f} .. {max(v):.2f}] ms  steps={steps}  {med / steps:.4f} ms/step", flush=True)
    per_call = [_joint_steps(model, enc, frames, 200) for _ in range(rounds)]
    for name in per_call[0]:
        v = [r[name] for r in per_call]
        rows[f"{tag} | joint step alone | {name}"] = dict(median=statistics.median(v), min=min(v), max=max(v))
        print(f"{tag} | joint step alone | {name}: {statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}] ms/call", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
