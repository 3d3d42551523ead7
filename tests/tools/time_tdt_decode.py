"""Timings of batched greedy TDT decoding (include/rnnt_tdt_greedy.h), by the method of tests/tools/time_tdt.py: device events,
warm-up, alternating rounds in one process, median [min .. max] in milliseconds.

    python -m tests.tools.time_tdt_decode [--out FILE] [--no-decode]
    python -m tests.tools.time_tdt_decode --calls 5      # no timing: a few steps of each route, to run under a kernel trace

Per step: compute_rnnt_tdt_greedy_step against compute_rnnt_greedy_step on the same tensors read as alphabet_size = V + D, B = 64,
J = 640: joint_dtype 1 at (V, D) = (1024, 5) and the f32-grade joint at (28, 5).  A window is CALLS steps after an untimed begin,
with utterances long enough that no hypothesis finishes inside a window (every row runs in every step of both decoders).
Per decode: tdt_greedy_search_batch against the host loop tdt_greedy_decode run over the B utterances with the same joint and
prediction network, and against decoding.greedy_search_batch with a standard joint of V columns on the same encoder output; the
decode steps of each are printed (their ratio is the frame skipping) with the durations the TDT decode chose.  The weights are
random: what they skip says nothing about a trained model."""
import argparse
import ctypes
import json
import statistics
import types

import numpy as np
import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib, decoding, tdt

DEV = "cuda:0"
DUR = [0, 1, 2, 3, 4]
ROUNDS, CALLS = 7, 10
STEP_SHAPES = [(1, 640, 1024), (0, 640, 28)]  # (joint_dtype, J, V)
B_STEP, T_STEP = 64, 64  # 10 steps of at most 4 frames stay inside 64 frames
BLANK_BIAS = 10.0  # added to the blank's b2 in the decode comparison: about the largest of 1024 random token logits, so that blanks occur


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _step_routes(dtype, J, V):
    """-> {name: (begin, step)} for the two decoders on the same tensors."""
    D, B, T, N = len(DUR), B_STEP, T_STEP, 4 * CALLS
    R = V + D
    g = torch.Generator().manual_seed(R)
    enc = torch.randn(B, T, J, generator=g).to(DEV)
    pred = torch.randn(B, J, generator=g).to(DEV)
    W2 = ((torch.rand(J, R, generator=g) * 2 - 1) * (6.0 / (J + R)) ** 0.5 * (3.0 if dtype == 0 else 12.0)).to(DEV)
    b2 = (0.1 * torch.randn(R, generator=g)).to(DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    hyps, hf = (torch.zeros(B, N, dtype=torch.int32, device=DEV) for _ in range(2))
    hl = torch.zeros(B, N, device=DEV)
    lengths, emitted, done = (torch.zeros(n, dtype=torch.int32, device=DEV) for n in (B, B, 1))
    scores = torch.zeros(B, device=DEV)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, 1)
    base, ext = _lib.load(), _lib.load_tdtgreedy()
    ws_g = torch.empty(_lib.greedy_workspace_bytes(T, B, J, R, dtype), dtype=torch.uint8, device=DEV)
    ws_t = torch.empty(_lib.tdt_greedy_workspace_bytes(T, B, J, V, D, dtype), dtype=torch.uint8, device=DEV)
    dur = (ctypes.c_int * D)(*DUR)
    keep = (enc, pred, W2, b2, frames, hyps, hf, hl, lengths, emitted, done, scores, ws_g, ws_t)
    p = lambda x: x.data_ptr()  # noqa: E731

    def g_begin():
        assert base.compute_rnnt_greedy_begin(p(enc), p(frames), None, p(W2), p(b2), J, R, B, 1, dtype, p(ws_g), opts) == 0

    def g_step():
        assert base.compute_rnnt_greedy_step(p(pred), p(hyps), N, p(lengths), p(scores), p(emitted), p(done), None, J, R, B, dtype,
                                             p(ws_g), opts) == 0

    def t_begin():
        assert ext.compute_rnnt_tdt_greedy_begin(p(enc), p(frames), None, p(W2), p(b2), J, V, dur, D, B, 1, dtype, p(ws_t), opts) == 0

    def t_step(times=False):
        assert ext.compute_rnnt_tdt_greedy_step(p(pred), p(hyps), p(hf) if times else None, p(hl) if times else None, N, p(lengths),
                                                p(scores), p(emitted), p(done), None, J, V, D, B, dtype, p(ws_t), opts) == 0

    return {"greedy step at alphabet_size = V + D": (g_begin, g_step), "tdt greedy step": (t_begin, t_step),
            "tdt greedy step with hyp_frames / hyp_logp": (t_begin, lambda: t_step(True))}, keep, done


def _window(begin, step, calls):
    begin()
    torch.cuda.synchronize()
    return _events(lambda: [step() for _ in range(calls)]) / calls


def _decode_setup(B=16, T=100, H=320, J=640, V=1024, seed=0):
    torch.manual_seed(seed)
    hp = pkg.HParams(vocab_size=V, mel_bins=4, downsample_factor=2, embedding_size=64, encoder_layers=1, encoder_size=H,
                     projection_size=H, time_reduction_index=0, pred_net_layers=1, pred_net_size=H, joint_net_size=J)
    pred = pkg.model.PredictionNetwork(hp).eval().to(DEV)
    jt = pkg.JointLoss(H, J, V + len(DUR)).to(DEV)
    js = pkg.JointLoss(H, J, V).to(DEV)
    with torch.no_grad():
        jt.W2.mul_(6.0)
        jt.b2[0] += BLANK_BIAS
        js.W1.copy_(jt.W1), js.b1.copy_(jt.b1), js.W2.copy_(jt.W2[:, :V]), js.b2.copy_(jt.b2[:V])  # the token head alone
    enc = torch.randn(B, T, H, device=DEV)
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    return pred, jt, js, enc, frames


def _host_loop(pred, jt, enc, frames, chosen):
    """tdt.tdt_greedy_decode over the utterances: the prediction network advanced one token at a time, one joint cell per call."""
    V = jt.W2.shape[1] - len(DUR)
    steps = 0
    out = []
    for b in range(enc.shape[0]):
        state = {"n": -1, "g": None, "s": [None] * len(pred.blocks)}

        def fn(t, y, b=b, state=state):
            nonlocal steps
            while state["n"] < len(y):  # (tokens only grow)
                tok = 0 if state["n"] < 0 else y[state["n"]]
                state["g"], state["s"] = decoding._pred_step(pred, torch.tensor([tok], dtype=torch.int32, device=DEV), state["s"])
                state["n"] += 1
            steps += 1
            lg = jt.logits(enc[b : b + 1, t : t + 1], state["g"][:, None, :])[0, 0, 0]
            chosen.append(DUR[int(torch.argmax(lg[V:]))])
            return lg
        with torch.no_grad():
            out.append(tdt.tdt_greedy_decode(fn, int(frames[b]), DUR, 0, 10))
    return out, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--calls", type=int, default=0, help="no timing: this many steps of each step route (for a kernel trace)")
    a = ap.parse_args()
    pkg.build()
    rows = {}
    for dtype, J, V in STEP_SHAPES:
        routes, keep, done = _step_routes(dtype, J, V)
        tag = f"B{B_STEP} J{J} V{V} D{len(DUR)} joint_dtype {dtype}"
        for begin, step in routes.values():
            _window(begin, step, CALLS)
        assert int(done.cpu()[0]) == 0, "a hypothesis finished inside a window"
        if a.calls:
            for begin, step in routes.values():
                _window(begin, step, a.calls)
            continue
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, (begin, step) in routes.items():
                times[k].append(_window(begin, step, CALLS))
        assert int(done.cpu()[0]) == 0
        for k, v in times.items():
            rows[f"{tag} | {k}"] = dict(median=statistics.median(v), min=min(v), max=max(v))
    if not a.calls and not a.no_decode:
        pred, jt, js, enc, frames = _decode_setup()
        B, T = enc.shape[0], enc.shape[1]
        std = types.SimpleNamespace(joint=js, prediction=pred)
        tag = f"B{B} T'{T} H320 J640 V1024 D{len(DUR)}"
        steps = {}

        def batched(route):
            tdt.tdt_greedy_search_batch(pred, jt, enc, frames, DUR, max_symbols_per_frame=10, prediction_route=route)
            steps[f"tdt_greedy_search_batch ({route} prediction)"] = tdt.LAST_STEPS

        def standard(route):
            decoding.greedy_search_batch(std, enc, frames, max_symbols_per_frame=10, prediction=route)
            steps[f"greedy_search_batch, V columns ({route} prediction)"] = decoding.LAST_STEPS

        routes = {}
        for route in ("torch", "engine"):
            routes[f"tdt_greedy_search_batch ({route} prediction)"] = lambda r=route: batched(r)
            routes[f"greedy_search_batch, V columns ({route} prediction)"] = lambda r=route: standard(r)
        for fn in routes.values():
            fn()
        times = {k: [] for k in routes}
        for _ in range(5):
            for k, fn in routes.items():
                times[k].append(_events(fn))
        chosen = []
        host_out, host_steps = _host_loop(pred, jt, enc, frames, chosen)  # (warm-up, and the durations chosen)
        hist = {d: chosen.count(d) for d in DUR}
        host_times = []
        for _ in range(2):
            host_times.append(_events(lambda: _host_loop(pred, jt, enc, frames, [])))
        times["tdt_greedy_decode host loop over the utterances"] = host_times
        steps["tdt_greedy_decode host loop over the utterances"] = host_steps
        ids, lengths, _ = tdt.tdt_greedy_search_batch(pred, jt, enc, frames, DUR, max_symbols_per_frame=10)
        same = sum(ids[b, : int(lengths[b])].tolist() == host_out[b][0] for b in range(B))
        for k, v in times.items():
            rows[f"{tag} | {k}"] = dict(median=statistics.median(v), min=min(v), max=max(v), steps=steps[k])
        rows[f"{tag} | decisions"] = dict(host_loop_joint_evaluations=host_steps, durations_chosen=hist, tokens=int(lengths.sum()),
                                          utterances_with_the_host_loop_s_tokens=f"{same} of {B}", frames=B * T)
    for k, r in rows.items():
        if "median" in r:
            extra = f"  steps={r['steps']}" if "steps" in r else ""
            print(f"{k}: {r['median']:.4f} [{r['min']:.4f} .. {r['max']:.4f}] ms{extra}", flush=True)
        else:
            print(f"{k}: {r}", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1, default=str)


if __name__ == "__main__":
    main()
