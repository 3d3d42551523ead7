"""What contextual biasing costs per frame: compute_rnnt_beam_step (step + select kernels) against compute_rnnt_beam_step_biased
with a 1,000-phrase context graph, through the C ABI, device-event times, at B 32, beam 4, joint size 640, for V = 28 (the
f32-grade joint) and V = 4096 (the f16 joint).  Each timed call is one frame of a decode that was begun once; the frame counter
runs on, so maxT is sized for warm-up + steps.  A third shape, V = 28 at joint size 704, times the wide f32-grade step kernel
(joint sizes above 640).  A report, not a gate.  Needs an MI355X.

    python tests/tools/time_context_bias.py [--steps 40] [--warmup 10] [--runs 4] [--unbiased-only] [--out time_context_bias.json]

--runs: the unbiased and the biased decode are timed alternately `runs` times; the spread of the medians is the noise floor.
--unbiased-only: the unbiased decode alone, touching nothing of the extension, so that it also runs on a libwarprnnt.so built
from an earlier commit (RNNT_LIBWARPRNNT=<path>): run it alternately on two builds to compare their unbiased route."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import _lib  # noqa: E402

DEV = "cuda:0"


def frames_ms(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def case(lib, V, dtype, J, steps, warmup, runs, unbiased_only, B=32, K=4):
    T = warmup + steps
    g = torch.Generator(device="cpu").manual_seed(V)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    enc, W2, b2 = rnd(B, T, J) * 0.5, rnd(J, V) * 0.1, rnd(V) * 0.1
    pp = rnd(B * K, J) * 0.5
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    graph = bias_lib = None
    if not unbiased_only:
        from rnnt_speech_recognition_amd.biasing import ContextGraph

        rng = np.random.default_rng(V)
        phrases = [tuple(int(x) for x in rng.integers(1, V, size=int(rng.integers(2, 7)))) for _ in range(1000)]
        graph = ContextGraph(phrases, boost=1.0, blank=0, vocab_size=V)
        bias_lib = _lib.load_bias()
    ws = torch.empty(_lib.beam_workspace_bytes(T, B, K, J, V, dtype), dtype=torch.uint8, device=DEV)
    parents = torch.empty(B * K, dtype=torch.int32, device=DEV)
    emitted, states = torch.empty_like(parents), torch.empty_like(parents)
    o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, 1)

    def begin():
        _lib.check(lib.compute_rnnt_beam_begin(enc.data_ptr(), frames.data_ptr(), W2.data_ptr(), b2.data_ptr(), J, V, B, K, dtype,
                                               ws.data_ptr(), o), "compute_rnnt_beam_begin")

    def plain():
        _lib.check(lib.compute_rnnt_beam_step(pp.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V, B, K, dtype,
                                              ws.data_ptr(), o), "compute_rnnt_beam_step")

    def biased():
        _lib.check(bias_lib.compute_rnnt_beam_step_biased(pp.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V, B, K,
                                                     dtype, ws.data_ptr(), o, graph.byref(DEV), states.data_ptr()),
                   "compute_rnnt_beam_step_biased")

    out = {"V": V, "joint_dtype": dtype, "B": B, "beam": K, "J": J, "library": _lib.LIB_PATH, "unbiased_ms_per_frame": []}
    legs = [("unbiased_ms_per_frame", plain)]
    if not unbiased_only:
        out.update(graph_states=graph.num_states, graph_arcs=graph.num_arcs, biased_ms_per_frame=[])
        legs.append(("biased_ms_per_frame", biased))
    for _ in range(runs):
        for name, fn in legs:
            begin()
            out[name].append(frames_ms(fn, steps, warmup))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--unbiased-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.LIB_PATH == pkg.LIB_PATH:
        pkg.build()
    lib = _lib.load()
    res = [case(lib, V, dtype, J, a.steps, a.warmup, a.runs, a.unbiased_only) for V, dtype, J in ((28, 0, 640), (4096, 1, 640), (28, 0, 704))]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
