"""What LM shallow fusion costs per frame: compute_rnnt_beam_step (step + select kernels) against compute_rnnt_beam_step_biased
with a 1,000-phrase context graph and compute_rnnt_beam_step_lm with a trigram LM estimated from random sequences, through the C
ABI, device-event times, at B 32, beam 4, joint size 640, for V = 28 (the f32-grade joint) and V = 4096 (the f16 joint).  Each
timed call is one frame of a decode that was begun once; the frame counter runs on, so maxT is sized for warm-up + steps.  A
report, not a gate.  Needs an MI355X.

    python tests/tools/time_lm_fusion.py [--steps 40] [--warmup 10] [--runs 4] [--parent-lib <libwarprnnt.so>] [--out time_lm_fusion.json]

--runs: the legs (unfused, biased, LM and, with --parent-lib, the unfused step of that other build of the base library, loaded
beside this tree's) are timed alternately `runs` times in one process; the spread of the medians is the noise floor."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import rnnt_speech_recognition_amd as pkg  # noqa: E402
from rnnt_speech_recognition_amd import _lib  # noqa: E402
from rnnt_speech_recognition_amd.biasing import ContextGraph  # noqa: E402
from rnnt_speech_recognition_amd.lm import NgramLM  # noqa: E402

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


def case(lib, parent, V, dtype, J, steps, warmup, runs, B=32, K=4):
    T = warmup + steps
    g = torch.Generator(device="cpu").manual_seed(V)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    enc, W2, b2 = rnd(B, T, J) * 0.5, rnd(J, V) * 0.1, rnd(V) * 0.1
    pp = rnd(B * K, J) * 0.5
    frames = torch.full((B,), T, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(V)
    phrases = [tuple(int(x) for x in rng.integers(1, V, size=int(rng.integers(2, 7)))) for _ in range(1000)]
    graph = ContextGraph(phrases, boost=1.0, blank=0, vocab_size=V)
    lm = NgramLM.estimate([[int(x) for x in rng.integers(1, V, size=20)] for _ in range(2000)], 3, 0, V, scale=0.5)
    bias_lib, lm_lib = _lib.load_bias(), _lib.load_lm()
    ws = torch.empty(_lib.beam_workspace_bytes(T, B, K, J, V, dtype), dtype=torch.uint8, device=DEV)
    parents = torch.empty(B * K, dtype=torch.int32, device=DEV)
    emitted, states = torch.empty_like(parents), torch.empty_like(parents)
    o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, 1)

    def begin(base):
        _lib.check(base.compute_rnnt_beam_begin(enc.data_ptr(), frames.data_ptr(), W2.data_ptr(), b2.data_ptr(), J, V, B, K, dtype,
                                                ws.data_ptr(), o), "compute_rnnt_beam_begin")

    def plain(base):
        return lambda: _lib.check(base.compute_rnnt_beam_step(pp.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V,
                                                              B, K, dtype, ws.data_ptr(), o), "compute_rnnt_beam_step")

    def biased():
        _lib.check(bias_lib.compute_rnnt_beam_step_biased(pp.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V, B, K,
                                                          dtype, ws.data_ptr(), o, graph.byref(DEV), states.data_ptr()),
                   "compute_rnnt_beam_step_biased")

    def fused():
        _lib.check(lm_lib.compute_rnnt_beam_step_lm(pp.data_ptr(), parents.data_ptr(), emitted.data_ptr(), None, None, None, J, V, B, K,
                                                    dtype, ws.data_ptr(), o, lm.byref(DEV), states.data_ptr()), "compute_rnnt_beam_step_lm")

    out = {"V": V, "joint_dtype": dtype, "B": B, "beam": K, "J": J, "graph_states": graph.num_states, "graph_arcs": graph.num_arcs,
           "lm_states": lm.num_states, "lm_arcs": lm.num_arcs}
    legs = [("unfused_ms_per_frame", lib, plain(lib)), ("biased_ms_per_frame", lib, biased), ("lm_ms_per_frame", lib, fused)]
    if parent is not None:
        legs.append(("parent_unfused_ms_per_frame", parent, plain(parent)))
    for name, _, _ in legs:
        out[name] = []
    for _ in range(runs):
        for name, base, fn in legs:
            begin(base)
            out[name].append(frames_ms(fn, steps, warmup))
    last = int(states.cpu().max())  # (the LM leg ran last but one or last: its states show the walk was not trivial)
    out["max_state_seen"] = last
    for name, _, _ in legs:
        out[name.replace("_ms_per_frame", "_median_ms")] = float(np.median(out[name]))
    return out


def load_other(path, lib):
    """Another build of the base library beside this tree's, with the two entry points the unfused leg calls."""
    other = ctypes.CDLL(path)
    for name in ("compute_rnnt_beam_begin", "compute_rnnt_beam_step"):
        fn, mine = getattr(other, name), getattr(lib, name)
        fn.restype, fn.argtypes = mine.restype, mine.argtypes
    return other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.LIB_PATH == pkg.LIB_PATH:
        pkg.build()
    lib = _lib.load()
    parent = load_other(a.parent_lib, lib) if a.parent_lib else None
    res = [case(lib, parent, V, dtype, J, a.steps, a.warmup, a.runs) for V, dtype, J in ((28, 0, 640), (4096, 1, 640))]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
