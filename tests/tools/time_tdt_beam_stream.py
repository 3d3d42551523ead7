"""Timings of the streaming TDT beam search (include/rnnt_tdt_beam_stream.h) against the offline one (include/rnnt_tdt_beam.h) at
equal live rows, by the method of tests/tools/time_tdt_beam.py: device events, warm-up, alternating rounds in one process, median
[min .. max].  A tool, not a test.

    python -m tests.tools.time_tdt_beam_stream [--out FILE] [--quick]
    python -m tests.tools.time_tdt_beam_stream --trace      # no timing: two short decodes of each route, to run under a kernel trace
    python -m tests.tools.time_tdt_beam_stream --stats DIR  # median [min .. max] per kernel from a kernel trace's CSV files under DIR

S = B = 64 streams, beam 4 (256 rows), V = 1024, D as given, H = J = 640, 40 frames in ONE chunk with N = max_hyp_len = 40 = maxT:
the shapes of the per-kernel table of profiles/tdt_beam_notes.md.  The joints alone are stepped, on fixed random pred_proj rows (no
prediction network): per frame one step call = the step kernel + the select kernel.  durations [1]: every occupied row is active
at every frame on both routes (equal live rows by construction); durations [0, 1, 2, 3, 4]: the two routes' enc_proj differ in the
last bits (torch's GEMM against the stream's FMA chain), so their beams may drift apart -- a second, looser comparison.
Reported: microseconds per frame of the step call on each route, and of one feed (projection + tables + slot state) of the stream,
whole and per frame of the chunk."""
import argparse
import csv
import glob
import json
import os
import statistics

import torch

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import tdt

DEV = "cuda:0"
H = J = 640
S, K, V, T = 64, 4, 1024, 40
SETS = {"durations [1]": [1], "durations [0, 1, 2, 3, 4]": [0, 1, 2, 3, 4]}


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def _setup(durations, seed=0):
    torch.manual_seed(seed)
    jt = pkg.JointLoss(H, J, V + len(durations)).to(DEV)
    with torch.no_grad():
        jt.W2.mul_(6.0)
        jt.b2[0] += 3.0  # (blanks and tokens both occur with random weights)
    enc = torch.randn(S, T, H, device=DEV)
    off = tdt.TDTBeamJoint(jt, durations, K)
    st = tdt.TDTBeamStreamJoint(jt, durations, K)
    assert off.engine and st.engine
    pp = torch.randn(S * K, off.Jp, device=DEV)
    frames = torch.full((S,), T, dtype=torch.int32, device=DEV)
    ones = torch.ones(S, dtype=torch.int32, device=DEV)
    st.begin(S, T, T)
    return off, st, enc, pp, frames, ones


def _steps(j, pp):
    for _ in range(T):
        j.step(pred_proj=pp)


def _stats(root):
    rows = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].split("(")[0]
            if "tdt_beam" in name or "greedy_stream_proj" in name:
                rows.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, v in sorted(rows.items()):
        print(f"{name}: {statistics.median(v):.1f} [{min(v):.1f} .. {max(v):.1f}] us  calls={len(v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="5 rounds instead of 11")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        return _stats(a.stats)
    pkg.build()
    rows = {}
    for tag, durations in SETS.items():
        off, st, enc, pp, frames, ones = _setup(durations)
        routes = {
            "offline begin (torch enc_proj + tables)": lambda: off.begin(enc, frames),
            "offline step call x 40": lambda: _steps(off, pp),
            "stream feed (40 frames)": lambda: st.feed(enc, frames, reset=ones, final=ones),
            "stream step call x 40": lambda: _steps(st, pp),
        }
        for _ in range(2):  # warm-up: allocations, workspaces, code objects
            for fn in routes.values():
                fn()
        if a.trace:
            continue
        times = {k: [] for k in routes}
        for _ in range(5 if a.quick else 11):
            for k, fn in routes.items():  # (begin / feed restart the decode its steps then run)
                times[k].append(_events(fn))
        for k, v in times.items():
            med = statistics.median(v)
            rows[f"{tag} | {k}"] = dict(median_us=med, min_us=min(v), max_us=max(v), per_frame_us=med / T)
            print(f"{tag} | {k}: {med:.1f} [{min(v):.1f} .. {max(v):.1f}] us  {med / T:.2f} us per frame", flush=True)
    torch.cuda.synchronize()
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
