"""Generates tests/golden/beam/beam_offline.npz: what compute_rnnt_beam_begin / _step / _results of the library write for seeded
inputs, recorded from the library as it stood before the beam kernels learnt a token stride and a persistent step counter
(the streaming beam search).  tests/test_streaming_beam_gpu.py replays the same calls and wants every output bit for bit: the
offline entry points' instruction stream may change, their outputs may not.

Needs an MI355X.  Run it on the commit to record from, or point RNNT_LIBWARPRNNT at a library built from that commit:
    python tests/golden/make_beam_offline_goldens.py
The inputs come from numpy's default_rng (stable across versions) and are not stored; only the outputs are."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "beam", "beam_offline.npz")

# (joint_dtype, J, V, B, K, T)
CASES = [
    (0, 64, 12, 3, 1, 6),
    (0, 640, 28, 2, 4, 7),
    (0, 64, 128, 3, 16, 6),
    (0, 704, 28, 2, 4, 5),
    (1, 128, 128, 3, 1, 6),
    (1, 640, 4096, 2, 4, 7),
    (1, 256, 1000, 3, 16, 6),
    (1, 128, 1024, 5, 16, 9),
]


def inputs(case):
    """enc_proj [B, T, J], frame_lengths [B], pred_proj per step [T, B K, J], W2 [J, V], b2 [V] of CASES[case]."""
    dtype, J, V, B, K, T = CASES[case]
    rng = np.random.default_rng(7700 + case)
    enc = rng.normal(size=(B, T, J)).astype(np.float32)
    pred = rng.normal(size=(T, B * K, J)).astype(np.float32)
    if B * K > 2:  # one enc row and one pred row beyond the e^{2x} table range: both tanh routes
        enc[1 % B, 0] *= 60.0
        pred[1, 2] *= 60.0
    W2 = (rng.uniform(-1, 1, size=(J, V)) * (6.0 / (J + V)) ** 0.5 * (3.0 if dtype == 0 else 12.0)).astype(np.float32)
    b2 = (0.1 * rng.normal(size=V)).astype(np.float32)
    b2[0] += 1.0  # blank competes: beams hold sequences of several lengths
    frames = np.full(B, T, np.int32)
    if B > 1:
        frames[1] = T - 3  # ragged; B > 2: one empty utterance
    if B > 2:
        frames[2] = 0
    return enc, frames, pred, W2, b2


def run(case):
    """The decode of CASES[case] through the C ABI on cuda:0, in a workspace pre-filled with 0xFF bytes -> dict of arrays."""
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from rnnt_speech_recognition_amd import _lib

    dev = torch.device("cuda:0")
    dtype, J, V, B, K, T = CASES[case]
    enc, frames, pred, W2, b2 = (torch.from_numpy(x).to(dev).contiguous() for x in inputs(case))
    R = B * K
    lib = _lib.load()
    o = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, 1)
    ws = torch.full((_lib.beam_workspace_bytes(T, B, K, J, V, dtype),), 0xFF, dtype=torch.uint8, device=dev)
    _lib.check(lib.compute_rnnt_beam_begin(enc.data_ptr(), frames.data_ptr(), W2.data_ptr(), b2.data_ptr(), J, V, B, K, dtype,
                                           ws.data_ptr(), o), "compute_rnnt_beam_begin")
    out = {k: [] for k in ("parents", "emitted", "topl", "tops", "lse", "hyps", "lengths", "scores")}
    for t in range(T):
        parents, emitted = (torch.full((R,), -9, dtype=torch.int32, device=dev) for _ in range(2))
        tl = torch.full((R, K), -123.0, device=dev)
        ts = torch.full((R, K), -7, dtype=torch.int32, device=dev)
        lse = torch.full((R,), -123.0, device=dev)
        _lib.check(lib.compute_rnnt_beam_step(pred[t].data_ptr(), parents.data_ptr(), emitted.data_ptr(), tl.data_ptr(),
                                              ts.data_ptr(), lse.data_ptr(), J, V, B, K, dtype, ws.data_ptr(), o),
                   "compute_rnnt_beam_step")
        hyps = torch.full((B, K, T), -9, dtype=torch.int32, device=dev)
        lengths = torch.full((B, K), -9, dtype=torch.int32, device=dev)
        scores = torch.full((B, K), -123.0, device=dev)
        _lib.check(lib.compute_rnnt_beam_results(hyps.data_ptr(), lengths.data_ptr(), scores.data_ptr(), J, V, B, K, dtype,
                                                 ws.data_ptr(), o), "compute_rnnt_beam_results")
        torch.cuda.synchronize()
        for k, v in zip(out, (parents, emitted, tl, ts, lse, hyps, lengths, scores)):
            out[k].append(v.cpu().numpy())
    return {k: np.stack(v) for k, v in out.items()}


def bits(x):
    """float arrays as their bit patterns (NaN payloads and signed zeros compare too)"""
    return x.view(np.int32) if x.dtype == np.float32 else x


if __name__ == "__main__":
    rec = {}
    for c in range(len(CASES)):
        r = run(c)
        rec.update({f"c{c}_{k}": v for k, v in r.items()})
        print(c, CASES[c], "emitted", int((r["emitted"] >= 0).sum()), "max length", int(r["lengths"].max()))
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **rec)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
