"""GPU tests of the streaming log-mel front end: compute_rnnt_frontend_begin / _feed through features.StreamingFrontEnd, the
same cases as tests/test_stream_frontend.py runs on the torch route, HIP-graph replay, and StreamingTranscriber end to end."""
import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import _lib, features
from tests import frontend_cases as fc
from tests import test_stream_frontend as cpu

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu


def test_rows_match_the_float64_restatement_and_the_oracle():
    fc.check_parity(DEV)
    fc.check_parity(DEV, engine=False)  # the torch route on the GPU (the probe's baseline)


def test_zero_audio_gives_exactly_log_1e_6():
    fc.check_zero_audio(DEV)
    fc.check_zero_audio(DEV, engine=False)


@pytest.mark.parametrize("rm", [1, 2, 4])
def test_a_stream_is_bitwise_independent_of_chunking_slot_and_neighbours(rm):
    fc.check_chunking_invariance(DEV, rm)


def test_state_machine():
    fc.check_state_machine(DEV)


def test_step_equal_to_length_and_other_fft_sizes():
    fc.check_other_shapes(DEV)


def test_engine_and_torch_route_agree():
    audio = fc.signal(0.9, seed=8)
    a, ca, _, fa = fc.feed_stream(audio, fc.ragged_chunks(len(audio), seed=4), fc.hparams(), 16000, 2, "running", DEV, slots=3, slot=1,
                                  neighbours=True, max_chunk=3000)
    b, cb, _, fb = fc.feed_stream(audio, fc.ragged_chunks(len(audio), seed=4), fc.hparams(), 16000, 2, "running", DEV, slots=3, slot=1,
                                  neighbours=True, max_chunk=3000, engine=False)
    assert fa.engine and fa.route == "engine" and not fb.engine and ca == cb
    assert float((a - b).abs().max()) < fc.BAR


def test_a_feed_replays_from_a_hip_graph_bit_for_bit():
    """Two feeds recorded into a HIP graph and replayed on new audio give bitwise what direct calls give: nothing in the
    library allocates or synchronises, and the state lives in the workspace."""
    lib = _lib.load()
    S, K, L, step, M, stack, rm = 4, 2000, 400, 160, 80, 3, 2
    fe = features.StreamingFrontEnd(fc.hparams(), 16000, S, K, rm, device=DEV)  # (its tables; the graph runs on a workspace of its own)
    shape = (K, S, L, step, M, stack, rm)
    R, F = fe.max_rows, M * stack
    audio = torch.zeros(2, S, K, device=DEV)
    samples = torch.tensor([[K, 1000, 0, 1999], [1500, K, 700, 1]], dtype=torch.int32, device=DEV)
    reset = torch.tensor([[1, 1, 1, 1], [0, 0, 0, 0]], dtype=torch.int32, device=DEV)
    final = torch.tensor([[0, 0, 0, 0], [1, 0, 1, 0]], dtype=torch.int32, device=DEV)
    rows, counts = torch.empty(2, S, R, F, device=DEV), torch.empty(2, S, dtype=torch.int32, device=DEV)
    ws = torch.empty(_lib.frontend_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)

    def call(stream):
        opts = _lib.make_options(stream.cuda_stream, 0, 1, 1)
        _lib.check(lib.compute_rnnt_frontend_begin(fe.window.data_ptr(), fe.mel_w.data_ptr(), *shape, ws.data_ptr(), opts), "begin")
        for i in range(2):
            _lib.check(lib.compute_rnnt_frontend_feed(audio[i].data_ptr(), K, samples[i].data_ptr(), reset[i].data_ptr(),
                                                      final[i].data_ptr(), 1, rows[i].data_ptr(), counts[i].data_ptr(), *shape,
                                                      ws.data_ptr(), opts), "feed")

    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        call(side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(torch.cuda.current_stream())
    for seed in (3, 4):
        audio.copy_(torch.tensor(np.random.default_rng(seed).normal(size=(2, S, K)).astype(np.float32) * 0.2))
        graph.replay()
        torch.cuda.synchronize()
        got_rows, got_counts = rows.clone(), counts.clone()
        rows.fill_(-1.0), counts.fill_(-1)
        call(torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert torch.equal(got_counts, counts) and torch.equal(got_rows, rows) and int(counts.sum()) > 0


@pytest.mark.parametrize("beam", [None, 4])
def test_transcriber_is_chunking_invariant_and_matches_the_batched_decoders(beam):
    cpu.fc_e2e(DEV, beam)
