"""Greedy transducer decoding (reference utils/decoding.py:6-108).

Behaviour kept from the reference:
  * only the FIRST utterance of the batch is decoded (utils/decoding.py:22,35);
  * the hypothesis starts with the blank/start token 0 (:28) and the returned ids drop it (:102);
  * per encoder frame, symbols are emitted until the joint's argmax is blank (id 0) (:61-76); there is no
    per-frame symbol cap, only the global `max_length` (:78-79): once max_length symbols exist, decoding stops;
  * the encoder runs in inference mode (BatchNorm statistics frozen, no dropout) (:37,63).
The reference re-runs the prediction network over the whole hypothesis for every joint evaluation (:63-64); it is a
causal LSTM stack, so carrying its state forward gives the same outputs at O(1) per symbol.  `stateless=True` keeps
the reference's formulation (used by the tests as the cross-check).

The joint is evaluated for ONE lattice cell at a time (T = U = 1), as the reference does (`joint`, utils/decoding.py:6-18).
On the device it goes through the engine's logits-only entry point (compute_rnnt_joint_logits via JointLoss.cell_logits):
the forward kernels of the fused loss, so the decoder sees the logits the loss was trained on.

greedy_decode_batch decodes EVERY utterance of a batch with the same per-utterance semantics: one decode step per decision
for all hypotheses at once, the joint + argmax + state update in one library call (compute_rnnt_greedy_step), no host sync
per step."""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from .joint import (BeamJoint, BeamStreamJoint, EncoderStream, GreedyJoint, GreedyStreamJoint, MultiBeamJoint, MultiBeamStreamJoint,
                    PredictionStep, TorchPredictionStep, _pred_step)  # noqa: F401  (_pred_step: one symbol through the prediction network, for callers of this module)
from .loss import reduced_lengths


@torch.no_grad()
def greedy_decode(model, mel_specs: torch.Tensor, max_length: Optional[int] = None, stateless: bool = False) -> torch.Tensor:
    """mel_specs [B, T, F] -> int32 ids [1, n] of the first utterance (blank-free, start token removed)."""
    was_training = model.training
    model.eval()
    try:
        x = mel_specs[:1]
        enc = model.encoder(x)  # [1, T', H]
        dev = enc.device
        hyp: List[int] = [0]
        pred_net = model.prediction
        joint = model.joint

        # incremental prediction-network state: one (h, c) per LSTM block
        states = [None] * len(pred_net.blocks)

        def pred_last_incremental(token: int) -> torch.Tensor:
            y = pred_net.embed(torch.tensor([[token]], device=dev))
            for i, blk in enumerate(pred_net.blocks):
                y, states[i] = blk.lstm(y, states[i])
                y = blk.norm(blk.drop(y))
            return y  # [1, 1, H]

        def pred_last_stateless() -> torch.Tensor:
            return pred_net(torch.tensor([hyp], device=dev))[:, -1:, :]

        g = pred_last_stateless() if stateless else pred_last_incremental(0)
        max_reached = False
        for i in range(enc.shape[1]):
            if max_reached:
                break
            f = enc[:, i : i + 1, :]
            while True:
                # (consumed by the argmax below before the next call: the engine may hand out its cached buffer)
                logits = joint.cell_logits(f, g, reuse_buffers=True)[0, 0, 0]  # [V]
                k = int(torch.argmax(torch.log_softmax(logits, dim=-1)).item())
                if k == joint.blank_label:
                    break
                hyp.append(k)
                g = pred_last_stateless() if stateless else pred_last_incremental(k)
                if max_length is not None and len(hyp) >= max_length + 1:
                    max_reached = True
                    break
        return torch.tensor([hyp[1:]], dtype=torch.int32, device=dev)
    finally:
        model.train(was_training)


def greedy_decode_fn(model):
    """The reference's factory shape: greedy_decode_fn(model, hparams) -> fn(inputs, max_length)."""
    def fn(inputs: torch.Tensor, max_length: Optional[int] = None) -> torch.Tensor:
        return greedy_decode(model, inputs, max_length)
    return fn


# ---------------------------------------------------------------------------------------------------------------------------
# Batched greedy decoding
# ---------------------------------------------------------------------------------------------------------------------------
CHECK_EVERY = 32  # decode steps between two reads of the all-done word (the only host reads of the loop)
_WORKSPACES = {}  # (device, stream) -> the greedy workspace of the last decode there
LAST_STEPS = 0    # decode steps the last greedy_decode_batch / greedy_search_batch took (timing tools)


def read_flag(x: torch.Tensor) -> int:
    """The loop's one host read (the all-done word, or a length bound), with torch's sync debug mode lowered around it."""
    mode = torch.cuda.get_sync_debug_mode() if x.is_cuda else 0
    if mode:
        torch.cuda.set_sync_debug_mode(0)
    try:
        return int(x.reshape(-1)[0].item())
    finally:
        if mode:
            torch.cuda.set_sync_debug_mode(mode)


def _stream_key(x: torch.Tensor, *extra):
    """The key of the per-stream workspace caches: (device, stream) + extra for a device tensor, None for a CPU tensor."""
    return (x.device, torch.cuda.current_stream(x.device).cuda_stream) + extra if x.is_cuda else None


def _begin_cached(cache: dict, key, obj, *args):
    """obj.begin(*args) on the workspace that `cache` holds under `key` -- the one of the last decode on this stream, which
    begin keeps when it is large enough (joint._workspace); the workspace obj has afterwards is held for the next one."""
    obj._ws = cache.get(key)
    out = obj.begin(*args)
    if key is not None and obj._ws is not None:
        cache[key] = obj._ws
    return out


_PRED_WORKSPACES = {}  # (device, stream) -> the prediction-network workspace of the last engine-route decode there
PREDICTIONS = ("torch", "engine")


def _joint_W1(jx):
    """The first Dense layer a PredictionStep for the joint jx projects through: the engine joint's, padded to its joint units;
    the torch joint takes the model's J."""
    return jx.W1 if jx.engine else jx.joint.W1


def _prediction_step(pred_net, W1: torch.Tensor, rows: int):
    """The engine route's PredictionStep of the prediction network pred_net through W1, begun for `rows` rows -> (step, pred_proj)."""
    ps = PredictionStep(pred_net, W1)
    return ps, _begin_cached(_PRED_WORKSPACES, _stream_key(ps.W1), ps, rows)


def _begin_prediction(route: str, pred_net, jx, rows: int, dev):
    """The prediction network of the joint jx's `rows` rows after the start token -> (stepper, its output).  "engine": a
    PredictionStep, the output through W1 (the joint step's pred_proj=); "torch": the model's own modules, the output as it is
    (the joint step's pred, which projects it itself)."""
    if route == "engine":
        return _prediction_step(pred_net, _joint_W1(jx), rows)
    ps = TorchPredictionStep(pred_net, dev)
    return ps, ps.begin(rows)


def _joint_step(jx, ps):
    return (lambda x: jx.step(pred_proj=x)) if ps.projected else jx.step


def _greedy_loop(jg, ps, x, check_every: int, carry: bool):
    """The greedy decoders' loop on a begun joint jg and a begun prediction stepper ps with the output x: joint step,
    prediction-network step for the rows that emitted, and every `check_every` joint steps one read of the all-done word -- 1 ends
    the loop, 2 (every running hypothesis has filled the buffer) grows the buffer.  carry False (a batch): the prediction network
    steps after the read, and not after the last joint step.  carry True (a stream): it steps before the read, after the last
    joint step too: the next feed goes on from it.  -> (joint steps, the stepper's last output)."""
    step = _joint_step(jg, ps)
    steps = 0
    while True:
        emitted = step(x)
        steps += 1
        if carry:
            x = ps.step(emitted)
        if steps % check_every == 0:
            flag = read_flag(jg.all_done)
            if flag == 1:
                return steps, x
            if flag == 2:
                jg.grow_hyps()
        if not carry:
            x = ps.step(emitted)


def _beam_loop(jb, ps, x, steps: int, carry: bool, before_step=None):
    """The beam decoders' loop, frame-synchronous (nothing is read from the host): `steps` joint steps, each followed by a
    prediction-network step from the parents' states -- but for the last one unless carry (a stream: the next feed goes on from
    it).  before_step(t), when given, runs before joint step t.  -> the stepper's last output."""
    step = _joint_step(jb, ps)
    for t in range(steps):
        if before_step is not None:
            before_step(t)
        parents, emitted = step(x)
        if carry or t + 1 < steps:
            x = ps.step(emitted, parents)
    return x


def _check_prediction(prediction: str):
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction must be one of {PREDICTIONS}, got {prediction!r}")


_ENC_WORKSPACES = {}  # (device, stream) -> the encoder workspace of the last engine-route decode there
ENCODERS = ("torch", "engine")


def _check_encoder(encoder: str):
    if encoder not in ENCODERS:
        raise ValueError(f"encoder must be one of {ENCODERS}, got {encoder!r}")


def _encode(model, mel_specs: torch.Tensor, encoder: str) -> torch.Tensor:
    """The encoder output of every row: model.encoder (encoder="torch") or one EncoderStream run (encoder="engine")."""
    if encoder == "torch":
        return model.encoder(mel_specs)
    es = EncoderStream(model.encoder)
    _begin_cached(_ENC_WORKSPACES, _stream_key(mel_specs) if es.engine else None, es, mel_specs.shape[0], mel_specs.shape[1])
    return es.run(mel_specs)


def _greedy_search(jg, cache: dict, pred_net, enc, frame_lengths, max_length, max_per_frame: int, check_every: int, prediction: str):
    """The batched greedy search on the fresh joint jg (its workspace from `cache`) -> (jg's results, the decode steps)."""
    B, T = enc.shape[0], enc.shape[1]
    dev = enc.device
    if max_length is None:
        maxsym, N = None, T + 16  # no bound (the reference's): the buffer grows when a hypothesis fills it
    elif isinstance(max_length, torch.Tensor):
        maxsym = max_length.to(device=dev, dtype=torch.int32).reshape(B)
        N = max(1, read_flag(maxsym.max().reshape(1)))
    else:
        maxsym = torch.full((B,), int(max_length), dtype=torch.int32, device=dev)
        N = max(1, int(max_length))
    _begin_cached(cache, _stream_key(enc), jg, enc, frame_lengths, maxsym, max_per_frame, N)
    ps, x = _begin_prediction(prediction, pred_net, jg, B, dev)
    steps, _ = _greedy_loop(jg, ps, x, check_every, carry=False)
    out = (jg.hyps, jg.lengths, jg.scores)
    return (out + (jg.frames, jg.logp) if jg.token_times else out), steps


@torch.no_grad()
def greedy_search_batch(model, enc: torch.Tensor, frame_lengths: torch.Tensor, max_length=None,
                        max_symbols_per_frame: Optional[int] = None, check_every: int = CHECK_EVERY, prediction: str = "torch",
                        token_times: bool = False):
    """Greedy search over encoder outputs enc [B, T', H] with frame_lengths [B] (the model in eval mode).  See greedy_decode_batch."""
    global LAST_STEPS
    _check_prediction(prediction)
    # (the current weights: a model may be trained between two decodes)
    jg = GreedyJoint(model.joint, token_times=True) if token_times else GreedyJoint(model.joint)
    out, LAST_STEPS = _greedy_search(jg, _WORKSPACES, model.prediction, enc, frame_lengths, max_length,
                                     int(max_symbols_per_frame or 0), check_every, prediction)
    return out


@torch.no_grad()
def greedy_decode_batch(model, mel_specs: torch.Tensor, spec_lengths: Optional[torch.Tensor] = None, max_length=None,
                        max_symbols_per_frame: Optional[int] = None, check_every: int = CHECK_EVERY, prediction: str = "torch",
                        encoder: str = "torch", token_times: bool = False):
    """Greedy decoding of EVERY utterance of a batch at once -> (ids int32 [B, N] zero-padded, lengths int32 [B], scores [B]).

    Per utterance the semantics of greedy_decode (utils/decoding.py:21-108): the hypothesis starts from token 0, symbols are
    emitted at a frame until the joint's argmax is joint.blank_label, then the next frame.  max_length (an int, or an int tensor
    [B]) bounds the symbols of an utterance (max_length = 0: none; greedy_decode stops only after its first symbol there);
    max_symbols_per_frame, when given, moves to the next frame after that many symbols at one frame (None: no cap, as the
    reference).  spec_lengths are spectrogram frames, reduced as Transducer.loss reduces them; None: every frame of every row.
    scores[b] = the sum of the log-softmax of every decision taken for utterance b (float32 on the engine; the model's dtype on
    the torch route).

    The prediction network steps all B rows at once (rows that emitted nothing keep their state), and on an MI355X the joint is
    the library's greedy step (GreedyJoint): no host synchronisation per step -- the all-done word is read every
    `check_every` steps (read_flag).  prediction="engine" steps the prediction network in the library too (PredictionStep:
    compute_rnnt_prednet_step, through W1 into the joint step), so that the loop body is library calls alone; "torch" (the
    default) steps it with the model's own modules.  encoder="engine" runs the encoder in the library (EncoderStream:
    compute_rnnt_encoder_run, every row in one call); "torch" (the default) runs model.encoder.

    token_times=True returns (ids, lengths, scores, frames int32 [B, N], logp [B, N]): per token the 0-based encoder frame whose
    joint evaluation emitted it (-1 past the hypothesis) and the log-softmax of that decision (0 past it) -- the convention of
    alignment.rnnt_align's token_frames / token_logp, so alignment.token_times and word_times apply.  ids, lengths and scores
    are bitwise those of token_times=False."""
    _check_prediction(prediction)
    _check_encoder(encoder)
    was_training = model.training
    model.eval()
    try:
        enc = _encode(model, mel_specs, encoder)  # [B, T', H]
        B, T = enc.shape[0], enc.shape[1]
        if spec_lengths is None:
            frames = torch.full((B,), T, dtype=torch.int32, device=enc.device)
        else:
            frames = reduced_lengths(spec_lengths.to(enc.device), model.hp.time_reduction_factor)
        if token_times:
            return greedy_search_batch(model, enc, frames, max_length, max_symbols_per_frame, check_every, prediction, True)
        return greedy_search_batch(model, enc, frames, max_length, max_symbols_per_frame, check_every, prediction)
    finally:
        model.train(was_training)


def greedy_decode_batch_fn(model, prediction: str = "torch", encoder: str = "torch"):
    """fn(inputs, max_length=None, spec_lengths=None) -> (ids, lengths, scores) of greedy_decode_batch."""
    _check_prediction(prediction)
    _check_encoder(encoder)

    def fn(inputs: torch.Tensor, max_length=None, spec_lengths: Optional[torch.Tensor] = None):
        return greedy_decode_batch(model, inputs, spec_lengths, max_length, prediction=prediction, encoder=encoder)
    return fn


# ---------------------------------------------------------------------------------------------------------------------------
# Batched beam search
# ---------------------------------------------------------------------------------------------------------------------------
_BEAM_WORKSPACES = {}  # (device, stream) -> the beam workspace of the last decode there


def _beam_search(jb, cache: dict, pred_net, enc, frame_lengths, prediction: str, before_step=None):
    """The batched beam search on the fresh joint jb (its workspace from `cache`; a timed decode keeps one of its own) -> jb's
    results.  before_step: _beam_loop's."""
    key = _stream_key(enc, "timed") if jb.token_times else _stream_key(enc)
    _begin_cached(cache, key, jb, enc, frame_lengths)
    ps, x = _begin_prediction(prediction, pred_net, jb, enc.shape[0] * jb.K, enc.device)
    _beam_loop(jb, ps, x, enc.shape[1], carry=False, before_step=before_step)
    return jb.results()


_MULTIBEAM_WORKSPACES = {}  # (device, stream) -> the workspace of the last several-symbols-per-frame decode there


def _multibeam_search(jm, cache: dict, pred_net, enc, frame_lengths, prediction: str):
    """The batched beam search with several symbols per frame on the fresh joint jm (its workspace from `cache`) -> jm's results:
    T' (E + 1) steps of _beam_loop over B 2 beam rows."""
    _begin_cached(cache, _stream_key(enc), jm, enc, frame_lengths)
    ps, x = _begin_prediction(prediction, pred_net, jm, enc.shape[0] * 2 * jm.K, enc.device)
    _beam_loop(jm, ps, x, enc.shape[1] * (jm.E + 1), carry=False)
    return jm.results()


@torch.no_grad()
def beam_search_batch(model, enc: torch.Tensor, frame_lengths: torch.Tensor, beam: int = 4, prediction: str = "torch",
                      token_times: bool = False, context=None, lm=None, symbols_per_frame: Optional[int] = None,
                      max_length: Optional[int] = None):
    """Modified beam search (one symbol per frame) over encoder outputs enc [B, T', H] with frame_lengths [B] (the model in eval
    mode) -> (ids int32 [B, beam, T'] zero-padded, lengths int32 [B, beam], scores [B, beam]): every utterance's n-best, sorted
    by score (empty slots: length 0, score -inf).  See include/rnnt.h for the algorithm; beam = 1 is greedy_search_batch with
    max_symbols_per_frame = 1.

    Runs enc.shape[1] steps without reading the host.  Per step the prediction network runs on all B beam rows; its output and
    LSTM state are gathered by `parents`, and the rows that emitted a symbol advance.  prediction="engine": that step is the
    library's (PredictionStep), as in greedy_search_batch.

    token_times=True returns two more: frames int32 [B, beam, T'] (-1 padded) and logp [B, beam, T'] (0 padded), per token the
    frame that emitted it and the log-softmax of that decision.  Where identical sequences were merged, the hypothesis keeps
    the frames and log-probabilities of its first-ranked member; its score still sums the members.

    context=biasing.ContextGraph: contextual biasing (hotword boosting).  Candidates are ranked with the graph's bonus, the
    scores include it, and the results are finalised -- a hypothesis that ends in the middle of a phrase gives back what it has
    not earned -- and re-sorted (stably) by the finalised score.  logp stays the model's log-probability.

    lm=lm.NgramLM: shallow fusion of a back-off n-gram LM (in place of a context: both together raise).  Candidates are ranked
    with the LM's score of the token (already scaled by the LM weight), the scores include it, and the results are finalised with
    the LM's end-of-sentence score and re-sorted (stably).  logp stays the model's log-probability.

    symbols_per_frame=E (an integer 1 ... 8; None: the search above, untouched): the time-synchronous search of
    include/rnnt_beam_multi.h on the STANDARD lattice -- up to E symbols per frame, which is what a model trained with rnnt_loss may
    need (more labels than frames included).  It runs T' (E + 1) steps on B 2 beam rows (MultiBeamJoint) and returns ids int32
    [B, beam, max_hyp_len], max_hyp_len = max_length or T' E: a hypothesis of max_hyp_len tokens emits no more.  token_times,
    context and lm raise together with it."""
    _check_prediction(prediction)
    if symbols_per_frame is not None:
        if token_times or context is not None or lm is not None:
            raise ValueError("symbols_per_frame= takes no token_times, context or lm")
        jm = MultiBeamJoint(model.joint, int(beam), int(symbols_per_frame), max_length)
        return _multibeam_search(jm, _MULTIBEAM_WORKSPACES, model.prediction, enc, frame_lengths, prediction)
    if max_length is not None:
        raise ValueError("max_length= bounds the hypotheses of the search with symbols_per_frame= alone")
    # (the current weights: a model may be trained between two decodes)
    jb = BeamJoint(model.joint, int(beam), token_times=bool(token_times), context=context, lm=lm)
    return _beam_search(jb, _BEAM_WORKSPACES, model.prediction, enc, frame_lengths, prediction)


@torch.no_grad()
def beam_decode_batch(model, mel_specs: torch.Tensor, spec_lengths: Optional[torch.Tensor] = None, beam: int = 4,
                      prediction: str = "torch", encoder: str = "torch", token_times: bool = False, context=None,
                      lm=None, symbols_per_frame: Optional[int] = None):
    """Beam search of EVERY utterance of a batch -> the best hypothesis of each: (ids int32 [B, T'] zero-padded, lengths int32
    [B], scores [B]).  spec_lengths are spectrogram frames, reduced as greedy_decode_batch reduces them; None: every frame.
    encoder= as in greedy_decode_batch.  token_times=True: (ids, lengths, scores, frames int32 [B, T'], logp [B, T']) of the
    best hypothesis, as beam_search_batch defines them.  context= and lm= as in beam_search_batch.  symbols_per_frame=E: the
    search with up to E symbols per frame (beam_search_batch); ids is then [B, T' E]."""
    _check_prediction(prediction)
    _check_encoder(encoder)
    was_training = model.training
    model.eval()
    try:
        enc = _encode(model, mel_specs, encoder)  # [B, T', H]
        B, T = enc.shape[0], enc.shape[1]
        if spec_lengths is None:
            frames = torch.full((B,), T, dtype=torch.int32, device=enc.device)
        else:
            frames = reduced_lengths(spec_lengths.to(enc.device), model.hp.time_reduction_factor)
        if symbols_per_frame is not None:
            ids, lengths, scores = beam_search_batch(model, enc, frames, beam, prediction, token_times, context=context, lm=lm,
                                                     symbols_per_frame=symbols_per_frame)
            return ids[:, 0], lengths[:, 0], scores[:, 0]
        if token_times:
            return tuple(x[:, 0] for x in beam_search_batch(model, enc, frames, beam, prediction, True, context=context, lm=lm))
        ids, lengths, scores = beam_search_batch(model, enc, frames, beam, prediction, context=context, lm=lm)
        return ids[:, 0], lengths[:, 0], scores[:, 0]
    finally:
        model.train(was_training)


def beam_decode_batch_fn(model, beam: int = 4, prediction: str = "torch", encoder: str = "torch"):
    """fn(inputs, max_length=None, spec_lengths=None) -> (ids, lengths, scores) of beam_decode_batch, for
    metrics.build_batch_accuracy_fn / build_batch_wer_fn.  The search has no symbol budget: max_length (an int or an int tensor
    [B]) truncates the best hypothesis afterwards."""
    _check_prediction(prediction)
    _check_encoder(encoder)

    def fn(inputs: torch.Tensor, max_length=None, spec_lengths: Optional[torch.Tensor] = None):
        ids, lengths, scores = beam_decode_batch(model, inputs, spec_lengths, beam, prediction, encoder)
        if max_length is not None:
            cap = torch.as_tensor(max_length, device=lengths.device).to(torch.int32)
            lengths = torch.minimum(lengths, cap)
            ids = torch.where(torch.arange(ids.shape[1], device=ids.device)[None, :] < lengths[:, None], ids, torch.zeros_like(ids))
        return ids, lengths, scores
    return fn


# ---------------------------------------------------------------------------------------------------------------------------
# Streaming greedy decoding
# ---------------------------------------------------------------------------------------------------------------------------
class _StreamingSlots:
    """What the streaming decoders share: the slots' encoder stream, the slot masks of start() and the argument checks of feed()."""

    def _init_slots(self, model, slots: int, max_chunk_frames: int) -> None:
        S, Tc = int(slots), int(max_chunk_frames)
        if not 1 <= S <= EncoderStream.MAX_ROWS:
            raise ValueError(f"slots must be in 1 ... {EncoderStream.MAX_ROWS}, got {slots}")
        if Tc < 1:
            raise ValueError(f"max_chunk_frames must be >= 1, got {max_chunk_frames}")
        self.model, self.S, self.Tc = model, S, Tc
        enc = model.encoder
        self.f = int(enc.reduce.factor)
        self.F = int(enc.input_norm.num_features)
        last = enc.blocks[len(enc.blocks) - 1].lstm
        self.H = int(last.proj_size or last.hidden_size)
        self.Te = -(-Tc // self.f)
        with self._eval():
            self.es = EncoderStream(enc)
            self.es.begin(S, Tc)
        self._pending = [False] * S  # encoder resets waiting for the next run

    class _EvalMode:
        def __init__(self, model):
            self.model = model

        def __enter__(self):
            self.was = self.model.training
            self.model.eval()

        def __exit__(self, *exc):
            self.model.train(self.was)

    def _eval(self):
        return self._EvalMode(self.model)

    def _mask(self, slots):
        t = torch.as_tensor(slots)
        if t.dtype == torch.bool:
            if t.numel() != self.S:
                raise ValueError(f"a slot mask must have {self.S} entries, got {t.numel()}")
            return [bool(v) for v in t.reshape(-1).tolist()]
        m = [False] * self.S
        for s in t.reshape(-1).tolist():
            if not 0 <= int(s) < self.S:
                raise ValueError(f"slot {s} is not in 0 ... {self.S - 1}")
            m[int(s)] = True
        return m

    def _check_feed(self, mel_chunk, frames, final):
        """feed()'s arguments -> (frames, final) as host lists of ints / bools."""
        S, f = self.S, self.f
        if mel_chunk.dim() != 3 or mel_chunk.shape[0] != S or mel_chunk.shape[2] != self.F:
            raise ValueError(f"mel_chunk must be [{S}, frames, {self.F}], got {tuple(mel_chunk.shape)}")
        Tc = int(mel_chunk.shape[1])
        if Tc > self.Tc:
            raise ValueError(f"mel_chunk has {Tc} frames; this decoder takes at most max_chunk_frames = {self.Tc}")
        fr = [int(v) for v in torch.as_tensor(frames).reshape(-1).tolist()]
        fi = [bool(v) for v in torch.as_tensor(final).reshape(-1).tolist()]
        if len(fr) != S or len(fi) != S:
            raise ValueError(f"frames and final must have {S} entries")
        for s in range(S):
            if not 0 <= fr[s] <= Tc:
                raise ValueError(f"frames[{s}] = {fr[s]} is not in 0 ... {Tc}")
            if not fi[s] and fr[s] % f != 0:
                raise ValueError(f"frames[{s}] = {fr[s]}: a non-final feed must bring a multiple of the reduction factor {f}")
        return fr, fi

    def _encode_chunk(self, mel_chunk, fr):
        """The encoder over every slot's new frames (inside _eval()) -> enc [slots, ceil(max(fr) / f), H], or None without frames."""
        T = max(fr)
        if T == 0:
            return None
        reset = self._pending if any(self._pending) else None
        enc = self.es.run(mel_chunk[:, :T], row_frames=fr, reset=reset)
        self._pending = [False] * self.S
        return enc


class StreamingGreedyDecoder(_StreamingSlots):
    """Greedy decoding of up to `slots` live audio streams at once, fed chunk by chunk (include/rnnt.h, streaming greedy
    decoding).  Each slot holds one stream at a time; streams start and end at different times.

    start(slots) (re)starts a stream in the given slots (indices, or a bool mask [slots]): zero encoder state, the prediction
    network's start token 0 from zero state, no symbols, score 0, frame 0.  The other slots are untouched.

    feed(mel_chunk [slots, Tc, F], frames [slots], final [slots]) -> (ids int32 [slots, N] zero-padded, counts int32 [slots]),
    on the model's device: the symbols each stream emitted in this call.  Slot s consumes mel_chunk[s, :frames[s]] (stacked
    log-mel rows, what model.Encoder takes); a slot with 0 frames and final False is left as it was.  In a non-final feed,
    frames[s] must be a multiple of the encoder's reduction factor f; a final feed may have any length (its odd tail is
    zero-padded after the LayerNorm, as one run over the whole input pads it).  frames and final are host data (lists, arrays
    or CPU tensors).  Greedy search runs with greedy_decode_batch's per-frame semantics until every live slot has consumed
    all encoder frames it has so far.  After its final feed, or once its max_length symbols are spent, a slot is finished: it
    emits nothing more until the next start.

    hypotheses() -> (ids [slots, N] zero-padded, lengths [slots], scores [slots]) of each slot's stream since its start.
    token_times=True adds timed_hypotheses() -> (ids, frames, logp), and the equivalence below covers them.

    A stream delivered through any chunking that follows the rule above, in any slot, beside any other traffic, ends with the
    ids, length and score of the same stream fed in one call to a 1-slot decoder: bitwise on an MI355X (every kernel on the path
    sums in a fixed order that depends on the shapes alone), and equal ids to greedy_decode_batch of the stream alone.

    On an MI355X the encoder (EncoderStream, compute_rnnt_encoder_run_rows), the prediction network (PredictionStep) and the
    joint (GreedyStreamJoint) run in the library, and a feed reads the host only for the all-done word every `check_every`
    steps and once for N.  On CPU, or for models and shapes the kernels do not take, the same state machine runs in torch, with
    the fallback rules of those three classes."""

    def __init__(self, model, slots: int, max_chunk_frames: int, max_length: Optional[int] = None,
                 max_symbols_per_frame: Optional[int] = None, check_every: int = CHECK_EVERY, token_times: bool = False):
        self._init_slots(model, slots, max_chunk_frames)
        S = self.S
        self.check_every = max(1, int(check_every))
        self.max_length = None if max_length is None else int(max_length)
        self.token_times = bool(token_times)
        with self._eval():
            self.gj = self._make_joint(model)
            dev = next(model.parameters()).device
            N = max(1, self.max_length) if self.max_length is not None else self.Te + 16
            self.gj.begin(S, self.Te, int(max_symbols_per_frame or 0), N, device=dev)
            self.ps = PredictionStep(model.prediction, _joint_W1(self.gj))
            self.pp = self.ps.begin(S)
        self.dev = self.gj.hyps.device

    def _make_joint(self, model):
        """The stream joint the decoder steps (a subclass decodes another kind of joint: tdt.StreamingTDTGreedyDecoder)."""
        return GreedyStreamJoint(model.joint, token_times=True) if self.token_times else GreedyStreamJoint(model.joint)

    @torch.no_grad()
    def start(self, slots) -> None:
        m = self._mask(slots)
        if not any(m):
            return
        with self._eval():
            self.pp = self.ps.reset(m)
            ms = None if self.max_length is None else [self.max_length] * self.S
            self.gj.feed(None, [0] * self.S, reset=m, final=None, max_symbols=ms)
        self._pending = [p or q for p, q in zip(self._pending, m)]

    @torch.no_grad()
    def feed(self, mel_chunk: torch.Tensor, frames, final):
        S, f = self.S, self.f
        fr, fi = self._check_feed(mel_chunk, frames, final)
        T = max(fr)
        with self._eval():
            enc = self._encode_chunk(mel_chunk, fr)
            self.gj.feed(enc, [-(-v // f) for v in fr], reset=None, final=[int(v) for v in fi])
            before = self.gj.lengths.clone()
            if T > 0:
                self._decode()
            counts = self.gj.lengths - before
            N = read_flag(counts.max().reshape(1)) if S > 0 else 0
            ar = torch.arange(N, device=self.dev)
            idx = (before.long()[:, None] + ar[None, :]).clamp(max=self.gj.hyps.shape[1] - 1)
            ids = torch.where(ar[None, :] < counts[:, None], self.gj.hyps.gather(1, idx), 0).to(torch.int32)
        return ids, counts

    def _decode(self):
        """Joint step, then prediction-network step, until every slot has consumed its chunk.  The prediction network always
        takes the last step's symbols: the next feed goes on from them."""
        global LAST_STEPS
        LAST_STEPS, self.pp = _greedy_loop(self.gj, self.ps, self.pp, self.check_every, carry=True)

    def hypotheses(self):
        """(ids int32 [slots, N] zero-padded, lengths int32 [slots], scores [slots]) of each slot's stream since its start."""
        h, n = self.gj.hyps, self.gj.lengths
        ids = torch.where(torch.arange(h.shape[1], device=h.device)[None, :] < n[:, None], h, 0)
        return ids, n.clone(), self.gj.scores.clone()

    def timed_hypotheses(self):
        """(ids int32 [slots, N] zero-padded, frames int32 [slots, N] -1 padded, logp [slots, N] 0 padded) of each slot's stream
        since its start: per token the encoder frame that emitted it, counted from the slot's start across all its chunks, and
        the log-softmax of that decision.  Greedy never rewrites a token: everything reported is final.  Needs token_times=True."""
        if not self.token_times:
            raise RuntimeError("timed_hypotheses() needs a decoder built with token_times=True")
        h, n = self.gj.hyps, self.gj.lengths
        live = torch.arange(h.shape[1], device=h.device)[None, :] < n[:, None]
        return (torch.where(live, h, 0), torch.where(live, self.gj.frames, -1),
                torch.where(live, self.gj.logp, torch.zeros_like(self.gj.logp)))


# ---------------------------------------------------------------------------------------------------------------------------
# Streaming beam search
# ---------------------------------------------------------------------------------------------------------------------------
class StreamingBeamDecoder(_StreamingSlots):
    """Modified beam search (one symbol per frame, include/rnnt.h) of up to `slots` live audio streams at once, fed chunk by
    chunk; the streaming counterpart of beam_decode_batch, with the slot handling of StreamingGreedyDecoder.

    start(slots) (re)starts a stream in the given slots: zero encoder state, the beam [((), 0)], its `beam` prediction-network
    rows from the start token.  The other slots are untouched.

    feed(mel_chunk [slots, Tc, F], frames [slots], final [slots]) -> (ids int32 [slots, N] zero-padded, lengths int32 [slots],
    stable int32 [slots]) on the model's device: the CURRENT BEST hypothesis of every slot and how much of it is final.  A later
    frame may rewrite a beam's best hypothesis, so a feed returns the whole of it, not a delta; its first stable[s] tokens are
    shared by every hypothesis of the beam and can no longer change.  frames and final follow StreamingGreedyDecoder.feed's rules
    (host data; a non-final feed brings a multiple of the reduction factor; frames <= max_chunk_frames).  After its final feed a
    slot is finished: further feeds leave it as it is until the next start.

    hypotheses() -> the best (ids [slots, N], lengths [slots], scores [slots]); nbest() -> (ids [slots, beam, N], lengths
    [slots, beam], scores [slots, beam]), best first (empty places: length 0, score -inf).

    max_length is N, the tokens one stream's hypothesis may hold; the default is 512.  The search emits at most one token per
    encoder frame, so no stream can reach 512 tokens in fewer than 512 encoder frames: 30.7 s of audio at the reference's 60 ms
    encoder frame (10 ms step, downsample 3, time reduction 2).  Speech fills a small part of its frames with tokens, so 512
    tokens are some minutes of it; how many depends on the vocabulary and is not measured here.  A hypothesis that holds N tokens
    is NOT reported as full: it goes on through the later frames on blanks alone and emits nothing more, silently.  lengths[s] ==
    N is the only sign; a caller that may meet it restarts the slot (start) or builds the decoder with a larger max_length.  The
    workspace holds 2 slots beam N ints and every frame copies each surviving token row, so N costs memory and time.
    slots * beam <= 1024 (the prediction network's rows).

    A stream delivered through any chunking that follows the rule above, in any slot, beside any other traffic, ends with the
    n-best (ids, lengths, scores) and stable of the same stream fed in one call to a 1-slot decoder: bitwise on an MI355X.  beam
    = 1 gives the ids of StreamingGreedyDecoder with max_symbols_per_frame = 1.

    On an MI355X the encoder (EncoderStream), the prediction network (PredictionStep) and the joint (BeamStreamJoint) run in the
    library and a feed reads nothing from the host: a chunk of n encoder frames is exactly n steps.  On CPU, or for models and
    shapes the kernels do not take, the same state machine runs in torch, with the fallback rules of those three classes."""

    DEFAULT_MAX_LENGTH = 512

    def __init__(self, model, slots: int, max_chunk_frames: int, beam: int = 4, max_length: Optional[int] = None,
                 token_times: bool = False, context=None, lm=None):
        K = int(beam)
        self.token_times = bool(token_times)
        if not 1 <= K <= 16:
            raise ValueError(f"beam must be in 1 ... 16, got {beam}")
        if int(slots) * K > BeamStreamJoint.MAX_ROWS:
            raise ValueError(f"slots * beam must be in 1 ... {BeamStreamJoint.MAX_ROWS}, got {slots} * {beam}")
        N = self.DEFAULT_MAX_LENGTH if max_length is None else int(max_length)
        if N < 1:
            raise ValueError(f"max_length must be >= 1, got {max_length}")
        self._init_slots(model, slots, max_chunk_frames)
        S = self.S
        self.K, self.max_length = K, N
        with self._eval():
            self.bj = self._make_joint(model, K, context, lm)
            dev = next(model.parameters()).device
            self.bj.begin(S, self.Te, N, device=dev)
            self.ps = PredictionStep(model.prediction, _joint_W1(self.bj))
            self.pp = self.ps.begin(S * K)
        self.dev = self.bj.parents.device

    def _make_joint(self, model, K, context, lm):
        """The stream joint the decoder steps (a subclass decodes another kind of joint: tdt.StreamingTDTBeamDecoder)."""
        return BeamStreamJoint(model.joint, K, token_times=self.token_times, context=context, lm=lm)

    @torch.no_grad()
    def start(self, slots) -> None:
        m = self._mask(slots)
        if not any(m):
            return
        with self._eval():
            self.pp = self.ps.reset([v for v in m for _ in range(self.K)])
            self.bj.feed(None, [0] * self.S, reset=[int(v) for v in m], final=None)
        self._pending = [p or q for p, q in zip(self._pending, m)]

    @torch.no_grad()
    def feed(self, mel_chunk: torch.Tensor, frames, final):
        global LAST_STEPS
        f = self.f
        fr, fi = self._check_feed(mel_chunk, frames, final)
        T = max(fr)
        with self._eval():
            enc = self._encode_chunk(mel_chunk, fr)
            self.bj.feed(enc, [-(-v // f) for v in fr], reset=None, final=[int(v) for v in fi])
            steps = -(-T // f)  # (host data: the search is frame-synchronous, so nothing is polled)
            self.pp = _beam_loop(self.bj, self.ps, self.pp, steps, carry=True)
            LAST_STEPS = steps
            ids, lengths, _, stable = self.bj.results()[:4]
        return ids[:, 0], lengths[:, 0], stable

    def hypotheses(self):
        """The best hypothesis of each slot's stream since its start: (ids int32 [slots, N] zero-padded, lengths int32 [slots],
        scores [slots])."""
        ids, lengths, scores = self.bj.results()[:3]
        return ids[:, 0], lengths[:, 0], scores[:, 0]

    def nbest(self):
        """(ids int32 [slots, beam, N] zero-padded, lengths int32 [slots, beam], scores [slots, beam]), best first."""
        ids, lengths, scores = self.bj.results()[:3]
        return ids, lengths, scores

    def bias_states(self):
        """int32 [slots, beam]: with context=, the context graph's state of every hypothesis.  The stream reports the beam's own
        scores and order; context.finalize(scores, states) is what a stream that ends here would keep."""
        return self.bj.bias_states().reshape(self.S, self.K)

    def lm_states(self):
        """int32 [slots, beam]: with lm=, the LM's state of every hypothesis.  The stream reports the beam's own scores and
        order; lm.finalize(scores, states) adds the end-of-sentence score a stream that ends here would get."""
        return self.bj.lm_states().reshape(self.S, self.K)

    def _timed(self):
        if not self.token_times:
            raise RuntimeError("timed results need a decoder built with token_times=True")
        return self.bj.results()

    def timed_hypotheses(self):
        """The best hypothesis of each slot with its times: (ids int32 [slots, N] zero-padded, frames int32 [slots, N] -1 padded,
        logp [slots, N] 0 padded); frames count encoder frames from the slot's start across all its chunks.  A hypothesis that
        absorbed merged candidates carries the times of its first-ranked member.  Needs token_times=True."""
        r = self._timed()
        return r[0][:, 0], r[4][:, 0], r[5][:, 0]

    def timed_nbest(self):
        """(ids [slots, beam, N], lengths [slots, beam], scores [slots, beam], frames [slots, beam, N], logp [slots, beam, N]),
        best first.  Needs token_times=True."""
        r = self._timed()
        return r[0], r[1], r[2], r[4], r[5]

    def timed_stable_lengths(self):
        """int32 [slots]: the leading tokens of a slot on which every hypothesis of its beam agrees in token AND emission frame:
        their ids and times are final.  Never more than feed()'s `stable`.  Needs token_times=True."""
        return self._timed()[6]


class StreamingMultiBeamDecoder(StreamingBeamDecoder):
    """Beam search with SEVERAL symbols per frame (time-synchronous, on the standard lattice: include/rnnt_beam_multi_stream.h) of up
    to `slots` live audio streams at once, fed chunk by chunk: the streaming counterpart of beam_decode_batch(symbols_per_frame=E),
    with the slot handling and the results of StreamingBeamDecoder.  It follows a model trained with the project's own loss,
    which may emit several labels in one frame, and can return more labels than frames.

    Each slot has 2 beam prediction-network rows (its open and its closed list); start(slots) resets a slot's 2 beam rows.  A
    chunk of n encoder frames is exactly n (symbols_per_frame + 1) steps, each a joint step and a prediction-network step.
    feed -> (best ids, lengths, stable) as the parent's; hypotheses(), nbest(), and with token_times=True timed_hypotheses() ->
    (ids, frames), timed_nbest() -> (ids, lengths, scores, frames) and timed_stable_lengths(): the frame rows carry frames only, no
    log-probabilities.  A hypothesis a closing was merged into reports the frames of the path it held.  context= and lm= are not
    taken (ValueError), as offline.

    max_length is N, the tokens one stream's hypothesis may hold; the default is 512.  With E symbols per frame a hypothesis can
    reach 512 tokens in 512 / E encoder frames.  A hypothesis that holds N tokens is NOT reported as full: it offers no expansion
    and goes on through the later frames on blanks alone, silently; lengths[s] == N is the only sign.  slots * 2 * beam <= 1024.

    A stream delivered through any chunking, in any slot, beside any other traffic, ends with the n-best, stable, frames and timed
    stable lengths of the same stream fed in one call to a 1-slot decoder: bitwise on an MI355X."""

    def __init__(self, model, slots: int, max_chunk_frames: int, beam: int = 4, symbols_per_frame: int = 2,
                 max_length: Optional[int] = None, token_times: bool = False, context=None, lm=None):
        if context is not None or lm is not None:
            raise ValueError("context= and lm= are not taken by the beam search with several symbols per frame")
        K, E = int(beam), int(symbols_per_frame)
        self.token_times = bool(token_times)
        if not 1 <= K <= 16:
            raise ValueError(f"beam must be in 1 ... 16, got {beam}")
        if not 1 <= E <= 8:
            raise ValueError(f"symbols_per_frame must be in 1 ... 8, got {symbols_per_frame}")
        if int(slots) * 2 * K > MultiBeamStreamJoint.MAX_ROWS:
            raise ValueError(f"slots * 2 * beam must be in 1 ... {MultiBeamStreamJoint.MAX_ROWS}, got {slots} * 2 * {beam}")
        N = self.DEFAULT_MAX_LENGTH if max_length is None else int(max_length)
        if N < 1:
            raise ValueError(f"max_length must be >= 1, got {max_length}")
        self._init_slots(model, slots, max_chunk_frames)
        self.K, self.E, self.max_length = K, E, N
        with self._eval():
            self.bj = MultiBeamStreamJoint(model.joint, K, E, token_times=self.token_times)
            dev = next(model.parameters()).device
            self.bj.begin(self.S, self.Te, N, device=dev)
            self.ps = PredictionStep(model.prediction, _joint_W1(self.bj))
            self.pp = self.ps.begin(self.S * 2 * K)
        self.dev = self.bj.parents.device

    @torch.no_grad()
    def start(self, slots) -> None:
        m = self._mask(slots)
        if not any(m):
            return
        with self._eval():
            self.pp = self.ps.reset([v for v in m for _ in range(2 * self.K)])
            self.bj.feed(None, [0] * self.S, reset=[int(v) for v in m], final=None)
        self._pending = [p or q for p, q in zip(self._pending, m)]

    @torch.no_grad()
    def feed(self, mel_chunk: torch.Tensor, frames, final):
        global LAST_STEPS
        f = self.f
        fr, fi = self._check_feed(mel_chunk, frames, final)
        T = max(fr)
        with self._eval():
            enc = self._encode_chunk(mel_chunk, fr)
            self.bj.feed(enc, [-(-v // f) for v in fr], reset=None, final=[int(v) for v in fi])
            steps = -(-T // f) * (self.E + 1)  # (host data: every frame takes E + 1 rounds, so nothing is polled)
            self.pp = _beam_loop(self.bj, self.ps, self.pp, steps, carry=True)
            LAST_STEPS = steps
            ids, lengths, _, stable = self.bj.results()[:4]
        return ids[:, 0], lengths[:, 0], stable

    def bias_states(self):
        raise RuntimeError("the beam search with several symbols per frame takes no context=")

    def lm_states(self):
        raise RuntimeError("the beam search with several symbols per frame takes no lm=")

    def timed_hypotheses(self):
        """The best hypothesis of each slot with its frames: (ids int32 [slots, N] zero-padded, frames int32 [slots, N] -1
        padded), counted in encoder frames from the slot's start across all its chunks.  Needs token_times=True."""
        r = self._timed()
        return r[0][:, 0], r[4][:, 0]

    def timed_nbest(self):
        """(ids [slots, beam, N], lengths [slots, beam], scores [slots, beam], frames [slots, beam, N]), best first.  Needs
        token_times=True."""
        r = self._timed()
        return r[0], r[1], r[2], r[4]

    def timed_stable_lengths(self):
        """int32 [slots]: the leading tokens on which every hypothesis of a slot agrees in token AND emission frame; never more
        than feed()'s `stable`, and final at frame boundaries (after a feed).  Needs token_times=True."""
        return self._timed()[5]


# ---------------------------------------------------------------------------------------------------------------------------
# Streaming transcription from raw audio
# ---------------------------------------------------------------------------------------------------------------------------
class StreamingTranscriber:
    """Raw audio in, hypotheses out, for up to `slots` live streams: a features.StreamingFrontEnd (its row_multiple the encoder's
    reduction factor, so that every non-final feed hands the decoder a multiple of it) in front of a StreamingGreedyDecoder, or
    of a StreamingBeamDecoder when `beam` is given.  The decoder is sized by the front end's max_rows; decoder_kwargs go to it
    (max_length, max_symbols_per_frame, check_every for greedy; max_length for beam).  context=biasing.ContextGraph (beam search
    only): contextual biasing, as StreamingBeamDecoder takes it; lm=lm.NgramLM (beam search only): LM shallow fusion, likewise.
    symbols_per_frame=E (with beam=K; with tdt_durations, tdt_beam, context or lm: ValueError): the decoder is a
    StreamingMultiBeamDecoder, the time-synchronous search with up to E symbols per frame (decoder_kwargs: max_length, token_times;
    no words(): it keeps frames, not per-token log-probabilities).
    tdt_durations=[...] (together with beam: ValueError): the model is a token-and-duration transducer with that duration set,
    and the decoder is a tdt.StreamingTDTGreedyDecoder (decoder_kwargs: joint, max_length, max_symbols_per_frame, check_every) or,
    with tdt_beam=K, a tdt.StreamingTDTBeamDecoder of beam K (decoder_kwargs: joint, max_length, token_times; no context= / lm=,
    and no words(): its beams keep frames and durations, not per-token log-probabilities).

    start(slots) starts a stream in the given slots of both; feed(audio [slots, N], samples [slots], final [slots]) (N <=
    max_chunk_samples; samples and final are host data) returns what the decoder's feed returns for the rows this audio
    completed; hypotheses() and nbest() (beam only) are the decoder's.  norm is the front end's: the default "running" subtracts
    the mean of the frames so far, which is NOT the per-utterance mean the reference trains on -- train the model on
    features.running_mean_log_mel for it.  A stream's result is bitwise independent of how its audio was chunked."""

    def __init__(self, model, hp, sample_rate, slots: int, max_chunk_samples: int, beam: Optional[int] = None,
                 norm: str = "running", context=None, lm=None, tdt_durations=None, tdt_beam: Optional[int] = None,
                 symbols_per_frame: Optional[int] = None, **decoder_kwargs):
        from .features import StreamingFrontEnd

        if symbols_per_frame is not None:
            if beam is None:
                raise ValueError("symbols_per_frame= needs beam search: build the StreamingTranscriber with beam=")
            if tdt_durations is not None or tdt_beam is not None:
                raise ValueError("symbols_per_frame= does not go with tdt_durations= / tdt_beam=: the TDT searches are not time-synchronous")
            if context is not None or lm is not None:
                raise ValueError("context= and lm= are not taken by the beam search with several symbols per frame (symbols_per_frame=)")

        if tdt_durations is not None and beam is not None:
            raise ValueError("tdt_durations= does not go with beam=: the TDT beam search is tdt_beam=K, build the StreamingTranscriber "
                             "without beam=")
        if tdt_beam is not None and tdt_durations is None:
            raise ValueError("tdt_beam= needs the model's duration set: build the StreamingTranscriber with tdt_durations=")
        if tdt_beam is not None and (context is not None or lm is not None):
            raise ValueError("context= and lm= are not taken by the TDT beam search (tdt_beam=)")

        if context is not None and beam is None:
            raise ValueError("context= needs beam search: build the StreamingTranscriber with beam=")
        if lm is not None and beam is None:
            raise ValueError("lm= needs beam search: build the StreamingTranscriber with beam=")

        dev = next(model.parameters()).device
        self.hp, self.sample_rate = hp, sample_rate
        self.front = StreamingFrontEnd(hp, sample_rate, slots, max_chunk_samples, int(model.encoder.reduce.factor), norm, device=dev)
        if tdt_beam is not None:
            from .tdt import StreamingTDTBeamDecoder

            self.decoder = StreamingTDTBeamDecoder(model, tdt_durations, slots, self.front.max_rows, beam=tdt_beam, **decoder_kwargs)
        elif tdt_durations is not None:
            from .tdt import StreamingTDTGreedyDecoder

            self.decoder = StreamingTDTGreedyDecoder(model, tdt_durations, slots, self.front.max_rows, **decoder_kwargs)
        elif beam is None:
            self.decoder = StreamingGreedyDecoder(model, slots, self.front.max_rows, **decoder_kwargs)
        elif symbols_per_frame is not None:
            self.decoder = StreamingMultiBeamDecoder(model, slots, self.front.max_rows, beam=beam, symbols_per_frame=symbols_per_frame,
                                                     **decoder_kwargs)
        else:
            self.decoder = StreamingBeamDecoder(model, slots, self.front.max_rows, beam=beam, context=context, lm=lm, **decoder_kwargs)

    def start(self, slots) -> None:
        self.front.start(slots)
        self.decoder.start(slots)

    def feed(self, audio: torch.Tensor, samples, final):
        rows, counts = self.front.feed(audio, samples, final)
        return self.decoder.feed(rows, counts, final)

    def hypotheses(self):
        return self.decoder.hypotheses()

    def nbest(self):
        if not hasattr(self.decoder, "nbest"):
            raise RuntimeError("nbest() needs beam search: build the StreamingTranscriber with beam=")
        return self.decoder.nbest()

    def words(self, slot: int, encoder=None):
        """The words of slot's current (best) hypothesis with times and confidences -> (words, final): words is a list of (word,
        start_seconds, end_seconds, confidence) and the first `final` of them can no longer change.  `encoder` is the character
        vocabulary the model was trained with (a features.CharEncoder; None: the reference's default vocabulary, CharEncoder()).
        Needs token_times=True (a decoder keyword).

        A word starts at the start of the frame that emitted its first token and ends at the end of the frame that emitted its
        last one (alignment.word_times x alignment.frame_seconds).  Its confidence is exp(min log-probability of its tokens):
        the weakest decision inside the word -- a product would punish long words, a mean would hide one bad letter.  final:
        for beam search the words that lie wholly inside the timed stable prefix (every hypothesis of the beam agrees on their
        tokens and frames); greedy never rewrites, so all words are final.  "Final" is about what was reported: a stream that
        goes on may still append letters to the last word until a space follows it."""
        from .alignment import frame_seconds
        from .features import CharEncoder

        dec = self.decoder
        if getattr(dec, "durations", None) is not None and hasattr(dec, "nbest"):
            raise RuntimeError("words() needs per-token log-probabilities, which the TDT beam search (tdt_beam=) does not keep")
        if isinstance(dec, StreamingMultiBeamDecoder):
            raise RuntimeError("words() needs per-token log-probabilities, which the beam search with several symbols per frame "
                               "(symbols_per_frame=) does not keep")
        if hasattr(dec, "timed_stable_lengths"):  # beam: one results call gives the best hypothesis and the timed stable length
            r = dec._timed()
            ids, frames, logp, stable = r[0][slot, 0].cpu(), r[4][slot, 0].cpu(), r[5][slot, 0].cpu(), int(r[6][slot])
        else:  # greedy never rewrites: every token reported is final
            ids, frames, logp = (x[slot].cpu() for x in dec.timed_hypotheses())
            stable = None
        n = int((frames >= 0).sum())
        return timed_words(ids[:n], frames[:n], logp[:n], encoder if encoder is not None else CharEncoder(),
                           frame_seconds(self.hp, self.sample_rate), stable)


def timed_words(ids, frames, logp, encoder, seconds_per_frame: float, stable_tokens: Optional[int] = None):
    """One hypothesis (ids, emission frames, log-probabilities per token) -> (words, final) as StreamingTranscriber.words
    describes them.  stable_tokens: the leading tokens that are final (None: all)."""
    from .alignment import word_times

    n = len(ids)
    by_frame = word_times(ids, frames, encoder)
    by_index = word_times(ids, list(range(n)), encoder)  # (the same split: first and last token index of every word)
    lp = [float(v) for v in torch.as_tensor(logp).flatten().tolist()]
    idl = [int(v) for v in torch.as_tensor(ids).flatten().tolist()]
    space = encoder.index.get(" ")
    stable = n if stable_tokens is None else int(stable_tokens)
    words, final = [], 0
    for (w, f0, f1), (_, i0, i1) in zip(by_frame, by_index):
        conf = math.exp(min(lp[i] for i in range(i0, i1 + 1) if idl[i] != space))
        words.append((w, f0 * seconds_per_frame, (f1 + 1) * seconds_per_frame, conf))
        if i1 < stable and final == len(words) - 1:
            final += 1
    return words, final
