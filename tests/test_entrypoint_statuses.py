"""Host-only table of what the decoder entry points answer before anything is enqueued: the base library's greedy, beam,
greedy-stream and beam-stream entry points and every entry point of the bias, lm, tdtgreedy, tdtstream, tdtbeam and tdtbeamstream
libraries.  A refusal row is one well-formed call with one argument spoilt and must answer RNNT_STATUS_INVALID_VALUE (2), one row
per clause of the shared argument checks; an acceptance row is the well-formed call itself on fake device pointers and must answer
anything but 2 (it passes validation and then fails for lack of a device, so those rows are skipped where a device is present).
Two structural checks follow: no extension library carries a base entry point it does not call, and no source under csrc/
includes a .hip file."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from rnnt_speech_recognition_amd.build import CSRC, lib_path

INVALID = 2
FAKE, MISALIGNED_4, MISALIGNED_256 = 256, 258, 260  # device pointers that are never dereferenced
J, V, DTYPE = 128, 28, 1  # a joint the decoders take (joint_dtype 1: joint_size a multiple of 128, alphabet_size <= 8192)

# ---- the entry points, argument names in header order ("o": the options; "G": the graph; "sz": size_t *) ----
_STEP = "pred_proj parents emitted topk_logits topk_symbols lse joint_size alphabet_size minibatch beam joint_dtype workspace o"
_STREAM_STEP = ("pred_proj parents emitted topk_logits topk_symbols lse joint_size alphabet_size slots beam max_hyp_len joint_dtype "
                "workspace o")
_BEAM_BEGIN = "enc_proj frame_lengths W2 b2 joint_size alphabet_size minibatch beam joint_dtype workspace o"
_BS_BEGIN = "W1 b1 W2 b2 enc_width joint_size alphabet_size slots beam max_hyp_len joint_dtype workspace o"
_BS_FEED = ("enc enc_frames chunk_frames reset final_chunk enc_width joint_size alphabet_size slots beam max_hyp_len joint_dtype "
            "workspace o")
_BS_TAIL = "joint_size alphabet_size slots beam max_hyp_len joint_dtype workspace o"
_TDT_STEP = ("pred_proj hyps hyp_frames hyp_logp max_hyp_len hyp_lengths scores emitted all_done logit_stats joint_size alphabet_size "
             "num_durations {rows} joint_dtype workspace o")
ENTRIES = {
    "base": {
        "get_rnnt_greedy_workspace_size": "maxT minibatch joint_size alphabet_size joint_dtype sz",
        "compute_rnnt_greedy_begin": ("enc_proj frame_lengths max_symbols W2 b2 joint_size alphabet_size minibatch max_per_frame "
                                      "joint_dtype workspace o"),
        "compute_rnnt_greedy_step": ("pred_proj hyps max_hyp_len hyp_lengths scores emitted all_done logit_stats joint_size "
                                     "alphabet_size minibatch joint_dtype workspace o"),
        "compute_rnnt_greedy_step_timed": ("pred_proj hyps hyp_frames hyp_logp max_hyp_len hyp_lengths scores emitted all_done "
                                           "logit_stats frame_base joint_size alphabet_size minibatch joint_dtype workspace o"),
        "get_rnnt_beam_workspace_size": "maxT minibatch beam joint_size alphabet_size joint_dtype sz",
        "compute_rnnt_beam_begin": _BEAM_BEGIN,
        "compute_rnnt_beam_step": _STEP,
        "compute_rnnt_beam_results": "hyps hyp_lengths scores joint_size alphabet_size minibatch beam joint_dtype workspace o",
        "get_rnnt_beam_timed_workspace_size": "maxT minibatch beam joint_size alphabet_size joint_dtype sz",
        "compute_rnnt_beam_timed_begin": _BEAM_BEGIN,
        "compute_rnnt_beam_timed_step": _STEP,
        "compute_rnnt_beam_timed_results": ("hyps hyp_lengths scores hyp_frames hyp_logp joint_size alphabet_size minibatch beam "
                                            "joint_dtype workspace o"),
        "get_rnnt_greedy_stream_workspace_size": "max_chunk_frames slots enc_width joint_size alphabet_size joint_dtype sz",
        "compute_rnnt_greedy_stream_begin": "W1 b1 W2 b2 enc_width joint_size alphabet_size slots joint_dtype workspace o",
        "compute_rnnt_greedy_stream_feed": ("enc enc_frames chunk_frames reset final_chunk max_symbols max_per_frame hyp_lengths scores "
                                            "all_done enc_width joint_size alphabet_size slots joint_dtype workspace o"),
        "compute_rnnt_greedy_stream_feed_timed": ("enc enc_frames chunk_frames reset final_chunk max_symbols max_per_frame hyp_lengths "
                                                  "scores all_done frame_base enc_width joint_size alphabet_size slots joint_dtype "
                                                  "workspace o"),
        "get_rnnt_beam_stream_workspace_size": "max_chunk_frames slots beam max_hyp_len enc_width joint_size alphabet_size joint_dtype sz",
        "compute_rnnt_beam_stream_begin": _BS_BEGIN,
        "compute_rnnt_beam_stream_feed": _BS_FEED,
        "compute_rnnt_beam_stream_step": _STREAM_STEP,
        "compute_rnnt_beam_stream_results": "hyps hyp_lengths scores stable_lengths " + _BS_TAIL,
        "get_rnnt_beam_stream_timed_workspace_size": ("max_chunk_frames slots beam max_hyp_len enc_width joint_size alphabet_size "
                                                      "joint_dtype sz"),
        "compute_rnnt_beam_stream_timed_begin": _BS_BEGIN,
        "compute_rnnt_beam_stream_timed_feed": _BS_FEED,
        "compute_rnnt_beam_stream_timed_step": _STREAM_STEP,
        "compute_rnnt_beam_stream_timed_results": "hyps hyp_lengths scores stable_lengths hyp_frames hyp_logp timed_stable_lengths " + _BS_TAIL,
    },
    "bias": {
        "compute_rnnt_beam_step_biased": _STEP + " G states",
        "compute_rnnt_beam_timed_step_biased": _STEP + " G states",
        "compute_rnnt_beam_stream_step_biased": _STREAM_STEP + " G states",
        "compute_rnnt_beam_stream_timed_step_biased": _STREAM_STEP + " G states",
    },
    "lm": {
        "compute_rnnt_beam_step_lm": _STEP + " G states",
        "compute_rnnt_beam_timed_step_lm": _STEP + " G states",
        "compute_rnnt_beam_stream_step_lm": _STREAM_STEP + " G states",
        "compute_rnnt_beam_stream_timed_step_lm": _STREAM_STEP + " G states",
    },
    "tdtgreedy": {
        "get_rnnt_tdt_greedy_workspace_size": "maxT minibatch joint_size alphabet_size num_durations joint_dtype sz",
        "compute_rnnt_tdt_greedy_begin": ("enc_proj frame_lengths max_symbols W2 b2 joint_size alphabet_size durations num_durations "
                                          "minibatch max_per_frame joint_dtype workspace o"),
        "compute_rnnt_tdt_greedy_step": _TDT_STEP.format(rows="minibatch"),
    },
    "tdtstream": {
        "get_rnnt_tdt_greedy_stream_workspace_size": ("max_chunk_frames slots enc_width joint_size alphabet_size num_durations "
                                                      "joint_dtype sz"),
        "compute_rnnt_tdt_greedy_stream_begin": ("W1 b1 W2 b2 enc_width joint_size alphabet_size durations num_durations slots "
                                                 "joint_dtype workspace o"),
        "compute_rnnt_tdt_greedy_stream_feed": ("enc enc_frames chunk_frames reset final_chunk max_symbols max_per_frame hyp_lengths "
                                                "scores all_done enc_width joint_size alphabet_size num_durations slots joint_dtype "
                                                "workspace o"),
        "compute_rnnt_tdt_greedy_stream_step": _TDT_STEP.format(rows="slots"),
    },
    "tdtbeam": {
        "get_rnnt_tdt_beam_workspace_size": "maxT minibatch beam joint_size alphabet_size num_durations joint_dtype timed sz",
        "compute_rnnt_tdt_beam_begin": ("enc_proj frame_lengths W2 b2 joint_size alphabet_size durations num_durations minibatch beam "
                                        "joint_dtype timed workspace o"),
        "compute_rnnt_tdt_beam_step": ("pred_proj parents emitted topk_logits topk_symbols dur_logits lse joint_size alphabet_size "
                                       "num_durations minibatch beam joint_dtype timed workspace o"),
        "compute_rnnt_tdt_beam_results": ("hyps hyp_lengths scores cursors hyp_frames hyp_durations joint_size alphabet_size "
                                          "num_durations minibatch beam joint_dtype timed workspace o"),
    },
    "tdtbeamstream": {
        "get_rnnt_tdt_beam_stream_workspace_size": ("max_chunk_frames slots beam max_hyp_len enc_width joint_size alphabet_size "
                                                    "num_durations joint_dtype timed sz"),
        "compute_rnnt_tdt_beam_stream_begin": ("W1 b1 W2 b2 enc_width joint_size alphabet_size durations num_durations slots beam "
                                               "max_hyp_len joint_dtype timed workspace o"),
        "compute_rnnt_tdt_beam_stream_feed": ("enc enc_frames chunk_frames reset final_chunk enc_width joint_size alphabet_size "
                                              "num_durations slots beam max_hyp_len joint_dtype timed workspace o"),
        "compute_rnnt_tdt_beam_stream_step": ("pred_proj parents emitted topk_logits topk_symbols dur_logits lse joint_size "
                                              "alphabet_size num_durations slots beam max_hyp_len joint_dtype timed workspace o"),
        "compute_rnnt_tdt_beam_stream_results": ("hyps hyp_lengths scores cursors stable_lengths hyp_frames hyp_durations "
                                                 "timed_stable_lengths joint_size alphabet_size num_durations slots beam max_hyp_len "
                                                 "joint_dtype timed workspace o"),
    },
}
LIB_OF = {fn: name for name, fns in ENTRIES.items() for fn in fns}
SIG = {fn: s.split() for fns in ENTRIES.values() for fn, s in fns.items()}
# The aligners' _path entry points take no alphabet_size and hand their shared checks a vocabulary made from the blank
# (rnnt_host.h vocab_holding): call() knows them, the tables of rows above do not.
ALIGN_PATH = {
    "compute_rnnt_align_path": ("base", "token_frames token_logp scores label_lengths input_lengths minibatch workspace o"),
    "compute_rnnt_modified_align_path": ("modalign", "token_frames token_logp scores label_lengths input_lengths minibatch workspace o"),
    "compute_rnnt_tdt_align_path": ("tdtalign", "token_frames token_durations token_logp scores label_lengths input_lengths durations "
                                                "num_durations minibatch workspace o"),
}
TDT = ("tdtgreedy", "tdtstream", "tdtbeam", "tdtbeamstream")

# the well-formed call: every integer argument by name; every other name is a pointer (FAKE)
INTS = dict(maxT=10, max_chunk_frames=10, minibatch=2, slots=2, joint_size=J, alphabet_size=V, joint_dtype=DTYPE, beam=4,
            max_hyp_len=8, max_per_frame=3, enc_width=16, enc_frames=4, num_durations=3, timed=1)
OPTIONS = dict(blank=0, maxT=10, maxU=5, loc=_lib.RNNT_GPU)
DURATIONS = [0, 1, 2]
# what a pointer argument must be besides non-NULL, per entry point: the names whose misalignment (to 4 bytes) it refuses.
# compute_rnnt_beam_begin / _step / _results check no alignment; their timed twins do: that difference is part of the interface.
_STEP_PTRS = "pred_proj parents emitted topk_logits topk_symbols lse".split()
ALIGNED4 = {
    "compute_rnnt_greedy_step_timed": "hyps hyp_frames hyp_logp frame_base".split(),
    "compute_rnnt_greedy_stream_feed_timed": ["frame_base"],
    "compute_rnnt_beam_timed_begin": "enc_proj frame_lengths W2 b2".split(),
    "compute_rnnt_beam_timed_step": _STEP_PTRS,
    "compute_rnnt_beam_timed_results": "hyps hyp_lengths scores hyp_frames hyp_logp".split(),
    "compute_rnnt_beam_stream_begin": "W1 b1 W2 b2".split(),
    "compute_rnnt_beam_stream_timed_begin": "W1 b1 W2 b2".split(),
    "compute_rnnt_beam_stream_feed": "enc chunk_frames reset final_chunk".split(),
    "compute_rnnt_beam_stream_timed_feed": "enc chunk_frames reset final_chunk".split(),
    "compute_rnnt_beam_stream_step": _STEP_PTRS,
    "compute_rnnt_beam_stream_timed_step": _STEP_PTRS,
    "compute_rnnt_beam_stream_results": "hyps hyp_lengths scores stable_lengths".split(),
    "compute_rnnt_beam_stream_timed_results": "hyps hyp_lengths scores stable_lengths hyp_frames hyp_logp timed_stable_lengths".split(),
    "compute_rnnt_tdt_greedy_step": "hyps hyp_frames hyp_logp".split(),
    "compute_rnnt_tdt_greedy_stream_step": "hyps hyp_frames hyp_logp".split(),
    "compute_rnnt_tdt_beam_stream_begin": "W1 b1 W2 b2".split(),
    "compute_rnnt_tdt_beam_stream_feed": "enc chunk_frames reset final_chunk".split(),
    "compute_rnnt_tdt_beam_stream_step": _STEP_PTRS + ["dur_logits"],
    "compute_rnnt_tdt_beam_stream_results": ("hyps hyp_lengths scores cursors stable_lengths hyp_frames hyp_durations "
                                             "timed_stable_lengths").split(),
}
for _fn in list(ENTRIES["bias"]) + list(ENTRIES["lm"]):  # a graph is given: the biased / LM twins check the step's pointers all four
    ALIGNED4[_fn] = _STEP_PTRS + ["states"]
# the pointers an entry point refuses when NULL (the others are optional)
REQUIRED = {
    "compute_rnnt_greedy_begin": "enc_proj frame_lengths W2 b2 workspace",
    "compute_rnnt_greedy_step": "pred_proj hyps hyp_lengths scores emitted all_done workspace",
    "compute_rnnt_greedy_step_timed": "pred_proj hyps hyp_frames hyp_logp hyp_lengths scores emitted all_done workspace",
    "compute_rnnt_beam_begin": "enc_proj frame_lengths W2 b2 workspace",
    "compute_rnnt_beam_timed_begin": "enc_proj frame_lengths W2 b2 workspace",
    "compute_rnnt_beam_results": "hyps hyp_lengths scores workspace",
    "compute_rnnt_beam_timed_results": "hyps hyp_lengths scores hyp_frames hyp_logp workspace",
    "compute_rnnt_greedy_stream_begin": "W1 b1 W2 b2 workspace",
    "compute_rnnt_greedy_stream_feed": "enc chunk_frames hyp_lengths scores all_done workspace",
    "compute_rnnt_greedy_stream_feed_timed": "enc chunk_frames hyp_lengths scores all_done frame_base workspace",
    "compute_rnnt_beam_stream_begin": "W1 b1 W2 b2 workspace",
    "compute_rnnt_beam_stream_timed_begin": "W1 b1 W2 b2 workspace",
    "compute_rnnt_beam_stream_feed": "enc chunk_frames workspace",
    "compute_rnnt_beam_stream_timed_feed": "enc chunk_frames workspace",
    "compute_rnnt_beam_stream_results": "hyps hyp_lengths scores workspace",
    "compute_rnnt_beam_stream_timed_results": "hyps hyp_lengths scores hyp_frames hyp_logp workspace",
    "compute_rnnt_tdt_greedy_begin": "enc_proj frame_lengths W2 b2 durations workspace",
    "compute_rnnt_tdt_greedy_step": "pred_proj hyps hyp_lengths scores emitted all_done workspace",
    "compute_rnnt_tdt_greedy_stream_begin": "W1 b1 W2 b2 durations workspace",
    "compute_rnnt_tdt_greedy_stream_feed": "enc chunk_frames hyp_lengths scores all_done workspace",
    "compute_rnnt_tdt_greedy_stream_step": "pred_proj hyps hyp_lengths scores emitted all_done workspace",
    "compute_rnnt_tdt_beam_begin": "enc_proj frame_lengths W2 b2 durations workspace",
    "compute_rnnt_tdt_beam_results": "hyps hyp_lengths scores workspace",
    "compute_rnnt_tdt_beam_stream_begin": "W1 b1 W2 b2 durations workspace",
    "compute_rnnt_tdt_beam_stream_feed": "enc chunk_frames workspace",
    "compute_rnnt_tdt_beam_stream_results": "hyps hyp_lengths scores workspace",
}
for _fn, _names in SIG.items():  # every beam step, plain, timed, stream, biased, LM and TDT
    if "parents" in _names:
        REQUIRED[_fn] = "pred_proj parents emitted workspace"
REQUIRED = {fn: names.split() for fn, names in REQUIRED.items()}


def _graph(lib_name):
    """A well-formed graph struct in host memory, its arrays fake device pointers."""
    if lib_name == "bias":
        return _lib.rnntBiasGraph(3, 2, FAKE, FAKE, FAKE, FAKE, FAKE)
    return _lib.rnntLmGraph(3, 2, 0, -1.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)


def call(fn, **spoilt):
    """The well-formed call of `fn` with the named arguments replaced.  Keys of OPTIONS replace fields of the options, "graph"
    the graph struct (None: a NULL graph), "durations" the duration set (a list; None: NULL)."""
    name, sig = (LIB_OF[fn], SIG[fn]) if fn in SIG else (ALIGN_PATH[fn][0], ALIGN_PATH[fn][1].split())
    lib = _lib._load(name)
    keep = []  # host memory the call reads
    args = []
    for a in sig:
        if a == "o":
            args.append(_lib.make_options(0, **{k: spoilt.get(k, v) for k, v in OPTIONS.items()}))
        elif a == "sz":
            keep.append(ctypes.c_size_t(0))
            args.append(None if spoilt.get("sz", 1) is None else ctypes.byref(keep[-1]))
        elif a == "G":
            g = spoilt.get("graph", _graph(name))
            keep.append(g)
            args.append(None if g is None else ctypes.byref(g))
        elif a == "durations":
            d = spoilt.get("durations", DURATIONS)
            keep.append(None if d is None else (ctypes.c_int * len(d))(*d))
            args.append(keep[-1])
        elif a == "num_durations":
            d = spoilt.get("durations", DURATIONS)
            args.append(spoilt.get(a, len(d) if d is not None else len(DURATIONS)))
        elif a in INTS:
            args.append(spoilt.get(a, INTS[a]))
        else:
            args.append(ctypes.c_void_p(spoilt[a]) if spoilt.get(a) is not None else (None if a in spoilt else ctypes.c_void_p(FAKE)))
    return getattr(lib, fn)(*args)


# ---- refusal rows: (entry point, the spoilt arguments) -> 2 ----
def _rows():
    rows = []
    for fn, names in SIG.items():
        lib_name, size_fn = LIB_OF[fn], fn.startswith("get_")
        tdt = lib_name in TDT
        add = lambda why, **kw: rows.append(pytest.param(fn, kw, id=f"{fn}-{why}"))  # noqa: E731
        if size_fn:
            add("null-size", sz=None)
            add("joint_dtype-2", joint_dtype=2)
            add("shape-refused", joint_size=100)
            if "beam" in names:
                add("beam-0", beam=0)
                add("beam-17", beam=17)
            if tdt:
                add("D-0", num_durations=0)
                add("D-9", num_durations=9)
            continue
        for p in REQUIRED[fn]:
            add("null-" + p, **{p: None})
        for p in ALIGNED4.get(fn, []):
            add("misaligned-" + p, **{p: MISALIGNED_4})
        add("workspace-260", workspace=MISALIGNED_256)
        add("joint_dtype-2", joint_dtype=2)
        add("blank-ge-V", blank=V + (3 if tdt else 0))
        if tdt:
            add("blank-in-duration-head", blank=V)
        add("shape-refused", joint_size=100)
        add("loc-cpu", loc=_lib.RNNT_CPU)
        add("maxU-9000", maxU=9000)
        if "beam" in names:
            add("beam-0", beam=0)
            add("beam-17", beam=17)
        if "beam" in names and "slots" in names:
            add("slots-x-beam-over-1024", slots=65, beam=16)
        if "max_hyp_len" in names:
            add("max_hyp_len-0", max_hyp_len=0)
        if tdt:
            add("D-0", num_durations=0)
            add("D-9", num_durations=9)
        if "durations" in names:
            for d in ([2, 1], [2, 3], [0], [1, 9]):
                add("durations-" + "-".join(map(str, d)), durations=d)
        if "max_per_frame" in names and tdt:
            add("max_per_frame-0", max_per_frame=0)
        if "G" in names:  # a NULL graph forwards to the base step: its checks still hold
            add("null-graph-null-pred_proj", graph=None, pred_proj=None)
            add("null-graph-beam-17", graph=None, beam=17)
            add("null-graph-workspace-260", graph=None, workspace=MISALIGNED_256)
            add("null-graph-blank-ge-V", graph=None, blank=V)
            add("null-graph-shape-refused", graph=None, joint_size=100)
            add("null-graph-loc-cpu", graph=None, loc=_lib.RNNT_CPU)
            if "timed" in fn or "stream" in fn:
                add("null-graph-misaligned-parents", graph=None, parents=MISALIGNED_4)
            if "stream" in fn:
                add("null-graph-max_hyp_len-0", graph=None, max_hyp_len=0)
    return rows


@pytest.fixture(scope="module", autouse=True)
def built():
    pkg.build()


@pytest.mark.parametrize("fn,spoilt", _rows())
def test_refused_before_anything_is_enqueued(fn, spoilt):
    assert call(fn, **spoilt) == INVALID


@pytest.mark.parametrize("fn", list(ALIGN_PATH))
def test_align_path_refuses_a_blank_no_vocabulary_holds(fn):
    """blank_label = INT_MAX: no int vocabulary holds it; refused without computing blank_label + 2."""
    for blank in (2**31 - 1, 2**31 - 2, -1):
        assert call(fn, blank=blank) == INVALID, blank
    import torch

    if not torch.cuda.is_available():  # (the well-formed call passes validation and then fails for lack of a device)
        assert call(fn) != INVALID and call(fn, blank=2**31 - 3) != INVALID


def _no_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("passes validation and would enqueue on the fake pointers")


@pytest.mark.parametrize("fn", [fn for fn in SIG if fn.startswith("get_")])
def test_size_queries_accept_the_well_formed_call(fn):
    """(no device is touched: these run everywhere)"""
    assert call(fn) == 0
    if "timed" in SIG[fn]:
        assert call(fn, timed=0) == 0


@pytest.mark.parametrize("fn", [fn for fn in SIG if not fn.startswith("get_")])
def test_accepted_on_fake_pointers(fn):
    _no_device()
    assert call(fn) != INVALID
    if "timed" in SIG[fn]:  # (untimed: the timed outputs must be NULL where the entry point takes them)
        nulls = {p: None for p in ("hyp_frames", "hyp_durations", "timed_stable_lengths") if p in SIG[fn]}
        assert call(fn, timed=0, **nulls) != INVALID
    if "G" in SIG[fn]:
        assert call(fn, graph=None) != INVALID


def test_untimed_offline_beam_entry_points_check_no_alignment():
    """The one difference between the twins that is kept: compute_rnnt_beam_begin / _step / _results take any pointer, their
    timed twins want 4-byte alignment (the refusals are rows above)."""
    _no_device()
    assert call("compute_rnnt_beam_step", parents=MISALIGNED_4) != INVALID
    assert call("compute_rnnt_beam_timed_step", parents=MISALIGNED_4) == INVALID
    assert call("compute_rnnt_beam_begin", W2=MISALIGNED_4) != INVALID
    assert call("compute_rnnt_beam_timed_begin", W2=MISALIGNED_4) == INVALID
    assert call("compute_rnnt_beam_results", hyps=MISALIGNED_4) != INVALID
    assert call("compute_rnnt_beam_timed_results", hyps=MISALIGNED_4) == INVALID
    for ext in ("biased", "lm"):  # the NULL-graph forward is the base step, alignment and all
        assert call("compute_rnnt_beam_step_" + ext, graph=None, parents=MISALIGNED_4) != INVALID
        assert call("compute_rnnt_beam_timed_step_" + ext, graph=None, parents=MISALIGNED_4) == INVALID


# ---- structure ----
FOREIGN = re.compile(r"^compute_rnnt_(joint|loss|encoder|lstm_train|frontend|align)")


@pytest.mark.parametrize("name", [n for n in ENTRIES if n != "base"])
def test_no_private_copy_of_a_base_entry_point(name):
    """The full symbol table, local symbols included: a library that borrows the base kernels carries none of the base boundary's
    loss, fused-joint, encoder, LSTM-trainer, front-end or aligner entry points (its version script would only hide them)."""
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    assert os.path.exists(nm), "neither binutils nm nor llvm-nm found: the symbol table cannot be checked"
    out = subprocess.run([nm, "--defined-only", lib_path(name)], check=True, capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert names, "the library is stripped: nothing to check"
    assert [n for n in names if FOREIGN.match(n)] == []


def test_no_source_includes_a_translation_unit():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            for i, line in enumerate(open(os.path.join(CSRC, f)), 1):
                if re.search(r'#include ".*\.hip"', line):
                    hits.append(f"{f}:{i}")
    assert hits == []
