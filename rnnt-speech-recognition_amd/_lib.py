"""ctypes binding of include/rnnt.h and of the extension headers beside it (one library each, as build.LIBRARIES lists them).
There is NO fallback: if a HIP library is missing or fails to load, every entry point raises (the reference silently
returns its logits instead, utils/loss.py:14-22 -- deliberately not reproduced)."""
from __future__ import annotations

import ctypes
import os

from .build import BUILT_LIBRARIES, EVERY_LIBRARY, NEXT_LIBRARIES, lib_path

# dev knob: load an experimental build of the library instead (scripts/build_variant.sh)
LIB_PATH = os.environ.get("RNNT_LIBWARPRNNT", lib_path("base"))
# where each library of build.LIBRARIES is loaded from.  The bias and LM extensions go with the base library: a variant base library
# is paired with the libwarprnnt_bias.so / libwarprnnt_lm.so beside it, never with the stock ones (they step each other's
# workspaces).  Every other extension shares nothing with the base library (its own kernels and workspace): always this tree's build.
_PATHS = {name: lib_path(name) for name in EVERY_LIBRARY}
if LIB_PATH != _PATHS["base"]:
    _PATHS["base"] = LIB_PATH
    for _n in ("bias", "lm"):
        _PATHS[_n] = os.path.join(os.path.dirname(LIB_PATH), os.path.basename(_PATHS[_n]))
_NEXT_PATHS = {name: lib_path(name) for name in NEXT_LIBRARIES}  # (tests pin the keys of _PATHS: the rows added since)
_libs = {}  # name -> the loaded and bound library

RNNT_CPU, RNNT_GPU = 0, 1
STATUS_SUCCESS = 0


class _LocUnion(ctypes.Union):
    _fields_ = [("num_threads", ctypes.c_uint), ("stream", ctypes.c_void_p)]


class rnntOptions(ctypes.Structure):
    _anonymous_ = ("u",)
    _fields_ = [
        ("loc", ctypes.c_int),
        ("u", _LocUnion),
        ("blank_label", ctypes.c_int),
        ("maxT", ctypes.c_int),
        ("maxU", ctypes.c_int),
        ("batch_first", ctypes.c_bool),
    ]


class rnntPrednetBlock(ctypes.Structure):
    """One LSTM block of the prediction network (include/rnnt.h): device pointers, widths and the LayerNorm epsilon."""
    _fields_ = [
        ("W_ih", ctypes.c_void_p),
        ("W_hh", ctypes.c_void_p),
        ("b_ih", ctypes.c_void_p),
        ("b_hh", ctypes.c_void_p),
        ("W_hr", ctypes.c_void_p),
        ("ln_weight", ctypes.c_void_p),
        ("ln_bias", ctypes.c_void_p),
        ("hidden", ctypes.c_int),
        ("proj", ctypes.c_int),
        ("ln_eps", ctypes.c_float),
    ]


class rnntBiasGraph(ctypes.Structure):
    """The context graph of the biased beam steps (include/rnnt_bias.h): a host struct of device pointers."""
    _fields_ = [
        ("num_states", ctypes.c_int),
        ("num_arcs", ctypes.c_int),
        ("arc_offsets", ctypes.c_void_p),
        ("arc_tokens", ctypes.c_void_p),
        ("arc_next", ctypes.c_void_p),
        ("arc_bias", ctypes.c_void_p),
        ("fail_bias", ctypes.c_void_p),
    ]


class rnntLmGraph(ctypes.Structure):
    """The n-gram LM of the fused beam steps (include/rnnt_lm.h): a host struct of device pointers."""
    _fields_ = [
        ("num_states", ctypes.c_int),
        ("num_arcs", ctypes.c_int),
        ("empty_state", ctypes.c_int),
        ("unk_score", ctypes.c_float),
        ("arc_offsets", ctypes.c_void_p),
        ("arc_tokens", ctypes.c_void_p),
        ("arc_next", ctypes.c_void_p),
        ("arc_score", ctypes.c_void_p),
        ("backoff_next", ctypes.c_void_p),
        ("backoff_score", ctypes.c_void_p),
    ]


RNNT_PRUNED_STANDARD, RNNT_PRUNED_MODIFIED = 0, 1
RNNT_SIMPLE_STANDARD, RNNT_SIMPLE_MODIFIED = 0, 1
RNNT_VISIT_ALL = 0x100  # include/rnnt.h: no occupancy floor -- the gradient kernels visit every lattice cell / row

vp, ci, cu, cf, opt = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, rnntOptions
sz, blk = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(rnntPrednetBlock)
# Per library of build.LIBRARIES: {symbol: argtypes}, every symbol its header declares, in header order (tests/test_abi.py checks the
# keys against the header text and the export table).  Every function returns int (rnntStatus_t) but those of _RESTYPES.
_BASE = {
    "get_warprnnt_version": [],
    "rnntGetStatusString": [ci],
    "get_workspace_size": [ci, ci, ci, ctypes.c_bool, sz],
    "compute_rnnt_loss": [vp] * 5 + [ci, ci, vp, vp, opt],
    "compute_rnnt_loss_fwd": [vp] * 4 + [ci, ci, vp, vp, opt],
    "compute_rnnt_loss_bwd": [vp] * 6 + [ci, ci, vp, opt],
    "compute_rnnt_loss_ex": [vp] * 6 + [ci, ci, vp, vp, opt],
    "compute_rnnt_loss_flags": [vp] * 6 + [ci, ci, vp, vp, opt, cu],
    "compute_rnnt_loss_fastemit": [vp] * 6 + [ci, ci, vp, vp, opt, cu, cf],
    "get_joint_workspace_size": [ci] * 5 + [sz],
    "compute_rnnt_joint_loss": [vp] * 8 + [ci] * 3 + [vp] * 5 + [ci, vp, opt],
    "compute_rnnt_joint_loss_fwd": [vp] * 7 + [ci, ci, ci, vp, ci, vp, opt],
    "compute_rnnt_joint_loss_bwd": [vp] * 8 + [ci] * 3 + [vp] * 4 + [ci, vp, opt],
    "compute_rnnt_joint_loss_bwd_fastemit": [vp] * 8 + [ci] * 3 + [vp] * 4 + [ci, vp, opt, cf],
    "compute_rnnt_joint_logits": [vp] * 4 + [ci, ci, ci, vp, ci, vp, opt],
    "compute_rnnt_joint_net_logits": [vp] * 6 + [ci] * 4 + [vp, ci, vp, opt],
    "get_rnnt_joint_backward_rows": [vp, ci, ci, ci, opt, ctypes.POINTER(ci)],
    "get_joint_net_workspace_size": [ci] * 6 + [sz],
    "compute_rnnt_joint_net_loss": [vp] * 10 + [ci] * 4 + [vp] * 7 + [ci, vp, opt],
    "compute_rnnt_joint_net_loss_fwd": [vp] * 9 + [ci] * 4 + [vp, ci, vp, opt],
    "compute_rnnt_joint_net_loss_bwd": [vp] * 10 + [ci] * 4 + [vp] * 6 + [ci, vp, opt],
    "compute_rnnt_joint_net_loss_bwd_fastemit": [vp] * 10 + [ci] * 4 + [vp] * 6 + [ci, vp, opt, cf],
    "get_rnnt_greedy_workspace_size": [ci] * 5 + [sz],
    "compute_rnnt_greedy_begin": [vp] * 5 + [ci] * 5 + [vp, opt],
    "compute_rnnt_greedy_step": [vp, vp, ci] + [vp] * 5 + [ci] * 4 + [vp, opt],
    "get_rnnt_beam_workspace_size": [ci] * 6 + [sz],
    "compute_rnnt_beam_begin": [vp] * 4 + [ci] * 5 + [vp, opt],
    "compute_rnnt_beam_step": [vp] * 6 + [ci] * 5 + [vp, opt],
    "compute_rnnt_beam_results": [vp] * 3 + [ci] * 5 + [vp, opt],
    "get_rnnt_prednet_workspace_size": [blk] + [ci] * 5 + [sz],
    "compute_rnnt_prednet_begin": [vp, blk, ci, ci, ci, vp, ci, ci, vp, vp, opt],
    "compute_rnnt_prednet_step": [vp, vp, vp, blk] + [ci] * 5 + [vp, opt],
    "get_rnnt_encoder_workspace_size": [blk] + [ci] * 6 + [sz],
    "compute_rnnt_encoder_begin": [blk, ci, ci, vp, vp, vp, vp, cf, ci, ci, ci, ci, vp, opt],
    "compute_rnnt_encoder_run": [vp, ci, vp, blk, ci, ci, cf, ci, ci, ci, ci, vp, opt],
    "compute_rnnt_encoder_run_rows": [vp, ci, vp, vp, vp, blk, ci, ci, cf, ci, ci, ci, ci, vp, opt],
    "compute_rnnt_prednet_reset": [vp, vp, blk] + [ci] * 5 + [vp, opt],
    "get_rnnt_greedy_stream_workspace_size": [ci] * 6 + [sz],
    "compute_rnnt_greedy_stream_begin": [vp] * 4 + [ci] * 5 + [vp, opt],
    "compute_rnnt_greedy_stream_feed": [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp] + [ci] * 5 + [vp, opt],
    "get_rnnt_lstm_train_workspace_size": [ci] * 4 + [sz],
    "compute_rnnt_lstm_train_fwd": [vp] * 6 + [ci] * 4 + [vp, opt],
    "compute_rnnt_lstm_train_bwd": [vp] * 6 + [ci] * 4 + [vp, opt],
    "get_rnnt_beam_stream_workspace_size": [ci] * 8 + [sz],
    "compute_rnnt_beam_stream_begin": [vp] * 4 + [ci] * 7 + [vp, opt],
    "compute_rnnt_beam_stream_feed": [vp, ci, vp, vp, vp] + [ci] * 7 + [vp, opt],
    "compute_rnnt_beam_stream_step": [vp] * 6 + [ci] * 6 + [vp, opt],
    "compute_rnnt_beam_stream_results": [vp] * 4 + [ci] * 6 + [vp, opt],
    "get_rnnt_frontend_workspace_size": [ci] * 7 + [sz],
    "compute_rnnt_frontend_begin": [vp, vp] + [ci] * 7 + [vp, opt],
    "compute_rnnt_frontend_feed": [vp, ci, vp, vp, vp, ci, vp, vp] + [ci] * 7 + [vp, opt],
    "get_rnnt_align_workspace_size": [ci, ci, ci, sz],
    "compute_rnnt_align_cells": [vp, ci, ci, vp, vp, vp, ci, ci, vp, opt],
    "compute_rnnt_align_path": [vp] * 5 + [ci, vp, opt],
    "compute_rnnt_align": [vp] * 4 + [ci, ci] + [vp] * 4 + [opt],
    "compute_rnnt_greedy_step_timed": [vp] * 4 + [ci] + [vp] * 6 + [ci] * 4 + [vp, opt],
    "compute_rnnt_greedy_stream_feed_timed": [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp] + [ci] * 5 + [vp, opt],
    "get_rnnt_beam_timed_workspace_size": [ci] * 6 + [sz],
    "compute_rnnt_beam_timed_begin": [vp] * 4 + [ci] * 5 + [vp, opt],
    "compute_rnnt_beam_timed_step": [vp] * 6 + [ci] * 5 + [vp, opt],
    "compute_rnnt_beam_timed_results": [vp] * 5 + [ci] * 5 + [vp, opt],
    "get_rnnt_beam_stream_timed_workspace_size": [ci] * 8 + [sz],
    "compute_rnnt_beam_stream_timed_begin": [vp] * 4 + [ci] * 7 + [vp, opt],
    "compute_rnnt_beam_stream_timed_feed": [vp, ci, vp, vp, vp] + [ci] * 7 + [vp, opt],
    "compute_rnnt_beam_stream_timed_step": [vp] * 6 + [ci] * 6 + [vp, opt],
    "compute_rnnt_beam_stream_timed_results": [vp] * 7 + [ci] * 6 + [vp, opt],
}
# the biased and the LM steps: each one's arguments are its base step's plus the graph and the states
_BEAM_STEPS = ("compute_rnnt_beam_step", "compute_rnnt_beam_timed_step", "compute_rnnt_beam_stream_step",
               "compute_rnnt_beam_stream_timed_step")
SIGNATURES = {
    "base": _BASE,
    "bias": {s + "_biased": _BASE[s] + [ctypes.POINTER(rnntBiasGraph), vp] for s in _BEAM_STEPS},
    "mod": {
        "get_rnnt_modified_workspace_size": [ci, ci, ci, sz],
        "compute_rnnt_loss_modified": [vp] * 6 + [ci, ci, vp, vp, opt, cf],
    },
    "modalign": {
        "get_rnnt_modified_align_workspace_size": [ci, ci, ci, sz],
        "compute_rnnt_modified_align_cells": [vp, ci, ci, vp, vp, vp, ci, ci, vp, opt],
        "compute_rnnt_modified_align_path": [vp] * 5 + [ci, vp, opt],
        "compute_rnnt_modified_align": [vp] * 4 + [ci, ci] + [vp] * 4 + [opt],
    },
    "pruned": {
        "get_rnnt_pruned_workspace_size": [ci, ci, ci, sz],
        "compute_rnnt_loss_pruned": [vp] * 7 + [ci] * 4 + [vp, vp, opt, cf],
    },
    "simple": {
        "get_rnnt_simple_workspace_size": [ci, ci, ci, sz],
        "compute_rnnt_loss_simple": [vp] * 9 + [ci] * 3 + [cf, cf, vp, vp, opt],
    },
    "prunedjoint": {
        "get_rnnt_pruned_joint_workspace_size": [ci, ci, ci, ci, sz],
        "compute_rnnt_joint_loss_pruned": [vp] * 9 + [ci] * 5 + [vp] * 6 + [opt, cf],
    },
    "pruneranges": {"compute_rnnt_prune_ranges": [vp, vp, vp, ci, ci, vp, opt]},
    "lm": {s + "_lm": _BASE[s] + [ctypes.POINTER(rnntLmGraph), vp] for s in _BEAM_STEPS},
}
# the libraries of build.MORE_LIBRARIES, in the same form (a second table for the reason given there).  Both named tables are
# frozen by the tests that pin them, as is the merged table (_ALL_SIGNATURES) below: a new library's row joins _LATER_SIGNATURES.
MORE_SIGNATURES = {
    "tdt": {
        "get_rnnt_tdt_workspace_size": [ci, ci, ci, ci, sz],
        "compute_rnnt_loss_tdt": [vp] * 6 + [ci, ctypes.POINTER(ci), ci, cf, ci, vp, vp, opt],
    },
}
_ALL_SIGNATURES = {
    **SIGNATURES,
    **MORE_SIGNATURES,
    "tdtgreedy": {
        "get_rnnt_tdt_greedy_workspace_size": [ci] * 6 + [sz],
        "compute_rnnt_tdt_greedy_begin": [vp] * 5 + [ci, ci, ctypes.POINTER(ci), ci, ci, ci, ci, vp, opt],
        "compute_rnnt_tdt_greedy_step": [vp] * 4 + [ci] + [vp] * 5 + [ci] * 5 + [vp, opt],
    },
}
# the libraries of build.LATER_LIBRARIES (the three tables above are frozen by the tests that pin them; this one is open)
_LATER_SIGNATURES = {
    "tdtstream": {
        "get_rnnt_tdt_greedy_stream_workspace_size": [ci] * 7 + [sz],
        "compute_rnnt_tdt_greedy_stream_begin": [vp] * 4 + [ci, ci, ci, ctypes.POINTER(ci), ci, ci, ci, vp, opt],
        "compute_rnnt_tdt_greedy_stream_feed": [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp] + [ci] * 6 + [vp, opt],
        "compute_rnnt_tdt_greedy_stream_step": [vp] * 4 + [ci] + [vp] * 5 + [ci] * 5 + [vp, opt],
    },
    "tdtalign": {
        "get_rnnt_tdt_align_workspace_size": [ci, ci, ci, ci, sz],
        "compute_rnnt_tdt_align_cells": [vp, ci, ci, vp, vp, vp, ci, ctypes.POINTER(ci), ci, cf, ci, vp, opt],
        "compute_rnnt_tdt_align_path": [vp] * 6 + [ctypes.POINTER(ci), ci, ci, vp, opt],
        "compute_rnnt_tdt_align": [vp] * 4 + [ci, ctypes.POINTER(ci), ci, cf, ci] + [vp] * 5 + [opt],
    },
    "tdtbeam": {
        "get_rnnt_tdt_beam_workspace_size": [ci] * 8 + [sz],
        "compute_rnnt_tdt_beam_begin": [vp] * 4 + [ci, ci, ctypes.POINTER(ci)] + [ci] * 5 + [vp, opt],
        "compute_rnnt_tdt_beam_step": [vp] * 7 + [ci] * 7 + [vp, opt],
        "compute_rnnt_tdt_beam_results": [vp] * 6 + [ci] * 7 + [vp, opt],
    },
    "tdtjoint": {
        "get_rnnt_tdt_joint_workspace_size": [ci] * 5 + [sz],
        "compute_rnnt_joint_loss_tdt": [vp] * 8 + [ci, ci, ctypes.POINTER(ci), ci, cf, ci] + [vp] * 6 + [opt],
    },
    "tdtbeamstream": {
        "get_rnnt_tdt_beam_stream_workspace_size": [ci] * 10 + [sz],
        "compute_rnnt_tdt_beam_stream_begin": [vp] * 4 + [ci, ci, ci, ctypes.POINTER(ci)] + [ci] * 6 + [vp, opt],
        "compute_rnnt_tdt_beam_stream_feed": [vp, ci, vp, vp, vp] + [ci] * 9 + [vp, opt],
        "compute_rnnt_tdt_beam_stream_step": [vp] * 7 + [ci] * 8 + [vp, opt],
        "compute_rnnt_tdt_beam_stream_results": [vp] * 8 + [ci] * 8 + [vp, opt],
    },
}
_EVERY_SIGNATURE = {**_ALL_SIGNATURES, **_LATER_SIGNATURES}
# the libraries of build.NEXT_LIBRARIES (the tables above are frozen by the tests that pin them, their lengths included)
_NEXT_SIGNATURES = {
    "multibeam": {
        "get_rnnt_multibeam_workspace_size": [ci] * 8 + [sz],
        "compute_rnnt_multibeam_begin": [vp] * 4 + [ci] * 7 + [vp, opt],
        "compute_rnnt_multibeam_step": [vp] * 3 + [ci] * 7 + [vp, opt],
        "compute_rnnt_multibeam_results": [vp] * 3 + [ci] * 7 + [vp, opt],
    },
    "multibeamstream": {
        "get_rnnt_multibeam_stream_workspace_size": [ci] * 10 + [sz],
        "compute_rnnt_multibeam_stream_begin": [vp] * 4 + [ci] * 9 + [vp, opt],
        "compute_rnnt_multibeam_stream_feed": [vp, ci, vp, vp, vp] + [ci] * 9 + [vp, opt],
        "compute_rnnt_multibeam_stream_step": [vp] * 3 + [ci] * 8 + [vp, opt],
        "compute_rnnt_multibeam_stream_results": [vp] * 6 + [ci] * 8 + [vp, opt],
    },
    "ctc": {
        "get_rnnt_ctc_workspace_size": [ci, ci, ci, sz],
        "compute_rnnt_ctc_loss": [vp] * 6 + [ci, ci, vp, vp, opt],
        "compute_rnnt_ctc_greedy": [vp, vp, ci, ci, vp, vp, vp, opt],
    },
}
_BUILT_SIGNATURES = {**_EVERY_SIGNATURE, **_NEXT_SIGNATURES}
_RESTYPES = {"rnntGetStatusString": ctypes.c_char_p}
del vp, ci, cu, cf, opt, sz, blk
SYMBOLS, BIAS_SYMBOLS, LM_SYMBOLS = list(SIGNATURES["base"]), list(SIGNATURES["bias"]), list(SIGNATURES["lm"])


class RNNTLibraryError(RuntimeError):
    pass


def _load(name: str):
    """Load one library of build.BUILT_LIBRARIES (once) and bind its row of _BUILT_SIGNATURES on it.
    Raises RNNTLibraryError loudly when it is absent, does not load or lacks a symbol: there is no fallback."""
    if name in _libs:
        return _libs[name]
    path = _PATHS[name] if name in _PATHS else _NEXT_PATHS[name]
    if not os.path.exists(path):
        raise RNNTLibraryError(f"{path} not found: the HIP extension has not been built. Run scripts/build_rnnt.sh (or "
                               f"__graft_entry__.build()). There is no eager fallback for include/{BUILT_LIBRARIES[name].header}.")
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {path}: {e}") from e
    variant = name == "base" and path != lib_path("base")  # an older revision (scripts/build_variant.sh) may lack the newer symbols
    for symbol, argtypes in _BUILT_SIGNATURES[name].items():
        if not hasattr(lib, symbol):
            if variant:
                continue
            raise RNNTLibraryError(f"{path} does not define {symbol}: it is not this tree's build")
        fn = getattr(lib, symbol)
        fn.restype, fn.argtypes = _RESTYPES.get(symbol, ctypes.c_int), argtypes
    _libs[name] = lib
    return lib


def load():
    """libwarprnnt.so: include/rnnt.h."""
    return _load("base")


def load_bias():
    """libwarprnnt_bias.so: the biased beam steps of include/rnnt_bias.h, on the workspaces that the entry points of load() set up."""
    return _load("bias")


def load_lm():
    """libwarprnnt_lm.so: the LM beam steps of include/rnnt_lm.h, on the workspaces that the entry points of load() set up."""
    return _load("lm")


def load_mod():
    """libwarprnnt_mod.so: the loss op on the modified (one symbol per frame) lattice, include/rnnt_modified.h."""
    return _load("mod")


def load_modalign():
    """libwarprnnt_modalign.so: forced alignment on the modified lattice, include/rnnt_modified_align.h."""
    return _load("modalign")


def load_pruned():
    """libwarprnnt_pruned.so: the loss op on a band of S symbols per frame, include/rnnt_pruned.h."""
    return _load("pruned")


def load_simple():
    """libwarprnnt_simple.so: the loss op of an additive joiner, include/rnnt_simple.h."""
    return _load("simple")


def load_prunedjoint():
    """libwarprnnt_prunedjoint.so: the fused joint on the pruned band, include/rnnt_pruned_joint.h."""
    return _load("prunedjoint")


def load_pruneranges():
    """libwarprnnt_pruneranges.so: the band positions of the pruned loss in a defined order of additions, include/rnnt_prune_ranges.h."""
    return _load("pruneranges")


def load_tdt():
    """libwarprnnt_tdt.so: the token-and-duration (TDT) transducer loss, include/rnnt_tdt.h."""
    return _load("tdt")


def load_tdtgreedy():
    """libwarprnnt_tdtgreedy.so: batched greedy decoding of the TDT transducer, include/rnnt_tdt_greedy.h."""
    return _load("tdtgreedy")


def load_tdtstream():
    """libwarprnnt_tdtstream.so: streaming greedy decoding of the TDT transducer over slots, include/rnnt_tdt_stream.h."""
    return _load("tdtstream")


def load_tdtalign():
    """libwarprnnt_tdtalign.so: forced alignment on the TDT lattice, include/rnnt_tdt_align.h."""
    return _load("tdtalign")


def load_tdtbeam():
    """libwarprnnt_tdtbeam.so: batched beam search of the TDT transducer, include/rnnt_tdt_beam.h."""
    return _load("tdtbeam")


def load_tdtjoint():
    """libwarprnnt_tdtjoint.so: the fused TDT joint, include/rnnt_tdt_joint.h."""
    return _load("tdtjoint")


def load_tdtbeamstream():
    """libwarprnnt_tdtbeamstream.so: streaming beam search of the TDT transducer over slots, include/rnnt_tdt_beam_stream.h."""
    return _load("tdtbeamstream")


def load_multibeam():
    """libwarprnnt_multibeam.so: batched beam search with several symbols per frame, include/rnnt_beam_multi.h."""
    return _load("multibeam")


def load_multibeam_stream():
    """libwarprnnt_multibeamstream.so: streaming beam search with several symbols per frame over slots,
    include/rnnt_beam_multi_stream.h."""
    return _load("multibeamstream")


def load_ctc():
    """libwarprnnt_ctc.so: the CTC loss and the greedy CTC decoder of the auxiliary head, include/rnnt_ctc.h."""
    return _load("ctc")


def status_string(status: int) -> str:
    return load().rnntGetStatusString(status).decode()


def check(status: int, what: str):
    if status != STATUS_SUCCESS:
        raise RuntimeError(f"{what} failed: rnntStatus_t={status} ({status_string(status)})")


def ptr(x):
    """An optional tensor as a C ABI argument: its address, or None (a null pointer) for None."""
    return None if x is None else x.data_ptr()


def make_options(stream: int, blank: int, maxT: int, maxU: int, loc: int = RNNT_GPU) -> rnntOptions:
    o = rnntOptions()
    o.loc = loc
    o.stream = stream
    o.blank_label = blank
    o.maxT = maxT
    o.maxU = maxU
    o.batch_first = True
    return o


def _size(lib, fn_name: str, *args) -> int:
    """What a get_*_workspace_size entry point writes through its last argument."""
    n = ctypes.c_size_t(0)
    check(getattr(lib, fn_name)(*args, ctypes.byref(n)), fn_name)
    return int(n.value)


def workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load(), "get_workspace_size", maxT, maxU, minibatch, True)


def joint_workspace_bytes(maxT: int, maxU: int, minibatch: int, joint_size: int, alphabet_size: int) -> int:
    return _size(load(), "get_joint_workspace_size", maxT, maxU, minibatch, joint_size, alphabet_size)


def joint_net_workspace_bytes(maxT: int, maxU: int, minibatch: int, hidden_size: int, joint_size: int, alphabet_size: int) -> int:
    return _size(load(), "get_joint_net_workspace_size", maxT, maxU, minibatch, hidden_size, joint_size, alphabet_size)


def greedy_workspace_bytes(maxT: int, minibatch: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_greedy_workspace_size", maxT, minibatch, joint_size, alphabet_size, joint_dtype)


def beam_workspace_bytes(maxT: int, minibatch: int, beam: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_beam_workspace_size", maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype)


def prednet_workspace_bytes(blocks, embed_size: int, vocab_size: int, joint_size: int, rows: int) -> int:
    """blocks: a ctypes array of rnntPrednetBlock (only the widths are read)."""
    return _size(load(), "get_rnnt_prednet_workspace_size", blocks, len(blocks), embed_size, vocab_size, joint_size, rows)


def encoder_workspace_bytes(blocks, feat_size: int, reduction_index: int, reduction_factor: int, rows: int,
                            max_frames: int) -> int:
    """blocks: a ctypes array of rnntPrednetBlock (only the widths are read)."""
    return _size(load(), "get_rnnt_encoder_workspace_size", blocks, len(blocks), feat_size, reduction_index, reduction_factor, rows,
                 max_frames)


def greedy_stream_workspace_bytes(max_chunk_frames: int, slots: int, enc_width: int, joint_size: int, alphabet_size: int,
                                  joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_greedy_stream_workspace_size", max_chunk_frames, slots, enc_width, joint_size, alphabet_size,
                 joint_dtype)


def beam_stream_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, max_hyp_len: int, enc_width: int, joint_size: int,
                                alphabet_size: int, joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_beam_stream_workspace_size", max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size,
                 alphabet_size, joint_dtype)


def beam_timed_workspace_bytes(maxT: int, minibatch: int, beam: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_beam_timed_workspace_size", maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype)


def beam_stream_timed_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, max_hyp_len: int, enc_width: int,
                                      joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    return _size(load(), "get_rnnt_beam_stream_timed_workspace_size", max_chunk_frames, slots, beam, max_hyp_len, enc_width,
                 joint_size, alphabet_size, joint_dtype)


def frontend_workspace_bytes(max_chunk_samples: int, slots: int, frame_len: int, frame_step: int, mel_bins: int, stack: int,
                             row_multiple: int) -> int:
    return _size(load(), "get_rnnt_frontend_workspace_size", max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack,
                 row_multiple)


def align_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load(), "get_rnnt_align_workspace_size", maxT, maxU, minibatch)


def lstm_train_workspace_bytes(rows: int, frames: int, hidden: int, proj: int) -> int:
    return _size(load(), "get_rnnt_lstm_train_workspace_size", rows, frames, hidden, proj)


def modified_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load_mod(), "get_rnnt_modified_workspace_size", maxT, maxU, minibatch)


def modified_align_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load_modalign(), "get_rnnt_modified_align_workspace_size", maxT, maxU, minibatch)


def pruned_workspace_bytes(maxT: int, s_range: int, minibatch: int) -> int:
    return _size(load_pruned(), "get_rnnt_pruned_workspace_size", maxT, s_range, minibatch)


def pruned_joint_workspace_bytes(maxT: int, s_range: int, minibatch: int, joint_size: int) -> int:
    return _size(load_prunedjoint(), "get_rnnt_pruned_joint_workspace_size", maxT, s_range, minibatch, joint_size)


def simple_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load_simple(), "get_rnnt_simple_workspace_size", maxT, maxU, minibatch)


def tdt_workspace_bytes(maxT: int, maxU: int, minibatch: int, num_durations: int) -> int:
    return _size(load_tdt(), "get_rnnt_tdt_workspace_size", maxT, maxU, minibatch, num_durations)


def tdt_greedy_workspace_bytes(maxT: int, minibatch: int, joint_size: int, alphabet_size: int, num_durations: int,
                               joint_dtype: int) -> int:
    return _size(load_tdtgreedy(), "get_rnnt_tdt_greedy_workspace_size", maxT, minibatch, joint_size, alphabet_size, num_durations,
                 joint_dtype)


def tdt_align_workspace_bytes(maxT: int, maxU: int, minibatch: int, num_durations: int) -> int:
    return _size(load_tdtalign(), "get_rnnt_tdt_align_workspace_size", maxT, maxU, minibatch, num_durations)


def tdt_beam_workspace_bytes(maxT: int, minibatch: int, beam: int, joint_size: int, alphabet_size: int, num_durations: int,
                             joint_dtype: int, timed: bool = False) -> int:
    return _size(load_tdtbeam(), "get_rnnt_tdt_beam_workspace_size", maxT, minibatch, beam, joint_size, alphabet_size, num_durations,
                 joint_dtype, int(bool(timed)))


def tdt_joint_workspace_bytes(maxT: int, maxU: int, minibatch: int, num_durations: int, joint_size: int) -> int:
    return _size(load_tdtjoint(), "get_rnnt_tdt_joint_workspace_size", maxT, maxU, minibatch, num_durations, joint_size)


def tdt_greedy_stream_workspace_bytes(max_chunk_frames: int, slots: int, enc_width: int, joint_size: int, alphabet_size: int,
                                      num_durations: int, joint_dtype: int) -> int:
    return _size(load_tdtstream(), "get_rnnt_tdt_greedy_stream_workspace_size", max_chunk_frames, slots, enc_width, joint_size,
                 alphabet_size, num_durations, joint_dtype)


def tdt_beam_stream_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, max_hyp_len: int, enc_width: int, joint_size: int,
                                    alphabet_size: int, num_durations: int, joint_dtype: int, timed: bool = False) -> int:
    return _size(load_tdtbeamstream(), "get_rnnt_tdt_beam_stream_workspace_size", max_chunk_frames, slots, beam, max_hyp_len, enc_width,
                 joint_size, alphabet_size, num_durations, joint_dtype, int(bool(timed)))


def multibeam_workspace_bytes(maxT: int, minibatch: int, beam: int, symbols_per_frame: int, max_hyp_len: int, joint_size: int,
                              alphabet_size: int, joint_dtype: int) -> int:
    return _size(load_multibeam(), "get_rnnt_multibeam_workspace_size", maxT, minibatch, beam, symbols_per_frame, max_hyp_len,
                 joint_size, alphabet_size, joint_dtype)


def multibeam_stream_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, symbols_per_frame: int, max_hyp_len: int,
                                     enc_width: int, joint_size: int, alphabet_size: int, joint_dtype: int, timed: bool = False) -> int:
    return _size(load_multibeam_stream(), "get_rnnt_multibeam_stream_workspace_size", max_chunk_frames, slots, beam,
                 symbols_per_frame, max_hyp_len, enc_width, joint_size, alphabet_size, joint_dtype, int(bool(timed)))


def ctc_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    return _size(load_ctc(), "get_rnnt_ctc_workspace_size", maxT, maxU, minibatch)
