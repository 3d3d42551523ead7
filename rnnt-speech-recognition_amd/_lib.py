"""ctypes binding of include/rnnt.h.  There is NO fallback: if the HIP library is missing or
fails to load, every entry point raises (the reference silently returns its logits instead,
utils/loss.py:14-22 -- deliberately not reproduced)."""
from __future__ import annotations

import ctypes
import os

from .build import BIAS_LIB_PATH as _DEFAULT_BIAS_LIB_PATH
from .build import LIB_PATH as _DEFAULT_LIB_PATH
from .build import LM_LIB_PATH as _DEFAULT_LM_LIB_PATH
from .build import MOD_LIB_PATH as _DEFAULT_MOD_LIB_PATH
from .build import MODALIGN_LIB_PATH as _DEFAULT_MODALIGN_LIB_PATH
from .build import PRUNED_LIB_PATH as _DEFAULT_PRUNED_LIB_PATH
from .build import SIMPLE_LIB_PATH as _DEFAULT_SIMPLE_LIB_PATH
from .build import PRUNEDJOINT_LIB_PATH as _DEFAULT_PRUNEDJOINT_LIB_PATH
from .build import PRUNERANGES_LIB_PATH as _DEFAULT_PRUNERANGES_LIB_PATH

# dev knob: load an experimental build of the library instead (scripts/build_variant.sh)
LIB_PATH = os.environ.get("RNNT_LIBWARPRNNT", _DEFAULT_LIB_PATH)
# the extension library goes with the base library: a variant base library is paired with the libwarprnnt_bias.so beside it, never
# with the stock one (the two step each other's workspaces)
BIAS_LIB_PATH = (_DEFAULT_BIAS_LIB_PATH if LIB_PATH == _DEFAULT_LIB_PATH
                 else os.path.join(os.path.dirname(LIB_PATH), "libwarprnnt_bias.so"))
# and so is the LM fusion library
LM_LIB_PATH = (_DEFAULT_LM_LIB_PATH if LIB_PATH == _DEFAULT_LIB_PATH
               else os.path.join(os.path.dirname(LIB_PATH), "libwarprnnt_lm.so"))
# the modified-topology library shares nothing with the base library (its own kernels and workspace): always this tree's build
MOD_LIB_PATH = _DEFAULT_MOD_LIB_PATH
# and so does the modified-lattice aligner
MODALIGN_LIB_PATH = _DEFAULT_MODALIGN_LIB_PATH
# and the pruned loss
PRUNED_LIB_PATH = _DEFAULT_PRUNED_LIB_PATH
# and the simple (additive joiner) loss, its first pass
SIMPLE_LIB_PATH = _DEFAULT_SIMPLE_LIB_PATH
# and the fused joint on the pruned band
PRUNEDJOINT_LIB_PATH = _DEFAULT_PRUNEDJOINT_LIB_PATH
# and the band positions between the two passes
PRUNERANGES_LIB_PATH = _DEFAULT_PRUNERANGES_LIB_PATH

RNNT_CPU, RNNT_GPU = 0, 1
STATUS_SUCCESS = 0

# every symbol include/rnnt.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "get_warprnnt_version",
    "rnntGetStatusString",
    "get_workspace_size",
    "compute_rnnt_loss",
    "compute_rnnt_loss_fwd",
    "compute_rnnt_loss_bwd",
    "compute_rnnt_loss_ex",
    "compute_rnnt_loss_flags",
    "compute_rnnt_loss_fastemit",
    "get_joint_workspace_size",
    "compute_rnnt_joint_loss",
    "compute_rnnt_joint_loss_fwd",
    "compute_rnnt_joint_loss_bwd",
    "compute_rnnt_joint_loss_bwd_fastemit",
    "compute_rnnt_joint_logits",
    "compute_rnnt_joint_net_logits",
    "get_rnnt_joint_backward_rows",
    "get_joint_net_workspace_size",
    "compute_rnnt_joint_net_loss",
    "compute_rnnt_joint_net_loss_fwd",
    "compute_rnnt_joint_net_loss_bwd",
    "compute_rnnt_joint_net_loss_bwd_fastemit",
    "get_rnnt_greedy_workspace_size",
    "compute_rnnt_greedy_begin",
    "compute_rnnt_greedy_step",
    "get_rnnt_beam_workspace_size",
    "compute_rnnt_beam_begin",
    "compute_rnnt_beam_step",
    "compute_rnnt_beam_results",
    "get_rnnt_prednet_workspace_size",
    "compute_rnnt_prednet_begin",
    "compute_rnnt_prednet_step",
    "get_rnnt_encoder_workspace_size",
    "compute_rnnt_encoder_begin",
    "compute_rnnt_encoder_run",
    "compute_rnnt_encoder_run_rows",
    "compute_rnnt_prednet_reset",
    "get_rnnt_greedy_stream_workspace_size",
    "compute_rnnt_greedy_stream_begin",
    "compute_rnnt_greedy_stream_feed",
    "get_rnnt_lstm_train_workspace_size",
    "compute_rnnt_lstm_train_fwd",
    "compute_rnnt_lstm_train_bwd",
    "get_rnnt_beam_stream_workspace_size",
    "compute_rnnt_beam_stream_begin",
    "compute_rnnt_beam_stream_feed",
    "compute_rnnt_beam_stream_step",
    "compute_rnnt_beam_stream_results",
    "get_rnnt_frontend_workspace_size",
    "compute_rnnt_frontend_begin",
    "compute_rnnt_frontend_feed",
    "get_rnnt_align_workspace_size",
    "compute_rnnt_align_cells",
    "compute_rnnt_align_path",
    "compute_rnnt_align",
    "compute_rnnt_greedy_step_timed",
    "compute_rnnt_greedy_stream_feed_timed",
    "get_rnnt_beam_timed_workspace_size",
    "compute_rnnt_beam_timed_begin",
    "compute_rnnt_beam_timed_step",
    "compute_rnnt_beam_timed_results",
    "get_rnnt_beam_stream_timed_workspace_size",
    "compute_rnnt_beam_stream_timed_begin",
    "compute_rnnt_beam_stream_timed_feed",
    "compute_rnnt_beam_stream_timed_step",
    "compute_rnnt_beam_stream_timed_results",
]


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


_lib = None
_bias_lib = None
BIAS_SYMBOLS = [  # include/rnnt_bias.h, exported by libwarprnnt_bias.so
    "compute_rnnt_beam_step_biased",
    "compute_rnnt_beam_timed_step_biased",
    "compute_rnnt_beam_stream_step_biased",
    "compute_rnnt_beam_stream_timed_step_biased",
]
_lm_lib = None
LM_SYMBOLS = [  # include/rnnt_lm.h, exported by libwarprnnt_lm.so
    "compute_rnnt_beam_step_lm",
    "compute_rnnt_beam_timed_step_lm",
    "compute_rnnt_beam_stream_step_lm",
    "compute_rnnt_beam_stream_timed_step_lm",
]
_mod_lib = None
MOD_SYMBOLS = [  # include/rnnt_modified.h, exported by libwarprnnt_mod.so
    "get_rnnt_modified_workspace_size",
    "compute_rnnt_loss_modified",
]
_modalign_lib = None
MODALIGN_SYMBOLS = [  # include/rnnt_modified_align.h, exported by libwarprnnt_modalign.so
    "get_rnnt_modified_align_workspace_size",
    "compute_rnnt_modified_align_cells",
    "compute_rnnt_modified_align_path",
    "compute_rnnt_modified_align",
]
_pruned_lib = None
PRUNED_SYMBOLS = [  # include/rnnt_pruned.h, exported by libwarprnnt_pruned.so
    "get_rnnt_pruned_workspace_size",
    "compute_rnnt_loss_pruned",
]
RNNT_PRUNED_STANDARD, RNNT_PRUNED_MODIFIED = 0, 1
_simple_lib = None
SIMPLE_SYMBOLS = [  # include/rnnt_simple.h, exported by libwarprnnt_simple.so
    "get_rnnt_simple_workspace_size",
    "compute_rnnt_loss_simple",
]
RNNT_SIMPLE_STANDARD, RNNT_SIMPLE_MODIFIED = 0, 1
_prunedjoint_lib = None
PRUNEDJOINT_SYMBOLS = [  # include/rnnt_pruned_joint.h, exported by libwarprnnt_prunedjoint.so
    "get_rnnt_pruned_joint_workspace_size",
    "compute_rnnt_joint_loss_pruned",
]
_pruneranges_lib = None
PRUNERANGES_SYMBOLS = [  # include/rnnt_prune_ranges.h, exported by libwarprnnt_pruneranges.so
    "compute_rnnt_prune_ranges",
]


class RNNTLibraryError(RuntimeError):
    pass


RNNT_VISIT_ALL = 0x100  # include/rnnt.h: no occupancy floor -- the gradient kernels visit every lattice cell / row


def load_bias():
    """Load libwarprnnt_bias.so (once): the biased beam steps of include/rnnt_bias.h.  They work on the workspaces that the
    entry points of load() set up.  Raises RNNTLibraryError loudly when the library is absent."""
    global _bias_lib
    if _bias_lib is not None:
        return _bias_lib
    if not os.path.exists(BIAS_LIB_PATH):
        raise RNNTLibraryError(f"{BIAS_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the biased beam steps.")
    try:
        lib = ctypes.CDLL(BIAS_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {BIAS_LIB_PATH}: {e}") from e
    vp, ci, gp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(rnntBiasGraph)
    for name, ints in zip(BIAS_SYMBOLS, (5, 5, 6, 6)):
        fn = getattr(lib, name)
        fn.restype = ci
        fn.argtypes = [vp] * 6 + [ci] * ints + [vp, rnntOptions, gp, vp]
    _bias_lib = lib
    return lib


def load_lm():
    """Load libwarprnnt_lm.so (once): the LM beam steps of include/rnnt_lm.h.  They work on the workspaces that the entry points
    of load() set up.  Raises RNNTLibraryError loudly when the library is absent."""
    global _lm_lib
    if _lm_lib is not None:
        return _lm_lib
    if not os.path.exists(LM_LIB_PATH):
        raise RNNTLibraryError(f"{LM_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the LM beam steps.")
    try:
        lib = ctypes.CDLL(LM_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {LM_LIB_PATH}: {e}") from e
    vp, ci, gp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(rnntLmGraph)
    for name, ints in zip(LM_SYMBOLS, (5, 5, 6, 6)):
        fn = getattr(lib, name)
        fn.restype = ci
        fn.argtypes = [vp] * 6 + [ci] * ints + [vp, rnntOptions, gp, vp]
    _lm_lib = lib
    return lib


def load_mod():
    """Load libwarprnnt_mod.so (once): the loss op on the modified (one symbol per frame) lattice, include/rnnt_modified.h.  Raises
    RNNTLibraryError loudly when the library is absent."""
    global _mod_lib
    if _mod_lib is not None:
        return _mod_lib
    if not os.path.exists(MOD_LIB_PATH):
        raise RNNTLibraryError(f"{MOD_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the modified topology of the loss.")
    try:
        lib = ctypes.CDLL(MOD_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {MOD_LIB_PATH}: {e}") from e
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.get_rnnt_modified_workspace_size.restype = ci
    lib.get_rnnt_modified_workspace_size.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_loss_modified.restype = ci
    lib.compute_rnnt_loss_modified.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions, ctypes.c_float]
    _mod_lib = lib
    return lib


def load_modalign():
    """Load libwarprnnt_modalign.so (once): forced alignment on the modified (one symbol per frame) lattice,
    include/rnnt_modified_align.h.  Raises RNNTLibraryError loudly when the library is absent."""
    global _modalign_lib
    if _modalign_lib is not None:
        return _modalign_lib
    if not os.path.exists(MODALIGN_LIB_PATH):
        raise RNNTLibraryError(f"{MODALIGN_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the modified-lattice aligner on a device.")
    try:
        lib = ctypes.CDLL(MODALIGN_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {MODALIGN_LIB_PATH}: {e}") from e
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.get_rnnt_modified_align_workspace_size.restype = ci
    lib.get_rnnt_modified_align_workspace_size.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_modified_align_cells.restype = ci
    lib.compute_rnnt_modified_align_cells.argtypes = [vp, ci, ci, vp, vp, vp, ci, ci, vp, rnntOptions]
    lib.compute_rnnt_modified_align_path.restype = ci
    lib.compute_rnnt_modified_align_path.argtypes = [vp, vp, vp, vp, vp, ci, vp, rnntOptions]
    lib.compute_rnnt_modified_align.restype = ci
    lib.compute_rnnt_modified_align.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, rnntOptions]
    _modalign_lib = lib
    return lib


def load_pruned():
    """Load libwarprnnt_pruned.so (once): the loss op on a band of S symbols per frame, include/rnnt_pruned.h.  Raises
    RNNTLibraryError loudly when the library is absent."""
    global _pruned_lib
    if _pruned_lib is not None:
        return _pruned_lib
    if not os.path.exists(PRUNED_LIB_PATH):
        raise RNNTLibraryError(f"{PRUNED_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the pruned loss on a device.")
    try:
        lib = ctypes.CDLL(PRUNED_LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {PRUNED_LIB_PATH}: {e}") from e
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.get_rnnt_pruned_workspace_size.restype = ci
    lib.get_rnnt_pruned_workspace_size.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_loss_pruned.restype = ci
    lib.compute_rnnt_loss_pruned.argtypes = [vp] * 7 + [ci] * 4 + [vp, vp, rnntOptions, ctypes.c_float]
    _pruned_lib = lib
    return lib


def load_prunedjoint():
    """Load libwarprnnt_prunedjoint.so (once): the fused joint on the pruned band, include/rnnt_pruned_joint.h.  Raises
    RNNTLibraryError if the library is missing or does not load."""
    global _prunedjoint_lib
    if _prunedjoint_lib is not None:
        return _prunedjoint_lib
    if not os.path.exists(PRUNEDJOINT_LIB_PATH):
        raise RNNTLibraryError(f"{PRUNEDJOINT_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the fused pruned joint on a device.")
    try:
        lib = ctypes.CDLL(PRUNEDJOINT_LIB_PATH)
    except OSError as e:
        raise RNNTLibraryError(f"failed to load {PRUNEDJOINT_LIB_PATH}: {e}") from e
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.get_rnnt_pruned_joint_workspace_size.restype = ci
    lib.get_rnnt_pruned_joint_workspace_size.argtypes = [ci, ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_joint_loss_pruned.restype = ci
    lib.compute_rnnt_joint_loss_pruned.argtypes = [vp] * 9 + [ci] * 5 + [vp] * 6 + [rnntOptions, ctypes.c_float]
    _prunedjoint_lib = lib
    return lib


def load_pruneranges():
    """Load libwarprnnt_pruneranges.so (once): the band positions of the pruned loss with a defined order of additions,
    include/rnnt_prune_ranges.h.  Raises RNNTLibraryError if it is missing: there is no fallback on a device."""
    global _pruneranges_lib
    if _pruneranges_lib is not None:
        return _pruneranges_lib
    if not os.path.exists(PRUNERANGES_LIB_PATH):
        raise RNNTLibraryError(f"{PRUNERANGES_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the ordered band positions on a device.")
    try:
        lib = ctypes.CDLL(PRUNERANGES_LIB_PATH)
    except OSError as e:
        raise RNNTLibraryError(f"failed to load {PRUNERANGES_LIB_PATH}: {e}") from e
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.compute_rnnt_prune_ranges.restype = ci
    lib.compute_rnnt_prune_ranges.argtypes = [vp, vp, vp, ci, ci, vp, rnntOptions]
    _pruneranges_lib = lib
    return lib


def load_simple():
    """Load libwarprnnt_simple.so (once): the loss op of an additive joiner, include/rnnt_simple.h.  Raises RNNTLibraryError if
    it is missing: there is no fallback on a device."""
    global _simple_lib
    if _simple_lib is not None:
        return _simple_lib
    if not os.path.exists(SIMPLE_LIB_PATH):
        raise RNNTLibraryError(f"{SIMPLE_LIB_PATH} not found: the HIP extension has not been built (__graft_entry__.build()). "
                               "There is no eager fallback for the simple loss on a device.")
    try:
        lib = ctypes.CDLL(SIMPLE_LIB_PATH)
    except OSError as e:
        raise RNNTLibraryError(f"failed to load {SIMPLE_LIB_PATH}: {e}") from e
    ci, vp = ctypes.c_int, ctypes.c_void_p
    lib.get_rnnt_simple_workspace_size.restype = ci
    lib.get_rnnt_simple_workspace_size.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_loss_simple.restype = ci
    lib.compute_rnnt_loss_simple.argtypes = [vp] * 9 + [ci] * 3 + [ctypes.c_float] * 2 + [vp, vp, rnntOptions]
    _simple_lib = lib
    return lib


def load():
    """Load libwarprnnt.so (once).  Raises RNNTLibraryError loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RNNTLibraryError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run scripts/build_rnnt.sh "
            "(or __graft_entry__.build()). There is no CPU/eager fallback for the transducer loss."
        )
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the ROCm runtime being present
        raise RNNTLibraryError(f"failed to load {LIB_PATH}: {e}") from e
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.get_warprnnt_version.restype = ci
    lib.rnntGetStatusString.restype = ctypes.c_char_p
    lib.rnntGetStatusString.argtypes = [ci]
    lib.get_workspace_size.restype = ci
    lib.get_workspace_size.argtypes = [ci, ci, ci, ctypes.c_bool, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_loss.restype = ci
    lib.compute_rnnt_loss.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions]
    lib.compute_rnnt_loss_fwd.restype = ci
    lib.compute_rnnt_loss_fwd.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions]
    lib.compute_rnnt_loss_bwd.restype = ci
    lib.compute_rnnt_loss_bwd.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, rnntOptions]
    lib.compute_rnnt_loss_ex.restype = ci
    lib.compute_rnnt_loss_ex.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_loss_flags"):
        lib.compute_rnnt_loss_flags.restype = ci
        lib.compute_rnnt_loss_flags.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions, ctypes.c_uint]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_loss_fastemit"):
        cf = ctypes.c_float
        lib.compute_rnnt_loss_fastemit.restype = ci
        lib.compute_rnnt_loss_fastemit.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, rnntOptions, ctypes.c_uint, cf]
        lib.compute_rnnt_joint_loss_bwd_fastemit.restype = ci
        lib.compute_rnnt_joint_loss_bwd_fastemit.argtypes = [vp] * 8 + [ci, ci, ci] + [vp] * 4 + [ci, vp, rnntOptions, cf]
        lib.compute_rnnt_joint_net_loss_bwd_fastemit.restype = ci
        lib.compute_rnnt_joint_net_loss_bwd_fastemit.argtypes = [vp] * 10 + [ci] * 4 + [vp] * 6 + [ci, vp, rnntOptions, cf]
    lib.get_joint_workspace_size.restype = ci
    lib.get_joint_workspace_size.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    lib.compute_rnnt_joint_loss.restype = ci
    lib.compute_rnnt_joint_loss.argtypes = [vp] * 8 + [ci, ci, ci] + [vp] * 5 + [ci, vp, rnntOptions]
    lib.compute_rnnt_joint_loss_fwd.restype = ci
    lib.compute_rnnt_joint_loss_fwd.argtypes = [vp] * 7 + [ci, ci, ci, vp, ci, vp, rnntOptions]
    lib.compute_rnnt_joint_loss_bwd.restype = ci
    lib.compute_rnnt_joint_loss_bwd.argtypes = [vp] * 8 + [ci, ci, ci] + [vp] * 4 + [ci, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_joint_logits"):  # (an older dev variant may lack it)
        lib.compute_rnnt_joint_logits.restype = ci
        lib.compute_rnnt_joint_logits.argtypes = [vp] * 4 + [ci, ci, ci, vp, ci, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "get_rnnt_joint_backward_rows"):
        lib.get_rnnt_joint_backward_rows.restype = ci
        lib.get_rnnt_joint_backward_rows.argtypes = [vp, ci, ci, ci, rnntOptions, ctypes.POINTER(ctypes.c_int)]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_joint_net_logits"):
        lib.compute_rnnt_joint_net_logits.restype = ci
        lib.compute_rnnt_joint_net_logits.argtypes = [vp] * 6 + [ci] * 4 + [vp, ci, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_joint_net_loss"):
        lib.get_joint_net_workspace_size.restype = ci
        lib.get_joint_net_workspace_size.argtypes = [ci] * 6 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_joint_net_loss.restype = ci
        lib.compute_rnnt_joint_net_loss.argtypes = [vp] * 10 + [ci] * 4 + [vp] * 7 + [ci, vp, rnntOptions]
        lib.compute_rnnt_joint_net_loss_fwd.restype = ci
        lib.compute_rnnt_joint_net_loss_fwd.argtypes = [vp] * 9 + [ci] * 4 + [vp, ci, vp, rnntOptions]
        lib.compute_rnnt_joint_net_loss_bwd.restype = ci
        lib.compute_rnnt_joint_net_loss_bwd.argtypes = [vp] * 10 + [ci] * 4 + [vp] * 6 + [ci, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_greedy_step"):
        lib.get_rnnt_greedy_workspace_size.restype = ci
        lib.get_rnnt_greedy_workspace_size.argtypes = [ci] * 5 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_greedy_begin.restype = ci
        lib.compute_rnnt_greedy_begin.argtypes = [vp] * 5 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_greedy_step.restype = ci
        lib.compute_rnnt_greedy_step.argtypes = [vp, vp, ci] + [vp] * 5 + [ci] * 4 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_beam_step"):
        lib.get_rnnt_beam_workspace_size.restype = ci
        lib.get_rnnt_beam_workspace_size.argtypes = [ci] * 6 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_beam_begin.restype = ci
        lib.compute_rnnt_beam_begin.argtypes = [vp] * 4 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_beam_step.restype = ci
        lib.compute_rnnt_beam_step.argtypes = [vp] * 6 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_beam_results.restype = ci
        lib.compute_rnnt_beam_results.argtypes = [vp] * 3 + [ci] * 5 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_prednet_step"):
        blk = ctypes.POINTER(rnntPrednetBlock)
        lib.get_rnnt_prednet_workspace_size.restype = ci
        lib.get_rnnt_prednet_workspace_size.argtypes = [blk] + [ci] * 5 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_prednet_begin.restype = ci
        lib.compute_rnnt_prednet_begin.argtypes = [vp, blk, ci, ci, ci, vp, ci, ci, vp, vp, rnntOptions]
        lib.compute_rnnt_prednet_step.restype = ci
        lib.compute_rnnt_prednet_step.argtypes = [vp, vp, vp, blk] + [ci] * 5 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_encoder_run"):
        blk, cf = ctypes.POINTER(rnntPrednetBlock), ctypes.c_float
        lib.get_rnnt_encoder_workspace_size.restype = ci
        lib.get_rnnt_encoder_workspace_size.argtypes = [blk] + [ci] * 6 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_encoder_begin.restype = ci
        lib.compute_rnnt_encoder_begin.argtypes = [blk, ci, ci, vp, vp, vp, vp, cf, ci, ci, ci, ci, vp, rnntOptions]
        lib.compute_rnnt_encoder_run.restype = ci
        lib.compute_rnnt_encoder_run.argtypes = [vp, ci, vp, blk, ci, ci, cf, ci, ci, ci, ci, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_greedy_stream_feed"):
        blk, cf = ctypes.POINTER(rnntPrednetBlock), ctypes.c_float
        lib.compute_rnnt_encoder_run_rows.restype = ci
        lib.compute_rnnt_encoder_run_rows.argtypes = [vp, ci, vp, vp, vp, blk, ci, ci, cf, ci, ci, ci, ci, vp, rnntOptions]
        lib.compute_rnnt_prednet_reset.restype = ci
        lib.compute_rnnt_prednet_reset.argtypes = [vp, vp, blk] + [ci] * 5 + [vp, rnntOptions]
        lib.get_rnnt_greedy_stream_workspace_size.restype = ci
        lib.get_rnnt_greedy_stream_workspace_size.argtypes = [ci] * 6 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_greedy_stream_begin.restype = ci
        lib.compute_rnnt_greedy_stream_begin.argtypes = [vp] * 4 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_greedy_stream_feed.restype = ci
        lib.compute_rnnt_greedy_stream_feed.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp] + [ci] * 5 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_lstm_train_fwd"):
        lib.get_rnnt_lstm_train_workspace_size.restype = ci
        lib.get_rnnt_lstm_train_workspace_size.argtypes = [ci] * 4 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_lstm_train_fwd.restype = ci
        lib.compute_rnnt_lstm_train_fwd.argtypes = [vp] * 6 + [ci] * 4 + [vp, rnntOptions]
        lib.compute_rnnt_lstm_train_bwd.restype = ci
        lib.compute_rnnt_lstm_train_bwd.argtypes = [vp] * 6 + [ci] * 4 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_beam_stream_feed"):
        lib.get_rnnt_beam_stream_workspace_size.restype = ci
        lib.get_rnnt_beam_stream_workspace_size.argtypes = [ci] * 8 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_beam_stream_begin.restype = ci
        lib.compute_rnnt_beam_stream_begin.argtypes = [vp] * 4 + [ci] * 7 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_feed.restype = ci
        lib.compute_rnnt_beam_stream_feed.argtypes = [vp, ci, vp, vp, vp] + [ci] * 7 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_step.restype = ci
        lib.compute_rnnt_beam_stream_step.argtypes = [vp] * 6 + [ci] * 6 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_results.restype = ci
        lib.compute_rnnt_beam_stream_results.argtypes = [vp] * 4 + [ci] * 6 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_frontend_feed"):
        lib.get_rnnt_frontend_workspace_size.restype = ci
        lib.get_rnnt_frontend_workspace_size.argtypes = [ci] * 7 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_frontend_begin.restype = ci
        lib.compute_rnnt_frontend_begin.argtypes = [vp, vp] + [ci] * 7 + [vp, rnntOptions]
        lib.compute_rnnt_frontend_feed.restype = ci
        lib.compute_rnnt_frontend_feed.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp] + [ci] * 7 + [vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_align"):
        lib.get_rnnt_align_workspace_size.restype = ci
        lib.get_rnnt_align_workspace_size.argtypes = [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_align_cells.restype = ci
        lib.compute_rnnt_align_cells.argtypes = [vp, ci, ci, vp, vp, vp, ci, ci, vp, rnntOptions]
        lib.compute_rnnt_align_path.restype = ci
        lib.compute_rnnt_align_path.argtypes = [vp, vp, vp, vp, vp, ci, vp, rnntOptions]
        lib.compute_rnnt_align.restype = ci
        lib.compute_rnnt_align.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, rnntOptions]
    if LIB_PATH == _DEFAULT_LIB_PATH or hasattr(lib, "compute_rnnt_greedy_step_timed"):
        lib.compute_rnnt_greedy_step_timed.restype = ci
        lib.compute_rnnt_greedy_step_timed.argtypes = [vp] * 4 + [ci] + [vp] * 6 + [ci] * 4 + [vp, rnntOptions]
        lib.compute_rnnt_greedy_stream_feed_timed.restype = ci
        lib.compute_rnnt_greedy_stream_feed_timed.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp] + [ci] * 5 + [vp, rnntOptions]
        lib.get_rnnt_beam_timed_workspace_size.restype = ci
        lib.get_rnnt_beam_timed_workspace_size.argtypes = [ci] * 6 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_beam_timed_begin.restype = ci
        lib.compute_rnnt_beam_timed_begin.argtypes = [vp] * 4 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_beam_timed_step.restype = ci
        lib.compute_rnnt_beam_timed_step.argtypes = [vp] * 6 + [ci] * 5 + [vp, rnntOptions]
        lib.compute_rnnt_beam_timed_results.restype = ci
        lib.compute_rnnt_beam_timed_results.argtypes = [vp] * 5 + [ci] * 5 + [vp, rnntOptions]
        lib.get_rnnt_beam_stream_timed_workspace_size.restype = ci
        lib.get_rnnt_beam_stream_timed_workspace_size.argtypes = [ci] * 8 + [ctypes.POINTER(ctypes.c_size_t)]
        lib.compute_rnnt_beam_stream_timed_begin.restype = ci
        lib.compute_rnnt_beam_stream_timed_begin.argtypes = [vp] * 4 + [ci] * 7 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_timed_feed.restype = ci
        lib.compute_rnnt_beam_stream_timed_feed.argtypes = [vp, ci, vp, vp, vp] + [ci] * 7 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_timed_step.restype = ci
        lib.compute_rnnt_beam_stream_timed_step.argtypes = [vp] * 6 + [ci] * 6 + [vp, rnntOptions]
        lib.compute_rnnt_beam_stream_timed_results.restype = ci
        lib.compute_rnnt_beam_stream_timed_results.argtypes = [vp] * 7 + [ci] * 6 + [vp, rnntOptions]
    _lib = lib
    return lib


def status_string(status: int) -> str:
    return load().rnntGetStatusString(status).decode()


def check(status: int, what: str):
    if status != STATUS_SUCCESS:
        raise RuntimeError(f"{what} failed: rnntStatus_t={status} ({status_string(status)})")


def make_options(stream: int, blank: int, maxT: int, maxU: int, loc: int = RNNT_GPU) -> rnntOptions:
    o = rnntOptions()
    o.loc = loc
    o.stream = stream
    o.blank_label = blank
    o.maxT = maxT
    o.maxU = maxU
    o.batch_first = True
    return o


def joint_workspace_bytes(maxT: int, maxU: int, minibatch: int, joint_size: int, alphabet_size: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_joint_workspace_size(maxT, maxU, minibatch, joint_size, alphabet_size, ctypes.byref(n)),
          "get_joint_workspace_size")
    return int(n.value)


def joint_net_workspace_bytes(maxT: int, maxU: int, minibatch: int, hidden_size: int, joint_size: int, alphabet_size: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_joint_net_workspace_size(maxT, maxU, minibatch, hidden_size, joint_size, alphabet_size, ctypes.byref(n)),
          "get_joint_net_workspace_size")
    return int(n.value)


def greedy_workspace_bytes(maxT: int, minibatch: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_greedy_workspace_size(maxT, minibatch, joint_size, alphabet_size, joint_dtype, ctypes.byref(n)),
          "get_rnnt_greedy_workspace_size")
    return int(n.value)


def beam_workspace_bytes(maxT: int, minibatch: int, beam: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_beam_workspace_size(maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype, ctypes.byref(n)),
          "get_rnnt_beam_workspace_size")
    return int(n.value)


def prednet_workspace_bytes(blocks, embed_size: int, vocab_size: int, joint_size: int, rows: int) -> int:
    """blocks: a ctypes array of rnntPrednetBlock (only the widths are read)."""
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_prednet_workspace_size(blocks, len(blocks), embed_size, vocab_size, joint_size, rows, ctypes.byref(n)),
          "get_rnnt_prednet_workspace_size")
    return int(n.value)


def encoder_workspace_bytes(blocks, feat_size: int, reduction_index: int, reduction_factor: int, rows: int,
                            max_frames: int) -> int:
    """blocks: a ctypes array of rnntPrednetBlock (only the widths are read)."""
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_encoder_workspace_size(blocks, len(blocks), feat_size, reduction_index, reduction_factor, rows, max_frames,
                                                 ctypes.byref(n)), "get_rnnt_encoder_workspace_size")
    return int(n.value)


def greedy_stream_workspace_bytes(max_chunk_frames: int, slots: int, enc_width: int, joint_size: int, alphabet_size: int,
                                  joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_greedy_stream_workspace_size(max_chunk_frames, slots, enc_width, joint_size, alphabet_size, joint_dtype,
                                                       ctypes.byref(n)), "get_rnnt_greedy_stream_workspace_size")
    return int(n.value)


def beam_stream_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, max_hyp_len: int, enc_width: int, joint_size: int,
                                alphabet_size: int, joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_beam_stream_workspace_size(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size,
                                                     alphabet_size, joint_dtype, ctypes.byref(n)),
          "get_rnnt_beam_stream_workspace_size")
    return int(n.value)


def beam_timed_workspace_bytes(maxT: int, minibatch: int, beam: int, joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_beam_timed_workspace_size(maxT, minibatch, beam, joint_size, alphabet_size, joint_dtype, ctypes.byref(n)),
          "get_rnnt_beam_timed_workspace_size")
    return int(n.value)


def beam_stream_timed_workspace_bytes(max_chunk_frames: int, slots: int, beam: int, max_hyp_len: int, enc_width: int,
                                      joint_size: int, alphabet_size: int, joint_dtype: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_beam_stream_timed_workspace_size(max_chunk_frames, slots, beam, max_hyp_len, enc_width, joint_size,
                                                           alphabet_size, joint_dtype, ctypes.byref(n)),
          "get_rnnt_beam_stream_timed_workspace_size")
    return int(n.value)


def frontend_workspace_bytes(max_chunk_samples: int, slots: int, frame_len: int, frame_step: int, mel_bins: int, stack: int,
                             row_multiple: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_frontend_workspace_size(max_chunk_samples, slots, frame_len, frame_step, mel_bins, stack, row_multiple,
                                                  ctypes.byref(n)), "get_rnnt_frontend_workspace_size")
    return int(n.value)


def align_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_align_workspace_size(maxT, maxU, minibatch, ctypes.byref(n)), "get_rnnt_align_workspace_size")
    return int(n.value)


def modified_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load_mod().get_rnnt_modified_workspace_size(maxT, maxU, minibatch, ctypes.byref(n)), "get_rnnt_modified_workspace_size")
    return int(n.value)


def modified_align_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load_modalign().get_rnnt_modified_align_workspace_size(maxT, maxU, minibatch, ctypes.byref(n)),
          "get_rnnt_modified_align_workspace_size")
    return int(n.value)


def pruned_workspace_bytes(maxT: int, s_range: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load_pruned().get_rnnt_pruned_workspace_size(maxT, s_range, minibatch, ctypes.byref(n)), "get_rnnt_pruned_workspace_size")
    return int(n.value)


def pruned_joint_workspace_bytes(maxT: int, s_range: int, minibatch: int, joint_size: int) -> int:
    n = ctypes.c_size_t(0)
    check(load_prunedjoint().get_rnnt_pruned_joint_workspace_size(maxT, s_range, minibatch, joint_size, ctypes.byref(n)),
          "get_rnnt_pruned_joint_workspace_size")
    return n.value


def simple_workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load_simple().get_rnnt_simple_workspace_size(maxT, maxU, minibatch, ctypes.byref(n)), "get_rnnt_simple_workspace_size")
    return int(n.value)


def lstm_train_workspace_bytes(rows: int, frames: int, hidden: int, proj: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_rnnt_lstm_train_workspace_size(rows, frames, hidden, proj, ctypes.byref(n)), "get_rnnt_lstm_train_workspace_size")
    return int(n.value)


def workspace_bytes(maxT: int, maxU: int, minibatch: int) -> int:
    n = ctypes.c_size_t(0)
    check(load().get_workspace_size(maxT, maxU, minibatch, True, ctypes.byref(n)), "get_workspace_size")
    return int(n.value)
