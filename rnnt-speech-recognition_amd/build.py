"""Build driver for libwarprnnt.so (the MI355X counterpart of the reference's
scripts/build_rnnt.sh:1-13, which runs cmake+make on warp-transducer and installs the binding).

hipcc cross-compiles for gfx950 without a GPU.  The library is built IN-TREE
(`rnnt-speech-recognition_amd/lib/libwarprnnt.so`) so that it travels with the source snapshot."""
from __future__ import annotations

import os
import shutil
import subprocess
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")


@dataclass(frozen=True)
class Library:
    """One shared library: lib/libwarprnnt.so ("base") or lib/libwarprnnt_<name>.so."""
    header: str  # its public header under include/
    sources: tuple  # its own sources under csrc/
    borrowed: tuple = ()  # sources of other entries whose objects it links as well, ahead of its own
    version_script: str | None = None  # under csrc/: the library exports what it names alone


_BASE_KERNELS = ("rnnt_kernels.hip", "rnnt_lin_kernels.hip", "joint_kernels.hip", "joint_f16_kernels.hip", "dense_kernels.hip",
                 "greedy_kernels.hip", "beam_kernels.hip", "prednet_kernels.hip", "encoder_kernels.hip", "lstm_train_kernels.hip",
                 "frontend_kernels.hip", "align_kernels.hip")
# The one description of what is built.  Every source is compiled once; a library links the objects of `borrowed` and `sources`.
# Every extension is self-contained (its own kernels, entry points and workspace) except where `borrowed` says otherwise, and its
# version script exports its own entry points alone: libwarprnnt.so holds nothing of any extension.
LIBRARIES = {
    "base": Library("rnnt.h", _BASE_KERNELS + ("rnnt_entrypoint.hip",)),
    # contextual biasing in the beam searches.  The host side of the beam search rests on the base kernels: it links their objects
    # and its own entry points (the argument checks both boundaries share are in rnnt_decode_host.h)
    "bias": Library("rnnt_bias.h", ("beam_bias_kernels.hip", "rnnt_bias_entrypoint.hip"), _BASE_KERNELS, "rnnt_bias.map"),
    # the loss op on the modified (one symbol per frame) lattice
    "mod": Library("rnnt_modified.h", ("rnnt_mod_kernels.hip", "rnnt_mod_entrypoint.hip"), (), "rnnt_mod.map"),
    # forced alignment on the modified lattice
    "modalign": Library("rnnt_modified_align.h", ("rnnt_modalign_kernels.hip", "rnnt_modalign_entrypoint.hip"), (), "rnnt_modalign.map"),
    # the loss op on a band of S symbols per frame
    "pruned": Library("rnnt_pruned.h", ("rnnt_pruned_kernels.hip", "rnnt_pruned_entrypoint.hip"), (), "rnnt_pruned.map"),
    # the loss op of an additive joiner (am + lm), the first pass of the pruned loss
    "simple": Library("rnnt_simple.h", ("rnnt_simple_kernels.hip", "rnnt_simple_entrypoint.hip"), (), "rnnt_simple.map"),
    # the fused joint on the pruned band: its own kernels and the lattice sweeps of the pruned loss, unchanged
    "prunedjoint": Library("rnnt_pruned_joint.h", ("rnnt_pruned_joint_kernels.hip", "rnnt_pruned_joint_entrypoint.hip"),
                           ("rnnt_pruned_kernels.hip",), "rnnt_pruned_joint.map"),
    # the band positions between the two passes of the pruned loss, with a defined order of additions (no workspace)
    "pruneranges": Library("rnnt_prune_ranges.h", ("rnnt_prune_ranges_kernels.hip", "rnnt_prune_ranges_entrypoint.hip"), (),
                           "rnnt_prune_ranges.map"),
    # n-gram LM shallow fusion in the beam searches: the base kernel objects and its own entry points, as "bias"
    "lm": Library("rnnt_lm.h", ("beam_lm_kernels.hip", "rnnt_lm_entrypoint.hip"), _BASE_KERNELS, "rnnt_lm.map"),
}
# More rows of the same table.  tests/test_abi.py pins list(LIBRARIES) to its own nine names and tests/test_abi_tdt.py pins
# list(MORE_LIBRARIES) to ["tdt"]: both named tables are frozen, and so is the merged table (ALL_LIBRARIES) below
# with the one row of its own.  A new library is a row of LATER_LIBRARIES further down.
MORE_LIBRARIES = {
    # the token-and-duration (TDT) transducer loss on materialised logits
    "tdt": Library("rnnt_tdt.h", ("rnnt_tdt_kernels.hip", "rnnt_tdt_entrypoint.hip"), (), "rnnt_tdt.map"),
}
ALL_LIBRARIES = {
    **LIBRARIES,
    **MORE_LIBRARIES,
    # batched greedy decoding of the TDT transducer: its own step and update kernels on the greedy decoder's prepare path and
    # per-hypothesis joint; the base kernel objects and its own entry points, as "bias"
    "tdtgreedy": Library("rnnt_tdt_greedy.h", ("tdt_greedy_kernels.hip", "rnnt_tdt_greedy_entrypoint.hip"), _BASE_KERNELS,
                         "rnnt_tdt_greedy.map"),
}
# Later rows.  tests/test_abi_tdt_greedy.py pins list(ALL_LIBRARIES) too, so the three tables above are frozen as they stand; this one
# was open until a test pinned the merged table's length (see NEXT_LIBRARIES below, where a new library is a row now).
LATER_LIBRARIES = {
    # greedy decoding of the TDT transducer over a stream of chunks per slot: its own feed and update kernels on the greedy
    # stream's projection and on the step kernel of "tdtgreedy", whose kernel object it links beside the base kernels'
    "tdtstream": Library("rnnt_tdt_stream.h", ("tdt_stream_kernels.hip", "rnnt_tdt_stream_entrypoint.hip"),
                         _BASE_KERNELS + ("tdt_greedy_kernels.hip",), "rnnt_tdt_stream.map"),
    # forced alignment on the TDT lattice: its own cell pass, sweep and back-trace; it borrows nothing
    "tdtalign": Library("rnnt_tdt_align.h", ("rnnt_tdtalign_kernels.hip", "rnnt_tdtalign_entrypoint.hip"), (), "rnnt_tdtalign.map"),
    # batched beam search of the TDT transducer: its own step, select, begin and results kernels on the greedy decoder's prepare
    # path and per-hypothesis joint; the base kernel objects and its own entry points, as "bias" (nothing of
    # tdt_greedy_kernels.hip is linked)
    "tdtbeam": Library("rnnt_tdt_beam.h", ("tdt_beam_kernels.hip", "rnnt_tdt_beam_entrypoint.hip"), _BASE_KERNELS, "rnnt_tdtbeam.map"),
    # the fused TDT joint: its own kernels and the lattice sweeps of the TDT loss, unchanged
    "tdtjoint": Library("rnnt_tdt_joint.h", ("rnnt_tdt_joint_kernels.hip", "rnnt_tdt_joint_entrypoint.hip"),
                        ("rnnt_tdt_kernels.hip",), "rnnt_tdt_joint.map"),
    # beam search of the TDT transducer over a stream of chunks per slot: its own begin, feed, step, select and results kernels (step
    # and select compiled from the text "tdtbeam" compiles: tdt_beam_step_body.h, tdt_beam_select_body.h) on the greedy stream's
    # projection; the base kernel objects and its own entry points, as "bias" (no object of "tdtbeam" is linked)
    "tdtbeamstream": Library("rnnt_tdt_beam_stream.h", ("tdt_nbest_stream_kernels.hip", "rnnt_tdt_nbest_stream_entrypoint.hip"),
                             _BASE_KERNELS, "rnnt_tdtbeamstream.map"),
}
EVERY_LIBRARY = {**ALL_LIBRARIES, **LATER_LIBRARIES}
# tests/test_abi_tdt_beam_stream.py pins len(EVERY_LIBRARY) to 16, so LATER_LIBRARIES and EVERY_LIBRARY are frozen as well.  The rows
# added since stand here, and BUILT_LIBRARIES is what the build and the binding work over.  No test pins the length of this table.
NEXT_LIBRARIES = {
    # batched beam search with several symbols per frame (time-synchronous, on the standard lattice): its own select, begin and
    # results kernels and the beam search's step body at a flag value of its own; the base kernel objects and its own entry
    # points, as "tdtbeam"
    "multibeam": Library("rnnt_beam_multi.h", ("multibeam_kernels.hip", "rnnt_multibeam_entrypoint.hip"), _BASE_KERNELS,
                         "rnnt_multibeam.map"),
    # "multibeam" over a stream of chunks per slot: its own begin, feed, step, select and results kernels (step and select compiled
    # from the text "multibeam" compiles: beam_step_body.h at the same flag value, multibeam_select_body.h) on the greedy stream's
    # projection; the base kernel objects and its own entry points (no object of "multibeam" is linked)
    "multibeamstream": Library("rnnt_beam_multi_stream.h", ("tsd_stream_kernels.hip", "rnnt_tsd_stream_entrypoint.hip"), _BASE_KERNELS,
                               "rnnt_tsdstream.map"),
    # the CTC loss and the greedy CTC decoder of the auxiliary head (hybrid transducer + CTC training): its own kernels, entry
    # points and workspace; it borrows nothing
    "ctc": Library("rnnt_ctc.h", ("rnnt_ctc_kernels.hip", "rnnt_ctc_entrypoint.hip"), (), "rnnt_ctc.map"),
}
BUILT_LIBRARIES = {**EVERY_LIBRARY, **NEXT_LIBRARIES}


def lib_path(name: str) -> str:
    return os.path.join(LIB_DIR, "libwarprnnt.so" if name == "base" else f"libwarprnnt_{name}.so")


LIB_PATH = lib_path("base")
BIAS_LIB_PATH = lib_path("bias")
MOD_LIB_PATH = lib_path("mod")
MODALIGN_LIB_PATH = lib_path("modalign")
PRUNED_LIB_PATH = lib_path("pruned")
SIMPLE_LIB_PATH = lib_path("simple")
PRUNEDJOINT_LIB_PATH = lib_path("prunedjoint")
PRUNERANGES_LIB_PATH = lib_path("pruneranges")
LM_LIB_PATH = lib_path("lm")
TDT_LIB_PATH = lib_path("tdt")
TDTGREEDY_LIB_PATH = lib_path("tdtgreedy")
TDTSTREAM_LIB_PATH = lib_path("tdtstream")
TDTALIGN_LIB_PATH = lib_path("tdtalign")
TDTBEAM_LIB_PATH = lib_path("tdtbeam")
TDTJOINT_LIB_PATH = lib_path("tdtjoint")
TDTBEAMSTREAM_LIB_PATH = lib_path("tdtbeamstream")
MULTIBEAM_LIB_PATH = lib_path("multibeam")
MULTIBEAMSTREAM_LIB_PATH = lib_path("multibeamstream")
CTC_LIB_PATH = lib_path("ctc")
# -fvisibility=hidden: the library exports exactly the entry points include/rnnt.h marks RNNT_API (tests/test_abi.py)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-inline-asm"]
# per-source extras.  -fno-slp-vectorize: no packed-f32 instructions (v_pk_fma_f32 ...) from the compiler -- in the linear sweeps
# they cost more register moves than they save (rnnt_lin_kernels.hip lin_alpha_step); in the MFMA kernels a packed-f32
# instruction does not overlap with the matrix pipe (scripts/probes/probe_pk.hip; fused step -0.6 %, config 5 -1.2 %).  The
# HBM-bound cell kernels of rnnt_kernels.hip keep the vectoriser (the op at config 5's shape: 16.4 against 17.0 ms).
_NO_SLP = ["-fno-slp-vectorize"]
EXTRA_FLAGS = {"rnnt_lin_kernels.hip": _NO_SLP, "joint_kernels.hip": _NO_SLP, "joint_f16_kernels.hip": _NO_SLP, "dense_kernels.hip": _NO_SLP,
               "greedy_kernels.hip": _NO_SLP, "tdt_greedy_kernels.hip": _NO_SLP, "tdt_stream_kernels.hip": _NO_SLP, "beam_kernels.hip": _NO_SLP, "beam_bias_kernels.hip": _NO_SLP,
               "beam_lm_kernels.hip": _NO_SLP, "tdt_beam_kernels.hip": _NO_SLP, "tdt_nbest_stream_kernels.hip": _NO_SLP,
               "multibeam_kernels.hip": _NO_SLP, "tsd_stream_kernels.hip": _NO_SLP,
               "prednet_kernels.hip": _NO_SLP, "encoder_kernels.hip": _NO_SLP, "lstm_train_kernels.hip": _NO_SLP,
               "rnnt_pruned_joint_kernels.hip": _NO_SLP, "rnnt_tdt_joint_kernels.hip": _NO_SLP}


def _deps():
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".map"))]
    return files + [os.path.join(os.path.dirname(_HERE), "include", lib.header) for lib in BUILT_LIBRARIES.values()]


def needs_build() -> bool:
    libs = [lib_path(name) for name in BUILT_LIBRARIES]
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    return any(os.path.getmtime(f) > t for f in _deps())


def _compile_one(args):
    hipcc, src, obj, verbose = args
    cmd = [hipcc] + [f for f in HIPCC_FLAGS if f != "-shared"] + EXTRA_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return obj


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every source of BUILT_LIBRARIES once (one hipcc per source, in parallel) and link each library from the
    objects its entry names, the extensions first and libwarprnnt.so last (needs_build() goes by the oldest of them).  Returns the path of
    libwarprnnt.so."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libwarprnnt.so (ROCm toolchain required)")
    os.makedirs(LIB_DIR, exist_ok=True)
    tag = f".tmp{os.getpid()}"  # several ranks may arrive here at once
    sources = list(dict.fromkeys(s for lib in BUILT_LIBRARIES.values() for s in lib.sources))
    jobs = [(hipcc, os.path.join(CSRC, s), os.path.join(LIB_DIR, s[:-4] + tag + ".o"), verbose) for s in sources]
    try:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
            obj = dict(zip(sources, ex.map(_compile_one, jobs)))
        for name in [n for n in BUILT_LIBRARIES if n != "base"] + ["base"]:
            lib = BUILT_LIBRARIES[name]
            extra = ["-Wl,--version-script=" + os.path.join(CSRC, lib.version_script)] if lib.version_script else []
            tmp = lib_path(name) + tag
            cmd = [hipcc] + HIPCC_FLAGS + extra + [obj[s] for s in lib.borrowed + lib.sources] + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(tmp, lib_path(name))
    finally:
        for _, _, o, _ in jobs:
            if os.path.exists(o):
                os.remove(o)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
