"""Build driver for libwarprnnt.so (the MI355X counterpart of the reference's
scripts/build_rnnt.sh:1-13, which runs cmake+make on warp-transducer and installs the binding).

hipcc cross-compiles for gfx950 without a GPU.  The library is built IN-TREE
(`rnnt-speech-recognition_amd/lib/libwarprnnt.so`) so that it travels with the source snapshot."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt.so")
# the extension library of include/rnnt_bias.h: the kernel objects of SOURCES (the host side of the beam search rests on them),
# the biased kernels and rnnt_bias_entrypoint.hip in place of rnnt_entrypoint.hip; rnnt_bias.map: it exports the four biased
# steps alone.  libwarprnnt.so is built from SOURCES as it always was and holds nothing of the extension.
BIAS_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_bias.so")
BIAS_SOURCES = ["beam_bias_kernels.hip", "rnnt_bias_entrypoint.hip"]
BIAS_MAP = os.path.join(CSRC, "rnnt_bias.map")
# the extension library of include/rnnt_modified.h: the loss op on the modified (one symbol per frame) lattice.  It is self-contained
# (its own kernels, entry points and workspace); rnnt_mod.map: it exports its two entry points alone.
MOD_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_mod.so")
MOD_SOURCES = ["rnnt_mod_kernels.hip", "rnnt_mod_entrypoint.hip"]
MOD_MAP = os.path.join(CSRC, "rnnt_mod.map")
# the extension library of include/rnnt_modified_align.h: forced alignment on the modified lattice.  Self-contained as well;
# rnnt_modalign.map: it exports its four entry points alone.
MODALIGN_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_modalign.so")
MODALIGN_SOURCES = ["rnnt_modalign_kernels.hip", "rnnt_modalign_entrypoint.hip"]
MODALIGN_MAP = os.path.join(CSRC, "rnnt_modalign.map")
# the extension library of include/rnnt_pruned.h: the loss op on a band of S symbols per frame.  Self-contained as well;
# rnnt_pruned.map: it exports its two entry points alone.
PRUNED_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_pruned.so")
PRUNED_SOURCES = ["rnnt_pruned_kernels.hip", "rnnt_pruned_entrypoint.hip"]
PRUNED_MAP = os.path.join(CSRC, "rnnt_pruned.map")
# the extension library of include/rnnt_simple.h: the loss op of an additive joiner (am + lm), the first pass of the pruned loss.
# Self-contained as well; rnnt_simple.map: it exports its two entry points alone.
SIMPLE_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_simple.so")
SIMPLE_SOURCES = ["rnnt_simple_kernels.hip", "rnnt_simple_entrypoint.hip"]
SIMPLE_MAP = os.path.join(CSRC, "rnnt_simple.map")
# the extension library of include/rnnt_pruned_joint.h: the fused joint on the pruned band.  Its own kernels and entry points, and
# the object of rnnt_pruned_kernels.hip (the lattice sweeps, unchanged); rnnt_pruned_joint.map: it exports its two entry points alone.
PRUNEDJOINT_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_prunedjoint.so")
PRUNEDJOINT_SOURCES = ["rnnt_pruned_joint_kernels.hip", "rnnt_pruned_joint_entrypoint.hip"]
PRUNEDJOINT_MAP = os.path.join(CSRC, "rnnt_pruned_joint.map")
# the extension library of include/rnnt_prune_ranges.h: the band positions between the two passes of the pruned loss, with a defined
# order of additions.  Self-contained as well (no workspace); rnnt_prune_ranges.map: it exports its one entry point alone.
PRUNERANGES_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_pruneranges.so")
PRUNERANGES_SOURCES = ["rnnt_prune_ranges_kernels.hip", "rnnt_prune_ranges_entrypoint.hip"]
PRUNERANGES_MAP = os.path.join(CSRC, "rnnt_prune_ranges.map")
# the extension library of include/rnnt_lm.h: n-gram LM shallow fusion in the beam searches.  Built as libwarprnnt_bias.so is: the
# kernel objects of SOURCES, the LM kernels and rnnt_lm_entrypoint.hip in place of rnnt_entrypoint.hip; rnnt_lm.map: it exports the
# four LM steps alone.
LM_LIB_PATH = os.path.join(LIB_DIR, "libwarprnnt_lm.so")
LM_SOURCES = ["beam_lm_kernels.hip", "rnnt_lm_entrypoint.hip"]
LM_MAP = os.path.join(CSRC, "rnnt_lm.map")
SOURCES = ["rnnt_kernels.hip", "rnnt_lin_kernels.hip", "joint_kernels.hip", "joint_f16_kernels.hip", "dense_kernels.hip", "greedy_kernels.hip",
           "beam_kernels.hip", "prednet_kernels.hip", "encoder_kernels.hip", "lstm_train_kernels.hip", "frontend_kernels.hip",
           "align_kernels.hip", "rnnt_entrypoint.hip"]
# -fvisibility=hidden: the library exports exactly the entry points include/rnnt.h marks RNNT_API (tests/test_abi.py)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-inline-asm"]
# per-source extras.  -fno-slp-vectorize: no packed-f32 instructions (v_pk_fma_f32 ...) from the compiler -- in the linear sweeps
# they cost more register moves than they save (rnnt_lin_kernels.hip lin_alpha_step); in the MFMA kernels a packed-f32
# instruction does not overlap with the matrix pipe (scripts/probes/probe_pk.hip; fused step -0.6 %, config 5 -1.2 %).  The
# HBM-bound cell kernels of rnnt_kernels.hip keep the vectoriser (the op at config 5's shape: 16.4 against 17.0 ms).
_NO_SLP = ["-fno-slp-vectorize"]
EXTRA_FLAGS = {"rnnt_lin_kernels.hip": _NO_SLP, "joint_kernels.hip": _NO_SLP, "joint_f16_kernels.hip": _NO_SLP, "dense_kernels.hip": _NO_SLP,
               "greedy_kernels.hip": _NO_SLP, "beam_kernels.hip": _NO_SLP, "beam_bias_kernels.hip": _NO_SLP,
               "beam_lm_kernels.hip": _NO_SLP,
               "prednet_kernels.hip": _NO_SLP, "encoder_kernels.hip": _NO_SLP, "lstm_train_kernels.hip": _NO_SLP,
               "rnnt_pruned_joint_kernels.hip": _NO_SLP}


def _deps():
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".map"))]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_bias.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_modified.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_modified_align.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_pruned.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_simple.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_pruned_joint.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_prune_ranges.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "rnnt_lm.h"))
    return files


def needs_build() -> bool:
    libs = (LIB_PATH, BIAS_LIB_PATH, MOD_LIB_PATH, MODALIGN_LIB_PATH, PRUNED_LIB_PATH, SIMPLE_LIB_PATH, PRUNEDJOINT_LIB_PATH,
            PRUNERANGES_LIB_PATH, LM_LIB_PATH)
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
    """Compile every HIP source (one hipcc per source, in parallel) and link lib/libwarprnnt.so and, from the same kernel
    objects, lib/libwarprnnt_bias.so, lib/libwarprnnt_mod.so from MOD_SOURCES, lib/libwarprnnt_modalign.so from MODALIGN_SOURCES,
    lib/libwarprnnt_pruned.so from PRUNED_SOURCES, lib/libwarprnnt_simple.so from SIMPLE_SOURCES, lib/libwarprnnt_prunedjoint.so
    from PRUNEDJOINT_SOURCES and the kernel object of PRUNED_SOURCES and lib/libwarprnnt_pruneranges.so from PRUNERANGES_SOURCES, and lib/libwarprnnt_lm.so
    from the kernel objects of SOURCES and LM_SOURCES; returns the path of the first."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libwarprnnt.so (ROCm toolchain required)")
    os.makedirs(LIB_DIR, exist_ok=True)
    tag = f".tmp{os.getpid()}"  # several ranks may arrive here at once
    jobs = [(hipcc, os.path.join(CSRC, s), os.path.join(LIB_DIR, s[:-4] + tag + ".o"), verbose) for s in SOURCES + BIAS_SOURCES + MOD_SOURCES + MODALIGN_SOURCES + PRUNED_SOURCES + SIMPLE_SOURCES + PRUNEDJOINT_SOURCES + PRUNERANGES_SOURCES + LM_SOURCES]
    objs = []
    try:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
            objs = list(ex.map(_compile_one, jobs))
        n = len(SOURCES)  # (SOURCES ends with rnnt_entrypoint.hip)
        m = n + len(BIAS_SOURCES)
        k = m + len(MOD_SOURCES)
        q = k + len(MODALIGN_SOURCES)
        r = q + len(PRUNED_SOURCES)
        v = r + len(SIMPLE_SOURCES)
        x = v + len(PRUNEDJOINT_SOURCES)
        z = x + len(PRUNERANGES_SOURCES)
        links = ((BIAS_LIB_PATH, objs[: n - 1] + objs[n:m], ["-Wl,--version-script=" + BIAS_MAP]),
                 (MOD_LIB_PATH, objs[m:k], ["-Wl,--version-script=" + MOD_MAP]),
                 (MODALIGN_LIB_PATH, objs[k:q], ["-Wl,--version-script=" + MODALIGN_MAP]),
                 (PRUNED_LIB_PATH, objs[q:r], ["-Wl,--version-script=" + PRUNED_MAP]),
                 (SIMPLE_LIB_PATH, objs[r:v], ["-Wl,--version-script=" + SIMPLE_MAP]),
                 (PRUNEDJOINT_LIB_PATH, objs[q:q + 1] + objs[v:x], ["-Wl,--version-script=" + PRUNEDJOINT_MAP]),
                 (PRUNERANGES_LIB_PATH, objs[x:z], ["-Wl,--version-script=" + PRUNERANGES_MAP]),
                 (LM_LIB_PATH, objs[: n - 1] + objs[z:], ["-Wl,--version-script=" + LM_MAP]), (LIB_PATH, objs[:n], []))
        for path, members, extra in links:
            tmp = path + tag
            cmd = [hipcc] + HIPCC_FLAGS + extra + members + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            os.replace(tmp, path)
    finally:
        for _, _, obj, _ in jobs:
            if os.path.exists(obj):
                os.remove(obj)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
