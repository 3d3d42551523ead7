"""CPU tests of the C-ABI boundary of libwarprnnt_tdtbeam.so, a row of the open table build.LATER_LIBRARIES: the checks
tests/test_abi_tdt_align.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_tdt_beam.h on fake
pointers.  The open table is not pinned to a list here: the next library is one more row of it."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib

build_mod = importlib.import_module("rnnt_speech_recognition_amd.build")  # (the package's `build` attribute is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tdtbeam"
EXPORTS = ["get_rnnt_tdt_beam_workspace_size", "compute_rnnt_tdt_beam_begin", "compute_rnnt_tdt_beam_step", "compute_rnnt_tdt_beam_results"]
INVALID = 2


def test_the_open_table_holds_the_library_and_the_older_tables_are_unchanged():
    assert NAME in build_mod.LATER_LIBRARIES and NAME in _lib._LATER_SIGNATURES
    assert list(build_mod.LATER_LIBRARIES) == list(_lib._LATER_SIGNATURES)
    assert list(build_mod.LATER_LIBRARIES)[:2] == ["tdtstream", "tdtalign"]  # the rows before it are where they were
    assert list(build_mod.LATER_LIBRARIES).index(NAME) > 1
    # the three older tables are what they were
    assert list(build_mod.LIBRARIES) == ["base", "bias", "mod", "modalign", "pruned", "simple", "prunedjoint", "pruneranges", "lm"]
    assert list(build_mod.MORE_LIBRARIES) == ["tdt"]
    assert list(build_mod.ALL_LIBRARIES) == list(build_mod.LIBRARIES) + ["tdt", "tdtgreedy"] == list(_lib._ALL_SIGNATURES)
    assert list(_lib.SIGNATURES) == list(build_mod.LIBRARIES) and list(_lib.MORE_SIGNATURES) == ["tdt"]
    every = list(build_mod.ALL_LIBRARIES) + list(build_mod.LATER_LIBRARIES)
    assert list(build_mod.EVERY_LIBRARY) == every == list(_lib._EVERY_SIGNATURE) == list(_lib._PATHS)
    assert not set(build_mod.ALL_LIBRARIES) & set(build_mod.LATER_LIBRARIES)
    lib = build_mod.LATER_LIBRARIES[NAME]
    assert type(lib) is type(build_mod.LIBRARIES["bias"])
    assert lib.borrowed == build_mod._BASE_KERNELS  # the base kernels alone: nothing of tdt_greedy_kernels.hip is linked
    assert lib.sources == ("tdt_beam_kernels.hip", "rnnt_tdt_beam_entrypoint.hip")
    assert lib.header == "rnnt_tdt_beam.h" and lib.version_script == "rnnt_tdtbeam.map"
    assert build_mod.EXTRA_FLAGS["tdt_beam_kernels.hip"] == build_mod.EXTRA_FLAGS["beam_kernels.hip"]  # the beam search's flags
    assert build_mod.TDTBEAM_LIB_PATH == build_mod.lib_path(NAME) == _lib._PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_tdtbeam.so"))
    deps = build_mod._deps()
    assert os.path.join(ROOT, "include", "rnnt_tdt_beam.h") in deps and os.path.join(build_mod.CSRC, "tdt_beam_common.h") in deps
    for name, other in build_mod.EVERY_LIBRARY.items():  # the thirteen other libraries are built from what they were built from
        if name != NAME:
            assert not any("tdt_beam" in s or "tdtbeam" in s for s in other.sources + other.borrowed), name
    assert build_mod.EVERY_LIBRARY["tdtalign"].sources == ("rnnt_tdtalign_kernels.hip", "rnnt_tdtalign_entrypoint.hip")
    assert build_mod.EVERY_LIBRARY["tdtstream"].borrowed == build_mod._BASE_KERNELS + ("tdt_greedy_kernels.hip",)


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.LATER_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._LATER_SIGNATURES[NAME]) == sorted(EXPORTS)
    for symbol in declared:  # as many parameters in the header as the binding passes
        params = re.search(symbol + r"\s*\(([^;{]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == len(_lib._LATER_SIGNATURES[NAME][symbol]), symbol
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.TDTBEAM_LIB_PATH)
    lib = _lib.load_tdtbeam()
    for symbol in declared:
        assert ctypes.cast(getattr(lib, symbol), ctypes.c_void_p).value


def test_dynamic_symbol_table_is_the_abi_and_nothing_else():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    assert os.path.exists(nm), "neither binutils nm nor llvm-nm found: the export table cannot be checked"
    pkg.build()
    out = subprocess.run([nm, "-D", "--defined-only", build_mod.lib_path(NAME)], check=True, capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    plain = sorted(n for n in names if not n.startswith("_Z") and not n.startswith("__hip_cuid_"))
    assert plain == sorted(EXPORTS)
    for kernel in ("tdt_beam_begin_kernel", "tdt_beam_step_kernel", "tdt_beam_select_kernel", "tdt_beam_select_timed_kernel",
                   "tdt_beam_results_kernel", "tdt_beam_results_timed_kernel"):
        assert any(kernel in n for n in names), kernel
    assert not any("tdt_greedy" in n for n in names)  # nothing of the greedy TDT decoder's kernels is in it
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_tdt_beam.h"):
        _lib.load_tdtbeam()


def test_workspace_size():
    """Monotone in every argument, in 256-byte multiples, the beam search's workspace at alphabet_size = V + D and then some; timed
    adds the {frame, duration} rows; every limit and one past it."""
    pkg.build()
    lib = _lib.load_tdtbeam()
    size = _lib.tdt_beam_workspace_bytes
    for T, B, K, J, V, D, dt in ((300, 16, 4, 640, 1024, 5, 1), (1, 1, 1, 64, 2, 1, 0), (9, 3, 4, 64, 27, 5, 0), (9, 3, 16, 128, 126, 5, 1),
                                 (7, 2, 8, 128, 1030, 5, 1), (7, 2, 8, 128, 125, 8, 1)):
        n = size(T, B, K, J, V, D, dt)
        assert n % 256 == 0
        base = _lib.beam_workspace_bytes(T, B, K, J, V + D, dt)
        NS = ((V + D + 31) // 32 + 3) // 4
        extra = n - base
        assert 2 * NS * B * K * 4 + B * K * 8 * 4 + 32 <= extra <= 2 * NS * B * K * 4 + B * K * 8 * 4 + 32 + 4 * 256
        nt = size(T, B, K, J, V, D, dt, True)
        assert nt % 256 == 0 and nt - n >= 2 * B * K * T * 8  # the pair rows, double-buffered
        assert size(T + 1, B, K, J, V, D, dt) > n and size(T, B + 1, K, J, V, D, dt) > n
        if K < 16:
            assert size(T, B, K + 1, J, V, D, dt) >= n and size(T, B, 16, J, V, D, dt) > n  # (256-byte regions: one slot may fit)
        if J < 640:
            assert size(T, B, K, J + (128 if dt else 64), V, D, dt) > n
        assert size(T, B, K, J, V + (128 if dt else 32), D, dt) > n and size(T, B, K, J, V + 1, D, dt) >= n
        if D < 8:
            assert size(T, B, K, J, V, D + 1, dt) >= n
    n = ctypes.c_size_t(0)
    bad = [(0, 4, 4, 64, 27, 5, 0, 0), (9, 0, 4, 64, 27, 5, 0, 0), (9, 4, 0, 64, 27, 5, 0, 0), (9, 4, 17, 64, 27, 5, 0, 0),
           (9, 4, 4, 0, 27, 5, 0, 0), (9, 4, 4, 64, 1, 5, 0, 0), (9, 4, 4, 64, 27, 0, 0, 0), (9, 4, 4, 64, 27, 9, 0, 0),
           (9, 4, 4, 64, 27, 5, 2, 0), (9, 4, 4, 64, 27, 5, -1, 0), (9, 4, 4, 63, 27, 5, 0, 0), (-1, 4, 4, 64, 27, 5, 0, 0),
           (1 << 15, 1 << 10, 4, 64, 27, 5, 0, 0)]  # minibatch * maxT * joint_size = 2^31
    for args in bad:
        assert lib.get_rnnt_tdt_beam_workspace_size(*args, ctypes.byref(n)) == INVALID, args
    assert lib.get_rnnt_tdt_beam_workspace_size(9, 4, 16, 64, 27, 8, 0, 1, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.get_rnnt_tdt_beam_workspace_size(9, 4, 4, 64, 27, 5, 0, 0, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_tdtbeam()
    fake, misaligned = ctypes.c_void_p(256), ctypes.c_void_p(260)
    o = _lib.make_options(0, 0, 10, 1)
    d5 = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def begin(enc=fake, fl=fake, W2=fake, b2=fake, J=64, V=27, dur=d5, D=5, B=4, K=4, dt=0, timed=0, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_beam_begin(enc, fl, W2, b2, J, V, dur, D, B, K, dt, timed, ws, opts)

    def step(pp=fake, parents=fake, emitted=fake, topl=None, tops=None, durl=None, lse=None, J=64, V=27, D=5, B=4, K=4, dt=0, timed=0,
             ws=fake, opts=o):
        return lib.compute_rnnt_tdt_beam_step(pp, parents, emitted, topl, tops, durl, lse, J, V, D, B, K, dt, timed, ws, opts)

    def results(hyps=fake, lens=fake, scores=fake, cursors=None, frames=None, durs=None, J=64, V=27, D=5, B=4, K=4, dt=0, timed=0, ws=fake,
                opts=o):
        return lib.compute_rnnt_tdt_beam_results(hyps, lens, scores, cursors, frames, durs, J, V, D, B, K, dt, timed, ws, opts)

    calls = (begin, step, results)
    for call, names in ((begin, ("enc", "fl", "W2", "b2", "dur", "ws")), (step, ("pp", "parents", "emitted", "ws")),
                        (results, ("hyps", "lens", "scores", "ws"))):
        for name in names:
            assert call(**{name: None}) == INVALID, (call, name)
    for call in calls:
        assert call(ws=misaligned) == INVALID  # the workspace: 256-byte aligned
        for K in (0, 17, -1):
            assert call(K=K) == INVALID, K
        for dt in (2, -1, 1 | 256):  # no flag bits
            assert call(dt=dt) == INVALID, dt
        assert call(J=0) == INVALID and call(J=63) == INVALID and call(B=0) == INVALID and call(B=-1) == INVALID
        assert call(V=1) == INVALID and call(V=0) == INVALID and call(V=-5) == INVALID
        assert call(D=0) == INVALID and call(D=9) == INVALID and call(D=-1) == INVALID
        assert call(V=8190, D=5, dt=1, J=128) == INVALID  # V + D beyond what the beam search takes
        assert call(opts=_lib.make_options(0, 27, 10, 1)) == INVALID  # the blank inside the duration head
        assert call(opts=_lib.make_options(0, -1, 10, 1)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 0, 1)) == INVALID and call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 1, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 1)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
        assert call(opts=_lib.make_options(0, 0, 1 << 15, 1), B=1 << 10) == INVALID  # minibatch * maxT * joint_size = 2^31
    # durations (begin alone reads them)
    for bad in ([0, 2, 1], [0, 1, 1], [-1, 0, 1], [0], [2, 3], [0, 1, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8]):
        arr = (ctypes.c_int * len(bad))(*bad)
        assert begin(dur=arr, D=len(bad)) == INVALID, bad
    # the timed outputs: both or neither, and only of a timed decode
    assert results(frames=fake, durs=None, timed=1) == INVALID and results(frames=None, durs=fake, timed=1) == INVALID
    assert results(frames=fake, durs=fake, timed=0) == INVALID
