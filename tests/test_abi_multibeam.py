"""CPU tests of the C-ABI boundary of libwarprnnt_multibeam.so, a row of build.NEXT_LIBRARIES: the checks
tests/test_abi_tdt_beam.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_beam_multi.h on fake
pointers.  (tests/test_abi_tdt_beam_stream.py pins the length of build.EVERY_LIBRARY, so the row stands in the table after it;
that table is not pinned to a list or a length here: the next library is one more row of it.)"""
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
NAME = "multibeam"
EXPORTS = ["get_rnnt_multibeam_workspace_size", "compute_rnnt_multibeam_begin", "compute_rnnt_multibeam_step",
           "compute_rnnt_multibeam_results"]
INVALID = 2


def test_the_open_table_holds_the_library_and_the_older_tables_are_unchanged():
    assert NAME in build_mod.NEXT_LIBRARIES and NAME in _lib._NEXT_SIGNATURES
    assert list(build_mod.NEXT_LIBRARIES) == list(_lib._NEXT_SIGNATURES) == list(_lib._NEXT_PATHS)
    assert list(build_mod.NEXT_LIBRARIES)[0] == NAME
    # the older tables are what they were
    assert list(build_mod.LIBRARIES) == ["base", "bias", "mod", "modalign", "pruned", "simple", "prunedjoint", "pruneranges", "lm"]
    assert list(build_mod.ALL_LIBRARIES) == list(build_mod.LIBRARIES) + ["tdt", "tdtgreedy"]
    assert list(build_mod.LATER_LIBRARIES) == ["tdtstream", "tdtalign", "tdtbeam", "tdtjoint", "tdtbeamstream"]
    assert list(build_mod.EVERY_LIBRARY) == list(build_mod.ALL_LIBRARIES) + list(build_mod.LATER_LIBRARIES) == list(_lib._PATHS)
    assert not set(build_mod.EVERY_LIBRARY) & set(build_mod.NEXT_LIBRARIES)
    assert list(build_mod.BUILT_LIBRARIES) == list(build_mod.EVERY_LIBRARY) + list(build_mod.NEXT_LIBRARIES) == list(_lib._BUILT_SIGNATURES)
    lib = build_mod.NEXT_LIBRARIES[NAME]
    assert type(lib) is type(build_mod.LIBRARIES["bias"])
    assert lib.borrowed == build_mod._BASE_KERNELS  # the base kernels alone, as "tdtbeam"
    assert lib.sources == ("multibeam_kernels.hip", "rnnt_multibeam_entrypoint.hip")
    assert lib.header == "rnnt_beam_multi.h" and lib.version_script == "rnnt_multibeam.map"
    assert build_mod.EXTRA_FLAGS["multibeam_kernels.hip"] == build_mod.EXTRA_FLAGS["beam_kernels.hip"]  # the beam search's flags
    assert build_mod.MULTIBEAM_LIB_PATH == build_mod.lib_path(NAME) == _lib._NEXT_PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_multibeam.so"))
    deps = build_mod._deps()
    assert os.path.join(ROOT, "include", "rnnt_beam_multi.h") in deps and os.path.join(build_mod.CSRC, "beam_step_body.h") in deps
    for name, other in build_mod.BUILT_LIBRARIES.items():  # the sixteen other libraries are built from what they were built from
        if name != NAME:
            assert not any("multibeam" in s for s in other.sources + other.borrowed), name
    text = open(os.path.join(build_mod.CSRC, "multibeam_kernels.hip")).read()
    assert "#define BEAM_STEP_BIAS 3" in text and '#include "beam_step_body.h"' in text  # the shared step body, its own flag value
    assert '.hip"' not in text  # no unit includes a unit


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.NEXT_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._NEXT_SIGNATURES[NAME]) == sorted(EXPORTS)
    for symbol in declared:  # as many parameters in the header as the binding passes
        params = re.search(symbol + r"\s*\(([^;{]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == len(_lib._NEXT_SIGNATURES[NAME][symbol]), symbol
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.MULTIBEAM_LIB_PATH)
    lib = _lib.load_multibeam()
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
    for kernel in ("multibeam_begin_kernel", "multibeam_step_kernel", "multibeam_select_kernel", "multibeam_results_kernel"):
        assert any(kernel in n for n in names), kernel
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._NEXT_PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_beam_multi.h"):
        _lib.load_multibeam()


def test_workspace_size():
    """Monotone in every argument, in 256-byte multiples, at least what its arrays need; every limit and one past it."""
    pkg.build()
    lib = _lib.load_multibeam()
    size = _lib.multibeam_workspace_bytes
    for T, B, K, E, N, J, V, dt in ((300, 16, 4, 2, 600, 640, 4096, 1), (1, 1, 1, 1, 1, 64, 2, 0), (9, 3, 4, 3, 27, 64, 27, 0),
                                    (9, 3, 16, 8, 72, 128, 126, 1), (7, 2, 8, 2, 5, 128, 1030, 1), (5, 32, 16, 1, 5, 64, 12, 0)):
        n = size(T, B, K, E, N, J, V, dt)
        assert n % 256 == 0
        NS = ((V + 31) // 32 + 3) // 4
        R = B * 2 * K
        need = 2 * R * N * 4 + 2 * B * T * J * 4 + NS * R * (2 + 2 * K) * 4 + R * 24 + R * 4  # rows, tables, lists, slots, blank
        assert n >= need
        assert n >= _lib.beam_workspace_bytes(T, B, K, J, V, dt) - 2 * B * K * T * 4  # the beam search's but for its token rows
        assert size(T, B, K, E + 1 if E < 8 else E, N, J, V, dt) == n  # the rounds cost no memory
        assert size(T + 1, B, K, E, N, J, V, dt) > n and size(T, B, K, E, N + 64, J, V, dt) > n
        if R + 2 * K <= 1024:
            assert size(T, B + 1, K, E, N, J, V, dt) > n
        if K < 16 and B * 32 <= 1024:
            assert size(T, B, K + 1, E, N, J, V, dt) >= n and size(T, B, 16, E, N, J, V, dt) > n
        if J < 640:
            assert size(T, B, K, E, N, J + (128 if dt else 64), V, dt) > n
        assert size(T, B, K, E, N, J, V + (128 if dt else 32), dt) > n and size(T, B, K, E, N, J, V + 1, dt) >= n
    n = ctypes.c_size_t(0)
    ok = (9, 4, 4, 2, 18, 64, 27, 0)
    assert lib.get_rnnt_multibeam_workspace_size(*ok, ctypes.byref(n)) == 0 and n.value > 0
    names = ("maxT", "minibatch", "beam", "symbols_per_frame", "max_hyp_len", "joint_size", "alphabet_size", "joint_dtype")
    bad = dict(maxT=(0, -1), minibatch=(0, -1, 129), beam=(0, 17, -1), symbols_per_frame=(0, 9, -1), max_hyp_len=(0, -3),
               joint_size=(0, 63, -64), alphabet_size=(0, -5), joint_dtype=(2, -1, 1 | 256))
    for i, name in enumerate(names):
        for value in bad[name]:
            args = list(ok)
            args[i] = value
            assert lib.get_rnnt_multibeam_workspace_size(*args, ctypes.byref(n)) == INVALID, (name, value)
    assert lib.get_rnnt_multibeam_workspace_size(9, 128, 4, 2, 18, 64, 27, 0, ctypes.byref(n)) == 0  # 1024 rows: the last that fit
    assert lib.get_rnnt_multibeam_workspace_size(9, 33, 16, 2, 18, 64, 27, 0, ctypes.byref(n)) == INVALID  # 1056 rows
    assert lib.get_rnnt_multibeam_workspace_size(1 << 15, 1 << 10, 1, 2, 18, 64, 27, 0, ctypes.byref(n)) == INVALID  # rows, and 2^31
    assert lib.get_rnnt_multibeam_workspace_size(1 << 19, 64, 1, 1, 4, 64, 27, 0, ctypes.byref(n)) == INVALID  # B maxT J = 2^31
    assert lib.get_rnnt_multibeam_workspace_size(9, 32, 16, 2, 1 << 20, 64, 27, 0, ctypes.byref(n)) == INVALID  # token rows = 2^31
    assert lib.get_rnnt_multibeam_workspace_size(*ok, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_multibeam()
    fake, misaligned = ctypes.c_void_p(256), ctypes.c_void_p(260)
    o = _lib.make_options(0, 0, 10, 1)

    def begin(enc=fake, fl=fake, W2=fake, b2=fake, J=64, V=27, B=4, K=4, E=2, N=20, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_begin(enc, fl, W2, b2, J, V, B, K, E, N, dt, ws, opts)

    def step(pp=fake, parents=fake, emitted=fake, J=64, V=27, B=4, K=4, E=2, N=20, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_step(pp, parents, emitted, J, V, B, K, E, N, dt, ws, opts)

    def results(hyps=fake, lens=fake, scores=fake, J=64, V=27, B=4, K=4, E=2, N=20, dt=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_results(hyps, lens, scores, J, V, B, K, E, N, dt, ws, opts)

    calls = (begin, step, results)
    for call, names in ((begin, ("enc", "fl", "W2", "b2", "ws")), (step, ("pp", "parents", "emitted", "ws")),
                        (results, ("hyps", "lens", "scores", "ws"))):
        for name in names:
            assert call(**{name: None}) == INVALID, (call, name)
    for call in calls:
        assert call(ws=misaligned) == INVALID  # the workspace: 256-byte aligned
        for K in (0, 17, -1):
            assert call(K=K) == INVALID, K
        for E in (0, 9, -1):  # symbols_per_frame outside [1, 8]
            assert call(E=E) == INVALID, E
        for N in (0, -1):  # max_hyp_len < 1
            assert call(N=N) == INVALID, N
        assert call(B=129, K=4) == INVALID and call(B=33, K=16) == INVALID  # minibatch * 2 * beam > 1024
        for dt in (2, -1, 1 | 256):  # no flag bits
            assert call(dt=dt) == INVALID, dt
        assert call(J=0) == INVALID and call(J=63) == INVALID and call(B=0) == INVALID and call(B=-1) == INVALID
        assert call(V=0) == INVALID and call(V=-5) == INVALID
        assert call(V=8200, dt=1, J=128) == INVALID  # beyond what the beam search takes
        assert call(opts=_lib.make_options(0, 27, 10, 1)) == INVALID  # the blank outside the alphabet
        assert call(opts=_lib.make_options(0, -1, 10, 1)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 0, 1)) == INVALID and call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 1, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 1)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
        assert call(opts=_lib.make_options(0, 0, 1 << 19, 1), B=64) == INVALID  # minibatch * maxT * joint_size = 2^31
        assert call(N=1 << 24, B=8) == INVALID  # the token rows beyond 2^31 words
