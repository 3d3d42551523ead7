"""CPU tests of the C-ABI boundary of libwarprnnt_multibeamstream.so, a row of build.NEXT_LIBRARIES: the checks
tests/test_abi_multibeam.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_beam_multi_stream.h on
fake pointers.  (The open table is not pinned to a list or a length here: the next library is one more row of it.)"""
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
NAME = "multibeamstream"
EXPORTS = ["get_rnnt_multibeam_stream_workspace_size", "compute_rnnt_multibeam_stream_begin", "compute_rnnt_multibeam_stream_feed",
           "compute_rnnt_multibeam_stream_step", "compute_rnnt_multibeam_stream_results"]
SOURCES = ("tsd_stream_kernels.hip", "rnnt_tsd_stream_entrypoint.hip")
INVALID = 2


def test_the_open_table_holds_the_library_after_multibeam_whose_row_is_unchanged():
    assert NAME in build_mod.NEXT_LIBRARIES and NAME in _lib._NEXT_SIGNATURES
    names = list(build_mod.NEXT_LIBRARIES)
    assert names == list(_lib._NEXT_SIGNATURES) == list(_lib._NEXT_PATHS)
    assert names[0] == "multibeam" and names.index(NAME) == 1
    assert list(build_mod.BUILT_LIBRARIES) == list(build_mod.EVERY_LIBRARY) + names == list(_lib._BUILT_SIGNATURES)
    old = build_mod.NEXT_LIBRARIES["multibeam"]  # the offline search's row is what it was
    assert old.sources == ("multibeam_kernels.hip", "rnnt_multibeam_entrypoint.hip") and old.borrowed == build_mod._BASE_KERNELS
    assert old.header == "rnnt_beam_multi.h" and old.version_script == "rnnt_multibeam.map"
    assert sorted(_lib._NEXT_SIGNATURES["multibeam"]) == sorted(["get_rnnt_multibeam_workspace_size", "compute_rnnt_multibeam_begin",
                                                                 "compute_rnnt_multibeam_step", "compute_rnnt_multibeam_results"])
    lib = build_mod.NEXT_LIBRARIES[NAME]
    assert type(lib) is type(build_mod.LIBRARIES["bias"])
    assert lib.borrowed == build_mod._BASE_KERNELS  # the base kernels alone: no object of "multibeam" is linked
    assert lib.sources == SOURCES and not any("multibeam" in s for s in lib.sources + lib.borrowed)
    assert lib.header == "rnnt_beam_multi_stream.h" and lib.version_script == "rnnt_tsdstream.map"
    assert build_mod.EXTRA_FLAGS["tsd_stream_kernels.hip"] == build_mod.EXTRA_FLAGS["multibeam_kernels.hip"]  # the offline unit's flags
    assert build_mod.MULTIBEAMSTREAM_LIB_PATH == build_mod.lib_path(NAME) == _lib._NEXT_PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_multibeamstream.so"))
    deps = build_mod._deps()
    for h in ("beam_step_body.h", "multibeam_select_body.h", "multibeam_common.h"):
        assert os.path.join(build_mod.CSRC, h) in deps
    assert os.path.join(ROOT, "include", "rnnt_beam_multi_stream.h") in deps
    for name, other in build_mod.BUILT_LIBRARIES.items():  # no other library lists or borrows the new sources
        if name != NAME:
            assert not set(SOURCES) & set(other.sources + other.borrowed), name


def test_step_and_select_are_the_offline_text_not_a_copy():
    read = lambda f: open(os.path.join(build_mod.CSRC, f)).read()  # noqa: E731
    new, old = read("tsd_stream_kernels.hip"), read("multibeam_kernels.hip")
    for text in (new, old):
        assert "#define BEAM_STEP_BIAS 3" in text and '#include "beam_step_body.h"' in text
        assert '#include "multibeam_select_body.h"' in text and '#include "multibeam_common.h"' in text
        assert '.hip"' not in text  # no unit includes a unit
        assert "struct MultiBeamArgs" not in text and "s_lsrc" not in text  # the shared text lives in the headers alone
    assert "multibeam_select_body<false>" in new and "multibeam_select_body<true>" in new and "multibeam_select_body<false>" in old
    assert '.hip"' not in read("rnnt_tsd_stream_entrypoint.hip")
    assert "check_multibeam_stream" in read("rnnt_decode_host.h")  # the argument checks stand beside the other decoders'


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.NEXT_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._NEXT_SIGNATURES[NAME]) == sorted(EXPORTS)
    for symbol in declared:  # as many parameters in the header as the binding passes
        params = re.search(symbol + r"\s*\(([^;{]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == len(_lib._NEXT_SIGNATURES[NAME][symbol]), symbol
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.MULTIBEAMSTREAM_LIB_PATH)
    lib = _lib.load_multibeam_stream()
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
    for kernel in ("tsd_stream_begin_kernel", "tsd_stream_feed_kernel", "tsd_stream_step_kernel", "tsd_stream_select_kernel",
                   "tsd_stream_select_timed_kernel", "tsd_stream_results_kernel", "tsd_stream_results_timed_kernel"):
        assert any(kernel in n for n in names), kernel
    assert not any("multibeam_select_kernel" in n or "multibeam_step_kernel" in n for n in names)  # its own kernels, its own names
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._NEXT_PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_beam_multi_stream.h"):
        _lib.load_multibeam_stream()


def test_workspace_size():
    """Monotone in every argument, in 256-byte multiples, at least what its arrays need and the offline search's workspace; timed
    >= untimed; every limit and one past it."""
    pkg.build()
    lib = _lib.load_multibeam_stream()
    size = _lib.multibeam_stream_workspace_bytes
    for T, S, K, E, N, H, J, V, dt in ((10, 16, 4, 2, 512, 640, 640, 4096, 1), (1, 1, 1, 1, 1, 1, 64, 2, 0), (9, 3, 4, 3, 27, 8, 64, 27, 0),
                                       (9, 3, 16, 8, 72, 16, 128, 126, 1), (7, 2, 8, 2, 5, 4096, 128, 1030, 1), (5, 32, 16, 1, 5, 8, 64, 12, 0)):
        n = size(T, S, K, E, N, H, J, V, dt)
        assert n % 256 == 0
        R = S * 2 * K
        assert n >= _lib.multibeam_workspace_bytes(T, S, K, E, N, J, V, dt) + H * J * 4 + J * 4 + S * 4  # + W1, b1, the frame bases
        nt = size(T, S, K, E, N, H, J, V, dt, True)
        assert nt % 256 == 0 and nt >= n + 2 * R * N * 4  # the frame rows
        for timed in (False, True):
            n = size(T, S, K, E, N, H, J, V, dt, timed)
            assert size(T, S, K, E + 1 if E < 8 else E, N, H, J, V, dt, timed) == n  # the rounds cost no memory
            assert size(T + 1, S, K, E, N, H, J, V, dt, timed) > n and size(T, S, K, E, N + 64, H, J, V, dt, timed) > n
            if H < 4096:
                assert size(T, S, K, E, N, H + 1, J, V, dt, timed) >= n and size(T, S, K, E, N, H + 64, J, V, dt, timed) > n
            if R + 2 * K <= 1024:
                assert size(T, S + 1, K, E, N, H, J, V, dt, timed) > n
            if K < 16 and S * 32 <= 1024:
                assert size(T, S, K + 1, E, N, H, J, V, dt, timed) >= n and size(T, S, 16, E, N, H, J, V, dt, timed) > n
            assert size(T, S, K, E, N, H, J, V + (128 if dt else 32), dt, timed) > n
    n = ctypes.c_size_t(0)
    ok = (9, 4, 4, 2, 18, 8, 64, 27, 0, 0)
    assert lib.get_rnnt_multibeam_stream_workspace_size(*ok, ctypes.byref(n)) == 0 and n.value > 0
    names = ("max_chunk_frames", "slots", "beam", "symbols_per_frame", "max_hyp_len", "enc_width", "joint_size", "alphabet_size",
             "joint_dtype")
    bad = dict(max_chunk_frames=(0, -1), slots=(0, -1, 129), beam=(0, 17, -1), symbols_per_frame=(0, 9, -1), max_hyp_len=(0, -3),
               enc_width=(0, -1, 4097), joint_size=(0, 63, -64), alphabet_size=(0, -5), joint_dtype=(2, -1, 1 | 256))
    for i, name in enumerate(names):
        for value in bad[name]:
            args = list(ok)
            args[i] = value
            assert lib.get_rnnt_multibeam_stream_workspace_size(*args, ctypes.byref(n)) == INVALID, (name, value)
    call = lambda *a: lib.get_rnnt_multibeam_stream_workspace_size(*a, ctypes.byref(n))  # noqa: E731
    assert call(9, 128, 4, 2, 18, 8, 64, 27, 0, 0) == 0  # 1024 rows: the last that fit
    assert call(9, 33, 16, 2, 18, 8, 64, 27, 0, 0) == INVALID  # 1056 rows
    assert call(9, 4, 4, 8, 18, 4096, 64, 27, 0, 1) == 0  # the widest encoder, the most rounds
    assert call(1 << 19, 64, 1, 1, 4, 8, 64, 27, 0, 0) == INVALID  # S max_chunk_frames J = 2^31
    # 4 S K N < 2^31 untimed, 8 S K N < 2^31 timed: S K = 512
    assert call(9, 32, 16, 2, (1 << 20) - 1, 8, 64, 27, 0, 0) == 0 and call(9, 32, 16, 2, 1 << 20, 8, 64, 27, 0, 0) == INVALID
    assert call(9, 32, 16, 2, (1 << 19) - 1, 8, 64, 27, 0, 1) == 0 and call(9, 32, 16, 2, 1 << 19, 8, 64, 27, 0, 1) == INVALID
    assert call(9, 32, 16, 2, 1 << 19, 8, 64, 27, 0, 0) == 0  # (untimed takes what timed refuses)
    assert lib.get_rnnt_multibeam_stream_workspace_size(*ok, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_multibeam_stream()
    fake, misaligned, odd = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    o = _lib.make_options(0, 0, 10, 1)

    def begin(W1=fake, b1=fake, W2=fake, b2=fake, H=8, J=64, V=27, S=4, K=4, E=2, N=20, dt=0, timed=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_stream_begin(W1, b1, W2, b2, H, J, V, S, K, E, N, dt, timed, ws, opts)

    def feed(enc=fake, Te=3, cf=fake, reset=fake, final=fake, H=8, J=64, V=27, S=4, K=4, E=2, N=20, dt=0, timed=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_stream_feed(enc, Te, cf, reset, final, H, J, V, S, K, E, N, dt, timed, ws, opts)

    def step(pp=fake, parents=fake, emitted=fake, J=64, V=27, S=4, K=4, E=2, N=20, dt=0, timed=0, ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_stream_step(pp, parents, emitted, J, V, S, K, E, N, dt, timed, ws, opts)

    def results(hyps=fake, lens=fake, scores=fake, stable=fake, frames=None, tstable=None, J=64, V=27, S=4, K=4, E=2, N=20, dt=0, timed=0,
                ws=fake, opts=o):
        return lib.compute_rnnt_multibeam_stream_results(hyps, lens, scores, stable, frames, tstable, J, V, S, K, E, N, dt, timed, ws, opts)

    calls = (begin, feed, step, results)
    for call, required, aligned in ((begin, ("W1", "b1", "W2", "b2", "ws"), ("W1", "b1", "W2", "b2")),
                                    (feed, ("enc", "cf", "ws"), ("enc", "cf", "reset", "final")),
                                    (step, ("pp", "parents", "emitted", "ws"), ("pp", "parents", "emitted")),
                                    (results, ("hyps", "lens", "scores", "ws"), ("hyps", "lens", "scores", "stable"))):
        for name in required:
            assert call(**{name: None}) == INVALID, (call, name)
        for name in aligned:  # every pointer: 4-byte aligned
            assert call(**{name: odd}) == INVALID, (call, name)
    for call in calls:
        assert call(ws=misaligned) == INVALID  # the workspace: 256-byte aligned
        for K in (0, 17, -1):
            assert call(K=K) == INVALID, K
        for E in (0, 9, -1):  # symbols_per_frame outside [1, 8]
            assert call(E=E) == INVALID, E
        for N in (0, -1):  # max_hyp_len < 1
            assert call(N=N) == INVALID, N
        assert call(S=129, K=4) == INVALID and call(S=33, K=16) == INVALID  # slots * 2 * beam > 1024
        for dt in (2, -1, 1 | 256):  # no flag bits
            assert call(dt=dt) == INVALID, dt
        assert call(J=0) == INVALID and call(J=63) == INVALID and call(S=0) == INVALID and call(S=-1) == INVALID
        assert call(V=0) == INVALID and call(V=-5) == INVALID
        assert call(V=8200, dt=1, J=128) == INVALID  # beyond what the beam search takes
        assert call(opts=_lib.make_options(0, 27, 10, 1)) == INVALID  # the blank outside the alphabet
        assert call(opts=_lib.make_options(0, -1, 10, 1)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 0, 1)) == INVALID and call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 1, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 1)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
        assert call(opts=_lib.make_options(0, 0, 1 << 19, 1), S=64) == INVALID  # slots * max_chunk_frames * joint_size = 2^31
        assert call(N=1 << 24, S=8) == INVALID  # 4 S K N = 2^31
        assert call(N=1 << 23, S=8, timed=1) == INVALID  # 8 S K N = 2^31 (the untimed workspace takes it)
    for call in (begin, feed):
        for H in (0, -1, 4097):
            assert call(H=H) == INVALID, H
    for Te in (-1, 11):  # enc_frames outside [0, options.maxT]
        assert feed(Te=Te) == INVALID, Te
    assert feed(enc=None, Te=3) == INVALID  # frames without an encoder output
    assert results(frames=fake) == INVALID and results(tstable=fake) == INVALID  # timed results from an untimed workspace
    assert results(frames=odd, timed=1) == INVALID and results(tstable=odd, timed=1) == INVALID
