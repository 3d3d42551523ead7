"""CPU tests of the C-ABI boundary of libwarprnnt_tdtstream.so, the first library of the open table build.LATER_LIBRARIES: the
checks tests/test_abi_tdt_greedy.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_tdt_stream.h
on fake pointers.  The open table is not pinned to a list here: the next library is one more row of it."""
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
NAME = "tdtstream"
EXPORTS = ["get_rnnt_tdt_greedy_stream_workspace_size", "compute_rnnt_tdt_greedy_stream_begin", "compute_rnnt_tdt_greedy_stream_feed",
           "compute_rnnt_tdt_greedy_stream_step"]
INVALID = 2


def test_the_open_table_holds_the_library_and_the_older_tables_are_unchanged():
    assert NAME in build_mod.LATER_LIBRARIES and NAME in _lib._LATER_SIGNATURES
    assert list(build_mod.LATER_LIBRARIES) == list(_lib._LATER_SIGNATURES)
    # the three older tables are what they were
    assert list(build_mod.LIBRARIES) == ["base", "bias", "mod", "modalign", "pruned", "simple", "prunedjoint", "pruneranges", "lm"]
    assert list(build_mod.MORE_LIBRARIES) == ["tdt"]
    assert list(build_mod.ALL_LIBRARIES) == list(build_mod.LIBRARIES) + ["tdt", "tdtgreedy"] == list(_lib._ALL_SIGNATURES)
    assert list(_lib.SIGNATURES) == list(build_mod.LIBRARIES) and list(_lib.MORE_SIGNATURES) == ["tdt"]
    # the union is what the build and the binding work over
    every = list(build_mod.ALL_LIBRARIES) + list(build_mod.LATER_LIBRARIES)
    assert list(build_mod.EVERY_LIBRARY) == every == list(_lib._EVERY_SIGNATURE) == list(_lib._PATHS)
    assert not set(build_mod.ALL_LIBRARIES) & set(build_mod.LATER_LIBRARIES)
    lib = build_mod.LATER_LIBRARIES[NAME]
    assert type(lib) is type(build_mod.LIBRARIES["bias"])
    assert lib.borrowed == build_mod.LIBRARIES["bias"].borrowed + ("tdt_greedy_kernels.hip",)
    assert lib.sources == ("tdt_stream_kernels.hip", "rnnt_tdt_stream_entrypoint.hip")
    assert lib.header == "rnnt_tdt_stream.h" and lib.version_script == "rnnt_tdt_stream.map"
    assert build_mod.EXTRA_FLAGS["tdt_stream_kernels.hip"] == build_mod.EXTRA_FLAGS["greedy_kernels.hip"]
    assert build_mod.TDTSTREAM_LIB_PATH == build_mod.lib_path(NAME) == _lib._PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_tdtstream.so"))
    deps = build_mod._deps()
    assert os.path.join(ROOT, "include", "rnnt_tdt_stream.h") in deps and os.path.join(build_mod.CSRC, "tdt_greedy_common.h") in deps
    for name in ("base", "tdt", "tdtgreedy"):  # what the feature must not touch
        assert "tdt_stream_kernels.hip" not in build_mod.EVERY_LIBRARY[name].sources + build_mod.EVERY_LIBRARY[name].borrowed


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.LATER_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._LATER_SIGNATURES[NAME]) == sorted(EXPORTS)
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.TDTSTREAM_LIB_PATH)
    lib = _lib.load_tdtstream()
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
    for kernel in ("tdt_stream_feed_kernel", "tdt_stream_update_kernel", "tdt_stream_begin_kernel", "tdt_greedy_step_kernel",
                   "greedy_stream_proj_kernel"):
        assert any(kernel in n for n in names), kernel
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_tdt_stream.h"):
        _lib.load_tdtstream()


def test_workspace_size():
    pkg.build()
    lib = _lib.load_tdtstream()
    size = _lib.tdt_greedy_stream_workspace_bytes
    for dtype, J, V, D, H in ((1, 640, 1024, 5, 320), (0, 640, 28, 5, 1), (0, 704, 27, 5, 16), (1, 128, 2, 1, 4096), (0, 64, 120, 8, 100)):
        n = size(20, 64, H, J, V, D, dtype)
        assert n % 256 == 0
        # the TDT greedy workspace at (max_chunk_frames, slots), W1 and b1, one frame base per slot
        assert n >= _lib.tdt_greedy_workspace_bytes(20, 64, J, V, D, dtype) + 4 * (H * J + J) + 4 * 64
        assert size(20, 65, H, J, V, D, dtype) >= n and size(20, 128, H, J, V, D, dtype) > n  # monotone in slots
        assert size(21, 64, H, J, V, D, dtype) > n  # ... and in chunk frames
    n = ctypes.c_size_t(0)
    bad = [(0, 64, 320, 640, 1024, 5, 1), (20, 0, 320, 640, 1024, 5, 1), (20, 1025, 320, 640, 1024, 5, 1), (20, 64, 0, 640, 1024, 5, 1),
           (20, 64, 4097, 640, 1024, 5, 1), (20, 64, 320, 0, 1024, 5, 1), (20, 64, 320, 640, 1, 5, 1), (20, 64, 320, 640, 1024, 0, 1),
           (20, 64, 320, 640, 1024, 9, 1), (20, 64, 320, 640, 1024, 5, 2), (20, 64, 320, 640, 1024, 5, -1),
           (20, 64, 320, 600, 1024, 5, 1), (20, 64, 320, 768, 1024, 5, 1), (20, 64, 320, 640, 8190, 5, 1),  # joint_dtype 1
           (20, 64, 320, 640, 124, 5, 0), (20, 64, 320, 704, 28, 5, 0),  # joint_dtype 0: R <= 128; R <= 32 above J = 640
           (1 << 13, 512, 320, 640, 1024, 5, 1)]  # slots * max_chunk_frames * joint_size >= 2^31
    for args in bad:
        assert lib.get_rnnt_tdt_greedy_stream_workspace_size(*args, ctypes.byref(n)) == INVALID, args
    assert lib.get_rnnt_tdt_greedy_stream_workspace_size(20, 1024, 4096, 640, 8187, 5, 1, ctypes.byref(n)) == 0  # every limit reached
    assert lib.get_rnnt_tdt_greedy_stream_workspace_size(20, 64, 320, 640, 1024, 5, 1, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_tdtstream()
    fake, misaligned, odd = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    o = _lib.make_options(0, 0, 10, 1)
    d5 = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def begin(W1=fake, b1=fake, W2=fake, b2=fake, H=320, J=640, V=1024, dur=d5, D=5, S=4, dtype=1, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_greedy_stream_begin(W1, b1, W2, b2, H, J, V, dur, D, S, dtype, ws, opts)

    def feed(enc=fake, Te=10, frames=fake, reset=None, final=None, maxsym=None, cap=10, lengths=fake, scores=fake, done=fake, H=320,
             J=640, V=1024, D=5, S=4, dtype=1, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_greedy_stream_feed(enc, Te, frames, reset, final, maxsym, cap, lengths, scores, done, H, J, V, D, S,
                                                       dtype, ws, opts)

    def step(pp=fake, hyps=fake, hf=fake, hl=fake, N=16, lengths=fake, scores=fake, emitted=fake, done=fake, stats=None, J=640, V=1024,
             D=5, S=4, dtype=1, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_greedy_stream_step(pp, hyps, hf, hl, N, lengths, scores, emitted, done, stats, J, V, D, S, dtype, ws,
                                                       opts)

    calls = (begin, feed, step)
    # required pointers
    for name in ("W1", "b1", "W2", "b2", "dur", "ws"):
        assert begin(**{name: None}) == INVALID, name
    for name in ("enc", "frames", "lengths", "scores", "done", "ws"):
        assert feed(**{name: None}) == INVALID, name
    for name in ("pp", "hyps", "lengths", "scores", "emitted", "done", "ws"):
        assert step(**{name: None}) == INVALID, name
    # the chunk: enc_frames inside [0, max_chunk_frames]
    assert feed(Te=-1) == INVALID and feed(Te=11) == INVALID
    # max_per_frame
    assert feed(cap=0) == INVALID and feed(cap=-1) == INVALID
    # hyp_frames / hyp_logp: both or neither; 4-byte alignment; max_hyp_len
    assert step(hf=None) == INVALID and step(hl=None) == INVALID
    for name in ("hyps", "hf", "hl"):
        assert step(**{name: odd}) == INVALID, name
    assert step(N=0) == INVALID and step(N=-3) == INVALID and step(N=1 << 29, S=4) == INVALID
    # the slots and the encoder width
    for call in calls:
        assert call(S=0) == INVALID and call(S=-1) == INVALID and call(S=1025) == INVALID, call
    for call in (begin, feed):
        assert call(H=0) == INVALID and call(H=-4) == INVALID and call(H=4097) == INVALID, call
    # the heads and the blank
    for call in calls:
        assert call(V=1) == INVALID and call(V=0) == INVALID and call(V=-5) == INVALID, call
        assert call(D=0) == INVALID and call(D=-1) == INVALID and call(D=9) == INVALID, call
        assert call(opts=_lib.make_options(0, 1024, 10, 1)) == INVALID  # the blank inside the duration head
        assert call(opts=_lib.make_options(0, 1029, 10, 1)) == INVALID and call(opts=_lib.make_options(0, -1, 10, 1)) == INVALID
    # durations
    for bad in ([0, 2, 1], [0, 1, 1], [-1, 0, 1], [0], [2, 3], [0, 1, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8]):
        arr = (ctypes.c_int * len(bad))(*bad)
        assert begin(dur=arr, D=len(bad)) == INVALID, bad
    # the greedy decoder's cases: sizes, joint_dtype, options, the workspace, the shapes
    for call in calls:
        assert call(J=0) == INVALID and call(opts=_lib.make_options(0, 0, 0, 1)) == INVALID, call
        assert call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
        assert call(dtype=2) == INVALID and call(dtype=-1) == INVALID and call(dtype=1 | 0x100) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 1, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 1)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
        assert call(ws=misaligned) == INVALID
        assert call(J=600) == INVALID and call(J=768) == INVALID and call(V=8190) == INVALID  # joint_dtype 1
        assert call(dtype=0, V=124) == INVALID and call(dtype=0, J=704, V=28) == INVALID  # joint_dtype 0: R <= 128; <= 32 above 640
        assert call(opts=_lib.make_options(0, 0, 1 << 13, 1), S=512) == INVALID  # slots * maxT * joint_size = 2^31 ... and beyond
