"""CPU tests of the C-ABI boundary of libwarprnnt_tdtalign.so, a row of the open table build.LATER_LIBRARIES: the checks
tests/test_abi_tdt_stream.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_tdt_align.h on fake
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
NAME = "tdtalign"
EXPORTS = ["get_rnnt_tdt_align_workspace_size", "compute_rnnt_tdt_align_cells", "compute_rnnt_tdt_align_path", "compute_rnnt_tdt_align"]
INVALID = 2


def test_the_open_table_holds_the_library_and_the_older_tables_are_unchanged():
    assert NAME in build_mod.LATER_LIBRARIES and NAME in _lib._LATER_SIGNATURES
    assert list(build_mod.LATER_LIBRARIES) == list(_lib._LATER_SIGNATURES)
    assert list(build_mod.LATER_LIBRARIES)[0] == "tdtstream"  # the rows before it are where they were
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
    assert lib.borrowed == ()  # it borrows nothing
    assert lib.sources == ("rnnt_tdtalign_kernels.hip", "rnnt_tdtalign_entrypoint.hip")
    assert lib.header == "rnnt_tdt_align.h" and lib.version_script == "rnnt_tdtalign.map"
    assert "rnnt_tdtalign_kernels.hip" not in build_mod.EXTRA_FLAGS  # the flags of the loss's kernels: none beyond HIPCC_FLAGS
    assert build_mod.TDTALIGN_LIB_PATH == build_mod.lib_path(NAME) == _lib._PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_tdtalign.so"))
    deps = build_mod._deps()
    assert os.path.join(ROOT, "include", "rnnt_tdt_align.h") in deps and os.path.join(build_mod.CSRC, "rnnt_tdtalign.h") in deps
    for name, other in build_mod.EVERY_LIBRARY.items():  # the twelve other libraries are built from what they were built from
        if name != NAME:
            assert not any("tdtalign" in s for s in other.sources + other.borrowed), name
    assert build_mod.EVERY_LIBRARY["tdt"].sources == ("rnnt_tdt_kernels.hip", "rnnt_tdt_entrypoint.hip")


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.LATER_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._LATER_SIGNATURES[NAME]) == sorted(EXPORTS)
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.TDTALIGN_LIB_PATH)
    lib = _lib.load_tdtalign()
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
    for kernel in ("tdtalign_cells_kernel", "tdtalign_path_kernel"):
        assert any(kernel in n for n in names), kernel
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_tdt_align.h"):
        _lib.load_tdtalign()


def test_workspace_size():
    """Monotone, in 256-byte multiples, independent of the vocabulary (the entry point takes none), at most 2 D floats and one
    decision byte per skewed node; every limit and one past it."""
    pkg.build()
    lib = _lib.load_tdtalign()
    size = _lib.tdt_align_workspace_bytes
    for T, U, B, D in ((600, 151, 32, 5), (1, 1, 1, 1), (7, 6, 1, 4), (40, 64, 3, 8), (40, 65, 3, 8), (9, 1024, 2, 2)):
        n = size(T, U, B, D)
        assert n % 256 == 0
        Up = (U + 63) // 64 * 64
        nodes = B * (T + U) * Up  # skewed rows n = t + u, Up columns
        assert nodes * (2 * D * 4 + 1) <= n <= nodes * (2 * D * 4 + 1) + 3 * 256  # the weights, the decisions; sigma and padding
        assert size(T + 1, U, B, D) > n and size(T, U, B + 1, D) > n  # monotone in frames and batch
        if U < 1024:
            assert size(T, U + 1, B, D) >= n and size(T, min(U + 64, 1024), B, D) > n  # ... in label positions
        if D < 8:
            assert size(T, U, B, D + 1) > n  # ... and in durations
    n = ctypes.c_size_t(0)
    bad = [(0, 10, 4, 5), (10, 0, 4, 5), (10, 10, 0, 5), (-1, 10, 4, 5), (10, 1025, 4, 5), (10, 10, 4, 0), (10, 10, 4, 9), (10, 10, 4, -1),
           (1 << 21, 1024, 1, 5), (1 << 11, 1024, 1024, 5)]  # minibatch * maxT * maxU = 2^31
    for args in bad:
        assert lib.get_rnnt_tdt_align_workspace_size(*args, ctypes.byref(n)) == INVALID, args
    assert lib.get_rnnt_tdt_align_workspace_size((1 << 21) - 1, 1024, 1, 8, ctypes.byref(n)) == 0  # every limit reached
    assert n.value >= ((1 << 21) - 1 + 1024) * 1024 * (2 * 8 * 4 + 1)
    assert lib.get_rnnt_tdt_align_workspace_size(10, 10, 4, 5, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_tdtalign()
    fake, misaligned, odd = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    o = _lib.make_options(0, 0, 10, 6)
    d5 = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def cells(acts=fake, S=10, t0=0, labels=fake, ll=fake, il=fake, V=28, dur=d5, D=5, sigma=0.0, B=4, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_align_cells(acts, S, t0, labels, ll, il, V, dur, D, sigma, B, ws, opts)

    def path(frames=fake, durs=fake, logp=fake, scores=fake, ll=fake, il=fake, dur=d5, D=5, B=4, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_align_path(frames, durs, logp, scores, ll, il, dur, D, B, ws, opts)

    def whole(acts=fake, labels=fake, ll=fake, il=fake, V=28, dur=d5, D=5, sigma=0.0, B=4, frames=fake, durs=fake, logp=fake,
              scores=fake, ws=fake, opts=o):
        return lib.compute_rnnt_tdt_align(acts, labels, ll, il, V, dur, D, sigma, B, frames, durs, logp, scores, ws, opts)

    calls = (cells, path, whole)
    # required pointers, and their 4-byte alignment
    for call, names in ((cells, ("acts", "labels", "ll", "il", "dur", "ws")),
                        (path, ("frames", "durs", "logp", "scores", "ll", "il", "dur", "ws")),
                        (whole, ("acts", "labels", "ll", "il", "dur", "frames", "durs", "logp", "scores", "ws"))):
        for name in names:
            assert call(**{name: None}) == INVALID, (call, name)
            if name not in ("dur", "ws"):
                assert call(**{name: odd}) == INVALID, (call, name)
    for call in calls:
        assert call(ws=misaligned) == INVALID  # the workspace: 256-byte aligned
    # the slab
    for S, t0 in ((0, 0), (-1, 0), (11, 0), (10, 1), (1, 10), (1, -1), (2**31 - 1, 2**31 - 1)):
        assert cells(S=S, t0=t0) == INVALID, (S, t0)
    # sigma
    for call in (cells, whole):
        for sigma in (-0.01, float("nan"), float("inf")):
            assert call(sigma=sigma) == INVALID, sigma
    # the vocabulary and the blank
    for call in (cells, whole):
        assert call(V=1) == INVALID and call(V=0) == INVALID and call(V=-5) == INVALID, call
        assert call(opts=_lib.make_options(0, 28, 10, 6)) == INVALID  # the blank inside the duration head
    for call in calls:
        assert call(opts=_lib.make_options(0, -1, 10, 6)) == INVALID
    # durations
    for call in calls:
        assert call(D=0) == INVALID and call(D=-1) == INVALID and call(D=9) == INVALID, call
        for bad in ([0, 2, 1], [0, 1, 1], [-1, 0, 1], [0], [2, 3], [0, 1, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8]):
            arr = (ctypes.c_int * len(bad))(*bad)
            assert call(dur=arr, D=len(bad)) == INVALID, bad
    # the shape, the device, the layout
    for call in calls:
        assert call(B=0) == INVALID and call(B=-1) == INVALID
        assert call(opts=_lib.make_options(0, 0, 0, 6)) == INVALID and call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 1025)) == INVALID  # maxU <= 1024
        assert call(opts=_lib.make_options(0, 0, 1 << 11, 1024), B=1024) == INVALID  # minibatch * maxT * maxU = 2^31
        assert call(opts=_lib.make_options(0, 0, 10, 6, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 6)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
