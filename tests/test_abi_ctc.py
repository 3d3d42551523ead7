"""CPU tests of the C-ABI boundary of libwarprnnt_ctc.so, a row of build.NEXT_LIBRARIES: the checks
tests/test_abi_multibeam_stream.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_ctc.h on fake
pointers.  (The open table is not pinned to a list or a length here: the next library is one more row of it.)"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest

import rnnt_speech_recognition_amd as pkg
from rnnt_speech_recognition_amd import _lib
from tests import ctc_cases as cc

build_mod = importlib.import_module("rnnt_speech_recognition_amd.build")  # (the package's `build` attribute is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc"
EXPORTS = ["get_rnnt_ctc_workspace_size", "compute_rnnt_ctc_loss", "compute_rnnt_ctc_greedy"]
SOURCES = ("rnnt_ctc_kernels.hip", "rnnt_ctc_entrypoint.hip")
INVALID = 2


def test_the_open_table_holds_the_library_after_the_two_rows_that_are_unchanged():
    assert NAME in build_mod.NEXT_LIBRARIES and NAME in _lib._NEXT_SIGNATURES
    names = list(build_mod.NEXT_LIBRARIES)
    assert names == list(_lib._NEXT_SIGNATURES) == list(_lib._NEXT_PATHS)
    assert names[:2] == ["multibeam", "multibeamstream"] and names.index(NAME) == 2
    assert list(build_mod.BUILT_LIBRARIES) == list(build_mod.EVERY_LIBRARY) + names == list(_lib._BUILT_SIGNATURES)
    old = build_mod.NEXT_LIBRARIES["multibeam"]
    assert old.sources == ("multibeam_kernels.hip", "rnnt_multibeam_entrypoint.hip") and old.borrowed == build_mod._BASE_KERNELS
    assert old.header == "rnnt_beam_multi.h" and old.version_script == "rnnt_multibeam.map"
    old = build_mod.NEXT_LIBRARIES["multibeamstream"]
    assert old.sources == ("tsd_stream_kernels.hip", "rnnt_tsd_stream_entrypoint.hip") and old.borrowed == build_mod._BASE_KERNELS
    assert old.header == "rnnt_beam_multi_stream.h" and old.version_script == "rnnt_tsdstream.map"
    assert len(_lib._NEXT_SIGNATURES["multibeam"]) == 4 and len(_lib._NEXT_SIGNATURES["multibeamstream"]) == 5
    lib = build_mod.NEXT_LIBRARIES[NAME]
    assert type(lib) is type(build_mod.LIBRARIES["bias"])
    assert lib.sources == SOURCES and lib.borrowed == ()  # self-contained, as "mod" and "simple"
    assert lib.header == "rnnt_ctc.h" and lib.version_script == "rnnt_ctc.map"
    assert build_mod.CTC_LIB_PATH == build_mod.lib_path(NAME) == _lib._NEXT_PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_ctc.so"))
    deps = build_mod._deps()
    assert os.path.join(build_mod.CSRC, "rnnt_ctc.h") in deps and os.path.join(ROOT, "include", "rnnt_ctc.h") in deps
    for name, other in build_mod.BUILT_LIBRARIES.items():  # no other library lists or borrows the new sources
        if name != NAME:
            assert not set(SOURCES) & set(other.sources + other.borrowed), name
    for f in SOURCES:
        assert '.hip"' not in open(os.path.join(build_mod.CSRC, f)).read()  # no unit includes a unit


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.NEXT_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._NEXT_SIGNATURES[NAME]) == sorted(EXPORTS)
    for symbol in declared:  # as many parameters in the header as the binding passes
        params = re.search(symbol + r"\s*\(([^;{]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == len(_lib._NEXT_SIGNATURES[NAME][symbol]), symbol
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.CTC_LIB_PATH)
    lib = _lib.load_ctc()
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
    for kernel in ("ctc_prepare_kernel", "ctc_rows_kernel", "ctc_sweep_kernel", "ctc_grad_kernel", "ctc_greedy_kernel"):
        assert any(kernel in n for n in names), kernel
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._NEXT_PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_ctc.h"):
        _lib.load_ctc()


def test_workspace_size():
    """Monotone in every argument, in 256-byte multiples, at least the arrays it must hold (float64 alpha and beta of 2U - 1 states
    and the 2U gathered edge log-probabilities per frame), independent of V (it takes none); every limit and one past it."""
    pkg.build()
    lib = _lib.load_ctc()
    size = _lib.ctc_workspace_bytes
    wave, switch, wide = cc.tier_boundaries()
    for T, U, B in ((1, 1, 1), (7, 1, 2), (10, 6, 3), (600, 151, 32), (300, 101, 32), (1500, 301, 16), (9, 64, 1), (9, 65, 1),
                    (5, switch, 1), (5, switch + 1, 1), (3, 8192, 1)):
        n = size(T, U, B)
        assert n % 256 == 0
        assert n >= B * T * ((2 * U - 1) * 8 * 2 + 2 * U * 4) + B * (8 + 4 * U)
        assert size(T + 1, U, B) > n and size(T, U, B + 1) > n
        if U < 8192:
            assert size(T, U + 1, B) >= n
    for U in wave + [switch] + wide:  # a tier more: a wider row
        assert size(9, U + 1, 2) > size(9, U, 2)
    n = ctypes.c_size_t(0)
    call = lambda *a: lib.get_rnnt_ctc_workspace_size(*a, ctypes.byref(n))  # noqa: E731
    assert call(10, 6, 3) == 0 and n.value > 0
    for args in ((0, 6, 3), (-1, 6, 3), (10, 0, 3), (10, -2, 3), (10, 6, 0), (10, 6, -1)):
        assert call(*args) == INVALID, args
    assert call(3, 8192, 1) == 0 and call(3, 8193, 1) == INVALID  # maxU in [1, 8192]
    # minibatch * maxT * (2 maxU - 1) < 2^31: 2 * 8192 - 1 = 16383, 2^31 / 16383 = 131080.0002...
    assert call(131080, 8192, 1) == 0 and call(131081, 8192, 1) == INVALID
    assert call((1 << 31) - 1, 1, 1) == 0 and call(1 << 30, 1, 2) == INVALID and call(1 << 29, 2, 2) == INVALID
    assert lib.get_rnnt_ctc_workspace_size(10, 6, 3, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_ctc()
    fake, misaligned, odd = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(258)
    o = _lib.make_options(0, 0, 10, 6)

    def loss(acts=fake, grads=fake, labels=fake, ll=fake, il=fake, scale=None, V=28, B=3, costs=fake, ws=fake, opts=o):
        return lib.compute_rnnt_ctc_loss(acts, grads, labels, ll, il, scale, V, B, costs, ws, opts)

    def greedy(acts=fake, il=fake, V=28, B=3, tokens=fake, frames=None, lengths=fake, opts=o):
        return lib.compute_rnnt_ctc_greedy(acts, il, V, B, tokens, frames, lengths, opts)

    for name in ("acts", "labels", "ll", "il", "ws"):
        assert loss(**{name: None}) == INVALID, name
    assert loss(grads=None, costs=None) == INVALID  # nothing to do
    for name in ("acts", "grads", "labels", "ll", "il", "scale", "costs"):  # every pointer: 4-byte aligned
        assert loss(**{name: odd}) == INVALID, name
    assert loss(ws=misaligned) == INVALID and loss(ws=odd) == INVALID  # the workspace: 256-byte aligned
    for name in ("acts", "il", "tokens", "lengths"):
        assert greedy(**{name: None}) == INVALID, name
    for name in ("acts", "il", "tokens", "frames", "lengths"):
        assert greedy(**{name: odd}) == INVALID, name
    for call in (loss, greedy):
        for V in (1, 0, -3):
            assert call(V=V) == INVALID, V
        for B in (0, -1):
            assert call(B=B) == INVALID, B
        assert call(opts=_lib.make_options(0, 28, 10, 6)) == INVALID  # the blank outside the alphabet
        assert call(opts=_lib.make_options(0, -1, 10, 6)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 0, 6)) == INVALID and call(opts=_lib.make_options(0, 0, -1, 6)) == INVALID
        assert call(opts=_lib.make_options(0, 0, 10, 6, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
        rows_first = _lib.make_options(0, 0, 10, 6)
        rows_first.batch_first = False
        assert call(opts=rows_first) == INVALID
        assert call(opts=_lib.make_options(0, 0, 1 << 19, 1), V=4096, B=1) == INVALID  # minibatch * maxT * alphabet_size = 2^31
    for U in (0, -1, 8193):  # maxU outside [1, 8192]; the decoder does not read it
        assert loss(opts=_lib.make_options(0, 0, 10, U)) == INVALID, U
    assert loss(opts=_lib.make_options(0, 0, 131081, 8192), B=1, V=2) == INVALID  # minibatch * maxT * (2 maxU - 1) >= 2^31
    assert loss(opts=_lib.make_options(0, 0, 1 << 29, 2), B=2, V=2) == INVALID
