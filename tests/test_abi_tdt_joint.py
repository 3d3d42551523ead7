"""CPU tests of the C-ABI boundary of libwarprnnt_tdtjoint.so, a row of the open table build.LATER_LIBRARIES: the checks
tests/test_abi_tdt_beam.py makes for its library, and every RNNT_STATUS_INVALID_VALUE case of include/rnnt_tdt_joint.h on fake
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
NAME = "tdtjoint"
EXPORTS = ["get_rnnt_tdt_joint_workspace_size", "compute_rnnt_joint_loss_tdt"]
INVALID = 2


def test_the_open_table_holds_the_library_and_the_older_tables_are_unchanged():
    assert NAME in build_mod.LATER_LIBRARIES and NAME in _lib._LATER_SIGNATURES
    assert list(build_mod.LATER_LIBRARIES) == list(_lib._LATER_SIGNATURES)
    assert list(build_mod.LATER_LIBRARIES)[:3] == ["tdtstream", "tdtalign", "tdtbeam"]  # the rows before it are where they were
    assert list(build_mod.LATER_LIBRARIES).index(NAME) > 2
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
    assert lib.borrowed == ("rnnt_tdt_kernels.hip",)  # the lattice sweeps of the TDT loss, as "prunedjoint" borrows the pruned loss's
    assert lib.sources == ("rnnt_tdt_joint_kernels.hip", "rnnt_tdt_joint_entrypoint.hip")
    assert lib.header == "rnnt_tdt_joint.h" and lib.version_script == "rnnt_tdt_joint.map"
    assert build_mod.EXTRA_FLAGS["rnnt_tdt_joint_kernels.hip"] == build_mod.EXTRA_FLAGS["rnnt_pruned_joint_kernels.hip"]
    assert build_mod.TDTJOINT_LIB_PATH == build_mod.lib_path(NAME) == _lib._PATHS[NAME]
    assert build_mod.lib_path(NAME).endswith(os.path.join("lib", "libwarprnnt_tdtjoint.so"))
    deps = build_mod._deps()
    assert os.path.join(ROOT, "include", "rnnt_tdt_joint.h") in deps and os.path.join(build_mod.CSRC, "rnnt_tdt_joint.h") in deps
    for name, other in build_mod.EVERY_LIBRARY.items():  # the fourteen other libraries are built from what they were built from
        if name != NAME:
            assert not any("tdt_joint" in s or "tdtjoint" in s for s in other.sources + other.borrowed), name
    assert build_mod.EVERY_LIBRARY["tdt"].sources == ("rnnt_tdt_kernels.hip", "rnnt_tdt_entrypoint.hip")
    assert build_mod.EVERY_LIBRARY["tdtbeam"].sources == ("tdt_beam_kernels.hip", "rnnt_tdt_beam_entrypoint.hip")


def test_header_binding_and_library_agree():
    text = open(os.path.join(ROOT, "include", build_mod.LATER_LIBRARIES[NAME].header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)))
    assert declared == sorted(_lib._LATER_SIGNATURES[NAME]) == sorted(EXPORTS)
    for symbol in declared:  # as many parameters in the header as the binding passes
        params = re.search(symbol + r"\s*\(([^;{]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == len(_lib._LATER_SIGNATURES[NAME][symbol]), symbol
    pkg.build()
    assert not build_mod.needs_build() and os.path.exists(build_mod.TDTJOINT_LIB_PATH)
    lib = _lib.load_tdtjoint()
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
    for kernel in ("tj_w2max_kernel", "tj_fwd_kernel", "tj_occ_kernel", "tj_bwd_dh_kernel", "tj_reduce_enc_kernel",
                   "tj_reduce_pred_kernel", "tj_bwd_dw_kernel", "tj_reduce_w_kernel", "tdt_sweep_kernel"):
        assert any(kernel in n for n in names), kernel
    for n in names:
        if n.startswith("_Z"):
            assert n.startswith("_ZN4rnnt") and "kernel" in n and "launch" not in n and "device_stub" not in n, n


def test_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.delitem(_lib._libs, NAME, raising=False)
    monkeypatch.setitem(_lib._PATHS, NAME, str(tmp_path / os.path.basename(build_mod.lib_path(NAME))))
    with pytest.raises(_lib.RNNTLibraryError, match="no eager fallback.*rnnt_tdt_joint.h"):
        _lib.load_tdtjoint()


def test_workspace_size():
    """In 256-byte multiples, monotone in each of the five arguments (it has no other), at least the TDT loss's workspace of the
    same lattice, and at the headline lattice below a quarter of B T U J floats: no per-cell [J] array exists.  Every limit and one
    past it."""
    pkg.build()
    lib = _lib.load_tdtjoint()
    size = _lib.tdt_joint_workspace_bytes
    for T, U, B, D, J in ((600, 150, 32, 5, 640), (1, 1, 1, 1, 64), (9, 3, 4, 5, 64), (31, 33, 2, 8, 128), (64, 1024, 1, 2, 576)):
        n = size(T, U, B, D, J)
        assert n % 256 == 0
        assert n >= _lib.tdt_workspace_bytes(T, U, B, D)
        assert size(T + 1, U, B, D, J) > n and size(T, U, B + 1, D, J) > n
        if U < 1024:
            assert size(T, U + 1, B, D, J) > n
        if D < 8:
            assert size(T, U, B, D + 1, J) > n
        if J < 640:
            assert size(T, U, B, D, J + 64) > n
    T, U, B, D, J = 600, 150, 32, 5, 640
    assert size(T, U, B, D, J) < B * T * U * J * 4 // 4
    n = ctypes.c_size_t(0)
    bad = [(0, 3, 4, 5, 64), (9, 0, 4, 5, 64), (9, 3, 0, 5, 64), (-1, 3, 4, 5, 64), (9, 1025, 4, 5, 64), (9, 3, 4, 0, 64),
           (9, 3, 4, 9, 64), (9, 3, 4, 5, 0), (9, 3, 4, 5, 63), (9, 3, 4, 5, 96), (9, 3, 4, 5, 704), (9, 3, 4, 5, -64),
           (1 << 11, 1 << 10, 1 << 10, 5, 64)]  # minibatch * maxT * maxU = 2^31
    for args in bad:
        assert lib.get_rnnt_tdt_joint_workspace_size(*args, ctypes.byref(n)) == INVALID, args
    assert lib.get_rnnt_tdt_joint_workspace_size(9, 1024, 4, 8, 640, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.get_rnnt_tdt_joint_workspace_size(9, 3, 4, 5, 64, None) == INVALID


def test_argument_validation_needs_no_device():
    """Every RNNT_STATUS_INVALID_VALUE case of the header, on pointers that are never dereferenced: nothing is enqueued."""
    pkg.build()
    lib = _lib.load_tdtjoint()
    fake, off4, off1 = ctypes.c_void_p(256), ctypes.c_void_p(260), ctypes.c_void_p(257)
    o = _lib.make_options(0, 0, 10, 4)
    d5 = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def call(enc=fake, pred=fake, W2=fake, b2=fake, labels=fake, ll=fake, il=fake, scale=None, J=64, V=27, dur=d5, D=5, sigma=0.0,
             B=4, costs=fake, d_enc=fake, d_pred=fake, dW2=fake, db2=fake, ws=fake, opts=o):
        return lib.compute_rnnt_joint_loss_tdt(enc, pred, W2, b2, labels, ll, il, scale, J, V, dur, D, sigma, B, costs, d_enc, d_pred,
                                               dW2, db2, ws, opts)

    for name in ("enc", "pred", "W2", "b2", "labels", "ll", "il", "dur", "ws"):  # a NULL required pointer
        assert call(**{name: None}) == INVALID, name
    none = dict(d_enc=None, d_pred=None, dW2=None, db2=None)
    assert call(costs=None, **none) == INVALID  # nothing to compute
    for name in none:  # the four gradients: all given or all NULL
        assert call(**{name: None}) == INVALID, name
        assert call(**{k: (fake if k == name else None) for k in none}) == INVALID, name
    for name in ("enc", "pred", "d_enc", "d_pred"):  # 16-byte aligned
        assert call(**{name: off4}) == INVALID, name
    for name in ("W2", "b2", "labels", "ll", "il", "scale", "costs", "dW2", "db2"):  # 4-byte aligned
        assert call(**{name: off1}) == INVALID, name
    assert call(ws=off4) == INVALID  # the workspace: 256-byte aligned
    for J in (0, 32, 63, 96, 704, -64):
        assert call(J=J) == INVALID, J
    for V in (1, 0, -5, 8188):  # V + D beyond 8192
        assert call(V=V) == INVALID, V
    for D in (0, 9, -1):
        assert call(D=D) == INVALID, D
    assert call(B=0) == INVALID and call(B=-1) == INVALID
    for sigma in (-0.1, float("inf"), float("nan")):
        assert call(sigma=sigma) == INVALID, sigma
    assert call(opts=_lib.make_options(0, 27, 10, 4)) == INVALID  # the blank inside the duration head
    assert call(opts=_lib.make_options(0, -1, 10, 4)) == INVALID
    assert call(opts=_lib.make_options(0, 0, 0, 4)) == INVALID and call(opts=_lib.make_options(0, 0, 10, 0)) == INVALID
    assert call(opts=_lib.make_options(0, 0, 10, 1025)) == INVALID  # maxU beyond the sweep's threads
    assert call(opts=_lib.make_options(0, 0, 10, 4, loc=_lib.RNNT_CPU)) == INVALID  # no CPU fallback
    rows_first = _lib.make_options(0, 0, 10, 4)
    rows_first.batch_first = False
    assert call(opts=rows_first) == INVALID
    assert call(opts=_lib.make_options(0, 0, 1 << 11, 1 << 10), B=1 << 10) == INVALID  # minibatch * maxT * maxU = 2^31
    for bad in ([0, 2, 1], [0, 1, 1], [-1, 0, 1], [0], [2, 3], [0, 1, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8]):
        arr = (ctypes.c_int * len(bad))(*bad)
        assert call(dur=arr, D=len(bad)) == INVALID, bad
