"""tests/dense_geometry.py against the source and against its own case table (no GPU): the copied constants equal the ones in
csrc/dense_kernels.hip, every case of tests/test_dense_geometry_gpu.py reaches the corner of the launch geometry it is named
for, dxcd_remap is a bijection, the K splits tile the chunks, and -- what makes the GPU tests' bar mean something -- the emulated
arithmetic with one MFMA term missing lies at least 32 times above the faithful emulation in the error measure rho."""
import functools
import os
import re

import numpy as np
import pytest

from tests import dense_geometry as geo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnnt-speech-recognition_amd", "csrc")
NAMES = sorted(geo.CASES)


def _constant(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*([^,;]+)[,;]", text)
    assert m, name
    assert re.fullmatch(r"[\d\s*<()]+", m.group(1)), (name, m.group(1))
    return eval(m.group(1))  # digits, *, << and parentheses only


@pytest.mark.parametrize("source", sorted(geo.SOURCES))
def test_copied_constants_equal_the_sources(source):
    with open(os.path.join(CSRC, source)) as fh:
        text = fh.read()
    for name, value in geo.SOURCES[source].items():
        assert _constant(text, name) == value, (source, name)
    if source == "dense_kernels.hip":  # rules that are one line each
        assert "int ns = (3 * 256 + tiles - 1) / tiles;" in text and "if (ns > c_all / 8) ns = c_all / 8;" in text
        assert "return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;" in text
        assert "enum { kSlotXe = 0, kSlotXp = 1, kSlotW = 2, kSlotDe = 3, kSlotDp = 4 };" in text
        assert "H >= 32 && J >= 64 && (H % 32) == 0 && (J % 64) == 0" in text


def test_every_case_reaches_the_corner_it_is_named_for():
    info = {}
    for name in NAMES:
        B, T, U, H, J = geo.CASES[name]
        L, g = geo.layout(B, T, U, H, J, 0), geo.launches(B, T, U, H, J)
        info[name] = (L, g)
        print(f"geometry dense {name}: R0={L['R0']} R0p={L['R0p']} R1={L['R1']} Rp={L['Rp']} nsplit={L['nsplit']} ns0={L['ns0']} "
              f"db_blocks={L['db_blocks']} proj={g['proj']} dX={g['dX']} dW1={g['dW1']}")
        assert H % 32 == 0 and J % 64 == 0 and H >= 32 and J >= 64
    L, g = info["a"]
    assert g["proj"]["chunks"] == 1 and L["c0"] == 1 and L["c_all"] == 2
    assert g["proj"]["M"] < 256 and g["proj"]["N"] < 128 and g["dX"]["N"] < 128 and 32 < 128 and 64 < 128  # every tile overhangs
    assert L["Rp"] - L["R0p"] - L["R1"] == 14 and L["R0p"] - L["R0"] == 1
    L, g = info["b"]
    assert L["R0"] % 16 == 0 and L["R0"] == L["R0p"] and g["proj"]["chunks"] == 2 and g["proj"]["N"] == 128
    assert L["Rp"] == L["R0p"] + L["R1"]  # and none behind the pred rows
    L, g = info["c"]
    assert (L["R0"], L["R0p"]) == (255, 256) and g["proj"]["tiles_m"] == 2  # the second M tile is the pred segment alone
    assert g["proj"]["N"] % 128 == 64 and g["proj"]["chunks"] == 3
    L, g = info["d"]
    assert (L["R0"], L["R0p"]) == (257, 272) and g["proj"]["tiles_m"] == 2  # tile 1: enc row 256, padding rows 257..271, the pred rows
    assert L["R0p"] + L["R1"] == 275 and g["dW1"]["tiles_m"] == 2 and geo.CASES["d"][3] - 128 == 32
    L, g = info["e"]
    assert (g["proj"]["tiles_m"], g["proj"]["tiles_n"], g["proj"]["grid"]) == (4, 3, 12) and g["dX"]["grid"] == 12
    assert (12 >> 3, 12 & 7) == (1, 4) and (L["nsplit"], L["ns0"]) == (6, 4) and g["dW1"]["grid"] == 54
    L, g = info["f"]
    assert g["proj"]["chunks"] == 32 and (g["dX"]["N"], g["dX"]["tiles_n"], g["dX"]["grid"]) == (1024, 8, 8) and g["dW1"]["tiles_m"] == 8
    L, g = info["g"]
    assert (g["dX"]["N"], g["dX"]["chunks"]) == (32, 20) and g["proj"]["tiles_n"] == 5
    # between them: the ring's prologue alone (1, 2 chunks), its first steady state (3) and long runs; grids with a remainder above 8
    assert {info[n][1]["proj"]["chunks"] for n in NAMES} >= {1, 2, 3, 32}
    assert any(info[n][1][p]["grid"] > 8 and info[n][1][p]["grid"] % 8 for n in NAMES for p in ("proj", "dX", "dW1"))


def test_xcd_remap_is_a_bijection():
    grids = set(range(1, 65))
    for name in NAMES:
        grids |= {g["grid"] for g in geo.launches(*geo.CASES[name]).values()}
    for n in sorted(grids):
        assert sorted(geo.xcd_remap(b, n) for b in range(n)) == list(range(n)), n


@pytest.mark.parametrize("name", NAMES)
def test_k_splits_tile_the_chunks_exactly_once(name):
    L = geo.layout(*geo.CASES[name], 0)
    r = geo.tn_ranges(L)
    assert len(r) == L["nsplit"] and r[0][0] == 0 and r[-1][1] == L["c_all"]
    assert all(lo < hi for lo, hi in r), r                             # none empty
    assert all(r[i][1] == r[i + 1][0] for i in range(len(r) - 1)), r   # each chunk once
    assert r[L["ns0"] - 1][1] == L["c0"] == r[L["ns0"]][0]             # no split mixes the two segments (and their scales)


def test_restated_layout_has_the_librarys_size():
    from rnnt_speech_recognition_amd import _lib

    for name in NAMES:
        B, T, U, H, J = geo.CASES[name]
        base = _lib.joint_workspace_bytes(T, U, B, J, geo.V)
        assert geo.layout(B, T, U, H, J, base)["total"] == _lib.joint_net_workspace_bytes(T, U, B, H, J, geo.V), name


def test_scale_and_split_follow_the_header():
    rng = np.random.default_rng(0)
    for mag in (1.0, 3e-5, 7e9, 2.0 ** -40, 2.0 ** 13, 2.0 ** 14):
        x = (rng.normal(size=4096) * mag).astype(np.float32)
        S = geo.scale_of(x)
        m = float(np.abs(x).max()) * float(S)
        assert 2.0 ** 13 <= m < 2.0 ** 14 and np.frexp(S)[0] == 0.5
        hi, lo = geo.split(x, S)
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - x.astype(np.float64) * float(S))
        assert err.max() <= 2.0 ** -9  # 22 bits below 2^14 (one more: lo carries its own sign)
    assert geo.scale_of(np.zeros(8, np.float32)) == 1 and geo.scale_of(np.array([1.0, np.inf], np.float32)) == 1
    assert geo.scale_of(np.array([np.nan], np.float32)) == 1
    # the cap: S, S_A S_B and 1 / (S_A S_B) are finite normal f32 numbers whatever the tensors hold
    tiny, huge = np.finfo(np.float32).tiny, np.finfo(np.float32).max
    scales = [geo.scale_of(np.array([v], np.float32)) for v in (1e-45, 1e-36, 2.0 ** -60, 1.0, 2.0 ** 60, 2e38)]
    assert scales[0] == scales[1] == 2.0 ** 63 and scales[-1] == 2.0 ** -63
    for a in scales:
        for b in scales:
            p = np.float32(a) * np.float32(b)
            assert tiny <= p <= huge and tiny <= np.float32(1) / p <= huge


@functools.lru_cache(maxsize=None)
def _separation(name):
    """rho of the four variants for the products of a case: its forward operands, and a stand-in for dproj behind them."""
    B, T, U, H, J = geo.CASES[name]
    L = geo.layout(B, T, U, H, J, 0)
    enc, pred, W1, b1 = geo.operands(name)[:4]
    enc, pred = enc.reshape(B * T, H), pred.reshape(B * U, H)
    de, dp = geo.dproj_standin(B * T, J, 7), geo.dproj_standin(B * U, J, 8)
    refs = {"proj_e": geo.ref_nt(enc, W1.T, b1), "proj_p": geo.ref_nt(pred, W1.T), "d_enc": geo.ref_nt(de, W1), "d_pred": geo.ref_nt(dp, W1),
            "dW1": geo.ref_dw(enc, pred, de, dp)}
    rows = {"d_enc": geo.loud_rows(de), "d_pred": geo.loud_rows(dp)}
    out = {}
    for v in geo.VARIANTS:
        got = dict(zip(("proj_e", "proj_p"), geo.emu_proj(enc, pred, W1, b1, L, v)))
        got.update(zip(("d_enc", "d_pred"), geo.emu_dx(de, dp, W1, L, v)))
        got["dW1"] = geo.emu_dw(enc, pred, de, dp, L, v)
        for key, (ref, den) in refs.items():
            out[key, v] = geo.rho(got[key], ref, den, rows.get(key))
            if key in rows:
                out[key + "_all_rows", v] = geo.rho(got[key], ref, den)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_a_lost_mfma_term_stands_32_times_above_the_faithful_emulation(name):
    """The condition under which `rho_gpu <= 8 max(rho_emu, 2^-24)` can tell a kernel that lost a fragment of a lo image from a
    sound one.  It holds for the forward products and for dW1 as they are.  For d_enc / d_pred it holds on the LOUD rows of dproj
    (within 2^-8 of the tensor's maximum): with ONE scale per tensor a row 2^-30 below the maximum has 8 bits left in its hi
    image and none in lo, so over all rows rho of the faithful scheme is about 2^-9 itself and no variant stands out (printed
    as *_all_rows; that is the scheme as documented -- 22 bits relative to the tensor's largest element -- not a fault)."""
    r = _separation(name)
    for key in ("proj_e", "proj_p", "d_enc", "d_pred", "dW1"):
        emu = r[key, "faithful"]
        print(f"separation {name} {key}: faithful {emu:.3e}  " + "  ".join(f"{v} {r[key, v]:.3e}" for v in geo.VARIANTS[1:]))
        assert emu <= 2.0 ** -20, (name, key, emu)  # the scheme is f32-grade on these operands to begin with
        for v in geo.VARIANTS[1:]:
            assert r[key, v] >= geo.SEPARATION * max(emu, geo.EPS), (name, key, v, r[key, v], emu)
    for key in ("d_enc_all_rows", "d_pred_all_rows"):
        print(f"separation {name} {key}: " + "  ".join(f"{v} {r[key, v]:.3e}" for v in geo.VARIANTS))
