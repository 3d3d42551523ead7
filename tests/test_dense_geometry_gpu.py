"""The three split-precision GEMMs of the joint's first Dense layer (csrc/dense_kernels.hip) looked at ALONE, behind the C ABI
(compute_rnnt_joint_net_loss_fwd, then _bwd, joint_dtype 0) on a workspace filled with 0xFF bytes: tests/dense_geometry.py says
where the layer's arrays lie in that workspace, so every product is compared with float64 of the very tensors it consumed --
proj_e / proj_p of enc, pred, W1, b1; d_enc, d_pred, dW1, db1 of the dproj the fused joint left in the workspace -- instead of
through tanh, the J x V product and the lattice (tests/test_dense_gpu.py, bar 1e-4).

Per case of dense_geometry.CASES (each named for a corner of the launch geometry):
  * the operand scales and the binary16 hi / lo images are bitwise the emulation's split of the same f32 tensors, padding rows
    exact zeros;
  * rho = max |C - ref64| / sum_k |a||b| of the five products is at most 8 max(rho_emu, 2^-24), rho_emu being the NumPy
    emulation's rho for the same operands (tests/test_dense_geometry.py: an MFMA term lost stands >= 32 times above it).  For
    d_enc / d_pred the same bar is also asked of the LOUD rows of dproj alone (dense_geometry.loud_rows), where it is sharp;
  * db1 against the float64 column sums, within the worst case of the summation depth the code has.
Then: exact zeros at padded positions, invariance under powers of two, no scale left over from an earlier call on the same
workspace, all-zero and vanishing tensors, and a misaligned operand.

The measured rho are printed and, with DENSE_ACCURACY_DIR set, collected in dense_accuracy.json in that directory (kept in
profiles/dense_accuracy_notes.md)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import rnnt_oracle as orc
from rnnt_speech_recognition_amd import _lib
from tests import dense_geometry as geo

pytestmark = pytest.mark.gpu
NAMES = sorted(geo.CASES)
KEYS = ("d_enc", "d_pred", "dW1", "db1", "dW2", "db2")
TOL = 1e-4  # tests/test_dense_gpu.py's bar, for the whole-network comparison of the vanishing-tensor test


def _record(route, **row):
    out = os.environ.get("DENSE_ACCURACY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "dense_accuracy.json")
    try:
        rows = json.load(open(path))
    except (OSError, ValueError):
        rows = {}
    rows[route] = row
    json.dump(rows, open(path, "w"), indent=1, sort_keys=True)


def _layout(ops):
    enc, pred, W1 = ops[:3]
    B, T, H = enc.shape
    U, J = pred.shape[1], W1.shape[1]
    return geo.layout(B, T, U, H, J, _lib.joint_workspace_bytes(T, U, B, J, geo.V)), (B, T, U, H, J)


def call(ops, scale, ws=None):
    """_fwd then _bwd through the C ABI -> dict of costs, the six gradients and the layer's arrays read back from the workspace
    (`ws`: a workspace to reuse; a fresh one is filled with 0xFF bytes)."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    L, (B, T, U, H, J) = _layout(ops)
    assert L["total"] == _lib.joint_net_workspace_bytes(T, U, B, H, J, geo.V)
    t = [torch.tensor(np.ascontiguousarray(x), device=dev) for x in ops]
    enc, pred, W1, b1, W2, b2, labels, il, ll = t
    sc = torch.tensor(np.asarray(scale, np.float32), device=dev)
    if ws is None:
        ws = torch.full((L["total"],), 0xFF, dtype=torch.uint8, device=dev)
    costs = torch.full((B,), float("nan"), device=dev)
    grads = [torch.full_like(x, float("nan")) for x in t[:6]]
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    head = [x.data_ptr() for x in (enc, pred, W1, b1, W2, b2, labels, ll, il)]
    _lib.check(lib.compute_rnnt_joint_net_loss_fwd(*head, H, J, geo.V, B, costs.data_ptr(), 0, ws.data_ptr(), opts), "joint_net_loss_fwd")
    _lib.check(lib.compute_rnnt_joint_net_loss_bwd(*head, sc.data_ptr(), H, J, geo.V, B, *(g.data_ptr() for g in grads), 0, ws.data_ptr(),
                                                   opts), "joint_net_loss_bwd")
    torch.cuda.synchronize()
    out = {"costs": costs.cpu().numpy(), "ws": ws, "L": L}
    out.update({k: g.cpu().numpy() for k, g in zip(KEYS, grads)})
    f32 = lambda key, n: ws[L[key]:L[key] + 4 * n].view(torch.float32).cpu().numpy()                     # noqa: E731
    f16 = lambda key, n: ws[L[key]:L[key] + 2 * n].view(torch.int16).cpu().numpy().view(np.float16)       # noqa: E731
    for key, rows in (("proj_e", L["R0"]), ("proj_p", L["R1"]), ("dproj_e", L["R0"]), ("dproj_p", L["R1"])):
        out[key] = f32(key, rows * J).reshape(rows, J)
    for key, shape in (("Xhi", (L["Rp"], H)), ("Xlo", (L["Rp"], H)), ("Dhi", (L["Rp"], J)), ("Dlo", (L["Rp"], J)), ("Whi", (H, J)),
                       ("Wlo", (H, J)), ("WThi", (J, H)), ("WTlo", (J, H))):
        out[key] = f16(key, shape[0] * shape[1]).reshape(shape)
    out["scal"] = f32("scal", 5)
    return out


def cost_scale(B):
    return (np.linspace(0.5, 1.5, B) / B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def run_case(name):
    ops = geo.operands(name)
    r = call(ops, cost_scale(ops[0].shape[0]))
    del r["ws"]
    return ops, r


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16 if x.dtype == np.float16 else np.uint32)


def check_images(ops, r):
    """scal[0..4] and the four image pairs are bitwise the emulation's; padding rows hold zeros, not what the workspace held."""
    enc, pred, W1 = ops[:3]
    L, H, J = r["L"], W1.shape[0], W1.shape[1]
    xh, xl, (Se, Sp) = geo.image(enc.reshape(-1, H), pred.reshape(-1, H), L)
    dh, dl, (Sde, Sdp) = geo.image(r["dproj_e"], r["dproj_p"], L)
    Sw = geo.scale_of(W1)
    wh, wl = geo.split(W1, Sw)
    assert np.array_equal(bits(r["scal"]), bits(np.array([Se, Sp, Sw, Sde, Sdp], np.float32))), (r["scal"], Se, Sp, Sw, Sde, Sdp)
    for key, want in (("Xhi", xh), ("Xlo", xl), ("Dhi", dh), ("Dlo", dl), ("Whi", wh), ("Wlo", wl), ("WThi", wh.T), ("WTlo", wl.T)):
        got = r[key]
        bad = np.argwhere(bits(got) != bits(want))
        assert not len(bad), (key, len(bad), bad[:4].tolist())
    pad = np.r_[L["R0"]:L["R0p"], L["R0p"] + L["R1"]:L["Rp"]]
    for key in ("Xhi", "Xlo", "Dhi", "Dlo"):
        assert not bits(r[key][pad]).any(), key


def check_products(tag, ops, r):
    """The five products against float64 of what they consumed, each within BAR x the emulation's own error."""
    enc, pred, W1, b1 = ops[:4]
    L, H = r["L"], W1.shape[0]
    B = enc.shape[0]
    e2, p2, de, dp = enc.reshape(-1, H), pred.reshape(-1, H), r["dproj_e"], r["dproj_p"]
    emu = dict(zip(("proj_e", "proj_p"), geo.emu_proj(e2, p2, W1, b1, L)))
    emu.update(zip(("d_enc", "d_pred"), geo.emu_dx(de, dp, W1, L)))
    emu["dW1"] = geo.emu_dw(e2, p2, de, dp, L)
    refs = {"proj_e": geo.ref_nt(e2, W1.T, b1), "proj_p": geo.ref_nt(p2, W1.T), "d_enc": geo.ref_nt(de, W1), "d_pred": geo.ref_nt(dp, W1),
            "dW1": geo.ref_dw(e2, p2, de, dp)}
    got = {k: r[k] for k in ("proj_e", "proj_p", "dW1")}
    got["d_enc"], got["d_pred"] = r["d_enc"].reshape(-1, H), r["d_pred"].reshape(-1, H)
    rows = {"d_enc_loud": ("d_enc", geo.loud_rows(de)), "d_pred_loud": ("d_pred", geo.loud_rows(dp))}
    rec, fails = {}, []
    for key in ("proj_e", "proj_p", "d_enc", "d_pred", "dW1", "d_enc_loud", "d_pred_loud"):
        src, mask = rows.get(key, (key, None))
        ref, den = refs[src]
        rho_gpu, rho_emu = geo.rho(got[src], ref, den, mask), geo.rho(emu[src], ref, den, mask)
        print(f"rho {tag} {key}: gpu {rho_gpu:.3e}  emu {rho_emu:.3e}  bar {geo.BAR * max(rho_emu, geo.EPS):.3e}"
              + (f"  ({int(mask.sum())} of {len(mask)} rows)" if mask is not None else ""))
        rec["rho_gpu_" + key], rec["rho_emu_" + key] = rho_gpu, rho_emu
        if not rho_gpu <= geo.BAR * max(rho_emu, geo.EPS):
            fails.append((key, rho_gpu, rho_emu))
    _record(tag, B=B, **rec)
    assert not fails, (tag, fails)


def test_restated_layout_has_the_librarys_size():
    for name in NAMES:
        B, T, U, H, J = geo.CASES[name]
        base = _lib.joint_workspace_bytes(T, U, B, J, geo.V)
        assert geo.layout(B, T, U, H, J, base)["total"] == _lib.joint_net_workspace_bytes(T, U, B, H, J, geo.V), name


@pytest.mark.parametrize("name", NAMES)
def test_scales_and_images_are_bitwise_the_split_of_the_f32_tensors(name):
    ops, r = run_case(name)
    assert np.isfinite(r["costs"]).all() and all(np.isfinite(r[k]).all() for k in KEYS)
    assert np.abs(r["dproj_e"]).max() > 0 and np.abs(r["dproj_p"]).max() > 0  # (a backward with something in it)
    check_images(ops, r)


@pytest.mark.parametrize("name", NAMES)
def test_five_products_against_float64_of_what_they_consumed(name):
    ops, r = run_case(name)
    check_products("case_" + name, ops, r)


@pytest.mark.parametrize("name", NAMES)
def test_db1_is_the_column_sum_of_dproj_e(name):
    """Worst case of the summation depth the code has: 16 rows per block in sequence, the blocks' partials in sequence per lane
    (db_blocks / 64 of them), then a six-level tree: (16 + db_blocks / 64 + 6) roundings of at most 2^-24 sum |x| each."""
    _, r = run_case(name)
    d = r["dproj_e"].astype(np.float64)
    err, room = np.abs(r["db1"] - d.sum(axis=0)), (22 + r["L"]["db_blocks"] / 64) * 2.0 ** -24 * np.abs(d).sum(axis=0)
    print(f"db1 {name}: max err / room {np.max(err / np.maximum(room, 1e-300)):.3f}  db_blocks {r['L']['db_blocks']}")
    _record("db1_" + name, worst_err_over_room=float(np.max(err / np.maximum(room, 1e-300))), db_blocks=r["L"]["db_blocks"])
    assert np.all(err <= room)


def test_padded_frames_and_label_positions_get_exact_zeros():
    ops, r = run_case("e")
    il, ll = ops[7], ops[8]
    assert (il < geo.CASES["e"][1]).any() and (ll + 1 < geo.CASES["e"][2]).any()  # ragged
    for b in range(len(il)):
        assert not r["d_enc"][b, il[b]:].any() and not r["d_pred"][b, ll[b] + 1:].any(), b
        assert r["d_enc"][b, :il[b]].any() and r["d_pred"][b, :ll[b] + 1].any(), b


def scaled(ops, k_enc=0, k_pred=0, k_w=0):
    out = list(ops)
    out[0], out[1], out[2] = np.ldexp(ops[0], k_enc), np.ldexp(ops[1], k_pred), np.ldexp(ops[2], k_w)
    return tuple(out)


@pytest.mark.parametrize("k", [40, -40])
def test_powers_of_two_move_through_the_gemms_exactly(k):
    """enc, pred x 2^k and W1 x 2^-k: the images are the same bits under other scales, so the projections are bit-identical and
    the three gradients are the k = 0 bits times the power of two."""
    ops, r0 = run_case("c")
    r = call(scaled(ops, k, k, -k), cost_scale(ops[0].shape[0]))
    for key in ("Xhi", "Xlo", "Whi", "Wlo", "WThi", "WTlo", "Dhi", "Dlo", "proj_e", "proj_p", "costs", "db1", "dW2", "db2"):
        assert np.array_equal(bits(r[key]), bits(r0[key])), key
    assert np.array_equal(r["scal"][:3], r0["scal"][:3] * np.float32(2.0) ** np.array([-k, -k, k], np.float32))
    for key, kk in (("d_enc", -k), ("d_pred", -k), ("dW1", k)):
        assert np.array_equal(bits(r[key]), bits(np.ldexp(r0[key], kk))), key


def test_every_tensor_carries_its_own_scale():
    """enc x 2^20, pred x 2^-20, W1 as it is: two segments of ONE image 2^40 apart."""
    ops = scaled(geo.operands("c"), 20, -20, 0)
    r = call(ops, cost_scale(ops[0].shape[0]))
    assert r["scal"][0] * 2.0 ** 40 == r["scal"][1]
    check_images(ops, r)
    check_products("case_c_enc_2p20_pred_2m20", ops, r)


def test_two_small_tensors_do_not_rescale_by_zero():
    """enc, pred and W1 all x 2^-50: uncapped, S_X S_W (about 2^62 2^66) overflows and pred_proj = acc / inf = 0, though the true
    product (about 2^-100) is a normal f32 number.  With the exponent of S held within +-63, W1 keeps 19 of its 22 bits here:
    the emulation knows, and the bar follows it."""
    ops = scaled(geo.operands("a"), -50, -50, -50)
    r = call(ops, cost_scale(ops[0].shape[0]))
    assert r["scal"][2] == 2.0 ** 63 and 2.0 ** 56 <= r["scal"][0] < 2.0 ** 63
    assert np.abs(r["proj_p"]).max() > 0
    check_images(ops, r)
    check_products("case_a_all_2m50", ops, r)


def test_no_scale_is_left_over_from_the_call_before():
    """Calls back to back on ONE workspace (no graph), the operands 2^10 larger and smaller from call to call: every result is
    bitwise what a fresh workspace gives (the scales are re-read with agent-scope loads: dense_max_of)."""
    ops = geo.operands("b")
    sc = cost_scale(ops[0].shape[0])
    ws = None
    for k in (0, 10, -10, 0):
        o, s = scaled(ops, k, k, -k), np.ldexp(sc, k)
        fresh = call(o, s)
        again = call(o, s, ws=ws)
        ws = again["ws"]
        for key in ("costs", "scal", "proj_e", "proj_p", "dproj_e", "dproj_p", "Xhi", "Xlo", "Dhi", "Dlo", "WThi", "WTlo") + KEYS:
            assert np.array_equal(bits(fresh[key]), bits(again[key])), (k, key)


def test_zero_cost_scale_gives_six_exact_zero_gradients():
    ops = geo.operands("a")
    r = call(ops, np.zeros(ops[0].shape[0], np.float32))
    assert np.isfinite(r["costs"]).all()
    for key in KEYS:
        assert not r[key].any(), key
    assert np.array_equal(r["scal"][3:5], np.ones(2, np.float32))  # an all-zero tensor: S = 1
    assert not bits(r["Dhi"]).any() and not bits(r["Dlo"]).any()


def test_a_vanishing_tensor_stays_finite():
    """pred = 1e-36 throughout (2^-120: below what S = 2^(14 - e) can scale up inside f32).  Everything stays finite, pred_proj
    stays within the product's own magnitude, and costs and gradients are those of the float64 network."""
    ops = list(geo.operands("b"))
    ops[1] = np.full_like(ops[1], 1e-36)
    B, H = ops[0].shape[0], ops[2].shape[0]
    sc = cost_scale(B)
    r = call(tuple(ops), sc)
    print(f"vanishing pred: scal {r['scal']}  max|proj_p| {np.abs(r['proj_p']).max():.3e}  costs {r['costs']}")
    for key in ("costs", "proj_e", "proj_p", "dproj_e", "dproj_p", "scal") + KEYS:
        assert np.isfinite(r[key]).all(), key
    assert np.abs(r["proj_p"]).max() <= H * 1e-36 * np.abs(ops[2]).max() * (1 + 2.0 ** -10)
    check_images(tuple(ops), r)
    ref = orc.joint_loss_and_grads(*ops, cost_scale=sc.astype(np.float64))
    assert np.all(np.abs(r["costs"] - ref["costs"]) <= TOL * np.maximum(1.0, np.abs(ref["costs"])))
    for key in KEYS:
        err = np.abs(r[key] - ref[key]).max()
        assert err <= TOL * max(1.0, np.abs(ref[key]).max()), (key, err)


def test_an_enc_pointer_off_the_16_byte_grid_is_refused():
    dev = torch.device("cuda:0")
    lib = _lib.load()
    ops = geo.operands("a")
    L, (B, T, U, H, J) = _layout(ops)
    t = [torch.tensor(x, device=dev) for x in ops]
    flat = torch.zeros(B * T * H + 1, device=dev)
    off = flat[1:]
    off.copy_(t[0].reshape(-1))
    assert flat.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    ws = torch.full((L["total"],), 0xFF, dtype=torch.uint8, device=dev)
    costs = torch.zeros(B, device=dev)
    opts = _lib.make_options(torch.cuda.current_stream().cuda_stream, 0, T, U)
    ptrs = [x.data_ptr() for x in (off, *t[1:6], t[6], t[8], t[7])]
    assert lib.compute_rnnt_joint_net_loss_fwd(*ptrs, H, J, geo.V, B, costs.data_ptr(), 0, ws.data_ptr(), opts) != 0
    ptrs[0] = t[0].data_ptr()
    assert lib.compute_rnnt_joint_net_loss_fwd(*ptrs, H, J, geo.V, B, costs.data_ptr(), 0, ws.data_ptr(), opts) == 0
    torch.cuda.synchronize()
