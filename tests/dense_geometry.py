"""The joint's first Dense layer (csrc/dense_kernels.hip), restated in plain Python: where its arrays lie in the workspace, which
tiles, K chunks and K splits a shape launches, and the split-precision arithmetic its header states, emulated in NumPy.

The restatement (constants copied from the .hip file; tests/test_dense_geometry.py compares the copies with the source) only says
WHERE things are and WHICH corner of the launch geometry a shape reaches, so that a retuned tile cannot silently move the GPU cases
of tests/test_dense_geometry_gpu.py off the corner they are named for.  The emulation says what rounding the documented scheme
allows: it yields the bar of the GPU tests (a multiple of ITS error against float64) and three faulty variants that the bar must
tell from it.  Neither is ever the numerical reference: that is the float64 product of the f32 operands."""
import numpy as np

# ---- constants (name in the source -> value)
DK = {"kDenseScaleLog2": 14, "kDenseScaleCapLog2": 63, "kAbsBlocks": 512, "kDbRows": 16, "kNtM": 256, "kNtN": 128, "kNtK": 32,
      "kNtStages": 3, "kTnT": 128, "kTnK": 16, "kTnStages": 3}
COMMON = {"kHookBlocks": 1024}
SOURCES = {"dense_kernels.hip": DK, "rnnt_common.h": COMMON}
SLOTS = {"Xe": 0, "Xp": 1, "W": 2, "De": 3, "Dp": 4}  # scal[slot] = S
V = 28


def _up(n, a):
    return (n + a - 1) // a * a


# ---- make_dense_layout
def layout(B, T, U, H, J, base):
    """-> dict of R0, R0p, R1, Rp, nsplit, ns0, db_blocks, c_all, c0, the byte offset of every array, and `total`."""
    tk, tt = DK["kTnK"], DK["kTnT"]
    L = dict(R0=B * T, R1=B * U)
    L["R0p"] = _up(L["R0"], tk)
    L["Rp"] = L["R0p"] + _up(L["R1"], tk)
    tiles = ((H + tt - 1) // tt) * ((J + tt - 1) // tt)
    c_all, c0 = L["Rp"] // tk, L["R0p"] // tk
    ns = (3 * 256 + tiles - 1) // tiles
    ns = min(ns, c_all // 8)
    ns = max(ns, 2)
    ns = min(ns, 64)
    ns0 = min(max(ns * c0 // c_all, 1), ns - 1)
    L.update(nsplit=ns, ns0=ns0, c_all=c_all, c0=c0, db_blocks=(L["R0"] + DK["kDbRows"] - 1) // DK["kDbRows"])
    off = base
    for name, nbytes in (("proj_e", L["R0"] * J * 4), ("proj_p", L["R1"] * J * 4), ("dproj_e", L["R0"] * J * 4), ("dproj_p", L["R1"] * J * 4),
                         ("Xhi", L["Rp"] * H * 2), ("Xlo", L["Rp"] * H * 2), ("Dhi", L["Rp"] * J * 2), ("Dlo", L["Rp"] * J * 2),
                         ("Whi", H * J * 2), ("Wlo", H * J * 2), ("WThi", H * J * 2), ("WTlo", H * J * 2),
                         ("dWpart", ns * H * J * 4), ("dbpart", L["db_blocks"] * J * 4),
                         ("scal", 256 + (3 * DK["kAbsBlocks"] + 2 * COMMON["kHookBlocks"]) * 4)):
        L[name] = off
        off = _up(off + nbytes, 256)
    L["total"] = off
    return L


# ---- the launches
def nt_launch(M, N, K):
    """dense_gemm_nt_kernel: (M tiles, N tiles, K chunks of the ring)."""
    return (M + DK["kNtM"] - 1) // DK["kNtM"], (N + DK["kNtN"] - 1) // DK["kNtN"], K // DK["kNtK"]


def tn_launch(H, J, L):
    """dense_gemm_tn_kernel: (M tiles, N tiles, workgroups)."""
    tm, tn = (H + DK["kTnT"] - 1) // DK["kTnT"], (J + DK["kTnT"] - 1) // DK["kTnT"]
    return tm, tn, tm * tn * L["nsplit"]


def tn_ranges(L):
    """The chunk range [c_lo, c_hi) of every K split: splits [0, ns0) share the enc chunks, the rest the pred chunks."""
    out = []
    for split in range(L["nsplit"]):
        first = split < L["ns0"]
        rs, rn = (split, L["ns0"]) if first else (split - L["ns0"], L["nsplit"] - L["ns0"])
        rc0, rcn = (0, L["c0"]) if first else (L["c0"], L["c_all"] - L["c0"])
        out.append((rc0 + rcn * rs // rn, rc0 + rcn * (rs + 1) // rn))
    return out


def xcd_remap(bid, nwg):
    xcd, idx, q, r = bid & 7, bid >> 3, nwg >> 3, nwg & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def launches(B, T, U, H, J):
    """Every GEMM launch of one forward + backward call: name -> dict(grid, chunks, ...)."""
    L = layout(B, T, U, H, J, 0)
    M = L["R0p"] + L["R1"]
    fm, fn, fk = nt_launch(M, J, H)
    bm, bn, bk = nt_launch(M, H, J)
    tm, tn, tg = tn_launch(H, J, L)
    return {"proj": dict(grid=fm * fn, tiles_m=fm, tiles_n=fn, chunks=fk, M=M, N=J),
            "dX": dict(grid=bm * bn, tiles_m=bm, tiles_n=bn, chunks=bk, M=M, N=H),
            "dW1": dict(grid=tg, tiles_m=tm, tiles_n=tn, ranges=tn_ranges(L))}


# ---- the arithmetic of the header, emulated
VARIANTS = ("faithful", "no_lo_hi", "no_hi_lo", "hi_hi_only")  # the three MFMA terms: hi.hi, (A lo).(B hi), (A hi).(B lo)
_TERMS = {"faithful": (0, 1, 2), "no_lo_hi": (0, 2), "no_hi_lo": (0, 1), "hi_hi_only": (0,)}


def scale_of(x):
    """S = 2^(14 - e) with max|x| < 2^e, its exponent kept within +-kDenseScaleCapLog2; 1 for an all-zero or non-finite tensor."""
    m = np.float32(np.max(np.abs(x))) if np.size(x) else np.float32(0)
    if not (m > 0) or not (m < np.float32(3.0e38)):
        return np.float32(1.0)
    e = int(np.frexp(np.float64(m))[1])  # m = f 2^e, f in [0.5, 1): e = ilogb(m) + 1, denormals included
    cap = DK["kDenseScaleCapLog2"]
    return np.float32(np.ldexp(1.0, int(np.clip(DK["kDenseScaleLog2"] - e, -cap, cap))))


def split(x, S):
    """hi = f16(S x), lo = f16(S x - hi), every step in f32 as the kernel does it."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sx = (np.asarray(x, np.float32) * np.float32(S)).astype(np.float32)
        hi = sx.astype(np.float16)
        lo = (sx - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def image(seg0, seg1, L):
    """The hi / lo image pair of two row segments as the prepare kernel leaves it: seg0 at rows [0, R0), seg1 at [R0p, R0p + R1),
    zero rows elsewhere; each segment with its own scale -> hi, lo [Rp, cols], (S0, S1)."""
    cols = seg0.shape[1]
    hi, lo = np.zeros((L["Rp"], cols), np.float16), np.zeros((L["Rp"], cols), np.float16)
    S0, S1 = scale_of(seg0), scale_of(seg1)
    hi[:L["R0"]], lo[:L["R0"]] = split(seg0, S0)
    hi[L["R0p"]:L["R0p"] + L["R1"]], lo[L["R0p"]:L["R0p"] + L["R1"]] = split(seg1, S1)
    return hi, lo, (S0, S1)


def _mma(acc, ah, al, bh, bl, variant):
    """One 16-deep k-step on a [M, 16] and a [N, 16] fragment: the products are exact, each term's sum is rounded into f32."""
    pairs = ((ah, bh), (al, bh), (ah, bl))
    for t in _TERMS[variant]:
        a, b = pairs[t]
        acc = (acc.astype(np.float64) + a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    return acc


def gemm_nt(Ahi, Alo, Bhi, Blo, variant="faithful"):
    """acc[m][n] = sum_k A[m][k] B[n][k], unscaled (f32)."""
    acc = np.zeros((Ahi.shape[0], Bhi.shape[0]), np.float32)
    for k in range(0, Ahi.shape[1], 16):
        acc = _mma(acc, Ahi[:, k:k + 16], Alo[:, k:k + 16], Bhi[:, k:k + 16], Blo[:, k:k + 16], variant)
    return acc


def _inv(Sa, Sb):
    return np.float32(1.0) / (np.float32(Sa) * np.float32(Sb))


def _rescale(acc, inv, bias=None):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        v = acc.astype(np.float64) * np.float64(inv)  # exact: a power of two
        if bias is not None:
            v = v + bias.astype(np.float64)           # one rounding, as the kernel's fmaf
        return v.astype(np.float32)


def emu_proj(enc, pred, W1, b1, L, variant="faithful"):
    """proj_e = enc . W1 + b1, proj_p = pred . W1 (enc [R0, H], pred [R1, H])."""
    xh, xl, (Se, Sp) = image(enc, pred, L)
    Sw = scale_of(W1)
    wh, wl = split(W1, Sw)
    M = L["R0p"] + L["R1"]
    acc = gemm_nt(xh[:M], xl[:M], wh.T, wl.T, variant)
    return _rescale(acc[:L["R0"]], _inv(Se, Sw), b1), _rescale(acc[L["R0p"]:M], _inv(Sp, Sw))


def emu_dx(de, dp, W1, L, variant="faithful"):
    """d_enc = dproj_e . W1^T, d_pred = dproj_p . W1^T."""
    dh, dl, (Se, Sp) = image(de, dp, L)
    Sw = scale_of(W1)
    wh, wl = split(W1, Sw)
    M = L["R0p"] + L["R1"]
    acc = gemm_nt(dh[:M], dl[:M], wh, wl, variant)
    return _rescale(acc[:L["R0"]], _inv(Se, Sw)), _rescale(acc[L["R0p"]:M], _inv(Sp, Sw))


def emu_dw(enc, pred, de, dp, L, variant="faithful"):
    """dW1 = enc^T . dproj_e + pred^T . dproj_p: one f32 partial per K split (chunks of 16 rows), the partials summed as
    dense_reduce_body<4> sums them (lane g takes partials g, g + 4, ... in order; then (0 + 2) + (1 + 3))."""
    xh, xl, (Sxe, Sxp) = image(enc, pred, L)
    dh, dl, (Sde, Sdp) = image(de, dp, L)
    parts = []
    for split_i, (c_lo, c_hi) in enumerate(tn_ranges(L)):
        acc = np.zeros((enc.shape[1], de.shape[1]), np.float32)
        for c in range(c_lo, c_hi):
            r = slice(16 * c, 16 * c + 16)
            acc = _mma(acc, xh[r].T, xl[r].T, dh[r].T, dl[r].T, variant)
        parts.append(_rescale(acc, _inv(Sxe, Sde) if split_i < L["ns0"] else _inv(Sxp, Sdp)))
    lanes = []
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for g in range(4):
            s = np.zeros_like(parts[0])
            for q in range(g, len(parts), 4):
                s = s + parts[q]
            lanes.append(s)
        return (lanes[0] + lanes[2]) + (lanes[1] + lanes[3])


# ---- the float64 reference and the error measure
def ref_nt(A, Bm, bias=None):
    """float64 A . Bm^T (+ bias) of the f32 operands, and sum_k |a||b| (+ |bias|)."""
    A, Bm = A.astype(np.float64), Bm.astype(np.float64)
    ref, den = A @ Bm.T, np.abs(A) @ np.abs(Bm).T
    if bias is not None:
        ref, den = ref + bias.astype(np.float64), den + np.abs(bias.astype(np.float64))
    return ref, den


def ref_dw(enc, pred, de, dp):
    e, p, a, b = (x.astype(np.float64) for x in (enc, pred, de, dp))
    return e.T @ a + p.T @ b, np.abs(e).T @ np.abs(a) + np.abs(p).T @ np.abs(b)


def rho(C, ref, den, rows=None):
    """max |C - ref| / sum_k |a||b|; an element whose sum is zero must be exactly zero.  `rows`: a mask, to look at some rows only."""
    C = np.asarray(C, np.float64)
    assert C.shape == ref.shape
    assert np.all(np.isfinite(C)), "non-finite output"
    dead = den == 0
    assert not C[dead].any(), "an element with no non-zero product is not exactly zero"
    r = np.zeros_like(ref)
    np.divide(np.abs(C - ref), den, out=r, where=~dead)
    if rows is not None:
        r = r[rows]
    return float(r.max()) if r.size else 0.0


def loud_rows(x, log2=8):
    """Rows whose largest magnitude is within 2^-log2 of the tensor's: they keep all 22 bits of the per-tensor split (hi + lo are
    full binary16 numbers while S |x| >= 2^-2), so on them a lost lo fragment shows at full size whatever the other rows hold."""
    m = np.abs(x).max(axis=1)
    return m >= np.ldexp(m.max(), -log2) if m.max() > 0 else np.zeros(len(x), bool)


BAR = 8.0         # GPU: rho_gpu <= BAR * max(rho_emu, EPS)  (the emulation fixes ONE accumulation order inside a k-step)
SEPARATION = 32.0  # CPU: every faulty variant has rho >= SEPARATION * max(rho_emu, EPS)
EPS = 2.0 ** -24


# ---- the cases (B, T, U, H, J), V = 28: the smallest shapes that reach each corner (tests/test_dense_geometry.py asserts them)
CASES = {
    "a": (1, 15, 2, 32, 64),      # one K chunk (ring prologue only), one 16-row chunk per segment, every tile overhangs, 14 of 16 pred rows padding
    "b": (1, 16, 16, 64, 128),    # R0 % 16 == 0 (no padding between the segments), two K chunks, an exact 128-column N tile
    "c": (3, 85, 7, 96, 192),     # R0 = 255, R0p = 256: the pred segment starts on a workgroup tile boundary; N overhangs by half a tile; three K chunks
    "d": (1, 257, 3, 160, 320),   # R0 = 257, R0p = 272: the second tile holds ONE enc row, the 15 padding rows and the pred rows; TN M tile with 32 live columns
    "e": (8, 80, 20, 320, 320),   # 4 x 3 = 12 NT workgroups (remap quotient 1, remainder 4), nsplit = 6, ns0 = 4; ragged
    "f": (2, 30, 12, 1024, 64),   # 32 K chunks forward; dX with N = 1024 (8 N tiles); 8 TN M tiles
    "g": (2, 9, 5, 32, 640),      # dX with K = 640 and N = 32, narrower than one wave's 64 columns
}


def operands(name, seed=None):
    """enc, pred, W1, b1, W2, b2, labels, input lengths, label lengths of a case: N(0,1) activations, Xavier weights; lengths between
    half and full (the first utterance full)."""
    B, T, U, H, J = CASES[name]
    rng = np.random.default_rng(1000 + sorted(CASES).index(name) if seed is None else seed)
    enc = rng.normal(size=(B, T, H)).astype(np.float32)
    pred = rng.normal(size=(B, U, H)).astype(np.float32)
    W1 = (rng.uniform(-1, 1, size=(H, J)) * np.sqrt(6.0 / (H + J))).astype(np.float32)
    b1 = (0.1 * rng.normal(size=J)).astype(np.float32)
    W2 = (rng.uniform(-1, 1, size=(J, V)) * np.sqrt(6.0 / (J + V)) * 2.0).astype(np.float32)
    b2 = (0.1 * rng.normal(size=V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U - 1)).astype(np.int32)
    il = rng.integers((T + 1) // 2, T + 1, size=B).astype(np.int32)
    ll = rng.integers((U - 1) // 2, U, size=B).astype(np.int32)
    il[0], ll[0] = T, U - 1
    return enc, pred, W1, b1, W2, b2, labels, il, ll


def dproj_standin(rows, J, seed):
    """What the fused joint hands back, in caricature: row magnitudes spread over 2^-30 .. 1, about half the rows exactly zero
    (padded frames, dead lattice rows); the first row loud, the second zero, whatever the draw."""
    rng = np.random.default_rng(seed)
    mag = np.ldexp(1.0, -rng.integers(0, 31, size=rows))
    mag[rng.random(rows) < 0.5] = 0.0
    mag[0] = 1.0
    if rows > 1:
        mag[1] = 0.0
    return (rng.normal(size=(rows, J)) * mag[:, None]).astype(np.float32)
