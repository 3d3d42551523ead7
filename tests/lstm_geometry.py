"""The launch geometry of the three LSTM engines, restated in plain Python, and the shapes that reach each corner of it.

csrc/lstm_train_kernels.hip, csrc/encoder_kernels.hip and csrc/prednet_kernels.hip share one recurrent GEMM body: TR rows by 32
(or 64) columns per workgroup, K split into fixed groups, weights packed k-major with zero padding.  TR comes from
lt_rows_per_wg / en_rows_per_wg / pn_rows_per_wg, the encoder's input GEMM runs in windows of window_of frames.  This file
restates those rules (constants copied from the .hip files; tests/test_lstm_geometry.py compares the copies with the sources)
and holds the case table of tests/test_lstm_geometry_gpu.py.  The restatement only says WHICH geometry a shape reaches, so
that a retuned constant cannot silently move the GPU cases off the geometry they are named for; it is never a numerical
reference."""

# ---- constants (name in the .hip file -> value), per source file
LT = {"kLtMaxRows": 1024, "kLtLds": 150 * 1024, "kLtMaxTr": 16, "kLtFewWgs": 256}
EN = {"kEnMaxRows": 1024, "kEnLds": 150 * 1024, "kEnPreBytes": 64 << 20, "kEnGatesKg": 32, "kEnProjKg": 64, "kEnMaxTr": 16}
PN = {"kPnMaxRows": 1024, "kPnLds": 150 * 1024, "kPnGatesWaves": 8, "kPnDenseWaves": 16, "kPnGatesRows": 16, "kPnDenseRows": 4}
SOURCES = {"lstm_train_kernels.hip": LT, "encoder_kernels.hip": EN, "prednet_kernels.hip": PN}


def r4(n):
    return (n + 3) // 4 * 4


def r8(n):
    return (n + 7) // 8 * 8


def r32(n):
    return (n + 31) // 32 * 32


def a64(n):
    return (n + 63) // 64 * 64


def _clamp(max_tr, per_row_floats, lds, R):
    """The two loops every rule starts with -> (tr after the LDS clamp, tr after the row clamp)."""
    tr = max_tr
    while tr > 1 and tr * per_row_floats * 4 > lds:
        tr >>= 1
    lds_tr = tr
    while tr > 1 and tr // 2 >= R:
        tr >>= 1
    return lds_tr, tr


# ---- the training layer
def lt_kgroups(Kpad):
    return 64 if Kpad > 512 else 32


def lt_rows_per_wg(Kpad, NKG, R, col_tiles):
    """-> (TR, TR after the LDS clamp alone)."""
    lds_tr, tr = _clamp(LT["kLtMaxTr"], Kpad + NKG * 32, LT["kLtLds"], R)
    while tr > 1 and col_tiles * ((R + tr - 1) // tr) < LT["kLtFewWgs"]:
        tr >>= 1
    return tr, lds_tr


def lt_roles(H, P, R):
    """role -> dict(Kpad, NKG, col_tiles, TR, lds_tr) for one layer (projected when P < H)."""
    proj = P < H
    Hp, Kp, Kh, ldp, ldh = r8(H), r4(P), r4(H), r32(P), r32(H)
    launches = {"FWD_GATES": (Kp, 4 * Hp)}
    if proj:
        launches["FWD_PROJ"] = (Kh, ldp)
        launches["BWD_DR"] = (4 * H, ldp)
        launches["BWD_CELL"] = (Kp, ldh)
    else:
        launches["BWD_CELL"] = (4 * H, ldp)
    out = {}
    for role, (Kpad, ld) in launches.items():
        NKG = lt_kgroups(Kpad)
        tr, lds_tr = lt_rows_per_wg(Kpad, NKG, R, ld // 32)
        out[role] = dict(Kpad=Kpad, NKG=NKG, col_tiles=ld // 32, TR=tr, lds_tr=lds_tr)
    return out


def lt_images(H, P, R):
    """The packed weight images of one call's workspace (make_lt_layout): name -> (offset in floats, Kpad, ld), and the
    workspace size in bytes.  The forward call writes whh_f / whr_f, the backward call whh_b / whr_b."""
    proj = P < H
    Hp, Kp, Kh, ldp, ldh = r8(H), r4(P), r4(H), r32(P), r32(H)
    out, off = {}, 0
    for name, Kpad, ld, there in (("whh_f", Kp, 4 * Hp, True), ("whr_f", Kh, ldp, proj), ("whh_b", 4 * H, ldp, True),
                                  ("whr_b", Kp, ldh, proj)):
        if there:
            out[name] = (off, Kpad, ld)
            off += a64(Kpad * ld)
    off += a64(R * H)  # the carry
    return out, (off * 4 + 255) // 256 * 256


# ---- the encoder
def en_images(feat, H, P, L, ridx, f, R, Tmax):
    """The packed images of the encoder's workspace (make_en_layout): per block {"wi" / "wh" / "b" / "wr": (offset in floats,
    Kpad, ld)}, and the workspace size in bytes."""
    F, proj = feat[0] * feat[1], P < H
    In = en_inputs(feat, P, L, ridx, f)
    Hp, off = r8(H), L * (a64(R * P) + a64(R * H))  # the state comes first
    xn, yn, pren = Tmax * F, 0, 0
    for l in range(L):
        Tl = (Tmax + f - 1) // f if l > ridx else Tmax
        xn, yn = max(xn, Tl * In[l]), max(yn, Tl * P)
        pren = max(pren, window_of(R, H, Tl) * R * 4 * Hp)
    off += a64(R * H if proj else 0) + a64(xn * R) + a64(yn * R) + a64(pren) + 3 * a64(F)
    out = []
    for l in range(L):
        ng, blk = 4 * Hp, {}
        blk["wi"] = (off, r4(In[l]), ng)
        off += a64(r4(In[l]) * ng)
        blk["wh"] = (off, r4(P), ng)
        off += a64(r4(P) * ng)
        blk["b"] = (off, 1, ng)
        off += a64(ng)
        if proj:
            blk["wr"] = (off, r4(H), a64(P))
            off += r4(H) * a64(P)
        off += 2 * a64(P)
        out.append(blk)
    return out, off * 4


def en_rows_per_wg(Kpad, NKG, R):
    lds_tr, tr = _clamp(EN["kEnMaxTr"], Kpad + NKG * 32, EN["kEnLds"], R)
    return tr, lds_tr


def window_of(R, H, Tl):
    per = R * 4 * r8(H) * 4
    return min(max(EN["kEnPreBytes"] // per, 1), Tl)


def en_inputs(feat, P, L, ridx, f):
    """The input width of every block."""
    return [feat[0] * feat[1] if l == 0 else (f * P if l == ridx + 1 else P) for l in range(L)]


def en_windows(R, H, L, ridx, f, T):
    """Per block, the frames of each input-GEMM window of one run of T frames."""
    out = []
    for l in range(L):
        Tl = (T + f - 1) // f if l > ridx else T
        Wn = window_of(R, H, Tl)
        out.append([min(Wn, Tl - t0) for t0 in range(0, Tl, Wn)])
    return out


def en_roles(H, P, R):
    launches = {"EN_GATES": (r4(P), EN["kEnGatesKg"])}
    if P < H:
        launches["EN_PROJ"] = (r4(H), EN["kEnProjKg"])
    out = {}
    for role, (Kpad, NKG) in launches.items():
        tr, lds_tr = en_rows_per_wg(Kpad, NKG, R)
        out[role] = dict(Kpad=Kpad, NKG=NKG, TR=tr, lds_tr=lds_tr)
    return out


# ---- the prediction step
def pn_rows_per_wg(Kpad, NW, R, max_tr):
    lds_tr, tr = _clamp(max_tr, Kpad + NW * 64, PN["kPnLds"], R)
    return tr, lds_tr


def pn_roles(E, H, P, L, R):
    out = {}
    for l in range(L):
        launches = {f"PN_GATES{l}": (r4((E if l == 0 else P) + P), PN["kPnGatesWaves"], PN["kPnGatesRows"])}
        if P < H:
            launches[f"PN_PROJ{l}"] = (r4(H), PN["kPnDenseWaves"], PN["kPnDenseRows"])
        if l == L - 1:
            launches["PN_OUT"] = (r4(P), PN["kPnDenseWaves"], PN["kPnDenseRows"])
        for role, (Kpad, NW, max_tr) in launches.items():
            tr, lds_tr = pn_rows_per_wg(Kpad, NW, R, max_tr)
            out[role] = dict(Kpad=Kpad, NKG=NW, TR=tr, lds_tr=lds_tr)
    return out


# ---- the cases.  `claim` is what the case is named for (tests/test_lstm_geometry.py asserts it for every R and role):
#   "partial"  every role has TR > 1 and a partial last row tile (R % TR != 0), or TR bound by the LDS clamp
#   "lds"      the named role's TR is bound by the LDS clamp (below the maximum, and below what R alone would give)
#   "windows"  at least 3 input-GEMM windows with a short last one in the first block
#   "short"    fewer frames than any other test runs on the device (training: T = 1, 2; encoder: T < f)
#   "max_rows" R at the limit
TRAIN = {
    "ragged_proj": dict(I=13, H=203, P=70, T=5, rows=(301,), claim="partial"),
    "ragged_unproj": dict(I=13, H=203, P=203, T=5, rows=(301,), claim="partial"),
    "short_proj_T1": dict(I=13, H=203, P=70, T=1, rows=(5,), claim="short"),
    "short_proj_T2": dict(I=13, H=203, P=70, T=2, rows=(5,), claim="short"),
    "short_unproj_T1": dict(I=13, H=203, P=203, T=1, rows=(5,), claim="short"),
    "short_unproj_T2": dict(I=13, H=203, P=203, T=2, rows=(5,), claim="short"),
    "max_rows": dict(I=6, H=40, P=12, T=3, rows=(1024,), claim="max_rows"),
}
TRAIN_ROWS = (0, 15, 16, 299, 300)  # of R = 301: both ends of the first row tiles, and the partial last tile of every role

ENCODER = {
    "ragged": dict(feat=(7, 1), H=203, P=70, L=3, ridx=1, f=3, T=11, rows=(5, 37), claim="partial"),
    "ragged_unproj": dict(feat=(7, 1), H=203, P=203, L=2, ridx=0, f=2, T=9, rows=(3, 21), claim="partial"),
    "lds_tile": dict(feat=(12, 1), H=512, P=128, L=2, ridx=0, f=2, T=6, rows=(24,), claim="lds", role="EN_PROJ"),
    "windows": dict(feat=(4, 3), H=256, P=128, L=3, ridx=1, f=2, T=37, rows=(1024,), claim="windows"),
    "short_T1": dict(feat=(7, 1), H=203, P=70, L=3, ridx=1, f=3, T=1, rows=(5,), claim="short"),
    "short_T2": dict(feat=(7, 1), H=203, P=70, L=3, ridx=1, f=3, T=2, rows=(5,), claim="short"),
}
WINDOW_ROWS = (0, 15, 16, 511, 1023)  # of the "windows" case, restated in float64

PREDNET = {
    "ragged_proj": dict(E=37, H=203, P=70, L=2, J=700, rows=(5, 37), claim="partial"),
    "ragged_unproj": dict(E=30, H=203, P=203, L=2, J=640, rows=(5, 37), claim="partial"),
}


def encoder_args(c):
    return c["feat"], c["H"], c["P"], c["L"], c["ridx"], c["f"]


def prednet_args(c):
    return c["E"], c["H"], c["P"], c["L"], c["J"]
