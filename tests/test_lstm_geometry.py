"""tests/lstm_geometry.py against the sources and against its own case table (no GPU): the copied constants equal the ones in
the .hip files, and every case of tests/test_lstm_geometry_gpu.py reaches the launch geometry it is named for.  A retuned
kLtFewWgs, kEnPreBytes or LDS budget fails here instead of silently moving the GPU cases onto tiles that are already covered."""
import os
import re

import pytest

from tests import lstm_geometry as geo

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnnt-speech-recognition_amd", "csrc")


def _constant(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*([^,;]+)[,;]", text)
    assert m, name
    expr = re.sub(r"\(size_t\)", "", m.group(1))
    assert re.fullmatch(r"[\d\s*<()]+", expr), (name, expr)
    return eval(expr)  # digits, *, << and parentheses only


@pytest.mark.parametrize("source", sorted(geo.SOURCES))
def test_copied_constants_equal_the_sources(source):
    with open(os.path.join(CSRC, source)) as fh:
        text = fh.read()
    for name, value in geo.SOURCES[source].items():
        assert _constant(text, name) == value, (source, name)
    if source == "lstm_train_kernels.hip":  # the k-group rule is one line
        assert "return Kpad > 512 ? 64 : 32;" in text


def _show(engine, name, R, roles, extra=""):
    for role, g in roles.items():
        print(f"geometry {engine} {name} R={R} {role}: Kpad={g['Kpad']} NKG={g['NKG']} TR={g['TR']} lds_TR={g['lds_tr']} "
              f"last_tile={R % g['TR'] or g['TR']}{extra}")


def _partial(g, R):
    return g["TR"] > 1 and R % g["TR"] != 0


def _lds_bound(g, max_tr):
    return g["TR"] == g["lds_tr"] < max_tr


def _assert_claim(engine, name, c, R, roles, max_tr):
    if c["claim"] == "partial":
        for role, g in roles.items():
            top = max_tr if isinstance(max_tr, int) else max_tr(role)
            assert _partial(g, R) or _lds_bound(g, top), (engine, name, R, role, g)
    elif c["claim"] == "lds":
        g = roles[c["role"]]
        assert _lds_bound(g, max_tr) and R >= g["TR"], (engine, name, R, g)
        assert any(_partial(v, R) for v in roles.values()), (engine, name, R)  # and a partial tile in another role
    elif c["claim"] == "max_rows":
        assert R == 1024


@pytest.mark.parametrize("name", sorted(geo.TRAIN))
def test_training_cases_reach_their_geometry(name):
    c = geo.TRAIN[name]
    H, P, T = c["H"], c["P"], c["T"]
    for R in c["rows"]:
        roles = geo.lt_roles(H, P, R)
        _show("lstm_train", name, R, roles, f" col_tiles={[g['col_tiles'] for g in roles.values()]}")
        _assert_claim("lstm_train", name, c, R, roles, geo.LT["kLtMaxTr"])
        if c["claim"] == "short":
            assert T in (1, 2)
    # real padding in every packed image: dead units in the last gate tile, padded k rows, padded columns
    if name.startswith("ragged"):
        assert H % 8 and P % 4 and H % 4 and P % 32 and H % 32
        R = c["rows"][0]
        # frames of y / dy / dr, and of c / h, that are not 16-byte aligned (a frame of gates is 16 R H bytes: always aligned)
        assert (R * P * 4) % 16 and (R * H * 4) % 16
        for r in geo.TRAIN_ROWS:
            assert r < R
        trs = {g["TR"] for g in geo.lt_roles(H, P, R).values()}
        for tr in trs:  # rows 299, 300 sit in the partial last tile of every role
            assert 300 // tr == (R - 1) // tr and R % tr
    if name == "ragged_proj":
        g = geo.lt_roles(H, P, 301)
        assert (g["FWD_GATES"]["TR"], g["FWD_GATES"]["col_tiles"]) == (16, 26)
        assert g["FWD_PROJ"]["TR"] == 2
        assert (g["BWD_DR"]["NKG"], g["BWD_DR"]["lds_tr"], g["BWD_DR"]["TR"]) == (64, 8, 2)
        assert g["BWD_CELL"]["TR"] == 8
    if name == "ragged_unproj":
        g = geo.lt_roles(H, P, 301)
        assert g["FWD_GATES"]["TR"] == 16
        assert (g["BWD_CELL"]["Kpad"], g["BWD_CELL"]["NKG"], g["BWD_CELL"]["lds_tr"], g["BWD_CELL"]["TR"]) == (812, 64, 8, 8)


@pytest.mark.parametrize("name", sorted(geo.ENCODER))
def test_encoder_cases_reach_their_geometry(name):
    c = geo.ENCODER[name]
    H, P, L, ridx, f, T = c["H"], c["P"], c["L"], c["ridx"], c["f"], c["T"]
    for R in c["rows"]:
        roles = geo.en_roles(H, P, R)
        wins = geo.en_windows(R, H, L, ridx, f, T)
        _show("encoder", name, R, roles, f" windows={wins}")
        _assert_claim("encoder", name, c, R, roles, geo.EN["kEnMaxTr"])
        if c["claim"] == "windows":
            w = wins[0]
            assert len(w) >= 3 and w[-1] < w[0], wins
            assert all(len(x) >= 2 for x in wins), wins
        else:
            assert all(len(x) == 1 for x in wins), wins
        if c["claim"] == "short":
            assert T < f and all(_partial(g, R) for g in roles.values())
    if name.startswith("ragged"):
        assert H % 8 and P % 4
        assert geo.en_inputs(c["feat"], P, L, ridx, f)[ridx + 1] % 4  # the stacked input after the time reduction
    if name == "ragged":
        assert geo.r4(geo.en_inputs(c["feat"], P, L, ridx, f)[2]) == 212
        assert geo.en_roles(H, P, 5)["EN_GATES"]["TR"] == 8 and geo.en_roles(H, P, 37)["EN_GATES"]["TR"] == 16 and 37 % 16 == 5
    if name == "lds_tile":
        g = geo.en_roles(H, P, 24)
        assert g["EN_PROJ"]["TR"] == 8 and g["EN_GATES"]["TR"] == 16 and 24 % 16 == 8
    if name == "windows":
        assert geo.en_windows(1024, H, L, ridx, f, T) == [[16, 16, 5], [16, 16, 5], [16, 3]]
        assert all(len(x) == 1 for x in geo.en_windows(16, H, L, ridx, f, T))  # the R = 16 runs it is compared with
        assert max(geo.WINDOW_ROWS) < 1024


@pytest.mark.parametrize("name", sorted(geo.PREDNET))
def test_prediction_step_cases_reach_their_geometry(name):
    c = geo.PREDNET[name]
    assert c["H"] % 16 not in (0, 8) and c["P"] % 4
    for R in c["rows"]:
        roles = geo.pn_roles(c["E"], c["H"], c["P"], c["L"], R)
        _show("prednet", name, R, roles)
        top = lambda role: geo.PN["kPnGatesRows"] if role.startswith("PN_GATES") else geo.PN["kPnDenseRows"]  # noqa: E731
        _assert_claim("prednet", name, c, R, roles, top)
        for role, g in roles.items():
            assert _partial(g, R), (role, g)
            assert g["TR"] == (4 if not role.startswith("PN_GATES") else (8 if R == 5 else 16)), (role, g)


def test_restated_workspace_layouts_have_the_librarys_sizes():
    """lt_images / en_images locate the packed weight images for the GPU test that reads them back; their totals are the
    library's own workspace sizes (the size queries need no device)."""
    from rnnt_speech_recognition_amd import _lib

    for c in geo.TRAIN.values():
        for R in c["rows"] + (5,):
            assert geo.lt_images(c["H"], c["P"], R)[1] == _lib.lstm_train_workspace_bytes(R, c["T"], c["H"], c["P"])
    for c in geo.ENCODER.values():
        blocks = (_lib.rnntPrednetBlock * c["L"])()
        for b in blocks:
            b.hidden, b.proj, b.ln_eps = c["H"], c["P"], 1e-5
            b.W_hr = 16 if c["P"] < c["H"] else None  # (only "projected or not" is read)
        for R in c["rows"]:
            for Tmax in (c["T"], 3 * c["T"] + 1):
                want = _lib.encoder_workspace_bytes(blocks, c["feat"][0] * c["feat"][1], c["ridx"], c["f"], R, Tmax)
                assert geo.en_images(*geo.encoder_args(c), R, Tmax)[1] == want, (c, R, Tmax)


def test_the_existing_suites_rows_are_whole_tiles():
    """Why the cases exist: every row count the older GPU suites run is a whole number of row tiles in every role."""
    for H, P, rows in ((256, 128, (1, 16, 64)), (320, 320, (64,)), (200, 72, (1, 16, 64)), (2048, 640, (16,))):
        for R in rows:
            assert not any(_partial(g, R) for g in geo.lt_roles(H, P, R).values()), (H, P, R)
    for H, P, rows in ((256, 128, (1, 16, 64)), (320, 320, (1, 16, 64)), (2048, 640, (4,)), (200, 72, (1, 16, 64))):
        for R in rows:
            assert not any(_partial(g, R) for g in geo.en_roles(H, P, R).values()), (H, P, R)
    for E, H, P, L in ((64, 256, 128, 2), (64, 640, 640, 1), (500, 2048, 640, 2), (37, 200, 72, 2)):
        for R in (1, 16, 256):
            assert not any(_partial(g, R) for g in geo.pn_roles(E, H, P, L, R).values()), (H, P, R)
