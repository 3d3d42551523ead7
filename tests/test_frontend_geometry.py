"""tests/frontend_geometry.py against the source and against its own case table (no GPU): the copied constants equal the ones in
frontend_kernels.hip, every case of tests/test_frontend_geometry_gpu.py reaches the FFT size, frame tiles, mel-loop trips, held
frames and empty filters it is named for, the float64 reference alone satisfies the condition of the 2e-3 bar (no mel energy, no
|X_k| of the spectrum group, below 1e-3), and the torch route on the CPU passes every case StreamingFrontEnd can express -- which
checks the restatement, the mirror and the inputs independently of the kernels."""
import os
import re

import numpy as np
import pytest
import torch

from rnnt_speech_recognition_amd import features
from tests import frontend_geometry as geo

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rnnt-speech-recognition_amd", "csrc",
                      "frontend_kernels.hip")


def test_copied_constants_equal_the_source():
    with open(SOURCE) as fh:
        text = fh.read()
    for name, value in geo.CONSTANTS.items():
        m = re.search(r"constexpr int " + name + r"\s*=\s*(\d+);", text)
        assert m and int(m.group(1)) == value, name
    # the loops the trip counts restate, and the launch rule
    assert "for (int j = lane; j < a.M; j += 64)" in text
    assert "for (int b = tid; b < M; b += kFeEmitThreads)" in text
    assert "const dim3 grid((nf + kFeTile - 1) / kFeTile, S);" in text
    assert "__shared__ float2 s_tw[N];" in text
    assert "__shared__ float s_re[kFeWaves][N], s_im[kFeWaves][N], s_mag[kFeWaves][NB];" in text


def test_lds_of_every_instantiation_fits_a_workgroup():
    for N in (256, 512, 1024, 2048):
        print(f"fe_frames_kernel<{N}>: {geo.lds_bytes(N)} bytes of LDS ({geo.lds_bytes(N) / 1024:.1f} KB)")
        assert geo.lds_bytes(N) <= geo.LDS_LIMIT
    assert geo.lds_bytes(2048) == 98320 and 2 * geo.lds_bytes(2048) > geo.LDS_LIMIT  # one workgroup per CU


def test_restated_workspace_and_limits_are_the_librarys():
    """geo.workspace_bytes (G = stack * rm held frames, NF frames of x per slot) equals the library's size query for every
    case, and the query refuses what lies one past each limit of include/rnnt.h (the size queries need no device)."""
    from rnnt_speech_recognition_amd import _lib

    shapes = [(c["K"], c["S"], c["L"], c["step"], c["M"], c["stack"], c["rm"]) for c in geo.CASES.values()]
    shapes += [(L + 16 * geo.SPECTRUM_STEP, 1, L, geo.SPECTRUM_STEP, M, 1, 1) for N, L in geo.SPECTRUM for M, _ in geo.spectrum_pickers(N)]
    for shape in shapes:
        assert geo.workspace_bytes(*shape) == _lib.frontend_workspace_bytes(*shape), shape
    ok = (1000, 1024, geo.MAX_LEN, geo.MAX_LEN, 1024, 16, 16)
    assert _lib.frontend_workspace_bytes(*ok) == geo.workspace_bytes(*ok)
    for i, v in ((0, 0), (0, (1 << 20) + 1), (1, 1025), (2, geo.MAX_LEN + 1), (2, 128), (3, 0), (4, 1025), (4, 0), (5, 17), (6, 17)):
        bad = list(ok)
        bad[i] = v
        with pytest.raises(RuntimeError):
            _lib.frontend_workspace_bytes(*bad)
    with pytest.raises(RuntimeError):
        _lib.frontend_workspace_bytes(1000, 1, 400, 401, 80, 3, 1)  # frame_step > frame_len
    assert _lib.frontend_workspace_bytes(1, 1, 129, 1, 1, 1, 1) > 0


@pytest.mark.parametrize("name", sorted(geo.CASES))
def test_cases_reach_their_geometry(name):
    c = geo.CASES[name]
    reach = dict(c["reach"])
    _, W = geo.tables(c)
    m, counts = geo.mirror_of(c)
    feeds = geo.feeds_of(c)
    nf = [[t["nf"] for t in tr] for tr in m.trace]
    print(f"{name}: nfft {geo.nfft_of(c['L'])}, feeds {len(feeds)}, frames per slot {[sum(x) for x in nf if sum(x)][:8]}, "
          f"band trips {geo.band_trips(c['M'])}, emit trips {geo.emit_trips(c['M'])}, empty filters {len(geo.empty_filters(W))}, "
          f"max h0 {max(t['h0'] for tr in m.trace for t in tr)}, K {c['K']}, max_rows "
          f"{geo.max_rows(c['K'], c['step'], c['stack'], c['rm'])}")
    assert geo.nfft_of(c["L"]) == reach.pop("nfft")
    assert c["K"] == max(len(x) for ch, _, _ in feeds for x in ch if x is not None)
    if "tiles" in reach:  # of the one feed, per live slot
        assert len(feeds) == 1 and [geo.tiles_of(nf[s][0]) for s in sorted(c["streams"])] == reach.pop("tiles")
    if "grid" in reach:
        assert geo.grid_tiles(max(len(x) for x in feeds[0][0]), c["step"]) == reach.pop("grid")
    if "band" in reach:
        assert (geo.band_trips(c["M"]), geo.emit_trips(c["M"])) == (reach.pop("band"), reach.pop("emit"))
    if "empty" in reach:
        assert len(geo.empty_filters(W)) == reach.pop("empty")
    if "frames" in reach:
        assert sum(nf[0]) == reach.pop("frames")
    if "first_frame_feed" in reach:
        assert c["K"] == 1 and [i + 1 for i, x in enumerate(nf[0]) if x][0] == reach.pop("first_frame_feed")
    if "live" in reach:
        live = [s for s in range(c["S"]) if any(t["live"] for t in m.trace[s])]
        assert live == list(range(0, 1024, 64)) and len(live) == reach.pop("live") and c["S"] == 1024
        assert all(sum(counts[i][s] for i in range(len(feeds))) > 0 for s in live)
    if "held" in reach:
        stack, rm, G = c["stack"], c["rm"], c["stack"] * c["rm"]
        tr = m.trace[1]
        assert G - 1 == reach.pop("held") == max(t["h0"] for t in tr)  # h0 climbs to G - 1 ...
        top = [i for i, t in enumerate(tr) if t["h0"] == G - 1][0]
        assert all(t["count"] == 0 for t in tr[:top]) and all(t["nf"] <= 5 for t in tr[:top])  # ... before a feed crosses G
        assert {0, 1} <= {t["nf"] for t in tr[:top + 1]} or G <= 2
        assert any(not t["final"] and t["count"] >= 2 * rm for t in tr)             # a non-final feed that emits several groups
        assert G == 1 or any(not t["final"] and t["count"] == 0 and t["nf"] > 0 for t in tr)  # one that emits nothing
        last = tr[-1]
        assert last["final"] and last["count"] > 0 and (stack == 1 or (last["h0"] + last["nf"]) % stack)  # a partial group
        short = m.trace[0]
        assert short[1]["final"] and short[1]["count"] == 0 and short[1]["h0"] + short[1]["nf"] < stack  # total < stack: 0 rows
        assert not any(t["live"] for t in m.trace[2])
    assert not reach, reach
    assert max(max(x) for x in counts) <= geo.max_rows(c["K"], c["step"], c["stack"], c["rm"])


def test_the_step1_stream_gives_a_frame_per_sample():
    c = geo.CASES["step1_L129"]
    m, _ = geo.mirror_of(c)
    chunks = c["streams"][0][1]
    assert [t["nf"] for t in m.trace[0]] == [0] + chunks[1:]  # k samples give k frames once L - 1 are carried


@pytest.mark.parametrize("name", sorted(geo.CASES))
def test_the_reference_alone_meets_the_condition_of_the_bar(name):
    c = geo.CASES[name]
    window, W = geo.tables(c)
    floors = {s: geo.floor_of(geo.stream_audio(c, s), window, W, c["step"]) for s in c["streams"]}
    print(f"{name}: smallest float64 mel energy over non-empty filters {min(floors.values()):.3e}")
    assert min(floors.values()) > geo.FLOOR, floors
    if name == "width_M1024_nfft2048":
        assert 1.3e-3 < floors[0] < 1.5e-3  # 1.4e-3: the narrowest margin of the table


@pytest.mark.parametrize("N,L", sorted(geo.SPECTRUM))
def test_every_bin_of_the_spectrum_reference_is_above_the_floor(N, L):
    assert geo.nfft_of(L) == N and (L == N or geo.nfft_of(L - 1) == N // 2)  # no padding; the smallest L of this N
    audio = geo.spectrum_audio(N, L)
    m = geo.Mirror(1, L, geo.SPECTRUM_STEP, 1, 1)
    assert m.feed(len(audio), [len(audio)], [1], [1]) == [17] and geo.tiles_of(17) == 2 and 17 % geo.TILE == 1
    covered = set()
    for M, off in geo.spectrum_pickers(N):
        W = geo.bin_picker(N // 2 + 1, M, off)
        assert M <= 1024 and not len(geo.empty_filters(W)) and (W.sum(axis=0) == 1).all()
        covered |= set(range(off, off + M))
        floor = geo.floor_of(audio, geo.spectrum_window(L), W, geo.SPECTRUM_STEP)
        print(f"spectrum nfft {N} L {L} bins {off} ... {off + M - 1}: smallest |X_k| {floor:.3e}")
        assert floor > geo.FLOOR
    assert covered == set(range(N // 2 + 1))  # DC through Nyquist


def _torch_route(c, norm):
    """The case through StreamingFrontEnd(engine=False) on the CPU -> (rows per stream slot, counts per feed)."""
    fe = features.StreamingFrontEnd(geo.hparams_of(c), c["sr"], c["S"], c["K"], c["rm"], "running" if norm else "none",
                                    device=torch.device("cpu"), engine=False)
    window, W = geo.tables(c)
    assert (fe.L, fe.step, fe.nfft, fe.M) == (c["L"], c["step"], geo.nfft_of(c["L"]), c["M"])
    assert np.array_equal(fe.window.numpy(), window) and np.array_equal(fe.mel_w.numpy(), W)  # the inputs the device gets
    got, counts = {s: [] for s in c["streams"]}, []
    for chunks, reset, final in geo.feeds_of(c):
        fe.start([s for s in range(c["S"]) if reset[s]])
        n = max(0 if x is None else len(x) for x in chunks)
        audio = torch.zeros(c["S"], n)
        for s, x in enumerate(chunks):
            if x is not None:
                audio[s, : len(x)] = torch.as_tensor(x)
        rows, cnt = fe.feed(audio, [0 if x is None else len(x) for x in chunks], [bool(v) for v in final])
        counts.append(cnt)
        for s in got:
            got[s].append(rows[s, : cnt[s]])
    return {s: torch.cat(v).numpy() for s, v in got.items()}, counts


@pytest.mark.parametrize("name", sorted(geo.CASES))
def test_the_torch_route_passes_every_case(name):
    c = geo.CASES[name]
    window, W = geo.tables(c)
    _, want = geo.mirror_of(c)
    for norm in c["norms"]:
        rows, counts = _torch_route(c, norm)
        assert counts == want
        top = max(geo.check_rows(rows[s], geo.stream_audio(c, s), window, W, c["step"], c["stack"], norm) for s in rows)
        print(f"torch route {name} norm {norm}: max error {top:.3e} (bar {geo.BAR:.0e})")


def test_the_mirror_extends_the_integer_rule():
    """Mirror against frontend_cases.expected_counts on a plain stream, and the rules only the C ABI reaches."""
    chunks = geo.fc.ragged_chunks(19200)
    m = geo.Mirror(1, 400, 160, 3, 2)
    got = [m.feed(3000, [k], [int(i == 0)], [int(i + 1 == len(chunks))])[0] for i, k in enumerate(chunks)]
    assert got == geo.fc.expected_counts(chunks, 400, 160, 3, 2)
    m = geo.Mirror(3, 400, 160, 1, 1)
    assert m.feed(1000, [1000, 1000, 1000]) == [0, 0, 0]                      # every slot begins FINISHED
    assert m.feed(1000, [-5, 2000, 560], [1, 1, 1]) == [0, 4, 2]              # clamped into 0 ... chunk_samples
    assert m.feed(0, [7, 7, 7]) == [0, 0, 0] and m.c == [0, 1000 - 4 * 160, 560 - 2 * 160]
    assert m.feed(1000, [1000, 0, 0], [0, 0, 1], [1, 1, 0]) == [4, 0, 0]      # the reset applies before the call's samples
    assert m.fin == [True, True, False] and m.c[2] == 0
