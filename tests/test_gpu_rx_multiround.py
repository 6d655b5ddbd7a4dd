"""The many-lane RX path at the launch forms its tuned batch shape never reaches, each compared
with the oracle bit for bit: classify tiles of several rounds (rx_classify<*, 1, *> and the MR = 0
form with nbuf == 2: tail pass with offsets from global memory, LDS indices wrapping at RX_ROUND,
per-round verdict stores, double-buffered descriptors with a partial last round, the round demux
pass fed from the argument-borne bind table), rx_scatter by fan-out and by lane count (32-bit
histogram, up to 16384 lanes), rx_scan_reduce / rx_scan_top / rx_scan_down as RX's scan
(UDPDK_RX_SCAN_COLS_TILES=0), lane overflow on rx_scatterw and rx_scatter, and single-lane tiles
of several rounds (UDPDK_ONE_LANE_TILE).

UDPDK_RX_HIST_CAP=65536 (the smallest accepted bound on lanes x tiles) makes the geometry double
the tile at small batches; test_trace_forms reads UDPDK_RX_TRACE's line and asserts, per shape,
the tile size, the histogram width and the scan and scatter kernels the call took, so a change
of the geometry cannot quietly turn these cases into one-round ones.

Inputs and oracle results are built once per module and shared by every form. The no-ptype
variant of a mixed batch is the same batch without its ptype array."""
import errno
import functools
import os

import numpy as np
import pytest

import oracle as O
from udpdk_amd import abi, frames as F

gpu = pytest.mark.gpu

HIST_CAP = 1 << 16
MAX_FRAMES = 1 << 17
MAX_LANES = 16384
IP1, IP9 = "172.31.100.1", "172.31.100.9"
ENV = ("UDPDK_RX_TAILG", "UDPDK_RX_MR", "UDPDK_RX_POLICY", "UDPDK_RX_SCAN_COLS_TILES",
       "UDPDK_SCATTER_MIN_WG", "UDPDK_RX_HIST_CAP", "UDPDK_RX_TRACE", "UDPDK_ONE_LANE_TILE")


def _geom(n, lanes, cap=HIST_CAP):
    """rx_plan.h's geometry(): (frames per tile, tiles)."""
    t = 1024
    while t < 8192 and -(-n // t) * lanes > cap:
        t *= 2
    return t, max(1, -(-n // t))


def _make_ctx(env):
    """A context created under env (on top of UDPDK_RX_HIST_CAP); the environment is restored."""
    env = dict(env, UDPDK_RX_HIST_CAP=str(HIST_CAP))
    old = {k: os.environ.get(k) for k in ENV}
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return abi.GpuContext(0, max_frames=MAX_FRAMES, max_lanes=MAX_LANES)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# (UDPDK_RX_TAILG, UDPDK_RX_MR, UDPDK_RX_POLICY, UDPDK_RX_SCAN_COLS_TILES, UDPDK_SCATTER_MIN_WG);
# None = unset. The first is the production form; the last adds rx_scatterw's grouped tiles
# (G > 1, 16 waves) reading the rows the 3-pass scan rescanned in place.
FORMS = [(2, None, 1, None, None), (2, 0, 1, None, None), (1, None, 1, None, None), (1, 0, 1, None, None),
         (2, None, 0, None, None), (1, None, 0, None, None), (2, None, 1, 0, None), (2, None, 1, 0, 1)]


def _form_env(f):
    names = ("UDPDK_RX_TAILG", "UDPDK_RX_MR", "UDPDK_RX_POLICY", "UDPDK_RX_SCAN_COLS_TILES",
             "UDPDK_SCATTER_MIN_WG")
    return {k: str(v) for k, v in zip(names, f) if v is not None}


def _form_id(f):
    return "g{}-mr{}-pol{}-cols{}-wg{}".format(*("x" if v is None else v for v in f))


@pytest.fixture(scope="module", params=FORMS, ids=_form_id)
def form_ctx(request):
    ctx = _make_ctx(_form_env(request.param))
    yield ctx
    ctx.close()


# ---- inputs, built once ---------------------------------------------------------------------------
PORTS = [10000 + i for i in range(600)]
UNBOUND = [9, 20000, 65535]
FEW_PORTS = [10001 + i for i in range(9)]
FEW_FDS = [0, 1000, 4095, 1, 2047, 2048, 63, 64, 4094]
LISTS1 = {abi.raw_port(10001): [(0, 0, 0)]}


@functools.lru_cache(maxsize=None)
def _mixed(n):
    return F.mixed_batch(1000 + n, n, PORTS, UNBOUND, [IP1, IP9], with_ptype=True)


@functools.lru_cache(maxsize=None)
def _mixed_few():
    return F.mixed_batch(77, 40000, FEW_PORTS, UNBOUND, [IP1, IP9], with_ptype=False)


def _no_ptype(b):
    return F.Batch(b.frames, b.offset, b.length, b.frames_bytes, None)


def _plain_lists(n_lanes, seed):
    """One binding per port on a seeded sockfd below n_lanes: ANY, every tenth on an address that
    only the frames to IP9 match."""
    fd = np.random.default_rng(seed).integers(0, n_lanes, len(PORTS))
    return {abi.raw_port(p): [(abi.raw_ip(IP9) if i % 10 == 3 else 0, int(fd[i]), 0)]
            for i, p in enumerate(PORTS)}


def _fan_lists():
    fd = np.random.default_rng(202).integers(0, 4096, (len(PORTS), 3))
    i1, i9 = abi.raw_ip(IP1), abi.raw_ip(IP9)
    out = {}
    for i, p in enumerate(PORTS):
        a, b, c = (int(x) for x in fd[i])
        out[abi.raw_port(p)] = [[(0, a, 0)],
                                [(0, a, 1), (i1, b, 1), (i1, c, 1)],
                                [(i9, a, 0)],
                                [(0, a, 1), (i1, b, 1)],
                                [(0, a, 0), (i1, b, 1)]][i % 5]
    return out


def _any_lists(n_lanes):
    return {abi.raw_port(10000 + i): [(0, i, 0)] for i in range(n_lanes)}


def _uniform64(n, n_lanes, seed):
    ports = 10000 + np.random.default_rng(seed).integers(0, n_lanes, n, dtype=np.uint32)
    return F.build_frames(np.full(n, 64, np.uint32), ports, seed)


def _edge_batch(n, n_lanes):
    """64-byte frames with every 97th to an unbound port, a 1500-byte frame as the last frame of
    every round of 1024 and as the last frame of the batch: a tail is pending across each round
    boundary and at the batch's last frame."""
    sizes = np.full(n, 64, np.uint32)
    sizes[1023::1024] = 1500
    sizes[n - 1] = 1500
    i = np.arange(n, dtype=np.uint32)
    ports = (10000 + i * 61 % n_lanes if n_lanes > 1 else np.full(n, 10001)).astype(np.uint32)
    ports[5::97] = 9
    return F.build_frames(sizes, ports, 300 + n % 1000)


def _fuzz(base, seed):
    """test_gpu_rx.py's test_fuzzed_headers_and_descriptors recipe over base."""
    rng = np.random.default_rng(seed)
    fr = base.frames.copy()
    for i in rng.choice(base.n, base.n * 3 // 10, replace=False):
        o = int(base.offset[i])
        for _ in range(int(rng.integers(1, 4))):
            pos = o + 12 + int(rng.integers(0, 40))
            if pos < base.frames_bytes:
                fr[pos] ^= np.uint8(1 << int(rng.integers(0, 8)))
    off = base.offset.astype(np.uint64).copy()
    ln = base.length.astype(np.uint32).copy()
    k = rng.choice(base.n, base.n // 20, replace=False)
    off[k] = rng.integers(0, base.frames_bytes + 5000, len(k))
    k = rng.choice(base.n, base.n // 20, replace=False)
    ln[k] = rng.choice([0, 1, 13, 14, 33, 41, 42, 43, 63, 64, 65, 2047, 65535], len(k))
    return F.Batch(fr, off.astype(np.uint32), ln.astype(np.uint16), base.frames_bytes, base.ptype)


@functools.lru_cache(maxsize=None)
def _case(key):
    """key -> (batch, port lists, lanes, the oracle's (meta, lane_off, lane_pkt, counters))."""
    kind = key[0]
    if kind in ("mixed", "fan"):                     # cases 1 and 2: (kind, frames, ptype array)
        b = _mixed(key[1]) if key[2] else _no_ptype(_mixed(key[1]))
        lists, lanes = (_plain_lists(4096, 101) if kind == "mixed" else _fan_lists()), 4096
    elif kind == "mixed16k":                         # case 3: case 1's batch over 16384 lanes
        b, lists, lanes = _mixed(20000), _plain_lists(16384, 303), 16384
    elif kind == "lanes":                            # case 3: (kind, lanes), one ANY port per lane
        b, lists, lanes = _uniform64(20000, key[1], key[1]), _any_lists(key[1]), key[1]
    elif kind == "imix":                             # case 4
        w = F.config_batch(4, n=70001)
        b, lists, lanes = w.batch, w.port_lists(), w.n_sockets
    elif kind == "few":                              # case 5: (kind, bound ports)
        b, lanes = _mixed_few(), 4096
        lists = {abi.raw_port(p): [(abi.raw_ip(IP9) if i == 2 else 0, FEW_FDS[i], 0)]
                 for i, p in enumerate(FEW_PORTS[:key[1]])}
    elif kind == "edge":                             # case 6: (kind, frames, lanes)
        b, lanes = _edge_batch(key[1], key[2]), key[2]
        lists = _any_lists(lanes) if lanes > 1 else LISTS1
    elif kind == "fuzz":                             # case 7: (kind, ptype array)
        b = _fuzz(_mixed(20000) if key[1] else _no_ptype(_mixed(20000)), 31 + key[1])
        lists, lanes = _plain_lists(4096, 101), 4096
    elif kind == "mixed1":                           # a mixed batch on one lane
        b = F.mixed_batch(9, 5000, [10001], UNBOUND, [IP1, IP9], with_ptype=True)
        lists, lanes = LISTS1, 1
    else:
        raise KeyError(key)
    want = O.rx(O.bindtable_from_lists(lists), b.frames, b.frames_bytes, b.offset, b.length, b.ptype,
                lanes, 0xFFFFFFFF)
    for x in want:
        x.setflags(write=False)
    return b, lists, lanes, want


def _run(ctx, key, cap=None, guard=0):
    """One udpdk_gpu_rx of the case on ctx -> (oracle's, (meta, lane_off, lane_pkt[:D], counters,
    rc), the whole lane_pkt buffer). cap: lane_cap (default: every delivery fits), with `guard`
    more words behind it, the buffer pre-filled with a pattern."""
    b, lists, lanes, want = _case(key)
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, lanes))
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, b.ptype)
    db.frames_bytes = b.frames_bytes
    cap = max(1, len(want[2])) if cap is None else cap
    out = abi.RxDeviceOut(ctx.alloc(4 * b.n), ctx.alloc(4 * (lanes + 1)),
                          ctx.upload(np.full(cap + guard, 0xA5A5A5A5, np.uint32)), cap, b.n, lanes)
    got = abi.rx_run(ctx, db, out)
    whole = ctx.download(out.lane_pkt, np.uint32, cap + guard)
    for x in (db.frames, db.offset, db.length, db.ptype, out.meta, out.lane_off, out.lane_pkt):
        if x is not None:
            x.free()
    return want, got, whole


def _same(want, got, what):
    wm, wl, wp, wc = want
    gm, gl, gp, gc, rc = got
    assert rc == 0, f"{what}: rc {rc}"
    bad = np.nonzero(wm != gm)[0]
    assert bad.size == 0, (f"{what}: {bad.size} verdict words differ, first at frame {bad[0]}: "
                           f"{wm[bad[0]]:#x} vs {gm[bad[0]]:#x}")
    assert np.array_equal(wl, gl), f"{what}: lane_off"
    assert len(wp) == len(gp) and np.array_equal(wp, gp), f"{what}: lane entries"
    assert np.array_equal(wc, gc), f"{what}: counters {wc} vs {gc}"


def _check(ctx, key):
    want, got, _ = _run(ctx, key)
    _same(want, got, str(key))
    return want


# ---- the geometry these cases rely on -----------------------------------------------------------
def test_geometry_helper():
    """_geom restates the library's geometry rule: equal to udpdk_gpu_rx_geometry at its bound of
    2^21 lanes x tiles, over a grid that holds this module's shapes scaled by 32 (the ratio of the
    two bounds)."""
    ns = [0, 1, 1023, 1024, 1025, 16384, 16385, 20000, 40000, 70001, 1 << 20, (1 << 20) + 1, 1 << 22,
          32 * 16384, 32 * 16385, 32 * 20000, 32 * 40000, 32 * 70001, (1 << 24) + 5]
    for lanes in (1, 2, 3, 8, 600, 1024, 4096, 5000, 8193, 16384):
        for n in ns:
            assert _geom(n, lanes, 1 << 21) == abi.geometry(n, lanes), (n, lanes)
    # the issue's table (the last tile's frames are n - (tiles - 1) T)
    assert _geom(20000, 4096) == (2048, 10) and 20000 - 9 * 2048 == 1024 + 544
    assert _geom(40000, 4096) == (4096, 10) and 40000 - 9 * 4096 == 3 * 1024 + 64
    assert _geom(20000, 16384) == (8192, 3) and 20000 - 2 * 8192 == 3616
    assert _geom(70001, 1024) == (2048, 35) and 70001 - 34 * 2048 == 369
    assert _geom(16384, 4096)[0] == 1024 and _geom(16385, 4096)[0] == 2048


# ---- cases 1-7 under every form -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ptype", [1, 0], ids=["ptype", "noptype"])
@pytest.mark.parametrize("n", [20000, 40000])
def test_mixed_many_lanes(form_ctx, n, ptype):
    """Case 1: every verdict but BAD_DESC, long and short frames, 600 bound ports on 4096 lanes,
    no fan-out (rx_scatterw, 16-bit histogram with the column scan)."""
    want = _check(form_ctx, ("mixed", n, ptype))
    b = _case(("mixed", n, ptype))[0]
    assert set(abi.meta_verdict(want[0]).tolist()) >= set(range(7))
    # 17 of mixed_batch's 21 kinds draw 0-199 payload bytes (frames of 42 + payload: 88.5 % above
    # 64 bytes), "big" is always longer, "pad", "tiny_ok" and "trunc" never are: 0.77 expected
    assert float(np.mean(b.length > 64)) > 0.75


@gpu
@pytest.mark.parametrize("ptype", [1, 0], ids=["ptype", "noptype"])
@pytest.mark.parametrize("n", [20000, 40000])
def test_mixed_fanout(form_ctx, n, ptype):
    """Case 2: the same batches with fan-out lists (rx_scatter, 32-bit histogram)."""
    want = _check(form_ctx, ("fan", n, ptype))
    assert int(abi.meta_fanout(want[0]).max()) == 3


@gpu
@pytest.mark.parametrize("lanes", [16384, 8193, 5000])
def test_lane_counts(form_ctx, lanes):
    """Case 3: more than 4096 lanes (rx_scatter by lane count; with the 3-pass scan,
    scan_lane_totals at 16 and 8 lanes per thread), odd counts among them."""
    _check(form_ctx, ("lanes", lanes))


@gpu
def test_mixed_16384_lanes(form_ctx):
    """Case 3: case 1's batch re-bound over 16384 lanes (8192-frame tiles, a 3616-frame last)."""
    _check(form_ctx, ("mixed16k",))


@gpu
def test_imix_1024_lanes(form_ctx):
    """Case 4: IMIX over 1024 ports, 35 tiles of 2048 frames, the last of 369."""
    _check(form_ctx, ("imix",))


@gpu
@pytest.mark.parametrize("nports", [5, 8, 9])
def test_few_ports_many_lanes(form_ctx, nports):
    """Case 5: 5 and 8 bound ports (the bind table rides in the kernel arguments and feeds the
    round demux pass of the several-round tile) and 9 (port table), sockfds at both ends of 4096
    lanes, one port bound to an address that only part of its frames match."""
    want = _check(form_ctx, ("few", nports))
    assert {abi.V_DELIVERED, abi.V_NO_BIND, abi.V_NO_MATCH} <= set(abi.meta_verdict(want[0]).tolist())


def _edge_counts(lanes, first, ks):
    """first, then k T + {0, 1, 63, 1024, 1025} for the tile size the geometry gives there."""
    out = [first]
    for k, t in ks:
        for d in (0, 1, 63, 1024, 1025):
            n = k * t + d
            assert _geom(n, lanes)[0] == t, (n, lanes)
            out.append(n)
    return out


EDGE_N = _edge_counts(4096, 16385, [(9, 2048), (9, 4096)])


@gpu
@pytest.mark.parametrize("n", EDGE_N)
def test_round_and_tile_edges(form_ctx, n):
    """Case 6: batches ending at a tile end, one frame, 63 frames, a round and a round and a frame
    past it (tiles of 2048 and 4096 frames), and the smallest batch with tiles of several rounds;
    a long frame at every round end and at the batch end."""
    assert _geom(n, 4096)[0] > 1024
    _check(form_ctx, ("edge", n, 4096))


@gpu
@pytest.mark.parametrize("ptype", [1, 0], ids=["ptype", "noptype"])
def test_fuzzed_multiround(form_ctx, ptype):
    """Case 7: flipped header bits, offsets anywhere (past the batch too) and edge lengths."""
    want = _check(form_ctx, ("fuzz", ptype))
    assert abi.V_BAD_DESC in set(abi.meta_verdict(want[0]).tolist())


@gpu
def test_alternating_calls(form_ctx):
    """Case 8: no fan-out, fan-out, no fan-out, fan-out on one context: the snapshot is uploaded
    again, the histogram changes width and the scan epochs advance between the calls."""
    for key in (("mixed", 20000, 1), ("fan", 40000, 0), ("mixed", 40000, 0), ("fan", 20000, 1)):
        _check(form_ctx, key)


@gpu
@pytest.mark.parametrize("kind", ["mixed", "fan"])
def test_lane_overflow_many_lanes(form_ctx, kind):
    """Case 9: lane_cap at a third of the deliveries on rx_scatterw and rx_scatter: ENOSPC, the
    whole lane_off, the entries that fit, nothing written past lane_cap."""
    key = (kind, 20000, 1)
    d = len(_case(key)[3][2])
    cap = d // 3
    assert cap > 1000
    want, got, whole = _run(form_ctx, key, cap=cap, guard=4096)
    assert got[4] == -errno.ENOSPC
    assert np.array_equal(want[0], got[0]), "verdict words"
    assert np.array_equal(want[1], got[1]), "lane_off"
    assert np.array_equal(want[2][:cap], whole[:cap]), "entries below lane_cap"
    assert np.all(whole[cap:] == 0xA5A5A5A5), "words past lane_cap written"


# ---- which kernels ran --------------------------------------------------------------------------
TRACE_FORMS = {"prod": {}, "mr0": {"UDPDK_RX_MR": "0"}, "3pass": {"UDPDK_RX_SCAN_COLS_TILES": "0"},
               "3pass-grouped": {"UDPDK_RX_SCAN_COLS_TILES": "0", "UDPDK_SCATTER_MIN_WG": "1"}}
# case -> (lanes, frames, scatter kernel without grouping, fan-out)
TRACE_SHAPES = {("lanes", 16384): (16384, 20000, "scatter1", False),
                ("lanes", 8193): (8193, 20000, "scatter1", False),
                ("lanes", 5000): (5000, 20000, "scatter1", False),
                ("mixed16k",): (16384, 20000, "scatter1", False),
                ("imix",): (1024, 70001, "scatterw8", False)}
for _n in (20000, 40000):
    for _p in (1, 0):
        TRACE_SHAPES[("mixed", _n, _p)] = (4096, _n, "scatterw8", False)
        TRACE_SHAPES[("fan", _n, _p)] = (4096, _n, "scatter1", True)
for _p in (5, 8, 9):
    TRACE_SHAPES[("few", _p)] = (4096, 40000, "scatterw8", False)
for _n in EDGE_N:
    TRACE_SHAPES[("edge", _n, 4096)] = (4096, _n, "scatterw8", False)
for _p in (1, 0):
    TRACE_SHAPES[("fuzz", _p)] = (4096, 20000, "scatterw8", False)


@pytest.fixture(scope="module", params=sorted(TRACE_FORMS))
def trace_ctx(request):
    ctx = _make_ctx(dict(TRACE_FORMS[request.param], UDPDK_RX_TRACE="1", UDPDK_RX_TAILG="2"))
    yield request.param, ctx
    ctx.close()


def _trace_line(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("udpdk_gpu_rx seq") and " form " in ln]
    assert len(lines) == 1, err
    w = lines[0].split(" form ")[1].split()
    return dict(zip(w[0::2], w[1::2]))


@gpu
@pytest.mark.parametrize("key", sorted(TRACE_SHAPES, key=str), ids=str)
def test_trace_forms(trace_ctx, capfd, key):
    """The form line of UDPDK_RX_TRACE for every shape: tiles of several rounds at the size the
    geometry helper gives, mr as forced, the 16-bit histogram only with the column scan and
    without fan-out, the scan and the scatter kernel."""
    form, ctx = trace_ctx
    lanes, n, scatter, fan = TRACE_SHAPES[key]
    _case(key)
    capfd.readouterr()
    want, got, _ = _run(ctx, key)
    tr = _trace_line(capfd.readouterr().err)
    _same(want, got, f"{form} {key}")
    t, tiles = _geom(n, lanes)
    assert t > 1024
    assert (int(tr["T"]), int(tr["tiles"])) == (t, tiles)
    assert tr["mr"] == ("0" if form == "mr0" else "1")
    cols = not form.startswith("3pass")
    assert tr["hist16"] == ("1" if cols and not fan else "0")
    assert (tr["scan"] in ("cols512", "cols1024")) if cols else tr["scan"] == "3pass"
    if form == "3pass-grouped" and scatter == "scatterw8" and lanes == 4096:
        # 4096 lanes hold the (frame, position) pairs of 16384 frames: groups of that many
        assert (tr["scatter"], int(tr["G"])) == ("scatterw16", 16384 // t)
    elif form != "3pass-grouped":
        assert (tr["scatter"], tr["G"]) == (scatter, "1")
    else:
        assert tr["scatter"] == scatter


# ---- single-lane tiles of several rounds (UDPDK_ONE_LANE_TILE) ------------------------------------
@pytest.fixture(scope="module", params=[(2048, 1), (8192, 2)], ids=lambda p: f"tile{p[0]}-g{p[1]}")
def one_lane_ctx(request):
    tile, g = request.param
    ctx = _make_ctx({"UDPDK_ONE_LANE_TILE": str(tile), "UDPDK_RX_TAILG": str(g), "UDPDK_RX_TRACE": "1"})
    yield tile, ctx
    ctx.close()


@gpu
def test_one_lane_multiround_tiles(one_lane_ctx, capfd):
    """One lane with tiles of 2048 and 8192 frames: rx_classify's several-round form with the
    argument-borne bind table in the round demux pass, then rx_compact1 without speculative
    entries. Round and tile edges with long frames at the round ends, and a mixed batch."""
    tile, ctx = one_lane_ctx
    for n in (2 * tile, 2 * tile + 1, 2 * tile + 63, 2 * tile + 1024, 2 * tile + 1025, 1025):
        capfd.readouterr()
        want, got, _ = _run(ctx, ("edge", n, 1))
        tr = _trace_line(capfd.readouterr().err)
        _same(want, got, f"tile {tile} n {n}")
        assert (int(tr["T"]), int(tr["tiles"]), tr["mr"], tr["scatter"]) == (tile, -(-n // tile), "1", "compact1")
    _check(ctx, ("mixed1",))


@gpu
def test_one_lane_multiround_overflow(one_lane_ctx):
    """lane_cap below the deliveries on the single lane's several-round tiles."""
    tile, ctx = one_lane_ctx
    key = ("edge", 2 * tile + 1025, 1)
    cap = len(_case(key)[3][2]) // 3
    want, got, whole = _run(ctx, key, cap=cap, guard=4096)
    assert got[4] == -errno.ENOSPC
    assert np.array_equal(want[1], got[1]), "lane_off"
    assert np.array_equal(want[2][:cap], whole[:cap]), "entries below lane_cap"
    assert np.all(whole[cap:] == 0xA5A5A5A5), "words past lane_cap written"
