"""The RX peer filter on the GPU (udpdk_gpu_rx_peer_select, udpdk_gpu_rx_peer) against the model of
rx_peer_util.py, which test_rx_peer_ref.py pins to the oracle: lane_off, lane_pkt and every stats
field, exactly. The explicit call takes any lane set, so most shapes are built by hand on the
kernel's boundaries (the 64-entry chunk, the 256-entry wave, the 1024-entry tile); the fan-out and
sticky tests take their lanes from udpdk_gpu_rx itself (pinned to the oracle by test_gpu_rx.py)."""
import ctypes as C
import errno

import numpy as np
import pytest

import rx_balance_util as UB
import rx_drop_util as UD
import rx_peer_util as U
from test_gpu_rx import IP1, IP9
from test_gpu_rx_balance import LISTS_SHAPES, PA, PB, PC, PX, RP_SHAPES, free, rx
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

E = 1024                    # entries per compaction tile (FLT_TILE, rx_filter.h)
SENT = 0xA5A5A5A5
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]       # chunk, wave, tile
# the ways an entry of a lane connected to U.PEER can look: (source, destination port)
PEER_F = (U.PEER, PA)
PATTERNS = {"ip": (U.STRANGERS[0], PA), "port": (U.STRANGERS[1], PA), "both": (U.STRANGERS[2], PA),
            "dport-is-peer-port": (U.STRANGERS[1], U.PEER[1])}
KINDS = [PEER_F] + list(PATTERNS.values())
ONE = {abi.raw_port(PA): [(0, 0, 0)]}


@pytest.fixture(scope="module")
def pctx():
    ctx = abi.GpuContext(0, max_frames=1 << 17, max_lanes=4096)
    ctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))         # (the explicit call wants sockfd lanes)
    yield ctx
    ctx.close()


def kinds_batch(kinds, seed, **kw):
    """One frame per (source, dport) of `kinds`."""
    return U.frames_from([k[0] for k in kinds], [k[1] for k in kinds], seed, **kw)


def random_kinds(n, seed):
    return [KINDS[int(k)] for k in np.random.default_rng(seed).integers(0, len(KINDS), n)]


def dev(ctx, b):
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, None)
    db.frames_bytes = b.frames_bytes
    return db


def check(ctx, b, db, loff, lpkt, peers, what, **kw):
    mk = {k: v for k, v in kw.items() if k in ("n", "lane_cap")}
    m = U.model(b, loff, lpkt, peers, frames_bytes=db.frames_bytes, **mk)
    go, gp, st, rc = abi.rx_peer_run(ctx, db, loff, lpkt, peers, pad=8, **kw)
    out_cap = len(gp) - 8
    assert np.array_equal(go, m.lane_off), f"{what}: lane_off"
    w = min(m.kept, out_cap)
    assert np.array_equal(gp[:w], m.lane_pkt[:w]), f"{what}: lane entries"
    assert np.all(gp[w:] == SENT), f"{what}: wrote past the kept entries"
    assert U.stats_tuple(st) == m.stats(), what
    assert rc == (-errno.ENOSPC if m.kept > out_cap else 0), what
    return m


# ---- the explicit call --------------------------------------------------------------------------
@pytest.mark.parametrize("d", COUNTS)
def test_entry_counts_one_lane(pctx, d):
    kinds = random_kinds(max(1, d), 100 + d)
    b = kinds_batch(kinds, d)
    db = dev(pctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [d])
        m = check(pctx, b, db, loff, np.resize(lpkt, max(1, d)), U.peer_table(1, {0: U.PEER}), f"d={d}", lane_cap=d)
        assert m.kept == sum(k == PEER_F for k in kinds[:d]) and m.refused == d - m.kept
        ident = check(pctx, b, db, loff, np.resize(lpkt, max(1, d)), U.peer_table(1, {}), f"off d={d}", lane_cap=d)
        assert ident.kept == d
    finally:
        free(db)


def test_workspace_grows_and_is_reused():
    """A fresh context's first three calls: one tile, then three (the workspace has to grow), then
    one again (the larger workspace is reused, with the second call's rows and masks beyond the
    live ones); lanes and stats exact after each."""
    ctx = abi.GpuContext(0, max_frames=1 << 12, max_lanes=8)
    try:
        ctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))
        for step, d in enumerate((64, 2 * E + 1, 64)):
            kinds = random_kinds(d, 900 + step)
            b = kinds_batch(kinds, 900 + step)
            db = dev(ctx, b)
            try:
                loff, lpkt = U.single_lanes(1, [d])
                m = check(ctx, b, db, loff, lpkt, U.peer_table(1, {0: U.PEER}), f"step {step} d={d}")
                assert m.kept == sum(k == PEER_F for k in kinds) and m.refused == d - m.kept
            finally:
                free(db)
    finally:
        ctx.close()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_patterns_at_chunk_and_tile_edges(pctx, pattern):
    """Each way to differ from the peer, alone, at the first and the last entry of chunks (also the
    ones that end a wave and a tile); every other entry is the peer's."""
    d = E + 128
    at = [0, 63, 64, 127, 255, 256, E - 1, E, E + 63, E + 64, d - 1]
    kinds = [PEER_F] * d
    for p in at:
        kinds[p] = PATTERNS[pattern]
    b = kinds_batch(kinds, 7)
    db = dev(pctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [d])
        m = check(pctx, b, db, loff, lpkt, U.peer_table(1, {0: U.PEER}), pattern)
        assert m.refused == len(at) and list(np.flatnonzero(~m.keep)) == at
        # and the other way round: a lane connected to that source keeps exactly those entries
        src = PATTERNS[pattern][0]
        m = check(pctx, b, db, loff, lpkt, U.peer_table(1, {0: src}), pattern + " inverse")
        assert list(m.lane_pkt) == at
    finally:
        free(db)


@pytest.fixture(scope="module")
def two_lane_batch(pctx):
    d = 2 * E + 252
    b = kinds_batch(random_kinds(d, 5), 5)
    db = dev(pctx, b)
    yield b, db, d
    free(db)


@pytest.mark.parametrize("conn", [0, 1])
@pytest.mark.parametrize("bnd", COUNTS)
def test_two_lanes_boundary(pctx, two_lane_batch, bnd, conn):
    """The lane boundary at every count, inside a wave and on a tile edge; either side connected."""
    b, db, d = two_lane_batch
    loff, lpkt = U.single_lanes(2, [bnd, d - bnd])
    m = check(pctx, b, db, loff, lpkt, U.peer_table(2, {conn: U.PEER}), f"bnd={bnd} conn={conn}")
    lo, hi = (0, bnd) if conn == 0 else (bnd, d)
    assert m.removed == int((~m.keep[lo:hi]).sum()) and m.keep[:lo].all() and m.keep[hi:].all()


def test_alternating_lanes_with_their_own_peers(pctx):
    """Connected and unconnected lanes alternate, every connected lane to another peer (so a record
    taken from a neighbour's lane shows), one of them empty; lane sizes off every boundary."""
    counts = [37, 5, 64, 1, 200, 0, 65, 63, 0, 256, 300, 3, 129, 64, 1, 700]
    srcs = [(f"10.7.{l}.1", 7000 + l) for l in range(16)]
    d = sum(counts)
    lane_of = np.repeat(np.arange(16), counts)
    rng = np.random.default_rng(3)
    # an entry's source: its lane's peer, a neighbour lane's peer, or the lane's address with the neighbour's port
    pick = rng.integers(0, 3, d)
    kinds = []
    for l, k in zip(lane_of, pick):
        o = (l + 2) % 16
        kinds.append(((srcs[l][0], srcs[l][1]) if k == 0 else srcs[o] if k == 1 else (srcs[l][0], srcs[o][1]), PA))
    b = kinds_batch(kinds, 11, gaps=rng.integers(0, 4, d))
    db = dev(pctx, b)
    try:
        loff, lpkt = U.single_lanes(16, counts)
        conn = {l: srcs[l] for l in range(0, 16, 2)}
        assert counts[8] == 0 and 8 in conn                          # a connected lane that is empty
        m = check(pctx, b, db, loff, lpkt, U.peer_table(16, conn), "alternating")
        want = (lane_of % 2 == 1) | (pick == 0)
        assert np.array_equal(m.keep, want) and m.refused == int((~want).sum()) > 300
    finally:
        free(db)


def test_4096_lanes_mostly_empty(pctx):
    n_lanes = 4096
    rng = np.random.default_rng(17)
    live = np.sort(rng.choice(n_lanes, 48, replace=False))
    counts = np.zeros(n_lanes, np.int64)
    counts[live] = rng.integers(1, 140, len(live))
    counts[[0, n_lanes - 1]] = [3, 70]
    d = int(counts.sum())
    b = kinds_batch(random_kinds(d, 18), 18)
    db = dev(pctx, b)
    try:
        loff, lpkt = U.single_lanes(n_lanes, counts)
        conn = {int(l): U.PEER for l in np.flatnonzero(counts)[::2]}
        conn.update({int(l): U.PEER for l in rng.choice(np.flatnonzero(counts == 0), 100, replace=False)})
        assert 0 in conn
        m = check(pctx, b, db, loff, lpkt, U.peer_table(n_lanes, conn), "4096 lanes")
        assert m.refused > 500 and m.kept > 500
    finally:
        free(db)


def test_fanout_frame_stays_in_the_unconnected_lane(pctx):
    """A frame delivered to a connected and an unconnected socket of one port: the second keeps it
    whatever its source is. Lanes from udpdk_gpu_rx."""
    lists = {abi.raw_port(PA): [(0, 0, 1), (0, 1, 1)], abi.raw_port(PB): [(0, 2, 0)]}
    kinds = [(k[0], PA if i % 3 else PB) for i, k in enumerate(random_kinds(1500, 21))]
    b = kinds_batch(kinds, 21)
    db, meta, loff, lpkt = rx(pctx, lists, b, 3, 2 * b.n)
    try:
        m = check(pctx, b, db, loff, lpkt, U.peer_table(3, {0: U.PEER}), "fan-out")
        l0, l1 = m.lane_pkt[m.lane_off[0]:m.lane_off[1]], m.lane_pkt[m.lane_off[1]:m.lane_off[2]]
        assert np.array_equal(l1, lpkt[loff[1]:loff[2]]) and len(l1) == 1000
        assert list(l0) == [i for i in l1 if kinds[i][0] == U.PEER] and 100 < len(l0) < 400
        assert m.lane_off[3] - m.lane_off[2] == 500
    finally:
        free(db)
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_frame_offsets(pctx, residue):
    """(offset + 26) & 3 at every value, and the batch's last frame ending at frames_bytes with
    frames_bytes % 4 != 0, in a buffer with only the documented tailroom behind it."""
    n = 300
    rng = np.random.default_rng(30 + residue)
    gaps = rng.integers(0, 4, n)
    gaps[-1] += (residue - (int(gaps.sum()) + 26)) % 4               # the last frame's residue
    kinds = random_kinds(n, 31 + residue)
    kinds[-1] = PEER_F
    b = kinds_batch(kinds, 32, gaps=gaps, tail=0)               # (abi.rx_upload adds abi.FRAMES_TAILROOM bytes)
    assert (int(b.offset[-1]) + 26) & 3 == residue and set((b.offset + 26) & 3) == {0, 1, 2, 3}
    assert int(b.offset[-1]) + 64 == b.frames_bytes == len(b.frames)
    assert (b.frames_bytes % 4 != 0) == (residue != 2)
    db = dev(pctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [n])
        m = check(pctx, b, db, loff, lpkt, U.peer_table(1, {0: U.PEER}), f"residue {residue}")
        assert m.lane_pkt[-1] == n - 1 and m.bad_frame == 0
    finally:
        free(db)


def test_bounds(pctx):
    n = 1500
    kinds = random_kinds(n, 40)
    b = kinds_batch(kinds, 40)
    b.length[7::50] = 41                                             # too short for the UDP ports
    b.length[8::50] = 0
    b.offset[9] = b.frames_bytes - 41                                # ends past the batch
    b.offset[10] = 0xFFFFFFF0                                        # offset + length wraps 32 bits
    cut = int(b.offset[-20]) + 63                                    # the last 20 frames end past this
    db = dev(pctx, b)
    peers = U.peer_table(4, {0: U.PEER, 2: U.PEER})
    try:
        loff, lpkt = U.single_lanes(4, [400, 300, 700, 100])
        m = check(pctx, b, db, loff, lpkt, peers, "descriptors")
        assert m.bad_frame == 22 + 22 + 2 and m.keep[400:700].all()  # (lanes 0 and 2 hold 1100 of the 1500)
        db.frames_bytes = cut
        m2 = check(pctx, b, db, loff, lpkt, peers, "frames_bytes cuts the last frames")
        assert m2.bad_frame == m.bad_frame and m2.keep[1480:].all()  # (they are lane 3's: unconnected, not read)
        m3 = check(pctx, b, db, loff, lpkt, U.peer_table(4, {3: U.PEER}), "... of a connected lane")
        assert m3.bad_frame == 20 + 4 and not m3.keep[1480:].any()
        db.frames_bytes = b.frames_bytes
        bad = lpkt.copy()
        bad[5::97] = n + np.arange(len(bad[5::97]))                  # entries >= n
        bad[11] = 0xFFFFFFFF
        m = check(pctx, b, db, loff, bad, peers, "entries >= n")
        assert m.bad_index == len(bad[5::97]) + 1
        check(pctx, b, db, loff, lpkt, peers, "n below the entries", n=n - 300)
        off2 = loff.copy()
        off2[3] = n + 1000                                           # an offset past D
        check(pctx, b, db, off2, lpkt, peers, "offset past D", lane_cap=n)
        off3 = loff.copy()
        off3[4] = n + 12345                                          # total past lane_cap
        m = check(pctx, b, db, off3, lpkt, peers, "truncated", lane_cap=n - 100)
        assert m.truncated == 1
        m = check(pctx, b, db, loff, lpkt, peers, "out_cap", out_cap=500)
        assert m.kept > 500
        check(pctx, b, db, loff, lpkt, peers, "out_cap 0", out_cap=0)
        ident = check(pctx, b, db, loff, bad, U.peer_table(4, {}), "all-off table")
        assert ident.removed == ident.bad_index > 10
    finally:
        free(db)


def test_arguments(pctx):
    L = abi.lib()
    b = kinds_batch(random_kinds(10, 50), 50)
    db = dev(pctx, b)
    loff, lpkt = U.single_lanes(2, [4, 6])
    bufs = [pctx.upload(x) for x in (loff, lpkt, U.peer_table(2, {1: U.PEER}).view(np.uint8),
                                     np.full(3, SENT, np.uint32), np.full(20, SENT, np.uint32))]
    od, pd, rd, oo, po = bufs
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)

    def call(bt_=bt, lanes=None, peer=rd.ptr, off_out=oo.ptr, pkt_out=po.ptr, n_lanes=2, out_cap=20, h=pctx.handle):
        ln = lanes or abi.RxLanes(None, b.n, od.ptr, pd.ptr, len(lpkt), n_lanes)
        return L.udpdk_gpu_rx_peer_select(h, C.byref(bt_) if bt_ else None, C.byref(ln), peer, off_out, pkt_out,
                                          out_cap)

    def untouched():
        pctx.sync()
        return (np.all(pctx.download(oo, np.uint32, 3) == SENT) and np.all(pctx.download(po, np.uint32, 20) == SENT))
    try:
        fresh = abi.GpuContext(0, max_frames=1024, max_lanes=4)
        try:
            st = abi.RxPeerStats()
            assert L.udpdk_gpu_rx_peer_stats(fresh.handle, C.byref(st)) == -errno.ENOENT     # before any run
            assert call(h=fresh.handle) == -errno.EINVAL                                     # no snapshot uploaded
            assert L.udpdk_gpu_rx_peer_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
            t = U.peer_table(5, {0: U.PEER})
            assert L.udpdk_gpu_rx_peer(fresh.handle, t.ctypes.data, 5) == -errno.EINVAL      # past max_lanes
            rs = abi.RxStats()
            r = C.c_uint32()
            assert L.udpdk_gpu_rx_peer_removed(fresh.handle, C.byref(rs), C.byref(r)) == -errno.ENOENT
        finally:
            fresh.close()
        assert call(h=None) == -errno.EINVAL and call(bt_=None) == -errno.EINVAL
        assert L.udpdk_gpu_rx_peer_select(pctx.handle, C.byref(bt), None, rd.ptr, oo.ptr, po.ptr, 20) == -errno.EINVAL
        assert call(peer=None) == -errno.EINVAL and call(off_out=None) == -errno.EINVAL
        assert call(pkt_out=None) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(None, b.n, None, pd.ptr, len(lpkt), 2)) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(None, b.n, od.ptr, None, len(lpkt), 2)) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(None, b.n - 1, od.ptr, pd.ptr, len(lpkt), 2)) == -errno.EINVAL   # n != batch n
        assert call(n_lanes=0) == -errno.EINVAL and call(n_lanes=abi.MAX_LANES + 1) == -errno.EINVAL
        assert call(off_out=od.ptr) == -errno.EINVAL and call(pkt_out=pd.ptr) == -errno.EINVAL   # aliases
        assert call(pkt_out=pd.ptr + 8, out_cap=4) == -errno.EINVAL
        for field in ("frames", "offset", "length"):
            args = dict(frames=db.frames.ptr, offset=db.offset.ptr, length=db.length.ptr)
            args[field] = None
            assert call(bt_=abi.RxBatch(args["frames"], db.frames_bytes, args["offset"], args["length"], None,
                                        b.n)) == -errno.EINVAL, field
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1, lane_mask=0xFF))
        assert call() == -errno.EINVAL                              # compat lanes: not sockfds
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))
        assert untouched()                                          # none of these enqueued anything
        assert call() == 0
        rc, st = abi.rx_peer_stats(pctx)
        m = U.model(b, loff, lpkt, U.peer_table(2, {1: U.PEER}))
        assert rc == 0 and U.stats_tuple(st) == m.stats() and not untouched()
        assert call(lanes=abi.RxLanes(od.ptr, b.n, od.ptr, pd.ptr, len(lpkt), 2)) == 0   # meta given: ignored
    finally:
        for x in bufs:
            x.free()
        free(db)


# ---- sticky mode --------------------------------------------------------------------------------
PEERS_SHAPES = {0: U.PEER, 2: U.PEER, 5: U.STRANGERS[0], 7: U.PEER, 9: U.PEER, 10: U.STRANGERS[1]}


def shapes_batch(seed, n=2500):
    """The mixed edge-case batch with half of the frames' sources rewritten to the peer's or a
    stranger's (their checksums then fail: the drop filter's share)."""
    b = F.mixed_batch(seed, n, [PA, PB, PC], [9, PX], [IP1, IP9])
    rng = np.random.default_rng(seed + 1)
    srcs = [U.PEER, U.PEER] + U.STRANGERS
    for i in np.flatnonzero(b.length >= 42):
        k = int(rng.integers(0, 2 * len(srcs)))
        if k < len(srcs):
            o = int(b.offset[i])
            b.frames[o + 26:o + 30] = UB.ip_bytes(srcs[k][0])
            b.frames[o + 34], b.frames[o + 35] = srcs[k][1] >> 8, srcs[k][1] & 0xFF
    return b


def sticky(ctx, peers=None, rp=None, drop=0):
    ctx.rx_peer(peers)
    ctx.rx_balance(rp)
    ctx.rx_drop(drop)


def test_sticky_equals_explicit_and_off_restores(pctx):
    b = shapes_batch(41)
    peers = U.peer_table(11, PEERS_SHAPES)
    never = abi.GpuContext(0, max_frames=1 << 14, max_lanes=16)     # a context that never had a table
    try:
        ndb, nmeta, nloff, nlpkt = rx(never, LISTS_SHAPES, b, 11, 5 * b.n)
        free(ndb)
    finally:
        never.close()
    db, meta, loff, lpkt = rx(pctx, LISTS_SHAPES, b, 11, 5 * b.n)
    out = abi.rx_alloc_out(pctx, b.n, 11, len(lpkt))
    try:
        assert np.array_equal(loff, nloff) and np.array_equal(lpkt, nlpkt)
        m = check(pctx, b, db, loff, lpkt, peers, "explicit")
        sticky(pctx, peers)
        try:
            gm, gl, gp, gc, rc = abi.rx_run(pctx, db, out)
            prc, pst = abi.rx_peer_stats(pctx)
        finally:
            sticky(pctx)
        assert rc == 0 and prc == 0 and np.array_equal(gm, meta)
        assert np.array_equal(gl, m.lane_off) and np.array_equal(gp, m.lane_pkt)
        assert int(gc[abi.C_DELIVERIES]) == len(lpkt) and len(gp) == m.kept
        assert U.stats_tuple(pst) == m.stats() and m.refused > 300 and m.bad_frame == 0
        # off again (NULL), then an all-off table: bit-identical to the context that never had one
        for table in (None, U.peer_table(11, {})):
            pctx.rx_peer(table)
            gm, gl, gp, gc, rc = abi.rx_run(pctx, db, out)
            assert rc == 0 and np.array_equal(gm, nmeta) and np.array_equal(gl, nloff) and np.array_equal(gp, nlpkt)
        # lane_cap below the total: overflow is the pre-stage total's
        small = abi.rx_alloc_out(pctx, b.n, 11, len(lpkt) - 200)
        sticky(pctx, peers)
        try:
            gm, gl, gp, gc, rc = abi.rx_run(pctx, db, small)
            prc, pst = abi.rx_peer_stats(pctx)
            mt = U.model(b, loff, lpkt, peers, lane_cap=len(lpkt) - 200)
            assert rc == -errno.ENOSPC and pst.truncated == 1
            assert np.array_equal(gl, mt.lane_off) and np.array_equal(gp, mt.lane_pkt)
        finally:
            sticky(pctx)
            for x in (small.meta, small.lane_off, small.lane_pkt):
                x.free()
    finally:
        free(db, out)
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


def test_sticky_with_drop_and_balance_commutes(pctx):
    """Each pair and all three: the call's lanes are the models composed, in either order, and every
    stage's own count is what udpdk_gpu_rx_removed / udpdk_gpu_rx_peer_removed report."""
    b = shapes_batch(43)
    peers = U.peer_table(11, PEERS_SHAPES)
    db, meta, loff, lpkt = rx(pctx, LISTS_SHAPES, b, 11, 5 * b.n)
    out = abi.rx_alloc_out(pctx, b.n, 11, len(lpkt))
    get = LISTS_SHAPES.get

    def drop(lo, lp):
        return UD.model(meta, lo, lp, UD.DROP_ALL)

    def bal(lo, lp):
        return UB.model(get, b, meta, lo, lp, RP_SHAPES)

    def peer(lo, lp):
        return U.model(b, lo, lp, peers)

    def compose(stages):
        lo, lp, removed = loff, lpkt, []
        for f in stages:
            r = f(lo, lp)
            lo, lp = r.lane_off, r.lane_pkt
            removed.append(r.removed)
        return lo, lp, removed
    try:
        for on in ([drop, peer], [bal, peer], [drop, bal, peer]):
            wo, wp, removed = compose(on)                            # the order the context runs them in
            ro, rp_, _ = compose(on[::-1])
            assert np.array_equal(wo, ro) and np.array_equal(wp, rp_) and min(removed) > 50
            sticky(pctx, peers, RP_SHAPES if bal in on else None, abi.RX_DROP_ALL if drop in on else 0)
            try:
                assert abi.rx_enqueue(pctx, db, out) == 0
                rc, st = abi.rx_stats(pctx)
                prc, pst = abi.rx_peer_stats(pctx)
            finally:
                sticky(pctx)
            assert rc == 0 and prc == 0 and st.deliveries == len(wp) == pst.kept
            assert st.counters[abi.C_DELIVERIES] == len(lpkt)
            assert np.array_equal(pctx.download(out.lane_off, np.uint32, 12), wo)
            assert np.array_equal(pctx.download(out.lane_pkt, np.uint32, len(wp)), wp)
            assert np.array_equal(pctx.download(out.meta, np.uint32, b.n), meta)
            dr, ba, rf = C.c_uint32(), C.c_uint32(), C.c_uint32()
            assert abi.lib().udpdk_gpu_rx_removed(pctx.handle, C.byref(st), C.byref(dr), C.byref(ba)) == 0
            assert abi.lib().udpdk_gpu_rx_peer_removed(pctx.handle, C.byref(st), C.byref(rf)) == 0
            want = dict(zip([f.__name__ for f in on], removed))
            assert (dr.value, ba.value, rf.value) == (want.get("drop", 0), want.get("bal", 0), want["peer"])
            assert pst.removed == want["peer"]
    finally:
        free(db, out)
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_sticky_pipeline_depths(pctx, depth):
    bs = [shapes_batch(50 + k, 1500 + 400 * k) for k in range(max(2, depth))]
    peers = U.peer_table(11, PEERS_SHAPES)
    devs, wants = [], []
    try:
        for b in bs:
            db, meta, loff, lpkt = rx(pctx, LISTS_SHAPES, b, 11, 5 * b.n)
            devs.append((db, abi.rx_alloc_out(pctx, b.n, 11, len(lpkt))))
            wants.append((meta, U.model(b, loff, lpkt, peers)))
        pctx.pipeline(depth)
        pctx.rx_peer(peers)
        try:
            for _ in range(2):
                for db, out in devs:
                    assert abi.rx_enqueue(pctx, db, out) == 0
            rc, st = abi.rx_stats(pctx)
            pctx.sync()
        finally:
            pctx.rx_peer(None)
            pctx.pipeline(1)
        for k, ((db, out), (meta, m)) in enumerate(zip(devs, wants)):
            assert np.array_equal(pctx.download(out.meta, np.uint32, out.n), meta), k
            assert np.array_equal(pctx.download(out.lane_off, np.uint32, 12), m.lane_off), k
            assert np.array_equal(pctx.download(out.lane_pkt, np.uint32, m.kept), m.lane_pkt), k
        assert rc == 0 and st.deliveries == wants[-1][1].kept
    finally:
        for db, out in devs:
            free(db, out)
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


def test_sticky_host_calls(pctx):
    """udpdk_gpu_rx_host, udpdk_gpu_rx_host_async (depths 1 and 3) and udpdk_gpu_pipe_rx_host: equal
    to udpdk_gpu_rx followed by the explicit call."""
    L = abi.lib()
    b = shapes_batch(61, 2000)
    peers = U.peer_table(11, PEERS_SHAPES)
    db, meta, loff, lpkt = rx(pctx, LISTS_SHAPES, b, 11, 5 * b.n)
    try:
        m = check(pctx, b, db, loff, lpkt, peers, "explicit")
    finally:
        free(db)
    cap = 5 * b.n

    def call(fn, depth, reps):
        pctx.pipeline(depth)
        res = []
        try:
            for r in range(reps):
                gm, gl, gp = np.zeros(b.n, np.uint32), np.zeros(12, np.uint32), np.zeros(cap, np.uint32)
                st = abi.RxStats()
                args = (b.frames.ctypes.data, b.frames_bytes, b.offset.ctypes.data)
                tail = (b.length.ctypes.data, None, b.n, gm.ctypes.data, gl.ctypes.data, gp.ctypes.data, cap, C.byref(st))
                if fn is L.udpdk_gpu_pipe_rx_host:
                    assert fn(pctx.handle, 1 + r % 3, *args, 0, *tail) == 0
                    assert L.udpdk_gpu_pipe_wait(pctx.handle, 1 + r % 3) == 0
                else:
                    assert fn(pctx.handle, *args, *tail) == 0
                res.append((gm, gl, gp, st))
            if fn is L.udpdk_gpu_rx_host_async:
                assert L.udpdk_gpu_rx_host_wait(pctx.handle) == 0
        finally:
            pctx.pipeline(1)
        return res
    try:
        for fn, depth in ((L.udpdk_gpu_rx_host, 1), (L.udpdk_gpu_rx_host_async, 1), (L.udpdk_gpu_rx_host_async, 3),
                          (L.udpdk_gpu_pipe_rx_host, 1)):
            pctx.rx_peer(peers)
            try:
                res = call(fn, depth, 3)
            finally:
                pctx.rx_peer(None)
            for gm, gl, gp, st in res:
                assert np.array_equal(gm, meta) and np.array_equal(gl, m.lane_off)
                assert st.deliveries == m.kept and st.overflow == 0 and st.counters[abi.C_DELIVERIES] == len(lpkt)
                assert np.array_equal(gp[:m.kept], m.lane_pkt)
            for gm, gl, gp, st in call(fn, depth, 1):                  # off again
                assert np.array_equal(gl, loff) and np.array_equal(gp[:st.deliveries], lpkt)
    finally:
        pctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))
