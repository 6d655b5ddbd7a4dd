"""The multicast membership filter on the GPU (udpdk_gpu_rx_mcast_select, udpdk_gpu_rx_mcast)
against the model of mcast_util.py, which test_mcast_ref.py pins to hand-written vectors: lane_off,
lane_pkt and every stats field, exactly. The explicit call takes any lane set, so most shapes are
built by hand on the kernel's boundaries (the 64-entry chunk, the 256-entry wave, the 1024-entry
tile); the fan-out and sticky tests take their lanes from udpdk_gpu_rx itself (pinned to the oracle
by test_gpu_rx.py)."""
import ctypes as C
import errno

import numpy as np
import pytest

import mcast_util as U
import rx_balance_util as UB
import rx_drop_util as UD
import rx_peer_util as UP
from test_gpu_rx import IP1, IP9
from test_gpu_rx_balance import LISTS_SHAPES, PA, PB, PC, PX, RP_SHAPES, free, rx
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

E = 1024                    # entries per compaction tile (FLT_TILE, rx_filter.h)
SENT = 0xA5A5A5A5
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]       # chunk, wave, tile
KINDS = list(U.KINDS.values())
MULTI = [U.KINDS[k] for k in ("other", "low", "high")]                   # groups lane 0 did not join
ONE = {abi.raw_port(PA): [(0, 0, 0)]}
RG1, RG2 = abi.raw_ip(U.G1), abi.raw_ip(U.G2)
TAB1 = U.build([(RG1, 0)], 2)                                            # lane 0 joined G1


@pytest.fixture(scope="module")
def mctx():
    ctx = abi.GpuContext(0, max_frames=1 << 17, max_lanes=4096)
    ctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))         # (the explicit call wants sockfd lanes)
    yield ctx
    ctx.close()


def random_dsts(n, seed):
    return [KINDS[int(k)] for k in np.random.default_rng(seed).integers(0, len(KINDS), n)]


def dev(ctx, b):
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, None)
    db.frames_bytes = b.frames_bytes
    return db


def check(ctx, b, db, loff, lpkt, lane_mc, tab, what, **kw):
    mk = {k: v for k, v in kw.items() if k in ("n", "lane_cap")}
    m = U.model(b, loff, lpkt, lane_mc, tab, frames_bytes=db.frames_bytes, **mk)
    go, gp, st, rc = abi.rx_mcast_run(ctx, db, loff, lpkt, lane_mc, U.as_records(tab), pad=8, **kw)
    out_cap = len(gp) - 8
    assert np.array_equal(go, m.lane_off), f"{what}: lane_off"
    w = min(m.kept, out_cap)
    assert np.array_equal(gp[:w], m.lane_pkt[:w]), f"{what}: lane entries"
    assert np.all(gp[w:] == SENT), f"{what}: wrote past the kept entries"
    assert U.stats_tuple(st) == m.stats(), what
    assert rc == (-errno.ENOSPC if m.kept > out_cap else 0), what
    return m


def gone(dsts):
    """How many of these destinations a checked lane that joined G1 alone loses."""
    return sum(d in MULTI for d in dsts)


# ---- the explicit call --------------------------------------------------------------------------
@pytest.mark.parametrize("d", COUNTS)
def test_entry_counts_one_lane(mctx, d):
    dsts = random_dsts(max(1, d), 100 + d)
    b = U.frames_to(dsts, PA, d)
    db = dev(mctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [d])
        m = check(mctx, b, db, loff, np.resize(lpkt, max(1, d)), [1], TAB1, f"d={d}", lane_cap=d)
        assert m.not_member == gone(dsts[:d]) and m.member == sum(x == U.G1 for x in dsts[:d])
        assert m.kept == d - m.not_member
        ident = check(mctx, b, db, loff, np.resize(lpkt, max(1, d)), [0], TAB1, f"exempt d={d}", lane_cap=d)
        assert ident.kept == d and ident.member == 0
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
            dsts = random_dsts(d, 900 + step)
            b = U.frames_to(dsts, PA, 900 + step)
            db = dev(ctx, b)
            try:
                loff, lpkt = U.single_lanes(1, [d])
                m = check(ctx, b, db, loff, lpkt, [1], TAB1, f"step {step} d={d}")
                assert m.not_member == gone(dsts) > 0
            finally:
                free(db)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["other", "low", "high"])
def test_kinds_at_chunk_and_tile_edges(mctx, kind):
    """Each group the lane did not join, alone, at the first and the last entry of chunks (also the
    ones that end a wave and a tile); every other entry is one the lane keeps, of every kept kind."""
    d = E + 128
    at = [0, 63, 64, 127, 255, 256, E - 1, E, E + 63, E + 64, d - 1]
    keepers = [U.KINDS[k] for k in ("member", "unicast", "bcast", "b223", "b240")]
    dsts = [keepers[p % 5] for p in range(d)]
    for p in at:
        dsts[p] = U.KINDS[kind]
    b = U.frames_to(dsts, PA, 7)
    db = dev(mctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [d])
        m = check(mctx, b, db, loff, lpkt, [1], TAB1, kind)
        assert m.not_member == len(at) and list(np.flatnonzero(~m.keep)) == at
        # and the other way round: a lane that joined that group alone loses the G1 entries instead
        tab = U.build([(abi.raw_ip(U.KINDS[kind]), 0)], 2)
        m = check(mctx, b, db, loff, lpkt, [1], tab, kind + " inverse")
        assert m.member == len(at) and m.not_member == sum(x == U.G1 for x in dsts)
    finally:
        free(db)


@pytest.fixture(scope="module")
def two_lane_batch(mctx):
    d = 2 * E + 252
    b = U.frames_to(random_dsts(d, 5), PA, 5)
    db = dev(mctx, b)
    yield b, db, d
    free(db)


@pytest.mark.parametrize("checked", [0, 1])
@pytest.mark.parametrize("bnd", COUNTS)
def test_two_lanes_boundary(mctx, two_lane_batch, bnd, checked):
    """The lane boundary at every count, inside a wave and on a tile edge; either side checked. Both
    lanes joined G1 in the table: the exempt one is not looked up."""
    b, db, d = two_lane_batch
    loff, lpkt = U.single_lanes(2, [bnd, d - bnd])
    mc = [0, 0]
    mc[checked] = 1
    m = check(mctx, b, db, loff, lpkt, mc, U.build([(RG1, 0), (RG1, 1)], 4), f"bnd={bnd} checked={checked}")
    lo, hi = (0, bnd) if checked == 0 else (bnd, d)
    assert m.removed == int((~m.keep[lo:hi]).sum()) and m.keep[:lo].all() and m.keep[hi:].all()


def test_alternating_lanes_with_their_own_groups(mctx):
    """Checked and exempt lanes alternate, every checked lane in a group of its own (so a lookup
    under a neighbour's lane shows), one of them empty; lane sizes off every boundary."""
    counts = [37, 5, 64, 1, 200, 0, 65, 63, 0, 256, 300, 3, 129, 64, 1, 700]
    groups = [f"239.7.{l}.1" for l in range(16)]
    d = sum(counts)
    lane_of = np.repeat(np.arange(16), counts)
    rng = np.random.default_rng(3)
    # an entry's destination: its lane's group, the group of the lane two further on, or unicast
    pick = rng.integers(0, 3, d)
    dsts = [groups[l] if k == 0 else groups[(l + 2) % 16] if k == 1 else U.OUR_IP for l, k in zip(lane_of, pick)]
    b = U.frames_to(dsts, PA, 11, gaps=rng.integers(0, 4, d))
    db = dev(mctx, b)
    try:
        loff, lpkt = U.single_lanes(16, counts)
        mc = [1 - l % 2 for l in range(16)]
        assert counts[8] == 0 and mc[8]                               # a checked lane that is empty
        members = [(abi.raw_ip(groups[l]), l) for l in range(16)]     # (the exempt lanes' are never read)
        m = check(mctx, b, db, loff, lpkt, mc, U.build(members, 32), "alternating")
        want = (lane_of % 2 == 1) | (pick != 1)
        assert np.array_equal(m.keep, want) and m.not_member == int((~want).sum()) > 200
    finally:
        free(db)


def test_4096_lanes_mostly_empty(mctx):
    n_lanes = 4096
    rng = np.random.default_rng(17)
    live = np.sort(rng.choice(n_lanes, 48, replace=False))
    counts = np.zeros(n_lanes, np.int64)
    counts[live] = rng.integers(1, 140, len(live))
    counts[[0, n_lanes - 1]] = [3, 70]
    d = int(counts.sum())
    b = U.frames_to(random_dsts(d, 18), PA, 18)
    db = dev(mctx, b)
    try:
        loff, lpkt = U.single_lanes(n_lanes, counts)
        mc = np.zeros(n_lanes, np.uint8)
        mc[np.flatnonzero(counts)[::2]] = 1
        mc[rng.choice(np.flatnonzero(counts == 0), 100, replace=False)] = 1
        assert mc[0]
        members = [(RG1, int(l)) for l in np.flatnonzero(mc)[::2]] + [(RG2, int(l)) for l in np.flatnonzero(mc)[1::3]]
        m = check(mctx, b, db, loff, lpkt, mc, U.build(members, U.slots_for(len(members))), "4096 lanes")
        assert m.not_member > 300 and m.member > 50 and m.kept > 500
    finally:
        free(db)


def test_fanout_frame_stays_in_the_joined_lane(mctx):
    """A frame delivered to a joined and an unjoined socket of one port stays in the first only;
    unicast stays in both. Lanes from udpdk_gpu_rx."""
    lists = {abi.raw_port(PA): [(0, 0, 1), (0, 1, 1)], abi.raw_port(PB): [(0, 2, 0)]}
    dsts = [U.G1 if i % 2 else U.G2 if i % 5 == 0 else U.OUR_IP for i in range(1500)]
    b = U.frames_to(dsts, [PA if i % 3 else PB for i in range(1500)], 21)
    db, meta, loff, lpkt = rx(mctx, lists, b, 3, 2 * b.n)
    try:
        assert np.array_equal(lpkt[loff[0]:loff[1]], lpkt[loff[1]:loff[2]]) and loff[1] == 1000   # the fan-out
        m = check(mctx, b, db, loff, lpkt, [1, 1, 1], U.build([(RG1, 0), (RG2, 2)], 4), "fan-out")
        l0, l1 = m.lane_pkt[m.lane_off[0]:m.lane_off[1]], m.lane_pkt[m.lane_off[1]:m.lane_off[2]]
        l2 = m.lane_pkt[m.lane_off[2]:m.lane_off[3]]
        assert list(l0) == [i for i in range(1500) if i % 3 and dsts[i] != U.G2]
        assert list(l1) == [i for i in range(1500) if i % 3 and dsts[i] == U.OUR_IP]
        assert list(l2) == [i for i in range(1500) if i % 3 == 0 and dsts[i] != U.G1]
        assert m.member > 400 and len(l1) > 100
    finally:
        free(db)
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_frame_offsets(mctx, residue):
    """(offset + 30) & 3 at every value, and the batch's last frame ending at frames_bytes with
    frames_bytes % 4 != 0, in a buffer with only the documented tailroom behind it."""
    n = 300
    rng = np.random.default_rng(30 + residue)
    gaps = rng.integers(0, 4, n)
    gaps[-1] += (residue - (int(gaps.sum()) + 30)) % 4               # the last frame's residue
    dsts = random_dsts(n, 31 + residue)
    dsts[-1] = U.G1
    b = U.frames_to(dsts, PA, 32, gaps=gaps, tail=0)            # (abi.rx_upload adds abi.FRAMES_TAILROOM bytes)
    assert (int(b.offset[-1]) + 30) & 3 == residue and set((b.offset + 30) & 3) == {0, 1, 2, 3}
    assert int(b.offset[-1]) + 64 == b.frames_bytes == len(b.frames)
    assert (b.frames_bytes % 4 != 0) == (residue != 2)
    db = dev(mctx, b)
    try:
        loff, lpkt = U.single_lanes(1, [n])
        m = check(mctx, b, db, loff, lpkt, [1], TAB1, f"residue {residue}")
        assert m.lane_pkt[-1] == n - 1 and m.bad_frame == 0 and m.not_member == gone(dsts)
        # the shortest frame the stage reads, last in the batch: nothing of it lies past byte 42
        b.length[-1] = 42
        cut = int(b.offset[-1]) + 42
        fr = abi.rx_upload(mctx, b.frames[:cut], b.offset, b.length, None)
        fr.frames_bytes = cut
        try:
            m = check(mctx, b, fr, loff, lpkt, [1], TAB1, f"residue {residue}, 42-byte last frame")
            assert m.lane_pkt[-1] == n - 1 and m.bad_frame == 0
        finally:
            free(fr)
    finally:
        free(db)


def test_tables(mctx):
    """Two slots, a chain that wraps past the last slot, and a table with no empty slot (a miss
    ends after `slots` probes): golden/mcast_vectors.json's tables on the device."""
    groups = [U.G1, U.G2, U.G3, "239.9.9.9"]
    n = 400
    rng = np.random.default_rng(60)
    dsts = [groups[int(k)] for k in rng.integers(0, 4, n)]
    b = U.frames_to(dsts, PA, 60)
    db = dev(mctx, b)
    try:
        n_lanes = 32
        order = rng.integers(0, n, 1600)
        counts = np.bincount(rng.integers(0, n_lanes, 1600), minlength=n_lanes)
        loff, lpkt = U.single_lanes(n_lanes, counts, order)
        mc = np.ones(n_lanes, np.uint8)
        wrap = [(RG1, 4), (RG1, 15), (RG1, 25)]                     # all start in slot 7 of 8
        assert [U.start(g, l, 8) for g, l in wrap] == [7, 7, 7]
        full8 = wrap + [(RG2, l) for l in (4, 5, 6)] + [(abi.raw_ip(U.G3), 25), (abi.raw_ip(U.G3), 31)]
        for members, slots in (([(RG1, 3)], 2), ([(RG1, 0), (RG1, 3)], 2), (wrap, 8), (full8, 8), ([], 2),
                               ([(RG1, l) for l in range(32)], 32)):
            tab = U.build(members, slots)
            if len(members) == slots:
                assert all(t[0] for t in tab)
            m = check(mctx, b, db, loff, lpkt, mc, tab, f"{len(members)} members in {slots} slots")
            lane_of = np.repeat(np.arange(n_lanes), counts)
            want = sum((abi.raw_ip(dsts[i]), int(l)) in members for i, l in zip(order, lane_of))
            assert m.member == want and m.member + m.not_member == 1600
    finally:
        free(db)


def test_bounds(mctx):
    n = 1500
    dsts = random_dsts(n, 40)
    b = U.frames_to(dsts, PA, 40)
    b.length[7::50] = 41                                             # too short for a UDP header
    b.length[8::50] = 0
    b.offset[9] = b.frames_bytes - 41                                # ends past the batch
    b.offset[10] = 0xFFFFFFF0                                        # offset + length wraps 32 bits
    cut = int(b.offset[-20]) + 63                                    # the last 20 frames end past this
    db = dev(mctx, b)
    mc = [1, 0, 1, 0]
    tab = U.build([(RG1, 0), (RG2, 2), (RG1, 3)], 8)
    try:
        loff, lpkt = U.single_lanes(4, [400, 300, 700, 100])
        m = check(mctx, b, db, loff, lpkt, mc, tab, "descriptors")
        assert m.bad_frame == 22 + 22 + 2 and m.keep[400:700].all()  # (lanes 0 and 2 hold 1100 of the 1500)
        db.frames_bytes = cut
        m2 = check(mctx, b, db, loff, lpkt, mc, tab, "frames_bytes cuts the last frames")
        assert m2.bad_frame == m.bad_frame and m2.keep[1480:].all()  # (they are lane 3's: exempt, not read)
        m3 = check(mctx, b, db, loff, lpkt, [0, 0, 0, 1], tab, "... of a checked lane")
        assert m3.bad_frame == 20 + 4 and not m3.keep[1480:].any()
        db.frames_bytes = b.frames_bytes
        bad = lpkt.copy()
        bad[5::97] = n + np.arange(len(bad[5::97]))                  # entries >= n
        bad[11] = 0xFFFFFFFF
        m = check(mctx, b, db, loff, bad, mc, tab, "entries >= n")
        assert m.bad_index == len(bad[5::97]) + 1
        check(mctx, b, db, loff, lpkt, mc, tab, "n below the entries", n=n - 300)
        off2 = loff.copy()
        off2[3] = n + 1000                                           # an offset past D
        check(mctx, b, db, off2, lpkt, mc, tab, "offset past D", lane_cap=n)
        off3 = loff.copy()
        off3[4] = n + 12345                                          # total past lane_cap
        m = check(mctx, b, db, off3, lpkt, mc, tab, "truncated", lane_cap=n - 100)
        assert m.truncated == 1
        full = check(mctx, b, db, loff, lpkt, mc, tab, "out_cap = lane_cap")
        m = check(mctx, b, db, loff, lpkt, mc, tab, "out_cap short by one", out_cap=full.kept - 1)
        assert m.kept == full.kept
        check(mctx, b, db, loff, lpkt, mc, tab, "out_cap exact", out_cap=full.kept)
        check(mctx, b, db, loff, lpkt, mc, tab, "out_cap 0", out_cap=0)
        ident = check(mctx, b, db, loff, bad, [0] * 4, tab, "all-zero lane_mc")
        assert ident.removed == ident.bad_index > 10
    finally:
        free(db)


def test_arguments(mctx):
    L = abi.lib()
    dsts = random_dsts(10, 50)
    b = U.frames_to(dsts, PA, 50)
    db = dev(mctx, b)
    loff, lpkt = U.single_lanes(2, [4, 6])
    tab = U.build([(RG1, 1)], 2)
    bufs = [mctx.upload(x) for x in (loff, lpkt, np.array([0, 1], np.uint8), U.as_records(tab).view(np.uint8),
                                     np.full(3, SENT, np.uint32), np.full(20, SENT, np.uint32))]
    od, pd, md, td, oo, po = bufs
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)

    def call(bt_=bt, lanes=None, mc=md.ptr, table=td.ptr, slots=2, off_out=oo.ptr, pkt_out=po.ptr, n_lanes=2,
             out_cap=20, h=mctx.handle):
        ln = lanes or abi.RxLanes(None, b.n, od.ptr, pd.ptr, len(lpkt), n_lanes)
        return L.udpdk_gpu_rx_mcast_select(h, C.byref(bt_) if bt_ else None, C.byref(ln), mc, table, slots, off_out,
                                           pkt_out, out_cap)

    def untouched():
        mctx.sync()
        return (np.all(mctx.download(oo, np.uint32, 3) == SENT) and np.all(mctx.download(po, np.uint32, 20) == SENT))
    try:
        fresh = abi.GpuContext(0, max_frames=1024, max_lanes=4)
        try:
            st = abi.RxMcastStats()
            assert L.udpdk_gpu_rx_mcast_stats(fresh.handle, C.byref(st)) == -errno.ENOENT     # before any run
            assert call(h=fresh.handle) == -errno.EINVAL                                      # no snapshot uploaded
            assert L.udpdk_gpu_rx_mcast_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
            mc5 = np.ones(5, np.uint8)
            assert L.udpdk_gpu_rx_mcast(fresh.handle, mc5.ctypes.data, 5, None, 0) == -errno.EINVAL   # past max_lanes
            mem = np.array([(RG1, 1), (RG1, 1)], U.MCAST_DTYPE)
            assert L.udpdk_gpu_rx_mcast(fresh.handle, mc5.ctypes.data, 4, mem.ctypes.data, 2) == -errno.EINVAL  # twice
            mem = np.array([(RG1, 4)], U.MCAST_DTYPE)
            assert L.udpdk_gpu_rx_mcast(fresh.handle, mc5.ctypes.data, 4, mem.ctypes.data, 1) == -errno.EINVAL  # lane
            assert L.udpdk_gpu_rx_mcast(fresh.handle, mc5.ctypes.data, 4, None, 1) == -errno.EINVAL
            assert L.udpdk_gpu_rx_mcast(fresh.handle, mc5.ctypes.data, 4, mem.ctypes.data, (1 << 19) + 1) == -errno.EINVAL
            rs = abi.RxStats()
            r = C.c_uint32()
            assert L.udpdk_gpu_rx_mcast_removed(fresh.handle, C.byref(rs), C.byref(r)) == -errno.ENOENT
        finally:
            fresh.close()
        assert call(h=None) == -errno.EINVAL and call(bt_=None) == -errno.EINVAL
        assert L.udpdk_gpu_rx_mcast_select(mctx.handle, C.byref(bt), None, md.ptr, td.ptr, 2, oo.ptr, po.ptr,
                                           20) == -errno.EINVAL
        assert call(mc=None) == -errno.EINVAL and call(table=None) == -errno.EINVAL
        assert call(table=td.ptr + 4) == -errno.EINVAL                                         # 8-byte records
        for slots in (0, 1, 3, 6, (1 << 20) + 1, 1 << 21):
            assert call(slots=slots) == -errno.EINVAL, slots
        assert call(off_out=None) == -errno.EINVAL and call(pkt_out=None) == -errno.EINVAL
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
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1, lane_mask=0xFF))
        assert call() == -errno.EINVAL                              # compat lanes: not sockfds
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))
        assert untouched()                                          # none of these enqueued anything
        assert call() == 0
        rc, st = abi.rx_mcast_stats(mctx)
        m = U.model(b, loff, lpkt, [0, 1], tab)
        assert rc == 0 and U.stats_tuple(st) == m.stats() and not untouched()
        assert call(lanes=abi.RxLanes(od.ptr, b.n, od.ptr, pd.ptr, len(lpkt), 2)) == 0   # meta given: ignored
    finally:
        for x in bufs:
            x.free()
        free(db)


# ---- sticky mode --------------------------------------------------------------------------------
MC_SHAPES = [1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0]        # the ANY sockets of LISTS_SHAPES (0, 9) and one bound to IP1
MEMBERS_SHAPES = [(RG1, 0), (RG2, 9), (RG2, 1)]      # (socket 1 never sees a group: bound to a unicast address)
# socket 9 is connected to the batch's own sender, so the peer filter leaves it the frames whose
# source shapes_batch did not rewrite; socket 0 stays unconnected
PEERS_SHAPES = {2: UP.PEER, 5: UP.STRANGERS[0], 7: UP.PEER, 9: (F.IP_SRC, F.UDP_SRC), 10: UP.STRANGERS[1]}


def shapes_batch(seed, n=2500):
    """The mixed edge-case batch to our addresses and to the two groups, with half of the frames'
    sources rewritten to the peer's or a stranger's (their checksums then fail: the drop filter's
    share)."""
    b = F.mixed_batch(seed, n, [PA, PB, PC], [9, PX], [IP1, IP9, U.G1, U.G2])
    rng = np.random.default_rng(seed + 1)
    srcs = [UP.PEER, UP.PEER] + UP.STRANGERS
    for i in np.flatnonzero(b.length >= 42):
        k = int(rng.integers(0, 2 * len(srcs)))
        if k < len(srcs):
            o = int(b.offset[i])
            b.frames[o + 26:o + 30] = UB.ip_bytes(srcs[k][0])
            b.frames[o + 34], b.frames[o + 35] = srcs[k][1] >> 8, srcs[k][1] & 0xFF
    return b


def sticky(ctx, mc=None, members=None, peers=None, rp=None, drop=0):
    ctx.rx_mcast(mc, members)
    ctx.rx_peer(peers)
    ctx.rx_balance(rp)
    ctx.rx_drop(drop)


def members_records():
    return np.array(MEMBERS_SHAPES, U.MCAST_DTYPE)


def sticky_table():
    return U.build(MEMBERS_SHAPES, U.slots_for(len(MEMBERS_SHAPES)))


def test_sticky_equals_explicit_and_off_restores(mctx):
    b = shapes_batch(41)
    never = abi.GpuContext(0, max_frames=1 << 14, max_lanes=16)     # a context that never had a table
    try:
        ndb, nmeta, nloff, nlpkt = rx(never, LISTS_SHAPES, b, 11, 5 * b.n)
        free(ndb)
    finally:
        never.close()
    db, meta, loff, lpkt = rx(mctx, LISTS_SHAPES, b, 11, 5 * b.n)
    out = abi.rx_alloc_out(mctx, b.n, 11, len(lpkt))
    try:
        assert np.array_equal(loff, nloff) and np.array_equal(lpkt, nlpkt)
        m = check(mctx, b, db, loff, lpkt, MC_SHAPES, sticky_table(), "explicit")
        sticky(mctx, MC_SHAPES, members_records())
        try:
            gm, gl, gp, gc, rc = abi.rx_run(mctx, db, out)
            prc, pst = abi.rx_mcast_stats(mctx)
        finally:
            sticky(mctx)
        assert rc == 0 and prc == 0 and np.array_equal(gm, meta)
        assert np.array_equal(gl, m.lane_off) and np.array_equal(gp, m.lane_pkt)
        assert int(gc[abi.C_DELIVERIES]) == len(lpkt) and len(gp) == m.kept
        assert U.stats_tuple(pst) == m.stats() and m.not_member > 100 and m.member > 50 and m.bad_frame == 0
        # checked lanes and no member at all: every multicast entry of theirs goes
        m0 = U.model(b, loff, lpkt, MC_SHAPES, U.build([], 2))
        mctx.rx_mcast(MC_SHAPES, None)
        try:
            gm, gl, gp, gc, rc = abi.rx_run(mctx, db, out)
        finally:
            sticky(mctx)
        assert rc == 0 and np.array_equal(gl, m0.lane_off) and np.array_equal(gp, m0.lane_pkt) and m0.member == 0
        # off again (NULL), then an all-zero lane_mc: bit-identical to the context that never had one
        for mc in (None, [0] * 11):
            mctx.rx_mcast(mc, members_records())
            gm, gl, gp, gc, rc = abi.rx_run(mctx, db, out)
            assert rc == 0 and np.array_equal(gm, nmeta) and np.array_equal(gl, nloff) and np.array_equal(gp, nlpkt)
        # lane_cap below the total: overflow is the pre-stage total's
        small = abi.rx_alloc_out(mctx, b.n, 11, len(lpkt) - 200)
        sticky(mctx, MC_SHAPES, members_records())
        try:
            gm, gl, gp, gc, rc = abi.rx_run(mctx, db, small)
            prc, pst = abi.rx_mcast_stats(mctx)
            mt = U.model(b, loff, lpkt, MC_SHAPES, sticky_table(), lane_cap=len(lpkt) - 200)
            assert rc == -errno.ENOSPC and pst.truncated == 1
            assert np.array_equal(gl, mt.lane_off) and np.array_equal(gp, mt.lane_pkt)
        finally:
            sticky(mctx)
            for x in (small.meta, small.lane_off, small.lane_pkt):
                x.free()
    finally:
        free(db, out)
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


@pytest.mark.parametrize("depth", [1, 3])
def test_sticky_with_drop_balance_and_peer_commutes(mctx, depth):
    """The membership filter with each other stage and with all three, at pipeline depths 1 and 3:
    the call's lanes are the models composed, in either order, and every stage's own count is what
    udpdk_gpu_rx_removed / _peer_removed / _mcast_removed report."""
    b = shapes_batch(43, 4000)
    peers = UP.peer_table(11, PEERS_SHAPES)
    db, meta, loff, lpkt = rx(mctx, LISTS_SHAPES, b, 11, 5 * b.n)
    outs = [abi.rx_alloc_out(mctx, b.n, 11, len(lpkt)) for _ in range(depth)]
    get = LISTS_SHAPES.get
    tab = sticky_table()

    def drop(lo, lp):
        return UD.model(meta, lo, lp, UD.DROP_ALL)

    def bal(lo, lp):
        return UB.model(get, b, meta, lo, lp, RP_SHAPES)

    def peer(lo, lp):
        return UP.model(b, lo, lp, peers)

    def mcast(lo, lp):
        return U.model(b, lo, lp, MC_SHAPES, tab)

    def compose(stages):
        lo, lp, removed = loff, lpkt, []
        for f in stages:
            r = f(lo, lp)
            lo, lp = r.lane_off, r.lane_pkt
            removed.append(r.removed)
        return lo, lp, removed
    mctx.pipeline(depth)
    try:
        for on in ([mcast], [drop, mcast], [bal, mcast], [peer, mcast], [drop, bal, peer, mcast]):
            wo, wp, removed = compose(on)                            # the order the context runs them in
            ro, rp_, _ = compose(on[::-1])
            assert np.array_equal(wo, ro) and np.array_equal(wp, rp_) and min(removed) > 20
            sticky(mctx, MC_SHAPES, members_records(), peers if peer in on else None,
                   RP_SHAPES if bal in on else None, abi.RX_DROP_ALL if drop in on else 0)
            try:
                for out in outs:
                    assert abi.rx_enqueue(mctx, db, out) == 0
                rc, st = abi.rx_stats(mctx)
                prc, pst = abi.rx_mcast_stats(mctx)
                mctx.sync()
            finally:
                sticky(mctx)
            assert rc == 0 and prc == 0 and st.deliveries == len(wp) == pst.kept
            assert st.counters[abi.C_DELIVERIES] == len(lpkt)
            for out in outs:
                assert np.array_equal(mctx.download(out.lane_off, np.uint32, 12), wo)
                assert np.array_equal(mctx.download(out.lane_pkt, np.uint32, len(wp)), wp)
                assert np.array_equal(mctx.download(out.meta, np.uint32, b.n), meta)
            dr, ba, rf, nm = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
            assert abi.lib().udpdk_gpu_rx_removed(mctx.handle, C.byref(st), C.byref(dr), C.byref(ba)) == 0
            assert abi.lib().udpdk_gpu_rx_peer_removed(mctx.handle, C.byref(st), C.byref(rf)) == 0
            assert abi.lib().udpdk_gpu_rx_mcast_removed(mctx.handle, C.byref(st), C.byref(nm)) == 0
            want = dict(zip([f.__name__ for f in on], removed))
            assert (dr.value, ba.value, rf.value, nm.value) == \
                (want.get("drop", 0), want.get("bal", 0), want.get("peer", 0), want["mcast"])
            assert pst.removed == want["mcast"]
    finally:
        mctx.pipeline(1)
        free(db, outs[0])
        for out in outs[1:]:
            for x in (out.meta, out.lane_off, out.lane_pkt):
                x.free()
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))


def test_sticky_host_calls(mctx):
    """udpdk_gpu_rx_host and udpdk_gpu_rx_host_async at depth 3: equal to udpdk_gpu_rx followed by
    the explicit call."""
    L = abi.lib()
    b = shapes_batch(61, 2000)
    db, meta, loff, lpkt = rx(mctx, LISTS_SHAPES, b, 11, 5 * b.n)
    try:
        m = check(mctx, b, db, loff, lpkt, MC_SHAPES, sticky_table(), "explicit")
    finally:
        free(db)
    cap = 5 * b.n
    try:
        for fn, depth in ((L.udpdk_gpu_rx_host, 1), (L.udpdk_gpu_rx_host_async, 3)):
            mctx.pipeline(depth)
            mctx.rx_mcast(MC_SHAPES, members_records())
            res = []
            try:
                for _ in range(3):
                    gm, gl, gp = np.zeros(b.n, np.uint32), np.zeros(12, np.uint32), np.zeros(cap, np.uint32)
                    st = abi.RxStats()
                    assert fn(mctx.handle, b.frames.ctypes.data, b.frames_bytes, b.offset.ctypes.data,
                              b.length.ctypes.data, None, b.n, gm.ctypes.data, gl.ctypes.data, gp.ctypes.data, cap,
                              C.byref(st)) == 0
                    res.append((gm, gl, gp, st))
                if fn is L.udpdk_gpu_rx_host_async:
                    assert L.udpdk_gpu_rx_host_wait(mctx.handle) == 0
            finally:
                mctx.rx_mcast(None)
                mctx.pipeline(1)
            for gm, gl, gp, st in res:
                assert np.array_equal(gm, meta) and np.array_equal(gl, m.lane_off)
                assert st.deliveries == m.kept and st.overflow == 0 and st.counters[abi.C_DELIVERIES] == len(lpkt)
                assert np.array_equal(gp[:m.kept], m.lane_pkt)
    finally:
        mctx.upload_snapshot(abi.snapshot_from_lists(ONE, 1))
