"""The reuse-port balance stage on the GPU (udpdk_gpu_rx_balance_select, udpdk_gpu_rx_balance, the
socket layer's [gpu] reuseport = balance) against the model of rx_balance_util.py, which
test_rx_balance_ref.py pins to the oracle. The lanes and verdict words the stage works on come from
udpdk_gpu_rx itself (pinned to the oracle by test_gpu_rx.py); every test also checks that the
model's walk makes exactly those deliveries."""
import ctypes as C
import errno
from types import SimpleNamespace

import numpy as np
import pytest

import rss_util as R
import rx_balance_util as U
import rx_drop_util as UD
from reasm_util import batch, split, udp_datagram
from test_gpu_rx import IP1, IP9
from test_rx_balance_ref import SEED_FLOWS
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

E = 1024                    # entries per compaction tile (FLT_TILE, rx_filter.h)
T = abi.BAL_TILE            # frames per rx_balance_pick workgroup
SENT = 0xA5A5A5A5
PA, PB, PC, PX = 10001, 10002, 10003, 20000      # PX: never bound
RIP1, RIP9 = abi.raw_ip(IP1), abi.raw_ip(IP9)


@pytest.fixture(scope="module")
def bctx():
    """A context of this module's own: its RSS configuration is what these tests set."""
    ctx = abi.GpuContext(0, max_frames=1 << 17, max_lanes=256)
    yield ctx
    ctx.close()


def group(port, members, ip=RIP1, first=0):
    return {abi.raw_port(port): [(ip, first + k, 1) for k in range(members)]}


def flows(n, seed, dports, dst=IP1, **kw):
    src, sport = U.random_flows(n, seed)
    dst = np.tile(np.array(U.ip_bytes(dst), np.uint8), (n, 1)) if isinstance(dst, str) else dst
    return U.flow_frames(src, sport, dst, np.broadcast_to(np.asarray(dports), (n,)), seed, **kw)


def upload(ctx, b, n_lanes, cap):
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, b.ptype)
    db.frames_bytes = b.frames_bytes
    return db, abi.rx_alloc_out(ctx, b.n, n_lanes, max(1, cap))


def free(db, out=None):
    for x in (db.frames, db.offset, db.length, db.ptype) + ((out.meta, out.lane_off, out.lane_pkt) if out else ()):
        if x is not None:
            x.free()


def rx(ctx, lists, b, n_lanes, cap):
    """udpdk_gpu_rx with the stage off: (device batch, meta, lane_off, lane_pkt); the model's walk
    makes the same deliveries."""
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, n_lanes))
    db, out = upload(ctx, b, n_lanes, cap)
    meta, loff, lpkt, _, rc = abi.rx_run(ctx, db, out)
    for x in (out.meta, out.lane_off, out.lane_pkt):
        x.free()
    assert rc == 0
    _, dels, _ = U.choose(lists.get, b, meta, np.zeros(n_lanes, np.uint8), np.zeros(b.n, np.uint32))
    lane_of = np.repeat(np.arange(n_lanes), np.diff(loff.astype(np.int64)))
    got = [[] for _ in range(b.n)]
    for l, i in zip(lane_of, lpkt):
        got[i].append(int(l))
    assert got == [sorted(d) for d in dels], "the model's walk differs from the lanes"
    return db, meta, loff, lpkt


def check(ctx, lists, b, db, meta, loff, lpkt, rp, what, hashes=None, key=R.STD_KEY, types=3, **kw):
    m = U.model(lists.get, b, meta, loff, lpkt, rp, hashes, key=key, types=types,
                **{k: v for k, v in kw.items() if k in ("n", "lane_cap")})
    go, gp, st, rc = abi.rx_balance_run(ctx, db, meta, loff, lpkt, rp, hashes=hashes, pad=8, **kw)
    out_cap = len(gp) - 8
    assert np.array_equal(go, m.lane_off), f"{what}: lane_off"
    w = min(m.kept, out_cap)
    assert np.array_equal(gp[:w], m.lane_pkt[:w]), f"{what}: lane entries"
    assert np.all(gp[w:] == SENT), f"{what}: wrote past the kept entries"
    assert (st.kept, st.removed, st.balanced, st.bad_index, st.truncated) == \
        (m.kept, m.removed, m.balanced, m.bad_index, m.truncated), what
    assert rc == (-errno.ENOSPC if m.kept > out_cap else 0), what
    return m


# ---- the explicit call --------------------------------------------------------------------------
LISTS_AB = {**group(PA, 3), abi.raw_port(PB): [(0, 3, 0)]}


@pytest.mark.parametrize("d", [0, 1, 63, 64, 65, E - 1, E, E + 1, 2 * E + 1])
def test_entry_counts(bctx, d):
    a, r = divmod(d, 3)
    dports = np.array([PA] * a + [PB] * r + [PX])
    b = flows(len(dports), 300 + d, dports[np.random.default_rng(d).permutation(len(dports))])
    db, meta, loff, lpkt = rx(bctx, LISTS_AB, b, 4, max(1, d))
    try:
        assert int(loff[4]) == d
        m = check(bctx, LISTS_AB, b, db, meta, loff, lpkt, [1, 1, 1, 0], f"d={d}")
        assert m.kept == a + r and m.balanced == a
    finally:
        free(db)


def test_workspace_grows_and_is_reused():
    """A fresh context's first three calls: one tile, then three (the workspace has to grow), then
    one again (the larger workspace is reused, with the second call's rows, masks and choices
    beyond the live ones); lanes and stats exact after each."""
    ctx = abi.GpuContext(0, max_frames=1 << 12, max_lanes=8)
    try:
        for step, d in enumerate((64, 2 * E + 1, 64)):
            a, r = divmod(d, 3)
            dports = np.array([PA] * a + [PB] * r + [PX])
            b = flows(len(dports), 900 + step, dports[np.random.default_rng(step).permutation(len(dports))])
            db, meta, loff, lpkt = rx(ctx, LISTS_AB, b, 4, d)
            try:
                assert int(loff[4]) == d
                m = check(ctx, LISTS_AB, b, db, meta, loff, lpkt, [1, 1, 1, 0], f"step {step} d={d}")
                assert m.kept == a + r and m.balanced == a
            finally:
                free(db)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1])
def test_frame_counts(bctx, n):
    lists = group(PA, 2)
    b = flows(n, 400 + n, PA)
    db, meta, loff, lpkt = rx(bctx, lists, b, 2, 2 * n)
    try:
        m = check(bctx, lists, b, db, meta, loff, lpkt, [1, 1], f"n={n}")
        assert m.kept == n == m.balanced
    finally:
        free(db)


@pytest.mark.parametrize("g", [1, 2, 3, 7, 64, 130])
def test_group_sizes(bctx, g):
    """Past 127 members the verdict word's fan-out saturates: the walk counts for itself."""
    lists = group(PA, g)
    n = 600
    b = flows(n, 500 + g, PA)
    db, meta, loff, lpkt = rx(bctx, lists, b, g, g * n)
    try:
        assert np.all(abi.meta_fanout(meta) == min(g, 127))
        m = check(bctx, lists, b, db, meta, loff, lpkt, np.ones(g, np.uint8), f"g={g}")
        assert m.kept == n and m.balanced == (n if g > 1 else 0)
        per = np.diff(m.lane_off.astype(np.int64))
        if g <= 7:
            assert per.min() > 0
        assert len(np.flatnonzero(per)) >= min(g, 50)        # 600 flows reach most of a large group
    finally:
        free(db)


LISTS_SHAPES = {
    abi.raw_port(PA): [(0, 0, 1), (RIP1, 1, 1), (RIP1, 2, 1), (RIP9, 3, 1), (RIP1, 4, 1)],   # ANY + specific
    abi.raw_port(PB): [(RIP1, 5, 1), (RIP1, 6, 1), (RIP1, 7, 0), (RIP1, 8, 1)],             # 7 ends the walk
    abi.raw_port(PC): [(0, 9, 0), (RIP1, 10, 1)],                                          # ANY swallows
}


@pytest.mark.parametrize("rp", [[1] * 11, [1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0], [0] * 11],
                         ids=["all", "interleaved", "few", "none"])
def test_group_shapes(bctx, rp):
    """Ports with different groups in one batch (ANY + specific members, a non-reuse binding that
    ends the walk inside a group, an ANY head that swallows), NO_MATCH, NO_BIND, NOT_UDP and FRAG
    frames between them; flagged and unflagged members interleaved."""
    b = F.mixed_batch(31, 3000, [PA, PB, PC], [9, PX], [IP1, IP9])
    db, meta, loff, lpkt = rx(bctx, LISTS_SHAPES, b, 11, 5 * b.n)
    try:
        assert set(np.unique(abi.meta_verdict(meta))) >= {0, 2, 3, 4, 5}
        hs = np.random.default_rng(32).integers(0, 1 << 32, b.n, dtype=np.uint64).astype(np.uint32)
        m = check(bctx, LISTS_SHAPES, b, db, meta, loff, lpkt, rp, "supplied", hashes=hs)
        assert (m.removed > 100) == (sum(rp) > 0)
        check(bctx, LISTS_SHAPES, b, db, meta, loff, lpkt, rp, "computed")
    finally:
        free(db)


def test_supplied_hashes(bctx):
    lists = group(PA, 3)
    edges = [0, 0xFFFFFFFF, 1, 0x55555555, 0x55555556, 0xAAAAAAAA, 0xAAAAAAAB, 0x80000000]
    b = flows(len(edges), 600, PA)
    db, meta, loff, lpkt = rx(bctx, lists, b, 3, 3 * b.n)
    try:
        m = check(bctx, lists, b, db, meta, loff, lpkt, [1, 1, 1], "edges", hashes=np.array(edges, np.uint32))
        assert list(m.chosen) == [0, 2, 0, 0, 1, 1, 2, 1]
    finally:
        free(db)


@pytest.mark.parametrize("conf", ["default", "key", "types1", "types2", "types3", "types0"])
def test_computed_hash(conf):
    """The stage's own hash: the default configuration on a context that never saw
    udpdk_gpu_rss_config, then a configured key and every hash_types value."""
    ctx = abi.GpuContext(0, max_frames=1 << 14, max_lanes=16)
    try:
        key, types = R.STD_KEY, 3
        if conf != "default":
            key = R.random_keys(1, 7)[0]
            types = {"key": 3, "types1": 1, "types2": 2, "types3": 3, "types0": 0}[conf]
            cf = abi.rss_conf(4, key=key, hash_types=types)
            assert abi.lib().udpdk_gpu_rss_config(ctx.handle, C.byref(cf)) == 0
        lists = group(PA, 5)
        b = flows(2000, 700, PA)
        db, meta, loff, lpkt = rx(ctx, lists, b, 5, 5 * b.n)
        try:
            m = check(ctx, lists, b, db, meta, loff, lpkt, [1] * 5, conf, key=key, types=types)
            per = np.diff(m.lane_off.astype(np.int64))
            assert (per.min() > 200) if types else (per[0] == b.n)
        finally:
            free(db)
    finally:
        ctx.close()


def test_destinations(bctx):
    """Limited broadcast and multicast keep every clone; 223.x and 240.x are balanced."""
    lists = {abi.raw_port(PA): [(0, 0, 1), (0, 1, 1), (0, 2, 1)]}
    dsts = ["255.255.255.255", "224.0.0.1", "239.255.255.255", "223.255.255.255", "240.0.0.1", "255.255.255.254"]
    n = 60
    dst = np.array([U.ip_bytes(dsts[i % len(dsts)]) for i in range(n)], np.uint8)
    b = flows(n, 800, PA, dst=dst)
    db, meta, loff, lpkt = rx(bctx, lists, b, 3, 3 * n)
    try:
        m = check(bctx, lists, b, db, meta, loff, lpkt, [1, 1, 1], "dst")
        keep_all = np.arange(n) % len(dsts) < 3
        assert np.all((m.chosen == U.KEEP_ALL) == keep_all)
        assert m.kept == 3 * keep_all.sum() + (~keep_all).sum()
    finally:
        free(db)


@pytest.mark.parametrize("first_gap", [0, 1, 2, 3])
def test_frame_alignment(bctx, first_gap):
    """Frames at every byte alignment; the last frame ends at frames_bytes with only the tailroom
    the contract asks for behind it."""
    lists = group(PA, 4)
    n = 257
    gaps = (np.arange(n) * 7 + first_gap) % 4
    b = flows(n, 900 + first_gap, PA, gaps=gaps, tail=0)
    assert len(b.frames) == b.frames_bytes and set(np.unique(b.offset % 4)) == {0, 1, 2, 3}
    db, meta, loff, lpkt = rx(bctx, lists, b, 4, 4 * n)
    try:
        m = check(bctx, lists, b, db, meta, loff, lpkt, [1] * 4, f"gap={first_gap}")
        assert m.balanced == n
    finally:
        free(db)


def test_bounds(bctx):
    lists = LISTS_AB
    b = flows(1500, 1000, np.where(np.arange(1500) % 4 == 3, PB, PA))
    db, meta, loff, lpkt = rx(bctx, lists, b, 4, 3 * b.n)
    rp = [1, 1, 1, 0]
    try:
        d = len(lpkt)
        bad = lpkt.copy()
        bad[5::97] = b.n + np.arange(len(bad[5::97]))              # entries >= n
        bad[11] = 0xFFFFFFFF
        m = check(bctx, lists, b, db, meta, loff, bad, rp, "entries >= n")
        assert m.bad_index == len(bad[5::97]) + 1
        check(bctx, lists, b, db, meta, loff, lpkt, rp, "n below the entries", n=b.n - 300)
        off2 = loff.copy()
        off2[3] = d + 1000                                         # an offset past D
        check(bctx, lists, b, db, meta, off2, lpkt, rp, "offset past D", lane_cap=d)
        off3 = loff.copy()
        off3[4] = d + 12345                                        # total past lane_cap
        m = check(bctx, lists, b, db, meta, off3, lpkt, rp, "truncated", lane_cap=d - 100)
        assert m.truncated == 1
        m = check(bctx, lists, b, db, meta, loff, lpkt, rp, "out_cap", out_cap=700)
        assert m.kept > 700
        check(bctx, lists, b, db, meta, loff, lpkt, rp, "out_cap 0", out_cap=0)
        ident = check(bctx, lists, b, db, meta, loff, bad, [0, 0, 0, 0], "all-zero flags")
        assert ident.removed == ident.bad_index
    finally:
        free(db)


@pytest.mark.parametrize("n_lanes", [1, 4096])
def test_lane_counts(gpu_ctx, n_lanes):
    """One lane (nothing to choose) and 4096 lanes, groups of four on every 16th socket."""
    if n_lanes == 1:
        lists = {abi.raw_port(PA): [(0, 0, 1)]}
        dports = np.full(500, PA)
    else:
        lists = {}
        for k in range(64):
            lists.update(group(PA + k, 4, first=64 * k + 7))
        dports = PA + np.arange(3000) % 64
    b = flows(len(dports), 1100, dports)
    db, meta, loff, lpkt = rx(gpu_ctx, lists, b, n_lanes, 4 * b.n)
    try:
        rp = np.ones(n_lanes, np.uint8)
        m = check(gpu_ctx, lists, b, db, meta, loff, lpkt, rp, f"lanes={n_lanes}", hashes=U.frame_hashes(b))
        assert m.kept == b.n
    finally:
        free(db)


def test_arguments(bctx):
    L = abi.lib()
    lists = group(PA, 2)
    b = flows(10, 1200, PA)
    db, meta, loff, lpkt = rx(bctx, lists, b, 2, 2 * b.n)
    bufs = [bctx.upload(x) for x in (meta, loff, lpkt, np.ones(2, np.uint8), np.zeros(3, np.uint32),
                                     np.zeros(20, np.uint32))]
    md, od, pd, rd, oo, po = bufs
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)

    def call(bt_=bt, lanes=None, rp=rd.ptr, off_out=oo.ptr, pkt_out=po.ptr, n_lanes=2, out_cap=20, h=bctx.handle):
        ln = lanes or abi.RxLanes(md.ptr, b.n, od.ptr, pd.ptr, len(lpkt), n_lanes)
        return L.udpdk_gpu_rx_balance_select(h, C.byref(bt_) if bt_ else None, C.byref(ln) if ln != 0 else None,
                                             rp, None, off_out, pkt_out, out_cap)
    try:
        assert call() == 0
        assert call(h=None) == -errno.EINVAL and call(bt_=None) == -errno.EINVAL
        assert call(rp=None) == -errno.EINVAL and call(off_out=None) == -errno.EINVAL
        assert call(pkt_out=None) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(None, b.n, od.ptr, pd.ptr, len(lpkt), 2)) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(md.ptr, b.n, None, pd.ptr, len(lpkt), 2)) == -errno.EINVAL
        assert call(lanes=abi.RxLanes(md.ptr, b.n, od.ptr, None, len(lpkt), 2)) == -errno.EINVAL
        assert call(n_lanes=0) == -errno.EINVAL and call(n_lanes=abi.MAX_LANES + 1) == -errno.EINVAL
        assert call(off_out=od.ptr) == -errno.EINVAL and call(pkt_out=pd.ptr) == -errno.EINVAL   # aliases
        assert call(pkt_out=pd.ptr + 8, out_cap=4) == -errno.EINVAL
        bctx.upload_snapshot(abi.snapshot_from_lists(lists, 2, lane_mask=0xFF))
        assert call() == -errno.EINVAL                              # compat lanes: not sockfds
        bctx.upload_snapshot(abi.snapshot_from_lists(lists, 2))
        assert call() == 0
        fresh = abi.GpuContext(0, max_frames=1024, max_lanes=4)
        try:
            st = abi.RxBalanceStats()
            assert L.udpdk_gpu_rx_balance_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
            assert call(h=fresh.handle) == -errno.EINVAL            # no snapshot uploaded
            assert L.udpdk_gpu_rx_balance(fresh.handle, np.ones(5, np.uint8).ctypes.data, 5) == -errno.EINVAL
        finally:
            fresh.close()
    finally:
        for x in bufs:
            x.free()
        free(db)


# ---- sticky mode --------------------------------------------------------------------------------
RP_SHAPES = [1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1]


def shapes_batch(seed, n=2500):
    return F.mixed_batch(seed, n, [PA, PB, PC], [9, PX], [IP1, IP9])


def sticky_run(ctx, db, out, rp, drop=0):
    ctx.rx_balance(rp)
    ctx.rx_drop(drop)
    try:
        res = abi.rx_run(ctx, db, out)
        return res, abi.rx_balance_stats(ctx)
    finally:
        ctx.rx_drop(0)
        ctx.rx_balance(None)


def test_sticky_equals_explicit_and_off_restores(bctx):
    b = shapes_batch(41)
    db, meta, loff, lpkt = rx(bctx, LISTS_SHAPES, b, 11, 5 * b.n)
    out = abi.rx_alloc_out(bctx, b.n, 11, len(lpkt))
    try:
        m = check(bctx, LISTS_SHAPES, b, db, meta, loff, lpkt, RP_SHAPES, "explicit")
        (gm, gl, gp, gc, rc), (brc, bst) = sticky_run(bctx, db, out, RP_SHAPES)
        assert rc == 0 and brc == 0 and np.array_equal(gm, meta)
        assert np.array_equal(gl, m.lane_off) and np.array_equal(gp, m.lane_pkt)
        assert int(gc[abi.C_DELIVERIES]) == len(lpkt) and len(gp) == m.kept == bst.kept
        assert (bst.removed, bst.balanced) == (m.removed, m.balanced) and m.removed > 300
        gm, gl, gp, gc, rc = abi.rx_run(bctx, db, out)
        assert rc == 0 and np.array_equal(gl, loff) and np.array_equal(gp, lpkt)
        # lane_cap below the fan-out total: overflow is the pre-stage total's
        small = abi.rx_alloc_out(bctx, b.n, 11, len(lpkt) - 200)
        try:
            (gm, gl, gp, gc, rc), (brc, bst) = sticky_run(bctx, db, small, RP_SHAPES)
            mt = U.model(LISTS_SHAPES.get, b, meta, loff, lpkt, RP_SHAPES, lane_cap=len(lpkt) - 200)
            assert rc == -errno.ENOSPC and bst.truncated == 1
            assert np.array_equal(gl, mt.lane_off) and np.array_equal(gp, mt.lane_pkt)
        finally:
            for x in (small.meta, small.lane_off, small.lane_pkt):
                x.free()
    finally:
        free(db, out)


def test_sticky_with_drop_commutes(bctx):
    b = shapes_batch(43)
    db, meta, loff, lpkt = rx(bctx, LISTS_SHAPES, b, 11, 5 * b.n)
    out = abi.rx_alloc_out(bctx, b.n, 11, len(lpkt))
    try:
        d1 = UD.model(meta, loff, lpkt, UD.DROP_ALL)
        m1 = U.model(LISTS_SHAPES.get, b, meta, d1.lane_off, d1.lane_pkt, RP_SHAPES)
        m2 = U.model(LISTS_SHAPES.get, b, meta, loff, lpkt, RP_SHAPES)
        d2 = UD.model(meta, m2.lane_off, m2.lane_pkt, UD.DROP_ALL)
        assert np.array_equal(m1.lane_off, d2.lane_off) and np.array_equal(m1.lane_pkt, d2.lane_pkt)
        assert d1.removed > 300 and m1.removed > 100
        (gm, gl, gp, gc, rc), (brc, bst) = sticky_run(bctx, db, out, RP_SHAPES, drop=abi.RX_DROP_ALL)
        drc, dst = abi.rx_drop_stats(bctx)
        assert rc == 0 and np.array_equal(gm, meta)
        assert np.array_equal(gl, m1.lane_off) and np.array_equal(gp, m1.lane_pkt)
        assert dst.removed == d1.removed and bst.removed == m1.removed and bst.kept == m1.kept
        # what each stage removed in the call a stats block belongs to (the socket layer's counters)
        bctx.rx_balance(RP_SHAPES)
        bctx.rx_drop(abi.RX_DROP_ALL)
        try:
            assert abi.rx_enqueue(bctx, db, out) == 0
            rc, st = abi.rx_stats(bctx)
        finally:
            bctx.rx_drop(0)
            bctx.rx_balance(None)
        dr, ba = C.c_uint32(), C.c_uint32()
        assert abi.lib().udpdk_gpu_rx_removed(bctx.handle, C.byref(st), C.byref(dr), C.byref(ba)) == 0
        assert rc == 0 and (dr.value, ba.value) == (d1.removed, m1.removed)
        assert st.deliveries == m1.kept and st.counters[abi.C_DELIVERIES] == len(lpkt)
    finally:
        free(db, out)


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_sticky_pipeline_depths(bctx, depth):
    bs = [shapes_batch(50 + k, 1500 + 400 * k) for k in range(depth)]
    devs, wants = [], []
    try:
        for b in bs:
            db, meta, loff, lpkt = rx(bctx, LISTS_SHAPES, b, 11, 5 * b.n)
            devs.append((db, abi.rx_alloc_out(bctx, b.n, 11, len(lpkt))))
            wants.append((meta, U.model(LISTS_SHAPES.get, b, meta, loff, lpkt, RP_SHAPES)))
        bctx.pipeline(depth)
        bctx.rx_balance(RP_SHAPES)
        try:
            for _ in range(2):
                for db, out in devs:
                    assert abi.rx_enqueue(bctx, db, out) == 0
            rc, st = abi.rx_stats(bctx)
            bctx.sync()
        finally:
            bctx.rx_balance(None)
            bctx.pipeline(1)
        for k, ((db, out), (meta, m)) in enumerate(zip(devs, wants)):
            assert np.array_equal(bctx.download(out.meta, np.uint32, out.n), meta), k
            assert np.array_equal(bctx.download(out.lane_off, np.uint32, 12), m.lane_off), k
            assert np.array_equal(bctx.download(out.lane_pkt, np.uint32, m.kept), m.lane_pkt), k
        assert rc == 0 and st.deliveries == wants[-1][1].kept
    finally:
        for db, out in devs:
            free(db, out)


def test_sticky_host_calls(bctx):
    """udpdk_gpu_rx_host, udpdk_gpu_rx_host_async (depths 1 and 3) and udpdk_gpu_pipe_rx_host."""
    L = abi.lib()
    b = shapes_batch(61, 2000)
    db, meta, loff, lpkt = rx(bctx, LISTS_SHAPES, b, 11, 5 * b.n)
    free(db)
    m = U.model(LISTS_SHAPES.get, b, meta, loff, lpkt, RP_SHAPES)
    cap = 5 * b.n

    def call(fn, depth, reps):
        bctx.pipeline(depth)
        res = []
        try:
            for r in range(reps):
                gm, gl, gp = np.zeros(b.n, np.uint32), np.zeros(12, np.uint32), np.zeros(cap, np.uint32)
                st = abi.RxStats()
                args = (b.frames.ctypes.data, b.frames_bytes, b.offset.ctypes.data)
                tail = (b.length.ctypes.data, None, b.n, gm.ctypes.data, gl.ctypes.data, gp.ctypes.data, cap, C.byref(st))
                if fn is L.udpdk_gpu_pipe_rx_host:
                    assert fn(bctx.handle, 1 + r % 3, *args, 0, *tail) == 0
                    assert L.udpdk_gpu_pipe_wait(bctx.handle, 1 + r % 3) == 0
                else:
                    assert fn(bctx.handle, *args, *tail) == 0
                res.append((gm, gl, gp, st))
            if fn is L.udpdk_gpu_rx_host_async:
                assert L.udpdk_gpu_rx_host_wait(bctx.handle) == 0
        finally:
            bctx.pipeline(1)
        return res

    for fn, depth in ((L.udpdk_gpu_rx_host, 1), (L.udpdk_gpu_rx_host_async, 1), (L.udpdk_gpu_rx_host_async, 3),
                      (L.udpdk_gpu_pipe_rx_host, 1)):
        bctx.rx_balance(RP_SHAPES)
        try:
            res = call(fn, depth, 3)
        finally:
            bctx.rx_balance(None)
        for gm, gl, gp, st in res:
            assert np.array_equal(gm, meta) and np.array_equal(gl, m.lane_off)
            assert st.deliveries == m.kept and st.overflow == 0 and st.counters[abi.C_DELIVERIES] == len(lpkt)
            assert np.array_equal(gp[:m.kept], m.lane_pkt)
        for gm, gl, gp, st in call(fn, depth, 1):                  # off again
            assert np.array_equal(gl, loff) and np.array_equal(gp[:st.deliveries], lpkt)


# ---- socket layer -------------------------------------------------------------------------------
def init(tmp_path, extra):
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.2\n"
                   "[port0_dst]\nmac_addr = 68:05:ca:95:fa:64\n"
                   "[gpu]\nmax_frames = 65536\nmax_lanes = 16\n"
                   "frag_buckets = 64\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    assert abi.lib().udpdk_init(3, argv) == 0


def poll_slice(b, lo, hi):
    """Frames [lo, hi) of a back-to-back batch through udpdk_poll_rx."""
    o0, o1 = int(b.offset[lo]), int(b.offset[hi - 1]) + int(b.length[hi - 1])
    buf = np.zeros(o1 - o0 + 64, np.uint8)
    buf[:o1 - o0] = b.frames[o0:o1]
    off = (b.offset[lo:hi] - o0).astype(np.uint32)
    ln = np.ascontiguousarray(b.length[lo:hi])
    st = abi.RxStats()
    assert abi.lib().udpdk_poll_rx(buf.ctypes.data, o1 - o0, off.ctypes.data, ln.ctypes.data, None, hi - lo,
                                   C.byref(st)) == 0
    return st


def drain(api, s):
    abi.lib().udpdk_interrupt(0)                # recvfrom on an empty ring: -1 instead of waiting
    out = []
    while True:
        n, data, _ = api.recvfrom(s, 2048)
        if n < 0:
            return out
        out.append(data)


def eight_sockets(api, port=PA, ip=IP1):
    socks = [api.socket() for _ in range(8)]
    for s in socks:
        assert api.setsockopt(s, abi.SOL_SOCKET, abi.SO_REUSEPORT, 1) == 0
        assert api.bind(s, ip, port) == 0
    return socks


def flow_dgrams(n_flows, per_flow, payload_len=22, seed=SEED_FLOWS):
    """per_flow rounds of one datagram per flow; the payload names the flow and the round."""
    src, sport = U.random_flows(n_flows, seed)
    n = n_flows * per_flow
    k = np.arange(n)
    pay = np.zeros((n, payload_len), np.uint8)
    pay[:, :4] = (k % n_flows).astype("<u4").view(np.uint8).reshape(n, 4)
    pay[:, 4] = k // n_flows
    dst = np.tile(np.array(U.ip_bytes(IP1), np.uint8), (n, 1))
    return U.flow_frames(np.tile(src, (per_flow, 1)), np.tile(sport, per_flow), dst, np.full(n, PA), 1,
                         payload_len=payload_len, payload=pay)


def model_rings(api, b, socks):
    """Per socket, the payloads the model sends it, in arrival order."""
    lists = api.port_lists()
    meta = np.full(b.n, 0x30 | len(socks) << 9, np.uint32)
    chosen, dels, _ = U.choose(lists.get, b, meta, api.reuseport_lanes(16)[1], U.frame_hashes(b))
    assert all(sorted(d) == sorted(socks) for d in dels)
    return chosen, [[b.rows[i, 42:].tobytes() for i in np.flatnonzero(chosen == s)] for s in socks]


def test_socket_layer_fanout_default(tmp_path, host_api):
    init(tmp_path, "")
    try:
        socks = eight_sockets(host_api)
        b = flow_dgrams(1024, 1)                    # (one poll: a ring holds 2048 datagrams)
        st = poll_slice(b, 0, b.n)
        want = [b.rows[i, 42:].tobytes() for i in range(b.n)]
        for s in socks:
            assert drain(host_api, s) == want
        assert st.deliveries == 8 * b.n and host_api.rx_balanced() == 0 and host_api.rx_dropped() == 0
    finally:
        abi.lib().udpdk_cleanup()


@pytest.mark.parametrize("extra", ["reuseport = balance\n", "reuseport = balance\ndevices = 0,0\n",
                                   "reuseport = balance\ndevices = 0,0\ndispatch = rss\n"],
                         ids=["one-context", "two-shards", "two-shards-rss"])
def test_socket_layer_balance(tmp_path, host_api, extra):
    """Eight SO_REUSEPORT sockets on one port, 4096 flows x 4 datagrams: the rings partition
    them, each flow stays on one socket in arrival order."""
    init(tmp_path, extra)
    try:
        assert host_api.config_reuseport(-1) == abi.REUSEPORT_BALANCE
        socks = eight_sockets(host_api)
        b = flow_dgrams(4096, 4)
        chosen, want = model_rings(host_api, b, socks)
        assert np.array_equal(chosen[:4096], chosen[4096:8192]) and min(len(w) for w in want) > 0
        got = [[] for _ in socks]
        for lo in range(0, b.n, 2048):
            st = poll_slice(b, lo, lo + 2048)
            assert st.deliveries == 2048 and st.counters[abi.C_DELIVERIES] == 8 * 2048
            for k, s in enumerate(socks):
                got[k] += drain(host_api, s)
        assert got == want
        assert host_api.rx_balanced() == 7 * b.n and host_api.rx_dropped() == 0 and host_api.rx_nobufs() == 0
        # a socket leaves: the flags and the group follow the bind table
        assert host_api.close(socks[3]) == 0
        poll_slice(b, 0, 512)
        rest = [s for s in socks if s != socks[3]]
        chosen2, want2 = model_rings(host_api, SimpleBatch(b, 512), rest)
        assert [drain(host_api, s) for s in rest] == want2
        # back to fanout through the config call
        assert host_api.config_reuseport(abi.REUSEPORT_FANOUT) == abi.REUSEPORT_BALANCE
        poll_slice(b, 0, 64)
        assert all(len(drain(host_api, s)) == 64 for s in rest)
    finally:
        abi.lib().udpdk_cleanup()


def SimpleBatch(b, n):
    return SimpleNamespace(frames=b.frames, offset=b.offset[:n], length=b.length[:n], frames_bytes=b.frames_bytes,
                           n=n, ptype=None, rows=b.rows[:n])


def test_socket_layer_chunked_poll(tmp_path, host_api):
    init(tmp_path, "poll_chunk_mb = 1\npoll_chunk_min_avg = 0\n")
    try:
        assert host_api.config_reuseport(abi.REUSEPORT_BALANCE) == 0
        socks = eight_sockets(host_api)
        b = flow_dgrams(1100, 2, payload_len=1400)
        _, want = model_rings(host_api, b, socks)
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == b.n and st.counters[abi.C_DELIVERIES] == 8 * b.n
        assert [drain(host_api, s) for s in socks] == want
        assert host_api.rx_balanced() == 7 * b.n
    finally:
        abi.lib().udpdk_cleanup()


def test_socket_layer_with_drop(tmp_path, host_api):
    """rx_drop = udp beside balance: each counter counts its own removals."""
    init(tmp_path, "reuseport = balance\nrx_drop = udp\n")
    try:
        socks = eight_sockets(host_api)
        b = flow_dgrams(1024, 2)
        _, want = model_rings(host_api, b, socks)
        badrows = np.arange(5, b.n, 16)
        bad = {b.rows[i, 42:].tobytes() for i in badrows}
        b.frames[b.offset[badrows].astype(np.int64) + 55] ^= 0x40
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == b.n - len(badrows)
        assert [drain(host_api, s) for s in socks] == [[p for p in w if p not in bad] for w in want]
        assert host_api.rx_dropped() == 8 * len(badrows)
        assert host_api.rx_balanced() == 7 * (b.n - len(badrows))
    finally:
        abi.lib().udpdk_cleanup()


def test_socket_layer_reassembly(tmp_path, host_api):
    """A fragmented and a plain datagram per flow land on the same socket: the reassembled
    datagram hashes like an unfragmented one."""
    init(tmp_path, "reuseport = balance\n")
    try:
        socks = eight_sockets(host_api)
        nfl = 256
        src, sport = U.random_flows(nfl, 77)
        rng = np.random.default_rng(78)
        frames, plain_rows = [], []
        pb = flow_dgrams(nfl, 1, seed=77)
        chosen, _ = model_rings(host_api, pb, socks)
        bigs = []
        for f in range(nfl):
            big = rng.integers(0, 256, 2000, dtype=np.uint8).tobytes()
            bigs.append(big)
            sip = int.from_bytes(bytes(src[f]), "little")
            d = udp_datagram(int.from_bytes(int(sport[f]).to_bytes(2, "big"), "little"), abi.raw_port(PA), big)
            frames += split(sip, RIP1, f, d, [1480, len(d) - 1480])
            frames.append(pb.rows[f].tobytes())
        buf, off, ln = batch(frames)
        st = abi.RxStats()
        assert abi.lib().udpdk_poll_rx(buf.ctypes.data, len(buf) - 64, off.ctypes.data, ln.ctypes.data, None,
                                       len(off), C.byref(st)) == 0
        for k, s in enumerate(socks):
            got = drain(host_api, s)
            mine = np.flatnonzero(chosen == s)
            assert sorted(got) == sorted([bigs[f] for f in mine] + [pb.rows[f, 42:].tobytes() for f in mine]), k
        assert host_api.rx_balanced() == 7 * 2 * nfl and host_api.rx_dropped() == 0
    finally:
        abi.lib().udpdk_cleanup()


def test_poll_echo_answers_once(tmp_path, host_api):
    init(tmp_path, "reuseport = balance\n")
    try:
        socks = eight_sockets(host_api)
        b = flow_dgrams(512, 1)
        chosen, _ = model_rings(host_api, b, socks)
        rc, err, replies, st, n = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length)
        assert rc == 0 and n == b.n == len(replies) == st.deliveries
        # replies come in lane order, each lane's in arrival order, with the request's payload
        order = np.argsort(chosen, kind="stable")
        assert [r[42:] for r in replies] == [b.rows[i, 42:].tobytes() for i in order]
        assert host_api.rx_balanced() == 7 * b.n
        host_api.config_reuseport(abi.REUSEPORT_FANOUT)
        rc, err, replies, st, n = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length, max_frames=8192)
        assert rc == 0 and n == 8 * b.n
    finally:
        abi.lib().udpdk_cleanup()
