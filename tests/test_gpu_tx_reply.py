"""udpdk_gpu_tx_reply_plan / udpdk_gpu_tx_reply on the GPU against the numpy model and the oracle's
frames (tests/tx_reply_util.py, pinned to oracle.recv_gather in test_tx_reply_ref.py).

The harness: the six plan arrays are 8 elements longer than the call may write and pre-filled with
0xA5 bytes, the output buffer is pre-filled with 0xEE and 4096 bytes longer than out_cap; every
downloaded byte is compared (descriptors, offsets, frames, fill), and the stats with the model's."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
import tx_reply_util as R
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

CFG_IP = abi.raw_ip("172.31.100.2")
IP1 = "172.31.100.1"
GUARD = 4096


def _cfg():
    return abi.TxConfig((C.c_uint8 * 6)(*R.SRC_MAC), (C.c_uint8 * 6)(*R.DST_MAC), CFG_IP)


def _slots(n_lanes):
    """Socket l: bound to ANY on odd l, to 10.0.x.y on even l, port 20000 + l."""
    return [(0 if l & 1 else abi.raw_ip(f"10.0.{l >> 8}.{l & 255 or 1}"), abi.raw_port(20000 + l), 1)
            for l in range(n_lanes)]


def _snapshot(ctx, lists, n_lanes, slots=None, lane_mask=0xFFFFFFFF):
    slots = _slots(n_lanes) if slots is None else slots
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, n_lanes, lane_mask=lane_mask, slots=slots))
    return slots


def _upload(ctx, b):
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    return db


def _free(ctx, db):
    for x in (db.frames, db.offset, db.length):
        x.free()


def _simple_batch(n, size=64, seed=7, port=10001):
    return F.build_frames(np.full(n, size, np.uint32), np.full(n, port, np.uint32), seed)


def _run_both(ctx, b, db, slots, loff, lpkt, first, count, *, mtu=0, flags=0, out_cap=None, **kw):
    """Plan alone and the full reply, each against the model; returns (model, reply result)."""
    P0 = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, first, count, mtu=mtu, **kw)
    out_cap = P0.stats["bytes_needed"] + 64 if out_cap is None else out_cap
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, first, count, mtu=mtu,
                     out_cap=out_cap, **kw)
    res = abi.tx_reply_plan_run(ctx, db, loff, lpkt, first, count, mtu=mtu, out_cap=out_cap, **kw)
    assert res["rc"] == 0
    R.check_plan(res, P, count)
    rc, st = abi.tx_reply_stats(ctx)
    assert rc == (-errno.ENOSPC if P.stats["no_room"] else 0)
    R.check_stats(st, P)
    res = abi.tx_reply_run(ctx, _cfg(), db, loff, lpkt, first, count, mtu=mtu, flags=flags, out_cap=out_cap,
                           guard=GUARD, **kw)
    assert res["rc"] == 0
    R.check_plan(res, P, count)
    rc, st = abi.tx_reply_stats(ctx)
    assert rc == (-errno.ENOSPC if P.stats["no_room"] else 0)
    R.check_stats(st, P)
    want, frames = R.image(P, b.frames, slots, CFG_IP, mtu, bool(flags & abi.TX_UDP_CKSUM), out_cap + GUARD)
    bad = np.nonzero(res["out"] != want)[0]
    assert bad.size == 0, f"{bad.size} output bytes differ, the first at {int(bad[0])} (end {P.stats['end']})"
    assert len(frames) == P.stats["frames"]
    return P, res


# ---- counts --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_lane(gpu_ctx):
    """4 x B + 1 delivered 64 B frames in one lane (lane 0 of 1)."""
    B, _ = abi.tx_reply_geometry(1)
    n = 4 * B + 1
    b = _simple_batch(n)
    db = _upload(gpu_ctx, b)
    loff = np.array([0, n], np.uint32)
    yield B, n, b, db, loff, np.arange(n, dtype=np.uint32)
    _free(gpu_ctx, db)


def _counts():
    B, _ = abi.tx_reply_geometry(1)
    return [1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 1]


@pytest.mark.parametrize("count", _counts())
def test_count_sweep(gpu_ctx, one_lane, count):
    B, n, b, db, loff, lpkt = one_lane
    slots = _snapshot(gpu_ctx, {}, 1)
    assert abi.tx_reply_geometry(count) == (B, -(-count // B))
    P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, count)
    assert P.stats["replied"] == count and P.stats["bytes_needed"] == 64 * count


@pytest.mark.parametrize("first", [0, 1, 63, 64, 100])
def test_first_sweep(gpu_ctx, one_lane, first):
    B, n, b, db, loff, lpkt = one_lane
    slots = _snapshot(gpu_ctx, {}, 1)
    lpkt = lpkt[::-1].copy()                                  # entries are not frame order
    P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, first, 2 * B + 3)
    assert np.array_equal(P.payload_off, b.offset[lpkt[first:first + 2 * B + 3]] + 42)
    # a range that runs past the entries that exist: the rest is skipped
    P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, n - 70 + first % 7, 200)
    assert P.stats["replied"] == 70 - first % 7 and P.reason[-1] == "past"


def test_more_blocks_than_one_base_step(gpu_ctx):
    """One workgroup more than the base pass's 256 lanes take one row each of: its lanes take two
    rows, the last ones none. The room ends inside a row of a lane's second step."""
    B, _ = abi.tx_reply_geometry(1)
    count = 256 * B + 1
    assert abi.tx_reply_geometry(count) == (B, 257)
    b = _simple_batch(count, seed=11)
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, {}, 1)
    loff, lpkt = np.array([0, count], np.uint32), np.arange(count, dtype=np.uint32)
    try:
        # with room for all: the plan alone (descriptors, offsets, stats)
        P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, count)
        res = abi.tx_reply_plan_run(gpu_ctx, db, loff, lpkt, 0, count, out_cap=64 * count)
        R.check_plan(res, P, count)
        rc, st = abi.tx_reply_stats(gpu_ctx)
        assert rc == 0 and st.replied == count and st.bytes_needed == 64 * count
        R.check_stats(st, P)
        # the room ends in workgroup 201, the second row of the base pass's lane 100
        fit = 201 * B + 17
        P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, count, out_cap=64 * fit + 5)
        assert P.stats["replied"] == fit and P.stats["no_room"] == count - fit
    finally:
        _free(gpu_ctx, db)


# ---- lanes ---------------------------------------------------------------------------------------
def test_three_lanes_among_empty_ones(gpu_ctx):
    """Sockets 2, 5 and 6 of 9 receive: empty lanes before, between and after."""
    lists = {abi.raw_port(10001): [(0, 2, 0)], abi.raw_port(10002): [(0, 5, 0)], abi.raw_port(10003): [(0, 6, 0)]}
    b = F.mixed_batch(21, 700, [10001, 10002, 10003], [7], [IP1])
    _, loff, lpkt, _ = O.rx(O.bindtable_from_lists(lists), b.frames, b.frames_bytes, b.offset, b.length, None, 9)
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, lists, 9)
    try:
        D = int(loff[9])
        P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, D)
        assert {int(s) for s in P.sockfd} == {2, 5, 6}
        _run_both(gpu_ctx, b, db, slots, loff, lpkt, int(loff[5]) - 3, int(loff[6] - loff[5]) + 40)
    finally:
        _free(gpu_ctx, db)


def test_4096_lanes_a_few_entries_each(gpu_ctx):
    """Lane l holds l % 4 entries: every wave spans dozens of lanes, a quarter of them empty."""
    nl = 4096
    per = np.arange(nl) % 4
    n = int(per.sum())
    b = _simple_batch(n, seed=23)
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, {}, nl)
    loff = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    lpkt = np.random.default_rng(23).permutation(n).astype(np.uint32)
    try:
        P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n)
        assert np.array_equal(P.sockfd, np.repeat(np.arange(nl), per))
        sel = (np.arange(nl) % 2).astype(np.uint8)            # alternating lanes
        P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 5, n - 5, lane_sel=sel)
        assert P.stats["unselected"] > 0 and all(s & 1 for s in P.sockfd if s >= 0)
    finally:
        _free(gpu_ctx, db)


def test_reuse_fanout_and_source_address_rule(gpu_ctx):
    """Port 10002 is bound by sockets 1 (a specific IP) and 3 (another bind of it) with reuse: one
    frame sits in two lanes and is answered twice, by two sockets. Socket 0 is bound ANY: its
    replies carry the configured source IP, the others their binding's. The lanes are the GPU's."""
    ip = abi.raw_ip(IP1)
    lists = {abi.raw_port(10001): [(0, 0, 0)], abi.raw_port(10002): [(ip, 1, 1), (ip, 3, 1)]}
    slots = [(0, abi.raw_port(10001), 1), (ip, abi.raw_port(10002), 1), (0, 0, 0), (ip, abi.raw_port(10002), 1)]
    b = F.mixed_batch(31, 600, [10001, 10002], [7], [IP1, "172.31.100.9"])
    db = _upload(gpu_ctx, b)
    _snapshot(gpu_ctx, lists, 4, slots)
    try:
        out = abi.rx_alloc_out(gpu_ctx, b.n, 4, 4 * b.n)
        _, loff, lpkt, _, rc = abi.rx_run(gpu_ctx, db, out)
        assert rc == 0 and loff[2] - loff[1] == loff[4] - loff[3] > 0
        D = int(loff[4])
        P, res = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, D, flags=abi.TX_UDP_CKSUM)
        assert np.array_equal(lpkt[loff[1]:loff[2]], lpkt[loff[3]:loff[4]])
        for k in range(D):
            fo = int(P.frame_off[k])
            src = int.from_bytes(res["out"][fo + 26:fo + 30].tobytes(), "little")
            assert src == (CFG_IP if P.sockfd[k] == 0 else ip)
            assert res["out"][fo + 30:fo + 34].tobytes() == b.frames[P.payload_off[k] - 16:P.payload_off[k] - 12].tobytes()
    finally:
        _free(gpu_ctx, db)


# ---- lengths -------------------------------------------------------------------------------------
def test_payload_lengths_padding_and_alignment(gpu_ctx):
    """Payloads 0, 1, 17, 18, 1458 and 1472; 60 B padded frames; dgram_len longer than the frame and
    shorter than 8 (the u16 wrap); every offset & 3; the last frame ends exactly at frames_bytes."""
    rng = np.random.default_rng(41)
    fr = []
    for rep in range(5):                                      # gaps of 1: every residue of offset & 3
        for pl in (0, 1, 17, 18, 1458, 1472):
            fr.append(F.make_frame(rng, dport=10001, payload_len=pl))
        for pl in (0, 1, 17):
            fr.append(F.make_frame(rng, dport=10001, payload_len=pl, pad=18 - pl))       # 60 B on the wire
        fr.append(F.make_frame(rng, dport=10001, payload_len=30, udp_len=8 + 30 + 25))   # longer than the frame
        for ul in (0, 3, 7):
            fr.append(F.make_frame(rng, dport=10001, payload_len=40, udp_len=ul))        # (ul - 8) & 0xFFFF
    buf, offs = bytearray(), []
    for f in fr:
        buf += bytes(1)
        offs.append(len(buf))
        buf += f
    total = len(buf)                                          # the last frame ends the buffer
    assert {o & 3 for o in offs} == {0, 1, 2, 3}
    flat = np.concatenate([np.frombuffer(bytes(buf), np.uint8), np.full(abi.FRAMES_TAILROOM, 0x5A, np.uint8)])
    b = F.Batch(flat, np.array(offs, np.uint32), np.array([len(f) for f in fr], np.uint16), total)
    n = b.n
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, {}, 2)
    loff = np.array([0, n // 2, n], np.uint32)
    lpkt = np.concatenate([np.arange(n - 1, -1, -2), np.arange(n - 2, -1, -2)]).astype(np.uint32)
    assert lpkt[0] == n - 1
    try:
        for flags in (0, abi.TX_UDP_CKSUM):
            P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n, flags=flags)
            assert P.stats["replied"] == n
        k60 = [k for k in range(n) if b.length[lpkt[k]] == 60]
        # (the padded ones and the 18-byte payloads, which need no padding)
        assert len(k60) == 20 and sorted({int(P.payload_len[k]) for k in k60}) == [0, 1, 17, 18]
        # one byte less: the last frame no longer lies inside frames_bytes and is not answered
        b2 = F.Batch(b.frames, b.offset, b.length, total - 1)
        db.frames_bytes = total - 1
        P, _ = _run_both(gpu_ctx, b2, db, slots, loff, lpkt, 0, n)
        assert P.reason[0] == "bad_frame" and P.stats["replied"] == n - 1
    finally:
        _free(gpu_ctx, db)


# ---- skips ---------------------------------------------------------------------------------------
def test_bad_entries_and_lane_off_beyond_lane_cap(gpu_ctx, one_lane):
    B, n, b, db, _, _ = one_lane
    slots = _snapshot(gpu_ctx, {}, 4)
    rng = np.random.default_rng(51)
    m = B + 100
    lpkt = rng.integers(0, n, m).astype(np.uint32)
    lpkt[[0, 63, 64, 65, B, m - 1]] = [n, 0xFFFFFFFF, n + 1, 1 << 31, n, n]
    # hand-written offsets: lanes 2 and 3 start beyond lane_cap = m - 10 (clamped to it)
    loff = np.array([0, 50, m + 7, m + 7, m + 9], np.uint32)
    P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, m, lane_cap=m - 10)
    assert P.stats["bad_index"] == 5 and P.reason[m - 10:] == ["past"] * 10
    assert {int(s) for s in P.sockfd if s >= 0} == {0, 1}
    # n smaller than the batch: the entries at and above it are bad indices, their frames unread
    P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 3, m - 3, lane_cap=m - 10, n=n // 2)
    assert P.stats["bad_index"] > 100
    # frames shorter than 42 bytes and descriptors past frames_bytes
    ln = b.length.copy()
    ln[lpkt[5]], ln[lpkt[70]] = 41, 0
    off = b.offset.copy()
    off[lpkt[9]] = b.frames_bytes - 63
    b2 = F.Batch(b.frames, off, ln, b.frames_bytes)
    db2 = abi.RxDeviceBatch(db.frames, b.frames_bytes, gpu_ctx.upload(off), gpu_ctx.upload(ln), None, n)
    lpkt[[0, 63, 64, 65, B, m - 1]] = 1
    P, _ = _run_both(gpu_ctx, b2, db2, slots, np.array([0, m], np.uint32), lpkt, 0, m)
    assert P.reason[5] == P.reason[70] == P.reason[9] == "bad_frame"


# ---- room ----------------------------------------------------------------------------------------
def test_out_cap_cuts_inside_the_range(gpu_ctx):
    """The room ends one byte short of an entry in the middle of a workgroup, at a workgroup's
    first entry, and before the first entry; sizes vary, so the cut is not at a fixed stride."""
    B, _ = abi.tx_reply_geometry(1)
    rng = np.random.default_rng(61)
    n = 3 * B + 50
    b = F.build_frames(rng.integers(42, 300, n).astype(np.uint32), np.full(n, 10001, np.uint32), 61)
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, {}, 2)
    loff, lpkt = np.array([0, n // 3, n], np.uint32), rng.permutation(n).astype(np.uint32)
    try:
        full = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, n)
        for kc in (B + 77, 2 * B, 0, n - 1):
            cap = int(full.frame_off[kc + 1]) - 1
            P, res = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n, out_cap=cap)
            assert P.stats["no_room"] == n - kc and P.stats["bytes_needed"] == full.stats["bytes_needed"]
            end = int(res["frame_off"][n])
            assert end == int(full.frame_off[kc]) and np.all(res["out"][end:] == R.FILL)
        P, _ = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n, out_cap=full.stats["bytes_needed"])
        assert P.stats["no_room"] == 0
    finally:
        _free(gpu_ctx, db)


# ---- MTU and flags -------------------------------------------------------------------------------
def _big_batch(seed):
    """Reassembled-style frames: datagrams of up to 3000 bytes in single frames."""
    rng = np.random.default_rng(seed)
    sizes = np.array([3000 + 42, 1500, 1501, 1514, 1515, 68, 69, 42, 43] + rng.integers(42, 3043, 90).tolist(), np.uint32)
    return F.build_frames(sizes, np.full(len(sizes), 10001, np.uint32), seed)


@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM], ids=["nocksum", "cksum"])
@pytest.mark.parametrize("mtu", [1500, 68])
def test_mtu_and_flags_equal_the_composition(gpu_ctx, mtu, flags):
    """A 3000 B datagram among others at MTU 1500 and 68, checksum on and off: the oracle's image,
    and byte for byte what udpdk_gpu_tx_build_flags makes of host-built descriptors and a gathered
    copy of the payloads (the composition the reply replaces)."""
    b = _big_batch(70 + mtu)
    n = b.n
    db = _upload(gpu_ctx, b)
    slots = _snapshot(gpu_ctx, {}, 3)
    loff = np.array([0, 40, 40, n], np.uint32)
    lpkt = np.random.default_rng(mtu).permutation(n).astype(np.uint32)
    try:
        P, res = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n, mtu=mtu, flags=flags)
        assert P.stats["frames"] > n and int(P.payload_len.max()) == 3000
        # the composition: payloads gathered into 3008-byte slots, descriptors built on the host
        g = abi.rx_alloc_gather(gpu_ctx, n + 1, 3008)         # (a spare slot: the payloads' tailroom)
        g.count = n
        lp = gpu_ctx.upload(lpkt)
        pay, ln, sip, spt = abi.rx_gather_run(gpu_ctx, db, lp, 0, g)
        assert np.array_equal(ln.astype(np.uint16), P.payload_len)
        sock = np.repeat(np.arange(3), np.diff(loff.astype(np.int64))).astype(np.int32)
        spans = np.array([R.span(int(L), mtu)[0] for L in ln], np.int64)
        fo = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(np.uint32)
        cap = int(spans.sum()) + 64
        bufs = [gpu_ctx.upload((np.arange(n) * 3008).astype(np.uint32)), gpu_ctx.upload(ln.astype(np.uint16)),
                gpu_ctx.upload(sock), gpu_ctx.upload(sip), gpu_ctx.upload(spt), gpu_ctx.upload(fo),
                gpu_ctx.upload(np.full(cap + GUARD, R.FILL, np.uint8))]
        tb = abi.TxBatch(g.payload.ptr, n * 3008, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, n)
        cfg = _cfg()
        assert abi.lib().udpdk_gpu_tx_build_flags(gpu_ctx.handle, C.byref(cfg), C.byref(tb),
                                                  C.byref(abi.TxOut(bufs[6].ptr, cap, bufs[5].ptr)), mtu, flags) == 0
        comp = gpu_ctx.download(bufs[6], np.uint8, cap + GUARD)
        assert np.array_equal(comp, res["out"])
        for x in bufs + [lp, g.payload, g.length, g.src_ip, g.src_port]:
            x.free()
    finally:
        _free(gpu_ctx, db)


# ---- loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM], ids=["nocksum", "cksum"])
def test_replies_are_delivered_by_a_mirrored_table(gpu_ctx, flags):
    """The replies go through udpdk_gpu_rx under the peer's bind table (the requests' source port
    bound on the requests' source address): every one is DELIVERED, its IPv4 checksum verifies,
    its UDP checksum is OK with the flag and NONE without, and its payload is its request's."""
    n = 1500
    rng = np.random.default_rng(81)
    b = F.build_frames(rng.integers(42, 400, n).astype(np.uint32), 10001 + rng.integers(0, 3, n).astype(np.uint32), 81)
    lists = {abi.raw_port(10001 + s): [(0, s, 0)] for s in range(3)}
    slots = [(0, abi.raw_port(10001 + s), 1) for s in range(3)]
    db = _upload(gpu_ctx, b)
    _snapshot(gpu_ctx, lists, 3, slots)
    try:
        out = abi.rx_alloc_out(gpu_ctx, n, 3, n)
        _, loff, lpkt, _, rc = abi.rx_run(gpu_ctx, db, out)
        assert rc == 0 and loff[3] == n
        P, res = _run_both(gpu_ctx, b, db, slots, loff, lpkt, 0, n, flags=flags)
        end = int(res["frame_off"][n])
        rb = F.Batch(np.concatenate([res["out"][:end], np.zeros(64, np.uint8)]), res["frame_off"][:n],
                     (P.payload_len.astype(np.uint32) + 42).astype(np.uint16), end)
        # the peer: one socket on 172.31.100.2:10000, where every request came from
        mirror = {abi.raw_port(F.UDP_SRC): [(abi.raw_ip(F.IP_SRC), 0, 0)]}
        gpu_ctx.upload_snapshot(abi.snapshot_from_lists(mirror, 1))
        rdb = _upload(gpu_ctx, rb)
        meta, loff2, lpkt2, cnt, rc = abi.rx_run(gpu_ctx, rdb, abi.rx_alloc_out(gpu_ctx, n, 1, n))
        assert rc == 0 and loff2[1] == n and np.array_equal(lpkt2, np.arange(n))
        assert np.all(abi.meta_verdict(meta) == abi.V_DELIVERED) and np.all((meta >> 4) & 1)
        assert np.all(abi.meta_udp(meta) == (abi.UDP_OK if flags else abi.UDP_NONE))
        pay, ln, _, _ = abi.rx_gather_run(gpu_ctx, rdb, gpu_ctx.upload(lpkt2), 0, abi.rx_alloc_gather(gpu_ctx, n, 368))
        want, wl, _, _ = O.recv_gather(b.frames, b.offset, b.length, lpkt, 0, n, 368)
        assert np.array_equal(ln, wl) and all(pay[k, :ln[k]].tobytes() == want[k, :wl[k]].tobytes() for k in range(n))
        _free(gpu_ctx, rdb)
    finally:
        _free(gpu_ctx, db)


# ---- arguments -----------------------------------------------------------------------------------
def test_argument_errors_write_nothing(gpu_ctx, one_lane):
    B, n, b, db, loff, lpkt = one_lane
    L, EINVAL = abi.lib(), -errno.EINVAL
    slots = _snapshot(gpu_ctx, {}, 1)
    cfg = _cfg()
    bufs = [gpu_ctx.upload(loff), gpu_ctx.upload(lpkt)]
    arrs = [gpu_ctx.upload(np.full(4 * 9, 0xA5, np.uint8)) for _ in range(6)]
    out = gpu_ctx.upload(np.full(4096, R.FILL, np.uint8))

    def call(*, ctx=gpu_ctx.handle, frames=db.frames.ptr, fbytes=b.frames_bytes, offset=db.offset.ptr,
             length=db.length.ptr, lo=bufs[0].ptr, lp=bufs[1].ptr, n_lanes=1, first=0, count=8, mtu=0, flags=0,
             outp=out.ptr, out_cap=4000, plan=None, null_plan=False, null_cfg=False, null_bt=False,
             null_lanes=False, reply=True):
        bt = abi.RxBatch(frames, fbytes, offset, length, None, n)
        ln = abi.RxLanes(None, n, lo, lp, n, n_lanes)
        pl = abi.TxReplyPlan(*(plan or [a.ptr for a in arrs]))
        pb = None if null_bt else C.byref(bt)
        pn = None if null_lanes else C.byref(ln)
        pp = None if null_plan else C.byref(pl)
        if reply:
            return L.udpdk_gpu_tx_reply(ctx, None if null_cfg else C.byref(cfg), pb, pn, first, count, None, mtu,
                                        flags, C.c_void_p(outp) if outp else None, out_cap, pp)
        return L.udpdk_gpu_tx_reply_plan(ctx, pb, pn, first, count, None, mtu, out_cap, pp)

    for reply in (True, False):
        bad = [dict(ctx=None), dict(null_bt=True), dict(null_lanes=True), dict(null_plan=True),
               dict(frames=None), dict(offset=None), dict(length=None), dict(lo=None), dict(lp=None),
               dict(n_lanes=0), dict(n_lanes=abi.MAX_LANES + 1), dict(fbytes=1 << 32), dict(out_cap=1 << 32),
               dict(mtu=67), dict(mtu=1501), dict(mtu=70000), dict(first=0xFFFFFFFF, count=1),
               dict(first=1, count=0xFFFFFFFF)]
        bad += [dict(plan=[None if j == i else a.ptr for j, a in enumerate(arrs)]) for i in range(6)]
        if reply:
            bad += [dict(null_cfg=True), dict(outp=None), dict(outp=out.ptr + 4), dict(flags=2), dict(flags=0x80000001)]
        for kw in bad:
            assert call(reply=reply, **kw) == EINVAL, (reply, kw)
        assert call(reply=reply, count=0) == 0
        # bad arguments are refused for an empty range too
        assert call(reply=reply, count=0, mtu=67) == EINVAL
    # no slot table, then a compat snapshot: a lane is not a sockfd
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists({}, 1))
    assert call() == EINVAL and call(reply=False) == EINVAL
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists({}, 256, lane_mask=0xFF, slots=slots))
    assert call() == EINVAL and call(reply=False) == EINVAL
    gpu_ctx.sync()
    for a in arrs:
        assert np.all(gpu_ctx.download(a, np.uint8, 36) == 0xA5)
    assert np.all(gpu_ctx.download(out, np.uint8, 4096) == R.FILL)
    _snapshot(gpu_ctx, {}, 1)
    assert call() == 0
    for x in bufs + arrs + [out]:
        x.free()


def test_stats_without_a_plan_run():
    with abi.GpuContext(0, max_frames=4096, max_lanes=8) as ctx:
        rc, _ = abi.tx_reply_stats(ctx)
        assert rc == -errno.ENOENT


# ---- pipelining ----------------------------------------------------------------------------------
def test_pipeline_depth_3_gives_the_same_bytes(one_lane):
    """RX calls rotating over three pipes, the reply after each on the context stream: the reply
    joins the pipes, so it sees the lanes its RX call made."""
    B, n, b, db0, _, _ = one_lane
    lists = {abi.raw_port(10001): [(0, 0, 0)]}
    with abi.GpuContext(0, max_frames=1 << 16, max_lanes=8) as ctx:
        slots = _snapshot(ctx, lists, 1)
        ctx.pipeline(3)
        db = _upload(ctx, b)
        outs = [abi.rx_alloc_out(ctx, n, 1, n) for _ in range(3)]
        want = None
        for r in range(4):
            o = outs[r % 3]
            assert abi.rx_enqueue(ctx, db, o) == 0
            loff = np.array([0, n], np.uint32)              # one lane, every frame delivered, in order
            bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, n)
            lanes = abi.RxLanes(o.meta.ptr, n, o.lane_off.ptr, o.lane_pkt.ptr, n, 1)
            arrs = [ctx.alloc(4 * (n + 1)) for _ in range(6)]
            outb = ctx.upload(np.full(64 * n + GUARD, R.FILL, np.uint8))
            cfg = _cfg()
            pl = abi.TxReplyPlan(*[a.ptr for a in arrs])
            assert abi.lib().udpdk_gpu_tx_reply(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(lanes), 0, n, None, 0,
                                                abi.TX_UDP_CKSUM, C.c_void_p(outb.ptr), 64 * n, C.byref(pl)) == 0
            rc, st = abi.tx_reply_stats(ctx)
            assert rc == 0 and st.replied == n and st.frames == n
            got = ctx.download(outb, np.uint8, 64 * n + GUARD)
            if want is None:
                P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, np.arange(n), 0, n)
                want, _ = R.image(P, b.frames, slots, CFG_IP, 0, True, 64 * n + GUARD)
            assert np.array_equal(got, want), r
            for x in arrs + [outb]:
                x.free()
