"""The RX drop filter on the GPU, exact against the numpy model (rx_drop_util.py, pinned against
the oracle in test_rx_drop_ref.py): udpdk_gpu_rx_filter over synthetic lane sets (entry counts
around the chunk and tile sizes, lane counts up to the maximum, lane starts at every residue,
empty lanes, bounds), the sticky mode (udpdk_gpu_rx_drop) behind every launch form of
udpdk_gpu_rx and the host-batch entry points, and the socket layer ([gpu] rx_drop)."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import oracle as O
import rx_drop_util as U
from reasm_util import batch
from test_gpu_rx import IP1, IP9, MIXED_LISTS
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

E = 1024                    # entries per filter tile (FLT_TILE, rx_filter.h)
PREFIX_THREADS = 256        # rx_filter_base: one tile per thread in a single pass up to here
SENT = 0xA5A5A5A5
FLAG_SETS = (0, 1, 2, 4, 8, 15)


def synth(seed, d, n_lanes, n=None, cuts=None, p_bad=0.25):
    """Random verdict words with the four reasons drawn independently (every other bit random),
    d random entries with repeats (fan-out), n_lanes lanes cut at random places (or at `cuts`)."""
    rng = np.random.default_rng(seed)
    n = max(1, d // 2) if n is None else n
    meta = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFFFE0F)
    meta |= (rng.random(n) >= p_bad).astype(np.uint32) << 4            # IPv4 checksum ok
    meta |= rng.choice(3, n, p=[p_bad, 1 - 2 * p_bad, p_bad]).astype(np.uint32) << 5
    meta |= (rng.random(n) < p_bad).astype(np.uint32) << 7
    meta |= (rng.random(n) < p_bad).astype(np.uint32) << 8
    pkt = rng.integers(0, n, d, dtype=np.uint32)
    if cuts is None:
        cuts = np.sort(rng.integers(0, d + 1, n_lanes - 1))
    off = np.concatenate([[0], np.asarray(cuts, np.int64), [d]]).astype(np.uint32)
    assert len(off) == n_lanes + 1
    return meta, off, pkt


def check(ctx, meta, off, pkt, flags, what, **kw):
    m = U.model(meta, off, pkt, flags, kw.get("n"), kw.get("lane_cap"))
    goff, gpkt, st, rc = abi.rx_filter_run(ctx, meta, off, pkt, flags, pad=64, fill=SENT, **kw)
    cap = len(gpkt) - 64
    assert rc == (0 if m.kept <= cap else -errno.ENOSPC), what
    assert np.array_equal(goff, m.lane_off), what
    w = min(m.kept, cap)
    assert np.array_equal(gpkt[:w], m.lane_pkt[:w]), what
    assert np.all(gpkt[w:] == SENT), f"{what}: written past the kept entries"
    assert (list(st.dropped), st.kept, st.removed, st.bad_index, st.truncated) == \
        (m.dropped, m.kept, m.removed, m.bad_index, m.truncated), what
    return m


@pytest.mark.parametrize("d", [0, 1, 63, 64, 65, E - 1, E, E + 1, 2 * E + 1, (PREFIX_THREADS + 44) * E + 17])
def test_entry_counts(gpu_ctx, d):
    """Entry counts around a ballot chunk and a tile, and one with more tiles than the tile
    prefix's threads (two tiles per thread), under every single flag, all four and none."""
    assert d < 1 << 19
    meta, off, pkt = synth(100 + d % 97, d, 7)
    for flags in FLAG_SETS:
        m = check(gpu_ctx, meta, off, pkt, flags, f"d={d} flags={flags}")
        if flags == 0:                                  # the identity copy
            assert np.array_equal(m.lane_off, off) and np.array_equal(m.lane_pkt, pkt)
        elif d >= 63:
            assert 0 < m.removed < d


def test_workspace_grows_and_is_reused():
    """A fresh context's first three calls: one tile, then three (the workspace has to grow), then
    one again (the larger workspace is reused, with the second call's rows and masks beyond the
    live ones); lanes and stats exact after each."""
    ctx = abi.GpuContext(0, max_frames=1 << 12, max_lanes=8)
    try:
        for step, d in enumerate((64, 2 * E + 1, 64)):
            meta, off, pkt = synth(900 + step, d, 7)
            m = check(ctx, meta, off, pkt, 15, f"step {step} d={d}")
            assert 0 < m.removed < d
    finally:
        ctx.close()


@pytest.mark.parametrize("n_lanes", [1, 2, 7, 4096, 16384])
@pytest.mark.parametrize("d", [5000, 40000])
def test_lane_counts(gpu_ctx, n_lanes, d):
    """One lane to UDPDK_GPU_MAX_LANES (more than the context's snapshot may have): the work is
    the same, only the offsets kernel's grid grows. Many lanes of a few (or no) entries."""
    meta, off, pkt = synth(n_lanes + d, d, n_lanes)
    for flags in (15, 2):
        check(gpu_ctx, meta, off, pkt, flags, f"lanes={n_lanes} d={d} flags={flags}")


def test_lane_starts_and_empty_lanes(gpu_ctx):
    """Lane starts at every residue mod 64, on and around tile ends, and runs of empty lanes at
    the front, in the middle and at the end."""
    d = 3 * E + 100
    starts = sorted(set([k * 65 for k in range(1, 48)] + [E - 1, E, E + 1, 2 * E - 1, 2 * E, 2 * E + 1,
                                                          3 * E, 3 * E + 63, 3 * E + 64]))
    assert {s % 64 for s in starts} >= set(range(1, 48)) | {0, 63}
    cuts = [0] * 9 + starts[:20] + [starts[20]] * 12 + starts[20:] + [d] * 10
    meta, off, pkt = synth(5, d, len(cuts) + 1, cuts=cuts)
    for flags in (15, 1, 0):
        check(gpu_ctx, meta, off, pkt, flags, f"starts flags={flags}")
    # every residue of the last entry's chunk as well: the offsets 2E-64 .. 2E+64 one by one
    cuts = list(range(2 * E - 64, 2 * E + 65))
    meta, off, pkt = synth(6, d, len(cuts) + 1, cuts=cuts)
    check(gpu_ctx, meta, off, pkt, 15, "residues")


def test_all_kept_and_all_dropped(gpu_ctx):
    d = 2 * E + 77
    meta, off, pkt = synth(7, d, 5)
    good = (meta & np.uint32(0xFFFFFE0F)) | np.uint32(0x30)           # ip ok, udp ok, no flags
    m = check(gpu_ctx, good, off, pkt, 15, "all kept")
    assert m.removed == 0 and np.array_equal(m.lane_pkt, pkt)
    bad = (meta & np.uint32(0xFFFFFE0F)) | np.uint32(0x50)            # udp bad
    m = check(gpu_ctx, bad, off, pkt, 2, "all dropped")
    assert m.kept == 0 and not m.lane_off.any()
    m = check(gpu_ctx, bad, off, pkt, 13, "bad but not selected")
    assert m.removed == 0


def test_bounds(gpu_ctx):
    """Entries >= n are removed without a verdict load and counted; a total beyond lane_cap is
    truncated and nothing past lane_cap influences the output (the tail holds a sentinel that
    would be a bad index); out_cap below the kept count gives ENOSPC with the first out_cap
    entries and nothing written past them; offsets that are not monotonic or beyond the total
    stay in bounds."""
    d = 2 * E + 300
    meta, off, pkt = synth(8, d, 6)
    n = len(meta)
    pkt2 = pkt.copy()
    pkt2[::37] = np.array([n, n + 1, 0x7FFFFFFF, 0xFFFFFFFF] * len(pkt2[::37]), np.uint32)[:len(pkt2[::37])]
    for flags in (0, 15):
        m = check(gpu_ctx, meta, off, pkt2, flags, f"bad index flags={flags}")
        assert m.bad_index == len(pkt2[::37])
    # n below the verdict array: the entries past it count as bad indices
    check(gpu_ctx, meta, off, pkt, 15, "n cut", n=n // 2)
    # truncated input
    cap = d - 500
    tail = pkt.copy()
    tail[cap:] = SENT
    m = check(gpu_ctx, meta, off, tail, 15, "truncated", lane_cap=cap)
    assert m.truncated == 1 and m.bad_index == 0 and m.lane_off[-1] == m.kept
    # out_cap below kept
    m = check(gpu_ctx, meta, off, pkt, 2, "out_cap", out_cap=700)
    assert m.kept > 700
    check(gpu_ctx, meta, off, pkt, 2, "out_cap 0", out_cap=0)
    # offsets out of order and past the total (no lane set of udpdk_gpu_rx looks like this)
    wild = off.copy()
    wild[2], wild[3] = 0xFFFFFFFF, 5
    check(gpu_ctx, meta, wild, pkt, 15, "wild offsets")


def test_filter_arguments(gpu_ctx):
    L = abi.lib()
    lanes = abi.RxLanes(None, 0, None, None, 0, 1)
    assert L.udpdk_gpu_rx_filter(gpu_ctx.handle, C.byref(lanes), 0, None, None, 0) == -errno.EINVAL
    buf = gpu_ctx.alloc(64)
    try:
        lanes = abi.RxLanes(None, 0, buf.ptr, None, 0, 1)
        assert L.udpdk_gpu_rx_filter(gpu_ctx.handle, C.byref(lanes), 16, C.c_void_p(buf.ptr), None, 0) == -errno.EINVAL
        lanes.n_lanes = 16385
        assert L.udpdk_gpu_rx_filter(gpu_ctx.handle, C.byref(lanes), 0, C.c_void_p(buf.ptr), None, 0) == -errno.EINVAL
    finally:
        buf.free()
    assert L.udpdk_gpu_rx_drop(gpu_ctx.handle, 16) == -errno.EINVAL
    assert gpu_ctx.rx_drop(-1) == 0


# ---- sticky mode behind udpdk_gpu_rx ------------------------------------------------------------
def mixed(seed, n=3000):
    return F.mixed_batch(seed, n, [10001, 10002, 10003, 10004, 10005], [9, 20000, 65535], [IP1, IP9])


def oracle_rx(b, lists, n_lanes):
    return O.rx(O.bindtable_from_lists(lists), b.frames, b.frames_bytes, b.offset, b.length, b.ptype, n_lanes)


def upload(ctx, b, n_lanes, cap):
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, b.ptype)
    db.frames_bytes = b.frames_bytes
    return db, abi.rx_alloc_out(ctx, b.n, n_lanes, cap)


def free(db, out):
    for x in (db.frames, db.offset, db.length, db.ptype, out.meta, out.lane_off, out.lane_pkt):
        if x is not None:
            x.free()


def sticky(ctx, b, lists, n_lanes, flags, what, want=None, cap=None):
    """One udpdk_gpu_rx under drop `flags`: verdict words and counters are the oracle's, the lanes
    the model's, deliveries == lane_off[n_lanes] == kept; then the same call with the mode back
    at 0 gives the oracle's lanes."""
    want = want or oracle_rx(b, lists, n_lanes)
    m = U.model(want[0], want[1], want[2], flags)
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, n_lanes))
    db, out = upload(ctx, b, n_lanes, cap or max(1, len(want[2])))
    try:
        assert ctx.rx_drop(flags) == 0
        try:
            gm, gl, gp, gc, rc = abi.rx_run(ctx, db, out)
            drc, dst = abi.rx_drop_stats(ctx)
        finally:
            assert ctx.rx_drop(0) == flags
        assert rc == 0 and drc == 0, what
        assert np.array_equal(gm, want[0]), f"{what}: verdict words"
        assert np.array_equal(gc, want[3]), f"{what}: counters"
        assert np.array_equal(gl, m.lane_off), f"{what}: lane_off"
        assert len(gp) == m.kept == int(gl[n_lanes]), f"{what}: deliveries"
        assert np.array_equal(gp, m.lane_pkt), f"{what}: lane entries"
        assert (list(dst.dropped), dst.kept, dst.removed) == (m.dropped, m.kept, m.removed), what
        gm, gl, gp, gc, rc = abi.rx_run(ctx, db, out)
        assert rc == 0 and np.array_equal(gl, want[1]) and np.array_equal(gp, want[2]), f"{what}: mode 0"
    finally:
        free(db, out)
    return m


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sticky_eight_lanes_fanout(gpu_ctx, seed):
    b = mixed(seed)
    want = oracle_rx(b, MIXED_LISTS, 8)
    for flags in (15, 2, 9):
        m = sticky(gpu_ctx, b, MIXED_LISTS, 8, flags, f"seed={seed} flags={flags}", want)
        assert m.removed > 100


LISTS1 = {abi.raw_port(10001): [(0, 0, 0)]}


def corrupt(b, rows, size=64):
    """One payload byte of each of the frames `rows` flipped: their UDP checksums fail."""
    v = b.frames[:b.n * size].reshape(b.n, size)
    v[rows, 50] ^= 0x21


@pytest.mark.parametrize("fuse", [1, 0], ids=["fused", "compact1"])
def test_sticky_single_lane_forms(fuse, monkeypatch):
    """One lane without fan-out, the fused completion and rx_classify + rx_compact1, each forced
    as test_gpu_rx_forms.py forces them: the stage follows both returns of the single-lane path.
    All frames delivered but the corrupted ones flagged, then with not-full tiles too."""
    monkeypatch.setenv("UDPDK_RX_FUSE", str(fuse))
    ctx = abi.GpuContext(0, max_frames=1 << 16, max_lanes=64)
    try:
        for k, n in enumerate((5000, 1025, 64)):
            b = F.build_frames(np.full(n, 64, np.uint32), np.full(n, 10001, np.uint32), 200 + k)
            corrupt(b, np.arange(3, n, 7))
            if k == 0:
                v = b.frames[:n * 64].reshape(n, 64)
                v[1100:1300:3, 36:38] = (0x4E, 0x20)             # unbound port: a tile not full
            for _ in range(2):
                m = sticky(ctx, b, LISTS1, 1, 2, f"fuse={fuse} n={n}")
            assert m.removed >= n // 8
    finally:
        ctx.close()


def test_sticky_4096_lanes(gpu_ctx):
    w = F.config_batch(5, 100000)
    corrupt(w.batch, np.arange(0, 100000, 50))
    m = sticky(gpu_ctx, w.batch, w.port_lists(), w.n_sockets, 15, "zipf 4096")
    assert m.removed == 2000 and m.dropped == [0, 2000, 0, 0]


def test_sticky_lane_overflow(gpu_ctx):
    """lane_cap below the deliveries: overflow and ENOSPC are still the pre-filter total's, the
    filtered lanes those of the truncated input."""
    b = mixed(4)
    want = oracle_rx(b, MIXED_LISTS, 8)
    cap = len(want[2]) - 400
    m = U.model(want[0], want[1], want[2], 15, lane_cap=cap)
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists(MIXED_LISTS, 8))
    db, out = upload(gpu_ctx, b, 8, cap)
    try:
        gpu_ctx.rx_drop(15)
        try:
            gm, gl, gp, gc, rc = abi.rx_run(gpu_ctx, db, out)
            _, dst = abi.rx_drop_stats(gpu_ctx)
        finally:
            gpu_ctx.rx_drop(0)
        assert rc == -errno.ENOSPC and dst.truncated == 1
        assert np.array_equal(gm, want[0]) and np.array_equal(gc, want[3])
        assert np.array_equal(gl, m.lane_off) and np.array_equal(gp, m.lane_pkt)
    finally:
        free(db, out)


def test_sticky_pipeline_depth_3(gpu_ctx):
    """Three batches in flight on three pipes, each filtered on its own stream."""
    bs = [mixed(10 + k, 2000 + 500 * k) for k in range(3)]
    wants = [oracle_rx(b, MIXED_LISTS, 8) for b in bs]
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists(MIXED_LISTS, 8))
    devs = [upload(gpu_ctx, b, 8, len(w[2])) for b, w in zip(bs, wants)]
    try:
        gpu_ctx.pipeline(3)
        gpu_ctx.rx_drop(15)
        try:
            for _ in range(2):
                for db, out in devs:
                    assert abi.rx_enqueue(gpu_ctx, db, out) == 0
            rc, st = abi.rx_stats(gpu_ctx)
            gpu_ctx.sync()
        finally:
            gpu_ctx.rx_drop(0)
            gpu_ctx.pipeline(1)
        for k, ((db, out), w) in enumerate(zip(devs, wants)):
            m = U.model(w[0], w[1], w[2], 15)
            assert np.array_equal(gpu_ctx.download(out.meta, np.uint32, out.n), w[0]), k
            assert np.array_equal(gpu_ctx.download(out.lane_off, np.uint32, 9), m.lane_off), k
            assert np.array_equal(gpu_ctx.download(out.lane_pkt, np.uint32, m.kept), m.lane_pkt), k
        assert rc == 0 and st.deliveries == m.kept
    finally:
        for db, out in devs:
            free(db, out)


def test_sticky_rx_host_and_async(gpu_ctx):
    L = abi.lib()
    b = mixed(21, 2000)
    want = oracle_rx(b, MIXED_LISTS, 8)
    m = U.model(want[0], want[1], want[2], 15)
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists(MIXED_LISTS, 8))

    def call(fn, depth, reps):
        gpu_ctx.pipeline(depth)
        res = []
        try:
            for _ in range(reps):
                meta, loff, pkt = np.zeros(b.n, np.uint32), np.zeros(9, np.uint32), np.zeros(4 * b.n, np.uint32)
                st = abi.RxStats()
                assert fn(gpu_ctx.handle, b.frames.ctypes.data, b.frames_bytes, b.offset.ctypes.data,
                          b.length.ctypes.data, None, b.n, meta.ctypes.data, loff.ctypes.data,
                          pkt.ctypes.data, 4 * b.n, C.byref(st)) == 0
                res.append((meta, loff, pkt, st))
            if fn is L.udpdk_gpu_rx_host_async:
                assert L.udpdk_gpu_rx_host_wait(gpu_ctx.handle) == 0
        finally:
            gpu_ctx.pipeline(1)
        return res

    for fn, depth in ((L.udpdk_gpu_rx_host, 1), (L.udpdk_gpu_rx_host_async, 1), (L.udpdk_gpu_rx_host_async, 3)):
        gpu_ctx.rx_drop(15)
        try:
            res = call(fn, depth, 3)
        finally:
            gpu_ctx.rx_drop(0)
        for meta, loff, pkt, st in res:
            assert np.array_equal(meta, want[0]) and np.array_equal(loff, m.lane_off)
            assert st.deliveries == m.kept and st.overflow == 0
            assert np.array_equal(pkt[:m.kept], m.lane_pkt)
            assert np.array_equal(np.array(st.counters[:], np.uint64), want[3])
        for meta, loff, pkt, st in call(fn, depth, 1):              # mode 0 again
            assert np.array_equal(loff, want[1]) and np.array_equal(pkt[:st.deliveries], want[2])


# ---- socket layer -------------------------------------------------------------------------------
def init(tmp_path, extra):
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.2\n"
                   "[port0_dst]\nmac_addr = 68:05:ca:95:fa:64\n"
                   "[gpu]\nmax_frames = 65536\nmax_lanes = 16\n"
                   "frag_buckets = 16\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    assert abi.lib().udpdk_init(3, argv) == 0


def poll(frames):
    buf, off, ln = batch(frames)
    st = abi.RxStats()
    assert abi.lib().udpdk_poll_rx(buf.ctypes.data, len(buf) - 64, off.ctypes.data, ln.ctypes.data, None,
                                   len(off), C.byref(st)) == 0
    return st


def drain(api, s):
    abi.lib().udpdk_interrupt(0)                # recvfrom on an empty ring: -1 instead of waiting
    out = []
    while True:
        n, data, _ = api.recvfrom(s, 70000)
        if n < 0:
            return out
        out.append(data)


def flip(frame, at):
    f = bytearray(frame)
    f[at] ^= 0x40
    return bytes(f)


@pytest.mark.parametrize("extra,drop", [("rx_drop = udp\n", True), ("rx_drop = none\n", False), ("", False),
                                        ("rx_drop = len, udp\ndevices = 0,0\n", True)],
                         ids=["udp", "none", "default", "udp-two-shards"])
def test_socket_layer_drops_corrupt_datagrams(tmp_path, host_api, extra, drop):
    """[gpu] rx_drop = udp: a plain datagram with a corrupted payload byte and a datagram GPU TX
    built with its checksum and fragmented, one byte of its second fragment corrupted on the way,
    never reach recvfrom; the intact ones arrive in order and udpdk_rx_dropped counts the two.
    Without the key (or with none) both come through, as they always did."""
    init(tmp_path, extra)
    try:
        assert host_api.config_rx_drop(-1) == (2 if "devices" not in extra else 6) * drop
        rx, tx = host_api.socket(), host_api.socket()
        assert host_api.bind(rx, "0.0.0.0", 10001) == 0
        assert host_api.bind(tx, "10.1.2.3", 5353) == 0
        host_api.config_tx_cksum(1)
        rng = np.random.default_rng(77)
        big = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
        assert host_api.sendto(tx, big, "172.31.100.1", 10001) == len(big)
        frags = host_api.tx_drain()
        assert len(frags) == 3 and frags[0][40:42] != b"\0\0"
        plain = [F.make_frame(rng, dport=10001, dst_ip="172.31.100.1", payload_len=100 + k) for k in range(4)]
        pay = [f[42:] for f in plain]
        st1 = poll([plain[0], flip(plain[1], 60), frags[0], flip(frags[1], 700), frags[2], plain[2]])
        st2 = poll([frags[0], frags[1], frags[2], plain[3]])
        got = drain(host_api, rx)
        bad_big = big[:1480 - 8 + 700 - 34] + bytes([big[1480 - 8 + 700 - 34] ^ 0x40]) + big[1480 - 8 + 700 - 33:]
        if drop:
            assert got == [pay[0], pay[2], big, pay[3]]
            assert host_api.rx_dropped() == 2
            assert st1.deliveries == 2 and st1.counters[abi.C_DELIVERIES] == 3
        else:
            assert got == [pay[0], flip(plain[1], 60)[42:], bad_big, pay[2], big, pay[3]]
            assert host_api.rx_dropped() == 0
            assert st1.deliveries == 3
        assert st2.deliveries == 1 and st1.counters[abi.C_UDP_BAD] == 1
    finally:
        abi.lib().udpdk_cleanup()


def test_socket_layer_chunked_poll(tmp_path, host_api):
    """The pipelined poll (as test_gpu_host_path.py sets it up: poll_chunk_mb = 1 over a batch of
    ~3 MB) filters every chunk on its own pipe; set through udpdk_config_rx_drop after init."""
    init(tmp_path, "poll_chunk_mb = 1\npoll_chunk_min_avg = 0\n")
    try:
        assert host_api.config_rx_drop(abi.RX_DROP_UDP_CKSUM) == 0
        socks = [host_api.socket() for _ in range(2)]
        for k, s in enumerate(socks):
            assert host_api.bind(s, "0.0.0.0", 10001 + k) == 0
        rng = np.random.default_rng(78)
        n = 2200
        frames = [F.make_frame(rng, dport=10001 + k % 2, dst_ip="172.31.100.1", payload_len=1400) for k in range(n)]
        bad = set(range(13, n, 100))
        st = poll([flip(f, 500) if k in bad else f for k, f in enumerate(frames)])
        assert st.counters[abi.C_DELIVERIES] == n and st.deliveries == n - len(bad)
        assert host_api.rx_dropped() == len(bad)
        for k, s in enumerate(socks):
            assert drain(host_api, s) == [f[42:] for i, f in enumerate(frames) if i % 2 == k and i not in bad]
        host_api.config_rx_drop(0)
        poll([flip(frames[0], 500), frames[1]])
        assert drain(host_api, socks[0]) == [flip(frames[0], 500)[42:]] and host_api.rx_dropped() == len(bad)
    finally:
        abi.lib().udpdk_cleanup()
