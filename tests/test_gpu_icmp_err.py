"""udpdk_gpu_icmp_errors on the GPU through the C ABI, exact against the model (tests/icmp_err_util.py):
every lane's word, every count, and nothing written past the lanes. The verdict words come from the
oracle's RX of the same batch, except in the closed loop, which is the device's from end to end."""
import ctypes as C
import errno

import numpy as np
import pytest

import icmp_err_util as E
import icmp_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

TILE = 256                                  # ICMP_ERR_TILE: frames per workgroup of the scan
PAD = 8
OUR = abi.raw_ip(E.OUR_IP)


def _snapshot(ctx, lists, snap_lanes=E.SNAP_LANES, lane_mask=0xFFFFFFFF):
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, snap_lanes, lane_mask))


def _check(ctx, buf, nb, off, ln, meta, lists, peers, n_lanes=E.N_LANES, *, our_ip=OUR, dev=None, sticky=False,
           pipe=0, n=None):
    """Run the stage and the model with the same arguments; compare everything. Returns (err, stats)."""
    n = len(off) if n is None else n
    err, st = E.model(buf, nb, off[:n], ln[:n], meta[:n], lists, peers, n_lanes, our_ip)
    b = dev if dev is not None else abi.rx_upload(ctx, buf, off, ln)
    g = abi.icmp_err_run(ctx, our_ip, b, meta, None if sticky else peers, n_lanes, n=n, pipe=pipe, pad=PAD)
    print("stats", g["stats"], "model", st)
    assert g["rc"] == 0 and g["stats_rc"] == 0
    assert g["stats"] == st
    bad = np.flatnonzero(g["err"][:n_lanes] != err)
    assert bad.size == 0, [(int(l), hex(int(g["err"][l])), hex(int(err[l]))) for l in bad[:8]]
    assert np.all(g["err"][n_lanes:] == 0xA5A5A5A5A5A5A5A5)          # nothing past the lanes
    return err, st


def test_mixed_batch(gpu_ctx):
    M = E.mixed(2, 600)                                              # two workgroups and a partial one
    _snapshot(gpu_ctx, M.lists)
    err, st = _check(gpu_ctx, M.buf, M.nb, M.off, M.ln, M.meta, M.lists, M.peers)
    assert all(st[k] >= 3 for k in ("errors", "msg_bad", "quote_bad", "soft", "no_socket")) and st["reported"] >= 20
    assert int(err[E.LAST_FD]) == ((len(M.off) - 1) << 8) | 2        # the hard error before the final soft one
    assert int(err[E.PAIR[0]]) == int(err[E.PAIR[1]]) != 0           # both reuse sockets
    # fewer lanes than sockets that would match: the higher ones are out
    _check(gpu_ctx, M.buf, M.nb, M.off, M.ln, M.meta, M.lists, M.peers[:7], 7)


def _edge_batch(rng, socks, n):
    """n open-port datagrams with a valid hard error at every wave and workgroup edge below n."""
    conn = [s for s in socks if s.peer and s.fd < E.N_LANES and s.fd not in E.PAIR]
    fl = [E.sent_frame(rng, E.Sock(0, conn[j % 5].peer[0], conn[j % 5].peer[1]),
                       to=(conn[j % 5].ip or E.OUR_IP, conn[j % 5].port)) for j in range(n)]
    edges = sorted({p for p in (0, 63, 64, TILE - 1, TILE, n - 1) if 0 <= p < n})
    for j, p in enumerate(edges):
        fl[p] = E.unreach_frame(E.sent_frame(rng, conn[6 + j]), 3)
    return fl, {conn[6 + j].fd: p for j, p in enumerate(edges)}


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1])
def test_frame_counts(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    socks = E.sockets()
    lists, peers = E.lists_of(socks), E.peers_of(socks, E.N_LANES)
    fl, where = _edge_batch(rng, socks, max(n, 1))
    buf, nb, off, ln = U.pack(fl, aligns=rng.integers(0, 16, len(fl)).tolist())
    meta = E.meta_of(lists, E.SNAP_LANES, buf, nb, off, ln)
    _snapshot(gpu_ctx, lists)
    err, st = _check(gpu_ctx, buf, nb, off, ln, meta, lists, peers, n=n)
    if n == 0:
        assert not err.any() and st == dict.fromkeys(E.STATS, 0)
    else:
        assert {fd: (int(err[fd]) >> 8) - 1 for fd in np.flatnonzero(err)} == where and st["reported"] == len(where)


# the issue's lengths, and 84 / 85: the last message its own lane sums and the first the wave sums
TLS = [56, 57, 63, 64, 65, 84, 85, 120, 576, 1500]


def test_message_lengths_at_every_alignment(gpu_ctx):
    """Every total length at frame offsets 0..15 mod 16, each once intact and once with its last
    message byte flipped (the sums reach the end and stop there: the frames are padded with 0xFF)."""
    rng = np.random.default_rng(7)
    socks = E.sockets()
    lists, peers = E.lists_of(socks), E.peers_of(socks, E.N_LANES)
    conn = [s for s in socks if s.peer and s.fd < E.N_LANES and s.fd not in E.PAIR]
    fl, al = [], []
    for tl in TLS:
        for a in range(16):
            s = conn[(a + tl) % len(conn)]
            f = bytearray(E.unreach_frame(E.sent_frame(rng, s, tl), 3, quote_len=tl - 28) + b"\xff" * (a % 5))
            assert len(f) == 14 + tl + a % 5
            fl.append(bytes(f))
            f[14 + tl - 1] ^= 0x10
            fl.append(bytes(f))
            al += [a, a]
    buf, nb, off, ln = U.pack(fl, al)
    meta = E.meta_of(lists, E.SNAP_LANES, buf, nb, off, ln)
    _snapshot(gpu_ctx, lists)
    err, st = _check(gpu_ctx, buf, nb, off, ln, meta, lists, peers)
    assert st["errors"] == 32 * len(TLS) and st["reported"] == st["msg_bad"] == 16 * len(TLS)


def test_candidates_with_unreadable_descriptors(gpu_ctx):
    """meta names candidates whose descriptors are short or out of range: bad_frame, and no byte of
    them is read; frames that are no candidates carry garbage descriptors that nothing looks at.
    (The buffer keeps its tailroom and is allocated past frames_bytes, so nothing here can fault.)"""
    rng = np.random.default_rng(23)
    socks = E.sockets()
    lists, peers = E.lists_of(socks), E.peers_of(socks, E.N_LANES)
    fl, where = _edge_batch(rng, socks, 300)
    buf, nb, off, ln = U.pack(fl)
    meta = E.meta_of(lists, E.SNAP_LANES, buf, nb, off, ln)
    cand_m = int(meta[0])
    assert cand_m & 0xF == abi.V_NOT_UDP
    off, ln, meta = off.copy(), ln.copy(), meta.copy()
    for p, (o, l) in {1: (0, 41), 2: (0, 0), 3: (nb - 10, 60), 65: (0xFFFFFFF0, 100), 66: (nb, 42),
                      254: (nb - 41, 42), 257: (0x80000000, 65535)}.items():
        off[p], ln[p], meta[p] = o, l, cand_m
    for p in (5, 6, 70, 258):                                        # not candidates: never read
        off[p], ln[p] = 0xFFFFF000 + p, 65535
    meta[7] = cand_m & ~0x10                                         # a bad header checksum by meta
    meta[8] = cand_m | 0x100                                         # IHL != 5 by meta
    meta[9] = (cand_m & ~0xF) | abi.V_FRAG
    big = np.concatenate([buf, np.zeros(4096, np.uint8)])            # allocated well past frames_bytes
    dev = abi.rx_upload(gpu_ctx, big, off, ln)
    dev.frames_bytes = nb
    _snapshot(gpu_ctx, lists)
    err, st = _check(gpu_ctx, buf, nb, off, ln, meta, lists, peers, dev=dev)
    assert st["bad_frame"] == 7 and st["reported"] == len(where) == st["errors"]


def test_no_candidate(gpu_ctx):
    rng = np.random.default_rng(29)
    socks = E.sockets()
    lists, peers = E.lists_of(socks), E.peers_of(socks, E.N_LANES)
    s = socks[0]
    fl = [E.sent_frame(rng, E.Sock(0, s.peer[0], s.peer[1]), j % 40, to=(s.ip, s.port)) for j in range(2 * TILE + 17)]
    buf, nb, off, ln = U.pack(fl)
    meta = E.meta_of(lists, E.SNAP_LANES, buf, nb, off, ln)
    assert np.all((meta & 0xF) == abi.V_DELIVERED)
    _snapshot(gpu_ctx, lists)
    err, st = _check(gpu_ctx, buf, nb, off, ln, meta, lists, peers)
    assert not err.any() and st == dict.fromkeys(E.STATS, 0)


def test_closed_loop_on_the_device(gpu_ctx):
    """A client's connected sockets send to a closed port of a server; the server's RX and ICMP answer
    stage build the errors; those frames, where they lie, are the client's next batch: its RX, then
    the error stage, report code 3 to exactly the sending sockets with their last error's index."""
    L, ctx = abi.lib(), gpu_ctx
    rng = np.random.default_rng(31)
    client, server = "172.31.100.2", U.OUR_IP
    socks = [E.Sock(fd, None if fd % 2 else client, 30000 + fd, 0, (server, U.CLOSED_PORT)) for fd in range(6)]
    socks += [E.Sock(6, None, 30006, 0, None), E.Sock(7, None, 30007, 0, (server, 8))]
    order = [int(k) for k in rng.integers(0, 8, 300)]
    reqs = [E.sent_frame(rng, socks[k], 10 + j % 50, our_ip=client, to=(server, U.CLOSED_PORT))
            for j, k in enumerate(order)]
    buf, nb, off, ln = U.pack(reqs, aligns=rng.integers(0, 16, len(reqs)).tolist())
    n = len(order)
    # the server: RX, then the answers
    _snapshot(ctx, U.LISTS, U.N_LANES)
    b1 = abi.rx_upload(ctx, buf, off, ln)
    o1 = abi.rx_alloc_out(ctx, n, U.N_LANES, n)
    assert abi.rx_enqueue(ctx, b1, o1) == 0
    cap = 70 * n
    out, ro, og = ctx.alloc(cap + 64), ctx.alloc(4 * (n + 1)), ctx.alloc(4 * n)
    cfg = U.tx_config(server)
    bt1 = abi.RxBatch(b1.frames.ptr, b1.frames_bytes, b1.offset.ptr, b1.length.ptr, None, n)
    io = abi.IcmpOut(out.ptr, cap, ro.ptr, og.ptr, n)
    assert L.udpdk_gpu_icmp_reply(ctx.handle, C.byref(cfg), C.byref(bt1), C.c_void_p(o1.meta.ptr), U.UNREACH, 0,
                                  U.NO_LIMIT, C.byref(io)) == 0
    ist = abi.IcmpStats()
    assert L.udpdk_gpu_icmp_stats(ctx.handle, C.byref(ist)) == 0
    assert ist.unreach_sent == n and ist.bytes_needed == cap
    # the client: the replies where the stage wrote them (reply_off is the offsets; every length 70)
    lists = E.lists_of(socks)
    _snapshot(ctx, lists, 8)
    peers = E.peers_of(socks, 8)
    ctx.rx_peer(peers)
    try:
        b2 = abi.RxDeviceBatch(abi.DevRef(out.ptr), cap, abi.DevRef(ro.ptr), ctx.upload(np.full(n, 70, np.uint16)), None, n)
        o2 = abi.rx_alloc_out(ctx, n, 8, n)
        assert abi.rx_enqueue(ctx, b2, o2) == 0
        errd = ctx.upload(np.full(8 + PAD, 0xA5A5A5A5A5A5A5A5, np.uint64))
        bt2 = abi.RxBatch(out.ptr, cap, ro.ptr, b2.length.ptr, None, n)
        assert L.udpdk_gpu_icmp_errors(ctx.handle, abi.raw_ip(client), C.byref(bt2), C.c_void_p(o2.meta.ptr), None, 8,
                                       C.c_void_p(errd.ptr)) == 0
        st = abi.IcmpErrStats()
        assert L.udpdk_gpu_icmp_err_stats(ctx.handle, C.byref(st)) == 0
        err = ctx.download(errd, np.uint64, 8 + PAD)
    finally:
        ctx.rx_peer(None)
    last = {k: j for j, k in enumerate(order)}
    assert set(last) == set(range(8))
    assert err[:8].tolist() == [((last[fd] + 1) << 8 | 3) if fd < 6 else 0 for fd in range(8)]
    assert np.all(err[8:] == 0xA5A5A5A5A5A5A5A5)
    n67 = order.count(6) + order.count(7)                            # unconnected; connected to another port
    got = {k: getattr(st, k) for k in E.STATS}
    assert got == dict(errors=n, msg_bad=0, quote_bad=0, soft=0, no_socket=n67, reported=n - n67, bad_frame=0)


def test_explicit_and_sticky_peer_tables(gpu_ctx):
    M = E.mixed(3, 400)
    _snapshot(gpu_ctx, M.lists)
    dev = abi.rx_upload(gpu_ctx, M.buf, M.off, M.ln)
    args = (gpu_ctx, M.buf, M.nb, M.off, M.ln, M.meta, M.lists, M.peers)
    want, wst = _check(*args, dev=dev)
    gpu_ctx.rx_peer(None)
    g = abi.icmp_err_run(gpu_ctx, OUR, dev, M.meta, None, E.N_LANES)
    assert g["rc"] == -errno.ENOENT and np.all(g["err"] == 0xA5A5A5A5A5A5A5A5)   # off: nothing enqueued
    try:
        gpu_ctx.rx_peer(M.peers)
        err, st = _check(*args, dev=dev, sticky=True)
        assert np.array_equal(err, want) and st == wst
        # a sticky table shorter than the call's lanes: the lanes past it are off
        gpu_ctx.rx_peer(M.peers[:9])
        short = M.peers.copy()
        short[9:] = (0, 0, 0)
        err, st = _check(*args[:7], short, dev=dev, sticky=True)
        assert not err[9:].any() and err[:9].any() and st["no_socket"] > wst["no_socket"]
    finally:
        gpu_ctx.rx_peer(None)


def test_argument_errors(gpu_ctx):
    L = abi.lib()
    M = E.mixed(4, 200)
    _snapshot(gpu_ctx, M.lists)
    b = abi.rx_upload(gpu_ctx, M.buf, M.off, M.ln)
    md = gpu_ctx.upload(M.meta)
    pd = gpu_ctx.upload(M.peers.view(np.uint8))
    ed = gpu_ctx.upload(np.full(E.N_LANES + 2, 0xA5A5A5A5A5A5A5A5, np.uint64))
    st = abi.IcmpErrStats()

    def call(ctx=gpu_ctx, batch=True, meta=md.ptr, peer=pd.ptr, lanes=E.N_LANES, err=ed.ptr, fb=M.nb, n=len(M.off),
             pipe=0, frames=b.frames.ptr):
        bt = abi.RxBatch(frames, fb, b.offset.ptr, b.length.ptr, None, n)
        a = (OUR, C.byref(bt) if batch else None, C.c_void_p(meta), C.c_void_p(peer), lanes, C.c_void_p(err))
        if pipe:
            return L.udpdk_gpu_pipe_icmp_errors(ctx.handle if ctx else None, pipe, *a)
        return L.udpdk_gpu_icmp_errors(ctx.handle if ctx else None, *a)
    for kw in (dict(ctx=None), dict(batch=False), dict(meta=None), dict(err=None), dict(peer=pd.ptr + 4),
               dict(err=ed.ptr + 4), dict(lanes=0), dict(lanes=16385), dict(fb=1 << 32), dict(frames=None),
               dict(pipe=4), dict(pipe=-1)):
        assert call(**kw) == -errno.EINVAL, kw
    assert call(peer=None) == -errno.ENOENT                          # no sticky table
    with abi.GpuContext(0, max_frames=1024, max_lanes=64) as fresh:
        assert L.udpdk_gpu_icmp_err_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
        assert L.udpdk_gpu_pipe_icmp_err_stats(fresh.handle, 1, C.byref(st)) == -errno.ENOENT
        assert call(ctx=fresh) == -errno.EINVAL                      # no snapshot
        fresh.upload_snapshot(abi.snapshot_from_lists(M.lists, 64, 0xFF))
        assert call(ctx=fresh) == -errno.EINVAL                      # compat mode: a lane is not a sockfd
        assert L.udpdk_gpu_icmp_err_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
    assert L.udpdk_gpu_pipe_icmp_err_stats(gpu_ctx.handle, 0, C.byref(st)) == -errno.EINVAL
    assert L.udpdk_gpu_pipe_icmp_err_stats(gpu_ctx.handle, 4, C.byref(st)) == -errno.EINVAL
    gpu_ctx.sync()
    assert np.all(gpu_ctx.download(ed, np.uint64, E.N_LANES + 2) == 0xA5A5A5A5A5A5A5A5)   # nothing was enqueued
    # an empty batch clears the lanes, and only them
    assert call(n=0) == 0 and L.udpdk_gpu_icmp_err_stats(gpu_ctx.handle, C.byref(st)) == 0
    got = gpu_ctx.download(ed, np.uint64, E.N_LANES + 2)
    assert not got[:E.N_LANES].any() and np.all(got[E.N_LANES:] == 0xA5A5A5A5A5A5A5A5)
    assert [getattr(st, k) for k in E.STATS] == [0] * 7
    assert call() == 0 and L.udpdk_gpu_icmp_err_stats(gpu_ctx.handle, C.byref(st)) == 0 and st.reported > 0


def test_pipes_equal_the_stream_call(gpu_ctx):
    M = E.mixed(5, 700)
    _snapshot(gpu_ctx, M.lists)
    dev = abi.rx_upload(gpu_ctx, M.buf, M.off, M.ln)
    args = (gpu_ctx, M.buf, M.nb, M.off, M.ln, M.meta, M.lists, M.peers)
    want, wst = _check(*args, dev=dev)
    gpu_ctx.pipeline(4)
    try:
        for pipe in (1, 2, 3, 1):                                    # back to back; pipe 1 reuses its workspace
            err, st = _check(*args, dev=dev, pipe=pipe)
            assert np.array_equal(err, want) and st == wst
        err, st = _check(*args, dev=dev)                             # the context stream joins the pipes
        assert np.array_equal(err, want) and st == wst
    finally:
        gpu_ctx.pipeline(1)
