"""Connected sockets through the socket layer on the GPU: udpdk_connect's peer filter in
udpdk_poll_rx (one-piece, chunked, sharded and RSS-dispatched polls, reassembled datagrams, ring
admission) and udpdk_poll_echo, against what rx_peer_util.py's rule says each ring holds.

Socket 0 is bound to ANY:10001 and connected to U.PEER; socket 1 is bound to ANY:10002 and not
connected. Every payload names its frame, so a ring's content is a list of frame indices."""
import ctypes as C
import errno
import socket

import numpy as np
import pytest

import rx_peer_util as U
from reasm_util import batch, split, udp_datagram
from test_gpu_rx_balance import drain, init, poll_slice
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

PA, PB = 10001, 10002
IP1 = "172.31.100.1"
SOURCES = [U.PEER] + U.STRANGERS


def two_sockets(api, connect=True):
    s0, s1 = api.socket(), api.socket()
    assert (s0, s1) == (0, 1)
    assert api.bind(s0, "0.0.0.0", PA) == 0 and api.bind(s1, "0.0.0.0", PB) == 0
    if connect:
        assert api.connect(s0, *U.PEER) == 0
    return s0, s1


def dgrams(kinds, payload_len=22, seed=1):
    """One frame per (source, dport); the payload's first four bytes are the frame's index."""
    n = len(kinds)
    pay = np.random.default_rng(seed).integers(0, 256, (n, payload_len), dtype=np.uint8)
    pay[:, :4] = np.arange(n).astype("<u4").view(np.uint8).reshape(n, 4)
    return U.frames_from([k[0] for k in kinds], [k[1] for k in kinds], seed, payload_len=payload_len, payload=pay)


def mixed_kinds(n, seed):
    rng = np.random.default_rng(seed)
    return [(SOURCES[int(a)], PA if c else PB) for a, c in zip(rng.integers(0, len(SOURCES), n), rng.integers(0, 2, n))]


def rows(b, idx):
    return [b.rows[i, 42:].tobytes() for i in idx]


def want_rings(kinds, peer=U.PEER):
    """(frames socket 0 receives when connected to `peer` (None: not connected), frames socket 1 receives)."""
    r0 = [i for i, k in enumerate(kinds) if k[1] == PA and (peer is None or k[0] == peer)]
    return r0, [i for i, k in enumerate(kinds) if k[1] == PB]


@pytest.mark.parametrize("extra,payload_len", [("", 22), ("devices = 0,0\n", 22), ("devices = 0,0\ndispatch = rss\n", 22),
                                               ("poll_chunk_mb = 1\npoll_chunk_min_avg = 0\n", 1400)],
                         ids=["one-context", "two-shards", "two-shards-rss", "chunked"])
def test_connected_socket_receives_only_its_peer(tmp_path, host_api, extra, payload_len):
    """Every poll form fills the rings the rule gives (so all of them the one-context poll's)."""
    init(tmp_path, extra)
    try:
        s0, s1 = two_sockets(host_api)
        kinds = mixed_kinds(2000, 5)
        b = dgrams(kinds, payload_len)
        r0, r1 = want_rings(kinds)
        n_pa = sum(k[1] == PA for k in kinds)
        assert len(r0) > 150 and n_pa - len(r0) > 500 and len(r1) > 800
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == len(r0) + len(r1) and st.counters[abi.C_DELIVERIES] == b.n
        assert host_api.rx_refused() == n_pa - len(r0)
        assert host_api.rx_dropped() == 0 and host_api.rx_balanced() == 0 and host_api.rx_nobufs() == 0
        # recv and recvfrom agree: alternate them over the connected socket's ring
        got = []
        for k in range(len(r0)):
            if k & 1:
                n, data = host_api.recv(s0, 2048)
            else:
                n, data, src = host_api.recvfrom(s0, 2048)
                assert src == U.PEER
            assert n == payload_len
            got.append(data)
        assert got == rows(b, r0)
        assert drain(host_api, s0) == []
        assert drain(host_api, s1) == rows(b, r1)               # the unconnected socket: everybody's
    finally:
        abi.lib().udpdk_cleanup()


def test_unspec_reconnect_and_close(tmp_path, host_api):
    """The table follows connect: AF_UNSPEC restores delivery from everyone at the next poll, a second
    connect replaces the peer, datagrams already queued stay, and the last close turns the stage off."""
    init(tmp_path, "")
    try:
        s0, s1 = two_sockets(host_api)
        kinds = mixed_kinds(600, 6)
        b = dgrams(kinds)
        n_pa = sum(k[1] == PA for k in kinds)
        poll_slice(b, 0, b.n)
        refused = host_api.rx_refused()
        assert refused == n_pa - len(want_rings(kinds)[0]) > 100
        # queued datagrams stay when the peer changes
        assert host_api.connect(s0, *U.STRANGERS[2]) == 0
        poll_slice(b, 0, b.n)
        r0b = want_rings(kinds, U.STRANGERS[2])[0]
        assert drain(host_api, s0) == rows(b, want_rings(kinds)[0]) + rows(b, r0b)
        assert host_api.rx_refused() == refused + n_pa - len(r0b)
        refused = host_api.rx_refused()
        assert len(drain(host_api, s1)) == 2 * len(want_rings(kinds)[1])
        assert host_api.connect(s0, 0, 0, family=socket.AF_UNSPEC) == 0
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == b.n and host_api.rx_refused() == refused
        assert drain(host_api, s0) == rows(b, want_rings(kinds, None)[0])
        drain(host_api, s1)
        # a connected socket that closes: the other socket goes on, nothing is refused
        assert host_api.connect(s0, *U.PEER) == 0
        assert host_api.close(s0) == 0
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == len(want_rings(kinds)[1]) == st.counters[abi.C_DELIVERIES]
        assert host_api.rx_refused() == refused
        assert drain(host_api, s1) == rows(b, want_rings(kinds)[1])
    finally:
        abi.lib().udpdk_cleanup()


def test_send_builds_sendtos_frames(tmp_path, host_api):
    """udpdk_send and udpdk_sendto(NULL) queue what udpdk_sendto to the peer queues: the drained
    frames are the same bytes."""
    init(tmp_path, "")
    try:
        s0, s1 = two_sockets(host_api)
        for p in (b"abc", b"", b"x" * 1400):
            assert host_api.send(s0, p) == len(p)
            assert host_api.sendto_null(s0, p) == len(p)
            assert host_api.sendto(s0, p, *U.PEER) == len(p)
        fr = host_api.tx_drain()
        assert len(fr) == 9
        for k in range(0, 9, 3):
            assert fr[k] == fr[k + 1] == fr[k + 2]
        assert fr[0][30:34] == bytes(U.B.ip_bytes(U.PEER[0])) and fr[0][36:38] == U.PEER[1].to_bytes(2, "big")
        assert host_api.send(s1, b"abc") == -1 and host_api.errno() == errno.ENOTCONN
    finally:
        abi.lib().udpdk_cleanup()


def test_reassembled_datagram_from_a_stranger_is_refused(tmp_path, host_api):
    """A reassembled datagram's frame carries the first fragment's header: the same rule."""
    init(tmp_path, "")
    try:
        s0, s1 = two_sockets(host_api)
        rng = np.random.default_rng(8)
        frames, bigs = [], []
        for ident, (ip, port) in enumerate([U.PEER, U.STRANGERS[0], U.STRANGERS[1], U.PEER]):
            big = rng.integers(0, 256, 2000 + ident, dtype=np.uint8).tobytes()
            bigs.append(big)
            d = udp_datagram(abi.raw_port(port), abi.raw_port(PA), big)
            frames += split(abi.raw_ip(ip), abi.raw_ip(IP1), ident, d, [1480, len(d) - 1480])
        d = udp_datagram(abi.raw_port(U.STRANGERS[0][1]), abi.raw_port(PB), bigs[0])
        frames += split(abi.raw_ip(U.STRANGERS[0][0]), abi.raw_ip(IP1), 9, d, [1480, len(d) - 1480])
        buf, off, ln = batch(frames)
        st = abi.RxStats()
        assert abi.lib().udpdk_poll_rx(buf.ctypes.data, len(buf) - 64, off.ctypes.data, ln.ctypes.data, None,
                                       len(off), C.byref(st)) == 0
        assert drain(host_api, s0) == [bigs[0], bigs[3]]
        assert drain(host_api, s1) == [bigs[0]]                 # unconnected: the stranger's arrives
        assert host_api.rx_refused() == 2
    finally:
        abi.lib().udpdk_cleanup()


def test_poll_echo_answers_only_the_peer(tmp_path, host_api):
    init(tmp_path, "")
    try:
        s0, s1 = two_sockets(host_api)
        kinds = mixed_kinds(500, 9)
        b = dgrams(kinds)
        r0, r1 = want_rings(kinds)
        rc, err, replies, st, n = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length)
        assert rc == 0 and n == len(replies) == st.deliveries == len(r0) + len(r1)
        # replies come in lane order, each lane's in arrival order, with the request's payload
        assert [r[42:] for r in replies] == rows(b, r0) + rows(b, r1)
        peer_ip = bytes(U.B.ip_bytes(U.PEER[0]))
        assert all(r[30:34] == peer_ip and r[36:38] == U.PEER[1].to_bytes(2, "big") for r in replies[:len(r0)])
        assert host_api.rx_refused() == sum(k[1] == PA for k in kinds) - len(r0)
        assert host_api.connect(s0, 0, 0, family=socket.AF_UNSPEC) == 0
        rc, err, replies, st, n = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length)
        assert rc == 0 and n == b.n == st.deliveries
    finally:
        abi.lib().udpdk_cleanup()


def test_strangers_burst_does_not_take_the_peers_place(tmp_path, host_api):
    """Ring admission is all-or-nothing per 128-frame burst. With room for 150 datagrams, a burst of
    128 strangers used to be admitted and the peer's 100 datagrams after it dropped; now the burst
    is gone before admission counts it."""
    init(tmp_path, "")
    try:
        s0, s1 = two_sockets(host_api)
        usable = 2047                                           # UDPDK_RX_RING_SIZE - 1
        fill = dgrams([(U.PEER, PA)] * (usable - 150), seed=2)
        assert poll_slice(fill, 0, fill.n).deliveries == fill.n
        kinds = [(U.STRANGERS[0], PA)] * 128 + [(U.PEER, PA)] * 100
        b = dgrams(kinds, seed=3)
        st = poll_slice(b, 0, b.n)
        assert st.deliveries == 100 and host_api.rx_refused() == 128
        assert drain(host_api, s0) == rows(fill, range(fill.n)) + rows(b, range(128, 228))
    finally:
        abi.lib().udpdk_cleanup()
