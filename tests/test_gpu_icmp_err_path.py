"""Received ICMP errors through the socket layer: with [gpu] icmp_errors = 1 udpdk_poll_rx runs
udpdk_gpu_icmp_errors after a batch's RX and a connected socket whose datagram came back as a
destination-unreachable gets the error from its next call (ECONNREFUSED for a closed port). The
stack answers its own datagrams here ([gpu] icmp = unreach): the polls are driven by hand,
udpdk_tx_drain -> udpdk_poll_rx, and its own address is 172.31.100.1."""
import ctypes as C
import errno
import socket
import threading

import numpy as np
import pytest

import icmp_err_util as E
import icmp_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

ON = "icmp = unreach\nicmp_errors = 1\n"
CLOSED = (U.OUR_IP, U.CLOSED_PORT)


def _mac(b):
    return ":".join(f"{x:02x}" for x in b)


def _init(tmp_path, extra=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {_mac(U.SRC_MAC)}\nip_addr = {U.OUR_IP}\n[port0_dst]\n"
                   f"mac_addr = {_mac(U.DST_MAC)}\n[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n"
                   "frag_buckets = 64\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


@pytest.fixture()
def api(tmp_path, host_api, request):
    assert _init(tmp_path, getattr(request, "param", ON)) == 0
    yield host_api
    abi.lib().udpdk_cleanup()


def _poll(frame_list):
    buf, nb, off, ln = U.pack(frame_list)
    flat = np.concatenate([buf, np.zeros(256, np.uint8)])
    st = abi.RxStats()
    assert abi.lib().udpdk_poll_rx(flat.ctypes.data, nb, off.ctypes.data, ln.ctypes.data, None, len(off), C.byref(st)) == 0
    return st


def _turn(api):
    """What is queued leaves and comes back in: one drain, one poll. Returns the frames."""
    frames = api.tx_drain()
    if frames:
        _poll(frames)
    return frames


def _client(api, port, peer=CLOSED):
    s = api.socket()
    assert api.bind(s, "0.0.0.0", port) == 0
    if peer:
        assert api.connect(s, *peer) == 0
    return s


def _so_error(api, s):
    rc, v = api.getsockopt(s, abi.SOL_SOCKET, socket.SO_ERROR)
    assert rc == 0
    return v


def _counts(api):
    c = api.icmp_err_counts()
    return {k: int(getattr(c, k)) for k, _ in c._fields_}


def test_refused_peer_and_unconnected_socket(api):
    assert api.config_icmp_errors(-1) == 1
    a, u = _client(api, 10050), _client(api, 10051, peer=None)
    assert api.send(a, b"anybody there?") == 14 and api.sendto(u, b"or there?", *CLOSED) == 9
    sent = _turn(api)                                                # the datagrams: nobody is bound there
    assert len(sent) == 2 and all(f[23] == 17 for f in sent)
    assert _so_error(api, a) == 0 and _counts(api)["errors"] == 0
    back = _turn(api)                                                # the stack's own port-unreachable errors
    assert len(back) == 2 and all(f[23] == 1 and f[34] == 3 and f[35] == 3 for f in back)
    assert _counts(api) == dict(errors=2, msg_bad=0, quote_bad=0, soft=0, no_socket=1, reported=1, posted=1)
    n, _ = api.recv(a)
    assert n == -1 and api.errno() == errno.ECONNREFUSED             # once
    assert _so_error(api, a) == 0 and _so_error(api, u) == 0         # the unconnected socket got nothing
    assert api.send(a, b"again") == 5                                # and the next call works
    assert _turn(api) and _turn(api)
    assert _so_error(api, a) == errno.ECONNREFUSED and _so_error(api, a) == 0
    assert api.tx_pending() == 0 and _turn(api) == []                # nothing answers an error


def test_error_is_reported_before_data_queued_in_the_same_poll(api):
    peer = ("10.0.0.9", 5003)
    a = _client(api, 10050, peer)
    rng = np.random.default_rng(1)
    me = E.Sock(a, None, 10050, 0, peer)
    data = E.sent_frame(rng, E.Sock(0, *peer), 11, to=(U.OUR_IP, 10050))
    err = E.unreach_frame(E.sent_frame(rng, me, 30), 3, src_ip=peer[0])
    other = E.unreach_frame(E.sent_frame(rng, me, 30, to=("10.0.0.9", 5004)), 3)       # not the peer's port
    soft = E.unreach_frame(E.sent_frame(rng, me, 30), 1)
    st = _poll([data, err, other, soft])
    assert st.counters[abi.V_DELIVERED] == 1 and st.counters[abi.V_NOT_UDP] == 3
    assert _counts(api) == dict(errors=3, msg_bad=0, quote_bad=0, soft=1, no_socket=1, reported=1, posted=1)
    n, _ = api.recv(a)
    assert n == -1 and api.errno() == errno.ECONNREFUSED
    assert api.recvfrom(a) == (11, data[42:], peer)                  # queued before the error, received after it
    assert _so_error(api, a) == 0
    # the last hard error of a poll wins; a reconnect between polls drops what was pending
    _poll([E.unreach_frame(E.sent_frame(rng, me, 5), 3), E.unreach_frame(E.sent_frame(rng, me, 5), 10), soft])
    assert _so_error(api, a) == errno.EHOSTUNREACH
    _poll([err])
    assert api.connect(a, "10.0.0.9", 5004) == 0 and _so_error(api, a) == 0
    _poll([err])                                                     # about the old peer: nobody's
    assert _so_error(api, a) == 0 and _counts(api)["no_socket"] == 2
    _poll([other])
    assert _so_error(api, a) == errno.ECONNREFUSED


@pytest.mark.parametrize("api", ["icmp = unreach\n"], indirect=True)
def test_switch_off_changes_nothing(api):
    assert api.config_icmp_errors(-1) == 0
    a = _client(api, 10050)
    assert api.send(a, b"anybody there?") == 14
    assert len(_turn(api)) == 1 and len(_turn(api)) == 1 and _turn(api) == []
    assert _so_error(api, a) == 0 and _counts(api) == dict.fromkeys(_counts(api), 0)
    assert api.icmp_counts().unreach_sent == 1
    # on at run time: the same sequence reports
    assert api.config_icmp_errors(1) == 0
    assert api.send(a, b"anybody there?") == 14
    assert len(_turn(api)) == 1 and len(_turn(api)) == 1
    assert _so_error(api, a) == errno.ECONNREFUSED and _counts(api)["posted"] == 1


@pytest.mark.parametrize("api", [ON + "poll_chunk_mb = 1\npoll_chunk_min_avg = 0\n"], indirect=True)
def test_chunked_poll_reports_the_same(api):
    """3000 x 1400 B of TCP (NOT_UDP: candidates by meta that are nobody's errors) in chunks of about
    1000 frames, with errors for three sockets in the first, second and third chunk; socket 0 has a
    second, later one in the third."""
    rng = np.random.default_rng(2)
    peers = [("10.0.0.9", 5003), ("10.0.1.9", 5004), ("10.0.2.9", 5005)]
    socks = [E.Sock(_client(api, 10050 + k, peers[k]), None, 10050 + k, 0, peers[k]) for k in range(3)]
    tcp = U.ip_frame(6, rng.integers(0, 256, 1380, dtype=np.uint8).tobytes())
    fl = [tcp] * 3000
    for p, k, code in ((10, 0, 3), (1500, 1, 10), (2800, 2, 2), (2900, 0, 7), (2950, 0, 0)):
        fl[p] = E.unreach_frame(E.sent_frame(rng, socks[k], 1000), code, quote_len=548)
    assert sum(len(f) for f in fl) > 3 << 20
    st = _poll(fl)
    assert st.counters[abi.V_NOT_UDP] == 3000
    assert _counts(api) == dict(errors=5, msg_bad=0, quote_bad=0, soft=1, no_socket=0, reported=4, posted=4)
    assert [_so_error(api, s.fd) for s in socks] == [errno.EHOSTDOWN, errno.EHOSTUNREACH, errno.ENOPROTOOPT]


def test_sharded_context_refuses(tmp_path, host_api):
    L = abi.lib()
    assert _init(tmp_path, "devices = 0,0\nicmp_errors = 1\n") == -1 and host_api.errno() == errno.ENOTSUP
    assert L.udpdk_gpu_context() is None
    host_api.reset()
    assert _init(tmp_path, "devices = 0,0\n") == 0
    try:
        assert host_api.config_icmp_errors(1) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_icmp_errors(0) == 0 and host_api.config_icmp_errors(-1) == 0
    finally:
        L.udpdk_cleanup()


def test_poller_thread_over_loopback(api):
    """The loopback port with the poller thread: a client of a dead service blocks in udpdk_recv and
    gets ECONNREFUSED, with no poll driven from here."""
    L = abi.lib()
    ops = abi.PortOps()
    assert L.udpdk_port_loopback(C.byref(ops)) == 0
    ops.batch_frames = 512
    a = _client(api, 10000)
    assert L.udpdk_port_attach(C.byref(ops)) == 0
    watchdog = threading.Timer(60.0, L.udpdk_interrupt, [0])        # a hang ends as EINTR
    watchdog.start()
    try:
        assert api.send(a, b"nobody home") == 11
        n, _ = api.recv(a)
        assert n == -1 and api.errno() == errno.ECONNREFUSED
        assert _so_error(api, a) == 0
        c = _counts(api)
        assert c["reported"] == c["posted"] == 1 and api.icmp_counts().unreach_sent == 1
    finally:
        watchdog.cancel()
        assert L.udpdk_port_detach() == 0
