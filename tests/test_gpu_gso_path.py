"""UDP_SEGMENT through the socket layer, with manual udpdk_tx_drain: a send with a segment size is one
ring entry that the drain cuts on the GPU (udpdk_gpu_tx_segment_plan in front of the build), and what
comes out is what the sendtos of its pieces would have produced. The stack is 172.31.100.1 /
68:05:ca:95:f8:ec and [port0_dst] is 68:05:ca:95:fa:64; socket 0 is bound ANY:10001."""
import ctypes as C
import threading

import numpy as np
import pytest

import arp_util as A
import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

UDP, SEG = abi.SOL_UDP, abi.UDP_SEGMENT
P1, M1 = "172.31.100.21", bytes.fromhex("02aa00000021")
P2 = "172.31.100.22"
G = 1200
BIG = bytes((7 * i + (i >> 8)) & 0xFF for i in range(10 * G + 100))        # 10 full segments and 100 bytes
LENS = [G] * 10 + [100]


def _mac(b):
    return ":".join(f"{x:02x}" for x in b)


def _init(tmp_path, extra=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {_mac(A.OUR_MAC)}\nip_addr = {A.OUR_IP}\n[port0_dst]\n"
                   f"mac_addr = {_mac(A.PEER_MAC)}\n[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


@pytest.fixture()
def api(tmp_path, host_api, request):
    assert _init(tmp_path, getattr(request, "param", "")) == 0
    _sockets(host_api)
    yield host_api
    abi.lib().udpdk_cleanup()


def _sockets(api):
    s0, s1 = api.socket(), api.socket()
    assert (s0, s1) == (0, 1)
    assert api.bind(s0, "0.0.0.0", 10001) == 0 and api.bind(s1, "172.31.100.7", 10002) == 0


def _pieces(data, g):
    return [data[i:i + g] for i in range(0, len(data), g)]


def _frame(payload, ip=P1, port=4000, mac=A.PEER_MAC):
    return O.tx_frame(A.OUR_MAC, mac, abi.raw_ip(A.OUR_IP), 1, 0, abi.raw_port(10001), abi.raw_ip(ip), abi.raw_port(port),
                      payload)


def _frames(out, off, ln):
    return [bytes(out[o:o + n]) for o, n in zip(off, ln)]


def _queue(api, how, mixed):
    """One segmented send, its size from the socket option or from the control message; mixed: among
    ordinary datagrams of two sockets. Returns the frames it makes."""
    if mixed:                                            # ordinary datagrams around it, one of them in fragments
        assert api.sendto(1, b"from the second socket", P2, 5000) == 22
        assert api.sendto(0, b"before", P1, 4000) == 6
    if how == "sockopt":
        assert api.setsockopt(0, UDP, SEG, G) == 0
        assert api.sendto(0, BIG, P1, 4000) == len(BIG)
        assert api.setsockopt(0, UDP, SEG, 0) == 0
    else:
        assert api.sendmsg(0, [BIG[:5000], b"", BIG[5000:]], P1, 4000, gso=G) == len(BIG)
    if mixed:
        assert api.sendto(0, bytes(3000), P1, 4001) == 3000
        assert api.sendto(1, b"and again", P2, 5000) == 9
        assert api.sendmsg(0, [b"x" * 30], P2, 4002, gso=10) == 30          # a second, small segmented send
    return len(_pieces(BIG, G)) + (1 + 1 + 3 + 1 + 3 if mixed else 0)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("cksum", [0, 1])
@pytest.mark.parametrize("how", ["sockopt", "cmsg"])
def test_drains_like_its_pieces(api, how, cksum, mixed):
    assert api.config_tx_cksum(cksum) in (0, 1)
    n = _queue(api, how, mixed)
    assert api.tx_pending() == (6 if mixed else 1)                           # a queued send counts as one
    got = api.tx_drain_raw()
    assert api.tx_pending() == 0 and len(got[1]) == n
    c = api.gso_counts()
    assert c == dict(sends=2 if mixed else 1, segments=14 if mixed else 11, plans=1, refused=0)
    # the pieces, queued one by one after a reset, drained by the code that always drained them
    api.reset()
    _sockets(api)
    assert api.config_tx_cksum(cksum) == 0
    if mixed:
        assert api.sendto(1, b"from the second socket", P2, 5000) == 22 and api.sendto(0, b"before", P1, 4000) == 6
    for p in _pieces(BIG, G):
        assert api.sendto(0, p, P1, 4000) == len(p)
    if mixed:
        assert api.sendto(0, bytes(3000), P1, 4001) == 3000 and api.sendto(1, b"and again", P2, 5000) == 9
        for p in _pieces(b"x" * 30, 10):
            assert api.sendto(0, p, P2, 4002) == 10
    assert api.tx_pending() == (18 if mixed else 11)
    want = api.tx_drain_raw()
    assert api.gso_counts() == dict(sends=0, segments=0, plans=0, refused=0)
    for name, g_, w_ in zip(("out", "out_off", "out_len"), got, want):
        assert np.array_equal(g_, w_), name
    if not mixed and not cksum:                                              # ... and they are the oracle's frames
        assert _frames(*got) == [_frame(p) for p in _pieces(BIG, G)]


def test_a_send_is_never_split(api):
    """max or out_cap smaller than what is left: the send waits whole; smaller than the send itself at
    the head of its ring: it is dropped, once."""
    span = sum(n + 42 for n in LENS)
    for limit in ("max", "out_cap"):
        assert api.sendto(0, b"first", P1, 4000) == 5
        assert api.sendmsg(0, [BIG], P1, 4000, gso=G) == len(BIG)
        assert api.sendto(0, b"last", P1, 4000) == 4
        kw = dict(max_frames=11) if limit == "max" else dict(cap=47 + span - 1)
        out, off, ln = api.tx_drain_raw(**kw)                                # room for `first` and 10 / all but a byte
        assert _frames(out, off, ln) == [_frame(b"first")] and api.tx_pending() == 2 and api.tx_dropped() == 0
        out, off, ln = api.tx_drain_raw(**(dict(max_frames=11) if limit == "max" else dict(cap=span)))
        assert [int(x) for x in ln] == [n + 42 for n in LENS] and api.tx_pending() == 1      # now it fits exactly
        assert api.tx_drain() == [_frame(b"last")]
    dropped = 0
    for kw in (dict(max_frames=10), dict(cap=span - 1)):
        assert api.sendmsg(0, [BIG], P1, 4000, gso=G) == len(BIG)
        assert api.sendto(0, b"behind it", P1, 4000) == 9
        assert api.tx_drain(**kw) == [_frame(b"behind it")]                  # can never fit: one drop, not 11
        dropped += 1
        assert api.tx_dropped() == dropped and api.tx_pending() == 0


def test_no_plan_without_a_segmented_send(api):
    assert api.sendto(0, b"plain", P1, 4000) == 5
    assert api.setsockopt(0, UDP, SEG, G) == 0
    assert api.sendto(0, b"q" * G, P1, 4000) == G                            # len <= g: an ordinary entry
    assert api.sendmsg(1, [b"r" * 5000], P2, 5000, gso=0) == 5000
    assert len(api.tx_drain()) == 6 and api.gso_counts() == dict(sends=0, segments=0, plans=0, refused=0)
    assert api.sendto(0, b"q" * (G + 1), P1, 4000) == G + 1
    assert [len(f) for f in api.tx_drain()] == [G + 42, 43]
    assert api.gso_counts() == dict(sends=1, segments=2, plans=1, refused=0)
    assert api.tx_drain() == [] and api.gso_counts()["plans"] == 1           # an empty drain launches nothing


@pytest.mark.parametrize("api", ["neigh = fallback\n"], indirect=True)
def test_neigh_fallback_resolves_every_segment(api):
    assert api.neigh_add(P1, M1) == 0
    assert api.sendmsg(0, [BIG], P1, 4000, gso=G) == len(BIG)
    assert api.sendmsg(0, [b"z" * 25], P2, 4000, gso=10) == 25               # unknown: the configured MAC, and one request
    got = api.tx_drain()
    assert got == [_frame(p, mac=M1) for p in _pieces(BIG, G)] + [_frame(p, ip=P2) for p in (b"z" * 10, b"z" * 10, b"z" * 5)]
    c = api.neigh_counts()
    assert c["hit"] == 11 and c["tx_unresolved"] == 0 and c["requests"] == 1
    assert api.tx_pending() == 1                                             # the who-has for the next drain


@pytest.mark.parametrize("api", ["neigh = 1\n"], indirect=True)
def test_neigh_strict_counts_every_segment(api):
    assert api.neigh_add(P1, M1) == 0
    assert api.sendto(0, b"known", P1, 4000) == 5
    assert api.sendmsg(0, [BIG], P2, 4000, gso=G) == len(BIG)                # unknown peer: nothing is built for it
    assert api.sendto(0, b"known too", P1, 4000) == 9
    assert api.tx_drain() == [_frame(b"known", mac=M1), _frame(b"known too", mac=M1)]
    c = api.neigh_counts()
    assert c["tx_unresolved"] == 11 and c["unresolved"] == 11 and c["hit"] == 2 and c["requests"] == 1
    assert api.gso_counts()["plans"] == 1


def test_over_loopback(api):
    """The loopback port with the poller thread: one segmented send arrives as its 11 datagrams, in
    order and with their lengths."""
    L = abi.lib()
    ops = abi.PortOps()
    assert L.udpdk_port_loopback(C.byref(ops)) == 0
    ops.batch_frames = 512
    assert L.udpdk_port_attach(C.byref(ops)) == 0
    watchdog = threading.Timer(60.0, L.udpdk_interrupt, [0])                 # a hang ends as EINTR
    watchdog.start()
    try:
        assert api.sendmsg(1, [BIG], A.OUR_IP, 10001, gso=G) == len(BIG)
        for p in _pieces(BIG, G):
            n, data, addr = api.recvfrom(0, 2048)
            assert n == len(p) and data == p and addr == ("172.31.100.7", 10002)
        assert api.gso_counts() == dict(sends=1, segments=11, plans=1, refused=0)
    finally:
        watchdog.cancel()
        assert L.udpdk_port_detach() == 0
