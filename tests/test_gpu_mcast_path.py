"""Multicast through the socket layer on the GPU: with [gpu] mcast = 1 udpdk_poll_rx delivers a
group's datagrams to the sockets that joined it (one-piece and chunked polls, reassembled datagrams)
and answers IGMP queries; udpdk_tx_drain emits the reports and leaves ahead of the socket datagrams.
With the switch off every socket bound to the port receives everything, as before.

Three sockets share port 5000, all SO_REUSEPORT, so a frame fans out to every one whose address
matches (the bind rules allow one ANY socket per port): socket 0 is bound to ANY, socket 1 to the
group address G1 itself, socket 2 to our unicast address. Socket 0 joined G1, socket 1 did not. Every
payload names its frame, so a ring's content is a list of frame indices. The expected frames are the models' (mcast_util.py, arp_util.py, icmp_util.py)."""
import ctypes as C

import numpy as np
import pytest

import arp_util as AU
import icmp_util as IU
import mcast_util as U
from reasm_util import batch, split, udp_datagram
from test_gpu_rx_balance import drain, poll_slice
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

PORT = 5000
MAC, IP = AU.OUR_MAC, AU.OUR_IP
CHUNKED = "poll_chunk_mb = 1\npoll_chunk_min_avg = 0\n"


def _mac(b):
    return ":".join(f"{x:02x}" for x in b)


def init(tmp_path, extra):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {_mac(MAC)}\nip_addr = {IP}\n[port0_dst]\nmac_addr = {_mac(AU.PEER_MAC)}\n"
                   "[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 16\n"
                   "frag_buckets = 64\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    assert abi.lib().udpdk_init(3, argv) == 0


def three_sockets(api):
    s = [api.socket() for _ in range(3)]
    assert s == [0, 1, 2]
    for k, ip in zip(s, ("0.0.0.0", U.G1, IP)):
        assert api.setsockopt(k, 1, 15, 1) == 0 and api.bind(k, ip, PORT) == 0
    return s


def dgrams(dsts, payload_len=22, seed=1):
    """One frame per destination; the payload's first four bytes are the frame's index."""
    n = len(dsts)
    pay = np.random.default_rng(seed).integers(0, 256, (n, payload_len), dtype=np.uint8)
    pay[:, :4] = np.arange(n).astype("<u4").view(np.uint8).reshape(n, 4)
    return U.frames_to(dsts, PORT, seed, payload_len=payload_len, payload=pay)


def rows(b, idx):
    return [b.rows[i, 42:].tobytes() for i in idx]


def mixed_dsts(n, seed):
    kinds = [U.G1, U.G2, IP]
    return [kinds[int(k)] for k in np.random.default_rng(seed).integers(0, 3, n)]


@pytest.mark.parametrize("extra,payload_len", [("", 22), (CHUNKED, 1400)], ids=["one-piece", "chunked"])
def test_group_goes_to_the_socket_that_joined(tmp_path, host_api, extra, payload_len):
    init(tmp_path, "mcast = 1\n" + extra)
    try:
        s0, s1, s2 = three_sockets(host_api)
        assert host_api.join(s0, U.G1) == 0
        assert host_api.tx_drain() == [U.report_frame(MAC, IP, U.G1)]        # the unsolicited report
        dsts = mixed_dsts(2000, 5)
        b = dgrams(dsts, payload_len)
        uni = [i for i, d in enumerate(dsts) if d == IP]
        g1 = [i for i, d in enumerate(dsts) if d == U.G1]
        n_g2 = len(dsts) - len(uni) - len(g1)
        assert min(len(uni), len(g1), n_g2) > 500
        st = poll_slice(b, 0, b.n)
        made = 2 * len(uni) + 2 * len(g1) + n_g2                             # ANY matches everything
        assert st.counters[abi.C_DELIVERIES] == made and st.deliveries == 2 * len(uni) + len(g1)
        assert host_api.rx_not_member() == len(g1) + n_g2                     # socket 1's G1, socket 0's G2
        assert host_api.rx_dropped() == 0 and host_api.rx_balanced() == 0 and host_api.rx_refused() == 0
        assert drain(host_api, s0) == rows(b, sorted(uni + g1))
        assert drain(host_api, s1) == []                                      # bound to the group is not joined to it
        assert drain(host_api, s2) == rows(b, uni)
        assert host_api.tx_pending() == 0 and host_api.mcast_counts()["scanned"] == 0   # pure UDP: no IGMP stage
        # a membership change reaches the next poll: socket 1 joins G1, socket 0 swaps G1 for G2
        assert host_api.join(s1, U.G1) == 0 and host_api.leave(s0, U.G1) == 0 and host_api.join(s0, U.G2) == 0
        before = host_api.rx_not_member()
        poll_slice(b, 0, 600)
        g16 = [i for i in range(600) if dsts[i] == U.G1]
        assert drain(host_api, s0) == rows(b, [i for i in range(600) if dsts[i] != U.G1])
        assert drain(host_api, s1) == rows(b, g16)
        assert host_api.rx_not_member() - before == len(g16)
        assert host_api.tx_drain() == [U.report_frame(MAC, IP, U.G2)]        # (G1 never lost its last holder)
        assert host_api.leave(s1, U.G1) == 0 and host_api.tx_drain() == [U.leave_frame(MAC, IP, U.G1)]
    finally:
        abi.lib().udpdk_cleanup()


@pytest.mark.parametrize("extra,payload_len", [("", 22), (CHUNKED, 1400)], ids=["one-piece", "chunked"])
def test_switch_off_delivers_to_every_socket_of_the_port(tmp_path, host_api, extra, payload_len):
    init(tmp_path, extra)
    try:
        s0, s1, s2 = three_sockets(host_api)
        assert host_api.config_mcast(-1) == 0
        assert host_api.join(s0, U.G1) == 0 and host_api.tx_pending() == 0   # recorded, nothing sent
        dsts = mixed_dsts(1200, 6)
        b = dgrams(dsts, payload_len)
        uni = [i for i, d in enumerate(dsts) if d == IP]
        st = poll_slice(b, 0, b.n)
        g1 = [i for i, d in enumerate(dsts) if d == U.G1]
        assert st.deliveries == st.counters[abi.C_DELIVERIES] == b.n + len(g1) + len(uni)
        assert drain(host_api, s0) == rows(b, range(b.n))                    # ANY: every group, joined or not
        assert drain(host_api, s1) == rows(b, g1) and drain(host_api, s2) == rows(b, uni)
        assert host_api.rx_not_member() == 0
        # a general query is not answered either
        q = U.pack([U.query(), U.query(group=U.G1)])
        poll_slice(q, 0, q.n)
        assert host_api.tx_pending() == 0 and not host_api.mcast_counts()["scanned"]
        # set at run time: the group already joined is announced, and the next poll filters
        assert host_api.config_mcast(1) == 0
        assert host_api.tx_drain() == [U.report_frame(MAC, IP, U.G1)]
        poll_slice(b, 0, 300)
        assert drain(host_api, s1) == []
        assert drain(host_api, s0) == rows(b, [i for i in range(300) if dsts[i] != U.G2])
        assert drain(host_api, s2) == rows(b, [i for i in range(300) if dsts[i] == IP])
    finally:
        abi.lib().udpdk_cleanup()


@pytest.mark.parametrize("extra", ["", CHUNKED], ids=["one-piece", "chunked"])
def test_queries_are_answered_and_reports_drain_first(tmp_path, host_api, extra):
    """A poll with datagrams, an ARP request, a general and a specific query and an echo request: the
    drain yields the ARP reply, one report per joined group, the echo reply, then the datagrams."""
    init(tmp_path, "mcast = 1\narp = 1\nicmp = echo\n" + extra)
    try:
        s0, s1, s2 = three_sockets(host_api)
        assert host_api.join(s0, U.G1) == 0 and host_api.join(s1, U.G2) == 0 and host_api.join(s1, U.G1) == 0
        assert host_api.join(s2, "224.0.0.1") == 0
        assert host_api.tx_drain() == [U.report_frame(MAC, IP, U.G1), U.report_frame(MAC, IP, U.G2)]
        rng = np.random.default_rng(11)
        d = dgrams([U.G1, U.G2, IP, "239.9.9.9"] * 60, 1400 if extra else 22)
        fl = [bytes(r) for r in d.rows]
        arp, echo = AU.arp_frame(), IU.echo_request(rng, 64)
        ctl = {31: arp, 77: U.query(), 78: U.query(group=U.G2), 120: echo, 150: U.query(group="239.9.9.9"),
               151: U.query(group=U.G1, typ=0x16), 200: U.query(igmp_cksum=False)}
        for at, f in ctl.items():
            fl[at] = f
        bt = U.pack(fl, gaps=rng.integers(0, 4, len(fl)))
        poll_slice(bt, 0, bt.n)
        arp_reply = AU.model(*AU.pack([arp])[:4], np.array([abi.V_NOT_IPV4], np.uint32))["frames_out"]
        e = AU.pack([echo])
        echo_reply = IU.model(e[0], e[1], e[2], e[3], np.array([abi.V_NOT_UDP | 0x10], np.uint32), flags=IU.ECHO,
                              mtu=1500).frames_out
        assert len(arp_reply) == 1 and len(echo_reply) == 1
        assert host_api.tx_pending() == 4
        assert host_api.sendto(s0, b"after the answers", "10.1.2.3", 4000) == 17
        got = host_api.tx_drain()
        assert got[:4] == arp_reply + [U.report_frame(MAC, IP, U.G1), U.report_frame(MAC, IP, U.G2)] + echo_reply
        assert len(got) == 5 and got[4][23] == 17 and got[4][42:] == b"after the answers"
        c = host_api.mcast_counts()
        want = dict(igmp=5, general=1, specific=1, not_member=1, other_type=1, bad_cksum=1, malformed=0, bad_dst=0,
                    reports=2, joins=4, leaves=0, reports_sent=4, leaves_sent=0)
        assert {k: c[k] for k in want} == want and c["scanned"] >= 1
        # the rings beside it: the control frames reach nobody, 239.9.9.9 nobody
        idx = [i for i in range(len(fl)) if i not in ctl]
        assert drain(host_api, s0) == [fl[i][42:] for i in idx if i % 4 in (0, 2)]
        assert drain(host_api, s1) == [fl[i][42:] for i in idx if i % 4 == 0]   # (bound to G1: only G1 reaches it)
        assert drain(host_api, s2) == [fl[i][42:] for i in idx if i % 4 == 2]
        # leaves: the last holder's drop, udpdk_close included; all-hosts never
        assert host_api.leave(s1, U.G1) == 0 and host_api.tx_pending() == 0
        assert host_api.close(s1) == 0 and host_api.close(s2) == 0
        assert host_api.tx_drain() == [U.leave_frame(MAC, IP, U.G2)]
        assert host_api.close(s0) == 0 and host_api.tx_drain() == [U.leave_frame(MAC, IP, U.G1)]
        poll_slice(bt, 70, 90)                                               # no group left: the stage does not run
        assert host_api.mcast_counts()["scanned"] == c["scanned"] and host_api.tx_pending() == 0
    finally:
        abi.lib().udpdk_cleanup()


def test_fragmented_datagram_reaches_only_the_joined_socket(tmp_path, host_api):
    init(tmp_path, "mcast = 1\n")
    try:
        s0, s1, s2 = three_sockets(host_api)
        assert host_api.join(s0, U.G1) == 0
        rng = np.random.default_rng(8)
        frames, bigs = [], []
        for ident, dst in enumerate([U.G1, U.G2, IP]):
            big = rng.integers(0, 256, 2000 + ident, dtype=np.uint8).tobytes()
            bigs.append(big)
            d = udp_datagram(abi.raw_port(7000), abi.raw_port(PORT), big)
            frames += split(abi.raw_ip("10.1.2.3"), abi.raw_ip(dst), ident, d, [1480, len(d) - 1480])
        buf, off, ln = batch(frames)
        st = abi.RxStats()
        assert abi.lib().udpdk_poll_rx(buf.ctypes.data, len(buf) - 64, off.ctypes.data, ln.ctypes.data, None,
                                       len(off), C.byref(st)) == 0
        assert drain(host_api, s0) == [bigs[0], bigs[2]]
        assert drain(host_api, s1) == [] and drain(host_api, s2) == [bigs[2]]
        assert host_api.rx_not_member() == 2                                 # socket 1's G1, socket 0's G2
    finally:
        abi.lib().udpdk_cleanup()
