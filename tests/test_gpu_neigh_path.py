"""The neighbour cache through the socket layer, with manual udpdk_poll_rx and udpdk_tx_drain: a drain resolves
every datagram's MAC on the GPU and queues who-has requests for what it does not know, a poll learns from the
ARP it is fed. Socket 0 is bound ANY:10001; the stack is 172.31.100.1 / 68:05:ca:95:f8:ec and [port0_dst] is
68:05:ca:95:fa:64. Expected data frames are the oracle's with the next hop's MAC in bytes 0-5."""
import ctypes as C
import errno

import numpy as np
import pytest

import arp_util as A
import neigh_util as U
import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

P1, M1 = "172.31.100.21", bytes.fromhex("02aa00000021")
P2, M2 = "172.31.100.22", bytes.fromhex("02aa00000022")
GW, MG = "172.31.100.254", bytes.fromhex("02aa000000fe")


def _mac(b):
    return ":".join(f"{x:02x}" for x in b)


def _init(tmp_path, extra="", port0=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {_mac(A.OUR_MAC)}\nip_addr = {A.OUR_IP}\n{port0}[port0_dst]\n"
                   f"mac_addr = {_mac(A.PEER_MAC)}\n[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


@pytest.fixture()
def api(tmp_path, host_api, request):
    extra, port0 = getattr(request, "param", ("", ""))
    assert _init(tmp_path, extra, port0) == 0
    s0 = host_api.socket()
    assert host_api.bind(s0, "0.0.0.0", 10001) == 0
    yield host_api
    abi.lib().udpdk_cleanup()


def _poll(frame_list):
    buf, nb, off, ln = A.pack(frame_list, aligns=[(7 * k + 3) % 16 for k in range(len(frame_list))])
    flat = np.concatenate([buf, np.zeros(256, np.uint8)])
    st = abi.RxStats()
    return abi.lib().udpdk_poll_rx(flat.ctypes.data, nb, off.ctypes.data, ln.ctypes.data, None, len(off), C.byref(st))


def _frame(mac, ip, port, payload):
    return O.tx_frame(A.OUR_MAC, mac, abi.raw_ip(A.OUR_IP), 1, 0, abi.raw_port(10001), abi.raw_ip(ip), abi.raw_port(port),
                      payload)


def _who_has(ip):
    return A.arp_frame(sha=A.OUR_MAC, spa=A.OUR_IP, tpa=ip)


def _reply(mac, ip):
    return A.arp_frame(op=2, sha=mac, spa=ip, tha=A.OUR_MAC, tpa=A.OUR_IP, eth_dst=A.OUR_MAC, pad_to=60)


def _nonzero(api):
    return {k: v for k, v in api.neigh_counts().items() if v}


STRICT = ("neigh = 1\n", "")


@pytest.mark.parametrize("api", [STRICT], indirect=True)
def test_strict_mode_asks_then_learns(api):
    assert api.config_neigh(-1) == 1
    assert api.sendto(0, b"too early", P1, 4000) == 9
    assert api.tx_drain() == []                                     # no data frame: its span is a gap
    assert _nonzero(api) == dict(inserted=1, unresolved=1, tx_unresolved=1, requests=1)
    assert api.tx_pending() == 1 and api.tx_dropped() == 0
    assert api.tx_drain() == [_who_has(P1)]                         # the who-has leaves first in the next drain
    # asked again at once: no second request while retrans_ms runs
    assert api.sendto(0, b"still early", P1, 4000) == 11
    assert api.tx_drain() == [] and api.tx_pending() == 0
    assert _nonzero(api) == dict(inserted=1, incomplete=1, unresolved=2, tx_unresolved=2, requests=1)
    # the reply comes in among other traffic
    rng = np.random.default_rng(1)
    assert _poll([A.udp_frame(rng, payload_len=10), _reply(M1, P1), A.udp_frame(rng, payload_len=30)]) == 0
    assert _nonzero(api)["updated"] == 1 and _nonzero(api)["arp"] == 1
    assert api.sendto(0, b"now it goes", P1, 4000) == 11
    assert api.tx_drain() == [_frame(M1, P1, 4000, b"now it goes")]
    assert _nonzero(api)["hit"] == 1 and api.tx_pending() == 0


@pytest.mark.parametrize("api", [STRICT], indirect=True)
def test_two_peers_two_macs_in_one_drain(api):
    assert _poll([_reply(M1, P1)]) == 0                             # never asked for: ignored
    assert _nonzero(api) == dict(arp=1, ignored=1)
    for ip in (P1, P2):
        assert api.sendto(0, b"x", ip, 9) == 1
    assert api.tx_drain() == [] and api.tx_drain() == [_who_has(P1), _who_has(P2)]
    assert _poll([_reply(M2, P2), _reply(M1, P1)]) == 0
    big = bytes(range(256)) * 8                                     # two fragments at the MTU: both carry the MAC
    sends = [(P1, b"one"), (P2, b"two"), (P1, big), (P2, b"four"), ("255.255.255.255", b"all"), ("224.0.0.251", b"mdns")]
    for ip, p in sends:
        assert api.sendto(0, p, ip, 5353) == len(p)
    want = []
    macs = {P1: M1, P2: M2, "255.255.255.255": b"\xff" * 6, "224.0.0.251": bytes.fromhex("01005e0000fb")}
    for ip, p in sends:
        f = _frame(macs[ip], ip, 5353, p)
        want += O.tx_fragment(f, 1500) if len(f) > 1500 else [f]
    got = api.tx_drain()
    assert got == want and len(got) == 7 and got[3][:6] == M1 and got[2][:6] == M1
    c = _nonzero(api)
    assert c["hit"] == 4 and c["bcast"] == 1 and c["mcast"] == 1 and c["requests"] == 2


@pytest.mark.parametrize("api", [("neigh = 1\n", f"netmask = 255.255.255.0\ngateway = {GW}\n")], indirect=True)
def test_off_link_goes_to_the_gateway(api):
    assert api.neigh_add(GW, MG) == 0
    sends = [("8.8.8.8", b"far"), (GW, b"near"), ("172.31.101.1", b"next door"), ("172.31.100.255", b"subnet")]
    for ip, p in sends:
        assert api.sendto(0, p, ip, 53) == len(p)
    macs = [MG, MG, MG, b"\xff" * 6]
    assert api.tx_drain() == [_frame(m, ip, 53, p) for m, (ip, p) in zip(macs, sends)]
    assert _nonzero(api) == dict(hit=3, bcast=1) and api.tx_pending() == 0


@pytest.mark.parametrize("api", [("neigh = 1\n", "netmask = 255.255.255.0\n")], indirect=True)
def test_no_route_is_dropped(api):
    assert api.sendto(0, b"nowhere", "8.8.8.8", 53) == 7
    assert api.tx_drain() == [] and api.tx_pending() == 0
    assert _nonzero(api) == dict(no_route=1, tx_unresolved=1)


@pytest.mark.parametrize("api", [("neigh = fallback\n", "")], indirect=True)
def test_fallback_mode_sends_to_the_configured_mac_and_asks(api):
    assert api.config_neigh(-1) == 2
    assert api.sendto(0, b"first", P1, 4000) == 5
    assert api.tx_drain() == [_frame(A.PEER_MAC, P1, 4000, b"first")]
    assert _nonzero(api) == dict(inserted=1, fallback=1, requests=1) and api.tx_pending() == 1
    assert api.tx_drain() == [_who_has(P1)]
    assert _poll([_reply(M1, P1)]) == 0
    assert api.sendto(0, b"second", P1, 4000) == 6
    assert api.tx_drain() == [_frame(M1, P1, 4000, b"second")]


@pytest.mark.parametrize("api", [("neigh = 1\narp = 1\n", "")], indirect=True)
def test_a_request_to_us_is_answered_and_its_sender_learned(api):
    ask = A.arp_frame(sha=M2, spa=P2, tpa=A.OUR_IP, pad_to=60)
    assert _poll([ask]) == 0
    assert _nonzero(api) == dict(arp=1, created=1)
    R = A.model(*A.pack([ask]), np.array([A.V_NOT_IPV4], np.uint32))
    assert api.tx_drain() == R["frames_out"] and len(R["frames_out"]) == 1      # the reply (rx_arp.c)
    assert api.sendto(0, b"hello back", P2, 7) == 10
    assert api.tx_drain() == [_frame(M2, P2, 7, b"hello back")]                 # no request: the asker is a neighbour
    assert _nonzero(api) == dict(arp=1, created=1, hit=1)


@pytest.mark.parametrize("api", [STRICT], indirect=True)
def test_static_entries_and_flush(api):
    assert api.neigh_add(P1, M1) == 0 and api.neigh_add(0, M1) == -1 and api.errno() == errno.EINVAL
    assert _poll([_reply(M2, P1)]) == 0                             # a static entry is not learned over
    assert _nonzero(api) == dict(arp=1, static_kept=1)
    assert api.sendto(0, b"static", P1, 1) == 6
    assert api.tx_drain() == [_frame(M1, P1, 1, b"static")]
    assert api.neigh_flush() == 0
    assert api.sendto(0, b"flushed", P1, 1) == 7
    assert api.tx_drain() == [] and api.tx_drain() == [_who_has(P1)]
    assert api.neigh_add(P1, M2) == 0                               # over the incomplete entry
    assert api.sendto(0, b"again", P1, 1) == 5
    assert api.tx_drain() == [_frame(M2, P1, 1, b"again")]


@pytest.mark.parametrize("api", [("", f"netmask = 255.255.255.0\ngateway = {GW}\n")], indirect=True)
def test_switch_off_is_todays_drain(api):
    assert api.config_neigh(-1) == 0
    sends = [(P1, b"one"), ("8.8.8.8", b"two"), ("255.255.255.255", b"three")]
    for ip, p in sends:
        assert api.sendto(0, p, ip, 4000) == len(p)
    assert _poll([_reply(M1, P1), A.arp_frame(sha=M2, spa=P2, tpa=A.OUR_IP)]) == 0
    assert api.tx_drain() == [_frame(A.PEER_MAC, ip, 4000, p) for ip, p in sends]
    assert _nonzero(api) == {} and api.tx_pending() == 0
    # set at run time, and off again
    assert api.config_neigh(2) == 0 and api.config_neigh(3) == -1 and api.errno() == errno.EINVAL
    assert api.sendto(0, b"four", P1, 4000) == 4
    assert api.tx_drain() == [_frame(A.PEER_MAC, P1, 4000, b"four")] and api.tx_drain() == [_who_has(P1)]
    assert api.config_neigh(0) == 2
    assert api.sendto(0, b"five", P1, 4000) == 4
    assert api.tx_drain() == [_frame(A.PEER_MAC, P1, 4000, b"five")] and api.tx_pending() == 0


def test_sharded_context_refuses(tmp_path, host_api):
    L = abi.lib()
    assert _init(tmp_path, "devices = 0,0\nneigh = 1\n") == -1 and host_api.errno() == errno.EINVAL
    assert L.udpdk_gpu_context() is None
    assert _init(tmp_path, "devices = 0,0\n") == 0
    try:
        assert host_api.config_neigh(1) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_neigh(0) == 0 and host_api.config_neigh(-1) == 0
    finally:
        L.udpdk_cleanup()
