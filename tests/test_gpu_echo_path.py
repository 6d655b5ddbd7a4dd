"""udpdk_poll_echo through the socket layer: its frames, in order, are those of an application that
echoes on a fresh session (udpdk_poll_rx -> recvfrom -> sendto back to the source -> udpdk_tx_drain),
and those of the oracle (tests/tx_reply_util.py over oracle.rx's lanes).

Two sockets: 0 bound ANY:10001, 1 bound 172.31.100.1:10002. The batch is small and mixed: unbound
ports, port 10002 on another address, one corrupt UDP checksum, one fragment, Ethernet padding,
empty and full-size payloads; fewer than 128 deliveries in all, so udpdk_tx_drain's burst order is
lane order."""
import ctypes as C
import errno

import numpy as np
import pytest

import oracle as O
import tx_reply_util as R
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

SRC_MAC, DST_MAC, SRC_IP = "68:05:ca:95:f8:ec", "68:05:ca:95:fa:64", "172.31.100.2"
IP1, IP9 = "172.31.100.1", "172.31.100.9"


def _batch():
    rng = np.random.default_rng(91)
    fr = []
    for k in range(70):
        pl = [0, 1, 17, 18, 100, 1472, 700, 33][k % 8]
        src = f"10.7.{k}.{1 + k % 5}"
        if k % 10 == 3:
            fr.append(F.make_frame(rng, dport=7, payload_len=pl, src_ip=src))                  # NO_BIND
        elif k % 10 == 6:
            fr.append(F.make_frame(rng, dport=10002, dst_ip=IP9, payload_len=pl, src_ip=src))  # NO_MATCH
        elif k % 3 == 0:
            fr.append(F.make_frame(rng, dport=10002, dst_ip=IP1, payload_len=pl, src_ip=src))
        elif k % 7 == 2:
            fr.append(F.make_frame(rng, dport=10001, payload_len=pl % 18, pad=18 - pl % 18, src_ip=src))
        else:
            fr.append(F.make_frame(rng, dport=10001, dst_ip=[IP1, IP9][k & 1], payload_len=pl, src_ip=src))
    fr[20] = F.make_frame(rng, dport=10001, payload_len=64, udp_cksum="bad", src_ip="10.8.8.8")
    fr[41] = F.make_frame(rng, dport=10001, payload_len=64, frag=0x2000, src_ip="10.9.9.9")    # FRAG
    buf, offs = bytearray(), []
    for k, f in enumerate(fr):
        buf += bytes(k % 4)
        offs.append(len(buf))
        buf += f
    total = len(buf)
    flat = np.concatenate([np.frombuffer(bytes(buf), np.uint8), np.zeros(256, np.uint8)])
    return F.Batch(flat, np.array(offs, np.uint32), np.array([len(f) for f in fr], np.uint16), total)


def _session(tmp_path, host_api, extra=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {SRC_MAC}\nip_addr = {SRC_IP}\n[port0_dst]\nmac_addr = {DST_MAC}\n"
                   "[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n"
                   "frag_buckets = 64\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    host_api.reset()
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    assert abi.lib().udpdk_init(3, argv) == 0
    s0, s1 = host_api.socket(), host_api.socket()
    assert (s0, s1) == (0, 1)
    assert host_api.bind(s0, "0.0.0.0", 10001) == 0 and host_api.bind(s1, IP1, 10002) == 0


def _oracle(b, drop, mtu, cksum):
    """(reply frames in order, deliveries per socket, meta) from the oracle's lanes."""
    lists = {abi.raw_port(10001): [(0, 0, 0)], abi.raw_port(10002): [(abi.raw_ip(IP1), 1, 0)]}
    meta, loff, lpkt, _ = O.rx(O.bindtable_from_lists(lists), b.frames, b.frames_bytes, b.offset, b.length, None, 2)
    keep = np.array([not (drop and abi.meta_udp(meta[e]) == abi.UDP_BAD) for e in lpkt], bool)
    per = [int(keep[loff[s]:loff[s + 1]].sum()) for s in range(2)]
    loff2, lpkt2 = np.array([0, per[0], per[0] + per[1]], np.uint32), lpkt[keep]
    slots = [(0, abi.raw_port(10001), 1), (abi.raw_ip(IP1), abi.raw_port(10002), 1)]
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff2, lpkt2, 0, len(lpkt2), mtu=mtu)
    _, frames = R.image(P, b.frames, slots, abi.raw_ip(SRC_IP), mtu, cksum, P.stats["bytes_needed"])
    return frames, per, meta


def _app_echo(host_api, b, per):
    """The application's way: poll, every socket receives its datagrams and sends each back."""
    st = abi.RxStats()
    assert abi.lib().udpdk_poll_rx(b.frames.ctypes.data, b.frames_bytes, b.offset.ctypes.data,
                                   b.length.ctypes.data, None, b.n, C.byref(st)) == 0
    for s in range(2):
        for _ in range(per[s]):
            n, pay, (ip, port) = host_api.recvfrom(s)
            assert n >= 0 and host_api.sendto(s, pay, ip, port) == n
    return host_api.tx_drain()


@pytest.mark.parametrize("mtu,cksum,drop", [(1500, 0, 0), (1500, 1, 0), (572, 1, abi.RX_DROP_UDP_CKSUM),
                                            (1500, 0, abi.RX_DROP_UDP_CKSUM)],
                         ids=["plain", "cksum", "mtu572-cksum-drop", "drop"])
def test_poll_echo_is_the_application_echo(tmp_path, host_api, mtu, cksum, drop):
    b = _batch()
    want, per, meta = _oracle(b, drop, mtu, bool(cksum))
    assert len(want) < 128 and min(per) > 10                 # (frames, fragments included: one TX burst)
    extra = f"tx_udp_cksum = {cksum}\n" + ("rx_drop = udp\n" if drop else "")
    _session(tmp_path, host_api, extra)
    try:
        assert abi.lib().udpdk_config_mtu(mtu) == 0
        rc, err, got, st, n_out = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length)
        assert rc == 0 and n_out == len(got) == len(want)
        assert got == want
        # the FRAG frame is counted and unanswered; the corrupt datagram's reply is there unless dropped
        assert st.counters[abi.V_FRAG] == 1 and st.counters[abi.C_UDP_BAD] >= 1
        assert st.deliveries == sum(per) and st.counters[abi.C_DELIVERIES] == sum(per) + (1 if drop else 0)
        assert sum(1 for f in got if f[30:34] == bytes([10, 8, 8, 8])) == (0 if drop else 1)
        assert not any(f[30:34] == bytes([10, 9, 9, 9]) for f in got)
        if mtu == 572:
            assert len(got) > sum(per)
        assert host_api.rx_dropped() == (1 if drop else 0)
        # the rings stayed empty and nothing waits for a drain
        assert host_api.tx_pending() == 0 and host_api.tx_drain() == []
        abi.lib().udpdk_interrupt(0)
        for s in range(2):
            assert host_api.recvfrom(s)[0] == -1 and host_api.errno() == errno.EINTR
    finally:
        abi.lib().udpdk_cleanup()
    _session(tmp_path, host_api, extra)
    try:
        assert abi.lib().udpdk_config_mtu(mtu) == 0
        assert _app_echo(host_api, b, per) == got
    finally:
        abi.lib().udpdk_cleanup()


def test_poll_echo_enobufs_then_retry(tmp_path, host_api):
    b = _batch()
    want, per, _ = _oracle(b, 0, 1500, False)
    need = sum(len(f) for f in want)
    _session(tmp_path, host_api)
    try:
        for kw in (dict(max_frames=len(want) - 1), dict(cap=need - 1), dict(max_frames=1, cap=64)):
            rc, err, got, _, n_out = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length, **kw)
            assert (rc, err, n_out, got) == (-1, errno.ENOBUFS, 0, [])
        rc, err, got, _, n_out = host_api.poll_echo(b.frames, b.frames_bytes, b.offset, b.length,
                                                    max_frames=len(want), cap=need)
        assert rc == 0 and got == want
        # an empty batch, and one without deliveries
        rc, _, got, st, n_out = host_api.poll_echo(b.frames, 0, np.zeros(0, np.uint32), np.zeros(0, np.uint16))
        assert rc == 0 and n_out == 0 and st.deliveries == 0
        rc, _, got, st, n_out = host_api.poll_echo(b.frames, b.frames_bytes, b.offset[41:42], b.length[41:42])
        assert rc == 0 and n_out == 0 and st.counters[abi.V_FRAG] == 1
    finally:
        abi.lib().udpdk_cleanup()
