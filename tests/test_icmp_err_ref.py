"""The model of udpdk_gpu_icmp_errors (tests/icmp_err_util.py) on vectors written out by hand, against
the model of the ICMP answers (tests/icmp_util.py: the errors one stack sends are what the other must
report), and udpdk_gpu_icmp_errno against the table. No GPU."""
import struct

import numpy as np

import icmp_err_util as E
import icmp_util as U
import oracle as O
from udpdk_amd import abi


def _csum(b: bytes) -> bytes:
    """RFC 1071 over b (even length) as the two bytes to store."""
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return struct.pack(">H", ~s & 0xFFFF)


def _hand_frame(code=3):
    """A port-unreachable from 10.0.0.9 to 172.31.100.1 about the datagram 172.31.100.1:20001 ->
    10.0.0.9:5003, byte by byte."""
    qip = bytes([0x45, 0, 0, 32, 0xAB, 0xCD, 0, 0, 64, 17, 0, 0, 172, 31, 100, 1, 10, 0, 0, 9])
    quote = qip + bytes([0x4E, 0x21, 0x13, 0x8B, 0, 12, 0, 0])      # ports 20001, 5003; UDP length 12
    icmp = bytearray(bytes([3, code, 0, 0, 0, 0, 0, 0]) + quote)
    icmp[2:4] = _csum(bytes(icmp))
    ip = bytearray([0x45, 0, 0, 56, 0, 1, 0, 0, 64, 1, 0, 0, 10, 0, 0, 9, 172, 31, 100, 1])
    ip[10:12] = _csum(bytes(ip))
    return bytes(12) + b"\x08\x00" + bytes(ip) + bytes(icmp)


META_ICMP = abi.V_NOT_UDP | 1 << 4                                  # NOT_UDP, header checksum fine, IHL 5


def _one(frames, metas, lists, peers, n_lanes=4):
    buf, nb, off, ln = U.pack(frames)
    return E.model(buf, nb, off, ln, np.array(metas, np.uint32), lists, peers, n_lanes)


def test_hand_written_port_unreachable():
    f = _hand_frame()
    assert len(f) == 70 and f[34] == 3 and f[35] == 3
    lists = {abi.raw_port(20001): [(0, 2, 0)]}
    peers = np.zeros(4, abi.PEER_DTYPE)
    peers[2] = (abi.raw_ip("10.0.0.9"), abi.raw_port(5003), 1)
    err, st = _one([bytes(60), f], [abi.V_DELIVERED, META_ICMP], lists, peers)
    assert err.tolist() == [0, 0, (2 << 8) | 3, 0]                  # frame 1: (1 + 1) << 8 | code 3, to lane 2
    assert st == dict(errors=1, msg_bad=0, quote_bad=0, soft=0, no_socket=0, reported=1, bad_frame=0)
    # the same bytes under other verdict words, tables and codes
    assert _one([f], [abi.V_NOT_UDP], lists, peers)[1]["errors"] == 0           # header checksum bit clear
    assert _one([f], [META_ICMP | 1 << 8], lists, peers)[1]["errors"] == 0      # IHL != 5
    assert _one([f], [abi.V_DELIVERED | 1 << 4], lists, peers)[1]["errors"] == 0
    peers[2]["port"] = abi.raw_port(5004)
    err, st = _one([f], [META_ICMP], lists, peers)
    assert not err.any() and st["no_socket"] == 1 and st["reported"] == 0
    peers[2]["port"] = abi.raw_port(5003)
    err, st = _one([_hand_frame(1)], [META_ICMP], lists, peers)
    assert not err.any() and st["soft"] == 1
    bad = bytearray(f)
    bad[50] ^= 1
    assert _one([bytes(bad)], [META_ICMP], lists, peers)[1]["msg_bad"] == 1
    # a specific bind that is not the quoted source; the descriptor gate
    assert _one([f], [META_ICMP], {abi.raw_port(20001): [(abi.raw_ip("172.31.100.9"), 2, 0)]}, peers)[1]["no_socket"] == 1
    assert _one([f[:41]], [META_ICMP], lists, peers)[1] == dict.fromkeys(E.STATS, 0) | {"bad_frame": 1}


def test_last_hard_error_wins_and_every_match_is_reported():
    lists = {abi.raw_port(20001): [(0, 0, 1), (0, 3, 1), (abi.raw_ip("172.31.100.1"), 1, 0)]}
    peers = np.zeros(4, abi.PEER_DTYPE)
    for l in (0, 1, 3):
        peers[l] = (abi.raw_ip("10.0.0.9"), abi.raw_port(5003), 1)
    err, st = _one([_hand_frame(3), _hand_frame(10), _hand_frame(0)], [META_ICMP] * 3, lists, peers)
    assert err.tolist() == [(2 << 8) | 10, (2 << 8) | 10, 0, (2 << 8) | 10]
    assert st["reported"] == 6 and st["soft"] == 1 and st["errors"] == 3
    err, st = _one([_hand_frame(3)], [META_ICMP], lists, peers, n_lanes=3)      # lane 3 is out of the call's lanes
    assert err.tolist() == [(1 << 8) | 3] * 2 + [0] and st["reported"] == 2


def test_the_errors_the_answer_model_builds_reach_their_sockets():
    """A client at 172.31.100.2 whose connected sockets send to a closed port of the server at
    172.31.100.1: every port-unreachable of icmp_util.model is reported to exactly the sender."""
    rng = np.random.default_rng(3)
    client, server = "172.31.100.2", U.OUR_IP
    socks = [E.Sock(fd, None if fd % 2 else client, 30000 + fd, 0, (server, U.CLOSED_PORT)) for fd in range(6)]
    socks += [E.Sock(6, None, 30006, 0, None), E.Sock(7, None, 30007, 0, (server, 8))]
    order = [0, 1, 2, 3, 4, 5, 6, 7, 2, 2, 5]
    reqs = [E.sent_frame(rng, socks[k], 10 + 3 * j, our_ip=client, to=(server, U.CLOSED_PORT)) for j, k in enumerate(order)]
    buf, nb, off, ln = U.pack(reqs)
    meta = O.rx(O.bindtable_from_lists(U.LISTS), buf, nb, off, ln, None, U.N_LANES)[0]
    R = U.model(buf, nb, off, ln, meta, flags=U.UNREACH)
    assert R.stats["unreach_sent"] == len(order)
    ebuf, enb, eoff, eln = U.pack(R.frames_out, aligns=list(range(len(order))))
    lists = E.lists_of(socks)
    emeta = E.meta_of(lists, 8, ebuf, enb, eoff, eln)
    assert np.all(emeta == META_ICMP)
    err, st = E.model(ebuf, enb, eoff, eln, emeta, lists, E.peers_of(socks, 8), 8, our_ip=abi.raw_ip(client))
    last = {k: j for j, k in enumerate(order)}
    want = [((last[fd] + 1) << 8 | 3) if fd < 6 else 0 for fd in range(8)]     # 6: unconnected; 7: another peer port
    assert err.tolist() == want
    assert st == dict(errors=11, msg_bad=0, quote_bad=0, soft=0, no_socket=2, reported=9, bad_frame=0)


def test_mixed_generator_covers_every_kind():
    M = E.mixed(1, 600)
    err, st = E.model(M.buf, M.nb, M.off, M.ln, M.meta, M.lists, M.peers, E.N_LANES)
    for k in ("errors", "msg_bad", "quote_bad", "soft", "no_socket", "reported"):
        assert st[k] >= 3, (k, st)
    n = len(M.kinds)
    assert M.kinds[-2:] == ["last_hard", "last_soft"] and int(err[E.LAST_FD]) == ((n - 1) << 8) | 2
    assert int(err[E.PAIR[0]]) == int(err[E.PAIR[1]]) != 0
    assert err[[s.fd for s in M.socks if not s.peer]].sum() == 0


def test_errno_table():
    for code in range(21):
        assert abi.icmp_errno(code) == E.table(code), code
    assert abi.lib().udpdk_gpu_icmp_errno(3, None) == E.TABLE[3][0]
    # the rows of the specification spelled out once more, by name
    import errno
    assert [abi.icmp_errno(c)[0] for c in (2, 3, 4, 5, 7, 8)] == [errno.ENOPROTOOPT, errno.ECONNREFUSED,
                                                                   errno.EMSGSIZE, errno.EOPNOTSUPP,
                                                                   errno.EHOSTDOWN, errno.ENONET]
    assert [c for c in range(21) if abi.icmp_errno(c)[1]] == [2, 3, 6, 7, 8, 9, 10, 13, 14, 15]
