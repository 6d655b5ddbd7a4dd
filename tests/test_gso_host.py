"""UDP_SEGMENT on the host: the socket option, udpdk_sendmsg and its control message, the size rules
of a send with a segment size in force, and udpdk_gso_counts. No GPU needed; the drain and the
frames are test_gpu_gso_path.py's."""
import ctypes as C
import errno
import json
import os
import struct

import pytest

from udpdk_amd import abi

VEC = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gso_vectors.json")))
UDP, SEG = abi.SOL_UDP, abi.UDP_SEGMENT
ZERO = dict(sends=0, segments=0, plans=0, refused=0)


def _errno(name):
    return getattr(errno, name) if name else None


@pytest.mark.parametrize("v", VEC["sockopt"], ids=lambda v: str(v["value"]))
def test_sockopt_values(host_api, v):
    s = host_api.socket()
    assert host_api.getsockopt(s, UDP, SEG) == (0, 0)
    rc = host_api.setsockopt(s, UDP, SEG, v["value"])
    if v["errno"]:
        assert rc == -1 and host_api.errno() == _errno(v["errno"])
        assert host_api.getsockopt(s, UDP, SEG) == (0, 0)
    else:
        assert rc == 0 and host_api.getsockopt(s, UDP, SEG) == (0, v["value"])


def test_sockopt_errors_and_lifetime(host_api):
    L = host_api.L
    s = host_api.socket()
    v = C.c_int(1200)
    ln = C.c_uint32(4)
    assert L.udpdk_setsockopt(s, UDP, SEG, C.byref(v), 3) == -1 and host_api.errno() == errno.EINVAL
    assert L.udpdk_setsockopt(s, UDP, SEG, None, 4) == -1 and host_api.errno() == errno.EFAULT
    assert L.udpdk_getsockopt(s, UDP, SEG, None, C.byref(ln)) == -1 and host_api.errno() == errno.EFAULT
    assert L.udpdk_setsockopt(s, UDP, SEG, C.byref(v), 8) == 0        # a longer value is fine
    assert host_api.getsockopt(s, UDP, SEG) == (0, 1200)
    assert host_api.setsockopt(4000, UDP, SEG, 1) == -1 and host_api.errno() == errno.EBADF
    assert host_api.setsockopt(-1, UDP, SEG, 1) == -1 and host_api.errno() == errno.EBADF
    # the option is the socket's own; SOL_SOCKET keeps its answers
    t = host_api.socket()
    assert host_api.getsockopt(t, UDP, SEG) == (0, 0)
    assert host_api.setsockopt(s, abi.socket.SOL_SOCKET, SEG, 1) == -1 and host_api.errno() == errno.ENOPROTOOPT
    # close clears it: the slot's next socket starts without one
    assert host_api.close(s) == 0
    assert host_api.getsockopt(s, UDP, SEG)[0] == -1 and host_api.errno() == errno.EBADF
    assert host_api.socket() == s and host_api.getsockopt(s, UDP, SEG) == (0, 0)
    assert host_api.setsockopt(s, UDP, SEG, 500) == 0
    host_api.reset()
    assert host_api.socket() == s and host_api.getsockopt(s, UDP, SEG) == (0, 0)


@pytest.mark.parametrize("how", ["sockopt", "cmsg", "send"])
@pytest.mark.parametrize("v", VEC["send_errno"], ids=lambda v: f"{v['gso']}-{v['mtu']}-{v['len']}")
def test_size_rules(host_api, v, how):
    """The errno table with the size from the socket option (udpdk_sendto), from the control message
    (udpdk_sendmsg) and on a connected socket (udpdk_send)."""
    assert host_api.L.udpdk_config_mtu(v["mtu"]) == 0
    s = host_api.socket()
    data = bytes(i & 0xFF for i in range(v["len"]))
    if how != "cmsg":
        assert host_api.setsockopt(s, UDP, SEG, v["gso"]) == 0
    if how == "sockopt":
        rc = host_api.sendto(s, data, "10.0.0.9", 7000)
    elif how == "send":
        assert host_api.connect(s, "10.0.0.9", 7000) == 0
        rc = host_api.send(s, data)
    else:
        rc = host_api.sendmsg(s, [data], "10.0.0.9", 7000, gso=v["gso"])
    want = _errno(v["errno"])
    if want:
        assert rc == -1 and host_api.errno() == want
        assert host_api.tx_pending() == 0
        assert host_api.gso_counts() == dict(ZERO, refused=int(want == errno.EINVAL))
    else:
        assert rc == v["len"] and host_api.tx_pending() == 1     # one entry, whatever its segments
        g = v["entry_gso"]
        assert host_api.gso_counts() == (dict(ZERO, sends=1, segments=-(-v["len"] // g)) if g else ZERO)


def test_cmsg_overrides_the_socket_option(host_api):
    s = host_api.socket()
    assert host_api.setsockopt(s, UDP, SEG, 1473) == 0          # 28 + 1473 > 1500: every send is refused
    assert host_api.sendto(s, b"x", "10.0.0.9", 7000) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.sendmsg(s, [b"x" * 300], "10.0.0.9", 7000, gso=100) == 300
    assert host_api.sendmsg(s, [b"x" * 300], "10.0.0.9", 7000, gso=0) == 300      # 0: off for this call
    assert host_api.gso_counts() == dict(sends=1, segments=3, plans=0, refused=1)
    assert host_api.getsockopt(s, UDP, SEG) == (0, 1473)


def test_sendmsg_control_parsing(host_api):
    s = host_api.socket()
    dst = ("10.0.0.9", 7000)
    two = struct.pack("<H", 100)
    bad = [abi.cmsg(UDP, SEG, struct.pack("<I", 100)),                   # an int, as setsockopt takes
           abi.cmsg(UDP, SEG, b"\x64"),                                  # one byte
           abi.cmsg(UDP, SEG + 1, two),                                  # another type (UDP_GRO)
           abi.cmsg(abi.socket.SOL_SOCKET, SEG, two),                    # another level
           abi.cmsg(UDP, SEG, two) + abi.cmsg(abi.socket.IPPROTO_IP, 8, struct.pack("<I", 0))]
    for c in bad:
        assert host_api.sendmsg(s, [b"y" * 300], *dst, control=c) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.tx_pending() == 0 and host_api.gso_counts() == ZERO  # (not the size rules' refusals)
    assert host_api.sendmsg(s, [b"y" * 300], *dst, control=abi.cmsg(UDP, SEG, two)) == 300
    # two good ones: the last wins
    assert host_api.sendmsg(s, [b"y" * 300], *dst, control=abi.cmsg(UDP, SEG, two) +
                            abi.cmsg(UDP, SEG, struct.pack("<H", 150))) == 300
    assert host_api.gso_counts() == dict(ZERO, sends=2, segments=5)
    # flags must be 0 (no MSG_MORE); a NULL msghdr
    assert host_api.sendmsg(s, [b"y"], *dst, flags=0x8000) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.L.udpdk_sendmsg(s, None, 0) == -1 and host_api.errno() == errno.EFAULT
    assert host_api.sendmsg(5000, [b"y"], *dst) == -1 and host_api.errno() == errno.ENOTSOCK
    assert host_api.sendmsg(77, [b"y"], *dst) == -1 and host_api.errno() == errno.EBADF


def test_sendmsg_without_a_size_is_sendto(host_api):
    """Auto-bind, EMSGSIZE and the queue as udpdk_sendto has them."""
    a, b = host_api.socket(), host_api.socket()
    assert host_api.sendto(a, b"hi", "9.9.9.9", 53) == 2
    assert host_api.sendmsg(b, [b"h", b"", b"i"], "9.9.9.9", 53) == 2
    assert host_api.slots(2) == [(0, 0, 1), (0, 1, 1)]          # both auto-bound the same way
    assert host_api.sendmsg(b, [], "9.9.9.9", 53) == 0          # an empty datagram
    assert host_api.sendmsg(b, [b"z" * 40000, b"z" * 25508], "9.9.9.9", 53) == -1
    assert host_api.errno() == errno.EMSGSIZE
    assert host_api.sendmsg(b, [b"z" * 40000, b"z" * 25507], "9.9.9.9", 53) == 65507
    assert host_api.tx_pending() == 4 and host_api.gso_counts() == ZERO
    # ENOBUFS when the ring is full, as for sendto
    for _ in range(2047 - 3):
        assert host_api.sendmsg(b, [b"q"], "9.9.9.9", 53) == 1
    assert host_api.sendmsg(b, [b"q"], "9.9.9.9", 53) == -1 and host_api.errno() == errno.ENOBUFS


def test_sendmsg_null_name(host_api):
    s = host_api.socket()
    assert host_api.sendmsg(s, [b"abc"], None, gso=2) == -1 and host_api.errno() == errno.EINVAL    # unconnected
    assert host_api.gso_counts() == ZERO and host_api.tx_pending() == 0
    assert host_api.connect(s, "10.0.0.7", 7007) == 0
    assert host_api.sendmsg(s, [b"ab", b"c"], None, gso=2) == 3
    assert host_api.sendmsg(s, [b"abc"], "10.0.0.8", 7008, gso=2) == 3      # an address wins, connected or not
    assert host_api.tx_pending() == 2 and host_api.gso_counts() == dict(ZERO, sends=2, segments=4)


def test_pending_error_comes_first(host_api):
    s = host_api.socket()
    assert host_api.connect(s, "10.0.0.7", 7007) == 0
    assert host_api.setsockopt(s, UDP, SEG, 1473) == 0          # would be refused with EINVAL
    assert host_api.sock_error_post(s, "10.0.0.7", 7007, 3) == 1
    assert host_api.sendmsg(s, [b"x" * 10], None) == -1 and host_api.errno() == errno.ECONNREFUSED
    assert host_api.gso_counts() == ZERO                        # the error was taken before the size rules
    assert host_api.sendmsg(s, [b"x" * 10], None) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.sock_error_post(s, "10.0.0.7", 7007, 3) == 1
    assert host_api.sendmsg(s, [b"x"], None, control=abi.cmsg(UDP, SEG, b"\1")) == -1
    assert host_api.errno() == errno.ECONNREFUSED               # ... and before the control messages
    assert host_api.gso_counts() == dict(ZERO, refused=1)


def test_counts_reset(host_api):
    s = host_api.socket()
    assert host_api.sendmsg(s, [b"x" * 640], "10.0.0.9", 7000, gso=10) == 640
    assert host_api.sendmsg(s, [b"x" * 641], "10.0.0.9", 7000, gso=10) == -1
    assert host_api.gso_counts() == dict(sends=1, segments=64, plans=0, refused=1)
    assert host_api.L.udpdk_gso_counts(None) == -1 and host_api.errno() == errno.EINVAL
    host_api.reset()
    assert host_api.gso_counts() == ZERO and host_api.tx_pending() == 0
