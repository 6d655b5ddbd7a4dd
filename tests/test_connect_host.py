"""Connected sockets on the host: udpdk_connect / udpdk_send / udpdk_recv / udpdk_getpeername /
udpdk_getsockname and the peer table a poll uploads (udpdk_peer_lanes). No GPU needed; the frames
and the filter are test_gpu_connect_path.py's."""
import errno
import socket

import numpy as np

from udpdk_amd import abi


def _peers(host_api, n):
    rc, t = host_api.peer_lanes(n)
    return rc, [(int(r["ip"]), int(r["port"]), int(r["on"])) for r in t]


def test_connect_errors(host_api):
    s = host_api.socket()
    assert host_api.connect(5000, "10.0.0.1", 7000) == -1 and host_api.errno() == errno.ENOTSOCK
    assert host_api.connect(-1, "10.0.0.1", 7000) == -1 and host_api.errno() == errno.ENOTSOCK
    assert host_api.connect(7, "10.0.0.1", 7000) == -1 and host_api.errno() == errno.EBADF
    assert host_api.connect(s, "10.0.0.1", 7000, addrlen=15) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.connect(s, "10.0.0.1", 7000, addrlen=0) == -1 and host_api.errno() == errno.EINVAL
    assert abi.lib().udpdk_connect(s, None, 16) == -1 and host_api.errno() == errno.EINVAL
    for fam in (socket.AF_INET6, socket.AF_UNIX, 99):
        assert host_api.connect(s, "10.0.0.1", 7000, family=fam) == -1
        assert host_api.errno() == errno.EAFNOSUPPORT, fam
    # nothing of this connected or bound the socket
    assert _peers(host_api, 2) == (0, [(0, 0, 0)] * 2)
    assert host_api.slots(1)[0] == (0, 0, 0)
    assert host_api.getpeername(s)[0] == -1 and host_api.errno() == errno.ENOTCONN
    # a longer address is fine, as for POSIX connect
    a = abi.C.create_string_buffer(abi.sockaddr_in("10.0.0.1", 7000) + b"\0" * 16, 32)
    assert abi.lib().udpdk_connect(s, a, 32) == 0
    assert host_api.getpeername(s)[1] == ("10.0.0.1", 7000)


def test_connect_autobinds_like_sendto(host_api):
    """An unbound socket gets the lowest free raw port on ANY, exactly as sendto binds it."""
    a, b, c = host_api.socket(), host_api.socket(), host_api.socket()
    assert host_api.sendto(a, b"hi", "9.9.9.9", 53) == 2
    assert host_api.connect(b, "9.9.9.9", 53) == 0
    assert host_api.bind(c, "10.0.0.3", 10003) == 0
    assert host_api.connect(c, "9.9.9.9", 53) == 0          # bound already: stays where it is
    slots = host_api.slots(3)
    assert slots[0] == (0, 0, 1) and slots[1] == (0, 1, 1)
    assert slots[2] == (abi.raw_ip("10.0.0.3"), abi.raw_port(10003), 1)
    snap = host_api.snapshot()
    assert snap.port_count[0] == 1 and snap.port_count[1] == 1 and snap.port_count[abi.raw_port(10003)] == 1
    assert host_api.getsockname(b) == (0, ("0.0.0.0", socket.ntohs(1)), 16)
    assert host_api.getsockname(c) == (0, ("10.0.0.3", 10003), 16)


def test_reconnect_and_unspec(host_api):
    s = host_api.socket()
    assert host_api.connect(s, "10.0.0.1", 7000) == 0
    assert host_api.getpeername(s) == (0, ("10.0.0.1", 7000), 16)
    assert _peers(host_api, 1) == (1, [(abi.raw_ip("10.0.0.1"), abi.raw_port(7000), 1)])
    assert host_api.connect(s, "10.0.0.2", 7001) == 0       # replaces the peer
    assert host_api.getpeername(s) == (0, ("10.0.0.2", 7001), 16)
    assert _peers(host_api, 1) == (1, [(abi.raw_ip("10.0.0.2"), abi.raw_port(7001), 1)])
    bound = host_api.slots(1)[0]
    assert host_api.connect(s, 0, 0, family=socket.AF_UNSPEC) == 0
    assert host_api.getpeername(s)[0] == -1 and host_api.errno() == errno.ENOTCONN
    assert _peers(host_api, 1) == (0, [(0, 0, 0)])
    assert host_api.slots(1)[0] == bound                    # still bound where it was
    assert host_api.connect(s, 0, 0, family=socket.AF_UNSPEC, addrlen=2) == 0   # idempotent, family alone
    assert host_api.connect(s, "10.0.0.1", 7000) == 0
    assert _peers(host_api, 1)[0] == 1


def test_send_queues_what_sendto_to_the_peer_queues(host_api):
    s, t = host_api.socket(), host_api.socket()
    assert host_api.send(s, b"abc") == -1 and host_api.errno() == errno.ENOTCONN
    assert host_api.sendto_null(s, b"abc") == -1 and host_api.errno() == errno.EINVAL   # as ever
    assert host_api.tx_pending() == 0 and host_api.slots(1)[0] == (0, 0, 0)             # ... and not bound
    assert host_api.send(5000, b"x") == -1 and host_api.errno() == errno.ENOTSOCK
    assert host_api.send(7, b"x") == -1 and host_api.errno() == errno.EBADF
    assert host_api.connect(s, "172.31.100.1", 10001) == 0
    assert host_api.sendto(t, b"abc", "172.31.100.1", 10001) == 3
    assert host_api.send(s, b"abc") == 3
    assert host_api.sendto_null(s, b"defg") == 4
    assert host_api.sendto(s, b"hi", "172.31.100.9", 10009) == 2      # an address still goes to that address
    assert host_api.tx_pending() == 4
    # the same destination as the sendto above, through the table a poll uploads; the same source
    # rule through the slot table (both ANY, auto-bound raw ports 0 and 1)
    assert _peers(host_api, 2) == (1, [(abi.raw_ip("172.31.100.1"), abi.raw_port(10001), 1), (0, 0, 0)])
    assert host_api.slots(2) == [(0, 0, 1), (0, 1, 1)]
    # sendto's own checks still apply
    assert host_api.send(s, b"x", flags=1) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.send(s, b"c" * 65508) == -1 and host_api.errno() == errno.EMSGSIZE
    assert host_api.send(s, b"") == 0
    assert host_api.tx_pending() == 5
    assert host_api.connect(s, 0, 0, family=socket.AF_UNSPEC) == 0
    assert host_api.send(s, b"abc") == -1 and host_api.errno() == errno.ENOTCONN
    assert host_api.sendto_null(s, b"abc") == -1 and host_api.errno() == errno.EINVAL
    assert host_api.tx_pending() == 5


def test_names(host_api):
    s = host_api.socket()
    assert host_api.getsockname(s) == (0, ("0.0.0.0", 0), 16)           # unbound
    assert host_api.getpeername(s)[0] == -1 and host_api.errno() == errno.ENOTCONN
    assert host_api.bind(s, "10.0.0.5", 7000) == 0
    assert host_api.getsockname(s) == (0, ("10.0.0.5", 7000), 16)
    assert host_api.connect(s, "10.0.0.6", 7001) == 0
    assert host_api.getsockname(s) == (0, ("10.0.0.5", 7000), 16)
    assert host_api.getpeername(s) == (0, ("10.0.0.6", 7001), 16)
    # truncation: the length written comes back
    rc, _, n = host_api.getpeername(s, addrlen=4)
    assert (rc, n) == (0, 4)
    rc, name, n = host_api.getsockname(s, addrlen=32)
    assert (rc, name, n) == (0, ("10.0.0.5", 7000), 16)
    for fn in (abi.lib().udpdk_getpeername, abi.lib().udpdk_getsockname):
        ln = abi.C.c_uint32(16)
        buf = abi.C.create_string_buffer(16)
        assert fn(5000, buf, abi.C.byref(ln)) == -1 and host_api.errno() == errno.ENOTSOCK
        assert fn(9, buf, abi.C.byref(ln)) == -1 and host_api.errno() == errno.EBADF
        assert fn(s, None, abi.C.byref(ln)) == -1 and host_api.errno() == errno.EINVAL
        assert fn(s, buf, None) == -1 and host_api.errno() == errno.EINVAL


def test_recv_validation_is_recvfroms(host_api):
    assert host_api.recv(5000)[0] == -1 and host_api.errno() == errno.ENOTSOCK
    assert host_api.recv(3)[0] == -1 and host_api.errno() == errno.EBADF
    s = host_api.socket()
    assert abi.lib().udpdk_recv(s, None, 0, 1) == -1 and host_api.errno() == errno.EINVAL


def test_peer_lanes_follow_bind_connect_close_reset(host_api):
    assert _peers(host_api, 4) == (0, [(0, 0, 0)] * 4)
    s = [host_api.socket() for _ in range(4)]
    assert s == [0, 1, 2, 3]
    assert host_api.bind(s[0], "0.0.0.0", 10001) == 0
    assert host_api.bind(s[2], "0.0.0.0", 10002) == 0
    assert _peers(host_api, 4)[0] == 0                       # binding connects nothing
    assert host_api.connect(s[2], "10.1.2.3", 7000) == 0
    assert host_api.connect(s[3], "10.1.2.4", 7001) == 0
    p2, p3 = (abi.raw_ip("10.1.2.3"), abi.raw_port(7000), 1), (abi.raw_ip("10.1.2.4"), abi.raw_port(7001), 1)
    assert _peers(host_api, 4) == (2, [(0, 0, 0), (0, 0, 0), p2, p3])
    assert _peers(host_api, 3) == (2, [(0, 0, 0), (0, 0, 0), p2])        # a short array: still counts all
    rc, t = host_api.peer_lanes(abi.C.c_uint32(4100).value)              # past the socket count: off
    assert rc == 2 and not t[4:].view(np.uint8).any()
    assert abi.lib().udpdk_peer_lanes(None, 4) == -errno.EINVAL
    assert host_api.close(s[2]) == 0
    assert _peers(host_api, 4) == (1, [(0, 0, 0), (0, 0, 0), (0, 0, 0), p3])
    assert host_api.socket() == 2                            # the slot comes back unconnected
    assert _peers(host_api, 4)[0] == 1
    assert host_api.getpeername(2)[0] == -1 and host_api.errno() == errno.ENOTCONN
    host_api.reset()
    assert _peers(host_api, 4) == (0, [(0, 0, 0)] * 4)
    assert host_api.rx_refused() == 0
