"""The multicast switch of the socket layer without a GPU: IP_ADD_MEMBERSHIP / IP_DROP_MEMBERSHIP and
their errno values, udpdk_close dropping a socket's groups, the ini key, what sharded polls refuse,
and the unsolicited report and the leave as udpdk_tx_pending and udpdk_mcast_counts see them (their
bytes as udpdk_tx_drain emits them are test_gpu_mcast_path.py's: the drain needs the session's GPU)."""
import ctypes as C
import errno
import struct

import pytest

import mcast_util as U
from udpdk_amd import abi

MAC, PEER_MAC, IP = U.SRC_MAC, U.QUERIER_MAC, "10.0.0.2"
ADD, DROP = abi.IP_ADD_MEMBERSHIP, abi.IP_DROP_MEMBERSHIP


def _init(tmp_path, lines):
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 10.0.0.2\n[gpu]\n" + lines)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


def _sent(api):
    c = api.mcast_counts()
    return c["joins"], c["leaves"], c["reports_sent"], c["leaves_sent"]


def test_membership_errors(host_api):
    assert host_api.config_set(MAC, PEER_MAC, IP) == 0
    s = host_api.socket()
    assert host_api.join(s, U.G1) == 0
    assert host_api.join(s, U.G1) == -1 and host_api.errno() == errno.EADDRINUSE
    assert host_api.join(s, U.G1, IP) == -1 and host_api.errno() == errno.EADDRINUSE      # our address names our port
    assert host_api.join(s, U.G2, IP) == 0
    assert host_api.join(s, U.G3, "10.0.0.3") == -1 and host_api.errno() == errno.ENODEV
    assert host_api.membership(s, ADD, U.G3, 0, ifindex=0) == 0                             # struct ip_mreqn
    assert host_api.membership(s, ADD, "239.3.3.3", 0, ifindex=2) == -1 and host_api.errno() == errno.ENODEV
    for not_a_group in ("223.255.255.255", "240.0.0.0", "10.0.0.2", "0.0.0.0", "255.255.255.255"):
        assert host_api.join(s, not_a_group) == -1 and host_api.errno() == errno.EINVAL, not_a_group
        assert host_api.leave(s, not_a_group) == -1 and host_api.errno() == errno.EINVAL, not_a_group
    assert host_api.leave(s, "239.9.9.9") == -1 and host_api.errno() == errno.EADDRNOTAVAIL
    assert host_api.leave(s, U.G1) == 0
    assert host_api.leave(s, U.G1) == -1 and host_api.errno() == errno.EADDRNOTAVAIL
    assert host_api.leave(s, U.G2, "10.0.0.3") == -1 and host_api.errno() == errno.ENODEV
    assert host_api.join(s, "224.0.0.1") == 0 and host_api.join(s, "239.255.255.255") == 0   # the ends of 224/4
    L = abi.lib()
    v = struct.pack("<II", abi.raw_ip(U.G1), 0)
    buf = C.create_string_buffer(v, 8)
    assert L.udpdk_setsockopt(s, abi.IPPROTO_IP, ADD, None, 8) == -1 and host_api.errno() == errno.EFAULT
    assert L.udpdk_setsockopt(s, abi.IPPROTO_IP, ADD, buf, 7) == -1 and host_api.errno() == errno.EINVAL
    for opt in (1, 2, 32, 33, 34, 37, 49):             # IP_TOS, IP_TTL, IP_MULTICAST_IF / _TTL / _LOOP, IP_UNBLOCK_SOURCE, IP_MULTICAST_ALL
        assert L.udpdk_setsockopt(s, abi.IPPROTO_IP, opt, buf, 8) == -1 and host_api.errno() == errno.ENOPROTOOPT, opt
    assert L.udpdk_setsockopt(s + 1, abi.IPPROTO_IP, ADD, buf, 8) == -1 and host_api.errno() == errno.EBADF
    assert L.udpdk_setsockopt(-1, abi.IPPROTO_IP, ADD, buf, 8) == -1 and host_api.errno() == errno.EBADF
    # every other level behaves as before
    assert L.udpdk_setsockopt(s, 17, ADD, buf, 8) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.setsockopt(s, 1, 15, 1) == 0 and host_api.getsockopt(s, 1, 15) == (0, 1)
    assert host_api.mcast_counts()["joins"] == 5 and host_api.mcast_counts()["leaves"] == 1


def test_twenty_groups_per_socket(host_api):
    s, t = host_api.socket(), host_api.socket()
    for k in range(20):
        assert host_api.join(s, f"239.2.0.{k}") == 0
    assert host_api.join(s, "239.2.0.20") == -1 and host_api.errno() == errno.ENOBUFS
    assert host_api.join(t, "239.2.0.20") == 0                       # the limit is per socket
    assert host_api.leave(s, "239.2.0.7") == 0 and host_api.join(s, "239.2.0.20") == 0
    assert host_api.join(s, "239.2.0.7") == -1 and host_api.errno() == errno.ENOBUFS


def test_switch_values(host_api):
    assert host_api.config_mcast(-1) == 0                            # off by default
    assert host_api.config_mcast(2) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_mcast(1) == 0 and host_api.config_mcast(-1) == 1 and host_api.config_mcast(-7) == 1
    assert host_api.config_mcast(0) == 1 and host_api.config_mcast(-1) == 0
    assert host_api.config_mcast(1) == 0
    host_api.reset()
    assert host_api.config_mcast(-1) == 0                            # udpdk_host_reset: off again
    assert host_api.rx_not_member() == 0 and not any(host_api.mcast_counts().values())
    assert abi.lib().udpdk_mcast_counts(None) == -1 and host_api.errno() == errno.EINVAL


def test_reports_and_leaves_queued(host_api):
    """The first join of a group queues one report, the last drop one leave; memberships are recorded
    with the switch off and announced when it goes on; 224.0.0.1 is never reported."""
    assert host_api.config_set(MAC, PEER_MAC, IP) == 0
    s, t = host_api.socket(), host_api.socket()
    assert host_api.join(s, U.G1) == 0 and host_api.join(s, "224.0.0.1") == 0
    assert host_api.tx_pending() == 0 and _sent(host_api) == (2, 0, 0, 0)           # the switch is off
    assert host_api.config_mcast(1) == 0
    assert host_api.tx_pending() == 1 and _sent(host_api) == (2, 0, 1, 0)           # G1, not all-hosts
    assert host_api.config_mcast(1) == 1 and host_api.tx_pending() == 1             # on already: nothing more
    assert host_api.join(t, U.G1) == 0 and host_api.tx_pending() == 1               # not the group's first
    assert host_api.join(t, U.G2) == 0 and host_api.tx_pending() == 2
    assert host_api.leave(s, U.G1) == 0 and host_api.tx_pending() == 2              # t still holds it
    assert host_api.leave(t, U.G1) == 0 and host_api.tx_pending() == 3              # the last drop: a leave
    assert host_api.leave(s, "224.0.0.1") == 0 and host_api.tx_pending() == 3
    assert _sent(host_api) == (4, 3, 2, 1)
    assert host_api.close(t) == 0                                                   # G2 goes with the socket
    assert host_api.tx_pending() == 4 and _sent(host_api) == (4, 4, 2, 2)
    t2 = host_api.socket()
    assert t2 == t and host_api.leave(t2, U.G2) == -1 and host_api.errno() == errno.EADDRNOTAVAIL
    assert host_api.join(t2, U.G2) == 0 and host_api.tx_pending() == 5              # a first join again
    assert host_api.config_mcast(0) == 1
    assert host_api.leave(t2, U.G2) == 0 and host_api.tx_pending() == 5             # off: recorded, not sent
    host_api.reset()
    assert host_api.tx_pending() == 0 and not any(host_api.mcast_counts().values())


def test_no_source_address_sends_nothing(host_api):
    assert host_api.config_set(MAC, PEER_MAC, "0.0.0.0") == 0
    assert host_api.config_mcast(1) == 0
    s = host_api.socket()
    assert host_api.join(s, U.G1) == 0 and host_api.leave(s, U.G1) == 0
    assert host_api.tx_pending() == 0 and _sent(host_api) == (1, 1, 0, 0)


@pytest.mark.parametrize("lines,want", [
    ("", 0), ("mcast = 0\n", 0), ("mcast = 1\n", 1), ("mcast = 1\narp = 1\n", 1),
    ("mcast = 2\n", None), ("mcast = on\n", None), ("mcast = \n", None), ("mcast = 1\ndevices = 0,0\n", None)])
def test_ini_key(tmp_path, host_api, lines, want):
    """udpdk_init reads the whole file before it looks for a GPU: a bad value is EINVAL either way, a
    good one leaves ENODEV here (or a session, on a machine with a GPU) and the parsed setting."""
    if abi.lib().udpdk_gpu_context():                        # (a session some other test left up)
        return
    rc = _init(tmp_path, lines)
    try:
        if want is None:
            assert rc == -1 and host_api.errno() == errno.EINVAL
        else:
            assert rc == 0 or host_api.errno() == errno.ENODEV
            assert host_api.config_mcast(-1) == want
    finally:
        abi.lib().udpdk_cleanup()


def test_sharded_polls_refuse_the_switch(tmp_path, host_api):
    """[gpu] devices with two entries: on is ENOTSUP, as for udpdk_config_arp; memberships still record."""
    if abi.lib().udpdk_gpu_context():
        return
    rc = _init(tmp_path, "devices = 0,0\n")
    try:
        assert rc == 0 or host_api.errno() == errno.ENODEV
        assert host_api.config_mcast(1) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_mcast(0) == 0 and host_api.config_mcast(-1) == 0
        assert host_api.config_mcast(2) == -1 and host_api.errno() == errno.EINVAL
        s = host_api.socket()
        assert host_api.join(s, U.G1) == 0 and host_api.leave(s, U.G1) == 0
    finally:
        abi.lib().udpdk_cleanup()
    rc = _init(tmp_path, "")                                 # the next session's ini is not sharded
    try:
        assert rc == 0 or host_api.errno() == errno.ENODEV
        assert host_api.config_mcast(1) == 0
    finally:
        abi.lib().udpdk_cleanup()
