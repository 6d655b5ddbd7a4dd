"""A connected socket's pending error on the host: udpdk_sock_error_post, the way the socket calls
report and clear it (as Linux reports sk_err), udpdk_config_icmp_errors and udpdk_icmp_err_counts. No
GPU needed; the device stage that finds the errors is test_gpu_icmp_err.py's, the polls
test_gpu_icmp_err_path.py's."""
import errno
import socket
import threading

import pytest

from udpdk_amd import abi

PEER = ("10.0.0.1", 7000)
SO_ERROR = socket.SO_ERROR


def _sock(api, peer=PEER):
    s = api.socket()
    assert api.bind(s, "0.0.0.0", 10001 + s) == 0
    if peer:
        assert api.connect(s, *peer) == 0
    return s


def _so_error(api, s):
    rc, v = api.getsockopt(s, abi.SOL_SOCKET, SO_ERROR)
    assert rc == 0
    return v


def _fails(api, call, err):
    rc = call()
    rc = rc[0] if isinstance(rc, tuple) else rc
    return rc == -1 and api.errno() == err


def test_error_comes_before_queued_data(host_api):
    s = _sock(host_api)
    assert host_api.rx_inject(s, b"first", *PEER) == 0 and host_api.rx_inject(s, b"second", *PEER) == 0
    assert host_api.sock_error_post(s, *PEER, 3) == 1
    assert _fails(host_api, lambda: host_api.recvfrom(s), errno.ECONNREFUSED)
    assert host_api.recvfrom(s) == (5, b"first", PEER)               # the data stayed queued
    assert host_api.sock_error_post(s, *PEER, 2) == 1
    assert _fails(host_api, lambda: host_api.recv(s), errno.ENOPROTOOPT)
    assert host_api.recv(s) == (6, b"second")
    assert _so_error(host_api, s) == 0


@pytest.mark.parametrize("call", ["recvfrom", "recv", "sendto", "send", "sendto_null", "so_error"])
def test_each_call_reports_once_and_clears(host_api, call):
    s = _sock(host_api)
    assert host_api.sock_error_post(s, *PEER, 3) == 1
    if call == "so_error":
        assert _so_error(host_api, s) == errno.ECONNREFUSED
    else:
        f = {"recvfrom": lambda: host_api.recvfrom(s), "recv": lambda: host_api.recv(s),
             "sendto": lambda: host_api.sendto(s, b"x", "10.9.9.9", 9), "send": lambda: host_api.send(s, b"x"),
             "sendto_null": lambda: host_api.sendto_null(s, b"x")}[call]
        assert _fails(host_api, f, errno.ECONNREFUSED)
        assert host_api.tx_pending() == 0                            # the failed send queued nothing
    assert _so_error(host_api, s) == 0                               # cleared
    assert host_api.send(s, b"again") == 5 and host_api.tx_pending() == 1
    assert host_api.rx_inject(s, b"data", *PEER) == 0 and host_api.recv(s) == (4, b"data")


def test_so_error_option_rules(host_api):
    s = _sock(host_api)
    assert host_api.setsockopt(s, abi.SOL_SOCKET, SO_ERROR, 0) == -1 and host_api.errno() == errno.ENOPROTOOPT
    assert host_api.getsockopt(99, abi.SOL_SOCKET, SO_ERROR)[0] == -1 and host_api.errno() == errno.EBADF
    assert host_api.getsockopt(s, 6, SO_ERROR)[0] == -1 and host_api.errno() == errno.EINVAL
    assert abi.lib().udpdk_getsockopt(s, abi.SOL_SOCKET, SO_ERROR, None, None) == -1 and host_api.errno() == errno.EFAULT
    assert _so_error(host_api, s) == 0
    assert host_api.getsockopt(s, abi.SOL_SOCKET, abi.SO_REUSEADDR) == (0, 0)    # the other options as ever


def test_posts_that_change_nothing(host_api):
    s, u = _sock(host_api), _sock(host_api, peer=None)
    for code in (0, 1, 4, 5, 11, 12, 16, 255):                      # soft codes, codes without an entry
        assert host_api.sock_error_post(s, *PEER, code) == 0, code
    assert host_api.sock_error_post(s, "10.0.0.2", 7000, 3) == 0     # another peer address
    assert host_api.sock_error_post(s, "10.0.0.1", 7001, 3) == 0     # another peer port
    assert host_api.sock_error_post(u, *PEER, 3) == 0                # not connected
    c = _sock(host_api)
    assert host_api.close(c) == 0
    assert host_api.sock_error_post(c, *PEER, 3) == 0                # closed
    assert host_api.sock_error_post(-1, *PEER, 3) == 0 and host_api.sock_error_post(1 << 20, *PEER, 3) == 0
    assert _so_error(host_api, s) == 0 and _so_error(host_api, u) == 0
    assert host_api.icmp_err_counts().posted == 0


def test_every_hard_code_posts_its_errno(host_api):
    s = _sock(host_api)
    want = {2: errno.ENOPROTOOPT, 3: errno.ECONNREFUSED, 6: errno.ENETUNREACH, 7: errno.EHOSTDOWN, 8: errno.ENONET,
            9: errno.ENETUNREACH, 10: errno.EHOSTUNREACH, 13: errno.EHOSTUNREACH, 14: errno.EHOSTUNREACH,
            15: errno.EHOSTUNREACH}
    for code, e in want.items():
        assert host_api.sock_error_post(s, *PEER, code) == 1 and _so_error(host_api, s) == e, code
    assert host_api.icmp_err_counts().posted == len(want)


def test_connect_close_and_reset_clear_it(host_api):
    s = _sock(host_api)
    assert host_api.sock_error_post(s, *PEER, 3) == 1
    assert host_api.connect(s, "10.0.0.2", 7001) == 0               # a new peer
    assert _so_error(host_api, s) == 0 and host_api.send(s, b"x") == 1
    assert host_api.sock_error_post(s, *PEER, 3) == 0                # the old peer's error is nobody's now
    assert host_api.sock_error_post(s, "10.0.0.2", 7001, 3) == 1
    assert host_api.connect(s, 0, 0, family=socket.AF_UNSPEC) == 0
    assert _so_error(host_api, s) == 0
    assert host_api.connect(s, *PEER) == 0 and host_api.sock_error_post(s, *PEER, 3) == 1
    assert host_api.close(s) == 0
    t = host_api.socket()                                            # the slot again
    assert t == s and _so_error(host_api, t) == 0
    assert host_api.connect(t, *PEER) == 0 and host_api.sock_error_post(t, *PEER, 3) == 1
    host_api.reset()
    t = host_api.socket()
    assert t == s and _so_error(host_api, t) == 0


def test_a_later_post_overwrites(host_api):
    s = _sock(host_api)
    assert host_api.sock_error_post(s, *PEER, 3) == 1 and host_api.sock_error_post(s, *PEER, 10) == 1
    assert host_api.sock_error_post(s, *PEER, 0) == 0                # a soft one does not touch it
    assert _so_error(host_api, s) == errno.EHOSTUNREACH and _so_error(host_api, s) == 0


def test_a_blocked_recvfrom_returns_the_error(host_api):
    s = _sock(host_api)
    got = {}
    started = threading.Event()

    def reader():
        started.set()
        n, _, _ = host_api.recvfrom(s, 64)
        got["n"], got["errno"] = n, host_api.errno()
    watchdog = threading.Timer(30.0, abi.lib().udpdk_interrupt, [0])     # a hang ends as EINTR
    watchdog.start()
    t = threading.Thread(target=reader)
    t.start()
    try:
        assert started.wait(10)
        assert host_api.sock_error_post(s, *PEER, 3) == 1
        t.join(20)
        assert not t.is_alive() and got == {"n": -1, "errno": errno.ECONNREFUSED}
    finally:
        watchdog.cancel()
        abi.lib().udpdk_interrupt(0)
        t.join(5)


def test_config_conventions(host_api):
    assert host_api.config_icmp_errors(-1) == 0                      # off by default
    assert host_api.config_icmp_errors(1) == 0 and host_api.config_icmp_errors(-1) == 1
    assert host_api.config_icmp_errors(2) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_icmp_errors(-5) == 1
    assert host_api.config_icmp_errors(0) == 1 and host_api.config_icmp_errors(1) == 0
    host_api.reset()
    assert host_api.config_icmp_errors(-1) == 0


def test_counters_and_reset(host_api):
    s = _sock(host_api)
    c = host_api.icmp_err_counts()
    assert [getattr(c, k) for k, _ in c._fields_] == [0] * 7
    assert host_api.sock_error_post(s, *PEER, 3) == 1 and host_api.sock_error_post(s, *PEER, 3) == 1
    assert host_api.sock_error_post(s, *PEER, 1) == 0
    c = host_api.icmp_err_counts()
    assert c.posted == 2 and c.errors == c.reported == 0             # the device counts come from polls
    assert abi.lib().udpdk_icmp_err_counts(None) == -1 and host_api.errno() == errno.EINVAL
    host_api.reset()
    assert host_api.icmp_err_counts().posted == 0
