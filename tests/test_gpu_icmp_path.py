"""ICMP answers through the socket layer: udpdk_poll_rx with [gpu] icmp set builds echo replies and
port-unreachable errors on the GPU and queues them; udpdk_tx_drain emits them first. Socket 0 is
bound ANY:10001, socket 1 172.31.100.9:10002 (tests/icmp_util.py's binding lists); the stack's own
address is 172.31.100.1. The expected frames are the model's over the oracle's verdict words."""
import ctypes as C
import errno
import threading

import numpy as np
import pytest

import icmp_util as U
import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu


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
    assert _init(tmp_path, getattr(request, "param", "")) == 0
    s0, s1 = host_api.socket(), host_api.socket()
    assert host_api.bind(s0, "0.0.0.0", 10001) == 0 and host_api.bind(s1, U.OTHER_IP, 10002) == 0
    yield host_api
    abi.lib().udpdk_cleanup()


def _poll(bt):
    buf, nb, off, ln = bt[:4]
    flat = np.concatenate([buf, np.zeros(256, np.uint8)])
    st = abi.RxStats()
    rc = abi.lib().udpdk_poll_rx(flat.ctypes.data, nb, off.ctypes.data, ln.ctypes.data, None, len(off), C.byref(st))
    return rc, st


def _model(bt, **kw):
    buf, nb, off, ln = bt[:4]
    meta = O.rx(O.bindtable_from_lists(U.LISTS), buf, nb, off, ln, None, U.N_LANES)[0]
    return U.model(buf, nb, off, ln, meta, mtu=1500, **kw)


def _open_payloads(bt):
    buf, nb, off, ln, kinds = bt
    return [bytes(buf[int(o) + 42:int(o) + int(l)]) for o, l, k in zip(off, ln, kinds) if k == "udp_open"]


def _recv_all(api, s):
    got = []
    abi.lib().udpdk_interrupt(0)                      # an empty ring answers EINTR instead of blocking
    while True:
        n, pay, _ = api.recvfrom(s)
        if n < 0:
            assert api.errno() == errno.EINTR
            return got
        got.append(pay)


def _counts(api):
    c = api.icmp_counts()
    return (c.echo_replied, c.unreach_sent, c.echo_bad, c.limited, c.queue_dropped)


def test_flags_off_changes_nothing(api):
    bt = U.mixed(41, 300)
    assert api.config_icmp(-1) == 0 and api.config_icmp_burst(-2) == 64
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NO_BIND] > 10 and st.counters[abi.V_NOT_UDP] > 10
    assert api.tx_pending() == 0 and api.tx_drain() == [] and _counts(api) == (0, 0, 0, 0, 0)
    assert _recv_all(api, 0) == _open_payloads(bt) and _recv_all(api, 1) == []


@pytest.mark.parametrize("api", ["icmp = all\n", "icmp = echo, unreach\nicmp_burst = 7\n"], indirect=True)
def test_flags_on_replies_drain_first(api):
    burst = api.config_icmp_burst(-2)
    assert api.config_icmp(-1) == U.ALL and burst in (64, 7)
    bt = U.mixed(42, 400)
    R = _model(bt, err_limit=burst)
    U.assert_mixed_counts(_model(bt), 10)
    assert R.stats["limited"] > 0 if burst == 7 else R.stats["limited"] == 0
    rc, st = _poll(bt)
    assert rc == 0
    k = R.stats["replies"]
    assert api.tx_pending() == k > 20
    assert api.sendto(0, b"after the answers", "10.1.2.3", 4000) == 17
    assert api.tx_pending() == k + 1
    assert _counts(api) == (R.stats["echo_replied"], R.stats["unreach_sent"], R.stats["echo_bad"], R.stats["limited"], 0)
    got = api.tx_drain()
    assert len(got) == k + 1 and got[:k] == R.frames_out
    assert got[k][23] == 17 and got[k][42:] == b"after the answers"
    assert api.tx_pending() == 0 and api.tx_drain() == []
    # the sockets got exactly the open-port datagrams
    assert _recv_all(api, 0) == _open_payloads(bt) and _recv_all(api, 1) == []
    # one flag alone, set at run time
    assert api.config_icmp(U.ECHO) == U.ALL and api.config_icmp(4) == -1 and api.errno() == errno.EINVAL
    assert _poll(bt)[0] == 0
    E = _model(bt, flags=U.ECHO)
    assert api.tx_drain() == E.frames_out and E.stats["unreach_sent"] == 0


def _long_batch(n):
    rng = np.random.default_rng(43)
    fl = [U.echo_request(rng, 1000) if j % 3 == 0 else U.udp_frame(rng, U.CLOSED_PORT, payload_len=1400)
          for j in range(n)]
    return U.pack(fl)


@pytest.mark.parametrize("api", ["icmp = all\nicmp_burst = 1200\npoll_chunk_mb = 1\npoll_chunk_min_avg = 0\n"], indirect=True)
def test_burst_counts_across_a_chunked_poll(api):
    bt = _long_batch(3000)                                  # 3.9 MB: three chunks of about 1000 frames
    assert bt[1] > 3 << 20
    R = _model(bt, err_limit=1200)
    assert R.stats["unreach_sent"] == 1200 and R.stats["limited"] == 800 and R.stats["echo_replied"] == 1000
    last_err = max(i for i, r in enumerate(R.reason) if r == "unreach")
    assert last_err > 1500                                  # the limit ends in the second chunk
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NO_BIND] == 2000
    assert _counts(api) == (1000, 1200, 0, 800, 0) and api.tx_pending() == 2200
    assert api.tx_drain() == R.frames_out                   # arrival order across the chunks


@pytest.mark.parametrize("api", ["icmp = all\n"], indirect=True)
def test_drain_limits_leave_frames_queued(api):
    rng = np.random.default_rng(44)
    bt = U.pack([U.echo_request(rng, 100 + 50 * j) for j in range(6)])
    R = _model(bt)
    assert _poll(bt)[0] == 0 and api.tx_pending() == 6
    assert api.sendto(0, b"x" * 10, "10.1.2.3", 4000) == 10
    assert api.tx_drain(max_frames=2) == R.frames_out[:2] and api.tx_pending() == 5
    assert api.tx_drain(cap=len(R.frames_out[2]) - 1) == [] and api.tx_pending() == 5
    # room for two more, not for the third: the datagram waits behind the queued frames
    assert api.tx_drain(cap=len(R.frames_out[2]) + len(R.frames_out[3]) + 60) == R.frames_out[2:4]
    assert api.tx_pending() == 3
    got = api.tx_drain()
    assert got[:2] == R.frames_out[4:] and len(got) == 3 and got[2][42:] == b"x" * 10
    assert api.tx_pending() == 0


@pytest.mark.parametrize("api", ["icmp = echo\n"], indirect=True)
def test_queue_overflow_is_counted(api):
    rng = np.random.default_rng(45)
    n = 4096 + 300
    bt = U.pack([U.echo_request(rng, 8 + j % 40) for j in range(n)])
    R = _model(bt, flags=U.ECHO)
    assert _poll(bt)[0] == 0
    assert _counts(api) == (n, 0, 0, 0, 300) and api.tx_pending() == 4096
    assert api.tx_drain(max_frames=8192) == R.frames_out[:4096]


@pytest.mark.parametrize("api", ["icmp = all\n"], indirect=True)
def test_reset_empties_the_queue(api):
    rng = np.random.default_rng(46)
    bt = U.pack([U.echo_request(rng, 64) for _ in range(5)])
    assert _poll(bt)[0] == 0 and api.tx_pending() == 5 and _counts(api)[0] == 5
    api.reset()
    assert api.tx_pending() == 0 and _counts(api) == (0, 0, 0, 0, 0) and api.config_icmp(-1) == 0
    assert api.config_icmp_burst(-2) == 64


def test_sharded_context_refuses(tmp_path, host_api):
    L = abi.lib()
    assert _init(tmp_path, "devices = 0,0\nicmp = all\n") == -1 and host_api.errno() == errno.EINVAL
    assert L.udpdk_gpu_context() is None
    assert _init(tmp_path, "devices = 0,0\n") == 0
    try:
        assert host_api.config_icmp(U.ALL) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_icmp(0) == 0 and host_api.config_icmp(-1) == 0
    finally:
        L.udpdk_cleanup()


@pytest.mark.parametrize("api", ["icmp = all\n"], indirect=True)
def test_poller_thread_over_loopback_runs_to_quiescence(api):
    """The loopback port with the poller thread: datagrams to a closed port are answered, the answers
    come back as ICMP type 3 and nothing answers those. A datagram to the open port, sent and received,
    is the barrier: the poller has polled everything sent before it."""
    L = abi.lib()
    ops = abi.PortOps()
    assert L.udpdk_port_loopback(C.byref(ops)) == 0
    ops.batch_frames = 512
    a = api.socket()
    assert api.bind(a, "0.0.0.0", 10000) == 0
    assert L.udpdk_port_attach(C.byref(ops)) == 0
    watchdog = threading.Timer(60.0, L.udpdk_interrupt, [0])    # a hang ends as EINTR
    watchdog.start()

    def barrier(tag):
        assert api.sendto(a, tag, U.OUR_IP, 10001) == len(tag)
        n, data, addr = api.recvfrom(0, 2048)
        assert data == tag and addr == (U.OUR_IP, 10000)
    try:
        for k in range(10):
            assert api.sendto(a, b"nobody home %d" % k, U.OUR_IP, U.CLOSED_PORT) > 0
        barrier(b"one")                                          # the ten were polled: errors queued
        for tag in (b"two", b"three", b"four"):                  # drained, looped back, polled
            barrier(tag)
        assert _counts(api) == (0, 10, 0, 0, 0)
        for tag in (b"five", b"six"):
            barrier(tag)
        assert _counts(api) == (0, 10, 0, 0, 0) and api.tx_pending() == 0
    finally:
        watchdog.cancel()
        assert L.udpdk_port_detach() == 0
