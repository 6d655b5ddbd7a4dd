"""ARP through the socket layer: udpdk_poll_rx with [gpu] arp = 1 answers the requests for the stack's
address on the GPU and queues the replies; udpdk_tx_drain emits them first, ahead of the poll's ICMP
answers and the socket datagrams. Socket 0 is bound ANY:10001; the stack's own address is 172.31.100.1.
The expected frames are the model's (tests/arp_util.py)."""
import ctypes as C
import errno
import threading

import numpy as np
import pytest

import arp_util as U
import icmp_util as IU
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

ZERO = {k: 0 for k, _ in abi.ArpCounts._fields_}


def _mac(b):
    return ":".join(f"{x:02x}" for x in b)


def _init(tmp_path, extra=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {_mac(U.OUR_MAC)}\nip_addr = {U.OUR_IP}\n[port0_dst]\n"
                   f"mac_addr = {_mac(U.PEER_MAC)}\n[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n"
                   "frag_buckets = 64\nfrag_bucket_entries = 16\nfrag_max_dgram = 16384\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


@pytest.fixture()
def api(tmp_path, host_api, request):
    assert _init(tmp_path, getattr(request, "param", "")) == 0
    s0 = host_api.socket()
    assert host_api.bind(s0, "0.0.0.0", 10001) == 0
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
    return U.model(buf, nb, off, ln, U.host_meta(buf, off, ln), **kw)


def _counts(api) -> dict:
    c = api.arp_counts()
    return {k: int(getattr(c, k)) for k, _ in abi.ArpCounts._fields_}


def _want_counts(R, scanned=1, **kw) -> dict:
    return dict({k: R["stats"][k] for k in U.STAT_FIELDS if k != "bad_frame"}, scanned=scanned, announced=0, **kw)


def _recv_all(api, s):
    got = []
    abi.lib().udpdk_interrupt(0)                      # an empty ring answers EINTR instead of blocking
    while True:
        n, pay, _ = api.recvfrom(s)
        if n < 0:
            assert api.errno() == errno.EINTR
            return got
        got.append(pay)


def _mixed_poll(seed=7, n=300):
    """UDP to the bound socket, ARP frames of every kind, and one echo request in the middle."""
    rng = np.random.default_rng(seed)
    names = list(U.KINDS)
    kinds = [names[k] for k in rng.integers(0, len(names), n)]
    fl = [U.kind_frame(rng, k) for k in kinds]
    echo_at = n // 2
    fl[echo_at], kinds[echo_at] = IU.echo_request(rng, 64), "echo"
    bt = U.pack(fl, aligns=rng.integers(0, 16, n).tolist())
    pays = [f[42:] for f, k in zip(fl, kinds) if k == "udp"]
    echo = IU.model(bt[0], bt[1], bt[2][echo_at:echo_at + 1], bt[3][echo_at:echo_at + 1],
                    np.array([abi.V_NOT_UDP | 0x10], np.uint32), flags=IU.ECHO, mtu=1500).frames_out
    assert len(echo) == 1 and len(pays) > 3
    return bt, pays, echo[0]


@pytest.mark.parametrize("api", ["arp = 1\nicmp = echo\n"], indirect=True)
def test_switch_on_replies_drain_first(api):
    assert api.config_arp(-1) == 1
    bt, pays, echo = _mixed_poll()
    R = _model(bt)
    k = R["stats"]["replies"]
    assert k > 20 and R["stats"]["no_room"] == 0
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NOT_IPV4] > k
    assert api.tx_pending() == k + 1
    assert api.sendto(0, b"after the answers", "10.1.2.3", 4000) == 17
    assert _counts(api) == _want_counts(R)
    got = api.tx_drain()
    assert len(got) == k + 2
    assert all(len(f) == 42 for f in got[:k]) and got[:k] == R["frames_out"]      # arrival order
    assert got[k] == echo                                                          # then the ICMP answer
    assert got[k + 1][23] == 17 and got[k + 1][42:] == b"after the answers"        # then the datagrams
    assert api.tx_pending() == 0 and api.tx_drain() == []
    assert _recv_all(api, 0) == pays
    assert api.icmp_counts().queue_dropped == 0


@pytest.mark.parametrize("api", ["icmp = echo\n"], indirect=True)
def test_switch_off_changes_nothing(api):
    assert api.config_arp(-1) == 0
    bt, pays, echo = _mixed_poll()
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NOT_IPV4] > 20
    assert api.tx_pending() == 1 and api.tx_drain() == [echo] and _counts(api) == ZERO
    assert _recv_all(api, 0) == pays                               # the ring holds the same with the switch on (above)
    # set at run time
    assert api.config_arp(1) == 0
    assert _poll(bt)[0] == 0
    R = _model(bt)
    assert api.tx_drain() == R["frames_out"] + [echo] and _counts(api) == _want_counts(R)


@pytest.mark.parametrize("api", ["arp = 1\n"], indirect=True)
def test_pure_udp_poll_does_not_run_the_stage(api):
    rng = np.random.default_rng(3)
    bt = U.pack([U.udp_frame(rng, payload_len=20) for _ in range(200)])
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NOT_IPV4] == 0 and st.counters[abi.V_DELIVERED] == 200
    assert _counts(api) == ZERO and api.tx_pending() == 0
    one = U.pack([U.arp_frame()])
    assert _poll(one)[0] == 0 and _counts(api)["scanned"] == 1 and api.tx_pending() == 1
    assert _poll(bt)[0] == 0 and _counts(api)["scanned"] == 1


@pytest.mark.parametrize("api", ["arp = 1\npoll_chunk_mb = 1\npoll_chunk_min_avg = 0\n"], indirect=True)
def test_chunked_poll_queues_in_chunk_order(api):
    rng = np.random.default_rng(43)
    n = 3000                                                # 4.3 MB: chunks of about 700 frames
    fl = [U.udp_frame(rng, 7, payload_len=1400) for _ in range(n)]
    at = list(range(5, n, 97))
    for j, p in enumerate(at):
        kind = ("request", "request_pad", "tpa_other", "op_reply", "conflict")[j % 5]
        fl[p] = U.kind_frame(rng, kind)
    bt = U.pack(fl)
    assert bt[1] > 4 << 20
    R = _model(bt)
    k = R["stats"]["replies"]
    assert k >= 12 and int(R["origin"][0]) < 700 and int(R["origin"][-1]) > 2300      # requests in the first and last chunk
    rc, st = _poll(bt)
    assert rc == 0 and st.counters[abi.V_NOT_IPV4] == len(at)
    c = _counts(api)
    assert 2 <= c["scanned"] <= 8
    assert c == _want_counts(R, scanned=c["scanned"])              # the counts sum over the chunks
    assert api.tx_drain() == R["frames_out"]                       # arrival order across the chunks


@pytest.mark.parametrize("api", ["arp = 1\n"], indirect=True)
def test_more_replies_than_the_first_copy(api):
    rng = np.random.default_rng(47)
    for n in (32, 33, 100):
        fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng), pad_to=60 * (j % 2)) for j in range(n)]
        bt = U.pack(fl, aligns=rng.integers(0, 16, n).tolist())
        R = _model(bt)
        assert R["stats"]["replies"] == n
        assert _poll(bt)[0] == 0 and api.tx_pending() == n
        assert api.tx_drain() == R["frames_out"]


@pytest.mark.parametrize("api", ["arp = 1\n"], indirect=True)
def test_more_requests_than_the_queue_holds(api):
    rng = np.random.default_rng(45)
    n = 4096 + 300
    bt = U.pack([U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) for _ in range(n)])
    R = _model(bt, max_replies=4096)
    assert R["stats"]["no_room"] == 300
    assert _poll(bt)[0] == 0
    assert _counts(api) == _want_counts(R) and api.tx_pending() == 4096
    assert api.icmp_counts().queue_dropped == 0
    assert api.tx_drain(max_frames=8192) == R["frames_out"][:4096]
    # a queue that already holds frames drops what does not fit, and counts it
    assert _poll(bt)[0] == 0 and api.tx_pending() == 4096
    small = U.pack([U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) for _ in range(10)])
    assert _poll(small)[0] == 0 and api.tx_pending() == 4096
    assert api.icmp_counts().queue_dropped == 10 and _counts(api)["replies"] == 2 * 4096 + 10


@pytest.mark.parametrize("api", ["arp = 1\n"], indirect=True)
def test_poll_echo_answers_no_arp(api):
    rng = np.random.default_rng(49)
    fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) if j % 2 else U.udp_frame(rng, payload_len=30)
          for j in range(40)]
    buf, nb, off, ln = U.pack(fl)
    flat = np.concatenate([buf, np.zeros(256, np.uint8)])
    rc, err, frames, st, n_out = api.poll_echo(flat, nb, off, ln)
    assert rc == 0 and n_out == 20 and all(f[12:14] == b"\x08\x00" for f in frames)
    assert st.counters[abi.V_NOT_IPV4] == 20
    assert _counts(api) == ZERO and api.tx_pending() == 0


def test_sharded_context_refuses(tmp_path, host_api):
    L = abi.lib()
    assert _init(tmp_path, "devices = 0,0\narp = 1\n") == -1 and host_api.errno() == errno.EINVAL
    assert L.udpdk_gpu_context() is None
    assert _init(tmp_path, "devices = 0,0\n") == 0
    try:
        assert host_api.config_arp(1) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_arp(0) == 0 and host_api.config_arp(-1) == 0
    finally:
        L.udpdk_cleanup()


@pytest.mark.parametrize("api", ["arp = 1\narp_announce = 1\n"], indirect=True)
def test_poller_thread_over_loopback_runs_to_quiescence(api):
    """The loopback port with the poller thread: the announcement udpdk_init queued is drained, comes
    back and is counted `own`; nothing answers it. A datagram to the open port, sent and received, is
    the barrier: the poller has polled everything sent before it."""
    L = abi.lib()
    assert api.tx_pending() == 1 and _counts(api) == dict(ZERO, announced=1)
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
        for tag in (b"one", b"two", b"three", b"four"):          # drained, looped back, polled
            barrier(tag)
        c = _counts(api)
        assert c == dict(ZERO, announced=1, scanned=1, arp=1, own=1) and api.tx_pending() == 0
        for tag in (b"five", b"six"):
            barrier(tag)
        assert _counts(api) == c and api.tx_pending() == 0
    finally:
        watchdog.cancel()
        assert L.udpdk_port_detach() == 0
