"""The reuse-port balance model (rx_balance_util.py) pinned against the oracle, which the GPU tests
(test_gpu_rx_balance.py) then use as their reference; the host-only entry points
(udpdk_gpu_rx_balance_rank, udpdk_reuseport_lanes, udpdk_config_reuseport, the ini key) and the
export map. No GPU needed."""
import ctypes as C
import errno
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
import rss_util as R
import rx_balance_util as U
from test_gpu_rx import IP1, IP9, MIXED_LISTS
from udpdk_amd import abi, frames as F

N_LANES = 8
SEED_FLOWS = 0xBA1A       # 4096 flows on an 8-member group: every member gets one (checked below)


def mixed(seed, n=3000):
    return F.mixed_batch(seed, n, [10001, 10002, 10003, 10004, 10005], [9, 20000, 65535], [IP1, IP9])


def lanes_as_deliveries(n, loff, lpkt):
    """Per frame, the sorted lanes its entries are in."""
    out = [[] for _ in range(n)]
    lane_of = np.repeat(np.arange(len(loff) - 1), np.diff(loff.astype(np.int64)))
    for l, i in zip(lane_of, lpkt):
        out[i].append(int(l))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_walk_equals_oracle_lanes(seed):
    b = mixed(seed)
    bt = O.bindtable_from_lists(MIXED_LISTS)
    meta, loff, lpkt, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset, b.length, None, N_LANES)
    _, dels, _ = U.choose(bt.port_list, b, meta, np.zeros(N_LANES, np.uint8), np.zeros(b.n, np.uint32))
    got = lanes_as_deliveries(b.n, loff, lpkt)
    multi = 0
    for i in range(b.n):
        assert sorted(dels[i]) == got[i], i
        if dels[i]:
            assert dels[i][0] == int(abi.meta_sockfd(meta[i])), i
            assert min(len(dels[i]), 127) == int(abi.meta_fanout(meta[i])), i
            multi += len(dels[i]) > 1
    assert multi > 100


def test_walk_equals_probes():
    """The fan-out probes of tests/golden/rx_probes.json: order and end of the walk."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rx_probes.json")
    rng = np.random.default_rng(0)
    seen = 0
    for p in json.load(open(here))["frames"]:
        if "binds" not in p or "expect_deliveries" not in p:
            continue
        bt = O.BindTable()
        for s, ip, opts in p["binds"]:
            assert bt.add(s, abi.raw_ip(ip), abi.raw_port(10001), opts) == 0
        f = F.make_frame(rng, dport=10001, dst_ip=p.get("dst_ip", "172.31.100.1"))
        b = SimpleNamespace(frames=np.frombuffer(f, np.uint8), offset=np.array([0]), n=1)
        assert U.walk(bt.port_list, *U.frame_key(b, 0)) == p["expect_deliveries"], p["id"]
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("types", [3, 2, 1, 0])
def test_model_hash_equals_oracle_rss(types):
    b = mixed(5, 1500)
    key = R.random_keys(1, 99)[0]
    want = O.rss(key, types, [0], 1, b.frames, b.frames_bytes, b.offset, b.length)[0]
    assert np.array_equal(U.frame_hashes(b, key, types), want)
    assert (want != 0).any() == (types != 0)


def test_model_invariants():
    b = mixed(7)
    bt = O.bindtable_from_lists(MIXED_LISTS)
    meta, loff, lpkt, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset, b.length, None, N_LANES)
    ident = U.model(bt.port_list, b, meta, loff, lpkt, np.zeros(N_LANES, np.uint8))
    assert np.array_equal(ident.lane_off, loff) and np.array_equal(ident.lane_pkt, lpkt)
    assert (ident.removed, ident.balanced, ident.bad_index) == (0, 0, 0)
    rp = np.array([0, 1, 1, 0, 1, 1, 0, 1], np.uint8)          # lanes 1, 2 (port 10002) and 4, 5 (10004)
    m = U.model(bt.port_list, b, meta, loff, lpkt, rp)
    before, after = lanes_as_deliveries(b.n, loff, lpkt), lanes_as_deliveries(b.n, m.lane_off, m.lane_pkt)
    two = 0
    for i in range(b.n):
        flagged = [l for l in before[i] if rp[l]]
        assert [l for l in after[i] if not rp[l]] == [l for l in before[i] if not rp[l]], i
        left = [l for l in after[i] if rp[l]]
        if len(flagged) >= 2:
            assert left == [int(m.chosen[i])] and left[0] in flagged, i
            two += 1
        else:
            assert left == flagged and m.chosen[i] == U.KEEP_ALL, i
    assert two > 100 and m.balanced == two and m.removed == two
    # arrival order inside each lane is kept
    for l in range(N_LANES):
        assert np.all(np.diff(m.lane_pkt[m.lane_off[l]:m.lane_off[l + 1]].astype(np.int64)) > 0)


def eight_group_batches():
    src, sport = U.random_flows(4096, SEED_FLOWS)
    dst = np.tile(np.array(U.ip_bytes("172.31.100.1"), np.uint8), (4096, 1))
    return [U.flow_frames(src, sport, dst, np.full(4096, 10001), 100 + k, payload_len=22 + 2 * k) for k in range(2)]


def test_flows_stick_and_spread():
    """Equal 4-tuples choose equal sockets across batches (whatever else the frames hold), and
    the 4096 flows of the seed the GPU test uses reach every member of an 8-member group."""
    lists = U.reuse_lists(10001, 8)
    rp = np.ones(8, np.uint8)
    ch = []
    for b in eight_group_batches():
        meta = np.full(b.n, 8 << 9 | 0x30, np.uint32)          # DELIVERED, fan-out 8
        ch.append(U.choose(lists.get, b, meta, rp, U.frame_hashes(b))[0])
    assert np.array_equal(ch[0], ch[1])
    cnt = np.bincount(ch[0], minlength=8)
    assert len(cnt) == 8 and cnt.min() >= 1
    assert cnt.min() > 400 and cnt.max() < 640                # 512 expected per member


def test_rank_helper():
    for h in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        for g in (1, 2, 3, 127, 128, 4095):
            assert abi.rx_balance_rank(h, g) == (h * g) >> 32 == U.rank(h, g), (h, g)
            assert abi.rx_balance_rank(h, g) < g


def test_reuseport_lanes(host_api):
    rc, f = host_api.reuseport_lanes(8)
    assert rc == 0 and not f.any()
    s = [host_api.socket() for _ in range(6)]
    assert s == list(range(6))
    for k in (1, 2, 5):
        assert host_api.setsockopt(s[k], abi.SOL_SOCKET, abi.SO_REUSEPORT, 1) == 0
    assert host_api.setsockopt(s[3], abi.SOL_SOCKET, abi.SO_REUSEADDR, 1) == 0
    assert host_api.reuseport_lanes(8)[0] == 0                # nothing bound yet
    for k in (0, 1, 2, 3):
        assert host_api.bind(s[k], "10.0.0.7" if k else "10.0.0.8", 10001) == 0, k
    rc, f = host_api.reuseport_lanes(8)
    assert rc == 2 and list(f) == [0, 1, 1, 0, 0, 0, 0, 0]
    assert host_api.bind(s[5], "10.0.0.9", 10002) == 0
    assert list(host_api.reuseport_lanes(6)[1]) == [0, 1, 1, 0, 0, 1]
    rc, f = host_api.reuseport_lanes(2)                        # a short array: still counts all
    assert rc == 3 and list(f) == [0, 1]
    assert host_api.close(s[1]) == 0
    assert list(host_api.reuseport_lanes(6)[1]) == [0, 0, 1, 0, 0, 1]
    assert abi.lib().udpdk_reuseport_lanes(None, 4) == -errno.EINVAL
    host_api.reset()
    assert host_api.reuseport_lanes(8)[0] == 0


def test_config_reuseport_round_trips(host_api):
    assert host_api.config_reuseport(-1) == abi.REUSEPORT_FANOUT == 0
    assert host_api.config_reuseport(abi.REUSEPORT_BALANCE) == 0
    assert host_api.config_reuseport(-1) == 1
    assert host_api.config_reuseport(2) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_reuseport(-5) == 1
    assert host_api.config_reuseport(abi.REUSEPORT_FANOUT) == 1
    host_api.config_reuseport(1)
    host_api.reset()
    assert host_api.config_reuseport(-1) == 0 and host_api.rx_balanced() == 0


@pytest.mark.parametrize("value,want", [("balance", 1), ("fanout", 0), ("both", None)])
def test_ini_key(tmp_path, host_api, value, want):
    """[gpu] reuseport: read by udpdk_init before it needs a device (which it may not find here)."""
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.2\n"
                   "[port0_dst]\nmac_addr = 68:05:ca:95:fa:64\n[gpu]\nmax_frames = 4096\nmax_lanes = 16\n"
                   f"reuseport = {value}\n")
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    host_api.config_reuseport(1 if want == 0 else 0)
    try:
        rc = abi.lib().udpdk_init(3, argv)
        if want is None:
            assert rc == -1 and host_api.errno() == errno.EINVAL
        else:
            assert rc == 0 or host_api.errno() == errno.ENODEV
            assert host_api.config_reuseport(-1) == want
    finally:
        abi.lib().udpdk_cleanup()


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("udpdk_gpu_rx_balance_select", "udpdk_gpu_rx_balance", "udpdk_gpu_rx_balance_stats",
                 "udpdk_gpu_rx_balance_rank", "udpdk_config_reuseport", "udpdk_rx_balanced",
                 "udpdk_reuseport_lanes"):
        assert name in exported and name in abi.declared_symbols(), name
    assert abi.lib().udpdk_gpu_abi_version() == 3
