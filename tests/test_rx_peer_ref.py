"""The peer filter model (rx_peer_util.py) pinned against the oracle, which the GPU tests
(test_gpu_rx_peer.py, test_gpu_connect_path.py) then use as their reference, and the model's
invariants. No GPU needed."""
import subprocess

import numpy as np
import pytest

import oracle as O
import rx_balance_util as B
import rx_drop_util as D
import rx_peer_util as U
from test_gpu_rx import IP1, IP9, MIXED_LISTS
from udpdk_amd import abi, frames as F

N_LANES = 8


def mixed_sources(seed, n=3000):
    """The mixed edge-case batch with a third of the frames' sources rewritten to the peer's or one
    of the strangers' (their checksums then fail, which the drop model sees), and its oracle lanes."""
    b = F.mixed_batch(seed, n, [10001, 10002, 10003, 10004, 10005], [9, 20000, 65535], [IP1, IP9])
    rng = np.random.default_rng(seed + 77)
    srcs = [U.PEER] + U.STRANGERS
    for i in np.flatnonzero(b.length >= 42):
        k = int(rng.integers(0, 3 * len(srcs)))
        if k >= len(srcs):
            continue
        o = int(b.offset[i])
        b.frames[o + 26:o + 30] = B.ip_bytes(srcs[k][0])
        b.frames[o + 34], b.frames[o + 35] = srcs[k][1] >> 8, srcs[k][1] & 0xFF
    bt = O.bindtable_from_lists(MIXED_LISTS)
    meta, loff, lpkt, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset, b.length, None, N_LANES)
    return b, bt, meta, loff, lpkt


def test_source_fields_equal_oracle_recv_gather():
    """What the model compares is what recvfrom reports as the source, at every offset & 3."""
    n = 64
    srcs = [(f"10.{k}.{2 * k}.{255 - k}", 1 + 1021 * k) for k in range(n)]
    gaps = [(k * 7 + 1) % 4 + (3 if k == 0 else 0) for k in range(n)]
    b = U.frames_from(srcs, np.full(n, 10001), 5, gaps=gaps)
    assert set(int(o) & 3 for o in b.offset) == {0, 1, 2, 3}
    lpkt = np.random.default_rng(1).permutation(n).astype(np.uint32)
    _, _, sip, spt = O.recv_gather(b.frames, b.offset, b.length, lpkt, 0, n, 64)
    ip, port = U.src_fields(b, lpkt)
    assert np.array_equal(ip, sip) and np.array_equal(port, spt)
    assert ip[0] == abi.raw_ip(srcs[lpkt[0]][0]) and port[0] == abi.raw_port(srcs[lpkt[0]][1])


@pytest.mark.parametrize("seed", [1, 2])
def test_model_equals_oracle_without_refused_frames(seed):
    """No fan-out, one connected socket: filtering its lane is receiving a batch from which the
    frames it refuses were taken out."""
    lists = {abi.raw_port(10001): [(0, 0, 0)], abi.raw_port(10002): [(0, 1, 0)], abi.raw_port(10003): [(0, 2, 0)]}
    rng = np.random.default_rng(seed)
    n = 2000
    all_src = [U.PEER] + U.STRANGERS
    srcs = [all_src[int(k)] for k in rng.integers(0, len(all_src), n)]
    dports = rng.choice([10001, 10002, 10003, 10009], n)
    b = U.frames_from(srcs, dports, seed, gaps=rng.integers(0, 4, n))
    bt = O.bindtable_from_lists(lists)
    meta, loff, lpkt, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset, b.length, None, 4)
    peers = U.peer_table(4, {1: U.PEER})
    m = U.model(b, loff, lpkt, peers)
    lane1 = lpkt[loff[1]:loff[2]]
    refused = np.array([i for i in lane1 if srcs[i] != U.PEER], np.int64)
    assert len(refused) > 100 and m.refused == len(refused) == m.removed
    assert (m.bad_frame, m.bad_index, m.truncated) == (0, 0, 0)
    keep = np.setdiff1d(np.arange(n), refused)
    _, loff2, lpkt2, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset[keep], b.length[keep], None, 4)
    assert np.array_equal(m.lane_off, loff2)
    assert np.array_equal(m.lane_pkt, keep[lpkt2])
    # and the connected lane holds the peer's frames only, in arrival order
    got1 = m.lane_pkt[m.lane_off[1]:m.lane_off[2]]
    assert [srcs[i] for i in got1] == [U.PEER] * len(got1) and np.all(np.diff(got1.astype(np.int64)) > 0)


def test_model_identity_and_idempotent():
    b, _, _, loff, lpkt = mixed_sources(3)
    ident = U.model(b, loff, lpkt, U.peer_table(N_LANES, {}))
    assert np.array_equal(ident.lane_off, loff) and np.array_equal(ident.lane_pkt, lpkt)
    assert ident.stats() == (len(lpkt), 0, 0, 0, 0, 0)
    peers = U.peer_table(N_LANES, {0: U.PEER, 2: U.PEER, 4: U.STRANGERS[0]})
    m = U.model(b, loff, lpkt, peers)
    assert m.refused > 100 and m.kept > 100
    again = U.model(b, m.lane_off, m.lane_pkt, peers)
    assert np.array_equal(again.lane_off, m.lane_off) and np.array_equal(again.lane_pkt, m.lane_pkt)
    assert again.removed == 0
    # fan-out (port 10002: lanes 1 and 2): the unconnected lane keeps every frame
    assert np.array_equal(m.lane_pkt[m.lane_off[1]:m.lane_off[2]], lpkt[loff[1]:loff[2]])
    assert m.lane_off[3] - m.lane_off[2] < loff[3] - loff[2]


@pytest.mark.parametrize("flags", [D.DROP_UDP, D.DROP_ALL])
def test_model_commutes_with_drop(flags):
    b, _, meta, loff, lpkt = mixed_sources(4)
    peers = U.peer_table(N_LANES, {0: U.PEER, 1: U.PEER, 5: U.STRANGERS[1]})
    d = D.model(meta, loff, lpkt, flags)
    a = U.model(b, d.lane_off, d.lane_pkt, peers)
    p = U.model(b, loff, lpkt, peers)
    c = D.model(meta, p.lane_off, p.lane_pkt, flags)
    assert d.removed > 50 and p.removed > 50 and a.removed > 0 and c.removed > 0
    assert np.array_equal(a.lane_off, c.lane_off) and np.array_equal(a.lane_pkt, c.lane_pkt)


def test_model_commutes_with_balance():
    b, bt, meta, loff, lpkt = mixed_sources(5)
    rp = np.array([0, 1, 1, 0, 1, 1, 0, 1], np.uint8)          # lanes 1, 2 (port 10002) and 4, 5 (10004)
    peers = U.peer_table(N_LANES, {0: U.PEER, 1: U.PEER, 4: U.STRANGERS[0]})
    x = B.model(bt.port_list, b, meta, loff, lpkt, rp)
    a = U.model(b, x.lane_off, x.lane_pkt, peers)
    p = U.model(b, loff, lpkt, peers)
    c = B.model(bt.port_list, b, meta, p.lane_off, p.lane_pkt, rp)
    assert x.removed > 50 and p.removed > 50 and a.removed > 0 and c.removed > 0
    assert np.array_equal(a.lane_off, c.lane_off) and np.array_equal(a.lane_pkt, c.lane_pkt)
    # the hash may pick a member connected to somebody else: that delivery is gone from both
    lost = 0
    # (group 4, 5 on port 10004, lane 4 connected to a source few frames have)
    for i in np.flatnonzero(x.chosen == 4):
        if i not in a.lane_pkt[a.lane_off[4]:a.lane_off[5]]:
            assert i in lpkt[loff[5]:loff[6]] and i not in a.lane_pkt[a.lane_off[5]:a.lane_off[6]]
            lost += 1
    assert lost > 50


def test_model_bounds():
    srcs = [U.PEER] * 6
    b = U.frames_from(srcs, np.full(6, 10001), 9)
    b.length[2] = 41                                       # too short to hold the ports' header
    fb = int(b.offset[5]) + 63                             # the last frame ends a byte past the batch
    off, pkt = U.single_lanes(2, [4, 5], order=[0, 1, 2, 9, 3, 4, 5, 2, 6])
    m = U.model(b, off, pkt, U.peer_table(2, {1: U.PEER}), frames_bytes=fb)
    assert list(m.lane_pkt) == [0, 1, 2, 3, 4] and list(m.lane_off) == [0, 3, 5]
    assert m.stats() == (5, 4, 0, 2, 2, 0)                 # lane 0 keeps the short frame: nothing of it is read
    t = U.model(b, off, pkt, U.peer_table(2, {1: U.PEER}), lane_cap=5, frames_bytes=fb)
    assert list(t.lane_pkt) == [0, 1, 2, 3] and list(t.lane_off) == [0, 3, 4] and t.truncated == 1


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("udpdk_gpu_rx_peer_select", "udpdk_gpu_rx_peer", "udpdk_gpu_rx_peer_stats",
                 "udpdk_gpu_rx_peer_removed", "udpdk_connect", "udpdk_send", "udpdk_recv", "udpdk_getpeername",
                 "udpdk_getsockname", "udpdk_rx_refused", "udpdk_peer_lanes"):
        assert name in exported and name in abi.declared_symbols(), name
    assert abi.lib().udpdk_gpu_abi_version() == 3
