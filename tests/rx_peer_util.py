"""The numpy model of the RX peer filter (udpdk_gpu_rx_peer_select / udpdk_gpu_rx_peer), for
test_rx_peer_ref.py (where it is pinned against the oracle), test_gpu_rx_peer.py and
test_gpu_connect_path.py, and small builders for peer tables and batches with chosen sources.

The rule, for entry p of lane l with frame i = lane_pkt[p], D = min(lane_off[-1], lane_cap):
    i >= n                                   removed, bad_index
    peers[l].on == 0                         kept
    length[i] < 42 or offset[i] + length[i] > frames_bytes
                                             removed, bad_frame
    u32 at frame bytes 26-29 == peers[l].ip and u16 at bytes 34-35 == peers[l].port
                                             kept, else removed: refused
    new_pkt = lane_pkt[keep];  new_off = concat([0], cumsum(keep))[min(lane_off, D)]
"""
from dataclasses import dataclass

import numpy as np

import rx_balance_util as B
from udpdk_amd import abi

PEER_DTYPE = abi.PEER_DTYPE


def peer_table(n_lanes, conn):
    """conn: {lane: (ip string or raw u32, port in host order)} -> records[n_lanes]."""
    t = np.zeros(n_lanes, PEER_DTYPE)
    for l, (ip, port) in conn.items():
        t[l] = (abi.raw_ip(ip) if isinstance(ip, str) else ip, abi.raw_port(port), 1)
    return t


def src_fields(b, idx):
    """(raw u32 at frame bytes 26-29, raw u16 at bytes 34-35) of the frames idx (all in range)."""
    f = np.asarray(b.frames, np.uint8)
    o = np.asarray(b.offset, np.uint32)[idx].astype(np.int64)
    ip = (f[o + 26].astype(np.uint32) | f[o + 27].astype(np.uint32) << 8 | f[o + 28].astype(np.uint32) << 16 |
          f[o + 29].astype(np.uint32) << 24)
    port = f[o + 34].astype(np.uint16) | f[o + 35].astype(np.uint16) << 8
    return ip, port


@dataclass
class Peered:
    lane_off: np.ndarray
    lane_pkt: np.ndarray
    kept: int
    removed: int
    refused: int
    bad_frame: int
    bad_index: int
    truncated: int
    keep: np.ndarray           # bool per input entry [D]

    def stats(self):
        return (self.kept, self.removed, self.refused, self.bad_frame, self.bad_index, self.truncated)


def stats_tuple(st):
    """The same tuple from an abi.RxPeerStats."""
    return (st.kept, st.removed, st.refused, st.bad_frame, st.bad_index, st.truncated)


def model(b, lane_off, lane_pkt, peers, n=None, lane_cap=None, frames_bytes=None) -> Peered:
    lane_off = np.asarray(lane_off, np.uint32).astype(np.int64)
    peers = np.asarray(peers, PEER_DTYPE)
    n_lanes = len(lane_off) - 1
    assert len(peers) >= n_lanes
    n = len(b.offset) if n is None else n
    fb = int(b.frames_bytes) if frames_bytes is None else frames_bytes
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    d = int(min(lane_off[-1], lane_cap))
    pkt = np.asarray(lane_pkt, np.uint32)[:d]
    off_c = np.minimum(lane_off, d)
    lane_of = np.searchsorted(off_c[1:], np.arange(d), side="right")     # largest l with off[l] <= p
    lane_of = np.minimum(lane_of, n_lanes - 1)
    valid = pkt < n
    conn = valid & (peers["on"][lane_of] != 0)
    ok = np.zeros(d, bool)
    ci = np.flatnonzero(conn)
    o = np.asarray(b.offset, np.uint32)[pkt[ci]].astype(np.int64)
    ln = np.asarray(b.length, np.uint16)[pkt[ci]].astype(np.int64)
    ok[ci] = (ln >= 42) & (o + ln <= fb)
    match = np.zeros(d, bool)
    oi = np.flatnonzero(ok)
    ip, port = src_fields(b, pkt[oi])
    match[oi] = (ip == peers["ip"][lane_of[oi]]) & (port == peers["port"][lane_of[oi]])
    keep = valid & (~conn | match)
    pre = np.concatenate([[0], np.cumsum(keep)])
    kept = int(keep.sum())
    return Peered(pre[off_c].astype(np.uint32), pkt[keep], kept, d - kept, int((ok & ~match).sum()),
                  int((conn & ~ok).sum()), int((~valid).sum()), int(lane_off[-1] > lane_cap), keep)


# ---- batches -------------------------------------------------------------------------------------
PEER = ("10.1.2.3", 7000)                                 # the peer the tests connect to
# one source per way an entry can differ from PEER: in the address only, in the port only, in both.
# (The fourth pattern of the tests is the second source sent TO port 7000: the peer's port is then
# the frame's destination port, two bytes further on, and must not match.)
STRANGERS = [("10.1.2.4", 7000), ("10.1.2.3", 7001), ("10.9.9.9", 9)]


def frames_from(sources, dports, seed, payload_len=22, gaps=None, tail=64, dst="172.31.100.1", payload=None):
    """One valid frame per (ip string, host port) source in `sources` to dports[i] (B.flow_frames)."""
    src = np.array([B.ip_bytes(ip) for ip, _ in sources], np.uint8).reshape(len(sources), 4)
    sport = np.array([p for _, p in sources], np.int64)
    dstb = np.tile(np.array(B.ip_bytes(dst), np.uint8), (len(sources), 1))
    return B.flow_frames(src, sport, dstb, np.asarray(dports, np.int64), seed, payload_len=payload_len,
                         gaps=gaps, tail=tail, payload=payload)


def single_lanes(n_lanes, counts, order=None):
    """A lane set of sum(counts) entries, frames 0.. in lane order (or `order`): (lane_off, lane_pkt)."""
    counts = np.asarray(counts, np.int64)
    assert len(counts) == n_lanes
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    pkt = np.arange(int(off[-1]), dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    return off, pkt

