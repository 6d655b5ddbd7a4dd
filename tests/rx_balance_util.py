"""The numpy/python model of the reuse-port balance stage (udpdk_gpu_rx_balance_select /
udpdk_gpu_rx_balance), for test_rx_balance_ref.py (where it is pinned against the oracle) and
test_gpu_rx_balance.py, and a frame builder with one flow (source address and port) per frame.

The rule, per DELIVERED frame i (every other frame keeps whatever entries it has):
    walk     the bindings of the raw dst port (frame bytes 36-37) in list order; a binding matches
             when ip == raw dst address (bytes 30-33) or ip == 0; every match is a delivery to its
             sockfd; the first match without `reuse` ends the walk
    G        the deliveries whose sockfd is < n_lanes and flagged in lane_rp; g = len(G)
    keep all when g <= 1, dst == 255.255.255.255 or the first dst byte is 224-239
    else     chosen = G[(hash_i * g) >> 32]
    entry p of lane l, frame i = lane_pkt[p], goes iff i >= n, or lane_rp[l] and chosen_i is a lane != l
    new_pkt = lane_pkt[keep];  new_off = concat([0], cumsum(keep))[min(lane_off, D)]
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import rss_util as R

KEEP_ALL = 0xFFFFFFFF
V_DELIVERED = 0
MAC = bytes.fromhex("6805ca95f8ec6805ca95fa64")


def rank(hash32: int, g: int) -> int:
    return (int(hash32) * int(g)) >> 32


def frame_key(b, i):
    """(raw dst port, raw dst address) of frame i."""
    o = int(b.offset[i])
    f = b.frames
    return int(f[o + 36]) | int(f[o + 37]) << 8, int.from_bytes(bytes(f[o + 30:o + 34]), "little")


def walk(port_list, dport_raw, dip_raw):
    """The sockfds frame (dport, dip) is delivered to, in the order the reference's loop makes
    them. port_list: raw port -> [(ip, sockfd, reuse)] (BindTable.port_list, or a dict's get)."""
    out = []
    for ip, s, reuse in port_list(dport_raw) or []:
        if ip == dip_raw or ip == 0:
            out.append(s)
            if not reuse:
                break
    return out


def frame_hashes(b, key=R.STD_KEY, types=3):
    """What udpdk_gpu_rss writes to hash_dev for the batch (rss_util's independent restatement)."""
    return R.rss_ref(key, types, [0], 1, b, getattr(b, "ptype", None))[0]


def choose(port_list, b, meta, lane_rp, hashes, n_lanes=None):
    """-> (chosen u32[n], deliveries list per frame, balanced frame count)."""
    lane_rp = np.asarray(lane_rp, np.uint8)
    n_lanes = len(lane_rp) if n_lanes is None else n_lanes
    n = len(meta)
    chosen = np.full(n, KEEP_ALL, np.uint32)
    dels = [[] for _ in range(n)]
    cache = {}
    balanced = 0
    for i in np.flatnonzero((np.asarray(meta, np.uint32) & 0xF) == V_DELIVERED):
        k = frame_key(b, i)
        if k not in cache:
            cache[k] = walk(port_list, *k)
        d = dels[i] = cache[k]
        G = [s for s in d if s < n_lanes and lane_rp[s]]
        dip = k[1]
        if len(G) <= 1 or dip == 0xFFFFFFFF or 224 <= (dip & 0xFF) <= 239:
            continue
        chosen[i] = G[rank(hashes[i], len(G))]
        balanced += 1
    return chosen, dels, balanced


@dataclass
class Balanced:
    lane_off: np.ndarray
    lane_pkt: np.ndarray
    kept: int
    removed: int
    balanced: int
    bad_index: int
    truncated: int
    chosen: np.ndarray


def model(port_list, b, meta, lane_off, lane_pkt, lane_rp, hashes=None, n=None, lane_cap=None,
          key=R.STD_KEY, types=3) -> Balanced:
    meta = np.asarray(meta, np.uint32)
    n = len(meta) if n is None else n
    meta = meta[:n]
    lane_off = np.asarray(lane_off, np.uint32).astype(np.int64)
    lane_rp = np.asarray(lane_rp, np.uint8)
    n_lanes = len(lane_off) - 1
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    d = int(min(lane_off[-1], lane_cap))
    pkt = np.asarray(lane_pkt, np.uint32)[:d]
    if hashes is None:
        hashes = frame_hashes(b, key, types)
    chosen, _, balanced = choose(port_list, b, meta, lane_rp, hashes, n_lanes)
    off_c = np.minimum(lane_off, d)
    lane_of = np.searchsorted(off_c[1:], np.arange(d), side="right")     # largest l with off[l] <= p
    lane_of = np.minimum(lane_of, n_lanes - 1)
    valid = pkt < n
    ch = np.full(d, KEEP_ALL, np.uint32)
    ch[valid] = chosen[pkt[valid]]
    gone = valid & (lane_rp[lane_of] != 0) & (ch != KEEP_ALL) & (ch != lane_of)
    keep = valid & ~gone
    pre = np.concatenate([[0], np.cumsum(keep)])
    kept = int(keep.sum())
    return Balanced(pre[off_c].astype(np.uint32), pkt[keep], kept, d - kept, balanced,
                    int((~valid).sum()), int(lane_off[-1] > lane_cap), chosen)


# ---- frames --------------------------------------------------------------------------------------
def _csum(words_be: np.ndarray) -> np.ndarray:
    s = words_be.astype(np.uint64).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF


def _be16(a: np.ndarray) -> np.ndarray:
    return a[:, 0::2].astype(np.uint64) << 8 | a[:, 1::2]


def ip_bytes(ip: str):
    return [int(x) for x in ip.split(".")]


def flow_frames(src, sport, dst, dport, seed, payload_len=22, gaps=None, tail=64, payload=None):
    """One valid Eth/IPv4/UDP frame per row: src / dst are uint8 [n, 4] address bytes, sport / dport
    host-order ports [n]; payload random by seed (or the rows of `payload`), IPv4 and UDP checksums right. gaps: bytes before
    each frame (None: back to back). `tail` spare bytes follow the frames in .frames (the tailroom
    a caller uploads); .frames_bytes is where the last frame ends."""
    src, dst = np.asarray(src, np.uint8), np.asarray(dst, np.uint8)
    sport, dport = np.asarray(sport, np.int64), np.asarray(dport, np.int64)
    n, L = len(sport), 42 + payload_len
    assert payload_len % 2 == 0
    rng = np.random.default_rng(seed)
    f = np.zeros((n, L), np.uint8)
    f[:, :12] = np.frombuffer(MAC, np.uint8)
    f[:, 12:15] = (0x08, 0x00, 0x45)
    f[:, 16], f[:, 17] = (L - 14) >> 8, (L - 14) & 0xFF
    f[:, 18:20] = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    f[:, 22], f[:, 23] = 64, 17
    f[:, 26:30], f[:, 30:34] = src, dst
    f[:, 34], f[:, 35] = sport >> 8, sport & 0xFF
    f[:, 36], f[:, 37] = dport >> 8, dport & 0xFF
    f[:, 38], f[:, 39] = (L - 34) >> 8, (L - 34) & 0xFF
    f[:, 42:] = rng.integers(0, 256, (n, payload_len), dtype=np.uint8) if payload is None else payload
    c = _csum(_be16(f[:, 14:34]))
    f[:, 24], f[:, 25] = c >> 8, c & 0xFF
    pseudo = np.concatenate([_be16(f[:, 26:34]), np.full((n, 1), 17, np.uint64),
                             np.full((n, 1), L - 34, np.uint64), _be16(f[:, 34:])], axis=1)
    c = _csum(pseudo)
    c[c == 0] = 0xFFFF
    f[:, 40], f[:, 41] = c >> 8, c & 0xFF
    gap = np.zeros(n, np.int64) if gaps is None else np.asarray(gaps, np.int64)
    off = np.cumsum(gap + L) - L
    total = int(off[-1] + L) if n else 0
    flat = np.zeros(total + tail, np.uint8)
    flat[off[:, None] + np.arange(L)[None, :]] = f
    return SimpleNamespace(frames=flat, offset=off.astype(np.uint32), length=np.full(n, L, np.uint16),
                           frames_bytes=total, n=n, ptype=None, rows=f)


def random_flows(n_flows, seed):
    """(src uint8 [n, 4], sport [n]): distinct random flows from 10.x.y.z."""
    rng = np.random.default_rng(seed)
    v = rng.choice(1 << 40, n_flows, replace=False)
    src = np.stack([np.full(n_flows, 10), (v >> 32) & 255, (v >> 24) & 255, (v >> 16) & 255], axis=1).astype(np.uint8)
    return src, (v & 0xFFFF).astype(np.int64)


def reuse_lists(port_host, n_members, ip="0.0.0.0", first_sock=0):
    """{raw port: [(ip, sockfd, 1)] x n_members}: sockets first_sock.. on one port, all reuse."""
    import socket
    import struct
    raw_ip = struct.unpack("<I", socket.inet_aton(ip))[0]
    raw_port = struct.unpack("<H", struct.pack(">H", port_host))[0]
    return {raw_port: [(raw_ip, first_sock + k, 1) for k in range(n_members)]}
