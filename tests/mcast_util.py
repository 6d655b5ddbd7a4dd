"""An independent Python model of the multicast membership filter (udpdk_gpu_rx_mcast_select /
udpdk_gpu_rx_mcast) with its own hash, table builder and probe, and of the IGMPv2 query responder
(udpdk_gpu_igmp_reply) with its own RFC 1071, for test_mcast_ref.py (where they are pinned to
hand-written vectors and the library's builder to the model), test_gpu_rx_mcast.py and
test_gpu_igmp.py, and small builders for member lists, batches with chosen destinations and IGMP
frames.

The rule, for entry p of lane l with frame i = lane_pkt[p], D = min(lane_off[-1], lane_cap):
    i >= n                                   removed, bad_index
    lane_mc[l] == 0                          kept
    length[i] < 42 or offset[i] + length[i] > frames_bytes
                                             removed, bad_frame
    dst = u32 at frame bytes 30-33; dst & 0xFF outside 224..239
                                             kept
    (dst, l) in the table                    kept (member), else removed: not_member
    new_pkt = lane_pkt[keep];  new_off = concat([0], cumsum(keep))[min(lane_off, D)]

The table: `slots` (group, lane) records, a power of two in 2..2^20, group == 0 empty; the probe of
(group, lane) starts at h >> (32 - log2(slots)), h = (group ^ lane * 0x9E3779B1) * 0x85EBCA6B mod
2^32, steps by one with wrap-around and ends at a match, an empty slot or after `slots` probes.
"""
from dataclasses import dataclass

import numpy as np

import rx_balance_util as B
from udpdk_amd import abi

MCAST_DTYPE = abi.MCAST_DTYPE
M32 = 0xFFFFFFFF


# ---- the table -----------------------------------------------------------------------------------
def hash32(group: int, lane: int) -> int:
    return (((group ^ ((lane * 0x9E3779B1) & M32)) & M32) * 0x85EBCA6B) & M32


def start(group: int, lane: int, slots: int) -> int:
    lg = slots.bit_length() - 1
    assert 2 <= slots <= 1 << 20 and 1 << lg == slots
    return hash32(group, lane) >> (32 - lg)


def build(members, slots: int):
    """[(group, lane)] in order -> list of `slots` (group, lane) tuples, (0, 0) where empty."""
    tab = [(0, 0)] * slots
    assert len(members) <= slots
    for g, l in members:
        assert g != 0 and (g, l) not in tab
        i = start(g, l, slots)
        while tab[i][0] != 0:
            i = (i + 1) % slots
        tab[i] = (int(g), int(l))
    return tab


def probe(tab, group: int, lane: int):
    """(found, probes made)."""
    slots = len(tab)
    i = start(group, lane, slots)
    for k in range(slots):
        if tab[i] == (group, lane):
            return True, k + 1
        if tab[i][0] == 0:
            return False, k + 1
        i = (i + 1) % slots
    return False, slots


def as_records(tab) -> np.ndarray:
    return np.array(tab, MCAST_DTYPE) if len(tab) else np.zeros(0, MCAST_DTYPE)


def slots_for(n_members: int) -> int:
    """What the sticky call sizes its table to: the smallest power of two >= 2 n, minimum 2."""
    s = 2
    while s < 2 * n_members:
        s *= 2
    return s


def members_of(joined):
    """{lane: [group ip strings or raw u32]} -> [(raw group, lane)] in lane order."""
    return [(abi.raw_ip(g) if isinstance(g, str) else int(g), int(l)) for l in sorted(joined) for g in joined[l]]


# ---- the filter ----------------------------------------------------------------------------------
def dst_field(b, idx):
    """The raw u32 at frame bytes 30-33 of the frames idx (all in range)."""
    f = np.asarray(b.frames, np.uint8)
    o = np.asarray(b.offset, np.uint32)[idx].astype(np.int64)
    return (f[o + 30].astype(np.uint32) | f[o + 31].astype(np.uint32) << 8 | f[o + 32].astype(np.uint32) << 16 |
            f[o + 33].astype(np.uint32) << 24)


@dataclass
class Filtered:
    lane_off: np.ndarray
    lane_pkt: np.ndarray
    kept: int
    removed: int
    member: int
    not_member: int
    bad_frame: int
    bad_index: int
    truncated: int
    keep: np.ndarray           # bool per input entry [D]

    def stats(self):
        return (self.kept, self.removed, self.member, self.not_member, self.bad_frame, self.bad_index,
                self.truncated)


def stats_tuple(st):
    """The same tuple from an abi.RxMcastStats."""
    return (st.kept, st.removed, st.member, st.not_member, st.bad_frame, st.bad_index, st.truncated)


def model(b, lane_off, lane_pkt, lane_mc, tab, n=None, lane_cap=None, frames_bytes=None) -> Filtered:
    """tab: the table as build() returns it (probed slot by slot, as the device does)."""
    lane_off = np.asarray(lane_off, np.uint32).astype(np.int64)
    lane_mc = np.asarray(lane_mc, np.uint8)
    n_lanes = len(lane_off) - 1
    assert len(lane_mc) >= n_lanes
    n = len(b.offset) if n is None else n
    fb = int(b.frames_bytes) if frames_bytes is None else frames_bytes
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    d = int(min(lane_off[-1], lane_cap))
    pkt = np.asarray(lane_pkt, np.uint32)[:d]
    off_c = np.minimum(lane_off, d)
    lane_of = np.searchsorted(off_c[1:], np.arange(d), side="right")     # largest l with off[l] <= p
    lane_of = np.minimum(lane_of, n_lanes - 1)
    valid = pkt < n
    chk = valid & (lane_mc[lane_of] != 0)
    ok = np.zeros(d, bool)
    ci = np.flatnonzero(chk)
    o = np.asarray(b.offset, np.uint32)[pkt[ci]].astype(np.int64)
    ln = np.asarray(b.length, np.uint16)[pkt[ci]].astype(np.int64)
    ok[ci] = (ln >= 42) & (o + ln <= fb)
    oi = np.flatnonzero(ok)
    dst = dst_field(b, pkt[oi])
    grp = np.zeros(d, bool)
    grp[oi] = ((dst & 0xFF) >= 224) & ((dst & 0xFF) <= 239)
    memb = np.zeros(d, bool)
    cache = {}
    for p, g in zip(oi, dst):
        if grp[p]:
            key = (int(g), int(lane_of[p]))
            if key not in cache:
                cache[key] = probe(tab, *key)[0]
            memb[p] = cache[key]
    keep = valid & (~chk | (ok & (~grp | memb)))
    pre = np.concatenate([[0], np.cumsum(keep)])
    kept = int(keep.sum())
    return Filtered(pre[off_c].astype(np.uint32), pkt[keep], kept, d - kept, int(memb.sum()),
                    int((grp & ~memb).sum()), int((chk & ~ok).sum()), int((~valid).sum()),
                    int(lane_off[-1] > lane_cap), keep)


# ---- batches -------------------------------------------------------------------------------------
OUR_IP = "172.31.100.1"
G1, G2, G3 = "239.1.2.3", "239.1.2.4", "224.0.0.251"        # G1: the group the tests join
# one destination per way an entry can look: the joined group, another group, the two ends of 224/4
# joined or not, unicast, limited broadcast, and the first bytes either side of 224..239
KINDS = {"member": G1, "other": G2, "low": "224.0.0.1", "high": "239.255.255.255", "unicast": OUR_IP,
         "bcast": "255.255.255.255", "b223": "223.1.2.3", "b240": "240.1.2.3"}


def frames_to(dsts, dport, seed, payload_len=22, gaps=None, tail=64, src="10.1.2.3", sport=7000, payload=None):
    """One valid frame per destination ip string in `dsts` (B.flow_frames)."""
    n = len(dsts)
    dst = np.array([B.ip_bytes(ip) for ip in dsts], np.uint8).reshape(n, 4)
    srcb = np.tile(np.array(B.ip_bytes(src), np.uint8), (n, 1))
    return B.flow_frames(srcb, np.full(n, sport, np.int64), dst, np.broadcast_to(np.asarray(dport, np.int64), (n,)),
                         seed, payload_len=payload_len, gaps=gaps, tail=tail, payload=payload)


def single_lanes(n_lanes, counts, order=None):
    """A lane set of sum(counts) entries, frames 0.. in lane order (or `order`): (lane_off, lane_pkt)."""
    counts = np.asarray(counts, np.int64)
    assert len(counts) == n_lanes
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    pkt = np.arange(int(off[-1]), dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    return off, pkt


# ---- IGMP ----------------------------------------------------------------------------------------
# The model of the IGMP query responder (udpdk_gpu_igmp_reply) with its own RFC 1071, and builders
# for the frames it reads and writes.
V_NOT_UDP = 3                                                # UDPDK_V_NOT_UDP
ALL_HOSTS, ALL_ROUTERS = "224.0.0.1", "224.0.0.2"
IGMP_STATS = abi.IGMP_STATS
SRC_MAC = bytes.fromhex("6805ca95f8ec")
QUERIER_MAC = bytes.fromhex("6805ca95fa64")


def rfc1071(data: bytes) -> int:
    """The 16-bit one's-complement sum of big-endian words, an odd length padded with a zero byte."""
    if len(data) % 2:
        data = data + b"\0"
    s = 0
    for k in range(0, len(data), 2):
        s += data[k] << 8 | data[k + 1]
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ip4(s: str) -> bytes:
    return bytes(int(x) for x in s.split("."))


def group_mac(group: bytes) -> bytes:
    return bytes([0x01, 0x00, 0x5E, group[1] & 0x7F, group[2], group[3]])


def igmp_frame(src_mac: bytes, src_ip: str, dst_ip: str, typ: int, group: str) -> bytes:
    """The 46-byte frame the stack sends: Ethernet, IPv4 with Router Alert (IHL 6, TOS c0, DF, TTL 1),
    an 8-byte IGMPv2 message."""
    g, d = ip4(group), ip4(dst_ip)
    ip = bytearray(bytes.fromhex("46c00020000040000102") + b"\0\0" + ip4(src_ip) + d + bytes.fromhex("94040000"))
    c = ~rfc1071(bytes(ip)) & 0xFFFF
    ip[10:12] = bytes([c >> 8, c & 0xFF])
    msg = bytearray(bytes([typ, 0, 0, 0]) + g)
    c = ~rfc1071(bytes(msg)) & 0xFFFF
    msg[2:4] = bytes([c >> 8, c & 0xFF])
    return group_mac(d) + src_mac + b"\x08\x00" + bytes(ip) + bytes(msg)


def report_frame(src_mac, src_ip, group):
    return igmp_frame(src_mac, src_ip, group, 0x16, group)


def leave_frame(src_mac, src_ip, group):
    return igmp_frame(src_mac, src_ip, ALL_ROUTERS, 0x17, group)


def query(group="0.0.0.0", dst=None, *, typ=0x11, ihl=6, msg_len=8, src="10.0.0.1", proto=2, max_resp=100,
          ip_cksum=True, igmp_cksum=True, total_len=None, pad=0, cut=None) -> bytes:
    """A frame as a querier sends it (or as one gets it wrong): IHL 5 has no option, 6 Router Alert,
    more pads with no-ops; msg_len 8 is v1/v2, 12 v3 (4 bytes follow the group), any other length
    random-ish filler. dst None: 224.0.0.1 for a general query, the group otherwise."""
    g = ip4(group)
    d = ip4(dst if dst is not None else (ALL_HOSTS if group == "0.0.0.0" else group))
    opts = b"" if ihl == 5 else bytes.fromhex("94040000") + b"\x01" * (4 * (ihl - 6))
    tl = 4 * ihl + msg_len if total_len is None else total_len
    ip = bytearray(bytes([0x40 | ihl, 0xC0, tl >> 8, tl & 0xFF, 0, 0, 0, 0, 1, proto, 0, 0]) + ip4(src) + d + opts)
    c = ~rfc1071(bytes(ip)) & 0xFFFF
    if not ip_cksum:
        c ^= 0x0100
    ip[10:12] = bytes([c >> 8, c & 0xFF])
    msg = bytearray(bytes([typ, max_resp, 0, 0]) + g + bytes((7 * k + 3) & 0xFF for k in range(max(0, msg_len - 8))))
    msg = msg[:msg_len]
    c = ~rfc1071(bytes(msg)) & 0xFFFF
    if not igmp_cksum:
        c ^= 0x0001
    if msg_len >= 4:
        msg[2:4] = bytes([c >> 8, c & 0xFF])
    f = group_mac(d) + QUERIER_MAC + b"\x08\x00" + bytes(ip) + bytes(msg) + bytes(pad)
    return f if cut is None else f[:cut]


def pack(frames, gaps=None, tail=64):
    """Frames back to back (or `gaps` bytes before each): a batch like B.flow_frames's."""
    from types import SimpleNamespace
    gaps = [0] * len(frames) if gaps is None else gaps
    out, offs = bytearray(), []
    for f, g in zip(frames, gaps):
        out += bytes(int(g))
        offs.append(len(out))
        out += f
    total = len(out)
    flat = np.zeros(total + tail, np.uint8)
    flat[:total] = np.frombuffer(bytes(out), np.uint8)
    return SimpleNamespace(frames=flat, offset=np.array(offs, np.uint32), length=np.array([len(f) for f in frames], np.uint16),
                           frames_bytes=total, n=len(frames), ptype=None)


def igmp_classify(f: bytes, groups) -> str | None:
    """The counter one candidate frame (all of it in range) lands in besides igmp, or None when it is
    not IGMP; groups: raw addresses."""
    if f[23] != 2:
        return None
    ihl = f[14] & 0xF
    tl = f[16] << 8 | f[17]
    if ihl < 5 or tl < 4 * ihl + 8 or 14 + tl > len(f) or rfc1071(f[14:14 + 4 * ihl]) != 0xFFFF:
        return "malformed"
    msg = f[14 + 4 * ihl:14 + tl]
    if rfc1071(msg) != 0xFFFF:
        return "bad_cksum"
    if msg[0] != 0x11:
        return "other_type"
    grp, dst = bytes(msg[4:8]), bytes(f[30:34])
    if grp == bytes(4):
        return "general" if dst == ip4(ALL_HOSTS) else "bad_dst"
    if dst != grp:
        return "bad_dst"
    return "specific" if int.from_bytes(grp, "little") in [int(g) for g in groups] else "not_member"


def igmp_model(b, meta, cfg_mac: bytes, cfg_ip: str, groups, max_reports=None, n=None, frames_bytes=None):
    """(stats dict, [report frames, 46 bytes each], [group index per report])."""
    groups = [int(g) for g in groups]
    n = b.n if n is None else n
    fb = int(b.frames_bytes) if frames_bytes is None else frames_bytes
    max_reports = len(groups) if max_reports is None else max_reports
    st = dict.fromkeys(IGMP_STATS, 0)
    ask = set()
    for i in range(n):
        if int(meta[i]) & 0xF != V_NOT_UDP:
            continue
        o, ln = int(b.offset[i]), int(b.length[i])
        if ln < 34 or o + ln > fb:
            st["bad_frame"] += 1
            continue
        f = bytes(b.frames[o:o + ln])
        k = igmp_classify(f, groups)
        if k is None:
            continue
        st["igmp"] += 1
        st[k] += 1
        if k == "general":
            ask |= {j for j, g in enumerate(groups) if g != abi.raw_ip(ALL_HOSTS)}
        elif k == "specific":
            ask.add(groups.index(int.from_bytes(f[14 + 4 * (f[14] & 0xF) + 4:][:4], "little")))
    order = sorted(ask)
    st["reports"] = min(len(order), max_reports)
    st["no_room"] = len(order) - st["reports"]
    idx = order[:st["reports"]]
    frames = [report_frame(cfg_mac, cfg_ip, ".".join(str(x) for x in groups[j].to_bytes(4, "little"))) for j in idx]
    return st, frames, idx
