"""The model of udpdk_gpu_icmp_reply (include/udpdk_gpu.h) in numpy, and builders for the frames its
tests need: echo requests of any message length at any byte alignment, other ICMP types, UDP to open
and closed ports. The gates are vectorised over the batch; the sums run per echo candidate."""
import socket
import struct
from dataclasses import dataclass, field

import numpy as np

from udpdk_amd import abi, frames as F

ECHO, UNREACH, ALL = 1, 2, 3
UNREACH_BYTES = 70
NO_LIMIT = 0xFFFFFFFF
OUR_IP = F.IP_DST                       # the stack's address: cfg.src_ip
SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")


def tx_config(src_ip: str = OUR_IP) -> abi.TxConfig:
    return abi.TxConfig((abi.C.c_uint8 * 6)(*SRC_MAC), (abi.C.c_uint8 * 6)(*DST_MAC), abi.raw_ip(src_ip))


# ---- RFC 1071 -----------------------------------------------------------------------------------
def word_sum(b) -> int:
    """Sum of the little-endian 16-bit words of b, an odd tail zero-padded; not folded."""
    a = np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else b
    if len(a) % 2:
        a = np.concatenate([a, np.zeros(1, np.uint8)])
    return int(a[0::2].astype(np.uint64).sum() + (a[1::2].astype(np.uint64).sum() << np.uint64(8)))


def fold(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def cksum(b) -> int:
    """The checksum field (as a little-endian word) of a message whose field is zero."""
    return ~fold(word_sum(b)) & 0xFFFF


def ipv4_header(tl: int, proto: int, src_raw: int, dst_raw: int) -> bytes:
    """The IPv4 header tx_build writes: id 0, fragment field 0, ttl 64, rte_ipv4_cksum (a sum of
    0xffff stays 0xffff)."""
    h = bytearray(struct.pack(">BBHHHBBH", 0x45, 0, tl, 0, 0, 64, proto, 0) + struct.pack("<II", src_raw, dst_raw))
    s = fold(word_sum(h))
    h[10:12] = struct.pack("<H", s if s == 0xFFFF else ~s & 0xFFFF)
    return bytes(h)


# ---- frame builders -----------------------------------------------------------------------------
def ip_frame(proto: int, l4: bytes, *, src_ip=F.IP_SRC, dst_ip=OUR_IP, ihl=5, frag=0, ip_cksum="ok", tl=None,
             pad_to=0, ident=0x1234) -> bytes:
    opts = bytes(4 * (ihl - 5))
    tl = 4 * ihl + len(l4) if tl is None else tl
    ip = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, tl, ident, frag, 64, proto, 0,
                               socket.inet_aton(src_ip), socket.inet_aton(dst_ip)) + opts)
    c = cksum(ip)
    ip[10:12] = struct.pack("<H", c ^ 0x0101 if ip_cksum == "bad" else c)
    f = F.ETH_DST + F.ETH_SRC + b"\x08\x00" + bytes(ip) + l4
    return f + bytes(max(0, pad_to - len(f)))


def icmp_msg(typ: int, code: int, ident: int, seq: int, data: bytes, bad_cksum=False) -> bytes:
    m = bytearray(struct.pack(">BBHHH", typ, code, 0, ident, seq) + data)
    c = cksum(m)
    m[2:4] = struct.pack("<H", c ^ 0x0400 if bad_cksum else c)
    return bytes(m)


def echo_request(rng, msg_len: int, *, ident=None, seq=None, data=None, typ=8, code=0, bad_cksum=False, **kw) -> bytes:
    """An ICMP echo request whose message (header + data) has msg_len >= 8 bytes."""
    ident = int(rng.integers(0, 65536)) if ident is None else ident
    seq = int(rng.integers(0, 65536)) if seq is None else seq
    data = rng.integers(0, 256, msg_len - 8, dtype=np.uint8).tobytes() if data is None else data
    return ip_frame(1, icmp_msg(typ, code, ident, seq, data, bad_cksum), **kw)


def udp_frame(rng, dport: int, **kw) -> bytes:
    return F.make_frame(rng, dport=dport, **kw)


def pack(frame_list, aligns=None, gap=0):
    """Frames into one buffer; frame k starts at an offset == aligns[k] mod 16 (None: back to back + gap)."""
    off, pos = [], 0
    for k, f in enumerate(frame_list):
        if aligns is not None:
            pos += (aligns[k] - pos) % 16
        off.append(pos)
        pos += len(f) + gap
    buf = np.zeros(pos, np.uint8)
    for o, f in zip(off, frame_list):
        buf[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return buf, pos, np.array(off, np.uint32), np.array([len(f) for f in frame_list], np.uint16)


# ---- the model ----------------------------------------------------------------------------------
@dataclass
class Replies:
    reply_off: np.ndarray            # [replies + 1]
    origin: np.ndarray               # [replies]
    out: np.ndarray                  # the written bytes, reply_off[-1] of them
    stats: dict
    reason: list = field(default_factory=list)   # per frame: "", "echo", "unreach", "echo_bad", "limited",
                                                  # "no_room", "bad_frame", "gate", "other"
    frames_out: list = field(default_factory=list)   # every reply the limit leaves, cut ones included


def model(frames, frames_bytes, offset, length, meta, *, src_ip=None, src_mac=SRC_MAC, dst_mac=DST_MAC, flags=ALL,
          mtu=0, err_limit=NO_LIMIT, out_cap=(1 << 32) - 1, max_replies=None) -> Replies:
    n = len(offset)
    src_ip = abi.raw_ip(OUR_IP) if src_ip is None else src_ip
    max_replies = n if max_replies is None else max_replies
    m = np.asarray(meta, np.uint32)[:n]
    off = np.asarray(offset, np.int64)
    ln = np.asarray(length, np.int64)
    v = m & 0xF
    gate1 = (((m >> 4) & 1) == 1) & (((m >> 8) & 1) == 0)
    c_echo = bool(flags & ECHO) & (v == abi.V_NOT_UDP) & gate1
    c_unr = bool(flags & UNREACH) & ((v == abi.V_NO_BIND) | (v == abi.V_NO_MATCH)) & gate1 & \
        (((m >> 5) & 3) != abi.UDP_BAD) & (((m >> 7) & 1) == 0)
    cand = c_echo | c_unr
    fok = cand & (ln >= 42) & (off + ln <= frames_bytes)
    fr = np.concatenate([np.asarray(frames, np.uint8)[:frames_bytes], np.zeros(64, np.uint8)])
    o = np.where(fok, off, 0)
    B = lambda k: fr[o + k].astype(np.int64)                      # noqa: E731  frame byte k of every frame
    dst = B(30) | B(31) << 8 | B(32) << 16 | B(33) << 24
    src = B(26) | B(27) << 8 | B(28) << 16 | B(29) << 24
    sb = B(26)
    gates = fok & (dst == src_ip) & (sb != 0) & (sb != 127) & (sb < 224)
    tl = B(16) << 8 | B(17)
    is_echo = c_echo & gates & (B(23) == 1) & (B(34) == 8) & (B(35) == 0)
    lens_ok = is_echo & (tl >= 28) & (14 + tl <= ln) & ((mtu == 0) | (tl <= mtu))
    elig = c_unr & gates
    reason = [""] * n
    for i in np.flatnonzero(cand):
        reason[i] = "bad_frame" if not fok[i] else "gate" if not gates[i] else "other"
    head = bytes(dst_mac) + bytes(src_mac) + b"\x08\x00"
    replies = []                                                   # (frame, bytes) the limit leaves
    n_elig = limited = echo_bad = 0
    for i in np.flatnonzero(is_echo | elig):
        i = int(i)
        f = fr[o[i]:o[i] + ln[i]]
        if elig[i]:
            n_elig += 1
            if n_elig > err_limit:
                limited += 1
                reason[i] = "limited"
                continue
            body = bytearray(b"\x03\x03\x00\x00\x00\x00\x00\x00" + f[14:42].tobytes())
            body[2:4] = struct.pack("<H", cksum(body))
            replies.append((i, head + ipv4_header(56, 1, src_ip, int(src[i])) + bytes(body)))
            reason[i] = "unreach"
        else:
            t = int(tl[i])
            if not lens_ok[i] or fold(word_sum(f[34:14 + t])) != 0xFFFF:
                echo_bad += 1
                reason[i] = "echo_bad"
                continue
            body = bytearray(b"\x00\x00\x00\x00" + f[38:14 + t].tobytes())
            body[2:4] = struct.pack("<H", cksum(body))
            replies.append((i, head + ipv4_header(t, 1, src_ip, int(src[i])) + bytes(body)))
            reason[i] = "echo"
    # room: rank below max_replies and end within out_cap; the rest is a tail
    ro, org, out, pos, no_room = [0], [], [], 0, 0
    st = dict(echo_replied=0, unreach_sent=0)
    for r, (i, b) in enumerate(replies):
        if no_room or r >= max_replies or pos + len(b) > out_cap:
            no_room += 1
            reason[i] = "no_room"
            continue
        st["unreach_sent" if b[34] == 3 else "echo_replied"] += 1
        pos += len(b)
        ro.append(pos)
        org.append(i)
        out.append(np.frombuffer(b, np.uint8))
    st.update(bytes_needed=sum(len(b) for _, b in replies), replies=len(org), echo_bad=echo_bad, limited=limited,
              no_room=no_room, bad_frame=int((cand & ~fok).sum()))
    return Replies(np.array(ro, np.uint32), np.array(org, np.uint32),
                   np.concatenate(out) if out else np.zeros(0, np.uint8), st, reason, [b for _, b in replies])


STAT_FIELDS = ("bytes_needed", "replies", "echo_replied", "unreach_sent", "echo_bad", "limited", "no_room", "bad_frame")


def stats_dict(st) -> dict:
    return {k: int(getattr(st, k)) for k in STAT_FIELDS}


# ---- a mixed batch ------------------------------------------------------------------------------
OPEN_PORTS, CLOSED_PORT, OTHER_IP = [10001, 10002], 7, "172.31.100.9"
# port 10002 is bound to another address: a datagram for it to ours is NO_MATCH
LISTS = {abi.raw_port(10001): [(0, 0, 0)], abi.raw_port(10002): [(abi.raw_ip(OTHER_IP), 1, 0)]}
N_LANES = 2

KINDS = ("echo", "echo_pad", "echo_badck", "echo_short_tl", "echo_long_tl", "udp_open", "udp_closed", "udp_nomatch",
         "udp_closed_badck", "udp_closed_badlen", "dst_other", "dst_bcast", "dst_mcast", "src_zero", "src_loop",
         "src_mcast", "ip_bad", "ihl6", "code1", "type0", "type13", "tcp", "frag", "closed_other_dst")


def kind_frame(rng, kind: str) -> bytes:
    ml = int(rng.choice([8, 9, 17, 56, 64, 65, 100, 300, 1400]))
    if kind == "echo":
        return echo_request(rng, ml)
    if kind == "echo_pad":
        return echo_request(rng, int(rng.integers(8, 18)), pad_to=60)
    if kind == "echo_badck":
        return echo_request(rng, ml, bad_cksum=True)
    if kind == "echo_short_tl":
        return echo_request(rng, ml, tl=int(rng.integers(20, 28)))
    if kind == "echo_long_tl":
        return echo_request(rng, ml, tl=20 + ml + int(rng.integers(1, 9)))
    if kind == "udp_open":
        return udp_frame(rng, 10001, payload_len=int(rng.integers(0, 200)))
    if kind == "udp_closed":
        return udp_frame(rng, CLOSED_PORT, payload_len=int(rng.integers(0, 200)),
                         udp_cksum=str(rng.choice(["ok", "none"])))
    if kind == "udp_nomatch":
        return udp_frame(rng, 10002, payload_len=int(rng.integers(0, 200)))
    if kind == "udp_closed_badck":
        return udp_frame(rng, CLOSED_PORT, payload_len=30, udp_cksum="bad")
    if kind == "udp_closed_badlen":
        return udp_frame(rng, CLOSED_PORT, payload_len=30, udp_len=200, udp_cksum="none")
    if kind == "closed_other_dst":
        return udp_frame(rng, CLOSED_PORT, dst_ip=OTHER_IP)
    if kind == "dst_other":
        return echo_request(rng, ml, dst_ip=OTHER_IP)
    if kind == "dst_bcast":
        return echo_request(rng, ml, dst_ip="255.255.255.255")
    if kind == "dst_mcast":
        return echo_request(rng, ml, dst_ip="224.0.0.1")
    if kind == "src_zero":
        return echo_request(rng, ml, src_ip="0.1.2.3")
    if kind == "src_loop":
        return udp_frame(rng, CLOSED_PORT, src_ip="127.0.0.1")
    if kind == "src_mcast":
        return echo_request(rng, ml, src_ip=str(rng.choice(["224.1.1.1", "240.0.0.1", "255.255.255.255"])))
    if kind == "ip_bad":
        return echo_request(rng, ml, ip_cksum="bad")
    if kind == "ihl6":
        return echo_request(rng, ml, ihl=6)
    if kind == "code1":
        return echo_request(rng, ml, code=1)
    if kind == "type0":
        return echo_request(rng, ml, typ=0)
    if kind == "type13":
        return echo_request(rng, 20, typ=13)
    if kind == "tcp":
        return ip_frame(6, rng.integers(0, 256, 20, dtype=np.uint8).tobytes())
    if kind == "frag":
        return echo_request(rng, ml, frag=0x2000)
    raise ValueError(kind)


def mixed(seed: int, n: int):
    """n frames of every kind above in random order at random alignments: (buf, bytes, offset, length, kinds)."""
    rng = np.random.default_rng(seed)
    kinds = [KINDS[k] for k in rng.integers(0, len(KINDS), n)]
    fl = [kind_frame(rng, k) for k in kinds]
    buf, nb, off, ln = pack(fl, aligns=rng.integers(0, 16, n).tolist())
    return buf, nb, off, ln, kinds


def assert_mixed_counts(R: Replies, least: int = 20):
    """No comparison on a mixed batch passes empty."""
    for r in ("echo", "unreach", "echo_bad", "gate", "other"):
        assert R.reason.count(r) >= least, (r, R.reason.count(r))
