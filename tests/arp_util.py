"""The model of udpdk_gpu_arp_reply (include/udpdk_gpu.h) in numpy, and builders for the frames its
tests need: ARP frames with each header field wrong in turn, every opcode and sender / target class,
padded or not, placed at any byte alignment, beside UDP and other ethertypes."""
import socket
import struct

import numpy as np

from udpdk_amd import abi, frames as F

FRAME_BYTES, SLOT_BYTES = 42, 64
OUR_IP = F.IP_DST                       # the stack's address: cfg.src_ip
OUR_MAC = bytes.fromhex("6805ca95f8ec")  # cfg.src_mac
PEER_MAC = bytes.fromhex("6805ca95fa64") # cfg.dst_mac (not used by the stage)
ASKER_MAC = bytes.fromhex("02a1b2c3d4e5")
ASKER_IP = "172.31.100.77"
OTHER_IP = "172.31.100.9"
BCAST = b"\xff" * 6
STAT_FIELDS = abi.ARP_STATS
V_NOT_IPV4 = 1                          # UDPDK_V_NOT_IPV4


def tx_config(src_ip: str = OUR_IP, src_mac: bytes = OUR_MAC) -> abi.TxConfig:
    return abi.TxConfig((abi.C.c_uint8 * 6)(*src_mac), (abi.C.c_uint8 * 6)(*PEER_MAC), abi.raw_ip(src_ip))


# ---- frame builders -----------------------------------------------------------------------------
def arp_frame(*, op=1, sha=ASKER_MAC, spa=ASKER_IP, tha=bytes(6), tpa=OUR_IP, htype=1, ptype=0x0800, hlen=6, plen=4,
              ethertype=0x0806, eth_dst=BCAST, eth_src=None, pad_to=0, trunc=None) -> bytes:
    """An Ethernet frame carrying one ARP packet (RFC 826 layout); trunc cuts it to that many bytes."""
    f = eth_dst + (sha if eth_src is None else eth_src) + struct.pack(">H", ethertype) + \
        struct.pack(">HHBBH", htype, ptype, hlen, plen, op) + sha + socket.inet_aton(spa) + tha + socket.inet_aton(tpa)
    f = f + bytes(max(0, pad_to - len(f)))
    return f if trunc is None else f[:trunc]


def udp_frame(rng, dport: int = F.PORT_RECV, **kw) -> bytes:
    return F.make_frame(rng, dport=dport, **kw)


def rand_mac(rng) -> bytes:
    """A unicast, nonzero MAC."""
    m = bytearray(rng.integers(0, 256, 6, dtype=np.uint8).tobytes())
    m[0] = (m[0] & 0xFE) | 0x02
    return bytes(m)


def rand_ip(rng) -> str:
    return "10.%d.%d.%d" % tuple(int(x) for x in rng.integers(1, 255, 3))


# kind -> the counter the frame lands in ("" = counted nowhere, "udp" = not a candidate)
KINDS = {
    "request": "eligible", "request_pad": "eligible", "request_43": "eligible", "probe": "eligible",
    "request_unicast": "eligible", "request_tha_junk": "eligible",
    "short_41": "bad_frame",
    "ipv6": "", "lldp": "",
    "htype_bad": "malformed", "ptype_bad": "malformed", "hlen_bad": "malformed", "plen_bad": "malformed",
    "op_reply": "other_op", "op_rarp": "other_op", "op_zero": "other_op", "op_256": "other_op",
    "own": "own", "sha_mcast": "sender_bad", "sha_bcast": "sender_bad", "sha_zero": "sender_bad",
    "tpa_other": "not_ours", "tpa_zero": "not_ours", "announce_other": "not_ours",
    "conflict": "conflict",
    "udp": "udp",
}


def kind_frame(rng, kind: str) -> bytes:
    sha, spa = rand_mac(rng), rand_ip(rng)
    a = dict(sha=sha, spa=spa)
    if kind == "request":
        return arp_frame(**a)
    if kind == "request_pad":
        return arp_frame(**a, pad_to=60)
    if kind == "request_43":
        return arp_frame(**a, pad_to=43)
    if kind == "probe":                                            # RFC 5227 §2.1.1: sender address 0.0.0.0
        return arp_frame(sha=sha, spa="0.0.0.0", pad_to=60)
    if kind == "request_unicast":                                  # a cache refresh sent to our MAC
        return arp_frame(**a, eth_dst=OUR_MAC, tha=OUR_MAC)
    if kind == "request_tha_junk":
        return arp_frame(**a, tha=rand_mac(rng), eth_dst=rand_mac(rng))
    if kind == "short_41":
        return arp_frame(**a, trunc=41)
    if kind == "ipv6":
        return arp_frame(**a, ethertype=0x86DD, pad_to=60)
    if kind == "lldp":
        return arp_frame(**a, ethertype=0x88CC)
    if kind == "htype_bad":
        return arp_frame(**a, htype=int(rng.choice([0, 6, 0x0100])))
    if kind == "ptype_bad":
        return arp_frame(**a, ptype=int(rng.choice([0x0806, 0x86DD, 0x0008])))
    if kind == "hlen_bad":
        return arp_frame(**a, hlen=int(rng.choice([0, 4, 8])))
    if kind == "plen_bad":
        return arp_frame(**a, plen=int(rng.choice([0, 6, 16])))
    if kind == "op_reply":
        return arp_frame(**a, op=2, tha=OUR_MAC, eth_dst=OUR_MAC)
    if kind == "op_rarp":
        return arp_frame(**a, op=3)
    if kind == "op_zero":
        return arp_frame(**a, op=0)
    if kind == "op_256":                                           # 01 00: the request's bytes swapped
        return arp_frame(**a, op=0x0100)
    if kind == "own":
        return arp_frame(sha=OUR_MAC, spa=spa)
    if kind == "sha_mcast":
        return arp_frame(sha=bytes([sha[0] | 1]) + sha[1:], spa=spa)
    if kind == "sha_bcast":
        return arp_frame(sha=BCAST, spa=spa)
    if kind == "sha_zero":
        return arp_frame(sha=bytes(6), spa=spa, eth_src=sha)
    if kind == "tpa_other":
        return arp_frame(**a, tpa=OTHER_IP)
    if kind == "tpa_zero":
        return arp_frame(**a, tpa="0.0.0.0")
    if kind == "announce_other":                                   # another host's announcement
        return arp_frame(sha=sha, spa=spa, tpa=spa)
    if kind == "conflict":                                         # another host announcing / probing with our address
        return arp_frame(sha=sha, spa=OUR_IP)
    if kind == "udp":
        return udp_frame(rng, payload_len=int(rng.integers(0, 60)))
    raise ValueError(kind)


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


def mixed(seed: int, n: int):
    """n frames of every kind above in random order, frame k at offset == k mod 16:
    (buf, bytes, offset, length, kinds)."""
    rng = np.random.default_rng(seed)
    names = list(KINDS)
    kinds = [names[k] for k in rng.integers(0, len(names), n)]
    fl = [kind_frame(rng, k) for k in kinds]
    buf, nb, off, ln = pack(fl, aligns=[(5 * k) % 16 for k in range(n)])
    return buf, nb, off, ln, kinds


def host_meta(frames, offset, length) -> np.ndarray:
    """Verdict words good enough for the stage, without an RX: NOT_IPV4 for every frame whose
    ethertype is not 0x0800 (or that is too short to have one), DELIVERED otherwise."""
    fr = np.asarray(frames, np.uint8)
    m = np.zeros(len(offset), np.uint32)
    for i, (o, l) in enumerate(zip(offset, length)):
        if l < 14 or fr[int(o) + 12] != 0x08 or fr[int(o) + 13] != 0x00:
            m[i] = V_NOT_IPV4
    return m


# ---- the model ----------------------------------------------------------------------------------
def reply_bytes(sha: bytes, spa: bytes, mac: bytes, ip: bytes) -> bytes:
    """The 42 bytes of the reply to a request from (sha, spa), by the table in udpdk_gpu.h."""
    return sha + mac + bytes.fromhex("08060001080006040002") + mac + ip + sha + spa


def model(frames, frames_bytes, offset, length, meta, *, mac=OUR_MAC, ip=None, max_replies=None) -> dict:
    """slots [replies, 64], origin [replies], stats (every udpdk_arp_stats_t field) and the per-frame
    reason: the counter's name, "" for a candidate counted nowhere, None for a frame that is no candidate."""
    n = len(offset)
    ip = abi.raw_ip(OUR_IP) if ip is None else ip
    ipb = struct.pack("<I", ip)
    max_replies = n if max_replies is None else max_replies
    fr = np.asarray(frames, np.uint8)
    st = {k: 0 for k in STAT_FIELDS}
    reason, answers = [None] * n, []
    for i in range(n):
        if (int(meta[i]) & 0xF) != V_NOT_IPV4:
            continue
        o, l = int(offset[i]), int(length[i])
        if l < 42 or o + l > frames_bytes:
            r = "bad_frame"
        else:
            f = fr[o:o + 42].tobytes()
            sha, spa, tpa = f[22:28], f[28:32], f[38:42]
            if f[12:14] != b"\x08\x06":
                r = ""
            elif f[14:20] != bytes.fromhex("000108000604"):
                r = "malformed"
            elif f[20:22] != b"\x00\x01":
                r = "other_op"
            elif sha == bytes(mac):
                r = "own"
            elif (sha[0] & 1) or sha == bytes(6):
                r = "sender_bad"
            elif tpa != ipb:
                r = "not_ours"
            elif spa == ipb:
                r = "conflict"
            else:
                r = "eligible"
                answers.append((i, reply_bytes(sha, spa, bytes(mac), ipb)))
            if r != "":
                st["arp"] += 1
        reason[i] = r
        if r not in ("", "eligible"):
            st[r] += 1
    st["eligible"] = len(answers)
    st["replies"] = min(len(answers), max_replies)
    st["no_room"] = len(answers) - st["replies"]
    k = st["replies"]
    slots = np.zeros((k, SLOT_BYTES), np.uint8)
    for r, (_, b) in enumerate(answers[:k]):
        slots[r, :FRAME_BYTES] = np.frombuffer(b, np.uint8)
    return {"slots": slots, "origin": np.array([i for i, _ in answers[:k]], np.uint32), "stats": st, "reason": reason,
            "frames_out": [b for _, b in answers]}
