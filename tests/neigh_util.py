"""The model of the neighbour cache (include/udpdk_gpu.h: udpdk_gpu_neigh_learn, udpdk_gpu_neigh_resolve) as
a serial walk in plain Python: the table is a dict raw ip -> [mac, state, stamp] with a capacity, learning is
rules 1-9, resolution rules R1-R5 with the request list. Frame builders come from arp_util."""
import socket
import struct

import numpy as np

import arp_util as A
from udpdk_amd import abi

OUR_IP, OUR_MAC = A.OUR_IP, A.OUR_MAC
FALLBACK_MAC = bytes.fromhex("6805ca95fa64")
EMPTY, INCOMPLETE, REACHABLE, STATIC = range(4)
LEARN_FIELDS, RESOLVE_FIELDS = abi.NEIGH_LEARN_STATS, abi.NEIGH_RESOLVE_STATS
CLASS_NAMES = ("skipped", "bcast", "mcast", "no_route", "self", "hit", "expired", "incomplete", "inserted", "table_full")
MISS = ("expired", "incomplete", "inserted", "table_full")
BCAST_MAC = b"\xff" * 6
U32 = 0xFFFFFFFF


def raw(ip) -> int:
    return abi.raw_ip(ip) if isinstance(ip, str) else int(ip)


def dotted(r: int) -> str:
    return socket.inet_ntoa(struct.pack("<I", r))


def cfg(*, src_ip=OUR_IP, src_mac=OUR_MAC, netmask=0, gateway=0, fallback_mac=FALLBACK_MAC, ttl_ms=30000,
        retrans_ms=1000, flags=0) -> abi.NeighCfg:
    return abi.neigh_cfg(src_ip, src_mac, netmask=netmask, gateway=gateway, fallback_mac=fallback_mac, ttl_ms=ttl_ms,
                         retrans_ms=retrans_ms, flags=flags)


def home(ip_raw: int, entries: int) -> int:
    """The home slot of a key (the statement in udpdk_gpu.h)."""
    return ((ip_raw * abi.NEIGH_HASH_K) & U32) >> (32 - entries.bit_length() + 1)


def colliding_ips(entries: int, slot: int, count: int, start: int = 1) -> list[str]:
    """`count` addresses 10.77.x.y whose home slot is `slot`."""
    out, k = [], start
    while len(out) < count:
        ip = "10.77.%d.%d" % (k >> 8 & 255, k & 255)
        if home(raw(ip), entries) == slot:
            out.append(ip)
        k += 1
    return out


class Table:
    """ip -> [mac, state, stamp]; a key, once in, stays (kernels never delete)."""

    def __init__(self, entries: int, init=()):
        self.entries = entries
        self.d = {}
        for ip, mac, state, stamp in init:
            self.d[raw(ip)] = [bytes(mac), state, stamp]

    def free(self) -> int:
        return self.entries - len(self.d)

    def as_map(self) -> dict:
        return {k: tuple(v) for k, v in self.d.items()}

    def tuples(self):
        return [(k, v[0], v[1], v[2]) for k, v in self.d.items()]


# ---- learning -------------------------------------------------------------------------------------
def learn_reason(f: bytes, c: abi.NeighCfg):
    """Steps 3-6 for the 42 bytes of a candidate past the frame gate: "" (counted nowhere), a counter, or None
    with the event (sip raw, sha, creating)."""
    if f[12:14] != b"\x08\x06":
        return "", None
    if f[14:20] != bytes.fromhex("000108000604"):
        return "malformed", None
    op = struct.unpack(">H", f[20:22])[0]
    if op not in (1, 2):
        return "other_op", None
    sha, spa, tpa = f[22:28], struct.unpack("<I", f[28:32])[0], struct.unpack("<I", f[38:42])[0]
    if sha == bytes(c.src_mac) or (sha[0] & 1) or sha == bytes(6):
        return "sender_bad", None
    if spa in (0, c.src_ip, U32) or (spa & 0xF0) == 0xE0:
        return "sender_bad", None
    return None, (spa, sha, op == 1 and tpa == c.src_ip)


def learn(tab: Table, c: abi.NeighCfg, frames, frames_bytes, offset, length, meta, now: int) -> dict:
    """Applies a batch to `tab` in frame order; returns the counts and the per-frame reason (None: no candidate)."""
    fr = np.asarray(frames, np.uint8)
    st = {k: 0 for k in LEARN_FIELDS}
    reason = [None] * len(offset)
    for i in range(len(offset)):
        if (int(meta[i]) & 0xF) != A.V_NOT_IPV4:
            continue
        o, l = int(offset[i]), int(length[i])
        if l < 42 or o + l > frames_bytes:
            r = "bad_frame"
        else:
            r, ev = learn_reason(fr[o:o + 42].tobytes(), c)
            if r != "":
                st["arp"] += 1
            if r is None:
                ip, sha, creating = ev
                e = tab.d.get(ip)
                if e is not None and e[1] == STATIC:
                    r = "static_kept"
                elif e is not None:
                    r = "refreshed" if (e[0] == sha and e[1] == REACHABLE) else "updated"
                    e[:] = [sha, REACHABLE, now]
                elif creating:
                    if tab.free() > 0:
                        tab.d[ip] = [sha, REACHABLE, now]
                        r = "created"
                    else:
                        r = "full"
                else:
                    r = "ignored"
        reason[i] = r
        if r:
            st[r] += 1
    return {"stats": st, "reason": reason}


# ---- resolution -----------------------------------------------------------------------------------
def classify(c: abi.NeighCfg, dst: int):
    """Rules R1-R4: (class name or "lookup", next hop, mac)."""
    onlink = ((dst ^ c.src_ip) & c.netmask) == 0
    if dst == U32 or (c.netmask != 0 and onlink and (dst | c.netmask) == U32):
        return "bcast", 0, BCAST_MAC
    b = struct.pack("<I", dst)
    if 224 <= b[0] <= 239:
        return "mcast", 0, bytes([0x01, 0x00, 0x5E, b[1] & 0x7F, b[2], b[3]])
    h = dst if onlink else c.gateway
    if h == 0:
        return "no_route", 0, bytes(6)
    if h == c.src_ip:
        return "self", h, bytes(c.src_mac)
    return "lookup", h, bytes(6)


def request_bytes(c: abi.NeighCfg, h: int) -> bytes:
    mac, ip = bytes(c.src_mac), struct.pack("<I", c.src_ip)
    return BCAST_MAC + mac + bytes.fromhex("08060001080006040001") + mac + ip + bytes(6) + struct.pack("<I", h)


def resolve(tab: Table, c: abi.NeighCfg, dst_ip, sockfd, now: int, req_cap=None) -> dict:
    """Applies a TX batch to `tab` in index order: dmac [n, 2] (uint32), sockfd_out, state, the request slots
    [requests, 64], their origins and next hops, and the counts."""
    n = len(dst_ip)
    req_cap = n if req_cap is None else req_cap
    fb = bool(c.flags & abi.NEIGH_FALLBACK)
    retrans = max(int(c.retrans_ms), 1)
    st = {k: 0 for k in RESOLVE_FIELDS}
    dmac, so, state = np.zeros((n, 2), np.uint32), np.array(sockfd, np.int32).copy(), np.zeros(n, np.uint8)
    asked = []                                                     # (first asking index, next hop)
    for i in range(n):
        mac = bytes(6)
        if int(sockfd[i]) < 0:
            cls = "skipped"
        else:
            cls, h, mac = classify(c, int(dst_ip[i]))
            if cls == "no_route":
                so[i] = -1
            elif cls == "lookup":
                e, ask = tab.d.get(h), False
                if e is not None and (e[1] == STATIC or (e[1] == REACHABLE and ((now - e[2]) & U32) <= c.ttl_ms)):
                    cls, mac = "hit", e[0]
                elif e is not None and e[1] == REACHABLE:
                    cls, ask = "expired", True
                    e[1], e[2] = INCOMPLETE, now & U32
                elif e is not None:
                    cls = "incomplete"
                    ask = ((now - e[2]) & U32) >= retrans
                    if ask:
                        e[2] = now & U32
                elif tab.free() > 0:
                    cls, ask = "inserted", True
                    tab.d[h] = [bytes(6), INCOMPLETE, now & U32]
                else:
                    cls = "table_full"
                if ask and all(a[1] != h for a in asked):
                    asked.append((i, h))
                if cls in MISS:
                    if fb:
                        mac = bytes(c.fallback_mac)
                        st["fallback"] += 1
                    else:
                        so[i] = -1
                        st["unresolved"] += 1
        st[cls] += 1
        state[i] = CLASS_NAMES.index(cls)
        dmac[i] = struct.unpack("<II", mac + b"\0\0")
    k = min(len(asked), req_cap)
    st["requests"], st["no_room"] = k, len(asked) - k
    req = np.zeros((k, A.SLOT_BYTES), np.uint8)
    for r, (_, h) in enumerate(asked[:k]):
        req[r, :42] = np.frombuffer(request_bytes(c, h), np.uint8)
    return {"dmac": dmac, "sockfd_out": so, "state": state, "req": req, "stats": st,
            "req_origin": np.array([i for i, _ in asked[:k]], np.uint32), "req_hops": [h for _, h in asked]}
