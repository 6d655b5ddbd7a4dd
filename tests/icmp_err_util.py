"""The model of udpdk_gpu_icmp_errors (include/udpdk_gpu.h) in numpy, and builders for the frames its
tests need: destination-unreachable messages quoting datagrams of connected sockets, with every way
of being wrong, on top of tests/icmp_util.py's ip_frame / icmp_msg. A client at OUR_IP owns the
sockets; the errors arrive from routers and peers elsewhere."""
import errno
import struct
from dataclasses import dataclass

import numpy as np

import icmp_util as U
import oracle as O
from udpdk_amd import abi

OUR_IP = U.OUR_IP                       # the stack's address: our_ip
OTHER_IP = U.OTHER_IP                   # a second local address some sockets bind
ROUTER_IP = "10.9.8.7"                  # where most errors come from
STATS = abi.ICMP_ERR_STATS

# Linux's icmp_err_convert as the issue states it: code -> (errno, hard)
TABLE = {0: (errno.ENETUNREACH, 0), 1: (errno.EHOSTUNREACH, 0), 2: (errno.ENOPROTOOPT, 1), 3: (errno.ECONNREFUSED, 1),
         4: (errno.EMSGSIZE, 0), 5: (errno.EOPNOTSUPP, 0), 6: (errno.ENETUNREACH, 1), 7: (errno.EHOSTDOWN, 1),
         8: (errno.ENONET, 1), 9: (errno.ENETUNREACH, 1), 10: (errno.EHOSTUNREACH, 1), 11: (errno.ENETUNREACH, 0),
         12: (errno.EHOSTUNREACH, 0), 13: (errno.EHOSTUNREACH, 1), 14: (errno.EHOSTUNREACH, 1),
         15: (errno.EHOSTUNREACH, 1)}


def table(code: int) -> tuple[int, int]:
    return TABLE.get(code, (0, 0))


# ---- sockets ------------------------------------------------------------------------------------
@dataclass
class Sock:
    fd: int
    ip: str | None                      # None: INADDR_ANY
    port: int                           # host order
    reuse: int = 0
    peer: tuple[str, int] | None = None


def lists_of(socks) -> dict:
    """raw port -> [(ip_raw, sockfd, reuse)]: ANY bindings first, then the specific ones, in the order given."""
    out = {}
    for s in socks:
        out.setdefault(abi.raw_port(s.port), []).append((abi.raw_ip(s.ip) if s.ip else 0, s.fd, s.reuse))
    return {p: [x for x in l if x[0] == 0] + [x for x in l if x[0] != 0] for p, l in out.items()}


def peers_of(socks, n_lanes: int) -> np.ndarray:
    t = np.zeros(n_lanes, abi.PEER_DTYPE)
    for s in socks:
        if s.peer and s.fd < n_lanes:
            t[s.fd] = (abi.raw_ip(s.peer[0]), abi.raw_port(s.peer[1]), 1)
    return t


def sent_frame(rng, s: Sock, payload_len: int = 20, *, our_ip: str = OUR_IP, to=None) -> bytes:
    """The datagram socket s sends to its peer (or to `to`): source = its bound address, or ours for ANY."""
    ip, port = to if to is not None else s.peer
    pay = rng.integers(0, 256, payload_len, dtype=np.uint8).tobytes()
    udp = struct.pack(">HHHH", s.port, port, 8 + payload_len, 0) + pay
    return U.ip_frame(17, udp, src_ip=s.ip or our_ip, dst_ip=ip, ident=int(rng.integers(0, 65536)))


def unreach_frame(quoted: bytes, code: int, *, quote_len: int = 28, typ: int = 3, bad_cksum: bool = False, tl=None,
                  pad_to: int = 0, q_ihl=None, q_proto=None, q_frag=None, src_ip: str = ROUTER_IP,
                  dst_ip: str = OUR_IP, **kw) -> bytes:
    """A destination-unreachable message quoting the first quote_len bytes of the datagram in the
    frame `quoted` from its IPv4 header on (zero-filled past its end). tl overrides the outer total
    length (the checksum still covers the whole message built); q_* override quote fields."""
    q = bytearray(quoted[14:14 + quote_len].ljust(quote_len, b"\0"))
    if q_ihl is not None:
        q[0] = 0x40 | q_ihl
    if q_proto is not None:
        q[9] = q_proto
    if q_frag is not None:
        q[6:8] = struct.pack(">H", q_frag)
    msg = U.icmp_msg(typ, code, 0, 0, bytes(q), bad_cksum)
    return U.ip_frame(1, msg, src_ip=src_ip, dst_ip=dst_ip, tl=tl, pad_to=pad_to, **kw)


# ---- the model ----------------------------------------------------------------------------------
def model(frames, frames_bytes, offset, length, meta, lists, peers, n_lanes, our_ip=None):
    """(err[n_lanes] uint64, stats dict) by the rules of udpdk_gpu_icmp_errors, frame by frame."""
    our_ip = abi.raw_ip(OUR_IP) if our_ip is None else our_ip
    fr = np.asarray(frames, np.uint8)
    err = np.zeros(n_lanes, np.uint64)
    st = dict.fromkeys(STATS, 0)
    u32 = lambda b: int.from_bytes(bytes(b), "little")            # noqa: E731
    for i in range(len(offset)):
        m = int(meta[i])
        if (m & 0xF) != abi.V_NOT_UDP or not (m >> 4) & 1 or (m >> 8) & 1:
            continue
        o, ln = int(offset[i]), int(length[i])
        if ln < 42 or o + ln > frames_bytes:
            st["bad_frame"] += 1
            continue
        f = fr[o:o + ln]
        if f[23] != 1 or f[34] != 3 or u32(f[30:34]) != our_ip:
            continue
        st["errors"] += 1
        tl = int(f[16]) << 8 | int(f[17])
        if tl < 56 or 14 + tl > ln or U.fold(U.word_sum(f[34:14 + tl])) != 0xFFFF:
            st["msg_bad"] += 1
            continue
        if f[42] != 0x45 or f[51] != 17 or ((int(f[48]) << 8 | int(f[49])) & 0x1FFF) != 0:
            st["quote_bad"] += 1
            continue
        code = int(f[35])
        if not table(code)[1]:
            st["soft"] += 1
            continue
        qsrc, qdst, sport, dport = u32(f[54:58]), u32(f[58:62]), u32(f[62:64]), u32(f[64:66])
        hit = 0
        for ip, fd, _ in lists.get(sport, []):
            if fd >= n_lanes or not (ip == qsrc or (ip == 0 and qsrc == our_ip)):
                continue
            p = peers[fd]
            if p["on"] and int(p["ip"]) == qdst and int(p["port"]) == dport:
                err[fd] = max(int(err[fd]), (i + 1) << 8 | code)
                hit += 1
        st["reported"] += hit
        st["no_socket"] += hit == 0
    return err, st


def meta_of(lists, snap_lanes, buf, nb, off, ln):
    return O.rx(O.bindtable_from_lists(lists), buf, nb, off, ln, None, snap_lanes)[0]


# ---- a mixed batch ------------------------------------------------------------------------------
N_LANES = 44                            # what the stage is called with
SNAP_LANES = 64                         # the snapshot's (socket 50 lies between the two)
LAST_FD = 5                             # only "multi" frames quote it: the batch ends with hard, then soft
PAIR = (10, 11)                         # two reuse sockets on one port, connected to the same peer


def sockets() -> list[Sock]:
    s = []
    for fd in range(40):
        if fd in PAIR:
            s.append(Sock(fd, OUR_IP, 21000, 1, ("10.0.0.77", 7077)))    # (two ANY binds of a port are refused)
            continue
        ip = None if fd % 3 else (OUR_IP if fd % 2 else OTHER_IP)
        peer = ("10.0.%d.%d" % (fd // 7, 20 + fd), 5000 + 3 * fd) if fd % 4 != 3 else None
        s.append(Sock(fd, ip, 20000 + fd, 0, peer))
    s.append(Sock(50, None, 20050, 0, ("10.0.50.50", 5050)))      # sockfd >= N_LANES
    return s


KINDS = tuple(f"code{c}" for c in range(17)) + (
    "multi", "bad_cksum", "tl55", "tl_past", "padded", "odd", "long", "q_ihl6", "q_tcp", "q_frag1",
    "wrong_peer_ip", "wrong_peer_port", "src_not_ours", "dst_not_ours", "ip_bad", "echo_req", "echo_rep",
    "udp_open", "udp_closed", "icmp_frag", "unconnected", "fd_high", "pair", "type11")


def kind_frame(rng, kind: str, socks) -> bytes:
    conn = [s for s in socks if s.peer and s.fd < N_LANES and s.fd != LAST_FD and s.fd not in PAIR]
    s = conn[int(rng.integers(0, len(conn)))]
    hard = int(rng.choice([2, 3, 6, 7, 8, 9, 10, 13, 14, 15]))
    q = sent_frame(rng, s, int(rng.integers(0, 64)))
    if kind.startswith("code"):
        return unreach_frame(q, int(kind[4:]))
    if kind == "multi":
        return unreach_frame(sent_frame(rng, socks[LAST_FD]), int(rng.integers(0, 16)))
    if kind == "bad_cksum":
        return unreach_frame(q, hard, bad_cksum=True)
    if kind == "tl55":
        return unreach_frame(q, hard, tl=55)
    if kind == "tl_past":
        return unreach_frame(q, hard, tl=56 + int(rng.integers(1, 9)))
    if kind == "padded":
        return unreach_frame(q, hard, pad_to=70 + int(rng.integers(1, 30)))
    if kind == "odd":
        return unreach_frame(q, hard, quote_len=int(rng.choice([29, 35, 37, 41])))
    if kind == "long":
        return unreach_frame(sent_frame(rng, s, 600), hard, quote_len=int(rng.choice([92, 548, 555])))
    if kind == "q_ihl6":
        return unreach_frame(q, hard, q_ihl=6)
    if kind == "q_tcp":
        return unreach_frame(q, hard, q_proto=6)
    if kind == "q_frag1":
        return unreach_frame(q, hard, q_frag=1)
    if kind == "wrong_peer_ip":
        return unreach_frame(sent_frame(rng, s, to=("10.200.1.1", s.peer[1])), hard)
    if kind == "wrong_peer_port":
        return unreach_frame(sent_frame(rng, s, to=(s.peer[0], s.peer[1] + 1)), hard)
    if kind == "src_not_ours":
        return unreach_frame(sent_frame(rng, Sock(s.fd, "172.31.100.77", s.port, 0, s.peer)), hard)
    if kind == "dst_not_ours":
        return unreach_frame(q, hard, dst_ip=OTHER_IP)
    if kind == "ip_bad":
        return unreach_frame(q, hard, ip_cksum="bad")
    if kind == "echo_req":
        return U.echo_request(rng, int(rng.integers(8, 100)))
    if kind == "echo_rep":
        return U.echo_request(rng, int(rng.integers(8, 100)), typ=0)
    if kind == "udp_open":
        return sent_frame(rng, Sock(0, s.peer[0], s.peer[1]), to=(s.ip or OUR_IP, s.port))
    if kind == "udp_closed":
        return sent_frame(rng, Sock(0, ROUTER_IP, 999), to=(OUR_IP, 7))
    if kind == "icmp_frag":
        return unreach_frame(q, hard, frag=0x2000)
    if kind == "unconnected":
        u = [x for x in socks if not x.peer]
        u = u[int(rng.integers(0, len(u)))]
        return unreach_frame(sent_frame(rng, u, to=("10.3.3.3", 3333)), hard)
    if kind == "fd_high":
        return unreach_frame(sent_frame(rng, socks[-1]), hard)
    if kind == "pair":
        return unreach_frame(sent_frame(rng, socks[PAIR[0]]), hard)
    if kind == "type11":
        return unreach_frame(q, 0, typ=11)
    raise ValueError(kind)


@dataclass
class Mixed:
    buf: np.ndarray
    nb: int
    off: np.ndarray
    ln: np.ndarray
    kinds: list
    meta: np.ndarray
    socks: list
    lists: dict
    peers: np.ndarray


def mixed(seed: int, n: int) -> Mixed:
    """n frames of every kind above in random order at random alignments, ending with a hard and then a
    soft error for socket LAST_FD; the verdict words are the oracle's."""
    rng = np.random.default_rng(seed)
    socks = sockets()
    assert n >= 2 * len(KINDS) + 2
    kinds = list(KINDS) * 2 + [KINDS[k] for k in rng.integers(0, len(KINDS), n - 2 - 2 * len(KINDS))]
    kinds = [kinds[k] for k in rng.permutation(len(kinds))]
    fl = [kind_frame(rng, k, socks) for k in kinds]
    last = sent_frame(rng, socks[LAST_FD])
    fl += [unreach_frame(last, 2), unreach_frame(last, 1)]
    kinds += ["last_hard", "last_soft"]
    buf, nb, off, ln = U.pack(fl, aligns=rng.integers(0, 16, n).tolist())
    lists = lists_of(socks)
    M = Mixed(buf, nb, off, ln, kinds, meta_of(lists, SNAP_LANES, buf, nb, off, ln), socks, lists,
              peers_of(socks, N_LANES))
    for k in KINDS:
        assert kinds.count(k) >= 1, k
    err, st = model(buf, nb, off, ln, M.meta, lists, M.peers, N_LANES)
    assert st["reported"] >= 20, st
    return M
