"""A numpy model of the reply plan (udpdk_gpu_tx_reply_plan) and the expected output image of
udpdk_gpu_tx_reply, for test_tx_reply_ref.py, test_gpu_tx_reply.py and test_gpu_echo_path.py.

The model follows the header's definition entry by entry: the lane lookup with offsets clamped to
D = min(lane_off[n_lanes], lane_cap), the skip rules in their order of precedence, rx_gather's
payload rule with an unbounded slot, and the 64-bit prefix of the spans with the tail that is out
of room. test_tx_reply_ref.py pins its payload, source address and spans to oracle.recv_gather and
udpdk_gpu_tx_span. The frame bytes then come from the oracle (O.tx_frame, O.tx_fragment) and,
with the checksum flag, from the tests' own RFC 768 sum (tx_cksum_util.py). No code is shared with
the library."""
from dataclasses import dataclass, field

import numpy as np

import tx_cksum_util as U

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
FILL = 0xEE                      # the output buffer's fill in abi.tx_reply_run


def span(L: int, mtu: int | None) -> tuple[int, int]:
    """(output bytes, frames) of one datagram of L payload bytes."""
    if mtu and L + 42 > mtu:
        nf = -(-(L + 8) // (mtu - 20))
        return L + 8 + 34 * nf, nf
    return L + 42, 1


@dataclass
class Plan:
    payload_off: np.ndarray
    payload_len: np.ndarray
    sockfd: np.ndarray
    dst_ip: np.ndarray
    dst_port: np.ndarray
    frame_off: np.ndarray        # [count + 1]
    reason: list = field(default_factory=list)     # per entry: "" or why it does not answer
    stats: dict = field(default_factory=dict)


def lane_of(lane_off, n_lanes: int, D: int, p: int) -> int:
    """The largest l < n_lanes with min(lane_off[l], D) <= p."""
    clamped = np.minimum(np.asarray(lane_off[:n_lanes], np.int64), D)
    return max(0, int(np.searchsorted(clamped, p, "right")) - 1)


def plan_model(frames, frames_bytes, offset, length, lane_off, lane_pkt, first, count, *, mtu=0,
               out_cap=1 << 24, lane_sel=None, lane_cap=None, n=None, n_lanes=None) -> Plan:
    n = len(offset) if n is None else n
    n_lanes = len(lane_off) - 1 if n_lanes is None else n_lanes
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    D = min(int(lane_off[n_lanes]), lane_cap)
    clamped = np.minimum(np.asarray(lane_off[:n_lanes], np.int64), D)
    P = Plan(np.zeros(count, np.uint32), np.zeros(count, np.uint16), np.full(count, -1, np.int32),
             np.zeros(count, np.uint32), np.zeros(count, np.uint16), np.zeros(count + 1, np.uint32))
    spans, nfs = np.zeros(count, np.int64), np.zeros(count, np.int64)
    for k in range(count):
        p = first + k
        why = ""
        if p >= D:
            why = "past"
        else:
            i = int(lane_pkt[p])
            if i >= n:
                why = "bad_index"
            elif int(length[i]) < 42 or int(offset[i]) + int(length[i]) > frames_bytes:
                why = "bad_frame"
            else:
                l = max(0, int(np.searchsorted(clamped, p, "right")) - 1)
                if lane_sel is not None and not lane_sel[l]:
                    why = "unselected"
        P.reason.append(why)
        if why:
            continue
        o, ln = int(offset[i]), int(length[i])
        f = frames[o:o + 42]
        dgram_len = (int(f[38]) << 8) | int(f[39])
        L = min(ln - 42, (dgram_len - 8) & 0xFFFF)
        P.payload_off[k], P.payload_len[k], P.sockfd[k] = o + 42, L, l
        P.dst_ip[k] = int.from_bytes(f[26:30].tobytes(), "little")
        P.dst_port[k] = int.from_bytes(f[34:36].tobytes(), "little")
        spans[k], nfs[k] = span(L, mtu)
    pre = np.concatenate([[0], np.cumsum(spans)])            # int64: the 64-bit prefix
    total = int(pre[-1])
    cut = (spans > 0) & (pre[1:] > out_cap)
    end = int(pre[:-1][cut][0]) if cut.any() else total
    if cut.any():                                            # the prefix is monotone: a tail
        kc = int(np.nonzero(cut)[0][0])
        assert cut[kc:][spans[kc:] > 0].all()
    for k in np.nonzero(cut)[0]:
        P.reason[k] = "no_room"
        P.payload_off[k] = P.payload_len[k] = P.dst_ip[k] = P.dst_port[k] = 0
        P.sockfd[k] = -1
    P.frame_off[:] = np.minimum(pre, end)
    replied = int((P.sockfd >= 0).sum())
    P.stats = dict(bytes_needed=total, replied=replied, skipped=count - replied,
                   bad_index=P.reason.count("bad_index"), unselected=P.reason.count("unselected"),
                   no_room=int(cut.sum()), frames=int(nfs[~cut].sum()), end=end)
    return P


def reply_blob(P: Plan, k: int, frames, slots, cfg_ip, mtu, cksum):
    """(output bytes, frames) of entry k's reply: sent by socket sockfd[k] (slots[l] = (ip, port,
    bound), raw) to the request's source, with the request's payload."""
    o, L = int(P.payload_off[k]), int(P.payload_len[k])
    return U.expected(SRC_MAC, DST_MAC, cfg_ip, slots[int(P.sockfd[k])], int(P.dst_ip[k]), int(P.dst_port[k]),
                      frames[o:o + L].tobytes(), mtu or None, cksum)


def image(P: Plan, frames, slots, cfg_ip, mtu, cksum, size):
    """The whole output buffer (size bytes, FILL where nothing is written) and the replies'
    frames in order."""
    want = np.full(size, FILL, np.uint8)
    out_frames = []
    for k in range(len(P.sockfd)):
        if P.sockfd[k] < 0:
            continue
        blob, fr = reply_blob(P, k, frames, slots, cfg_ip, mtu, cksum)
        fo = int(P.frame_off[k])
        assert len(blob) == span(int(P.payload_len[k]), mtu)[0]
        want[fo:fo + len(blob)] = np.frombuffer(blob, np.uint8)
        out_frames += fr
    return want, out_frames


def check_plan(res: dict, P: Plan, count: int, pad: int = 8):
    """The downloaded plan arrays of abi.tx_reply_plan_run / tx_reply_run against the model,
    and the `pad` elements after each still 0xA5."""
    for name in ("sockfd", "payload_len", "payload_off", "dst_ip", "dst_port", "frame_off"):
        got, want = res[name], getattr(P, name)
        m = len(want)
        bad = np.nonzero(got[:m] != want)[0]
        assert bad.size == 0, (f"{name}: {bad.size} differ, first at {int(bad[0])}: got {got[bad[0]]} want "
                               f"{want[bad[0]]} ({P.reason[min(int(bad[0]), count - 1)] or 'answers'})")
        assert np.all(got[m:].view(np.uint8) == 0xA5), f"{name}: written past its end"


def check_stats(st, P: Plan):
    for f in ("bytes_needed", "replied", "skipped", "bad_index", "unselected", "no_room", "frames"):
        assert int(getattr(st, f)) == P.stats[f], (f, int(getattr(st, f)), P.stats[f])
