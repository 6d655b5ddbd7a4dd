"""A numpy model of the segment plan (udpdk_gpu_tx_segment_plan) and the expected output image of
udpdk_gpu_tx_segment, for test_gso_ref.py, test_gpu_tx_segment.py and test_gpu_gso_path.py.

The model follows the header's definition send by send: the skip rules in their order of precedence,
the segment count, the two prefixes in 64 bits with the tail that is out of room, the placement of
every segment and the -1 padding up to max_segs. The frame bytes then come from the oracle
(O.tx_frame, O.tx_fragment) and, with the checksum flag, from the tests' own RFC 768 sum
(tx_cksum_util.py) over the model's expanded descriptors. No code is shared with the library."""
from dataclasses import dataclass, field

import numpy as np

import tx_cksum_util as U

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
FILL = 0xEE                      # the output buffer's fill in abi.tx_segment_run
MAX_PAYLOAD = 65507
REASONS = ("skipped", "too_long", "bad_range", "too_many", "no_room")


def span(L: int, mtu: int | None) -> tuple[int, int]:
    """(output bytes, frames) of one datagram of L payload bytes (udpdk_gpu_tx_span: an mtu the
    build refuses, below 68 or with mtu - 20 no multiple of 8, counts as none)."""
    if mtu and mtu >= 68 and (mtu - 20) % 8 == 0 and L + 42 > mtu:
        nf = -(-(L + 8) // (mtu - 20))
        return L + 8 + 34 * nf, nf
    return L + 42, 1


def seg_lengths(L: int, g: int) -> list[int]:
    """The segments of one send: one datagram when g == 0 or L <= g (an empty one for L == 0), else
    full segments of g bytes and the remainder."""
    if g == 0 or L <= g:
        return [L]
    return [min(g, L - t * g) for t in range(-(-L // g))]


def send_span(L: int, g: int, mtu: int | None) -> tuple[int, int, int]:
    """(output bytes, segments, frames) of one send, summed over its segments."""
    sp = [span(x, mtu) for x in seg_lengths(L, g)]
    return sum(s for s, _ in sp), len(sp), sum(f for _, f in sp)


def make_sends(rows) -> dict:
    """rows: (payload_off, payload_len, gso_size, sockfd, dst_ip, dst_port) per send -> the dict of
    arrays abi.tx_segment_plan_run takes."""
    cols = list(zip(*rows)) if rows else [[]] * 6
    dts = (np.uint32, np.uint16, np.uint16, np.int32, np.uint32, np.uint16)
    names = ("payload_off", "payload_len", "gso_size", "sockfd", "dst_ip", "dst_port")
    return {n: np.array(c, dt) for n, c, dt in zip(names, cols, dts)}


@dataclass
class Plan:
    payload_off: np.ndarray      # [max_segs]
    payload_len: np.ndarray
    sockfd: np.ndarray
    dst_ip: np.ndarray
    dst_port: np.ndarray
    frame_off: np.ndarray        # [max_segs + 1]
    seg_off: np.ndarray          # [k + 1]
    reason: list = field(default_factory=list)     # per send: "" or why it has no segments
    stats: dict = field(default_factory=dict)


def plan_model(sends: dict, payload_bytes: int, max_segs: int, *, mtu=0, seg_limit=0, out_cap=1 << 24) -> Plan:
    k = len(sends["payload_off"])
    nseg, spans, nfs, reason = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64), []
    for j in range(k):
        off, L, g = int(sends["payload_off"][j]), int(sends["payload_len"][j]), int(sends["gso_size"][j])
        why = ""
        if int(sends["sockfd"][j]) < 0:
            why = "skipped"
        elif L > MAX_PAYLOAD:
            why = "too_long"
        elif off + L > payload_bytes:
            why = "bad_range"
        elif seg_limit and len(seg_lengths(L, g)) > seg_limit:
            why = "too_many"
        reason.append(why)
        if not why:
            spans[j], nseg[j], nfs[j] = send_span(L, g, mtu)
    # room: both prefixes over every send the rules above let through (int64: the 64-bit prefixes)
    pre_s = np.concatenate([[0], np.cumsum(nseg)])
    pre_b = np.concatenate([[0], np.cumsum(spans)])
    cut = (nseg > 0) & ((pre_s[1:] > max_segs) | (pre_b[1:] > out_cap))
    if cut.any():                                            # the prefixes are monotone: a tail
        jc = int(np.nonzero(cut)[0][0])
        assert cut[jc:][nseg[jc:] > 0].all()
    for j in np.nonzero(cut)[0]:
        reason[j] = "no_room"
    fit = np.where(cut, 0, nseg)
    seg_off = np.concatenate([[0], np.cumsum(fit)])
    N = int(seg_off[-1])
    P = Plan(np.zeros(max_segs, np.uint32), np.zeros(max_segs, np.uint16), np.full(max_segs, -1, np.int32),
             np.zeros(max_segs, np.uint32), np.zeros(max_segs, np.uint16), np.zeros(max_segs + 1, np.uint32),
             seg_off.astype(np.uint32), reason)
    fo = 0
    for j in range(k):
        if not fit[j]:
            continue
        off, L, g = int(sends["payload_off"][j]), int(sends["payload_len"][j]), int(sends["gso_size"][j])
        for t, sl in enumerate(seg_lengths(L, g)):
            m = int(seg_off[j]) + t
            P.payload_off[m], P.payload_len[m] = off + t * g if t else off, sl
            P.sockfd[m], P.dst_ip[m], P.dst_port[m] = sends["sockfd"][j], sends["dst_ip"][j], sends["dst_port"][j]
            P.frame_off[m] = fo
            fo += span(sl, mtu)[0]
    P.frame_off[N:] = fo                                     # where the output ends, and the padding
    P.stats = dict(bytes_needed=int(pre_b[-1]), segs_needed=int(pre_s[-1]), sends=int((fit > 0).sum()), segments=N,
                   frames=int(nfs[fit > 0].sum()), end=fo, **{r: reason.count(r) for r in REASONS})
    return P


def image(P: Plan, payload, slots, cfg_ip, mtu, cksum, size):
    """The whole output buffer (size bytes, FILL where nothing is written) and the segments' frames
    in order: segment m is sent by socket sockfd[m] (slots[s] = (ip, port, bound), raw)."""
    want = np.full(size, FILL, np.uint8)
    out_frames = []
    for m in range(len(P.sockfd)):
        if P.sockfd[m] < 0:
            continue
        o, L = int(P.payload_off[m]), int(P.payload_len[m])
        blob, fr = U.expected(SRC_MAC, DST_MAC, cfg_ip, slots[int(P.sockfd[m])], int(P.dst_ip[m]), int(P.dst_port[m]),
                              payload[o:o + L].tobytes(), mtu or None, cksum)
        fo = int(P.frame_off[m])
        assert len(blob) == span(L, mtu)[0]
        want[fo:fo + len(blob)] = np.frombuffer(blob, np.uint8)
        out_frames += fr
    return want, out_frames


def check_plan(res: dict, P: Plan):
    """The downloaded arrays of abi.tx_segment_plan_run / tx_segment_run against the model, and the
    pad elements after each still 0xA5."""
    for name in ("seg_off", "sockfd", "payload_len", "payload_off", "dst_ip", "dst_port", "frame_off"):
        got, want = res[name], getattr(P, name)
        m = len(want)
        bad = np.nonzero(got[:m] != want)[0]
        assert bad.size == 0, (f"{name}: {bad.size} differ, first at {int(bad[0])}: got {got[bad[0]]} want "
                               f"{want[bad[0]]} (N {P.stats['segments']})")
        assert np.all(got[m:].view(np.uint8) == 0xA5), f"{name}: written past its end"


def check_stats(st, P: Plan):
    for f in ("bytes_needed", "segs_needed", "sends", "segments", "frames") + REASONS:
        assert int(getattr(st, f)) == P.stats[f], (f, int(getattr(st, f)), P.stats[f])
