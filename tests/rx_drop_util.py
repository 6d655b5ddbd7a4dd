"""The numpy model of the RX drop filter (udpdk_gpu_rx_filter / udpdk_gpu_rx_drop), for
test_rx_drop_ref.py (where it is pinned against the oracle) and test_gpu_rx_drop.py:

    keep    = ~any selected reason(meta[lane_pkt])
    new_pkt = lane_pkt[keep]
    new_off = concat([0], cumsum(keep))[lane_off]
"""
from dataclasses import dataclass

import numpy as np

DROP_IP, DROP_UDP, DROP_LEN, DROP_IHL, DROP_ALL = 1, 2, 4, 8, 15
UDP_BAD = 2


def reasons(meta):
    """[4, len(meta)] bool: the verdict word shows the reason of flag 1 << k."""
    m = np.asarray(meta, np.uint32)
    return np.stack([((m >> 4) & 1) == 0, ((m >> 5) & 3) == UDP_BAD, ((m >> 7) & 1) == 1,
                     ((m >> 8) & 1) == 1])


@dataclass
class Filtered:
    lane_off: np.ndarray
    lane_pkt: np.ndarray
    dropped: list          # entries per reason (ip, udp, len, ihl), selected reasons only
    kept: int
    removed: int
    bad_index: int
    truncated: int


def model(meta, lane_off, lane_pkt, flags, n=None, lane_cap=None) -> Filtered:
    """The filter over entries [0, min(lane_off[-1], lane_cap)) of lane_pkt; offsets beyond that
    count as that, entries >= n are removed (bad_index) and counted under no reason."""
    meta = np.asarray(meta, np.uint32)
    lane_off = np.asarray(lane_off, np.uint32).astype(np.int64)
    n = len(meta) if n is None else n
    lane_cap = len(lane_pkt) if lane_cap is None else lane_cap
    d = int(min(lane_off[-1], lane_cap))
    pkt = np.asarray(lane_pkt, np.uint32)[:d]
    valid = pkt < n
    r = np.zeros((4, d), bool)
    r[:, valid] = reasons(meta[pkt[valid]])
    sel = np.array([(flags >> k) & 1 for k in range(4)], bool)
    r &= sel[:, None]
    keep = valid & ~r.any(axis=0)
    pre = np.concatenate([[0], np.cumsum(keep)])
    new_off = pre[np.minimum(lane_off, d)].astype(np.uint32)
    kept = int(keep.sum())
    return Filtered(new_off, pkt[keep], [int(x) for x in r.sum(axis=1)], kept, d - kept,
                    int((~valid).sum()), int(lane_off[-1] > lane_cap))
