"""The RX drop filter's numpy model (rx_drop_util.py) pinned against the oracle, which the GPU tests
(test_gpu_rx_drop.py) then use as their reference, and the socket layer's configuration entry
point. No GPU needed."""
import errno

import numpy as np
import pytest

import oracle as O
import rx_drop_util as U
from test_gpu_rx import IP1, IP9, MIXED_LISTS
from udpdk_amd import abi, frames as F

N_LANES = 8


def mixed(seed):
    return F.mixed_batch(seed, 3000, [10001, 10002, 10003, 10004, 10005], [9, 20000, 65535], [IP1, IP9])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_equals_oracle_on_remaining_frames(seed):
    """Filtering the lanes of a batch = receiving the batch without the dropped frames: for each
    flag set the frames showing a selected reason are taken out of the batch, the oracle runs on
    the rest, and its lanes, mapped back through the kept frame indices, are the model's."""
    b = mixed(seed)
    bt = O.bindtable_from_lists(MIXED_LISTS)
    meta, loff, lpkt, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset, b.length, None, N_LANES)
    lane_of = np.repeat(np.arange(N_LANES), np.diff(loff.astype(np.int64)))
    for flags in (1, 2, 4, 8, 3, 15):
        m = U.model(meta, loff, lpkt, flags)
        sel = np.array([(flags >> k) & 1 for k in range(4)], bool)
        gone = (U.reasons(meta) & sel[:, None]).any(axis=0)
        kept_idx = np.flatnonzero(~gone)
        _, loff2, lpkt2, _ = O.rx(bt, b.frames, b.frames_bytes, b.offset[kept_idx], b.length[kept_idx],
                                  None, N_LANES)
        assert np.array_equal(loff2, m.lane_off), (seed, flags)
        assert np.array_equal(kept_idx[lpkt2], m.lane_pkt), (seed, flags)
        assert m.kept == int(loff2[N_LANES]) and m.removed == int(loff[N_LANES]) - m.kept
        assert m.bad_index == 0 and m.truncated == 0
        # the batch exercises the flag set: every selected reason drops entries, in most lanes
        for k in range(4):
            assert (m.dropped[k] > 0) == bool(sel[k]), (seed, flags, k)
        lost = np.unique(lane_of[gone[lpkt]])
        assert len(lost) >= 5, (seed, flags, lost)
    # the oracle marks every LEN_BAD delivery UDP BAD as well: flag 4 selects a subset of flag 2
    r = U.reasons(meta[lpkt])
    assert np.all(r[1][r[2]])
    assert np.array_equal(U.model(meta, loff, lpkt, 6).lane_pkt, U.model(meta, loff, lpkt, 2).lane_pkt)


def test_model_bounds():
    """Entries >= n, offsets past the entries and a total past lane_cap, in the model itself."""
    meta = np.array([0x30, 0x50, 0x30, 0x1B0], np.uint32)       # ok, udp bad, ok, len bad + ihl
    pkt = np.array([0, 1, 9, 2, 3, 1, 0], np.uint32)
    m = U.model(meta, [0, 2, 2, 9], pkt, 2, lane_cap=6)
    assert list(m.lane_pkt) == [0, 2, 3] and list(m.lane_off) == [0, 1, 1, 3]
    assert (m.kept, m.removed, m.bad_index, m.truncated, m.dropped) == (3, 3, 1, 1, [0, 2, 0, 0])
    m = U.model(meta, [0, 7], pkt, 0)
    assert list(m.lane_pkt) == [0, 1, 2, 3, 1, 0] and m.bad_index == 1


def test_config_rx_drop_round_trips(host_api):
    """udpdk_config_rx_drop: default 0, returns the previous flags, a negative argument only
    queries, a bit outside the four is EINVAL and changes nothing, udpdk_host_reset restores 0."""
    assert "udpdk_config_rx_drop" in abi.declared_symbols() and "udpdk_rx_dropped" in abi.declared_symbols()
    assert host_api.config_rx_drop(-1) == 0
    assert host_api.config_rx_drop(abi.RX_DROP_UDP_CKSUM) == 0
    assert host_api.config_rx_drop(-1) == 2
    assert host_api.config_rx_drop(abi.RX_DROP_ALL) == 2
    assert host_api.config_rx_drop(16) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_rx_drop(17) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_rx_drop(-1) == 15
    assert host_api.config_rx_drop(0) == 15
    assert host_api.config_rx_drop(-1) == 0
    host_api.config_rx_drop(5)
    host_api.reset()
    assert host_api.config_rx_drop(-1) == 0
    assert host_api.rx_dropped() == 0
