"""udpdk_gpu_tx_segment_plan / udpdk_gpu_tx_segment on the GPU against the numpy model and the
oracle's frames (tests/tx_gso_util.py, pinned to hand-derived vectors in test_gso_ref.py).

The harness: the plan arrays and seg_off are 8 elements longer than the call may write and
pre-filled with 0xA5 bytes, the output buffer is pre-filled with 0xEE and 4096 bytes longer than
out_cap; every downloaded byte is compared (descriptors, offsets, frames, fill), and the stats with
the model's. S = segments per workgroup, B = sends per workgroup (udpdk_gpu_tx_segment_geometry)."""
import ctypes as C
import errno

import numpy as np
import pytest

import tx_gso_util as G
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

CFG_IP = abi.raw_ip("172.31.100.2")
GUARD = 4096
N_SOCK = 4
PBYTES = 8192                                        # the payload buffer, + 16 bytes of tailroom
PAYLOAD = np.random.default_rng(11).integers(0, 256, PBYTES + 16, dtype=np.uint8)
SLOTS = [(0 if l & 1 else abi.raw_ip(f"10.0.0.{l + 1}"), abi.raw_port(20000 + l), 1) for l in range(N_SOCK)]
B, S, _, _ = abi.tx_segment_geometry(1, 1)


def _cfg():
    return abi.TxConfig((C.c_uint8 * 6)(*G.SRC_MAC), (C.c_uint8 * 6)(*G.DST_MAC), CFG_IP)


def _send(j, off, ln, g, sock=None):
    """Send j: socket j mod 4, a destination of its own."""
    return (off, ln, g, j % N_SOCK if sock is None else sock, abi.raw_ip(f"10.1.{j >> 8}.{j & 255}"),
            abi.raw_port(30000 + j))


def _by_nseg(counts, g=8):
    """One send per entry of counts with that many segments of g bytes (the last one g - 3, so every
    send with more than one segment has a remainder), at offsets that wander over the buffer."""
    rows, off = [], 3
    for j, c in enumerate(counts):
        ln = c * g - 3
        if off + ln > PBYTES:
            off = j % 5
        rows.append(_send(j, off, ln, g))
        off += 7
    return G.make_sends(rows)


def _fill(N, first=40):
    """Segment counts that sum to N: `first`, then 64-segment sends, then the remainder: from the
    second tile on, a 64-segment send straddles every tile edge (S is a multiple of 64, first is not)."""
    counts = [min(first, N)]
    while sum(counts) < N:
        counts.append(min(64, N - sum(counts)))
    return counts


def _run_both(ctx, sends, max_segs, *, mtu=1500, flags=0, seg_limit=0, out_cap=None, pbytes=PBYTES):
    """Plan alone and the full call, each against the model; returns the model."""
    ctx.upload_snapshot(abi.snapshot_from_lists({}, N_SOCK, slots=SLOTS))
    P0 = G.plan_model(sends, pbytes, max_segs, mtu=mtu, seg_limit=seg_limit)
    out_cap = P0.stats["end"] + 64 if out_cap is None else out_cap
    P = G.plan_model(sends, pbytes, max_segs, mtu=mtu, seg_limit=seg_limit, out_cap=out_cap)
    want_rc = -errno.ENOSPC if P.stats["no_room"] else 0
    res = abi.tx_segment_plan_run(ctx, PAYLOAD, pbytes, sends, max_segs, mtu=mtu, seg_limit=seg_limit, out_cap=out_cap)
    assert res["rc"] == 0
    G.check_plan(res, P)
    rc, st = abi.tx_segment_stats(ctx)
    assert rc == want_rc
    G.check_stats(st, P)
    res = abi.tx_segment_run(ctx, _cfg(), PAYLOAD, pbytes, sends, max_segs, mtu=mtu, flags=flags, seg_limit=seg_limit,
                             out_cap=out_cap, guard=GUARD)
    assert res["rc"] == 0
    G.check_plan(res, P)
    rc, st = abi.tx_segment_stats(ctx)
    assert rc == want_rc
    G.check_stats(st, P)
    want, frames = G.image(P, PAYLOAD, SLOTS, CFG_IP, mtu, bool(flags & abi.TX_UDP_CKSUM), out_cap + GUARD)
    bad = np.nonzero(res["out"] != want)[0]
    assert bad.size == 0, f"{bad.size} output bytes differ, the first at {int(bad[0])} (end {P.stats['end']})"
    assert len(frames) == P.stats["frames"]
    return P


# ---- one send ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM])
@pytest.mark.parametrize("ln,g", [(99, 100), (100, 100), (101, 100), (6400, 100), (0, 100), (500, 0), (64, 1)])
def test_one_send(gpu_ctx, ln, g, flags):
    """len < g, == g, == g + 1, == 64 g; an empty send; no segment size; g == 1 (43-byte frames at
    odd offsets). max_segs leaves five padding slots."""
    sends = G.make_sends([_send(0, 5, ln, g)])
    nseg = len(G.seg_lengths(ln, g))
    P = _run_both(gpu_ctx, sends, nseg + 5, flags=flags)
    assert P.stats["segments"] == nseg and P.stats["sends"] == 1 and list(P.sockfd[nseg:]) == [-1] * 5


@pytest.mark.parametrize("mtu,g", [(0, 1473), (1500, 1472), (1500, 1473), (580, 600)])
@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM])
def test_mtu(gpu_ctx, mtu, g, flags):
    """No mtu; an exact fit; every full segment two fragments (the remainder one); a small mtu."""
    sends = G.make_sends([_send(0, 1, 3 * g + 54, g), _send(1, 2, 2 * g, g), _send(2, 64, 100, 0)])
    P = _run_both(gpu_ctx, sends, 8, mtu=mtu, flags=flags)
    assert P.stats["segments"] == 7
    assert P.stats["frames"] == {(0, 1473): 7, (1500, 1472): 7, (1500, 1473): 12, (580, 600): 12}[(mtu, g)]


# ---- tile edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [S - 1, S, S + 1, 2 * S + 1])
def test_segment_tile_edges(gpu_ctx, N):
    P = _run_both(gpu_ctx, _by_nseg(_fill(N)), N)                # max_segs == N: no padding at all
    assert P.stats["segments"] == N
    P = _run_both(gpu_ctx, _by_nseg(_fill(N)), N + 3, mtu=0)
    assert P.stats["segments"] == N


@pytest.mark.parametrize("lead", [[1], [63], [1] * 63, [2, 61]])
def test_full_send_off_the_wave_boundary(gpu_ctx, lead):
    """One 64-segment send that starts at lane 1 and at lane 63 of a wave, behind one send or many."""
    P = _run_both(gpu_ctx, _by_nseg(lead + [64, 2]), sum(lead) + 66 + 4)
    assert P.stats["segments"] == sum(lead) + 66


def test_many_sends_in_a_wave(gpu_ctx):
    """1-2 segment sends, some skipped in between: every wave holds more than two sends, and a wave's
    first and last send have sends without segments between and around them."""
    counts = [1 + (j * 7 % 3 != 0) for j in range(300)]
    sends = _by_nseg(counts)
    sends["sockfd"][[0, 5, 6, 7, 100, 101, 299]] = -1
    sends["payload_len"][[40, 41]] = 0                          # empty sends: one empty datagram each
    P = _run_both(gpu_ctx, sends, 2 * 300)
    assert P.stats["skipped"] == 7 and P.stats["sends"] == 293
    # a wave of exactly two sends with one skipped between them
    sends = _by_nseg([30, 5, 34])
    sends["sockfd"][1] = -1
    P = _run_both(gpu_ctx, sends, 64)
    assert list(P.seg_off) == [0, 30, 30, 64]


@pytest.mark.parametrize("K", [B - 1, B, B + 1])
def test_send_tile_edges(gpu_ctx, K):
    counts = [1] * K
    for j in (0, B - 3, K - 1):
        counts[j] = 3
    P = _run_both(gpu_ctx, _by_nseg(counts), K + 6 + 2, mtu=0)
    assert P.stats["segments"] == K + 6 and P.stats["sends"] == K


# ---- skip rules ----------------------------------------------------------------------------------
def _bad(kind, j):
    return {"skipped": _send(j, 0, 100, 10, sock=-1), "too_long": _send(j, 0, 65508, 0),
            "bad_range": _send(j, PBYTES - 99, 100, 10), "too_many": _send(j, 0, 650, 10)}[kind]


@pytest.mark.parametrize("kind", ["skipped", "too_long", "bad_range", "too_many"])
def test_skip_reason_alone(gpu_ctx, kind):
    rows = [_send(0, 0, 100, 10), _bad(kind, 1), _send(2, PBYTES - 100, 100, 10)]
    P = _run_both(gpu_ctx, G.make_sends(rows), 24, seg_limit=64)
    assert P.reason == ["", kind, ""] and P.stats[kind] == 1 and P.stats["segments"] == 20
    P = _run_both(gpu_ctx, G.make_sends([_bad(kind, 0)]), 4, seg_limit=64)        # nothing at all comes out
    assert P.stats["segments"] == 0 and P.stats["end"] == 0 and P.stats["sends"] == 0


def test_skip_precedence_and_mix(gpu_ctx):
    rows = [_send(0, 0, 65508, 0, sock=-1),                     # skipped before too_long
            _send(1, PBYTES, 65508, 1),                         # too_long before bad_range and too_many
            _send(2, PBYTES - 10, 100, 1),                      # bad_range before too_many
            _send(3, 0, 640, 10),                               # 64 segments: within seg_limit 64
            _send(4, 0, 641, 10),                               # 65: too_many
            _send(5, PBYTES - 1, 1, 1),                         # the buffer's last byte
            _send(6, PBYTES, 0, 0),                             # an empty send at the buffer's end
            _send(7, 0, 100, 10)]                               # out of room (max_segs)
    P = _run_both(gpu_ctx, G.make_sends(rows), 70, seg_limit=64)
    assert P.reason == ["skipped", "too_long", "bad_range", "", "too_many", "", "", "no_room"]
    assert P.stats["segments"] == 66
    # bad_range is judged against payload_bytes, not against the allocation
    P = _run_both(gpu_ctx, G.make_sends(rows[5:7]), 4, pbytes=PBYTES - 1)
    assert P.reason == ["bad_range", "bad_range"]


@pytest.mark.parametrize("seg_limit", [0, 64])
def test_seg_limit(gpu_ctx, seg_limit):
    rows = [_send(0, 0, 64, 1), _send(1, 9, 65, 1), _send(2, 0, 130, 1)]
    P = _run_both(gpu_ctx, G.make_sends(rows), 300, seg_limit=seg_limit)
    assert P.stats["too_many"] == (2 if seg_limit else 0) and P.stats["segments"] == (64 if seg_limit else 259)


def _room_cases():
    K = 2 * B + 10
    return K, [("first", 5), ("last", 2 * B + 5), ("edge", B), ("send0", 0)]


@pytest.mark.parametrize("cause", ["max_segs", "out_cap"])
@pytest.mark.parametrize("where,jc", _room_cases()[1], ids=[w for w, _ in _room_cases()[1]])
def test_no_room(gpu_ctx, cause, where, jc):
    """Room ends in the first workgroup, in the last, at the first send of a workgroup and at send 0;
    exactly on a send boundary, and one short of the next one (the send is never split)."""
    K, _ = _room_cases()
    sends = _by_nseg([2] * K, g=10)                             # every send: 2 segments, 52 + 49 bytes
    sends["sockfd"][[jc + 1, K - 1]] = -1                       # skipped ones in the tail stay `skipped`
    full = G.plan_model(sends, PBYTES, 2 * K, mtu=0)
    for slack in (0, 1):                                        # room for sends [0, jc), and 1 more unit
        if cause == "max_segs":
            P = _run_both(gpu_ctx, sends, max(1, 2 * jc + slack), mtu=0, out_cap=full.stats["end"])
        else:
            P = _run_both(gpu_ctx, sends, 2 * K, mtu=0, out_cap=101 * jc + 100 * slack)
        if cause == "max_segs" and jc == 0 and slack == 0:
            continue                                            # (max_segs 0 is refused: that was max_segs 1)
        assert P.stats["sends"] == jc and P.stats["segments"] == 2 * jc and P.stats["end"] == 101 * jc
        assert P.stats["no_room"] == K - jc - 2 and P.stats["skipped"] == 2
        assert P.stats["bytes_needed"] == 101 * (K - 2) and P.stats["segs_needed"] == 2 * (K - 2)


def test_padding_is_not_built(gpu_ctx):
    """max_segs far above N: the slots are -1 and tx_build writes nothing for them (the image check
    covers the output's end and the guard)."""
    P = _run_both(gpu_ctx, _by_nseg([3, 1, 64]), 68 + 2 * S + 7, flags=abi.TX_UDP_CKSUM)
    assert P.stats["segments"] == 68 and (P.sockfd[68:] == -1).all() and (P.frame_off[68:] == P.stats["end"]).all()


# ---- argument checks -----------------------------------------------------------------------------
def _untouched(res):
    return all(np.all(res[n].view(np.uint8) == 0xA5) for n, _ in abi.PLAN_FIELDS + (("seg_off", 0),))


def test_einval_enqueues_nothing(gpu_ctx):
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists({}, N_SOCK, slots=SLOTS))
    sends = _by_nseg([3, 2])
    ok = dict(mtu=1500, out_cap=1 << 20)
    cases = [dict(ok, mtu=67), dict(ok, mtu=1501), dict(ok, mtu=70004), dict(ok, out_cap=1 << 32),
             dict(ok, pbytes=1 << 32), dict(ok, max_segs=0), dict(ok, k=0xFFFFFFF0, max_segs=16)]
    cases += [dict(ok, null=("sends", f)) for f, _ in abi.TxSends._fields_ if f.endswith("_dev")]
    cases += [dict(ok, null=("plan", f)) for f, _ in abi.TxSegmentPlan._fields_ if f.endswith("_dev")]
    for c in cases:
        c = dict(c)
        res = abi.tx_segment_plan_run(gpu_ctx, PAYLOAD, c.pop("pbytes", PBYTES), sends, c.pop("max_segs", 8), **c)
        assert res["rc"] == -errno.EINVAL and _untouched(res), c
    # the full call refuses the same (the pointers and a 4 GiB output aside) and its own flags
    for c in [x for x in cases if "null" not in x and x["out_cap"] < 1 << 32] + [dict(ok, flags=2)]:
        c = dict(c)
        res = abi.tx_segment_run(gpu_ctx, _cfg(), PAYLOAD, c.pop("pbytes", PBYTES), sends, c.pop("max_segs", 8),
                                 guard=0, **c)
        assert res["rc"] == -errno.EINVAL and _untouched(res) and np.all(res["out"] == G.FILL), c
    L = abi.lib()
    sd, pl = abi.TxSends(), abi.TxSegmentPlan()
    assert L.udpdk_gpu_tx_segment_plan(None, C.byref(sd), 0, 0, 0, C.byref(pl)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_segment_plan(gpu_ctx.handle, None, 0, 0, 0, C.byref(pl)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_segment_plan(gpu_ctx.handle, C.byref(sd), 0, 0, 0, None) == -errno.EINVAL
    assert L.udpdk_gpu_tx_segment(gpu_ctx.handle, None, C.byref(sd), 0, 0, 0, None, 0, C.byref(pl)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_segment_stats(gpu_ctx.handle, None) == -errno.EINVAL
    # k == 0: 0, and nothing is written
    res = abi.tx_segment_plan_run(gpu_ctx, PAYLOAD, PBYTES, G.make_sends([]), 8)
    assert res["rc"] == 0 and _untouched(res)


def test_stats_without_a_plan():
    with abi.GpuContext(0, max_frames=1024, max_lanes=4) as ctx:
        rc, _ = abi.tx_segment_stats(ctx)
        assert rc == -errno.ENOENT
        res = abi.tx_segment_plan_run(ctx, PAYLOAD, PBYTES, G.make_sends([]), 8)        # k == 0 is no plan
        assert res["rc"] == 0 and abi.tx_segment_stats(ctx)[0] == -errno.ENOENT
        res = abi.tx_segment_plan_run(ctx, PAYLOAD, PBYTES, _by_nseg([2]), 8)
        assert res["rc"] == 0 and abi.tx_segment_stats(ctx)[0] == 0
