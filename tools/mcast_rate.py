"""What the multicast stages cost, each beside its yardstick on the same batch, in the same process,
alternating:

  filter    1 M x 64 B deliveries in 4096 lanes of 256, every lane checked and joined to a group of
            its own, half of the entries to the lane's group and half to another: the membership
            filter (udpdk_gpu_rx_mcast_select) beside the peer filter (udpdk_gpu_rx_peer_select)
            with every lane connected and half of the entries from its peer. The two read the same
            bytes per entry (the entry, a lane record, the descriptor, one request into the header).
  igmp      bench config 2's batch (1 M x 64 B UDP to a bound port: no candidate) through
            udpdk_gpu_igmp_reply beside udpdk_gpu_arp_reply.

  python tools/mcast_rate.py [--calls 20] [--reps 5] [--out profiles/NAME.txt]

Before timing, the filter's first lanes are compared with the model of tests/mcast_util.py and the
full run's counts with what the batch was built to give. Each timing is the wall time around `calls`
back-to-back calls and a synchronise, after a warm-up. One JSON line with the medians, the spread
(min, max) and every repetition."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import arp_util as AU  # noqa: E402
import mcast_util as U  # noqa: E402
import rx_balance_util as B  # noqa: E402
import rx_peer_util as UP  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402

LANES, PER = 4096, 256
PEER_IP, PEER_PORT = (10, 1, 2, 3), 7000


def filter_batch(seed=1):
    """(batch, lane_off, lane_pkt, lane_mc, members, peers, joined[n], from_peer[n])."""
    n = LANES * PER
    rng = np.random.default_rng(seed)
    lane = np.repeat(np.arange(LANES), PER)
    joined, from_peer = rng.integers(0, 2, n).astype(bool), rng.integers(0, 2, n).astype(bool)
    dst = np.stack([np.full(n, 239), np.where(joined, lane >> 8, 200), lane & 255, np.ones(n, np.int64)], axis=1)
    src = np.tile(np.array(PEER_IP), (n, 1))
    src[~from_peer, 3] = 4
    b = B.flow_frames(src.astype(np.uint8), np.full(n, PEER_PORT), dst.astype(np.uint8), np.full(n, 5000), seed)
    members = np.zeros(LANES, abi.MCAST_DTYPE)
    members["group"] = 239 | (np.arange(LANES) >> 8) << 8 | (np.arange(LANES) & 255) << 16 | 1 << 24
    members["lane"] = np.arange(LANES)
    peers = UP.peer_table(LANES, {l: (".".join(map(str, PEER_IP)), PEER_PORT) for l in range(LANES)})
    off = (PER * np.arange(LANES + 1)).astype(np.uint32)
    return b, off, np.arange(n, dtype=np.uint32), np.ones(LANES, np.uint8), members, peers, joined, from_peer


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    L = abi.lib()
    b, loff, lpkt, mc, members, peers, joined, from_peer = filter_batch()
    n = b.n
    ctx = abi.GpuContext(0, max_frames=n, max_lanes=LANES)
    ctx.upload_snapshot(abi.snapshot_from_lists({abi.raw_port(5000): [(0, 0, 0)]}, 1))
    slots = U.slots_for(LANES)
    rc, table = abi.mcast_table_build(members, slots)
    abi._check(rc, "udpdk_gpu_mcast_table_build")
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    # the first sixteen lanes against the model, then the whole set's counts
    k = 16 * PER
    tab = [(int(g), int(l)) for g, l in table]
    m = U.model(b, loff[:17], lpkt[:k], mc, tab)
    go, gp, st, rc = abi.rx_mcast_run(ctx, db, loff[:17], lpkt[:k], mc[:16], table)
    if rc or not np.array_equal(go, m.lane_off) or not np.array_equal(gp[:m.kept], m.lane_pkt) or \
            U.stats_tuple(st) != m.stats():
        raise SystemExit(f"filter: differs from the model ({rc}, {U.stats_tuple(st)}, {m.stats()})")
    bufs = [ctx.upload(x) for x in (loff, lpkt, mc, table.view(np.uint8), peers.view(np.uint8))]
    od, pd, md, td, rd = bufs
    oo, po = ctx.alloc(4 * (LANES + 1)), ctx.alloc(4 * n)
    bt = abi.RxBatch(db.frames.ptr, b.frames_bytes, db.offset.ptr, db.length.ptr, None, n)
    lanes = abi.RxLanes(None, n, od.ptr, pd.ptr, n, LANES)

    def mcast():
        return L.udpdk_gpu_rx_mcast_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(md.ptr), C.c_void_p(td.ptr),
                                           slots, C.c_void_p(oo.ptr), C.c_void_p(po.ptr), n)

    def peer():
        return L.udpdk_gpu_rx_peer_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(rd.ptr), C.c_void_p(oo.ptr),
                                          C.c_void_p(po.ptr), n)
    abi._check(mcast(), "udpdk_gpu_rx_mcast_select")
    rc, st = abi.rx_mcast_stats(ctx)
    want = int(joined.sum())
    if rc or (st.kept, st.member, st.not_member, st.bad_frame, st.bad_index) != (want, want, n - want, 0, 0):
        raise SystemExit(f"filter: counts {U.stats_tuple(st)}, {want} joined of {n}")
    abi._check(peer(), "udpdk_gpu_rx_peer_select")
    rc, pst = abi.rx_peer_stats(ctx)
    if rc or (pst.kept, pst.refused) != (int(from_peer.sum()), n - int(from_peer.sum())):
        raise SystemExit(f"peer: counts {UP.stats_tuple(pst)}")

    # the IGMP stage on config 2's batch
    w = F.config_batch(2, None)
    c2 = w.batch
    ictx = abi.GpuContext(0, max_frames=max(c2.n, 1024), max_lanes=1)
    ictx.upload_snapshot(abi.snapshot_from_lists({abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}, 1))
    db2 = abi.rx_upload(ictx, c2.frames, c2.offset, c2.length)
    db2.frames_bytes = c2.frames_bytes
    o2 = abi.rx_alloc_out(ictx, c2.n, 1, c2.n)
    meta, _, _, _, rc = abi.rx_run(ictx, db2, o2)
    abi._check(rc, "udpdk_gpu_rx_stats")
    bt2 = abi.RxBatch(db2.frames.ptr, c2.frames_bytes, db2.offset.ptr, db2.length.ptr, None, c2.n)
    cfg = AU.tx_config()
    groups = ictx.upload(np.array([abi.raw_ip(U.G1), abi.raw_ip(U.G2)], np.uint32))
    s_i, x_i = ictx.alloc(64 * 4096), ictx.alloc(4 * 4096)
    s_a, x_a = ictx.alloc(64 * 4096), ictx.alloc(4 * 4096)
    iout, aout = abi.IgmpOut(s_i.ptr, x_i.ptr, 4096), abi.ArpOut(s_a.ptr, x_a.ptr, 4096)

    def igmp():
        return L.udpdk_gpu_igmp_reply(ictx.handle, C.byref(cfg), C.byref(bt2), C.c_void_p(o2.meta.ptr),
                                      C.c_void_p(groups.ptr), 2, C.byref(iout))

    def arp():
        return L.udpdk_gpu_arp_reply(ictx.handle, C.byref(cfg), C.byref(bt2), C.c_void_p(o2.meta.ptr), C.byref(aout))
    abi._check(igmp(), "udpdk_gpu_igmp_reply")
    ist = abi.IgmpStats()
    if L.udpdk_gpu_igmp_stats(ictx.handle, C.byref(ist)) or any(getattr(ist, f) for f in abi.IGMP_STATS):
        raise SystemExit("igmp: a batch without a candidate counted something")

    cases = {"mcast_filter_us": (mcast, ctx), "peer_filter_us": (peer, ctx), "igmp_none_us": (igmp, ictx),
             "arp_none_us": (arp, ictx)}
    us = {name: [] for name in cases}
    for _ in range(a.reps):
        for name, (fn, cx) in cases.items():
            for _ in range(3):
                abi._check(fn(), name)
            cx.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            cx.sync()
            us[name].append(round(1e6 * (time.perf_counter() - t0) / a.calls, 2))
    res = {"entries": n, "lanes": LANES, "slots": slots, "calls": a.calls, "joined": want, "workload_igmp": w.name,
           "verdicts_igmp": np.bincount(meta & 0xF, minlength=8).tolist()}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["spread_" + name] = [min(us[name]), max(us[name])]
        res["reps_" + name] = us[name]
    res["mcast_over_peer"] = round(res["mcast_filter_us"] / res["peer_filter_us"], 4)
    res["igmp_over_arp"] = round(res["igmp_none_us"] / res["arp_none_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    ctx.close()
    ictx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
