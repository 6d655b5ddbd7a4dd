"""What the peer filter (udpdk_gpu_rx_peer_select) costs: tools/balance_rate.py's workload, bench
config 2's frames (1 M x 64 B to one port, source addresses randomised) against eight sockets on
that port, 8 M lane entries.

  python tools/peer_rate.py [--calls 20] [--reps 5] [--n FRAMES] [--out profiles/NAME.txt]

udpdk_gpu_rx makes the lanes once; then, alternating in one process on one context, `reps` rounds
of: the filter with all eight lanes connected to one fixed peer (the source of frame 0: nearly
every entry is refused, every entry's header is read), with one of the eight connected, with none
connected (an identity copy that reads the peer records only), and udpdk_gpu_rx_filter(flags = 0)
on the same lane set (the shared compaction alone: the floor for this stage). Each timing is the
wall time around `calls` back-to-back calls and a synchronise, after a warm-up. One JSON line with
the medians and every repetition. Before timing, every case's output is compared with the model of
tests/rx_peer_util.py."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rx_peer_util as U  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402

GROUP = 8


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--n", type=int, default=None, help="frames (default: config 2's 2^20)")
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    L = abi.lib()
    w = F.config_batch(2, a.n)
    b = w.batch
    rows = b.frames[:b.n * 64].reshape(b.n, 64)
    rows[:, 26:30] = np.random.default_rng(2).integers(0, 256, (b.n, 4), dtype=np.uint8)
    lists = {abi.raw_port(F.PORT_RECV): [(0, k, 1) for k in range(GROUP)]}
    ctx = abi.GpuContext(0, max_frames=max(b.n, 1024), max_lanes=GROUP)
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, GROUP))
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    cap = GROUP * b.n
    out = abi.rx_alloc_out(ctx, b.n, GROUP, cap)
    meta, loff, pkt, _, rc = abi.rx_run(ctx, db, out)
    abi._check(rc, "udpdk_gpu_rx_stats")
    assert int(loff[-1]) == cap

    ip, port = U.src_fields(b, np.array([0]))
    peer = (int(ip[0]), int(port[0]))
    raw = lambda lanes: {l: (peer[0], socket.ntohs(peer[1])) for l in lanes}     # (peer_table: host-order port)
    tables = {"peer_all8_us": U.peer_table(GROUP, raw(range(GROUP))), "peer_one_of8_us": U.peer_table(GROUP, raw([3])),
              "peer_none_us": U.peer_table(GROUP, {})}
    dev = {name: ctx.upload(t.view(np.uint8)) for name, t in tables.items()}
    oo, po = ctx.alloc(4 * (GROUP + 1)), ctx.alloc(4 * cap)
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)
    lanes = abi.RxLanes(out.meta.ptr, b.n, out.lane_off.ptr, out.lane_pkt.ptr, cap, GROUP)

    def peer_call(name):
        return L.udpdk_gpu_rx_peer_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(dev[name].ptr),
                                          C.c_void_p(oo.ptr), C.c_void_p(po.ptr), cap)

    def copy():
        return L.udpdk_gpu_rx_filter(ctx.handle, C.byref(lanes), 0, C.c_void_p(oo.ptr), C.c_void_p(po.ptr), cap)

    kept = {}
    for name, t in tables.items():
        abi._check(peer_call(name), "udpdk_gpu_rx_peer_select")
        rc, st = abi.rx_peer_stats(ctx)
        m = U.model(b, loff, pkt, t)
        go = ctx.download(oo, np.uint32, GROUP + 1)
        gp = ctx.download(po, np.uint32, m.kept)
        if rc or U.stats_tuple(st) != m.stats() or not np.array_equal(go, m.lane_off) or \
                not np.array_equal(gp, m.lane_pkt):
            raise SystemExit(f"{name}: differs from the model ({rc}, {U.stats_tuple(st)}, {m.stats()})")
        kept[name] = m.kept

    cases = {name: (lambda name=name: peer_call(name)) for name in tables}
    cases["filter_flags0_us"] = copy
    us = {name: [] for name in cases}
    for _ in range(a.reps):
        for name, fn in cases.items():
            for _ in range(3):
                abi._check(fn(), name)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            ctx.sync()
            us[name].append(round(1e6 * (time.perf_counter() - t0) / a.calls, 2))
    res = {"workload": w.name, "group": GROUP, "frames": b.n, "entries": cap, "calls": a.calls,
           "kept": {k[:-3]: v for k, v in kept.items()}}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["reps_" + name] = us[name]
    line = json.dumps(res)
    print(line, flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
