"""What the reuse-port balance stage (udpdk_gpu_rx_balance_select) costs: bench config 2's frames
(1 M x 64 B to one port) against eight reuse-port sockets on that port, 8 M lane entries.

  python tools/balance_rate.py [--calls 20] [--reps 5] [--n FRAMES] [--out profiles/NAME.txt]

The frames' source addresses are randomised on the host (config 2 sends one flow), so the hash
spreads the frames over the group. udpdk_gpu_rx makes the lanes once; then, alternating in one
process on one context, `reps` rounds of: the balance computing its hash, the balance with a
supplied hash_dev, and udpdk_gpu_rx_filter(flags = 0) on the same lane set (the cost of compacting
those entries without the stage: an identity copy through the same compaction). Each timing is
the wall time around `calls` back-to-back calls and a synchronise, after a warm-up. One JSON line
with the medians and every repetition. Before timing, the balanced lanes are compared with the
model of tests/rx_balance_util.py on a prefix of the batch."""
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

import rx_balance_util as U  # noqa: E402
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

    hashes = U.frame_hashes(b)
    rp = ctx.upload(np.ones(GROUP, np.uint8))
    hd = ctx.upload(hashes)
    oo, po = ctx.alloc(4 * (GROUP + 1)), ctx.alloc(4 * cap)
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)
    lanes = abi.RxLanes(out.meta.ptr, b.n, out.lane_off.ptr, out.lane_pkt.ptr, cap, GROUP)

    def balance(h):
        return L.udpdk_gpu_rx_balance_select(ctx.handle, C.byref(bt), C.byref(lanes), C.c_void_p(rp.ptr),
                                             C.c_void_p(h) if h else None, C.c_void_p(oo.ptr), C.c_void_p(po.ptr), cap)

    def copy():
        return L.udpdk_gpu_rx_filter(ctx.handle, C.byref(lanes), 0, C.c_void_p(oo.ptr), C.c_void_p(po.ptr), cap)

    # the result against the model, on the frames of a prefix (the model walks in python)
    k = min(b.n, 20000)
    sub = type("B", (), dict(frames=b.frames, offset=b.offset[:k], length=b.length[:k],
                             frames_bytes=b.frames_bytes, n=k, ptype=None))
    chosen, _, _ = U.choose(lists.get, sub, meta[:k], np.ones(GROUP, np.uint8), hashes[:k])
    for h in (0, hd.ptr):
        abi._check(balance(h), "udpdk_gpu_rx_balance_select")
        rc, st = abi.rx_balance_stats(ctx)
        go = ctx.download(oo, np.uint32, GROUP + 1)
        gp = ctx.download(po, np.uint32, b.n)
        if rc or st.kept != b.n or st.balanced != b.n:
            raise SystemExit(f"balance stats {rc} {st.kept} {st.balanced}")
        for l in range(GROUP):
            mine = gp[go[l]:go[l + 1]]
            if not np.array_equal(mine[mine < k], np.flatnonzero(chosen == l)):
                raise SystemExit(f"lane {l} differs from the model")

    cases = {"balance_us": lambda: balance(0), "balance_hash_supplied_us": lambda: balance(hd.ptr),
             "filter_flags0_us": copy}
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
    res = {"workload": w.name, "group": GROUP, "frames": b.n, "entries": cap, "calls": a.calls}
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
