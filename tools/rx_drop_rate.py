"""What the RX drop filter (udpdk_gpu_rx_drop) costs: bench configs 2 and 5 through udpdk_gpu_rx
with drop 0 and with drop 15, alternating, in one process on one context.

  python tools/rx_drop_rate.py [--steps 50] [--reps 5] [--n FRAMES] [--out profiles/NAME.json]

Per config twice: the clean batch (nothing is dropped, the stage only copies) and the batch with
the UDP checksum of every 100th frame corrupted on the host before upload. `reps` rounds of (drop
0, drop 15), each `steps` back-to-back calls between two events after a warm-up, as bench.py times
its GPU time (depth 1, one stream). One JSON line per case with both times (median and every
repetition) and their ratio. Before timing, the filtered lanes are compared with the numpy model
of tests/rx_drop_util.py applied to the unfiltered lanes of the same batch."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bench  # noqa: E402
import rx_drop_util as U  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402


def case(ctx, cfg: int, n: int | None, corrupt: bool, steps: int, reps: int) -> dict:
    w = F.config_batch(cfg, n)
    b = w.batch
    if corrupt:                                 # 64-byte frames back to back: a payload byte
        b.frames[:b.n * 64].reshape(b.n, 64)[::100, 50] ^= 0x21
    ctx.upload_snapshot(abi.snapshot_from_lists(w.port_lists(), w.n_sockets))
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    out = abi.rx_alloc_out(ctx, b.n, w.n_sockets, b.n)

    # the filtered lanes against the model of the unfiltered ones
    meta, loff, pkt, _, rc = abi.rx_run(ctx, db, out)
    abi._check(rc, "udpdk_gpu_rx_stats")
    m = U.model(meta, loff, pkt, abi.RX_DROP_ALL)
    ctx.rx_drop(abi.RX_DROP_ALL)
    meta2, loff2, pkt2, _, rc = abi.rx_run(ctx, db, out)
    ctx.rx_drop(0)
    if rc or not (np.array_equal(meta2, meta) and np.array_equal(loff2, m.lane_off) and
                  np.array_equal(pkt2, m.lane_pkt)):
        raise SystemExit(f"config {cfg}: filtered lanes differ from the model")

    ev = bench.HipEvents(ctx)
    us = {0: [], abi.RX_DROP_ALL: []}
    for _ in range(reps):
        for flags in (0, abi.RX_DROP_ALL):
            ctx.rx_drop(flags)
            for _ in range(5):
                abi._check(abi.rx_enqueue(ctx, db, out), "udpdk_gpu_rx")
            ctx.sync()
            ev.record(0)
            for _ in range(steps):
                abi.rx_enqueue(ctx, db, out)
            ev.record(1)
            ctx.sync()
            us[flags].append(round(1e3 * ev.elapsed_ms() / steps, 2))
    ctx.rx_drop(0)
    ev.close()
    for x in (db.frames, db.offset, db.length, out.meta, out.lane_off, out.lane_pkt):
        x.free()
    a, d = statistics.median(us[0]), statistics.median(us[abi.RX_DROP_ALL])
    return {"workload": w.name, "config": cfg, "corrupt_every": 100 if corrupt else 0, "steps": steps,
            "deliveries": int(loff[-1]), "removed": m.removed, "us_drop0": a, "us_drop15": d,
            "ratio": round(d / a, 4), "reps_drop0": us[0], "reps_drop15": us[abi.RX_DROP_ALL]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--n", type=int, default=None, help="frames per batch (default: the config's)")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = p.parse_args()
    ctx = abi.GpuContext(0, max_frames=1 << 22, max_lanes=4096)
    lines = []
    for cfg in (2, 5):
        for corrupt in (False, True):
            lines.append(json.dumps(case(ctx, cfg, a.n, corrupt, a.steps, a.reps)))
            print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
