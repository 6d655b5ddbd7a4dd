"""What answering on the device costs: 1 M x 64 B and 1 M x 1500 B frames (bench.py's configs 2 and
3), every frame delivered to one socket and answered, timed three ways in one process on one
context, alternating:

  (a) plan     udpdk_gpu_tx_reply_plan alone, against the byte floor of tx_reply.hip's header
  (b) reply    udpdk_gpu_tx_reply (the plan + tx_build reading the payloads in the RX frame buffer)
  (c) compose  the most favourable device-only composition without the plan: the descriptors of
               both calls prebuilt on the host outside the timed region, then
               udpdk_gpu_rx_gather_packed + udpdk_gpu_tx_build_flags (the gather writes every
               payload once more and tx_build reads it back)

  python tools/tx_reply_rate.py [--steps 20] [--reps 5] [--out profiles/NAME.json]

Per form: `reps` rounds, each `steps` back-to-back calls between two events after a warm-up, as
bench.tx_line times them; the median and every repetition, one JSON line per workload. Before
timing, (b)'s output bytes are compared with (c)'s: they must be equal."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402

FLOOR_BYTES = 94          # per entry, tx_reply.hip's header
HBM_TBPS = 6.3            # achievable, MI355X


def workload(ctx, cfg: int, steps: int, reps: int, mtu: int = 1500) -> dict:
    w = F.config_batch(cfg)
    b, n = w.batch, w.batch.n
    ctx.upload_snapshot(abi.snapshot_from_lists(w.port_lists(), 1, slots=[(0, abi.raw_port(w.base_port), 1)]))
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    out = abi.rx_alloc_out(ctx, n, 1, n)
    _, loff, lpkt, _, rc = abi.rx_run(ctx, db, out)
    assert rc == 0 and loff[1] == n, "every frame is delivered"
    L = abi.lib()
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, n)
    lanes = abi.RxLanes(out.meta.ptr, n, out.lane_off.ptr, out.lane_pkt.ptr, n, 1)
    plen = int(b.length[0]) - 42
    span = int(L.udpdk_gpu_tx_span(plen, mtu, None))
    cap = n * span + 64
    arrs = [ctx.alloc(4 * (n + 1)) for _ in range(6)]
    plan = abi.TxReplyPlan(*[a.ptr for a in arrs])
    fr_b, fr_c = ctx.alloc(cap), ctx.alloc(cap)
    cfgt = abi.TxConfig((C.c_uint8 * 6)(*bytes.fromhex("6805ca95f8ec")),
                        (C.c_uint8 * 6)(*bytes.fromhex("6805ca95fa64")), abi.raw_ip("172.31.100.2"))
    # (c): packed gather slots and tx_build descriptors, prebuilt
    slot = (plen + 15) & ~15
    slot_off = ctx.upload((np.arange(n + 1, dtype=np.uint64) * slot).astype(np.uint32))
    g = [ctx.alloc(n * slot + 64), ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(2 * n)]
    gt = abi.RxGather(g[0].ptr, 16, g[1].ptr, g[2].ptr, g[3].ptr)
    hdr = b.frames[:int(b.frames_bytes)].reshape(n, -1)[:, 26:36][lpkt]
    d = [ctx.upload(np.full(n, plen, np.uint16)), ctx.upload(np.zeros(n, np.int32)),
         ctx.upload(np.ascontiguousarray(hdr[:, 0:4]).view(np.uint32).ravel()),
         ctx.upload(np.ascontiguousarray(hdr[:, 8:10]).view(np.uint16).ravel()),
         ctx.upload((np.arange(n, dtype=np.uint64) * span).astype(np.uint32))]
    tb = abi.TxBatch(g[0].ptr, n * slot, slot_off.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, n)
    to = abi.TxOut(fr_c.ptr, cap, d[4].ptr)

    def plan_only():
        return L.udpdk_gpu_tx_reply_plan(ctx.handle, C.byref(bt), C.byref(lanes), 0, n, None, mtu, cap, C.byref(plan))

    def reply():
        return L.udpdk_gpu_tx_reply(ctx.handle, C.byref(cfgt), C.byref(bt), C.byref(lanes), 0, n, None, mtu, 0,
                                    C.c_void_p(fr_b.ptr), cap, C.byref(plan))

    def compose():
        rc = L.udpdk_gpu_rx_gather_packed(ctx.handle, C.byref(bt), C.c_void_p(out.lane_pkt.ptr), 0, n,
                                          C.c_void_p(slot_off.ptr), C.byref(gt))
        return rc or L.udpdk_gpu_tx_build_flags(ctx.handle, C.byref(cfgt), C.byref(tb), C.byref(to), mtu, 0)

    # the two ways give the same bytes
    abi._check(reply(), "udpdk_gpu_tx_reply")
    rc, st = abi.tx_reply_stats(ctx)
    assert rc == 0 and st.replied == n and st.bytes_needed == n * span
    abi._check(compose(), "gather + tx_build")
    ctx.sync()
    for lo in range(0, n * span, 1 << 28):
        m = min(1 << 28, n * span - lo)
        x = abi.download_ptr(ctx, fr_b.ptr + lo, np.uint8, m)
        y = abi.download_ptr(ctx, fr_c.ptr + lo, np.uint8, m)
        if not np.array_equal(x, y):
            raise SystemExit(f"config {cfg}: the reply's bytes differ from the composition's")

    ev = bench.HipEvents(ctx)
    forms = {"plan": plan_only, "reply": reply, "compose": compose}
    us = {k: [] for k in forms}
    for _ in range(reps):
        for name, f in forms.items():
            for _ in range(3):
                abi._check(f(), name)
            ctx.sync()
            ev.record(0)
            for _ in range(steps):
                f()
            ev.record(1)
            ctx.sync()
            us[name].append(round(1e3 * ev.elapsed_ms() / steps, 2))
    ev.close()
    for x in arrs + [fr_b, fr_c, slot_off] + g + d + [db.frames, db.offset, db.length, out.meta, out.lane_off, out.lane_pkt]:
        x.free()
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"workload": w.name, "n": n, "frame_bytes": int(b.length[0]), "mtu": mtu, "steps": steps,
            "us_plan": med["plan"], "us_plan_floor": round(n * FLOOR_BYTES / HBM_TBPS / 1e6, 2),
            "us_reply": med["reply"], "us_compose": med["compose"],
            "reply_over_compose": round(med["reply"] / med["compose"], 4),
            "reps_plan": us["plan"], "reps_reply": us["reply"], "reps_compose": us["compose"]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--configs", default="2,3")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = p.parse_args()
    ctx = abi.GpuContext(0, max_frames=1 << 20, max_lanes=8)
    lines = []
    for cfg in [int(x) for x in a.configs.split(",")]:
        lines.append(json.dumps(workload(ctx, cfg, a.steps, a.reps)))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
