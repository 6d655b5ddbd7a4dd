"""What the ICMP stage (udpdk_gpu_icmp_reply) costs, each case beside udpdk_gpu_rx of the same batch on
the same box:

  none      bench config 2's batch (1 M x 64 B UDP to a bound port) with both flags: no candidates,
            the cost every poll pays with the feature on
  echo      1 M echo requests of 64 B
  unreach   config 2's frames with nothing bound (every datagram to a closed port), err_limit
            unlimited and 64

  python tools/icmp_rate.py [--calls 20] [--reps 5] [--n FRAMES] [--out profiles/NAME.txt]

Before timing, every case's first 4096 frames go through the stage and are compared with the model
of tests/icmp_util.py (reply_off, origin, bytes, counts), and the full batch's counts are checked.
Each timing is the wall time around `calls` back-to-back calls and a synchronise, after a warm-up,
alternating the cases in one process on one context. One JSON line with the medians and every
repetition."""
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

import icmp_util as U  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402


def echo_batch(n: int):
    """n echo requests of 64 bytes (a 30-byte message) back to back, identifier and sequence varied."""
    one = np.frombuffer(U.echo_request(np.random.default_rng(1), 30, ident=0, seq=0), np.uint8)
    rows = np.tile(one, (n, 1))
    k = np.arange(n, dtype=np.uint32)
    rows[:, 38], rows[:, 39], rows[:, 40], rows[:, 41] = (k >> 24) & 0xFF, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF
    rows[:, 36:38] = 0
    w = rows[:, 34:64].astype(np.uint32)
    s = w[:, 0::2].sum(1) + (w[:, 1::2].sum(1) << 8)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    rows[:, 36], rows[:, 37] = s & 0xFF, s >> 8
    flat = np.concatenate([rows.reshape(-1), np.zeros(256, np.uint8)])
    return flat, 64 * n, (64 * k).astype(np.uint32), np.full(n, 64, np.uint16)


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
    n = b.n
    ctx = abi.GpuContext(0, max_frames=max(n, 1024), max_lanes=1)
    cfg = U.tx_config(F.IP_DST)
    bound = abi.snapshot_from_lists({abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}, 1)
    unbound = abi.snapshot_from_lists({abi.raw_port(9): [(0, 0, 0)]}, 1)
    ef, enb, eoff, eln = echo_batch(n)
    batches = {"none": (b.frames, b.frames_bytes, b.offset, b.length, bound),
               "echo": (ef, enb, eoff, eln, bound),
               "unreach": (b.frames, b.frames_bytes, b.offset, b.length, unbound)}
    out_cap = 72 * n + 64
    ro, og, ob = ctx.alloc(4 * (n + 1)), ctx.alloc(4 * n), ctx.alloc(out_cap)
    io = abi.IcmpOut(ob.ptr, out_cap, ro.ptr, og.ptr, n)
    dev, verdicts = {}, {}
    for name, (fr, nb, off, ln, snap) in batches.items():
        ctx.upload_snapshot(snap)
        db = abi.rx_upload(ctx, fr, off, ln)
        db.frames_bytes = nb
        o = abi.rx_alloc_out(ctx, n, 1, n)
        meta, _, _, _, rc = abi.rx_run(ctx, db, o)
        abi._check(rc, "udpdk_gpu_rx_stats")
        dev[name] = (db, o, abi.RxBatch(db.frames.ptr, nb, db.offset.ptr, db.length.ptr, None, n), snap)
        verdicts[name] = np.bincount(meta & 0xF, minlength=8).tolist()
        # the model on the first frames, the counts on all of them
        k = min(n, 4096)
        g = abi.icmp_run(ctx, cfg, db, meta[:k], n=k, out_cap=72 * k + 64, max_replies=k)
        m = U.model(fr, nb, off[:k], ln[:k], meta[:k], src_ip=cfg.src_ip)
        r = m.stats["replies"]
        if g["rc"] or U.stats_dict(g["stats"]) != m.stats or not np.array_equal(g["reply_off"][:r + 1], m.reply_off) or \
                not np.array_equal(g["origin"][:r], m.origin) or not np.array_equal(g["out"][:len(m.out)], m.out):
            raise SystemExit(f"{name}: differs from the model ({g['rc']}, {U.stats_dict(g['stats'])}, {m.stats})")

    def stage(name, limit):
        return L.udpdk_gpu_icmp_reply(ctx.handle, C.byref(cfg), C.byref(dev[name][2]), C.c_void_p(dev[name][1].meta.ptr),
                                      abi.ICMP_ALL, 0, limit, C.byref(io))

    def rx(name):
        return abi.rx_enqueue(ctx, dev[name][0], dev[name][1])

    counts = {}
    st = abi.IcmpStats()
    for name, limit, want in (("none", U.NO_LIMIT, (0, 0, 0)), ("echo", U.NO_LIMIT, (n, 0, 0)),
                              ("unreach", U.NO_LIMIT, (0, n, 0)), ("unreach", 64, (0, min(n, 64), n - min(n, 64)))):
        abi._check(stage(name, limit), "udpdk_gpu_icmp_reply")
        abi._check(L.udpdk_gpu_icmp_stats(ctx.handle, C.byref(st)), "udpdk_gpu_icmp_stats")
        if (st.echo_replied, st.unreach_sent, st.limited) != want:
            raise SystemExit(f"{name} limit {limit}: {U.stats_dict(st)}")
        counts[f"{name}_{'all' if limit == U.NO_LIMIT else limit}"] = U.stats_dict(st)

    cases = {"icmp_none_us": lambda: stage("none", U.NO_LIMIT), "rx_none_us": lambda: rx("none"),
             "icmp_echo_us": lambda: stage("echo", U.NO_LIMIT), "rx_echo_us": lambda: rx("echo"),
             "icmp_unreach_all_us": lambda: stage("unreach", U.NO_LIMIT),
             "icmp_unreach_64_us": lambda: stage("unreach", 64), "rx_unreach_us": lambda: rx("unreach")}
    snap_of = {"none": "none", "echo": "echo", "unre": "unreach"}
    us = {name: [] for name in cases}
    for _ in range(a.reps):
        for name, fn in cases.items():
            if name.startswith("rx_"):
                ctx.upload_snapshot(dev[snap_of[name[3:7]]][3])
            for _ in range(3):
                abi._check(fn(), name)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            ctx.sync()
            us[name].append(round(1e6 * (time.perf_counter() - t0) / a.calls, 2))
    res = {"workload": w.name, "frames": n, "calls": a.calls, "verdicts": verdicts, "counts": counts}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["reps_" + name] = us[name]
    res["none_over_rx"] = round(res["icmp_none_us"] / res["rx_none_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
