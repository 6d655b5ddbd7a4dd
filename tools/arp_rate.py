"""What the ARP reply stage (udpdk_gpu_arp_reply) costs, each case beside udpdk_gpu_rx and beside
udpdk_gpu_icmp_reply (flags all) of the same batch on the same box:

  none      bench config 2's batch (1 M x 64 B UDP to a bound port): no candidate, what a caller pays
            who runs the stage without looking at the RX counters first
  sparse    the same batch with one eligible request per 4096 frames
  flood     1 M eligible 60-byte requests with max_replies = 4096

  python tools/arp_rate.py [--calls 20] [--reps 5] [--n FRAMES] [--out profiles/NAME.txt]

Before timing, every case's first 4096 frames go through the stage and are compared with the model of
tests/arp_util.py (slots, origin and counts), and the full batch's counts are checked. Each timing is
the wall time around `calls` back-to-back calls and a synchronise, after a warm-up, alternating the
cases in one process on one context. One JSON line with the medians and every repetition."""
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

import arp_util as U  # noqa: E402
import icmp_util as IU  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402

MAX_REPLIES = 4096
EVERY = 4096


def flood_batch(n: int):
    """n copies of one eligible request padded to 60 bytes, back to back."""
    one = np.frombuffer(U.arp_frame(pad_to=60), np.uint8)
    flat = np.concatenate([np.tile(one, n), np.zeros(256, np.uint8)])
    return flat, 60 * n, (60 * np.arange(n)).astype(np.uint32), np.full(n, 60, np.uint16)


def sparse_batch(b):
    """The UDP batch with the first bytes of every EVERY-th frame overwritten by a 60-byte request."""
    fr = b.frames.copy()
    req = np.frombuffer(U.arp_frame(pad_to=60), np.uint8)
    at = np.arange(EVERY // 2, b.n, EVERY)
    if int(b.length[at].min()) < 60:
        raise SystemExit("sparse: a frame is shorter than 60 bytes")
    for i in at:
        o = int(b.offset[i])
        fr[o:o + 60] = req
    return fr, len(at)


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
    ctx.upload_snapshot(abi.snapshot_from_lists({abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}, 1))
    sfr, n_sparse = sparse_batch(b)
    ff, fnb, foff, fln = flood_batch(n)
    batches = {"none": (b.frames, b.frames_bytes, b.offset, b.length), "sparse": (sfr, b.frames_bytes, b.offset, b.length),
               "flood": (ff, fnb, foff, fln)}
    cfg = U.tx_config()
    slots, org = ctx.alloc(64 * MAX_REPLIES), ctx.alloc(4 * MAX_REPLIES)
    aout = abi.ArpOut(slots.ptr, org.ptr, MAX_REPLIES)
    i_out, i_ro, i_org = ctx.alloc(1 << 20), ctx.alloc(4 * (MAX_REPLIES + 1)), ctx.alloc(4 * MAX_REPLIES)
    iout = abi.IcmpOut(i_out.ptr, 1 << 20, i_ro.ptr, i_org.ptr, MAX_REPLIES)
    dev, verdicts = {}, {}
    for name, (fr, nb, off, ln) in batches.items():
        db = abi.rx_upload(ctx, fr, off, ln)
        db.frames_bytes = nb
        o = abi.rx_alloc_out(ctx, n, 1, n)
        meta, _, _, _, rc = abi.rx_run(ctx, db, o)
        abi._check(rc, "udpdk_gpu_rx_stats")
        dev[name] = (db, o, abi.RxBatch(db.frames.ptr, nb, db.offset.ptr, db.length.ptr, None, n))
        verdicts[name] = np.bincount(meta & 0xF, minlength=8).tolist()
        k = min(n, 4096)
        g = abi.arp_run(ctx, cfg, db, meta[:k], n=k)
        R = U.model(fr, nb, off[:k], ln[:k], meta[:k])
        r = R["stats"]["replies"]
        if g["rc"] or g["stats"] != R["stats"] or not np.array_equal(g["slots"][:r], R["slots"]) or \
                not np.array_equal(g["origin"][:r], R["origin"]):
            raise SystemExit(f"{name}: differs from the model ({g['rc']}, {g['stats']}, {R['stats']})")

    def arp(name):
        return L.udpdk_gpu_arp_reply(ctx.handle, C.byref(cfg), C.byref(dev[name][2]), C.c_void_p(dev[name][1].meta.ptr),
                                     C.byref(aout))

    def icmp(name):
        return L.udpdk_gpu_icmp_reply(ctx.handle, C.byref(cfg), C.byref(dev[name][2]), C.c_void_p(dev[name][1].meta.ptr),
                                      IU.ALL, 0, IU.NO_LIMIT, C.byref(iout))

    def rx(name):
        return abi.rx_enqueue(ctx, dev[name][0], dev[name][1])

    counts = {}
    st = abi.ArpStats()
    for name, elig in (("none", 0), ("sparse", n_sparse), ("flood", n)):
        abi._check(arp(name), "udpdk_gpu_arp_reply")
        rc = L.udpdk_gpu_arp_stats(ctx.handle, C.byref(st))
        if rc not in (0, -28) or (st.eligible, st.replies, st.no_room) != (elig, min(elig, MAX_REPLIES),
                                                                           elig - min(elig, MAX_REPLIES)):
            raise SystemExit(f"{name}: {rc} {[getattr(st, k) for k in abi.ARP_STATS]}")
        counts[name] = {k: getattr(st, k) for k in abi.ARP_STATS}

    cases = {}
    for name in batches:
        cases[f"arp_{name}_us"] = lambda name=name: arp(name)
        cases[f"icmp_{name}_us"] = lambda name=name: icmp(name)
        cases[f"rx_{name}_us"] = lambda name=name: rx(name)
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
    res = {"workload": w.name, "frames": n, "calls": a.calls, "max_replies": MAX_REPLIES, "verdicts": verdicts,
           "counts": counts}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["reps_" + name] = us[name]
    res["arp_none_over_icmp_none"] = round(res["arp_none_us"] / res["icmp_none_us"], 4)
    res["arp_none_over_rx_none"] = round(res["arp_none_us"] / res["rx_none_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
