"""What the ICMP error stage (udpdk_gpu_icmp_errors) costs, each case beside udpdk_gpu_rx of the same
batch on the same box:

  none      bench config 2's batch (1 M x 64 B UDP to a bound port), the socket connected: no
            candidates, the cost every poll pays with the feature on
  errors    1 M port-unreachable messages of 70 B, all about the one connected socket's datagrams
            (every frame a hard error for the same lane: the worst case for the atomic)

  python tools/icmp_err_rate.py [--calls 20] [--reps 5] [--n FRAMES] [--out profiles/NAME.txt]

Before timing, every case's first 4096 frames go through the stage and are compared with the model
of tests/icmp_err_util.py (words and counts), and the full batch's counts are checked. Each timing is
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

import icmp_err_util as E  # noqa: E402
from udpdk_amd import abi, frames as F  # noqa: E402

PEER = ("10.0.0.9", 5003)


def error_batch(n: int, sock: E.Sock):
    """n copies of one port-unreachable (70 bytes) back to back."""
    rng = np.random.default_rng(1)
    one = np.frombuffer(E.unreach_frame(E.sent_frame(rng, sock, 20, our_ip=F.IP_DST), 3, dst_ip=F.IP_DST), np.uint8)
    flat = np.concatenate([np.tile(one, n), np.zeros(256, np.uint8)])
    return flat, 70 * n, (70 * np.arange(n)).astype(np.uint32), np.full(n, 70, np.uint16)


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
    our = abi.raw_ip(F.IP_DST)
    sock = E.Sock(0, None, F.PORT_RECV, 0, PEER)
    lists = E.lists_of([sock])
    peers = E.peers_of([sock], 1)
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, 1))
    pd = ctx.upload(peers.view(np.uint8))
    ed = ctx.alloc(8)
    ef, enb, eoff, eln = error_batch(n, sock)
    batches = {"none": (b.frames, b.frames_bytes, b.offset, b.length), "errors": (ef, enb, eoff, eln)}
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
        g = abi.icmp_err_run(ctx, our, db, meta[:k], peers, 1, n=k)
        err, st = E.model(fr, nb, off[:k], ln[:k], meta[:k], lists, peers, 1, our)
        if g["rc"] or g["stats"] != st or not np.array_equal(g["err"][:1], err):
            raise SystemExit(f"{name}: differs from the model ({g['rc']}, {g['stats']}, {st})")

    def stage(name):
        return L.udpdk_gpu_icmp_errors(ctx.handle, our, C.byref(dev[name][2]), C.c_void_p(dev[name][1].meta.ptr),
                                       C.c_void_p(pd.ptr), 1, C.c_void_p(ed.ptr))

    def rx(name):
        return abi.rx_enqueue(ctx, dev[name][0], dev[name][1])

    counts = {}
    st = abi.IcmpErrStats()
    for name, want in (("none", (0, 0)), ("errors", (n, n))):
        abi._check(stage(name), "udpdk_gpu_icmp_errors")
        abi._check(L.udpdk_gpu_icmp_err_stats(ctx.handle, C.byref(st)), "udpdk_gpu_icmp_err_stats")
        if (st.errors, st.reported) != want:
            raise SystemExit(f"{name}: {[getattr(st, k) for k in abi.ICMP_ERR_STATS]}")
        counts[name] = {k: getattr(st, k) for k in abi.ICMP_ERR_STATS}
    word = int(ctx.download(ed, np.uint64, 1)[0])
    if word != (n << 8 | 3):
        raise SystemExit(f"errors: the lane's word is {word:#x}")

    cases = {"err_none_us": lambda: stage("none"), "rx_none_us": lambda: rx("none"),
             "err_errors_us": lambda: stage("errors"), "rx_errors_us": lambda: rx("errors")}
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
    res = {"workload": w.name, "frames": n, "calls": a.calls, "verdicts": verdicts, "counts": counts}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["reps_" + name] = us[name]
    res["none_over_rx"] = round(res["err_none_us"] / res["rx_none_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
