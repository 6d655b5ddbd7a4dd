"""What the neighbour cache costs, all from one box and one run: 1 M datagrams of 22 bytes (64-byte frames) to
256 distinct on-link destinations that are all in the table (every datagram a hit), and the RX side beside them:

  resolve        udpdk_gpu_neigh_resolve over the batch
  build_neigh    udpdk_gpu_tx_build_neigh with the MACs resolve wrote
  build_flags    udpdk_gpu_tx_build_flags over the same batch, this tree
  learn_none     udpdk_gpu_neigh_learn over bench config 2's batch (1 M x 64 B UDP): no candidate
  learn_256      the same batch with one ARP reply per 4096 frames, from 256 hosts the table knows

  python tools/neigh_rate.py [--calls 20] [--reps 5] [--n DATAGRAMS] [--parent tools/var/parent.so]
                             [--ab-reps 3] [--out profiles/neigh_rate.txt]

Before timing, resolve's output is compared with the model of tests/neigh_util.py on the first 4096 datagrams and
its counts on the whole batch; the frames of build_neigh are build_flags' frames with bytes 0-5 replaced; and both
learn cases' counts are the model's. Each timing is the wall time around `calls` back-to-back calls and a
synchronise, after a warm-up, alternating the cases in one process on one context.

--parent names a library built from the parent commit (tools/build_rev.sh): udpdk_gpu_tx_build_flags of both
libraries is then taken with tools/ab.py (its line `txflags`, which calls flags_line below: a fresh process per
library and repetition, alternating), and the result states the spread of each library's repetitions beside the
difference of the medians. One JSON line with the medians and every repetition."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from udpdk_amd import abi, frames as F  # noqa: E402

PAYLOAD = 22
N_HOSTS = 256
EVERY = 4096
LEARN_NOW, RESOLVE_NOW = 1500, 2000      # what learn refreshes stays fresh for resolve: every datagram a hit
SRC_MAC, DST_MAC = bytes.fromhex("6805ca95f8ec"), bytes.fromhex("6805ca95fa64")


def host_ip(k: int) -> int:
    return abi.raw_ip("172.31.%d.%d" % (100 + (k >> 7), 2 + (k & 127)))


def host_mac(k: int) -> bytes:
    return bytes([0x02, 0xAA, 0, 0, k >> 8, k & 255])


class TxSide:
    """The TX batch on the device: n datagrams of PAYLOAD bytes from one bound socket, frames back to back."""

    def __init__(self, ctx, n: int):
        self.n = n
        ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=[(0, abi.raw_port(10000), 1)]))
        rng = np.random.default_rng(7)
        pay = rng.integers(0, 256, n * PAYLOAD + 64, dtype=np.uint8)
        span = PAYLOAD + 42
        self.dst = np.array([host_ip(int(k)) for k in rng.integers(0, N_HOSTS, n)], np.uint32)
        self.bufs = [ctx.upload(pay), ctx.upload((np.arange(n, dtype=np.uint64) * PAYLOAD).astype(np.uint32)),
                     ctx.upload(np.full(n, PAYLOAD, np.uint16)), ctx.upload(np.zeros(n, np.int32)), ctx.upload(self.dst),
                     ctx.upload(np.full(n, abi.raw_port(10001), np.uint16)),
                     ctx.upload((np.arange(n, dtype=np.uint64) * span).astype(np.uint32))]
        self.cap = n * span + 64
        self.out = ctx.alloc(self.cap)
        self.cfg = abi.TxConfig((C.c_uint8 * 6)(*SRC_MAC), (C.c_uint8 * 6)(*DST_MAC), abi.raw_ip("172.31.100.1"))
        b = self.bufs
        self.bt = abi.TxBatch(b[0].ptr, pay.nbytes - 64, b[1].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, n)
        self.ot = abi.TxOut(self.out.ptr, self.cap, b[6].ptr)

    def flags(self, ctx):
        return abi.lib().udpdk_gpu_tx_build_flags(ctx.handle, C.byref(self.cfg), C.byref(self.bt), C.byref(self.ot), 0, 0)


def timed(ctx, fn, calls: int) -> float:
    for _ in range(3):
        abi._check(fn(), "warm-up")
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.sync()
    return round(1e6 * (time.perf_counter() - t0) / calls, 2)


def flags_line(ctx, n: int = 1 << 20, calls: int = 20, reps: int = 5) -> dict:
    """udpdk_gpu_tx_build_flags alone (tools/ab.py, line `txflags`: whatever library the process loaded)."""
    tx = TxSide(ctx, n)
    us = [timed(ctx, lambda: tx.flags(ctx), calls) for _ in range(reps)]
    return {"workload": f"TX {n} x {PAYLOAD + 42} B frames, udpdk_gpu_tx_build_flags", "us_per_call": statistics.median(us),
            "reps_us": us}


def learn_batches(n):
    """bench config 2's batch, and the same with an ARP reply from a known host in every EVERY-th frame."""
    import arp_util as A
    import neigh_util as U
    b = F.config_batch(2, n).batch
    fr = b.frames.copy()
    at = np.arange(EVERY // 2, b.n, EVERY)
    if int(b.length[at].min()) < 60:
        raise SystemExit("learn_256: a frame is shorter than 60 bytes")
    for j, i in enumerate(at):
        o = int(b.offset[i])
        k = j % N_HOSTS
        fr[o:o + 60] = np.frombuffer(A.arp_frame(op=2, sha=host_mac(k), spa=U.dotted(host_ip(k)), tha=SRC_MAC,
                                                 tpa="172.31.100.1", pad_to=60), np.uint8)
    return b, {"learn_none": b.frames, "learn_256": fr}, len(at)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--n", type=int, default=1 << 20)
    p.add_argument("--parent", default=None, help="the parent commit's library, for the A/B through tools/ab.py")
    p.add_argument("--ab-reps", type=int, default=3)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    import arp_util as A
    import neigh_util as U
    L = abi.lib()
    n = a.n
    ctx = abi.GpuContext(0, max_frames=max(n, 1024), max_lanes=1)
    tx = TxSide(ctx, n)
    cfg = U.cfg(src_ip="172.31.100.1", src_mac=SRC_MAC, netmask="255.255.254.0")
    init = [(host_ip(k), host_mac(k), U.REACHABLE, 1000) for k in range(N_HOSTS)]
    abi._check(abi.neigh_create(ctx, 1024), "udpdk_gpu_neigh_create")
    abi._check(abi.neigh_set(ctx, init), "udpdk_gpu_neigh_set")

    # resolve against the model, then its output buffers for the timed calls
    k = min(n, 4096)
    sock = np.zeros(k, np.int32)
    g = abi.neigh_resolve_run(ctx, cfg, tx.dst[:k], sock, RESOLVE_NOW, req_cap=16)
    R = U.resolve(U.Table(1024, init), cfg, tx.dst[:k], sock, RESOLVE_NOW, req_cap=16)
    if g["rc"] or g["stats"] != R["stats"] or not np.array_equal(g["dmac"][:k], R["dmac"]) or R["stats"]["hit"] != k:
        raise SystemExit(f"resolve differs from the model ({g['rc']}, {g['stats']}, {R['stats']})")
    dmac, so, state = ctx.alloc(8 * n), ctx.alloc(4 * n), ctx.alloc(n)
    req, org = ctx.alloc(64 * 16), ctx.alloc(4 * 16)
    nout = abi.NeighOut(dmac.ptr, so.ptr, state.ptr, req.ptr, org.ptr, 16)

    def resolve():
        return L.udpdk_gpu_neigh_resolve(ctx.handle, C.byref(cfg), C.c_void_p(tx.bufs[4].ptr), C.c_void_p(tx.bufs[3].ptr), n,
                                         RESOLVE_NOW, C.byref(nout))

    def build_neigh():
        return L.udpdk_gpu_tx_build_neigh(ctx.handle, C.byref(tx.cfg), C.byref(tx.bt), C.byref(tx.ot), 0, 0,
                                          C.c_void_p(dmac.ptr))
    abi._check(resolve(), "udpdk_gpu_neigh_resolve")
    rst = abi.NeighResolveStats()
    abi._check(L.udpdk_gpu_neigh_resolve_stats(ctx.handle, C.byref(rst)), "udpdk_gpu_neigh_resolve_stats")
    if rst.hit != n:
        raise SystemExit(f"resolve: {[getattr(rst, f) for f in abi.NEIGH_RESOLVE_STATS]}")
    abi._check(tx.flags(ctx), "udpdk_gpu_tx_build_flags")
    plain = ctx.download(tx.out, np.uint8, tx.cap - 64).reshape(n, PAYLOAD + 42)
    abi._check(build_neigh(), "udpdk_gpu_tx_build_neigh")
    got = ctx.download(tx.out, np.uint8, tx.cap - 64).reshape(n, PAYLOAD + 42)
    macs = np.array([list(host_mac(j)) for j in range(N_HOSTS)], np.uint8)
    which = {host_ip(j): j for j in range(N_HOSTS)}
    want = macs[[which[int(d)] for d in tx.dst]]
    if not (np.array_equal(got[:, 6:], plain[:, 6:]) and np.array_equal(got[:, :6], want) and np.all(plain[:, :6] == list(DST_MAC))):
        raise SystemExit("build_neigh: frames differ from build_flags' with the MACs replaced")

    # the RX side
    b, frames, n_arp = learn_batches(n)
    ctx.upload_snapshot(abi.snapshot_from_lists({abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}, 1))
    dev, counts = {}, {}
    lst = abi.NeighLearnStats()
    for name, fr in frames.items():
        db = abi.rx_upload(ctx, fr, b.offset, b.length)
        db.frames_bytes = b.frames_bytes
        o = abi.rx_alloc_out(ctx, b.n, 1, b.n)
        meta, _, _, _, rc = abi.rx_run(ctx, db, o)
        abi._check(rc, "udpdk_gpu_rx_stats")
        bt = abi.RxBatch(db.frames.ptr, b.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)
        dev[name] = (bt, o)
        model = U.learn(U.Table(1024, init), cfg, fr, b.frames_bytes, b.offset, b.length, meta, LEARN_NOW)["stats"]
        abi._check(L.udpdk_gpu_neigh_learn(ctx.handle, C.byref(cfg), C.byref(bt), C.c_void_p(o.meta.ptr), LEARN_NOW), name)
        abi._check(L.udpdk_gpu_neigh_learn_stats(ctx.handle, C.byref(lst)), name)
        counts[name] = {f: getattr(lst, f) for f in abi.NEIGH_LEARN_STATS}
        if counts[name] != model or model["arp"] != (n_arp if name == "learn_256" else 0):
            raise SystemExit(f"{name}: {counts[name]} differs from the model {model}")
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=[(0, abi.raw_port(10000), 1)]))

    def learn(name):
        return L.udpdk_gpu_neigh_learn(ctx.handle, C.byref(cfg), C.byref(dev[name][0]), C.c_void_p(dev[name][1].meta.ptr), LEARN_NOW)
    cases = {"resolve_us": resolve, "build_neigh_us": build_neigh, "build_flags_us": lambda: tx.flags(ctx),
             "learn_none_us": lambda: learn("learn_none"), "learn_256_us": lambda: learn("learn_256")}
    us = {name: [] for name in cases}
    for _ in range(a.reps):
        for name, fn in cases.items():
            us[name].append(timed(ctx, fn, a.calls))
    # still all hits after the timed calls (the learn cases refresh the entries resolve reads)
    abi._check(resolve(), "udpdk_gpu_neigh_resolve")
    abi._check(L.udpdk_gpu_neigh_resolve_stats(ctx.handle, C.byref(rst)), "udpdk_gpu_neigh_resolve_stats")
    if rst.hit != n:
        raise SystemExit(f"resolve after timing: {[getattr(rst, f) for f in abi.NEIGH_RESOLVE_STATS]}")
    res = {"workload": f"{n} x {PAYLOAD + 42} B datagrams to {N_HOSTS} on-link hosts, all hits; RX: {b.n} x 64 B frames",
           "datagrams": n, "calls": a.calls, "arp_frames": n_arp, "counts": counts}
    for name in cases:
        res[name] = statistics.median(us[name])
        res["reps_" + name] = us[name]
    res["build_neigh_over_build_flags"] = round(res["build_neigh_us"] / res["build_flags_us"], 4)
    res["resolve_over_build_flags"] = round(res["resolve_us"] / res["build_flags_us"], 4)
    ctx.close()

    if a.parent:
        # the same kernel in two libraries: a fresh process per library and repetition, alternating
        name = os.path.splitext(os.path.basename(a.parent))[0]
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", "ab.py"), "--libs",
                            f"base,{name}", "--line", "txflags", "--reps", str(a.ab_reps)], cwd=ROOT,
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode:
            raise SystemExit(f"tools/ab.py failed rc={r.returncode}")
        # its lines: "r<rep> <library> <workload>  us_per_call <us>"
        ab = {lib: [float(m.group(1)) for m in re.finditer(rf"^r\d+ {re.escape(lib)} .* us_per_call (\S+)", r.stdout, re.M)]
              for lib in ("base", name)}
        if any(len(v) != a.ab_reps for v in ab.values()):
            raise SystemExit(f"tools/ab.py: {ab}")
        med = {lib: statistics.median(v) for lib, v in ab.items()}
        res["ab_build_flags_us"] = {"this_tree": med["base"], "parent": med[name], "reps_this_tree": ab["base"],
                                    "reps_parent": ab[name]}
        res["ab_spread_us"] = {"this_tree": round(max(ab["base"]) - min(ab["base"]), 2),
                               "parent": round(max(ab[name]) - min(ab[name]), 2)}
        res["ab_this_tree_minus_parent_us"] = round(med["base"] - med[name], 2)
        res["ab_within_spread"] = abs(med["base"] - med[name]) <= max(res["ab_spread_us"].values())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
