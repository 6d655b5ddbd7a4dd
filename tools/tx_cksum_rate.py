"""What UDPDK_TX_UDP_CKSUM costs: bench.py's three TX shapes, each built with flags 0 and with the
checksum, alternating, in one process on one context.

  python tools/tx_cksum_rate.py [--steps 50] [--reps 5] [--out profiles/NAME.json]

Per shape: `reps` rounds of (flags 0, checksum), each `steps` back-to-back launches between two
events after a warm-up, as bench.tx_line times them. One JSON line per shape with both times
(median and every repetition) and their ratio; the moved bytes are the same in both forms, so the
ratio is kernel overhead. Before timing, the checksum form's output is compared with the flags-0
output: it may differ at bytes 40-41 of each datagram only, and must there."""
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
from udpdk_amd import abi  # noqa: E402

SHAPES = [(22, 1 << 20, 0), (1458, 1 << 20, 0), (2952, 1 << 18, 1500)]


def shape(ctx, payload_len: int, n: int, mtu: int, steps: int, reps: int) -> dict:
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=[(0, abi.raw_port(10000), 1)]))
    rng = np.random.default_rng(7)
    pay = rng.integers(0, 256, n * payload_len + 64, dtype=np.uint8)
    nf = C.c_uint32()
    span = int(abi.lib().udpdk_gpu_tx_span(payload_len, mtu, C.byref(nf)))
    bufs = [ctx.upload(pay), ctx.upload((np.arange(n, dtype=np.uint64) * payload_len).astype(np.uint32)),
            ctx.upload(np.full(n, payload_len, np.uint16)), ctx.upload(np.zeros(n, np.int32)),
            ctx.upload(np.full(n, abi.raw_ip("172.31.100.1"), np.uint32)),
            ctx.upload(np.full(n, abi.raw_port(10001), np.uint16)),
            ctx.upload((np.arange(n, dtype=np.uint64) * span).astype(np.uint32))]
    cap = n * span + 64
    out = ctx.alloc(cap)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*bytes.fromhex("6805ca95f8ec")),
                       (C.c_uint8 * 6)(*bytes.fromhex("6805ca95fa64")), abi.raw_ip("172.31.100.2"))
    bt = abi.TxBatch(bufs[0].ptr, pay.nbytes, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, n)
    ot = abi.TxOut(out.ptr, cap, bufs[6].ptr)
    f = abi.lib().udpdk_gpu_tx_build_flags

    def args(flags):
        return (ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot), mtu, flags)

    # parity of the two forms on this very batch
    abi._check(f(*args(0)), "udpdk_gpu_tx_build_flags")
    off = ctx.download(out, np.uint8, n * span)
    abi._check(f(*args(abi.TX_UDP_CKSUM)), "udpdk_gpu_tx_build_flags")
    on = ctx.download(out, np.uint8, n * span)
    diff = np.nonzero(on != off)[0]
    field = (diff % span == 40) | (diff % span == 41)
    has = on.reshape(n, span)[:, 40:42].any(axis=1)
    if not field.all() or not has.all() or off.reshape(n, span)[:, 40:42].any():
        raise SystemExit(f"checksum form differs from flags 0 outside bytes 40-41 ({payload_len} B)")
    del on, off

    ev = bench.HipEvents(ctx)
    us = {0: [], abi.TX_UDP_CKSUM: []}
    for _ in range(reps):
        for flags in (0, abi.TX_UDP_CKSUM):
            for _ in range(5):
                abi._check(f(*args(flags)), "udpdk_gpu_tx_build_flags")
            ctx.sync()
            ev.record(0)
            for _ in range(steps):
                f(*args(flags))
            ev.record(1)
            ctx.sync()
            us[flags].append(round(1e3 * ev.elapsed_ms() / steps, 2))
    ev.close()
    for b in bufs + [out]:
        b.free()
    a, b = statistics.median(us[0]), statistics.median(us[abi.TX_UDP_CKSUM])
    what = f"TX {n} x {payload_len + 42} B frames" if nf.value == 1 else \
        f"TX {n} x {payload_len} B datagrams -> {nf.value} fragments at MTU {mtu}"
    nbytes = n * payload_len + n * span + 12 * n
    return {"workload": what, "steps": steps, "us_flags0": a, "us_cksum": b, "ratio": round(b / a, 4),
            "gbps_flags0": round(nbytes / a / 1e3, 1), "gbps_cksum": round(nbytes / b / 1e3, 1),
            "reps_flags0": us[0], "reps_cksum": us[abi.TX_UDP_CKSUM]}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = p.parse_args()
    ctx = abi.GpuContext(0, max_frames=1 << 22, max_lanes=4096)
    lines = []
    for plen, n, mtu in SHAPES:
        d = shape(ctx, plen, n, mtu, a.steps, a.reps)
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
