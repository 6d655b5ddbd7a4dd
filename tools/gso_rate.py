"""What segmented sends (UDP_SEGMENT) buy on the socket path, and what the segment plan costs, on one
box in one run:

  socket path   the same bytes queued as N-byte datagrams by udpdk_sendto and as 64-segment sends of
                segment size N (udpdk_sendto on a socket with the option set), each round queued on one
                socket and drained by udpdk_tx_drain: calls queued per second, datagrams queued per
                second and datagrams drained per second (the drain: selection, staging, the GPU work
                and the copy back). The calls go through ctypes, whose cost per call both forms pay.
  device        udpdk_gpu_tx_segment_plan for 2^14 sends x 64 segments beside udpdk_gpu_tx_build_flags
                over the plan's arrays (the same output), back-to-back calls on one context

  python tools/gso_rate.py [--seg 1000] [--rounds 20] [--calls 20] [--reps 5] [--out profiles/NAME.txt]

Before timing, the drained frames of the two forms are compared with each other, and the plan's arrays
and counts with their closed form. One JSON line with the medians and every repetition."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from udpdk_amd import abi  # noqa: E402

SEGS = abi.GSO_MAX_SEGS
SENDS_PER_ROUND = 31                       # 31 x 64 = 1984 datagrams: what one socket's TX ring takes
DST = ("172.31.100.21", 4000)
INI = ("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.1\n[port0_dst]\nmac_addr = 68:05:ca:95:fa:64\n"
       "[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n")


def socket_path(seg: int, rounds: int, reps: int) -> dict:
    L = abi.lib()
    api = abi.HostApi()
    with tempfile.TemporaryDirectory() as d:
        ini = os.path.join(d, "udpdk.ini")
        with open(ini, "w") as fh:
            fh.write(INI)
        argv = (C.c_char_p * 4)(b"prog", b"-c", ini.encode(), None)
        if L.udpdk_init(3, argv):
            raise SystemExit(f"udpdk_init: errno {api.errno()}")
    plain, gso = api.socket(), api.socket()
    assert api.bind(plain, "0.0.0.0", 10001) == 0 and api.bind(gso, "0.0.0.0", 10001 + 1) == 0
    assert api.setsockopt(gso, abi.SOL_UDP, abi.UDP_SEGMENT, seg) == 0
    n_dg = SENDS_PER_ROUND * SEGS
    big = bytes((i * 7) & 0xFF for i in range(seg * SEGS))
    one = C.create_string_buffer(big[:seg], seg)
    whole = C.create_string_buffer(big, len(big))
    addr = C.create_string_buffer(abi.sockaddr_in(*DST), 16)
    cap, maxf = n_dg * (seg + 42) + 4096, n_dg + 64
    out, off, ln = np.zeros(cap, np.uint8), np.zeros(maxf, np.uint32), np.zeros(maxf, np.uint16)
    n_out = C.c_uint32()

    def queue_plain():
        for _ in range(n_dg):
            L.udpdk_sendto(plain, one, seg, 0, addr, 16)
        return n_dg

    def queue_gso():
        for _ in range(SENDS_PER_ROUND):
            L.udpdk_sendto(gso, whole, len(big), 0, addr, 16)
        return SENDS_PER_ROUND

    def drain():
        if L.udpdk_tx_drain(out.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, maxf, C.byref(n_out)):
            raise SystemExit(f"udpdk_tx_drain: errno {api.errno()}")
        if n_out.value != n_dg or api.tx_pending():
            raise SystemExit(f"drained {n_out.value} of {n_dg}")

    # the two forms produce the same frames but for the source port
    queue_plain()
    drain()
    a = out[:n_dg * (seg + 42)].reshape(n_dg, seg + 42).copy()
    queue_gso()
    drain()
    b = out[:n_dg * (seg + 42)].reshape(n_dg, seg + 42).copy()
    # every segment of a send repeats the first one's payload in the plain form: compare piecewise
    want = np.frombuffer(big, np.uint8).reshape(SEGS, seg)
    same_hdr = np.array_equal(np.delete(a[:, :42], [34, 35], axis=1), np.delete(b[:, :42], [34, 35], axis=1))
    if not same_hdr or not np.array_equal(b[:SEGS, 42:], want) or not np.array_equal(a[0, 42:], want[0]):
        raise SystemExit("socket path: the two forms' frames differ")

    res = {k: [] for k in ("plain_calls_per_s", "plain_queued_dgrams_per_s", "plain_drained_dgrams_per_s",
                           "gso_calls_per_s", "gso_queued_dgrams_per_s", "gso_drained_dgrams_per_s")}
    for _ in range(reps):
        for name, fn in (("plain", queue_plain), ("gso", queue_gso)):
            tq = td = 0.0
            calls = 0
            for _ in range(rounds):
                t0 = time.perf_counter()
                calls += fn()
                t1 = time.perf_counter()
                drain()
                t2 = time.perf_counter()
                tq += t1 - t0
                td += t2 - t1
            res[f"{name}_calls_per_s"].append(round(calls / tq))
            res[f"{name}_queued_dgrams_per_s"].append(round(rounds * n_dg / tq))
            res[f"{name}_drained_dgrams_per_s"].append(round(rounds * n_dg / td))
    counts = api.gso_counts()
    L.udpdk_cleanup()
    med = {k: statistics.median(v) for k, v in res.items()}
    med.update({"reps_" + k: v for k, v in res.items()})
    med["gso_counts"] = counts
    med["dgrams_per_round"] = n_dg
    return med


def device(calls: int, reps: int) -> dict:
    L = abi.lib()
    K, g = 1 << 14, 64
    N = K * SEGS
    ctx = abi.GpuContext(0, max_frames=1024, max_lanes=4)
    slots = [(0, abi.raw_port(20000 + s), 1) for s in range(4)]
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 4, slots=slots))
    pbytes = K * g * SEGS
    pay = ctx.upload(np.random.default_rng(3).integers(0, 256, pbytes + 16, dtype=np.uint8))
    j = np.arange(K)
    s_off = (j * g * SEGS).astype(np.uint32)
    ins = [ctx.upload(x) for x in (s_off, np.full(K, g * SEGS, np.uint16), np.full(K, g, np.uint16),
                                   (j % 4).astype(np.int32), (0x0A000000 + j).astype(np.uint32),
                                   (j & 0xFFFF).astype(np.uint16))]
    sd = abi.TxSends(pay.ptr, pbytes, *[x.ptr for x in ins], K)
    sizes = (4 * N, 2 * N, 4 * N, 4 * N, 2 * N, 4 * (N + 1), 4 * (K + 1))
    arrs = [ctx.alloc(x) for x in sizes]
    plan = abi.TxSegmentPlan(*[x.ptr for x in arrs], N)
    span = g + 42
    out_cap = N * span
    out = ctx.alloc(out_cap + 64)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*bytes.fromhex("6805ca95f8ec")), (C.c_uint8 * 6)(*bytes.fromhex("6805ca95fa64")),
                       abi.raw_ip("172.31.100.1"))
    tb = abi.TxBatch(pay.ptr, pbytes, arrs[0].ptr, arrs[1].ptr, arrs[2].ptr, arrs[3].ptr, arrs[4].ptr, N)
    to = abi.TxOut(out.ptr, out_cap + 64, arrs[5].ptr)

    def run_plan():
        return L.udpdk_gpu_tx_segment_plan(ctx.handle, C.byref(sd), 0, SEGS, out_cap, C.byref(plan))

    def run_build():
        return L.udpdk_gpu_tx_build_flags(ctx.handle, C.byref(cfg), C.byref(tb), C.byref(to), 0, 0)

    abi._check(run_plan(), "udpdk_gpu_tx_segment_plan")
    rc, st = abi.tx_segment_stats(ctx)
    m = np.arange(N)
    checks = [(arrs[0], np.uint32, N, (m * g).astype(np.uint32)), (arrs[1], np.uint16, N, np.full(N, g, np.uint16)),
              (arrs[2], np.int32, N, ((m // SEGS) % 4).astype(np.int32)),
              (arrs[5], np.uint32, N + 1, (np.arange(N + 1) * span).astype(np.uint32)),
              (arrs[6], np.uint32, K + 1, (np.arange(K + 1) * SEGS).astype(np.uint32))]
    if rc or (st.segments, st.sends, st.frames, st.bytes_needed) != (N, K, N, out_cap):
        raise SystemExit(f"device: stats {rc} {[getattr(st, k) for k in abi.SEGMENT_STATS]}")
    for buf, dt, cnt, want in checks:
        if not np.array_equal(ctx.download(buf, dt, cnt), want):
            raise SystemExit("device: the plan differs from its closed form")
    abi._check(run_build(), "udpdk_gpu_tx_build_flags")
    ctx.sync()
    us = {"plan_us": [], "build_us": []}
    for _ in range(reps):
        for name, fn in (("plan_us", run_plan), ("build_us", run_build)):
            for _ in range(3):
                abi._check(fn(), name)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            ctx.sync()
            us[name].append(round(1e6 * (time.perf_counter() - t0) / calls, 2))
    ctx.close()
    res = {"sends": K, "segments": N, "seg_bytes": g, "output_bytes": out_cap, "calls": calls}
    for name, v in us.items():
        res[name] = statistics.median(v)
        res["reps_" + name] = v
    res["plan_over_build"] = round(res["plan_us"] / res["build_us"], 4)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seg", type=int, default=1000, help="segment size N in bytes (64 N <= 65507)")
    p.add_argument("--rounds", type=int, default=20, help="queue + drain rounds per repetition")
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = p.parse_args()
    if not 0 < a.seg * SEGS <= 65507:
        raise SystemExit("--seg: a 64-segment send must fit one datagram's 65507 bytes")
    res = {"label": "self-run: one process on one MI355X box, wall-clock times", "seg": a.seg, "segs_per_send": SEGS, "rounds": a.rounds, "socket_path": socket_path(a.seg, a.rounds, a.reps),
           "device": device(a.calls, a.reps)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
