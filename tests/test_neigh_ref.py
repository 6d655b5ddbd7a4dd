"""The neighbour cache without a GPU:
- the model (tests/neigh_util.py) against cases written out by hand (tests/golden/neigh_vectors.json);
- udpdk_gpu_neigh_class, the host statement of rules R1-R4 the kernel compiles too, against the model;
- the symbols, struct sizes and argument errors that need no device."""
import ctypes as C
import errno
import json
import os
import subprocess

import numpy as np
import pytest

import arp_util as A
import neigh_util as U
from udpdk_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "neigh_vectors.json")))


def _table(rows):
    return {U.raw(ip): (bytes.fromhex(mac), state, stamp) for ip, mac, state, stamp in rows}


def _init(case):
    return U.Table(case["entries"], [(ip, bytes.fromhex(mac), st, ts) for ip, mac, st, ts in case["init"]])


@pytest.mark.parametrize("case", VEC["learn"], ids=[c["name"] for c in VEC["learn"]])
def test_learn_model_against_hand_written_cases(case):
    fl = [A.arp_frame(op=f["op"], sha=bytes.fromhex(f["sha"]), spa=f["spa"], tpa=f["tpa"], pad_to=60 * (k % 2))
          for k, f in enumerate(case["frames"])]
    buf, nb, off, ln = A.pack(fl, aligns=[5 * k + 3 for k in range(len(fl))])
    tab = _init(case)
    R = U.learn(tab, U.cfg(), buf, nb, off, ln, A.host_meta(buf, off, ln), case["now"])
    assert R["stats"] == dict({k: 0 for k in U.LEARN_FIELDS}, **case["stats"])
    assert tab.as_map() == _table(case["table"])


@pytest.mark.parametrize("case", VEC["resolve"], ids=[c["name"] for c in VEC["resolve"]])
def test_resolve_model_against_hand_written_cases(case):
    c = U.cfg(netmask=case["netmask"], gateway=case["gateway"], ttl_ms=case["ttl_ms"], retrans_ms=case["retrans_ms"],
              flags=case["flags"])
    tab = _init(case)
    dst = [U.raw(d) for d in case["dst"]]
    R = U.resolve(tab, c, dst, [0] * len(dst), case["now"])
    assert [U.CLASS_NAMES[s] for s in R["state"]] == case["class"]
    got = [(int(lo) | int(hi) << 32).to_bytes(8, "little")[:6].hex() for lo, hi in R["dmac"]]
    assert got == case["mac"]
    assert R["sockfd_out"].tolist() == case["sockfd_out"]
    assert R["req_hops"] == [U.raw(h) for h in case["requests"]]
    for r, h in enumerate(R["req_hops"]):
        f = bytes(R["req"][r])
        assert f[:6] == b"\xff" * 6 and f[6:12] == U.OUR_MAC and f[12:22] == bytes.fromhex("08060001080006040001")
        assert f[22:28] == U.OUR_MAC and f[28:32] == U.raw(U.OUR_IP).to_bytes(4, "little") and f[32:38] == bytes(6)
        assert f[38:42] == h.to_bytes(4, "little") and not any(f[42:])
    assert tab.as_map() == _table(case["table"])


def test_model_request_limit_and_skips():
    c = U.cfg(retrans_ms=0)                                         # taken as 1: one request per next hop and call
    tab = U.Table(8)
    dst = [U.raw(f"172.31.100.{60 + k % 3}") for k in range(9)]
    sock = [0, 0, -1, 0, 0, 0, 0, 0, 0]
    R = U.resolve(tab, c, dst, sock, 10, req_cap=2)
    assert R["stats"]["requests"] == 2 and R["stats"]["no_room"] == 1 and R["req_origin"].tolist() == [0, 1]
    assert R["req_hops"] == dst[:2] + [dst[5]]                      # .62 is first asked for by datagram 5
    assert R["stats"]["skipped"] == 1 and R["stats"]["inserted"] == 3 and R["stats"]["incomplete"] == 5
    assert R["stats"]["unresolved"] == 8 and R["sockfd_out"].tolist() == [-1] * 9
    assert all(v[1] == U.INCOMPLETE and v[2] == 10 for v in tab.d.values()) and len(tab.d) == 3


# (destination, netmask, gateway) -> (class, next hop, mac); the stack is 172.31.100.1
CLASS_CASES = [
    ("255.255.255.255", "255.255.255.0", "0.0.0.0", "bcast", None, "ffffffffffff"),
    ("255.255.255.255", "0.0.0.0", "0.0.0.0", "bcast", None, "ffffffffffff"),
    ("172.31.100.255", "255.255.255.0", "0.0.0.0", "bcast", None, "ffffffffffff"),          # directed, /24
    ("172.31.100.3", "255.255.255.252", "0.0.0.0", "bcast", None, "ffffffffffff"),          # directed, /30
    ("172.31.100.255", "255.255.255.252", "172.31.100.2", "lookup", "172.31.100.2", None),  # off-link under /30
    ("172.31.100.255", "0.0.0.0", "0.0.0.0", "lookup", "172.31.100.255", None),             # no mask: no directed form
    ("172.31.101.255", "255.255.255.0", "172.31.100.254", "lookup", "172.31.100.254", None),
    ("224.0.0.1", "255.255.255.0", "0.0.0.0", "mcast", None, "01005e000001"),
    ("239.255.255.255", "255.255.255.0", "0.0.0.0", "mcast", None, "01005e7fffff"),          # the 23-bit fold
    ("224.128.0.1", "0.0.0.0", "0.0.0.0", "mcast", None, "01005e000001"),
    ("240.0.0.1", "255.255.255.0", "172.31.100.254", "lookup", "172.31.100.254", None),      # not multicast
    ("223.255.255.255", "255.255.255.0", "172.31.100.254", "lookup", "172.31.100.254", None),
    ("172.31.100.254", "255.255.255.0", "172.31.100.9", "lookup", "172.31.100.254", None),   # on-link at the mask edge
    ("172.31.101.0", "255.255.255.0", "172.31.100.9", "lookup", "172.31.100.9", None),       # off-link at the mask edge
    ("172.31.99.255", "255.255.255.0", "172.31.100.9", "lookup", "172.31.100.9", None),
    ("172.31.101.7", "255.255.254.0", "172.31.100.9", "lookup", "172.31.101.7", None),       # /23: on-link
    ("8.8.8.8", "0.0.0.0", "172.31.100.9", "lookup", "8.8.8.8", None),                       # netmask 0: all on-link
    ("8.8.8.8", "255.255.255.0", "0.0.0.0", "no_route", None, None),                         # gateway 0
    ("172.31.100.1", "255.255.255.0", "172.31.100.9", "self", "172.31.100.1", "6805ca95f8ec"),
    ("9.9.9.9", "255.255.255.0", "172.31.100.1", "self", "172.31.100.1", "6805ca95f8ec"),    # we are the gateway
]


@pytest.mark.parametrize("dst,mask,gw,cls,hop,mac", CLASS_CASES)
def test_class_function_and_model_against_hand_written_classes(dst, mask, gw, cls, hop, mac):
    c = U.cfg(netmask=mask, gateway=gw)
    want = (cls, U.raw(hop) if hop else 0, bytes.fromhex(mac) if mac else bytes(6))
    assert U.classify(c, U.raw(dst)) == want
    code, h, m = abi.neigh_class(c, U.raw(dst))
    names = {abi.NEIGH_C_BCAST: "bcast", abi.NEIGH_C_MCAST: "mcast", abi.NEIGH_C_NO_ROUTE: "no_route",
             abi.NEIGH_C_SELF: "self", abi.NEIGH_C_LOOKUP: "lookup"}
    assert (names[code], h, m) == want


def test_class_function_against_the_model_over_random_destinations():
    rng = np.random.default_rng(7)
    for mask, gw in (("255.255.255.0", "172.31.100.254"), ("255.255.0.0", "0.0.0.0"), ("0.0.0.0", "0.0.0.0"),
                     ("255.255.255.252", "172.31.100.2"), ("255.255.255.255", "172.31.100.1")):
        c = U.cfg(netmask=mask, gateway=gw)
        near = U.raw(U.OUR_IP) ^ (rng.integers(0, 1 << 12, 300).astype(np.uint32) << np.uint32(20))
        for dst in list(rng.integers(0, 1 << 32, 300, dtype=np.uint64)) + list(near) + [0, 0xFFFFFFFF]:
            code, h, m = abi.neigh_class(c, int(dst))
            cls, wh, wm = U.classify(c, int(dst))
            assert code == (abi.NEIGH_C_LOOKUP if cls == "lookup" else U.CLASS_NAMES.index(cls)) and (h, m) == (wh, wm), dst


def test_hash_statement_and_collision_helper():
    assert U.home(1, 8) == 0x9E3779B1 >> 29 and U.home(0x0100007F, 1024) == ((0x0100007F * 0x9E3779B1) & U.U32) >> 22
    ips = U.colliding_ips(8, 7, 5)
    assert len(set(ips)) == 5 and all(U.home(U.raw(i), 8) == 7 for i in ips)


def test_symbols_sizes_and_argument_errors_without_a_device():
    L = abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = {"udpdk_gpu_neigh_" + k for k in ("create", "set", "dump", "flush", "learn", "learn_stats", "resolve",
                                               "resolve_stats", "geometry", "class")}
    names |= {"udpdk_gpu_pipe_neigh_learn", "udpdk_gpu_pipe_neigh_learn_stats", "udpdk_gpu_tx_build_neigh"}
    assert names <= exported
    assert C.sizeof(abi.NeighEntry) == 16 and C.sizeof(abi.NeighCfg) == 36 and C.sizeof(abi.NeighOut) == 48
    assert C.sizeof(abi.NeighLearnStats) == 44 and C.sizeof(abi.NeighResolveStats) == 56
    T, B = abi.neigh_geometry()
    assert T >= 64 and T % 64 == 0 and B >= 64 and B % 64 == 0
    assert L.udpdk_gpu_neigh_geometry(None, None) == -errno.EINVAL
    c = U.cfg()
    h = C.c_uint32()
    mac = (C.c_uint8 * 6)()
    assert L.udpdk_gpu_neigh_class(None, 1, C.byref(h), mac) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_class(C.byref(c), 1, None, mac) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_class(C.byref(c), 1, C.byref(h), None) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_create(None, 8) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_set(None, None, 0) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_flush(None, 0) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_learn(None, C.byref(c), None, None, 0) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_resolve(None, C.byref(c), None, None, 0, 0, None) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_learn_stats(None, None) == -errno.EINVAL
    assert L.udpdk_gpu_neigh_resolve_stats(None, None) == -errno.EINVAL
    assert L.udpdk_gpu_tx_build_neigh(None, None, None, None, 0, 0, None) == -errno.EINVAL
