"""The multicast membership filter without a GPU: the model of mcast_util.py against the
hand-written vectors of golden/mcast_vectors.json, and the library's table builder
(udpdk_gpu_mcast_table_build, which runs the header's hash and probe) against the model and the same
vectors."""
import errno
import json
import os

import numpy as np
import pytest

import mcast_util as U
from udpdk_amd import abi

V = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcast_vectors.json")))


def pairs(members):
    return [(abi.raw_ip(g), l) for g, l in members]


def table_of(rows):
    return [(0, 0) if r is None else (abi.raw_ip(r[0]), r[1]) for r in rows]


def lib_table(members, slots):
    rc, tab = abi.mcast_table_build(np.array(members, U.MCAST_DTYPE) if members else np.zeros(0, U.MCAST_DTYPE), slots)
    return rc, [(int(g), int(l)) for g, l in tab]


# ---- the hash ------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V["hash"], ids=lambda v: f"{v['group']}-{v['lane']}")
def test_hash_literals(v):
    g = abi.raw_ip(v["group"])
    assert U.hash32(g, v["lane"]) == int(v["h"], 16)
    for slots in (2, 8, 1 << 20):
        assert U.start(g, v["lane"], slots) == v[f"start_{slots}"]
        # the header's hash: a lone member sits at its start index
        rc, tab = lib_table([(g, v["lane"])], slots)
        assert rc == 0 and tab[v[f"start_{slots}"]] == (g, v["lane"])
        assert sum(t != (0, 0) for t in tab) == 1


# ---- the table -----------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V["tables"], ids=lambda v: v["name"][:24])
def test_tables(v):
    want = table_of(v["table"])
    assert U.build(pairs(v["members"]), v["slots"]) == want
    rc, tab = lib_table(pairs(v["members"]), v["slots"])
    assert rc == 0 and tab == want
    for p in v.get("probes", []):
        assert U.probe(want, abi.raw_ip(p["group"]), p["lane"]) == (p["found"], p["probes"]), p
    for g, l in pairs(v["members"]):
        assert U.probe(want, g, l)[0]


@pytest.mark.parametrize("n,slots", [(0, 2), (1, 2), (2, 2), (5, 8), (8, 8), (300, 512), (512, 512), (1000, 4096)])
def test_builder_equals_model(n, slots):
    rng = np.random.default_rng(n * 31 + slots)
    seen, members = set(), []
    while len(members) < n:
        m = (int(rng.integers(224, 240)) | int(rng.integers(0, 4)) << 24, int(rng.integers(0, 64)))   # few groups: chains
        if m not in seen:
            seen.add(m)
            members.append(m)
    rc, tab = lib_table(members, slots)
    want = U.build(members, slots)
    assert rc == 0 and tab == want
    assert all(U.probe(want, g, l)[0] for g, l in members)
    if n == slots:
        assert all(t[0] != 0 for t in want)
        assert U.probe(want, abi.raw_ip("239.9.9.9"), 70) == (False, slots)     # bounded without an empty slot


def test_builder_errors():
    g = abi.raw_ip(U.G1)
    for slots in (0, 1, 3, 6, 1 << 21, (1 << 20) + 1):
        rc, tab = abi.mcast_table_build(np.array([(g, 0)], U.MCAST_DTYPE), slots)
        assert rc == -errno.EINVAL and np.all(tab.view(np.uint8) == 0xA5), slots   # nothing written
    assert lib_table([(g, 0), (g, 1), (g, 2)], 2)[0] == -errno.ENOSPC
    assert lib_table([(g, 0), (g, 1), (g, 0)], 8)[0] == -errno.EINVAL          # a pair given twice
    assert lib_table([(0, 1)], 8)[0] == -errno.EINVAL                          # group 0 is the empty mark
    rc, tab = lib_table([], 4)
    assert rc == 0 and tab == [(0, 0)] * 4
    L = abi.lib()
    m = np.array([(g, 0)], U.MCAST_DTYPE)
    assert L.udpdk_gpu_mcast_table_build(m.ctypes.data, 1, None, 2) == -errno.EINVAL
    assert L.udpdk_gpu_mcast_table_build(None, 1, m.ctypes.data, 2) == -errno.EINVAL
    assert U.slots_for(0) == 2 and U.slots_for(1) == 2 and U.slots_for(2) == 4 and U.slots_for(3) == 8
    assert U.slots_for(1 << 19) == 1 << 20


# ---- the filter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("v", V["filter"], ids=lambda v: v["name"][:24])
def test_filter_vectors(v):
    b = U.frames_to(v["dst"], 5000, 1)
    if "length" in v:
        b.length[:] = v["length"]
    fb = b.frames_bytes - v.get("frames_bytes_cut", 0)
    tab = U.build(pairs(v["members"]), v["slots"])
    m = U.model(b, v["lane_off"], v["lane_pkt"], v["lane_mc"], tab, n=v["n"], lane_cap=v.get("lane_cap"),
                frames_bytes=fb)
    assert list(m.lane_off) == v["want_lane_off"] and list(m.lane_pkt) == v["want_lane_pkt"]
    w = v["want_stats"]
    assert m.stats() == (w["kept"], w["removed"], w["member"], w["not_member"], w["bad_frame"], w["bad_index"],
                         w["truncated"])


def test_abi_records():
    import ctypes as C
    assert U.MCAST_DTYPE.itemsize == 8 and C.sizeof(abi.RxMcastStats) == 28


# ---- IGMP ----------------------------------------------------------------------------------------
def test_igmp_frames_pinned():
    f = V["igmp_frames"]
    mac = bytes.fromhex(f["src_mac"])
    for kind, build in (("report", U.report_frame), ("leave", U.leave_frame)):
        got = build(mac, f["src_ip"], f["group"])
        want = f[kind + "_fields"]
        assert got.hex() == f[kind] and len(got) == abi.IGMP_FRAME_BYTES
        assert got[:6].hex() == want["dst_mac"] and got[24:26].hex() == want["ip_cksum"]
        assert got[40:42].hex() == want["igmp_cksum"]
        assert U.rfc1071(got[14:38]) == 0xFFFF and U.rfc1071(got[38:46]) == 0xFFFF


def test_rfc1071():
    assert U.rfc1071(bytes.fromhex("0001f203f4f5f6f7")) == 0xDDF2          # RFC 1071 section 3's example
    assert U.rfc1071(b"\x12") == 0x1200 and U.rfc1071(b"") == 0 and U.rfc1071(b"\xff\xff\x00\x01") == 1


@pytest.mark.parametrize("c", V["igmp_queries"]["cases"], ids=lambda c: c["name"][:28])
def test_igmp_query_vectors(c):
    groups = [abi.raw_ip(g) for g in V["igmp_queries"]["groups"]]
    f = bytes.fromhex(c["frame"])
    assert U.igmp_classify(f, groups) == c["counter"]
    # and as a batch of one: the counters, and the report a query that is answered gets
    b = U.pack([f])
    st, frames, idx = U.igmp_model(b, [U.V_NOT_UDP], U.SRC_MAC, "10.0.0.2", groups)
    want = dict.fromkeys(U.IGMP_STATS, 0)
    if c["counter"]:
        want["igmp"] = want[c["counter"]] = 1
    if c["counter"] in ("general", "specific"):
        want["reports"] = 1
        assert [x.hex() for x in frames] == [V["igmp_frames"]["report"]] and idx == [0]
    else:
        assert frames == []
    assert st == want
    assert U.igmp_model(b, [0], U.SRC_MAC, "10.0.0.2", groups)[0] == dict.fromkeys(U.IGMP_STATS, 0)   # not a candidate


def test_igmp_model_answer_set():
    """A general and specific queries in one batch: one report per group, in index order, 224.0.0.1
    never; max_reports cuts a tail."""
    groups = [abi.raw_ip(g) for g in ("239.0.0.9", U.ALL_HOSTS, U.G1, U.G2)]
    b = U.pack([U.query(group=U.G2), U.query(), U.query(group=U.G1), U.query(group=U.G1), U.query(group=U.ALL_HOSTS)])
    st, frames, idx = U.igmp_model(b, [U.V_NOT_UDP] * 5, U.SRC_MAC, "10.0.0.2", groups)
    assert (st["general"], st["specific"], st["reports"], st["no_room"]) == (1, 4, 4, 0) and idx == [0, 1, 2, 3]
    st, frames, idx = U.igmp_model(b, [U.V_NOT_UDP] * 4, U.SRC_MAC, "10.0.0.2", groups, n=4, max_reports=2)
    assert (st["reports"], st["no_room"]) == (2, 1) and idx == [0, 2]
    assert frames[1] == U.report_frame(U.SRC_MAC, "10.0.0.2", U.G1)


# ---- the host's builder --------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.environ.get("UDPDK_IGMP_FRAME_CHECK") or os.path.join(ROOT, "build", "igmp_frame_check")


def _frame_tool(kind: str, mac: bytes, ip: str, group: str) -> bytes:
    """csrc/host/igmp_frame.h, what the library queues for a join and a leave, through the stand-alone
    build/igmp_frame_check (UDPDK_IGMP_FRAME_CHECK names another build of it: `make igmp-asan`)."""
    import subprocess
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/igmp_frame_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([CHECK, kind, ":".join(f"{b:02x}" for b in mac), ip, group], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return bytes.fromhex(out.stdout.strip())


def test_host_built_join_and_leave_bytes():
    f = V["igmp_frames"]
    mac = bytes.fromhex(f["src_mac"])
    assert _frame_tool("report", mac, f["src_ip"], f["group"]).hex() == f["report"]
    assert _frame_tool("leave", mac, f["src_ip"], f["group"]).hex() == f["leave"]
    for mac, ip, g in ((bytes.fromhex("02a1b2c3d4e5"), "192.168.7.9", "224.0.0.251"),
                       (mac, "172.31.100.2", "239.255.255.255"), (mac, "10.0.0.2", "225.129.2.3")):   # bit 23 of the group
        assert _frame_tool("report", mac, ip, g) == U.report_frame(mac, ip, g)
        assert _frame_tool("leave", mac, ip, g) == U.leave_frame(mac, ip, g)
    # on the wire a report of ours is other_type to the stage: the stack does not answer itself
    assert U.igmp_classify(bytes.fromhex(f["report"]), [abi.raw_ip(f["group"])]) == "other_type"
