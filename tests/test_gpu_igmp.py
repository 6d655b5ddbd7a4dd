"""The IGMPv2 query responder on the GPU (udpdk_gpu_igmp_reply, udpdk_gpu_pipe_igmp_reply) against
the model of mcast_util.py, which test_mcast_ref.py pins to hand-written vectors: every counter, the
reports' bytes and the group indices, exactly, and nothing written past them."""
import ctypes as C
import errno
import json
import os

import numpy as np
import pytest

import mcast_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

PAD = 8
OUR_IP = "10.0.0.2"
V = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcast_vectors.json")))
GROUPS = [abi.raw_ip(g) for g in ("239.0.0.9", U.ALL_HOSTS, U.G1, U.G2, U.G3)]
UDP = abi.V_DELIVERED


def cfg(ip=OUR_IP, mac=U.SRC_MAC):
    return abi.TxConfig((C.c_uint8 * 6)(*mac), (C.c_uint8 * 6)(*U.QUERIER_MAC), abi.raw_ip(ip))


def run(ctx, b, meta, groups, what="", pipe=0, max_reports=None, n=None, frames_bytes=None):
    """The stage on the device against the model."""
    meta = np.asarray(meta, np.uint32)
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length, None)
    db.frames_bytes = b.frames_bytes if frames_bytes is None else frames_bytes
    try:
        g = abi.igmp_run(ctx, cfg(), db, meta, groups, max_reports=max_reports, n=n, pipe=pipe, pad=PAD)
    finally:
        for x in (db.frames, db.offset, db.length):
            x.free()
    st, frames, idx = U.igmp_model(b, meta, U.SRC_MAC, OUR_IP, groups, max_reports=max_reports, n=n,
                                   frames_bytes=db.frames_bytes)
    assert g["rc"] == 0 and g["stats"] == st, what
    assert g["stats_rc"] == (-errno.ENOSPC if st["no_room"] else 0), what
    r = st["reports"]
    for k in range(r):
        assert bytes(g["slots"][k][:46]) == frames[k], f"{what}: report {k}"
        assert not g["slots"][k][46:].any(), f"{what}: slot {k} bytes 46-63"
    assert list(g["group_index"][:r]) == idx, what
    assert np.all(g["slots"][r:] == 0xA5) and np.all(g["group_index"][r:] == 0xA5A5A5A5), f"{what}: wrote past the reports"
    return st


def traffic(n, seed):
    """n UDP datagrams (not candidates) to pad a batch with."""
    return [bytes(r) for r in U.frames_to([U.OUR_IP] * n, 5000, seed).rows]


def scatter(n, queries, seed):
    """A batch of n frames, `queries` at random places among UDP traffic: (batch, meta)."""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(n, len(queries), replace=False)) if queries else []
    frames = traffic(n, seed)
    meta = np.full(n, UDP, np.uint32)
    for p, q in zip(at, queries):
        frames[p] = q
        meta[p] = U.V_NOT_UDP | 0x10                                  # (other bits of the word are not looked at)
    return U.pack(frames, gaps=rng.integers(0, 4, n)), meta


def test_geometry():
    e, k = abi.igmp_geometry(1)
    assert (e, k) == (1024, 1) and abi.igmp_geometry(0) == (e, 1)
    assert abi.igmp_geometry(e) == (e, 1) and abi.igmp_geometry(e + 1) == (e, 2)


@pytest.mark.parametrize("c", V["igmp_queries"]["cases"], ids=lambda c: c["name"][:28])
def test_one_frame_per_counter(gpu_ctx, c):
    b = U.pack([bytes.fromhex(c["frame"])])
    st = run(gpu_ctx, b, [U.V_NOT_UDP], [abi.raw_ip(g) for g in V["igmp_queries"]["groups"]], c["name"])
    if c["counter"]:
        assert st["igmp"] == st[c["counter"]] == 1
    st = run(gpu_ctx, b, [UDP], [abi.raw_ip(U.G1)], c["name"] + ", not a candidate")
    assert not any(st.values())


def test_bad_frames(gpu_ctx):
    """Candidates shorter than 34 bytes or out of range are counted and not read."""
    q = U.query()
    b = U.pack([q, q, q, q[:33], q])
    b.length[1] = 33
    b.offset[2] = 0xFFFFFFF0
    st = run(gpu_ctx, b, [U.V_NOT_UDP] * 5, GROUPS, "short / wrapped")
    assert (st["bad_frame"], st["general"]) == (3, 2)
    st = run(gpu_ctx, b, [U.V_NOT_UDP] * 5, GROUPS, "cut", frames_bytes=b.frames_bytes - 1)
    assert (st["bad_frame"], st["general"]) == (4, 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, "two"])
def test_frame_counts(gpu_ctx, n):
    """Queries of every kind among UDP traffic, the last frame one of them; n up to two workgroups'
    worth, and one frame more than one workgroup's."""
    e, _ = abi.igmp_geometry(1)
    n = 2 * e if n == "two" else n
    kinds = [U.query(), U.query(group=U.G1), U.query(group=U.G2, ihl=5), U.query(group="239.9.9.9"),
             U.query(group=U.G1, typ=0x16), U.query(igmp_cksum=False), U.query(ip_cksum=False), U.query(proto=1),
             U.query(dst=U.G1), U.query(msg_len=12)]
    qs = [kinds[k % len(kinds)] for k in range(min(n, 40))]
    for nn in sorted({n, n + (1 if n >= e else 0)}):
        b, meta = scatter(nn, qs[:-1], nn)
        last = U.query(group=U.G3)
        frames = [bytes(b.frames[o:o + l]) for o, l in zip(b.offset, b.length)]
        frames[-1] = last
        meta[-1] = U.V_NOT_UDP
        st = run(gpu_ctx, U.pack(frames, gaps=[k % 4 for k in range(nn)]), meta, GROUPS, f"n={nn}")
        assert st["specific"] >= 1 and st["igmp"] == sum(v for k, v in st.items() if k in
                                                         ("malformed", "bad_cksum", "other_type", "bad_dst", "general",
                                                          "not_member", "specific"))


def test_general_and_specific_one_report_each(gpu_ctx):
    """A general query and specific queries for the same groups, some of them twice and in two
    workgroups: each group gets one report; 224.0.0.1 only when asked for by name."""
    e, _ = abi.igmp_geometry(1)
    qs = [U.query(group=U.G2), U.query(), U.query(group=U.G1), U.query(group=U.G1), U.query(), U.query(group=U.G3)]
    b, meta = scatter(e + 300, qs, 5)
    st = run(gpu_ctx, b, meta, GROUPS, "general + specific")
    assert (st["general"], st["specific"], st["reports"]) == (2, 4, 4)
    b, meta = scatter(700, qs + [U.query(group=U.ALL_HOSTS)], 6)
    st = run(gpu_ctx, b, meta, GROUPS, "... and all-hosts by name")
    assert (st["specific"], st["reports"]) == (5, 5)
    b, meta = scatter(50, [U.query(group=U.G3), U.query(group=U.G1)], 7)
    st = run(gpu_ctx, b, meta, GROUPS, "specific only")
    assert (st["general"], st["reports"]) == (0, 2)


@pytest.mark.parametrize("n_groups", [1, 64, 65, 4096])
def test_group_counts_and_room(gpu_ctx, n_groups):
    """A general query over n_groups groups (224.0.0.1 among them when there is room), with room
    for none, all but one and all of the reports; then specific queries for the first and last."""
    groups = [abi.raw_ip(f"239.{1 + k // 65536}.{(k >> 8) & 255}.{k & 255}") for k in range(n_groups)]
    if n_groups > 1:
        groups[n_groups // 2] = abi.raw_ip(U.ALL_HOSTS)
    want = n_groups - (n_groups > 1)
    b, meta = scatter(20, [U.query()], n_groups)
    for room in sorted({0, want - 1, want}):
        st = run(gpu_ctx, b, meta, groups, f"{n_groups} groups, room {room}", max_reports=room)
        assert (st["reports"], st["no_room"]) == (room, want - room)
    first, last = (".".join(str(x) for x in int(g).to_bytes(4, "little")) for g in (groups[0], groups[-1]))
    b, meta = scatter(20, [U.query(group=last), U.query(group=first)], n_groups + 1)
    st = run(gpu_ctx, b, meta, groups, f"{n_groups} groups, first and last")
    assert st["specific"] == 2 and st["reports"] == len({first, last})


def test_no_candidate_and_empty(gpu_ctx):
    b, meta = scatter(1500, [], 9)
    st = run(gpu_ctx, b, meta, GROUPS, "no candidate")
    assert not any(st.values())
    st = run(gpu_ctx, b, meta, [], "no groups", max_reports=4)
    assert not any(st.values())
    b, meta = scatter(30, [U.query(), U.query(group=U.G1)], 10)
    st = run(gpu_ctx, b, meta, [], "queries, no groups", max_reports=4)
    assert (st["general"], st["not_member"], st["reports"]) == (1, 1, 0)
    st = run(gpu_ctx, b, meta, GROUPS, "n = 0", n=0)
    assert not any(st.values())


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_alignments_and_lengths(gpu_ctx, residue):
    """Queries at each offset residue, the last one ending the batch; an odd-length message (padded
    with a zero byte for the sum), an IHL 15 header, a long message and Ethernet padding."""
    qs = [U.query(group=U.G1), U.query(msg_len=9), U.query(group=U.G2, msg_len=13), U.query(ihl=15),
          U.query(group=U.G3, ihl=15, msg_len=11), U.query(msg_len=1400), U.query(group=U.G1, pad=14),
          U.query(msg_len=9, igmp_cksum=False), U.query(ihl=15, ip_cksum=False), U.query(group=U.G2)]
    for k, q in enumerate(qs):
        # (k 46-byte ICMP frames before it: the query starts at residue + 46 k, every residue mod 4 over k)
        b = U.pack([U.query(proto=1)] * k + [q], gaps=[residue] + [0] * k, tail=0)
        st = run(gpu_ctx, b, [U.V_NOT_UDP] * (k + 1), GROUPS, f"query {k} residue {residue}")
        assert st["igmp"] == 1 and st["malformed"] + st["bad_cksum"] == (k in (7, 8))


@pytest.mark.parametrize("pipe", [1, 2, 3])
def test_pipe_form(gpu_ctx, pipe):
    L = abi.lib()
    st = abi.IgmpStats()
    fresh = abi.GpuContext(0, max_frames=1024, max_lanes=1)
    try:
        assert L.udpdk_gpu_pipe_igmp_stats(fresh.handle, pipe, C.byref(st)) == -errno.ENOENT
        assert L.udpdk_gpu_igmp_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
    finally:
        fresh.close()
    b, meta = scatter(1300, [U.query(group=U.G1), U.query(), U.query(group="239.9.9.9")], 20 + pipe)
    gpu_ctx.pipeline(4)
    try:
        for rep in range(2):                                          # (the second launch finds the answer set zeroed)
            s = run(gpu_ctx, b, meta, GROUPS, f"pipe {pipe} rep {rep}", pipe=pipe)
            assert (s["general"], s["specific"], s["not_member"], s["reports"]) == (1, 1, 1, 4)
        s = run(gpu_ctx, b, meta, GROUPS, "context stream with pipes on")
        assert s["reports"] == 4
    finally:
        gpu_ctx.pipeline(1)


def test_arguments(gpu_ctx):
    L = abi.lib()
    b, meta = scatter(10, [U.query()], 30)
    db = abi.rx_upload(gpu_ctx, b.frames, b.offset, b.length, None)
    db.frames_bytes = b.frames_bytes
    bufs = [gpu_ctx.upload(meta), gpu_ctx.upload(np.array(GROUPS, np.uint32)),
            gpu_ctx.upload(np.full(64 * 8, 0xA5, np.uint8)), gpu_ctx.upload(np.full(8, 0xA5A5A5A5, np.uint32))]
    md, gd, sd, xd = bufs
    bt = abi.RxBatch(db.frames.ptr, db.frames_bytes, db.offset.ptr, db.length.ptr, None, b.n)

    def call(h=gpu_ctx.handle, c=cfg(), bt_=bt, m=md.ptr, g=gd.ptr, ng=len(GROUPS), slots=sd.ptr, idx=xd.ptr, room=8,
             pipe=0):
        o = abi.IgmpOut(slots, idx, room)
        args = (C.byref(c) if c else None, C.byref(bt_) if bt_ else None, m, g, ng, C.byref(o))
        return L.udpdk_gpu_pipe_igmp_reply(h, pipe, *args) if pipe else L.udpdk_gpu_igmp_reply(h, *args)
    try:
        assert call(h=None) == -errno.EINVAL and call(c=None) == -errno.EINVAL and call(bt_=None) == -errno.EINVAL
        assert call(m=None) == -errno.EINVAL and call(g=None) == -errno.EINVAL
        assert call(ng=abi.IGMP_MAX_GROUPS + 1) == -errno.EINVAL and call(c=cfg("0.0.0.0")) == -errno.EINVAL
        assert call(slots=None) == -errno.EINVAL and call(idx=None) == -errno.EINVAL
        assert call(slots=sd.ptr + 8) == -errno.EINVAL                                  # 16-byte aligned slots
        assert call(slots=db.frames.ptr) == -errno.EINVAL and call(idx=db.frames.ptr) == -errno.EINVAL   # overlap
        assert call(pipe=4) == -errno.EINVAL and call(pipe=-1) == -errno.EINVAL
        assert L.udpdk_gpu_igmp_reply(gpu_ctx.handle, C.byref(cfg()), C.byref(bt), md.ptr, gd.ptr, 5, None) == -errno.EINVAL
        assert L.udpdk_gpu_igmp_geometry(5, None, None) == -errno.EINVAL
        gpu_ctx.sync()
        assert np.all(gpu_ctx.download(sd, np.uint8, 64 * 8) == 0xA5)                   # none of these enqueued anything
        assert call(g=None, ng=0) == 0 and call() == 0
        st = abi.IgmpStats()
        assert L.udpdk_gpu_igmp_stats(gpu_ctx.handle, C.byref(st)) == 0 and (st.general, st.reports) == (1, 4)
    finally:
        for x in bufs + [db.frames, db.offset, db.length]:
            x.free()
