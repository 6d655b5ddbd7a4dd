"""udpdk_gpu_icmp_reply on the GPU through the C ABI, byte-exact against the model (tests/icmp_util.py):
reply_off, origin, every reply byte, every count, and nothing written past what the call may write.
The verdict words come from the oracle's RX of the same batch."""
import ctypes as C
import errno

import numpy as np
import pytest

import icmp_util as U
import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

FPB, _ = abi.icmp_geometry(1)


def _meta(buf, nb, off, ln):
    return O.rx(O.bindtable_from_lists(U.LISTS), buf, nb, off, ln, None, U.N_LANES)[0]


def _batch(frame_list, aligns=None):
    buf, nb, off, ln = U.pack(frame_list, aligns)
    return buf, nb, off, ln, _meta(buf, nb, off, ln)


def _check(ctx, bt, meta=None, *, pipe=0, guard=4096, pad=8, dev=None, **kw):
    """Run the stage and the model with the same arguments; compare everything. Returns the model."""
    buf, nb, off, ln, m0 = bt
    meta = m0 if meta is None else meta
    R = U.model(buf, nb, off, ln, meta, **kw)
    b = dev if dev is not None else abi.rx_upload(ctx, buf, off, ln)
    out_cap = kw.get("out_cap", max(64, R.stats["bytes_needed"] + 32))
    mr = kw.get("max_replies", len(off))
    g = abi.icmp_run(ctx, U.tx_config(), b, meta, flags=kw.get("flags", U.ALL), mtu=kw.get("mtu", 0),
                     err_limit=kw.get("err_limit", U.NO_LIMIT), out_cap=out_cap, max_replies=mr, pipe=pipe,
                     pad=pad, guard=guard)
    assert g["rc"] == 0
    k = R.stats["replies"]
    print("stats", U.stats_dict(g["stats"]), "model", R.stats)
    assert U.stats_dict(g["stats"]) == R.stats
    assert g["stats_rc"] == (-errno.ENOSPC if R.stats["no_room"] else 0)
    assert np.array_equal(g["reply_off"][:k + 1], R.reply_off)
    assert np.all(g["reply_off"][k + 1:] == 0xA5A5A5A5)             # nothing past reply_off[replies]
    assert np.array_equal(g["origin"][:k], R.origin) and np.all(g["origin"][k:] == 0xA5A5A5A5)
    end = int(R.reply_off[-1])
    assert end <= out_cap
    bad = np.flatnonzero(g["out"][:end] != R.out)
    assert bad.size == 0, (bad[:8], np.searchsorted(R.reply_off, bad[:8], side="right") - 1)
    assert np.all(g["out"][end:] == 0xEE)                           # the guard, and the room not used
    return R


def _filler(rng, n):
    return [U.udp_frame(rng, 10001, payload_len=int(rng.integers(0, 40))) for _ in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, FPB - 1, FPB, FPB + 1, 2 * FPB + 1])
def test_frame_counts(gpu_ctx, n):
    rng = np.random.default_rng(n)
    fl = _filler(rng, n)
    edges = sorted({p for p in (0, 63, 64, 127, 128, FPB - 1, FPB, FPB + 63, FPB + 64, 2 * FPB - 1, 2 * FPB, n - 1)
                    if 0 <= p < n})
    for j, p in enumerate(edges):
        fl[p] = U.echo_request(rng, 8 + 31 * j) if j % 2 == 0 else U.udp_frame(rng, U.CLOSED_PORT)
    R = _check(gpu_ctx, _batch(fl))
    assert R.stats["replies"] == len(edges) and list(R.origin) == edges


MSG_LENS = [8, 9, 10, 11, 12, 23, 24, 25, 63, 64, 65, 67, 68, 69, 255, 256, 257, 1479, 1480]


def test_echo_lengths_at_every_alignment(gpu_ctx):
    """Every message length at request offsets 0..15 mod 16; errors interleaved so that the replies
    start at every residue mod 16 as well. (67-69: around the lane / wave sum threshold.)"""
    rng = np.random.default_rng(7)
    fl, al = [], []
    for ml in MSG_LENS:
        for a in range(16):
            fl.append(U.echo_request(rng, ml))
            al.append(a)
            if (a + ml) % 3 == 0:
                fl.append(U.udp_frame(rng, U.CLOSED_PORT, payload_len=a))
                al.append(int(rng.integers(0, 16)))
    R = _check(gpu_ctx, _batch(fl, al))
    assert R.stats["echo_replied"] == 16 * len(MSG_LENS) and R.stats["unreach_sent"] > 50
    assert R.stats["echo_bad"] == 0
    starts = R.reply_off[:-1]
    echo_start = {int(starts[r]) % 16 for r in range(len(R.origin)) if R.out[int(starts[r]) + 34] == 0}
    assert echo_start == set(range(16)) and {int(s) % 16 for s in starts} == set(range(16))
    for ml in (1479, 1480):                                        # each long message at every output residue pair
        assert sum(1 for b in R.frames_out if len(b) == 34 + ml) == 16


def test_echo_refusals_padding_and_checksum_edges(gpu_ctx):
    rng = np.random.default_rng(11)
    corrupt = bytearray(U.echo_request(rng, 300))
    corrupt[200] ^= 0x10
    fl = [U.echo_request(rng, 8, pad_to=60), U.echo_request(rng, 13, pad_to=60), U.echo_request(rng, 26, pad_to=60),
          bytes(corrupt), U.echo_request(rng, 40, bad_cksum=True), U.echo_request(rng, 1000, bad_cksum=True),
          U.echo_request(rng, 40, tl=20 + 41), U.echo_request(rng, 40, tl=2000),       # tl beyond the frame
          U.echo_request(rng, 8, tl=27, pad_to=60), U.echo_request(rng, 8, tl=20, pad_to=60),   # tl < 28
          U.echo_request(rng, 48), U.echo_request(rng, 49),                              # tl 68, 69 around the MTU
          U.echo_request(rng, 8, ident=0, seq=0), U.echo_request(rng, 8, ident=0, seq=0, pad_to=60),
          U.echo_request(rng, 40, ident=0, seq=0, data=bytes(32)),
          U.echo_request(rng, 200, ident=0, seq=0, data=bytes(192)),
          U.echo_request(rng, 8, ident=0xFFFF, seq=0), U.echo_request(rng, 200, ident=0xFFFF, seq=0, data=bytes(192))]
    want = ["echo"] * 3 + ["echo_bad"] * 7 + ["echo"] * 8
    bt = _batch(fl, [3, 5, 7, 9, 11, 13, 15, 1, 2, 4, 6, 8, 10, 12, 14, 0, 1, 2])
    R = _check(gpu_ctx, bt)
    assert R.reason == want
    assert [bytes(b[36:38]) for b in R.frames_out[-6:]] == [b"\xff\xff"] * 4 + [b"\x00\x00"] * 2
    # an MTU of 68 (this test's choice): the 68-byte packet is answered, the 69-byte one and the long ones are not
    R = _check(gpu_ctx, bt, mtu=68)
    assert R.reason[10] == "echo" and R.reason[11] == R.reason[15] == R.reason[17] == "echo_bad"
    assert R.reason[:3] == ["echo"] * 3 and R.reason[12:15] == ["echo"] * 3


GATES = [("dst_other", "gate"), ("dst_bcast", "gate"), ("dst_mcast", "gate"), ("src_zero", "gate"),
         ("src_loop", "gate"), ("src_mcast", "gate"), ("ip_bad", ""), ("ihl6", ""), ("code1", "other"),
         ("type0", "other"), ("type13", "other"), ("tcp", "other"), ("frag", ""), ("udp_open", ""),
         ("udp_closed_badck", ""), ("udp_closed_badlen", ""), ("udp_closed", "unreach"), ("udp_nomatch", "unreach"),
         ("closed_other_dst", "gate"), ("echo", "echo")]


def test_every_gate(gpu_ctx):
    rng = np.random.default_rng(13)
    kinds = [k for k, _ in GATES] * 3
    fl = [U.kind_frame(rng, k) for k in kinds]
    for src in ("240.0.0.1", "255.255.255.255", "224.0.0.5", "127.9.9.9", "0.0.0.0"):   # each excluded source class
        fl.append(U.echo_request(rng, 20, src_ip=src))
        fl.append(U.udp_frame(rng, U.CLOSED_PORT, src_ip=src))
    bt = _batch(fl, rng.integers(0, 16, len(fl)).tolist())
    v = bt[4] & 0xF
    assert v[kinds.index("udp_closed")] == abi.V_NO_BIND and v[kinds.index("udp_nomatch")] == abi.V_NO_MATCH
    assert v[kinds.index("frag")] == abi.V_FRAG and v[kinds.index("tcp")] == abi.V_NOT_UDP
    R = _check(gpu_ctx, bt)
    assert R.reason == [r for _, r in GATES] * 3 + ["gate"] * 10


@pytest.mark.parametrize("flags", [U.ECHO, U.UNREACH, U.ALL])
def test_flags(gpu_ctx, flags):
    buf, nb, off, ln, kinds = U.mixed(21, 600)
    R = _check(gpu_ctx, (buf, nb, off, ln, _meta(buf, nb, off, ln)), flags=flags)
    assert (R.stats["echo_replied"] > 10) == bool(flags & U.ECHO)
    assert (R.stats["unreach_sent"] > 10) == bool(flags & U.UNREACH)


def test_err_limit(gpu_ctx):
    rng = np.random.default_rng(17)
    fl = []
    for j in range(700):                                          # echo replies on both sides of every limit
        fl.append(U.udp_frame(rng, U.CLOSED_PORT) if j % 3 else U.echo_request(rng, 8 + j % 90))
    bt = _batch(fl)
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    elig = sum(1 for j in range(700) if j % 3)
    for lim in (0, 1, 21, 171, elig - 1, elig, elig + 1, U.NO_LIMIT):   # 21: inside the first wave; 171: the second block
        R = _check(gpu_ctx, bt, err_limit=lim, dev=dev)
        assert R.stats["unreach_sent"] == min(lim, elig) and R.stats["limited"] == elig - min(lim, elig)
        assert R.stats["echo_replied"] == 700 - elig
        if 0 < lim < elig:
            last_err = max(int(o) for r, o in enumerate(R.origin) if R.out[int(R.reply_off[r]) + 34] == 3)
            assert any(o > last_err for o in R.origin) and any(o < last_err for o in R.origin)


def test_room(gpu_ctx):
    rng = np.random.default_rng(19)
    fl = [U.udp_frame(rng, U.CLOSED_PORT) if j % 2 else U.echo_request(rng, 8 + (j * 7) % 200) for j in range(600)]
    bt = _batch(fl)
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    full = U.model(*bt)
    ro, need = full.reply_off, full.stats["bytes_needed"]
    assert len(ro) == 601 and need == int(ro[-1])
    for cap in (0, int(ro[1]) - 1, int(ro[1]), int(ro[300]) + 5, int(ro[FPB + 3]), need - 1, need):
        R = _check(gpu_ctx, bt, out_cap=cap, dev=dev, guard=8192)
        assert R.stats["bytes_needed"] == need and R.stats["replies"] == int(np.searchsorted(ro, cap, side="right")) - 1
        assert R.stats["no_room"] == 600 - R.stats["replies"]
    for mr in (0, 1, 300, FPB + 3, 599, 600):
        R = _check(gpu_ctx, bt, max_replies=mr, out_cap=need + 64, dev=dev)
        assert R.stats["replies"] == mr and R.stats["no_room"] == 600 - mr and R.stats["bytes_needed"] == need
    # both at once with a limit: the limit is applied first
    R = _check(gpu_ctx, bt, max_replies=200, out_cap=int(ro[150]) + 1, err_limit=40, dev=dev)
    assert R.stats["limited"] == 260 and R.stats["no_room"] > 0


def test_untrusted_meta(gpu_ctx):
    """meta names candidates whose descriptors are short or out of range: bad_frame, and no byte of
    them is read (the buffers keep their tailroom, so nothing here can fault)."""
    rng = np.random.default_rng(23)
    fl = _filler(rng, 300)
    for p in (5, 70, 290):
        fl[p] = U.echo_request(rng, 64)
    buf, nb, off, ln = U.pack(fl)
    meta = _meta(buf, nb, off, ln)
    off, ln = off.copy(), ln.copy()
    echo_m, unr_m = int(meta[5]), (int(meta[5]) & ~0xF) | abi.V_NO_BIND
    for p, (o, l, m) in {1: (0, 41, echo_m), 2: (0, 0, unr_m), 3: (nb - 10, 60, echo_m), 64: (0xFFFFFFF0, 100, unr_m),
                         65: (nb, 42, echo_m), 255: (nb - 41, 42, unr_m), 256: (0x80000000, 65535, echo_m)}.items():
        off[p], ln[p], meta[p] = o, l, m
    meta[10] = unr_m                 # an open-port datagram called NO_BIND: the stage believes meta
    meta[11] = (unr_m & ~0x60) | (abi.UDP_BAD << 5)
    R = _check(gpu_ctx, (buf, nb, off, ln, meta))
    assert R.stats["bad_frame"] == 7 and R.reason[10] == "unreach" and R.reason[11] == ""
    assert R.stats["echo_replied"] == 3


def test_no_candidates_leaves_the_output_untouched(gpu_ctx):
    rng = np.random.default_rng(29)
    bt = _batch(_filler(rng, 2 * FPB + 17))
    assert np.all((bt[4] & 0xF) == abi.V_DELIVERED)
    R = _check(gpu_ctx, bt, out_cap=4096)
    assert R.stats["replies"] == 0 and R.stats["bytes_needed"] == 0 and list(R.reply_off) == [0]


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_batches(gpu_ctx, seed):
    buf, nb, off, ln, kinds = U.mixed(seed, 2000)
    bt = (buf, nb, off, ln, _meta(buf, nb, off, ln))
    R = _check(gpu_ctx, bt, err_limit=100, mtu=1500 if seed == 1 else 0)
    U.assert_mixed_counts(R)
    assert R.reason.count("limited") >= 20
    R = _check(gpu_ctx, bt, out_cap=R.stats["bytes_needed"] // 2)
    assert R.reason.count("no_room") >= 20


def test_pipes_equal_the_stream_call(gpu_ctx):
    buf, nb, off, ln, kinds = U.mixed(5, 1500)
    bt = (buf, nb, off, ln, _meta(buf, nb, off, ln))
    dev = abi.rx_upload(gpu_ctx, buf, off, ln)
    want = _check(gpu_ctx, bt, err_limit=50, dev=dev)
    for pipe in (1, 2, 3, 1):                                      # back to back; pipe 1 reuses its workspace
        R = _check(gpu_ctx, bt, err_limit=50, dev=dev, pipe=pipe)
        assert R.stats == want.stats
    st = abi.IcmpStats()
    assert abi.lib().udpdk_gpu_pipe_icmp_stats(gpu_ctx.handle, 4, C.byref(st)) == -errno.EINVAL
    assert abi.lib().udpdk_gpu_pipe_icmp_stats(gpu_ctx.handle, 0, C.byref(st)) == -errno.EINVAL


def test_argument_errors_and_empty_batch(gpu_ctx):
    L = abi.lib()
    st = abi.IcmpStats()
    with abi.GpuContext(0, max_frames=1024, max_lanes=1) as fresh:
        assert L.udpdk_gpu_icmp_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
        assert L.udpdk_gpu_pipe_icmp_stats(fresh.handle, 1, C.byref(st)) == -errno.ENOENT
    rng = np.random.default_rng(31)
    buf, nb, off, ln, meta = _batch([U.echo_request(rng, 64)] * 4)
    b = abi.rx_upload(gpu_ctx, buf, off, ln)
    md, ro, og = gpu_ctx.upload(meta), gpu_ctx.upload(np.full(8, 7, np.uint32)), gpu_ctx.alloc(64)
    out = gpu_ctx.alloc(4096)
    cfg = U.tx_config()

    def call(flags=3, mtu=0, out_ptr=out.ptr, cap=4096, fb=nb, n=4, ro_ptr=ro.ptr, meta_ptr=md.ptr):
        bt = abi.RxBatch(b.frames.ptr, fb, b.offset.ptr, b.length.ptr, None, n)
        o = abi.IcmpOut(out_ptr, cap, ro_ptr, og.ptr, 4)
        return L.udpdk_gpu_icmp_reply(gpu_ctx.handle, C.byref(cfg), C.byref(bt), C.c_void_p(meta_ptr), flags, mtu,
                                      U.NO_LIMIT, C.byref(o))
    for kw in (dict(flags=0), dict(flags=4), dict(flags=7), dict(mtu=67), dict(mtu=69), dict(mtu=65536),
               dict(out_ptr=out.ptr + 8), dict(cap=1 << 32), dict(fb=1 << 32), dict(out_ptr=None), dict(ro_ptr=None),
               dict(meta_ptr=None), dict(out_ptr=b.frames.ptr + 16 * ((nb + 15) // 16), cap=64),
               dict(out_ptr=b.frames.ptr, cap=16)):
        assert call(**kw) == -errno.EINVAL, kw
    gpu_ctx.sync()
    assert gpu_ctx.download(ro, np.uint32, 8).tolist() == [7] * 8           # nothing was enqueued
    assert call(n=0) == 0
    assert L.udpdk_gpu_icmp_stats(gpu_ctx.handle, C.byref(st)) == 0 and st.replies == 0 and st.bytes_needed == 0
    assert gpu_ctx.download(ro, np.uint32, 8).tolist() == [0] + [7] * 7
    assert call() == 0 and L.udpdk_gpu_icmp_stats(gpu_ctx.handle, C.byref(st)) == 0 and st.echo_replied == 4
