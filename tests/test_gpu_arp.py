"""udpdk_gpu_arp_reply on the GPU through the C ABI, bit-exact against the model (tests/arp_util.py):
the slots [0, replies), origin, every count, and nothing written at or past `replies`."""
import ctypes as C
import errno

import numpy as np
import pytest

import arp_util as U
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

T, _ = abi.arp_geometry(1)
LISTS = {abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}
PAD = 8


def _rx_meta(ctx, dev):
    """The verdict words udpdk_gpu_rx gives the uploaded batch."""
    ctx.upload_snapshot(abi.snapshot_from_lists(LISTS, 1))
    out = abi.rx_alloc_out(ctx, dev.n, 1, dev.n)
    return abi.rx_run(ctx, dev, out)[0]


def _check(ctx, bt, meta, *, dev=None, pipe=0, max_replies=None, cfg=None):
    """Run the stage and the model with the same arguments; compare everything. Returns the model."""
    buf, nb, off, ln = bt
    n = len(off)
    mr = n if max_replies is None else max_replies
    R = U.model(buf, nb, off, ln, meta, max_replies=mr)
    b = dev if dev is not None else abi.rx_upload(ctx, buf, off, ln)
    g = abi.arp_run(ctx, cfg or U.tx_config(), b, meta, max_replies=mr, pipe=pipe, pad=PAD)
    print("stats", g["stats"], "model", R["stats"])
    assert g["rc"] == 0
    assert g["stats"] == R["stats"]
    assert g["stats_rc"] == (-errno.ENOSPC if R["stats"]["no_room"] else 0)
    k = R["stats"]["replies"]
    bad = np.flatnonzero((g["slots"][:k] != R["slots"]).any(axis=1))
    assert bad.size == 0, (bad[:8], g["slots"][bad[0]].tobytes().hex(), R["slots"][bad[0]].tobytes().hex())
    assert not g["slots"][:k, 42:].any()                           # bytes 42-63 of every written slot
    assert np.all(g["slots"][k:] == 0xA5)                          # the canary at and beyond `replies`
    assert np.array_equal(g["origin"][:k], R["origin"]) and np.all(g["origin"][k:] == 0xA5A5A5A5)
    assert np.array_equal(g["meta"], np.asarray(meta, np.uint32))  # meta is only read
    assert np.array_equal(ctx.download(b.frames, np.uint8, len(buf)), buf)   # and so are the frames
    R["gpu"] = g
    return R


def _filler(rng, n):
    return [U.udp_frame(rng, payload_len=int(rng.integers(0, 40))) for _ in range(n)]


def _every_rule_batch():
    buf, nb, off, ln, kinds = U.mixed(1, 2000)
    assert {int(o) % 16 for o in off} == set(range(16))
    assert {42, 43, 60, 41} <= {int(x) for x in ln}
    return (buf, nb, off, ln), kinds


def test_every_rule_with_meta_from_rx(gpu_ctx):
    bt, kinds = _every_rule_batch()
    buf, nb, off, ln = bt
    want = U.model(buf, nb, off, ln, U.host_meta(buf, off, ln), max_replies=100)
    for k in U.STAT_FIELDS:                                        # no comparison below passes empty
        assert want["stats"][k] > 0, k
    dev = abi.rx_upload(gpu_ctx, buf, off, ln)
    meta = _rx_meta(gpu_ctx, dev)
    assert np.array_equal((meta & 0xF) == U.V_NOT_IPV4, U.host_meta(buf, off, ln) == U.V_NOT_IPV4)
    R = _check(gpu_ctx, bt, meta, dev=dev, max_replies=100)
    assert R["stats"] == want["stats"]
    R = _check(gpu_ctx, bt, meta, dev=dev)
    assert R["stats"]["no_room"] == 0 and R["stats"]["replies"] == want["stats"]["eligible"]
    for i, k in enumerate(kinds):
        assert R["reason"][i] == (None if k == "udp" else U.KINDS[k]), (i, k)


def test_every_rule_with_a_ptype_array(gpu_ctx):
    """The same batch with NIC packet types given: ARP and the other ethertypes carry no IPv4 bit."""
    bt, kinds = _every_rule_batch()
    buf, nb, off, ln = bt
    pt = np.array([0x211 if k == "udp" else 0x1 for k in kinds], np.uint32)
    dev = abi.rx_upload(gpu_ctx, buf, off, ln, pt)
    meta = _rx_meta(gpu_ctx, dev)
    assert np.array_equal((meta & 0xF) == U.V_NOT_IPV4, pt == 0x1)
    R = _check(gpu_ctx, bt, meta, dev=dev)
    assert R["stats"]["eligible"] > 100 and R["stats"]["bad_frame"] > 10


def test_foreign_meta(gpu_ctx):
    """All-NOT_IPV4 meta over a batch whose descriptors are short or out of range: bad_frame, and no
    byte of them is read (the buffers keep their tailroom, so nothing here can fault) or written."""
    rng = np.random.default_rng(23)
    fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) for _ in range(300)]
    buf, nb, off, ln = U.pack(fl)
    off, ln = off.copy(), ln.copy()
    broken = {1: (0, 41), 2: (0, 0), 3: (nb - 10, 60), 64: (0xFFFFFFF0, 100), 65: (nb, 42), 255: (nb - 41, 42),
              256: (0x80000000, 65535), 299: (0xFFFFFFFF, 42)}
    for p, (o, l) in broken.items():
        off[p], ln[p] = o, l
    meta = np.full(300, U.V_NOT_IPV4, np.uint32)
    R = _check(gpu_ctx, (buf, nb, off, ln), meta)
    assert R["stats"]["bad_frame"] == len(broken) and R["stats"]["replies"] == 300 - len(broken)
    # every descriptor out of range: nothing but bad_frame
    off[:], ln[:] = nb - 20, 42
    R = _check(gpu_ctx, (buf, nb, off, ln), meta)
    assert R["stats"] == dict({k: 0 for k in U.STAT_FIELDS}, bad_frame=300)
    # a UDP batch called NOT_IPV4: candidates by meta, counted nowhere
    fl = _filler(rng, 200)
    bt = U.pack(fl)
    R = _check(gpu_ctx, bt, np.full(200, U.V_NOT_IPV4, np.uint32))
    assert R["stats"] == {k: 0 for k in U.STAT_FIELDS}


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1])
def test_sizes_around_the_launch_geometry(gpu_ctx, n):
    """Eligible requests at the first and last frame of every block, and nowhere else."""
    rng = np.random.default_rng(n)
    fl = _filler(rng, n)
    edges = sorted({p for blk in range((n + T - 1) // T) for p in (blk * T, min(n, (blk + 1) * T) - 1)})
    for p in edges:
        fl[p] = U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng), pad_to=int(rng.choice([0, 60])))
    bt = U.pack(fl, aligns=rng.integers(0, 16, n).tolist())
    R = _check(gpu_ctx, bt, U.host_meta(bt[0], bt[2], bt[3]))
    assert list(R["origin"]) == edges and R["stats"]["arp"] == len(edges)


def test_every_frame_eligible(gpu_ctx):
    rng = np.random.default_rng(41)
    n = 2 * T + 1
    fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) for _ in range(n)]
    bt = U.pack(fl)
    R = _check(gpu_ctx, bt, U.host_meta(bt[0], bt[2], bt[3]))
    assert R["stats"]["replies"] == n and list(R["origin"]) == list(range(n))


def test_more_than_256_workgroups(gpu_ctx):
    """Past 256 workgroups the finishing workgroup holds several rows per lane and finds a reply's row
    in two steps. The descriptors alias a few frames (the stage only reads them), so the batch is large
    in frames only: requests at the edges of some blocks, a run of blocks full of them, none elsewhere."""
    rng = np.random.default_rng(53)
    n = 2 * 256 * T + 77
    reqs = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng), pad_to=60 * (j % 2)) for j in range(16)]
    buf, nb, foff, fln = U.pack([U.udp_frame(rng, payload_len=18)] + reqs, aligns=list(range(17)))
    which = np.zeros(n, np.int64)                                  # 0: the UDP frame
    at = {blk * T + e for blk in (0, 1, 2, 3, 255, 256, 257, 300, 510, 511, 512) for e in (0, T - 1) if blk * T + e < n}
    at |= set(range(258 * T - 5, 261 * T + 9)) | {n - 1}
    at = np.array(sorted(at))
    which[at] = 1 + rng.integers(0, 16, len(at))
    off, ln = foff[which], fln[which]
    meta = np.where(which > 0, U.V_NOT_IPV4, abi.V_DELIVERED).astype(np.uint32)
    mr = len(at) + 50
    R = _check(gpu_ctx, (buf, nb, off, ln), meta, max_replies=mr)
    assert R["stats"]["replies"] == len(at) > 3 * T and np.array_equal(R["origin"], at)
    R = _check(gpu_ctx, (buf, nb, off, ln), meta, max_replies=T + 3)
    assert R["stats"]["no_room"] == len(at) - T - 3


def test_room(gpu_ctx):
    rng = np.random.default_rng(19)
    n = T + 300
    fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) if j % 3 else U.udp_frame(rng) for j in range(n)]
    bt = U.pack(fl)
    meta = U.host_meta(bt[0], bt[2], bt[3])
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    elig = sum(1 for j in range(n) if j % 3)
    full = _check(gpu_ctx, bt, meta, dev=dev)
    assert full["stats"]["replies"] == elig
    for mr in (0, 1, 300, elig - 1):
        R = _check(gpu_ctx, bt, meta, dev=dev, max_replies=mr)
        assert R["stats"]["replies"] == mr and R["stats"]["no_room"] == elig - mr and R["stats"]["eligible"] == elig
        assert R["gpu"]["stats_rc"] == -errno.ENOSPC
        assert np.array_equal(R["origin"], full["origin"][:mr])                  # the cut is a tail


def test_no_candidate_leaves_the_output_untouched(gpu_ctx):
    rng = np.random.default_rng(29)
    bt = U.pack(_filler(rng, 2 * T + 17))
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    meta = _rx_meta(gpu_ctx, dev)
    assert np.all((meta & 0xF) == abi.V_DELIVERED)
    R = _check(gpu_ctx, bt, meta, dev=dev)
    assert R["stats"] == {k: 0 for k in U.STAT_FIELDS}


@pytest.mark.parametrize("res", [1, 2, 3])
def test_last_frame_ends_at_frames_bytes(gpu_ctx, res):
    """The batch's last frame is an eligible 42-byte request that ends exactly at frames_bytes with
    frames_bytes % 4 == res; the device buffer has the documented tailroom and no more."""
    rng = np.random.default_rng(res)
    fl = _filler(rng, 70) + [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng))]
    for gap in range(4):
        buf, nb, off, ln = U.pack([bytes(gap)] + fl)
        if nb % 4 == res:
            break
    off, ln = off[1:], ln[1:]
    assert nb % 4 == res and int(off[-1]) + 42 == nb == len(buf)
    R = _check(gpu_ctx, (buf, nb, off, ln), U.host_meta(buf, off, ln))
    assert list(R["origin"]) == [70]


def test_two_runs_give_identical_output(gpu_ctx):
    bt, _ = _every_rule_batch()
    meta = U.host_meta(bt[0], bt[2], bt[3])
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    a = _check(gpu_ctx, bt, meta, dev=dev)["gpu"]
    b = _check(gpu_ctx, bt, meta, dev=dev)["gpu"]
    assert a["stats"] == b["stats"] and np.array_equal(a["slots"], b["slots"]) and np.array_equal(a["origin"], b["origin"])


def test_other_address_and_mac(gpu_ctx):
    """The stage answers for cfg's address with cfg's MAC, whatever they are."""
    rng = np.random.default_rng(5)
    mac, ip = bytes.fromhex("0200deadbeef"), "10.9.8.7"
    fl = [U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng), tpa=ip), U.arp_frame(sha=mac, spa=ip, tpa=ip),
          U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)), U.arp_frame(sha=U.OUR_MAC, spa=U.rand_ip(rng), tpa=ip)]
    buf, nb, off, ln = U.pack(fl, aligns=[1, 6, 11, 15])
    meta = U.host_meta(buf, off, ln)
    R = U.model(buf, nb, off, ln, meta, mac=mac, ip=abi.raw_ip(ip))
    assert R["reason"] == ["eligible", "own", "not_ours", "eligible"]
    g = abi.arp_run(gpu_ctx, U.tx_config(ip, mac), abi.rx_upload(gpu_ctx, buf, off, ln), meta)
    assert g["stats"] == R["stats"] and np.array_equal(g["slots"][:2], R["slots"]) and list(g["origin"][:2]) == [0, 3]


def test_pipes_after_pipe_rx_host():
    """The pipe form on the batch udpdk_gpu_pipe_rx_host staged on that pipe, with its device verdict
    words, at every pipelining depth."""
    L = abi.lib()
    bt, _ = _every_rule_batch()
    buf, nb, off, ln = bt
    n = len(off)
    frames = np.concatenate([buf, np.zeros(abi.FRAMES_TAILROOM, np.uint8)])
    o32, l16 = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(ln, np.uint16)
    for depth in (2, 3, 4):
        with abi.GpuContext(0, max_frames=4096, max_lanes=8) as ctx:
            ctx.pipeline(depth)
            st = abi.ArpStats()
            for pipe in (1, 2, 3):
                assert L.udpdk_gpu_pipe_arp_stats(ctx.handle, pipe, C.byref(st)) == -errno.ENOENT
            assert L.udpdk_gpu_pipe_arp_stats(ctx.handle, 4, C.byref(st)) == -errno.EINVAL
            assert L.udpdk_gpu_pipe_arp_stats(ctx.handle, 0, C.byref(st)) == -errno.EINVAL
            ctx.upload_snapshot(abi.snapshot_from_lists(LISTS, 1))
            for pipe, mr in ((1, n), (2, 50), (3, n), (1, 7)):          # pipe 1 reuses its workspace
                meta, loff, lpkt = np.zeros(n, np.uint32), np.zeros(2, np.uint32), np.zeros(n, np.uint32)
                rst = abi.RxStats()
                assert L.udpdk_gpu_pipe_rx_host(ctx.handle, pipe, abi._ptr(frames), nb, abi._ptr(o32), 0, abi._ptr(l16),
                                                None, n, abi._ptr(meta), abi._ptr(loff), abi._ptr(lpkt), n,
                                                C.byref(rst)) == 0
                assert L.udpdk_gpu_pipe_wait(ctx.handle, pipe) == 0
                staged, meta_dev = abi.RxBatch(), C.c_void_p()
                assert L.udpdk_gpu_pipe_batch(ctx.handle, pipe, C.byref(staged), C.byref(meta_dev)) == 0
                R = U.model(buf, nb, off, ln, meta, max_replies=mr)
                assert R["stats"]["eligible"] > 100
                slots = ctx.upload(np.full(64 * (mr + PAD), 0xA5, np.uint8))
                org = ctx.upload(np.full(4 * (mr + PAD), 0xA5, np.uint8))
                o = abi.ArpOut(slots.ptr, org.ptr, mr)
                cfg = U.tx_config()
                assert L.udpdk_gpu_pipe_arp_reply(ctx.handle, pipe, C.byref(cfg), C.byref(staged), meta_dev, C.byref(o)) == 0
                assert L.udpdk_gpu_pipe_wait(ctx.handle, pipe) == 0
                src = L.udpdk_gpu_pipe_arp_stats(ctx.handle, pipe, C.byref(st))
                assert src == (-errno.ENOSPC if R["stats"]["no_room"] else 0)
                assert {k: getattr(st, k) for k in U.STAT_FIELDS} == R["stats"]
                k = R["stats"]["replies"]
                gs = ctx.download(slots, np.uint8, 64 * (mr + PAD)).reshape(-1, 64)
                go = ctx.download(org, np.uint32, mr + PAD)
                assert np.array_equal(gs[:k], R["slots"]) and np.all(gs[k:] == 0xA5)
                assert np.array_equal(go[:k], R["origin"]) and np.all(go[k:] == 0xA5A5A5A5)
                slots.free()
                org.free()


def test_argument_errors_and_empty_batch(gpu_ctx):
    L = abi.lib()
    st = abi.ArpStats()
    with abi.GpuContext(0, max_frames=1024, max_lanes=1) as fresh:
        assert L.udpdk_gpu_arp_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
        assert L.udpdk_gpu_pipe_arp_stats(fresh.handle, 1, C.byref(st)) == -errno.ENOENT
    rng = np.random.default_rng(31)
    buf, nb, off, ln = U.pack([U.arp_frame(sha=U.rand_mac(rng), spa=U.rand_ip(rng)) for _ in range(4)])
    meta = U.host_meta(buf, off, ln)
    b = abi.rx_upload(gpu_ctx, buf, off, ln)
    md, og = gpu_ctx.upload(meta), gpu_ctx.upload(np.full(8, 7, np.uint32))
    out = gpu_ctx.upload(np.full(4 * 64 + 64, 0x77, np.uint8))
    cfg, cfg0 = U.tx_config(), U.tx_config("0.0.0.0")

    def call(out_ptr=out.ptr, fb=nb, n=4, og_ptr=og.ptr, meta_ptr=md.ptr, c=cfg, mr=4, ctx=gpu_ctx.handle, bt=True, o=True):
        btv = abi.RxBatch(b.frames.ptr, fb, b.offset.ptr, b.length.ptr, None, n)
        ov = abi.ArpOut(out_ptr, og_ptr, mr)
        return L.udpdk_gpu_arp_reply(ctx, C.byref(c) if c is not None else None, C.byref(btv) if bt else None,
                                     C.c_void_p(meta_ptr), C.byref(ov) if o else None)
    for kw in (dict(out_ptr=None), dict(og_ptr=None), dict(meta_ptr=None), dict(c=None), dict(ctx=None), dict(bt=False),
               dict(o=False), dict(c=cfg0), dict(fb=1 << 32), dict(out_ptr=out.ptr + 8),
               dict(out_ptr=b.frames.ptr + 16 * ((nb + 15) // 16)),       # inside the tailroom
               dict(out_ptr=b.frames.ptr), dict(og_ptr=b.frames.ptr + 4),
               dict(out_ptr=b.frames.ptr - 64 * 4 + 16, mr=4)):            # its last slot reaches into the frames
        assert call(**kw) == -errno.EINVAL, kw
    gpu_ctx.sync()
    assert gpu_ctx.download(og, np.uint32, 8).tolist() == [7] * 8             # nothing was enqueued
    assert np.all(gpu_ctx.download(out, np.uint8, 4 * 64 + 64) == 0x77)
    assert call(n=0) == 0
    assert L.udpdk_gpu_arp_stats(gpu_ctx.handle, C.byref(st)) == 0
    assert all(getattr(st, k) == 0 for k in U.STAT_FIELDS)
    assert gpu_ctx.download(og, np.uint32, 8).tolist() == [7] * 8
    assert call() == 0 and L.udpdk_gpu_arp_stats(gpu_ctx.handle, C.byref(st)) == 0 and st.replies == 4
    assert gpu_ctx.download(og, np.uint32, 8).tolist() == [0, 1, 2, 3] + [7] * 4
