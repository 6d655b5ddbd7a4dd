"""udpdk_gpu_neigh_learn on the GPU through the C ABI against the model (tests/neigh_util.py): the table as a
map and every count. The table's layout is never looked at, except where a call must leave it bit-identical."""
import ctypes as C
import errno

import numpy as np
import pytest

import arp_util as A
import neigh_util as U
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

T, _ = abi.neigh_geometry()
LISTS = {abi.raw_port(F.PORT_RECV): [(0, 0, 0)]}
US = U.OUR_IP


def _setup(ctx, entries, init=()):
    """A fresh table on the device and its model, with the same (REACHABLE / STATIC) entries."""
    assert abi.neigh_create(ctx, entries) == 0
    tab = U.Table(entries, init)
    assert abi.neigh_set(ctx, tab.tuples()) == 0
    assert abi.neigh_dump(ctx) == tab.as_map()
    return tab


def _check(ctx, tab, bt, meta, now, *, cfg=None, dev=None, pipe=0, exact=True):
    """Run the stage and the model with the same arguments; compare the counts and (exact) the table."""
    buf, nb, off, ln = bt
    cfg = cfg or U.cfg()
    R = U.learn(tab, cfg, buf, nb, off, ln, meta, now)
    b = dev if dev is not None else abi.rx_upload(ctx, buf, off, ln)
    g = abi.neigh_learn_run(ctx, cfg, b, meta, now, pipe=pipe)
    print("stats", g["stats"], "model", R["stats"])
    assert g["rc"] == 0 and g["stats_rc"] == 0
    assert g["stats"] == R["stats"]
    if exact:
        assert abi.neigh_dump(ctx) == tab.as_map()
    assert np.array_equal(g["meta"], np.asarray(meta, np.uint32))  # meta is only read
    assert np.array_equal(ctx.download(b.frames, np.uint8, len(buf)), buf)   # and so are the frames
    return R


def _filler(rng, n):
    return [A.udp_frame(rng, payload_len=int(rng.integers(0, 40))) for _ in range(n)]


def _ip(k):
    return "10.%d.%d.%d" % (1 + (k >> 16), k >> 8 & 255, k & 255)


def _request(rng, k, **kw):
    """A request for our address from host k (a creating event)."""
    return A.arp_frame(sha=A.rand_mac(rng), spa=_ip(k), tpa=US, pad_to=int(rng.choice([0, 60])), **kw)


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T + 3])
def test_sizes_around_the_launch_geometry(gpu_ctx, n):
    """ARP frames at every one of the 16 byte alignments among UDP filler, at the first and last frame of every
    workgroup and at 40 other places: new hosts asking for us, then (a second call) the same hosts with new MACs
    in replies and 9 hosts nobody knows."""
    rng = np.random.default_rng(n)
    tab = _setup(gpu_ctx, 1024)
    at = {p for blk in range((n + T - 1) // T) for p in (blk * T, min(n, (blk + 1) * T) - 1)}
    at |= {int(x) for x in rng.integers(0, n, 40)}
    at = sorted(at)
    fl = _filler(rng, n)
    for j, p in enumerate(at):
        fl[p] = _request(rng, j)
    al = rng.integers(0, 16, n)
    al[at] = [j % 16 for j in range(len(at))]
    bt = A.pack(fl, aligns=al.tolist())
    assert len(at) < 16 or {int(o) % 16 for o in bt[2][at]} == set(range(16))
    R = _check(gpu_ctx, tab, bt, A.host_meta(bt[0], bt[2], bt[3]), 1000)
    assert R["stats"]["created"] == R["stats"]["arp"] == len(at) and len(tab.d) == len(at)
    for j, p in enumerate(at):
        fl[p] = A.arp_frame(op=2, sha=A.rand_mac(rng), spa=_ip(j if j % 5 else 100000 + j), tpa=US, tha=U.OUR_MAC)
    bt = A.pack(fl, aligns=al.tolist())
    R = _check(gpu_ctx, tab, bt, A.host_meta(bt[0], bt[2], bt[3]), 2000)
    assert R["stats"]["updated"] + R["stats"]["ignored"] == len(at) and R["stats"]["ignored"] == (len(at) + 4) // 5


def test_same_sender_in_the_first_and_the_last_workgroup(gpu_ctx):
    """One address with four MACs over three workgroups: the last frame's MAC stays, and each frame counts against
    the one before it. A second address is first heard of in a reply (ignored), then asks (created)."""
    rng = np.random.default_rng(3)
    n = 2 * T + 3
    tab = _setup(gpu_ctx, 64)
    fl = _filler(rng, n)
    m = [bytes.fromhex("02ee0000000%d" % k) for k in range(4)]
    fl[0] = A.arp_frame(sha=m[0], spa="10.5.5.5", tpa=US)                    # created
    fl[1] = A.arp_frame(sha=m[0], spa="10.5.5.5", tpa="10.5.5.9")            # refreshed
    fl[T - 1] = A.arp_frame(op=2, sha=m[1], spa="10.5.5.5", tpa=US)          # updated
    fl[T] = A.arp_frame(op=2, sha=m[1], spa="10.5.5.5", tpa=US)              # refreshed
    fl[2 * T + 1] = A.arp_frame(sha=m[2], spa="10.5.5.5", tpa="10.5.5.5")    # updated (gratuitous)
    fl[2 * T + 2] = A.arp_frame(sha=m[3], spa="10.5.5.5", tpa=US)            # updated: the last wins
    fl[7] = A.arp_frame(op=2, sha=m[0], spa="10.6.6.6", tpa=US)              # ignored
    fl[2 * T] = A.arp_frame(sha=m[1], spa="10.6.6.6", tpa=US)                # created
    bt = A.pack(fl)
    R = _check(gpu_ctx, tab, bt, A.host_meta(bt[0], bt[2], bt[3]), 77)
    assert R["stats"] == dict({k: 0 for k in U.LEARN_FIELDS}, arp=8, created=2, refreshed=2, updated=3, ignored=1)
    assert tab.as_map() == {U.raw("10.5.5.5"): (m[3], U.REACHABLE, 77), U.raw("10.6.6.6"): (m[1], U.REACHABLE, 77)}


def test_more_than_256_workgroups(gpu_ctx):
    """Past 256 workgroups the finishing workgroup holds several rows per lane, and an event's workgroup is found
    by bisection across the lanes' runs. The descriptors alias a few frames (the stage only reads them), so the
    batch is large in frames only: a new host asking for us at the first and last frame of some blocks and at the
    last frame, UDP elsewhere. One address asks from block 0 and again, with another MAC, from block 512."""
    rng = np.random.default_rng(59)
    n = 2 * 256 * T + 77
    at = sorted({p for blk in (0, 1, 255, 256, 257, 300, 510, 511, 512) for p in (blk * T, min(n, (blk + 1) * T) - 1)}
                | {n - 1})
    assert len(at) == 18 and at[-1] == n - 1 and at[-2] == 512 * T
    reqs = [_request(rng, j) for j in range(len(at))]
    m0, m1 = bytes.fromhex("02ee00000001"), bytes.fromhex("02ee00000002")
    reqs[0] = A.arp_frame(sha=m0, spa=_ip(0), tpa=US)
    reqs[at.index(512 * T)] = A.arp_frame(sha=m1, spa=_ip(0), tpa=US)                   # host 0 again, a new MAC
    buf, nb, foff, fln = A.pack([A.udp_frame(rng, payload_len=18)] + reqs, aligns=[j % 16 for j in range(1 + len(at))])
    which = np.zeros(n, np.int64)                                  # 0: the UDP frame
    which[at] = 1 + np.arange(len(at))
    off, ln = foff[which], fln[which]
    meta = np.where(which > 0, A.V_NOT_IPV4, abi.V_DELIVERED).astype(np.uint32)
    tab = _setup(gpu_ctx, 64)
    R = _check(gpu_ctx, tab, (buf, nb, off, ln), meta, 4000)
    assert R["stats"] == dict({k: 0 for k in U.LEARN_FIELDS}, arp=len(at), created=len(at) - 1, updated=1)
    assert tab.as_map()[U.raw(_ip(0))] == (m1, U.REACHABLE, 4000)


def _every_class_batch(rng, n=1500):
    """Every learn class and every ARP kind of arp_util among UDP filler, frame k at offset == 5 k mod 16."""
    known = [_ip(200 + k) for k in range(8)]                       # REACHABLE in the table
    stat = [_ip(300 + k) for k in range(3)]                        # STATIC
    asked = [_ip(400 + k) for k in range(4)]                       # INCOMPLETE (resolve asked for them)
    macs = {ip: A.rand_mac(rng) for ip in known + stat}
    fl = []
    for k in range(n):
        r = int(rng.integers(0, 12))
        if r == 0:
            fl.append(_request(rng, int(rng.integers(0, 60))))                                   # created, then updated
        elif r == 1:
            ip = known[int(rng.integers(0, 8))]
            fl.append(A.arp_frame(op=int(rng.integers(1, 3)), sha=macs[ip], spa=ip, tpa=_ip(9)))   # refreshed (or updated)
        elif r == 2:
            ip = known[int(rng.integers(0, 8))]
            fl.append(A.arp_frame(op=2, sha=A.rand_mac(rng), spa=ip, tpa=US, pad_to=60))         # updated
        elif r == 3:
            fl.append(A.arp_frame(op=2, sha=A.rand_mac(rng), spa=stat[int(rng.integers(0, 3))], tpa=US))   # static_kept
        elif r == 4:
            fl.append(A.arp_frame(op=2, sha=A.rand_mac(rng), spa=asked[int(rng.integers(0, 4))], tpa=US))  # a solicited reply
        elif r == 5:
            ip = _ip(5000 + int(rng.integers(0, 50)))
            fl.append(A.arp_frame(op=int(rng.integers(1, 3)), sha=A.rand_mac(rng), spa=ip, tpa=ip))        # ignored
        elif r == 6:
            spa = ["0.0.0.0", US, "255.255.255.255", "224.0.0.9", "239.1.2.3"][int(rng.integers(0, 5))]
            fl.append(A.arp_frame(sha=A.rand_mac(rng), spa=spa, tpa=US))                         # sender_bad
        elif r == 7:
            fl.append(A.kind_frame(rng, ["own", "sha_mcast", "sha_zero", "op_rarp", "op_zero", "op_256", "htype_bad",
                                         "plen_bad", "short_41", "ipv6", "lldp"][int(rng.integers(0, 11))]))
        else:
            fl.append(A.udp_frame(rng, payload_len=int(rng.integers(0, 60))))
    bt = A.pack(fl, aligns=[(5 * k) % 16 for k in range(n)])
    init = [(ip, macs[ip], U.REACHABLE, 10) for ip in known] + [(ip, macs[ip], U.STATIC, 0) for ip in stat]
    return bt, init, asked


def _setup_every_class(ctx, init, asked):
    tab = _setup(ctx, 256, init)
    c = U.cfg()
    dst = [U.raw(ip) for ip in asked]
    U.resolve(tab, c, dst, [0] * len(dst), 50)
    g = abi.neigh_resolve_run(ctx, c, dst, [0] * len(dst), 50)
    assert g["rc"] == 0 and g["stats"]["inserted"] == len(asked)
    assert abi.neigh_dump(ctx) == tab.as_map()
    return tab


def test_every_class_with_meta_from_rx(gpu_ctx):
    bt, init, asked = _every_class_batch(np.random.default_rng(11))
    buf, nb, off, ln = bt
    want = U.learn(_model_only(init, asked), U.cfg(), buf, nb, off, ln, A.host_meta(buf, off, ln), 900)
    for k in set(U.LEARN_FIELDS) - {"full"}:                       # no comparison below passes empty
        assert want["stats"][k] > 0, k
    tab = _setup_every_class(gpu_ctx, init, asked)
    dev = abi.rx_upload(gpu_ctx, buf, off, ln)
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists(LISTS, 1))
    meta = abi.rx_run(gpu_ctx, dev, abi.rx_alloc_out(gpu_ctx, dev.n, 1, dev.n))[0]
    assert np.array_equal((meta & 0xF) == A.V_NOT_IPV4, A.host_meta(buf, off, ln) == A.V_NOT_IPV4)
    R = _check(gpu_ctx, tab, bt, meta, 900, dev=dev)
    assert R["stats"] == want["stats"]
    assert all(tab.d[U.raw(ip)][1] == U.REACHABLE for ip in asked)  # every solicited reply found its entry
    # the same batch again: nothing is created, every sender is known or still not asked for
    R = _check(gpu_ctx, tab, bt, meta, 901, dev=dev)
    assert R["stats"]["created"] == 0 and R["stats"]["ignored"] == want["stats"]["ignored"]


def _model_only(init, asked):
    tab = U.Table(256, init)
    U.resolve(tab, U.cfg(), [U.raw(ip) for ip in asked], [0] * len(asked), 50)
    return tab


def test_foreign_meta(gpu_ctx):
    """All-NOT_IPV4 meta over a batch whose descriptors are short or out of range: bad_frame, and no byte of them
    is read (the buffers keep their tailroom, so nothing here can fault) or written."""
    rng = np.random.default_rng(23)
    tab = _setup(gpu_ctx, 1024)
    fl = [_request(rng, k) for k in range(300)]
    buf, nb, off, ln = A.pack(fl)
    off, ln = off.copy(), ln.copy()
    broken = {1: (0, 41), 2: (0, 0), 3: (nb - 10, 60), 64: (0xFFFFFFF0, 100), 65: (nb, 42), 255: (nb - 41, 42),
              256: (0x80000000, 65535), 299: (0xFFFFFFFF, 42)}
    for p, (o, l) in broken.items():
        off[p], ln[p] = o, l
    meta = np.full(300, A.V_NOT_IPV4, np.uint32)
    R = _check(gpu_ctx, tab, (buf, nb, off, ln), meta, 5)
    assert R["stats"]["bad_frame"] == len(broken) and R["stats"]["created"] == 300 - len(broken)
    off[:], ln[:] = nb - 20, 42                                    # every descriptor out of range
    before = abi.neigh_dump(gpu_ctx, as_list=True)
    R = _check(gpu_ctx, tab, (buf, nb, off, ln), meta, 6)
    assert R["stats"] == dict({k: 0 for k in U.LEARN_FIELDS}, bad_frame=300)
    assert abi.neigh_dump(gpu_ctx, as_list=True) == before
    bt = A.pack(_filler(rng, 200))                                 # a UDP batch called NOT_IPV4: counted nowhere
    R = _check(gpu_ctx, tab, bt, np.full(200, A.V_NOT_IPV4, np.uint32), 7)
    assert R["stats"] == {k: 0 for k in U.LEARN_FIELDS}


def test_a_table_of_eight(gpu_ctx):
    rng = np.random.default_rng(31)
    # keys that collide and wrap past the end: five whose home is the last slot, one whose home is slot 1
    ips = U.colliding_ips(8, 7, 5) + U.colliding_ips(8, 1, 1)
    tab = _setup(gpu_ctx, 8)
    fl = [A.arp_frame(sha=A.rand_mac(rng), spa=ip, tpa=US) for ip in ips]
    bt = A.pack(fl, aligns=[3, 9, 14, 0, 7, 11])
    R = _check(gpu_ctx, tab, bt, A.host_meta(bt[0], bt[2], bt[3]), 100)
    assert R["stats"]["created"] == 6
    # the same hosts answer with new MACs, found again through the same wrapped probes
    fl = [A.arp_frame(op=2, sha=A.rand_mac(rng), spa=ip, tpa=US) for ip in reversed(ips)]
    bt = A.pack(fl)
    R = _check(gpu_ctx, tab, bt, A.host_meta(bt[0], bt[2], bt[3]), 200)
    assert R["stats"]["updated"] == 6
    # 12 distinct new senders into 5 free slots (3 entries are there, one of them static)
    init = [(ips[0], A.rand_mac(rng), U.REACHABLE, 1), (ips[1], A.rand_mac(rng), U.STATIC, 2), (ips[5], A.rand_mac(rng), U.REACHABLE, 3)]
    tab = _setup(gpu_ctx, 8, init)
    new = [_ip(700 + k) for k in range(12)]
    sha = {ip: A.rand_mac(rng) for ip in new}
    fl = _filler(rng, T + 40)
    for k, ip in enumerate(new):
        fl[[0, 5, 63, 64, 65, 255, 256, 600, T - 1, T, T + 1, T + 39][k]] = A.arp_frame(sha=sha[ip], spa=ip, tpa=US)
    bt = A.pack(fl)
    meta = A.host_meta(bt[0], bt[2], bt[3])
    model = U.Table(8, init)
    R = _check(gpu_ctx, model, bt, meta, 300, exact=False)         # which keys got in is unspecified
    assert R["stats"]["created"] == 5 and R["stats"]["full"] == 7
    got = abi.neigh_dump(gpu_ctx)
    assert len(got) == 8 and all(got[U.raw(ip)] == (mac, st, ts) for ip, mac, st, ts in init)
    inside = [ip for ip in new if U.raw(ip) in got]
    assert len(inside) == 5 and all(got[U.raw(ip)] == (sha[ip], U.REACHABLE, 300) for ip in inside)
    # a second identical call: all refreshed or full again
    tab = U.Table(8, init + [(ip, sha[ip], U.REACHABLE, 300) for ip in inside])
    R = _check(gpu_ctx, tab, bt, meta, 400)
    assert R["stats"] == dict({k: 0 for k in U.LEARN_FIELDS}, arp=12, refreshed=5, full=7)


def test_no_candidate_leaves_the_table_bit_identical(gpu_ctx):
    rng = np.random.default_rng(29)
    init = [(_ip(k), A.rand_mac(rng), U.REACHABLE if k % 3 else U.STATIC, 1000 + k) for k in range(40)]
    tab = _setup(gpu_ctx, 64, init)
    before = abi.neigh_dump(gpu_ctx, as_list=True)
    bt = A.pack(_filler(rng, 2 * T + 17))
    dev = abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3])
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists(LISTS, 1))
    meta = abi.rx_run(gpu_ctx, dev, abi.rx_alloc_out(gpu_ctx, dev.n, 1, dev.n))[0]
    assert np.all((meta & 0xF) == abi.V_DELIVERED)
    R = _check(gpu_ctx, tab, bt, meta, 5000, dev=dev)
    assert R["stats"] == {k: 0 for k in U.LEARN_FIELDS}
    assert abi.neigh_dump(gpu_ctx, as_list=True) == before


def test_pipe_form_equals_the_stream_form():
    bt, init, asked = _every_class_batch(np.random.default_rng(13), 1100)
    meta = A.host_meta(bt[0], bt[2], bt[3])
    L = abi.lib()
    with abi.GpuContext(0, max_frames=4096, max_lanes=8) as ctx:
        ctx.pipeline(2)
        st = abi.NeighLearnStats()
        assert L.udpdk_gpu_pipe_neigh_learn_stats(ctx.handle, 1, C.byref(st)) == -errno.ENOENT
        assert L.udpdk_gpu_pipe_neigh_learn_stats(ctx.handle, 0, C.byref(st)) == -errno.EINVAL
        assert L.udpdk_gpu_pipe_neigh_learn_stats(ctx.handle, 4, C.byref(st)) == -errno.EINVAL
        assert L.udpdk_gpu_neigh_learn_stats(ctx.handle, C.byref(st)) == -errno.ENOENT
        dev = abi.rx_upload(ctx, bt[0], bt[2], bt[3])
        out = {}
        for pipe in (0, 1):
            tab = _setup_every_class(ctx, init, asked)
            out[pipe] = _check(ctx, tab, bt, meta, 900, dev=dev, pipe=pipe)["stats"], abi.neigh_dump(ctx)
        assert out[0] == out[1] and out[0][0]["updated"] > 0 and out[0][0]["created"] > 0


def test_argument_errors_and_empty_batch(gpu_ctx):
    L = abi.lib()
    rng = np.random.default_rng(37)
    buf, nb, off, ln = A.pack([_request(rng, k) for k in range(4)])
    b = abi.rx_upload(gpu_ctx, buf, off, ln)
    md = gpu_ctx.upload(A.host_meta(buf, off, ln))
    for bad in (0, 4, 7, 12, 1000, 1 << 17):
        assert abi.neigh_create(gpu_ctx, bad) == -errno.EINVAL
    with abi.GpuContext(0, max_frames=1024, max_lanes=1) as fresh:                # no table
        bt = abi.RxBatch(b.frames.ptr, nb, b.offset.ptr, b.length.ptr, None, 4)
        c = U.cfg()
        assert L.udpdk_gpu_neigh_learn(fresh.handle, C.byref(c), C.byref(bt), C.c_void_p(md.ptr), 1) == -errno.EINVAL
        assert abi.neigh_set(fresh, []) == -errno.EINVAL and abi.neigh_flush(fresh) == -errno.EINVAL
    tab = _setup(gpu_ctx, 8)

    def call(c=U.cfg(), fb=nb, n=4, meta_ptr=md.ptr, bt=True):
        btv = abi.RxBatch(b.frames.ptr, fb, b.offset.ptr, b.length.ptr, None, n)
        return L.udpdk_gpu_neigh_learn(gpu_ctx.handle, C.byref(c) if c is not None else None, C.byref(btv) if bt else None,
                                       C.c_void_p(meta_ptr), 9)
    for kw in (dict(c=None), dict(bt=False), dict(meta_ptr=None), dict(c=U.cfg(src_ip="0.0.0.0")), dict(c=U.cfg(flags=2)),
               dict(c=U.cfg(flags=0x80000001)), dict(fb=1 << 32)):
        assert call(**kw) == -errno.EINVAL, kw
    assert abi.neigh_dump(gpu_ctx) == {}                                          # nothing was enqueued
    st = abi.NeighLearnStats()
    assert call(n=0) == 0 and L.udpdk_gpu_neigh_learn_stats(gpu_ctx.handle, C.byref(st)) == 0
    assert all(getattr(st, k) == 0 for k in U.LEARN_FIELDS) and abi.neigh_dump(gpu_ctx) == {}
    assert call() == 0 and L.udpdk_gpu_neigh_learn_stats(gpu_ctx.handle, C.byref(st)) == 0 and st.created == 4
    # set / dump / flush
    assert abi.neigh_set(gpu_ctx, [(U.raw("10.0.0.1"), bytes(6), U.INCOMPLETE, 0)]) == -errno.EINVAL
    assert abi.neigh_set(gpu_ctx, [(0, bytes(6), U.STATIC, 0)]) == -errno.EINVAL
    more = [(U.raw(_ip(900 + k)), A.rand_mac(rng), U.STATIC if k < 2 else U.REACHABLE, k) for k in range(5)]
    assert abi.neigh_set(gpu_ctx, more) == -errno.ENOSPC                          # four fit beside the four learned
    got = abi.neigh_dump(gpu_ctx)
    assert len(got) == 8 and all(got[ip] == (mac, s, ts) for ip, mac, s, ts in more[:4])
    arr = (abi.NeighEntry * 3)()
    cnt = C.c_uint32()
    assert L.udpdk_gpu_neigh_dump(gpu_ctx.handle, arr, 3, C.byref(cnt)) == -errno.ENOSPC and cnt.value == 8
    assert abi.neigh_set(gpu_ctx, [(more[0][0], more[4][1], U.REACHABLE, 99)]) == 0   # overwriting needs no room
    assert abi.neigh_dump(gpu_ctx)[more[0][0]] == (more[4][1], U.REACHABLE, 99)
    assert abi.neigh_flush(gpu_ctx, keep_static=True) == 0
    assert abi.neigh_dump(gpu_ctx) == {more[1][0]: (more[1][1], U.STATIC, 1)}
    assert abi.neigh_flush(gpu_ctx) == 0 and abi.neigh_dump(gpu_ctx) == {}
