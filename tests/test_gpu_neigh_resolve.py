"""udpdk_gpu_neigh_resolve on the GPU through the C ABI against the model (tests/neigh_util.py): dmac, sockfd_out,
states, the request slots [0, k) and their origins, every count and the table afterwards; canaries at and past
every count; dst_ip and sockfd only read."""
import ctypes as C
import errno

import numpy as np
import pytest

import arp_util as A
import neigh_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

_, B = abi.neigh_geometry()
PAD = 4
MASK, GW = "255.255.255.0", "172.31.100.254"


def _setup(ctx, entries, init=()):
    assert abi.neigh_create(ctx, entries) == 0
    tab = U.Table(entries, init)
    assert abi.neigh_set(ctx, tab.tuples()) == 0
    return tab


def _check(ctx, tab, cfg, dst, sock, now, req_cap=None, exact=True):
    """Run the stage and the model with the same arguments; compare everything. Returns the model's result."""
    dst = np.array([U.raw(d) for d in dst], np.uint32)
    sock = np.array(sock, np.int32)
    n = len(dst)
    R = U.resolve(tab, cfg, dst, sock, now, req_cap)
    g = abi.neigh_resolve_run(ctx, cfg, dst, sock, now & U.U32, req_cap=req_cap, pad=PAD)
    print("stats", g["stats"], "model", R["stats"])
    assert g["rc"] == 0
    assert g["stats"] == R["stats"]
    assert g["stats_rc"] == (-errno.ENOSPC if R["stats"]["no_room"] else 0)
    assert np.array_equal(g["state"][:n], R["state"]) and np.all(g["state"][n:] == 0xA5)
    assert np.array_equal(g["dmac"][:n], R["dmac"]) and np.all(g["dmac"][n:] == 0xA5A5A5A5)
    assert np.array_equal(g["sockfd_out"][:n], R["sockfd_out"]) and np.all(g["sockfd_out"][n:] == np.int32(-0x5A5A5A5B))
    k = R["stats"]["requests"]
    assert np.array_equal(g["req"][:k], R["req"]) and np.all(g["req"][k:] == 0xA5)
    assert np.array_equal(g["req_origin"][:k], R["req_origin"]) and np.all(g["req_origin"][k:] == 0xA5A5A5A5)
    assert np.array_equal(g["dst_ip"], dst) and np.array_equal(g["sockfd"], sock)          # only read
    if exact:
        assert abi.neigh_dump(ctx) == tab.as_map()
    R["gpu"] = g
    return R


def _every_class(rng, n, now=100000):
    """n datagrams of every class R1-R5 in random order, and the table they meet."""
    fresh = [f"172.31.100.{10 + k}" for k in range(6)]
    old = [f"172.31.100.{30 + k}" for k in range(4)]                # REACHABLE, older than the ttl
    stat = [f"172.31.100.{50 + k}" for k in range(2)]
    new = [f"172.31.100.{70 + k}" for k in range(5)]
    init = [(ip, A.rand_mac(rng), U.REACHABLE, now - int(rng.integers(0, 30001))) for ip in fresh]
    init += [(ip, A.rand_mac(rng), U.REACHABLE, now - 30001 - int(rng.integers(0, 1000))) for ip in old]
    init += [(ip, A.rand_mac(rng), U.STATIC, 0) for ip in stat]
    init += [(GW, A.rand_mac(rng), U.REACHABLE, now)]
    pools = [fresh, old, stat, new, ["255.255.255.255", "172.31.100.255"], ["224.0.0.1", "239.255.255.255", "232.9.8.7"],
             ["8.8.8.8", "172.31.101.1", "240.0.0.1"], [U.OUR_IP]]
    dst = [pools[k][int(rng.integers(0, len(pools[k])))] for k in rng.integers(0, len(pools), n)]
    sock = np.where(rng.random(n) < 0.1, -1 - rng.integers(0, 3, n), rng.integers(0, 64, n))
    return init, dst, sock


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2 * B + 1])
def test_sizes_with_every_class(gpu_ctx, n):
    rng = np.random.default_rng(n)
    init, dst, sock = _every_class(rng, n)
    if n == 1:
        dst, sock = ["172.31.100.70"], [5]
    tab = _setup(gpu_ctx, 64, init)
    c = U.cfg(netmask=MASK, gateway=GW)
    R = _check(gpu_ctx, tab, c, dst, sock, 100000)
    if n >= 2 * B:
        for k in ("skipped", "bcast", "mcast", "self", "hit", "expired", "incomplete", "inserted", "unresolved", "requests"):
            assert R["stats"][k] > 0, k                            # no comparison above passes empty
    # without a gateway the off-link ones have no route; with fallback every miss keeps its socket
    tab = _setup(gpu_ctx, 64, init)
    c = U.cfg(netmask=MASK, gateway=0, flags=abi.NEIGH_FALLBACK)
    R = _check(gpu_ctx, tab, c, dst, sock, 100000)
    if n >= 2 * B:
        assert R["stats"]["no_route"] > 0 and R["stats"]["fallback"] > 0 and R["stats"]["unresolved"] == 0


def test_requests_in_first_index_order_and_retransmission(gpu_ctx):
    """200 datagrams to 3 unknown next hops spread over both workgroups: 3 requests, in first-index order; none
    one millisecond before retrans_ms has passed, 3 again when it has."""
    assert B < 200
    rng = np.random.default_rng(5)
    hops = ["172.31.100.93", "172.31.100.91", "172.31.100.92"]
    dst = [hops[0]] * 40 + [hops[1]] + [hops[int(rng.integers(0, 2))] for _ in range(41, B + 3)]
    dst += [hops[2]] + [hops[int(rng.integers(0, 3))] for _ in range(B + 4, 200)]   # .92 is first seen in the second workgroup
    assert len(dst) == 200
    tab = _setup(gpu_ctx, 1024)
    c = U.cfg(retrans_ms=1000)
    R = _check(gpu_ctx, tab, c, dst, [1] * 200, 7000)
    assert R["req_hops"] == [U.raw(h) for h in hops] and R["req_origin"].tolist() == [0, 40, B + 3]
    assert R["stats"]["inserted"] == 3 and R["stats"]["incomplete"] == 197
    R = _check(gpu_ctx, tab, c, dst, [1] * 200, 7999)
    assert R["stats"]["requests"] == 0 and R["stats"]["incomplete"] == 200
    assert all(v[2] == 7000 for v in tab.d.values())
    R = _check(gpu_ctx, tab, c, dst, [1] * 200, 8000)
    assert R["stats"]["requests"] == 3 and R["req_origin"][2] == B + 3
    assert all(v[2] == 8000 for v in tab.d.values())
    # req_cap = 2: the third is cut, and its stamp moves all the same
    R = _check(gpu_ctx, tab, c, dst, [1] * 200, 9000, req_cap=2)
    assert R["stats"]["requests"] == 2 and R["stats"]["no_room"] == 1 and R["gpu"]["stats_rc"] == -errno.ENOSPC
    assert all(v[2] == 9000 for v in tab.d.values())
    R = _check(gpu_ctx, tab, c, dst, [1] * 200, 10000, req_cap=0)
    assert R["stats"]["requests"] == 0 and R["stats"]["no_room"] == 3


def test_fallback_against_strict_on_the_same_batch(gpu_ctx):
    rng = np.random.default_rng(9)
    init, dst, sock = _every_class(rng, 300)
    out = {}
    for flags in (0, abi.NEIGH_FALLBACK):
        tab = _setup(gpu_ctx, 64, init)
        out[flags] = _check(gpu_ctx, tab, U.cfg(netmask=MASK, gateway=GW, flags=flags), dst, sock, 100000)
    s, f = out[0], out[abi.NEIGH_FALLBACK]
    miss = np.isin(s["state"], [abi.NEIGH_C_EXPIRED, abi.NEIGH_C_INCOMPLETE, abi.NEIGH_C_INSERTED])
    assert miss.sum() > 20 and np.array_equal(s["state"], f["state"]) and np.array_equal(s["req"], f["req"])
    assert np.all(s["sockfd_out"][miss] == -1) and np.array_equal(f["sockfd_out"], np.array(sock, np.int32))
    fb = np.array(U.struct.unpack("<II", U.FALLBACK_MAC + b"\0\0"), np.uint32)
    assert np.all(f["dmac"][miss] == fb) and not s["dmac"][miss].any()
    assert np.array_equal(s["dmac"][~miss], f["dmac"][~miss])
    assert f["stats"]["fallback"] == s["stats"]["unresolved"] == miss.sum()


@pytest.mark.parametrize("now", [50000, (1 << 32) + 20000], ids=["plain", "wrapped"])
def test_expiry_at_the_ttl_and_past_it(gpu_ctx, now):
    """Entries whose age is ttl_ms - 1, ttl_ms and ttl_ms + 1, and incomplete ones whose age is retrans_ms - 1 and
    retrans_ms; `wrapped`: now has passed 2^32 since the stamps were taken."""
    ttl, rt = 30000, 1000
    macs = [bytes([2, 0, 0, 0, 0, k]) for k in range(5)]
    ips = [f"172.31.100.{120 + k}" for k in range(5)]
    init = [(ips[k], macs[k], U.REACHABLE, (now - age) & U.U32) for k, age in enumerate((ttl - 1, ttl, ttl + 1))]
    tab = _setup(gpu_ctx, 16, init)
    c = U.cfg(ttl_ms=ttl, retrans_ms=rt)
    # two unknown hosts become incomplete at now - rt + 1 and now - rt
    _check(gpu_ctx, tab, c, [ips[3]], [0], now - rt + 1)
    _check(gpu_ctx, tab, c, [ips[4]], [0], now - rt)
    R = _check(gpu_ctx, tab, c, ips + ips, [0] * 10, now)
    names = [U.CLASS_NAMES[s] for s in R["state"]]
    assert names == ["hit", "hit", "expired", "incomplete", "incomplete"] + ["hit", "hit"] + ["incomplete"] * 3
    assert R["req_hops"] == [U.raw(ips[2]), U.raw(ips[4])] and R["req_origin"].tolist() == [2, 4]
    assert tab.d[U.raw(ips[2])] == [macs[2], U.INCOMPLETE, now & U.U32]
    assert tab.d[U.raw(ips[3])][2] == (now - rt + 1) & U.U32 and tab.d[U.raw(ips[4])][2] == now & U.U32


def test_a_full_table_of_eight(gpu_ctx):
    rng = np.random.default_rng(17)
    ips = U.colliding_ips(8, 7, 5) + U.colliding_ips(8, 2, 3)      # probes that wrap past the end
    init = [(ip, A.rand_mac(rng), [U.REACHABLE, U.STATIC][k % 2], 1000) for k, ip in enumerate(ips)]
    tab = _setup(gpu_ctx, 8, init)
    new = U.colliding_ips(8, 7, 2, start=5000) + ["10.3.3.3"]
    dst = [ips[k % 8] for k in range(150)]
    for k in range(0, 150, 7):
        dst[k] = new[(k // 7) % 3]
    c = U.cfg(ttl_ms=5000)
    before = abi.neigh_dump(gpu_ctx, as_list=True)
    R = _check(gpu_ctx, tab, c, dst, [3] * 150, 2000)
    assert R["stats"]["table_full"] == 22 and R["stats"]["hit"] == 128 and R["stats"]["requests"] == 0
    assert abi.neigh_dump(gpu_ctx, as_list=True) == before         # nothing to write: bit-identical
    # later the four learned ones have expired: they ask, the static ones still hit, the new ones still do not fit
    R = _check(gpu_ctx, tab, c, dst, [3] * 150, 7000)
    assert R["stats"]["expired"] == 4 and R["stats"]["requests"] == 4 and R["stats"]["table_full"] == 22
    # seven entries and two new next hops in one call: one gets in, which one is unspecified
    _setup(gpu_ctx, 8, init[:7])
    g = abi.neigh_resolve_run(gpu_ctx, c, [U.raw(x) for x in [new[0], new[2]] * 5], [0] * 10, 2000)
    want = dict({k: 0 for k in U.RESOLVE_FIELDS}, inserted=1, incomplete=4, table_full=5, unresolved=10, requests=1)
    assert g["rc"] == 0 and g["stats"] == want
    got = abi.neigh_dump(gpu_ctx)
    inside = [ip for ip in (new[0], new[2]) if U.raw(ip) in got]
    assert len(got) == 8 and len(inside) == 1 and got[U.raw(inside[0])] == (bytes(6), U.INCOMPLETE, 2000)
    assert bytes(g["req"][0][38:42]) == U.raw(inside[0]).to_bytes(4, "little") and np.all(g["req"][1:] == 0xA5)


def test_learn_a_reply_then_resolve(gpu_ctx):
    """resolve asks, the reply is learned, resolve hits with the learned MAC: the request resolve wrote, turned
    around by the peer, is the frame learn takes."""
    tab = _setup(gpu_ctx, 1024)
    c = U.cfg()
    peer_ip, peer_mac = "172.31.100.200", bytes.fromhex("02c0ffee0001")
    R = _check(gpu_ctx, tab, c, [peer_ip], [4], 100)
    assert R["stats"]["inserted"] == R["stats"]["requests"] == R["stats"]["unresolved"] == 1
    req = bytes(R["gpu"]["req"][0][:42])
    assert req == A.arp_frame(sha=U.OUR_MAC, spa=U.OUR_IP, tpa=peer_ip)
    reply = A.arp_frame(op=2, sha=peer_mac, spa=peer_ip, tha=req[22:28], tpa=U.dotted(int.from_bytes(req[28:32], "little")),
                        eth_dst=req[6:12])
    bt = A.pack([A.udp_frame(np.random.default_rng(1)), reply], aligns=[0, 7])
    meta = A.host_meta(bt[0], bt[2], bt[3])
    L = U.learn(tab, c, *bt, meta, 150)
    g = abi.neigh_learn_run(gpu_ctx, c, abi.rx_upload(gpu_ctx, bt[0], bt[2], bt[3]), meta, 150)
    assert g["stats"] == L["stats"] and L["stats"]["updated"] == 1
    R = _check(gpu_ctx, tab, c, [peer_ip, peer_ip], [4, 4], 200)
    assert R["stats"]["hit"] == 2 and R["stats"]["requests"] == 0
    assert bytes(R["gpu"]["dmac"][0].tobytes()[:6]) == peer_mac and R["gpu"]["sockfd_out"][:2].tolist() == [4, 4]


def test_more_misses_than_one_finishing_round(gpu_ctx):
    """3 B + 5 misses to 300 next hops: the finishing workgroup takes them a workgroup's width at a time, and a next
    hop first asked for in one round is known in the next."""
    rng = np.random.default_rng(21)
    n = 3 * B + 5
    hops = [f"10.8.{k >> 8}.{k & 255}" for k in range(1, 301)]
    dst = [hops[int(rng.integers(0, 300))] for _ in range(n)]
    tab = _setup(gpu_ctx, 1024)
    R = _check(gpu_ctx, tab, U.cfg(), dst, [0] * n, 1)
    assert R["stats"]["inserted"] == len(set(dst)) == R["stats"]["requests"] and R["stats"]["incomplete"] == n - len(set(dst))
    R = _check(gpu_ctx, tab, U.cfg(), dst, [0] * n, 500, req_cap=7)
    assert R["stats"]["requests"] == 0 and R["stats"]["incomplete"] == n


def test_argument_errors_and_empty_batch(gpu_ctx):
    L = abi.lib()
    tab = _setup(gpu_ctx, 8)
    d = gpu_ctx.upload(np.full(4, U.raw("172.31.100.9"), np.uint32))
    s = gpu_ctx.upload(np.zeros(4, np.int32))
    o = [gpu_ctx.upload(np.full(64, 0x77, np.uint8)) for _ in range(3)]
    rq = gpu_ctx.upload(np.full(64 * 4 + 64, 0x77, np.uint8))
    og = gpu_ctx.upload(np.full(8, 7, np.uint32))

    def call(c=U.cfg(), dp=d.ptr, sp=s.ptr, n=4, out=True, dm=o[0].ptr, so=o[1].ptr, st=o[2].ptr, rp=rq.ptr, op=og.ptr,
             cap=4, ctx=gpu_ctx.handle):
        ov = abi.NeighOut(dm, so, st, rp, op, cap)
        return L.udpdk_gpu_neigh_resolve(ctx, C.byref(c) if c is not None else None, C.c_void_p(dp), C.c_void_p(sp), n, 5,
                                         C.byref(ov) if out else None)
    for kw in (dict(c=None), dict(ctx=None), dict(dp=None), dict(sp=None), dict(out=False), dict(dm=None), dict(so=None),
               dict(st=None), dict(rp=None), dict(op=None), dict(dm=o[0].ptr + 4), dict(rp=rq.ptr + 8),
               dict(c=U.cfg(src_ip="0.0.0.0")), dict(c=U.cfg(flags=2))):
        assert call(**kw) == -errno.EINVAL, kw
    with abi.GpuContext(0, max_frames=1024, max_lanes=1) as fresh:                # no table
        st = abi.NeighResolveStats()
        assert L.udpdk_gpu_neigh_resolve_stats(fresh.handle, C.byref(st)) == -errno.ENOENT
    gpu_ctx.sync()
    assert abi.neigh_dump(gpu_ctx) == {} and np.all(gpu_ctx.download(rq, np.uint8, 320) == 0x77)   # nothing was enqueued
    st = abi.NeighResolveStats()
    assert call(n=0) == 0 and L.udpdk_gpu_neigh_resolve_stats(gpu_ctx.handle, C.byref(st)) == 0
    assert all(getattr(st, k) == 0 for k in U.RESOLVE_FIELDS)
    assert call(rp=None, op=None, cap=0) == 0                                      # no room for requests is allowed
    assert L.udpdk_gpu_neigh_resolve_stats(gpu_ctx.handle, C.byref(st)) == -errno.ENOSPC
    assert (st.inserted, st.incomplete, st.requests, st.no_room) == (1, 3, 0, 1)
    assert gpu_ctx.download(og, np.uint32, 8).tolist() == [7] * 8
