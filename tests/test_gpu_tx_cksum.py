"""udpdk_gpu_tx_build_flags with UDPDK_TX_UDP_CKSUM: tx_build<true> on both of its paths (tx_small
and the chunk sweep), with fragmentation, over several rounds and groups per wave, and from the
socket layer.

The harness is that of test_gpu_tx_edges.py: the output is pre-filled with 0xEE, frames_bytes is
4096 bytes short of the allocation, and the whole downloaded buffer, guard included, is compared
with an image built per datagram from O.tx_frame, the tests' own RFC 768 sum at bytes 40-41
(tx_cksum_util.py, pinned against the oracle's RX in test_tx_cksum_ref.py) and O.tx_fragment.
The downloaded frames then go through the oracle's RX, which must find every checksum good
(fragmented datagrams after concatenating their fragments' IPv4 payloads)."""
import ctypes as C
import errno
import os

import numpy as np
import pytest

import oracle as O
import tx_cksum_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
SRC_IP = abi.raw_ip("172.31.100.2")
SLOTS = [(0, 10000, 1), (abi.raw_ip("10.1.2.3"), 5353, 1), (abi.raw_ip("10.9.9.9"), 7, 0)]
GUARD = 4096
ENV = ("UDPDK_TX_PARTS", "UDPDK_TX_GRID")
CK = abi.TX_UDP_CKSUM


def _forced_ctx(env):
    old = {k: os.environ.get(k) for k in ENV}
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return abi.GpuContext(0, max_frames=1 << 16, max_lanes=8)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def grid3_ctx():
    ctx = _forced_ctx({"UDPDK_TX_GRID": "3"})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def parts4_ctx():
    ctx = _forced_ctx({"UDPDK_TX_PARTS": "4"})
    yield ctx
    ctx.close()


def _span(L, mtu):
    if mtu and L + 42 > mtu:
        return L + 8 + 34 * -(-(L + 8) // (mtu - 20))
    return L + 42


def _rand_bytes(rng, n):
    """Never 0x00 (an out-of-range load), 0xEE (the output fill) or 0xA5 (the tailroom fill)."""
    b = rng.integers(1, 254, n, dtype=np.uint8)
    b[b == 0xA5] = 0xFE
    b[b == 0xEE] = 0xFF
    return b


class TxCase:
    """One tx_build call: descriptors, the payload buffer and the output geometry."""

    def __init__(self, rng, lens, *, mtu=None, frame_start=0, frame_gap=lambda i: 0, frame_res=None,
                 pay_gap=lambda i: i % 3, pay_res=None, slots=SLOTS, exact=False):
        n = len(lens)
        self.n, self.mtu, self.slots, self.exact = n, mtu, slots, exact
        self.lens = np.asarray(lens, np.int64)
        self.fo = np.zeros(n, np.int64)
        self.po = np.zeros(n, np.int64)
        pos, ppos = frame_start, 0
        for i in range(n):
            if frame_res is not None:                      # 1-16 untouched bytes, then residue
                pos += 1 if i else 0
                pos += (int(frame_res[i]) - pos) % 16
            if pay_res is not None:
                ppos += (int(pay_res[i]) - ppos) % 16
            self.fo[i], self.po[i] = pos, ppos
            pos += _span(int(self.lens[i]), mtu) + (0 if frame_res is not None else frame_gap(i))
            ppos += int(self.lens[i]) + (0 if pay_res is not None else pay_gap(i))
        if frame_res is None and n:
            pos -= frame_gap(n - 1)
        if exact or pay_res is not None:
            ppos = int(self.po[-1] + self.lens[-1])
        self.frames_bytes = pos                            # the last frame ends the buffer
        self.payload_bytes = ppos
        tail = abi.FRAMES_TAILROOM if exact else 256
        self.pay = np.concatenate([_rand_bytes(rng, ppos), np.full(tail, 0xA5, np.uint8)])
        self.sock = rng.integers(0, len(slots), n).astype(np.int64)
        self.dip = rng.integers(0, 2**32, n, dtype=np.uint64)
        self.dport = rng.integers(0, 65536, n)

    def payload(self, i):
        return self.pay[self.po[i]:self.po[i] + self.lens[i]].tobytes()

    def written(self, i):
        """The contract of udpdk_gpu_tx_build: a datagram whose socket, payload range or frame
        range is outside the batch is skipped."""
        L = int(self.lens[i])
        return (0 <= self.sock[i] < len(self.slots) and self.fo[i] + _span(L, self.mtu) <= self.frames_bytes
                and self.po[i] + L <= self.payload_bytes)

    def expected(self, i, cksum):
        return U.expected(SRC_MAC, DST_MAC, SRC_IP, self.slots[self.sock[i]], int(self.dip[i]),
                          int(self.dport[i]), self.payload(i), self.mtu, cksum)


def _run(ctx, t, flags=CK, rc_want=0, entry="flags"):
    """One call of udpdk_gpu_tx_build_flags (or, entry = 'mtu', udpdk_gpu_tx_build_mtu): the
    whole output buffer, guard included."""
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=t.slots))
    bufs = [ctx.upload(t.pay), ctx.upload(t.po.astype(np.uint32)), ctx.upload(t.lens.astype(np.uint16)),
            ctx.upload(t.sock.astype(np.int32)), ctx.upload(t.dip.astype(np.uint32)),
            ctx.upload(t.dport.astype(np.uint16)), ctx.upload(t.fo.astype(np.uint32))]
    size = t.frames_bytes + GUARD
    out = ctx.alloc(size)
    abi.lib().udpdk_gpu_memset(ctx.handle, C.c_void_p(out.ptr), 0xEE, size)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*SRC_MAC), (C.c_uint8 * 6)(*DST_MAC), SRC_IP)
    bt = abi.TxBatch(bufs[0].ptr, t.payload_bytes, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                     bufs[5].ptr, t.n)
    ot = abi.TxOut(out.ptr, t.frames_bytes, bufs[6].ptr)
    if entry == "mtu":
        rc = abi.lib().udpdk_gpu_tx_build_mtu(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot), t.mtu or 0)
    else:
        rc = abi.lib().udpdk_gpu_tx_build_flags(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot),
                                                t.mtu or 0, flags)
    assert rc == rc_want
    res = ctx.download(out, np.uint8, size)
    for b in bufs + [out]:
        b.free()
    return res


def _image(t, cksum):
    size = t.frames_bytes + GUARD
    want = np.full(size, 0xEE, np.uint8)
    owner = np.full(size, -1, np.int64)
    done = []
    for i in range(t.n):
        if not t.written(i):
            continue
        blob, frames = t.expected(i, cksum)
        fo = int(t.fo[i])
        assert len(blob) == _span(int(t.lens[i]), t.mtu), i
        want[fo:fo + len(blob)] = np.frombuffer(blob, np.uint8)
        owner[fo:fo + len(blob)] = i
        done.append((i, fo, frames))
    return want, owner, done


def _check(t, res, want_written=None, cksum=True):
    """The whole buffer against the patched-oracle image; then the oracle's RX on what was
    downloaded: CSUM_OK on every datagram (CSUM_NONE on all of them with the flag off)."""
    want, owner, done = _image(t, cksum)
    if want_written is not None:
        assert [d[0] for d in done] == want_written
    bad = np.nonzero(res != want)[0]
    if bad.size:
        b = int(bad[0])
        i = int(owner[b])
        where = "guard" if b >= t.frames_bytes else "untouched bytes" if i < 0 else \
            f"datagram {i} (len {t.lens[i]}, frame_off {t.fo[i]}, payload_off {t.po[i]}, byte {b - t.fo[i]})"
        raise AssertionError(f"{bad.size} bytes differ, the first at {b}: got {res[b]:#04x} want "
                             f"{want[b]:#04x}, {where}")
    whole = []
    for i, fo, frames in done:
        if len(frames) == 1:
            whole.append(res[fo:fo + len(frames[0])].tobytes())
        else:           # fragment 0's header without its fragment field, then every fragment's data
            pos, parts = fo, []
            for f in frames:
                parts.append(res[pos + 34:pos + len(f)].tobytes())
                pos += t.mtu + 14
            whole.append(res[fo:fo + 20].tobytes() + b"\0\0" + res[fo + 22:fo + 34].tobytes() + b"".join(parts))
    # (a frame length is 16 bits in the RX ABI: a reassembled datagram longer than that is
    # checked with the helper instead)
    state = abi.UDP_OK if cksum else abi.UDP_NONE
    for k, f in enumerate(whole):
        if len(f) > 0xFFFF:
            assert (U.patch(f) == f) if cksum else (f[40:42] == b"\0\0"), done[k][0]
    ids = [k for k, f in enumerate(whole) if len(f) <= 0xFFFF]
    if ids:
        st = U.rx_csum_states([whole[k] for k in ids])
        assert st == [state] * len(ids), [done[k][0] for k, s in zip(ids, st) if s != state][:8]
    return done


def _cksum_bytes(t):
    """Buffer positions of bytes 40-41 of every written datagram's first frame."""
    pos = [int(t.fo[i]) + 40 for i in range(t.n) if t.written(i)]
    return np.array(pos + [p + 1 for p in pos], np.int64)


def _only_cksum_differs(t, on, off):
    """Flag on against flag off: nothing but the checksum fields differs, and those are 0 off."""
    d = np.nonzero(on != off)[0]
    assert np.isin(d, _cksum_bytes(t)).all(), "a byte outside the checksum fields differs"
    assert not off[_cksum_bytes(t)].any()


# ---- both paths and the boundary between them --------------------------------------------------
EDGE_SMALL = [0, 1, 2, 21, 22, 37, 38]
EDGE_SWEEP = [39, 40, 1457, 1458]


@pytest.mark.parametrize("start", [0, 5], ids=["even", "odd"])
def test_lengths_both_paths(gpu_ctx, start):
    """Group 0: frames of at most 80 bytes (tx_small, 38 its last length). Group 1: the same
    lengths beside 39 (the first sweep length), 40, 1457 and 1458, so all go through the sweep.
    Group 2: one 1458-byte datagram forces 63 small ones onto the sweep. Frames back to back, so
    both frame-offset parities occur in every group."""
    rng = np.random.default_rng(200 + start)
    g0 = EDGE_SMALL + list(rng.integers(0, 39, 64 - len(EDGE_SMALL)))
    g1 = EDGE_SMALL + EDGE_SWEEP + list(rng.integers(0, 200, 64 - len(EDGE_SMALL) - len(EDGE_SWEEP)))
    g2 = list(rng.integers(0, 39, 64))
    g2[17] = 1458
    t = TxCase(rng, g0 + g1 + g2, frame_start=start)
    assert {int(x) & 1 for x in t.fo[:64]} == {0, 1}
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


# ---- alignment ----------------------------------------------------------------------------------
@pytest.mark.parametrize("path,lens", [("small", (22, 23)), ("sweep", (100, 101))])
def test_alignment(gpu_ctx, path, lens):
    """All 16 x 16 pairs of (frame_off mod 16, payload_off mod 16) at an even and an odd length:
    odd frame offsets take the byte-lane swap, odd lengths the zero pad."""
    rng = np.random.default_rng(210)
    trip = [(a, b, L) for a in range(16) for b in range(16) for L in lens]
    t = TxCase(rng, [x[2] for x in trip], frame_res=[x[0] for x in trip], pay_res=[x[1] for x in trip])
    assert all(t.fo[i] % 16 == x[0] and t.po[i] % 16 == x[1] for i, x in enumerate(trip))
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


# ---- a sum whose complement is zero ------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("path,lens", [("small", [2, 22, 38, 30]), ("sweep", [40, 100, 1458, 64])])
def test_zero_sum_is_sent_as_ffff(gpu_ctx, path, lens, parity):
    """Every payload's last word is chosen so that the complemented sum is 0: the field on the
    wire is 0xFFFF, at even and at odd frame offsets."""
    rng = np.random.default_rng(220 + parity)
    lens = lens * 4
    t = TxCase(rng, lens, frame_res=[(2 * i + parity) % 16 for i in range(len(lens))], pay_gap=lambda i: 1 + i % 3)
    for i in range(t.n):
        frame = O.tx_frame(SRC_MAC, DST_MAC, SRC_IP, t.slots[t.sock[i]][2], t.slots[t.sock[i]][0],
                           t.slots[t.sock[i]][1], int(t.dip[i]), int(t.dport[i]), t.payload(i))
        end = int(t.po[i] + t.lens[i])
        t.pay[end - 2:end] = np.frombuffer(U.zero_sum_word(frame), np.uint8)
    res = _run(gpu_ctx, t)
    _check(t, res, list(range(t.n)))
    assert all(t.fo[i] % 2 == parity for i in range(t.n))
    assert np.all(res[_cksum_bytes(t)] == 0xFF)


# ---- source address -----------------------------------------------------------------------------
def test_source_address_per_slot(gpu_ctx):
    """Sockets bound to a specific address, bound to ANY and unbound in one batch, on both paths:
    the pseudo-header carries the address the IPv4 header got."""
    rng = np.random.default_rng(230)
    t = TxCase(rng, [20 + i % 19 for i in range(64)] + [100 + 7 * i for i in range(64)], frame_start=1)
    t.sock = np.arange(t.n) % 3
    done = _check(t, _run(gpu_ctx, t), list(range(t.n)))
    for i, fo, frames in done:
        ip, _, bound = SLOTS[t.sock[i]]
        assert int.from_bytes(frames[0][26:30], "little") == (ip if bound and ip else SRC_IP)


# ---- fragmentation ------------------------------------------------------------------------------
def test_fragments_mtu_1500(gpu_ctx):
    """1458 goes out whole, 1459 as two frames (the second carries 1 byte), 2952 as two and 65507
    as 45: the checksum covers the whole datagram and is in fragment 0 only; every other byte is
    the flag-off build's."""
    rng = np.random.default_rng(240)
    lens = [1458, 1459, 2952, 65507, 0, 30, 1472, 1473] + list(rng.integers(0, 4000, 80))
    t = TxCase(rng, lens, mtu=1500, frame_start=3)
    on = _run(gpu_ctx, t)
    _check(t, on, list(range(t.n)))
    _only_cksum_differs(t, on, _run(gpu_ctx, t, flags=0))


def test_fragments_mtu_68_sum_persists_over_rounds(gpu_ctx):
    """One 65507-byte datagram in 48-byte fragments: 1365 frames, 22 rounds of 64, its sum kept
    from round to round; a small datagram follows it in the same group (odd and even offsets)."""
    rng = np.random.default_rng(241)
    for start in (0, 7):
        t = TxCase(rng, [65507, 20, 27, 5000], mtu=68, frame_start=start, frame_gap=lambda i: 1)
        on = _run(gpu_ctx, t)
        _check(t, on, list(range(t.n)))
        _only_cksum_differs(t, on, _run(gpu_ctx, t, flags=0))


def test_fragments_mtu_572_many_frames_per_group(gpu_ctx):
    """64 datagrams of about 3000 bytes at MTU 572: six frames each, 384 frames in the group, so
    frame, datagram and lane all differ."""
    rng = np.random.default_rng(242)
    t = TxCase(rng, rng.integers(2900, 3100, 64), mtu=572, frame_start=9, frame_gap=lambda i: i % 4)
    on = _run(gpu_ctx, t)
    _check(t, on, list(range(t.n)))
    _only_cksum_differs(t, on, _run(gpu_ctx, t, flags=0))


# ---- several groups per wave --------------------------------------------------------------------
@pytest.mark.parametrize("mtu", [None, 1500])
def test_group_reuse(grid3_ctx, mtu):
    """Three workgroups (12 waves) for 27 groups: every wave runs the group loop two or three
    times, so a group's sums must not leak into the next; all-small groups (every third) between
    mixed ones."""
    rng = np.random.default_rng(250 + (mtu or 0))
    n = 64 * 26 + 17
    lens = rng.integers(0, 4000 if mtu else 1459, n)
    for g in range(0, n // 64 + 1, 3):
        lens[64 * g:64 * g + 64] = rng.integers(0, 39, len(lens[64 * g:64 * g + 64]))
    t = TxCase(rng, lens, mtu=mtu, frame_start=9, frame_gap=lambda i: i % 4)
    _check(t, _run(grid3_ctx, t), list(range(n)))


# ---- parts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mtu", [None, 1500])
def test_parts_knob_is_ignored(parts4_ctx, mtu):
    """A context forced to four waves per group: the checksum form still runs one and gives the
    same images; with flags 0 the output is udpdk_gpu_tx_build_mtu's, byte for byte."""
    rng = np.random.default_rng(260 + (mtu or 0))
    lens = rng.integers(0, 4000 if mtu else 1459, 64 * 3 + 5)
    t = TxCase(rng, lens, mtu=mtu, frame_start=5)
    _check(t, _run(parts4_ctx, t), list(range(t.n)))
    off = _run(parts4_ctx, t, flags=0)
    _check(t, off, list(range(t.n)), cksum=False)
    assert np.array_equal(off, _run(parts4_ctx, t, entry="mtu"))


# ---- skipped datagrams --------------------------------------------------------------------------
BAD = [0, 30, 31, 32, 63, 64]


@pytest.mark.parametrize("mtu", [None, 1500])
@pytest.mark.parametrize("kind", ["frame", "payload", "sock_neg", "sock_n"])
def test_skipped_datagrams_get_no_patch(gpu_ctx, kind, mtu):
    """Descriptors one byte past their buffer or a socket outside the table, on lanes 0, 63 and
    three consecutive ones of a sweep-path wave: nothing is written for them, not even the two
    checksum bytes, and every neighbour is exact."""
    rng = np.random.default_rng(270 + (mtu or 0))
    n = 128
    lens = rng.integers(100, 1459, n)
    if mtu:
        lens[[5, 31, 40, 70, 100, n - 1]] = [2000, 3000, 1459, 1473, 2952, 2953]
    t = TxCase(rng, lens, mtu=mtu, frame_start=11, frame_gap=lambda i: 1 + i % 7, exact=True)
    for i in BAD:
        L = int(lens[i])
        if kind == "frame":
            t.fo[i] = t.frames_bytes + 1 - _span(L, mtu)
        elif kind == "payload":
            t.po[i] = t.payload_bytes + 1 - L
        else:
            t.sock[i] = -1 if kind == "sock_neg" else len(t.slots)
    _check(t, _run(gpu_ctx, t), [i for i in range(n) if i not in BAD])


def test_skipped_datagrams_small_path(gpu_ctx):
    """The same on a wave of small frames (tx_small)."""
    rng = np.random.default_rng(275)
    lens = rng.integers(0, 39, 128)
    lens[[31, 64]] = [20, 10]
    t = TxCase(rng, lens, frame_start=3, frame_gap=lambda i: 1 + i % 5, exact=True)
    t.sock[[0, 63]] = [-1, len(t.slots)]
    t.fo[31] = t.frames_bytes + 1 - _span(20, None)
    t.po[64] = t.payload_bytes + 1 - 10
    _check(t, _run(gpu_ctx, t), [i for i in range(t.n) if i not in (0, 31, 63, 64)])


# ---- flag off -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mtu", [None, 1500])
def test_flags_zero_is_tx_build_mtu(gpu_ctx, mtu):
    """udpdk_gpu_tx_build_flags(..., 0) on a random mixed batch: udpdk_gpu_tx_build_mtu's output,
    byte for byte, with bytes 40-41 of every datagram zero."""
    rng = np.random.default_rng(280 + (mtu or 0))
    lens = rng.integers(0, 4000 if mtu else 1459, 64 * 4 + 9)
    lens[64:128] = rng.integers(0, 39, 64)
    t = TxCase(rng, lens, mtu=mtu, frame_start=5, frame_gap=lambda i: i % 3)
    off = _run(gpu_ctx, t, flags=0)
    _check(t, off, list(range(t.n)), cksum=False)
    assert not off[_cksum_bytes(t)].any()
    assert np.array_equal(off, _run(gpu_ctx, t, entry="mtu"))


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFE])
def test_unknown_flag_bits_rejected(gpu_ctx, flags):
    rng = np.random.default_rng(290)
    t = TxCase(rng, [100, 20, 2000])
    assert np.all(_run(gpu_ctx, t, flags=flags, rc_want=-errno.EINVAL) == 0xEE)


# ---- round trip through the RX path on the GPU --------------------------------------------------
def test_round_trip_rx_verifies_every_checksum(gpu_ctx):
    """tx_build<true> at MTU 1500 -> udpdk_gpu_rx -> udpdk_gpu_rx_reassemble -> udpdk_gpu_rx on the
    reassembled datagrams: unfragmented ones are DELIVERED with CSUM_OK by the first pass, the
    others (last fragments of 1-7 bytes among them) by the second; no frame reports CSUM_NONE."""
    rng = np.random.default_rng(300)
    mtu = 1500
    lens = [1480 * m + k - 8 for m in (1, 2, 3) for k in range(1, 8)]
    lens += [0, 1, 22, 38, 39, 100, 1457, 1458] + rng.integers(0, 1459, 60).tolist()
    lens += rng.integers(1459, 5900, 60).tolist()
    lens = [int(lens[k]) for k in rng.permutation(len(lens))]
    n = len(lens)
    port = abi.raw_port(10001)
    gpu_ctx.upload_snapshot(abi.snapshot_from_lists({port: [(0, 0, 0)]}, 1, slots=[(0, abi.raw_port(10000), 1)]))
    abi.frag_table_create(gpu_ctx, bucket_num=64, bucket_entries=16, max_cycles=1000)
    po = np.cumsum([0] + lens[:-1]).astype(np.uint32)
    pay = np.concatenate([rng.integers(0, 256, int(po[-1]) + lens[-1], dtype=np.uint8), np.zeros(64, np.uint8)])
    spans = [_span(L, mtu) for L in lens]
    fo = np.cumsum([0] + spans[:-1]).astype(np.uint32)
    cap = int(fo[-1]) + spans[-1] + 64
    bufs = [gpu_ctx.upload(pay), gpu_ctx.upload(po), gpu_ctx.upload(np.array(lens, np.uint16)),
            gpu_ctx.upload(np.zeros(n, np.int32)), gpu_ctx.upload(np.full(n, abi.raw_ip("172.31.100.1"), np.uint32)),
            gpu_ctx.upload(np.full(n, port, np.uint16)), gpu_ctx.upload(fo)]
    frames = gpu_ctx.alloc(cap)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*SRC_MAC), (C.c_uint8 * 6)(*DST_MAC), SRC_IP)
    tb = abi.TxBatch(bufs[0].ptr, len(pay) - 64, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, n)
    assert abi.lib().udpdk_gpu_tx_build_flags(gpu_ctx.handle, C.byref(cfg), C.byref(tb),
                                              C.byref(abi.TxOut(frames.ptr, cap - 64, bufs[6].ptr)), mtu, CK) == 0
    off, ln, whole = [], [], []
    for L, f0 in zip(lens, fo):
        nf = -(-(L + 8) // (mtu - 20)) if L + 42 > mtu else 1
        whole += [nf == 1] * nf
        for k in range(nf):
            off.append(int(f0) + k * (mtu + 14))
            ln.append(mtu + 14 if k + 1 < nf else _span(L, mtu) - (nf - 1) * (mtu + 14))
    whole = np.array(whole)
    db = abi.RxDeviceBatch(frames, cap - 64, gpu_ctx.upload(np.array(off, np.uint32)),
                           gpu_ctx.upload(np.array(ln, np.uint16)), None, len(off))
    out = abi.rx_alloc_out(gpu_ctx, len(off), 1, len(off))
    m1, _, _, c1, rc = abi.rx_run(gpu_ctx, db, out)
    assert rc == 0
    assert np.all(abi.meta_verdict(m1[whole]) == abi.V_DELIVERED) and np.all(abi.meta_udp(m1[whole]) == abi.UDP_OK)
    assert np.all(abi.meta_verdict(m1[~whole]) == abi.V_FRAG)
    n_whole = sum(1 for L in lens if L + 42 <= mtu)
    assert c1[abi.C_UDP_NONE] == 0 and c1[abi.C_UDP_BAD] == 0 and c1[abi.C_UDP_OK] == n_whole
    rb, origin, st = abi.rx_reassemble(gpu_ctx, db, out.meta, 0)
    assert st["done"] == n - n_whole and st["errors"] == st["holes"] == st["stored"] == 0
    out2 = abi.rx_alloc_out(gpu_ctx, rb.n, 1, rb.n)
    m2, _, _, c2, rc = abi.rx_run(gpu_ctx, rb, out2)
    assert rc == 0 and rb.n == n - n_whole
    assert np.all(abi.meta_verdict(m2) == abi.V_DELIVERED) and np.all(abi.meta_udp(m2) == abi.UDP_OK)
    assert c2[abi.C_UDP_NONE] == 0 and c2[abi.C_UDP_BAD] == 0 and c2[abi.C_UDP_OK] == n - n_whole


# ---- socket layer -------------------------------------------------------------------------------
S_SRC_MAC, S_DST_MAC, S_SRC_IP = "68:05:ca:95:f8:ec", "68:05:ca:95:fa:64", "172.31.100.2"


def _init(tmp_path, extra):
    ini = tmp_path / "udpdk.ini"
    ini.write_text(f"[port0]\nmac_addr = {S_SRC_MAC}\nip_addr = {S_SRC_IP}\n"
                   f"[port0_dst]\nmac_addr = {S_DST_MAC}\n"
                   "[gpu]\ndevice = 0\nmax_frames = 65536\nmax_lanes = 64\n" + extra)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    assert abi.lib().udpdk_init(3, argv) == 0


SENDS = [0, 1, 22, 39, 1458, 1459, 5000]


def _send_and_drain(api, s, seed):
    """SENDS through sendto and one drain: (got frames, expected frames with and without the
    checksum), datagram by datagram."""
    rng = np.random.default_rng(seed)
    pays = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in SENDS]
    for p in pays:
        assert api.sendto(s, p, "172.31.100.1", 10001) == len(p)
    got = api.tx_drain()
    want = {}
    for ck in (True, False):
        want[ck] = [f for p in pays for f in U.expected(SRC_MAC, DST_MAC, SRC_IP, (abi.raw_ip("10.1.2.3"), abi.raw_port(5353), 1),
                                                        abi.raw_ip("172.31.100.1"), abi.raw_port(10001), p, 1500, ck)[1]]
    return got, want


@pytest.mark.parametrize("key,on", [("tx_udp_cksum = 1\n", True), ("tx_udp_cksum = 0\n", False), ("", False)],
                         ids=["on", "off", "default"])
def test_socket_layer_ini_key(tmp_path, host_api, key, on):
    """[gpu] tx_udp_cksum = 1: the drained frames (one datagram over the MTU among them) carry
    the helper's checksum; 0 or no key: bytes 40-41 are 0, the frames are the reference's."""
    _init(tmp_path, key)
    try:
        assert host_api.config_tx_cksum(-1) == int(on)
        s = host_api.socket()
        assert host_api.bind(s, "10.1.2.3", 5353) == 0
        got, want = _send_and_drain(host_api, s, 310)
        assert got == want[on]
        assert all((f[40:42] != b"\0\0") == on for f in got if not (f[20] & 0x1F or f[21]))
    finally:
        abi.lib().udpdk_cleanup()


def test_socket_layer_toggle_between_drains(tmp_path, host_api):
    """udpdk_config_tx_cksum between two drains changes the second drain only, both ways."""
    _init(tmp_path, "")
    try:
        s = host_api.socket()
        assert host_api.bind(s, "10.1.2.3", 5353) == 0
        got, want = _send_and_drain(host_api, s, 320)
        assert got == want[False]
        assert host_api.config_tx_cksum(1) == 0
        got, want = _send_and_drain(host_api, s, 321)
        assert got == want[True]
        assert host_api.config_tx_cksum(0) == 1
        got, want = _send_and_drain(host_api, s, 322)
        assert got == want[False]
    finally:
        abi.lib().udpdk_cleanup()
