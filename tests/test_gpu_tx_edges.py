"""tx_build at its edges: every launch form forced (UDPDK_TX_PARTS / UDPDK_TX_GRID, read at
context creation), every 16-byte alignment of frame and payload on both paths (tx_small and the
chunk sweep), payloads and frames ending at the last byte of their buffers, out-of-range
descriptors on the sweep path, and the MTU range's ends.

Every run pre-fills the output with 0xEE, passes a frames_bytes 4096 bytes short of the
allocation and compares the whole downloaded buffer, guard included, with an image built from
O.tx_frame / O.tx_fragment: a byte written outside a frame, or not written inside one, fails
whichever datagram it belongs to. Each written datagram is then checked from the test's own
inputs with no oracle in between: frame bytes from 42 on are the payload; fragments' IPv4
payloads concatenate to the UDP header + payload, every fragment header sums to 0xFFFF (RFC 1071),
MF is on all but the last and the fragment offsets are contiguous."""
import ctypes as C
import errno
import os
import struct

import numpy as np
import pytest

import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
SRC_IP = abi.raw_ip("172.31.100.2")
SLOTS = [(0, 10000, 1), (abi.raw_ip("10.1.2.3"), 5353, 1), (abi.raw_ip("10.9.9.9"), 7, 0)]
GUARD = 4096
ENV = ("UDPDK_TX_PARTS", "UDPDK_TX_GRID")


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


@pytest.fixture(scope="module", params=[1, 2, 3, 4], ids=lambda p: f"parts{p}")
def parts_ctx(request):
    ctx = _forced_ctx({"UDPDK_TX_PARTS": str(request.param)})
    yield ctx
    ctx.close()


@pytest.fixture(scope="module", params=[1, 4], ids=lambda p: f"grid3-parts{p}")
def stride_ctx(request):
    ctx = _forced_ctx({"UDPDK_TX_PARTS": str(request.param), "UDPDK_TX_GRID": "3"})
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


def _run(ctx, t, mtu_arg=None, rc_want=0):
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=t.slots))
    mtu = t.mtu if mtu_arg is None else mtu_arg
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
    if mtu is None:
        rc = abi.lib().udpdk_gpu_tx_build(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot))
    else:
        rc = abi.lib().udpdk_gpu_tx_build_mtu(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot), mtu)
    assert rc == rc_want
    res = ctx.download(out, np.uint8, size)
    for b in bufs + [out]:
        b.free()
    return res


def _sum16(b):
    s = sum(b[i] | (b[i + 1] << 8) for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def _own_check(got, pay, mtu, sport, dport, what):
    """The datagram's output bytes against the test's inputs alone."""
    L = len(pay)
    if not (mtu and L + 42 > mtu):
        assert got[42:] == pay, f"{what}: payload"
        return
    fpl = mtu - 20
    ipp = struct.pack("<HH", sport & 0xFFFF, dport) + struct.pack(">H", L + 8) + b"\0\0" + pay
    nf = -(-len(ipp) // fpl)
    off = 0
    for k in range(nf):
        m = min(fpl, len(ipp) - off)
        f = got[k * (mtu + 14):k * (mtu + 14) + 34 + m]
        h = f[14:34]
        assert _sum16(h) == 0xFFFF, f"{what}: fragment {k} header checksum"
        assert (h[2] << 8 | h[3]) == 20 + m, f"{what}: fragment {k} total length"
        ff = h[6] << 8 | h[7]
        assert (ff & 0x1FFF) * 8 == off, f"{what}: fragment {k} offset"
        assert bool(ff & 0x2000) == (k + 1 < nf) and not ff & 0xC000, f"{what}: fragment {k} flags"
        assert f[34:] == ipp[off:off + m], f"{what}: fragment {k} payload"
        off += m
    assert off == len(ipp) and len(got) == len(ipp) + 34 * nf, what


def _check(t, res, want_written=None):
    size = t.frames_bytes + GUARD
    want = np.full(size, 0xEE, np.uint8)
    owner = np.full(size, -1, np.int64)
    done = []
    for i in range(t.n):
        if not t.written(i):
            continue
        ip, port, bound = t.slots[t.sock[i]]
        pay = t.payload(i)
        frame = O.tx_frame(SRC_MAC, DST_MAC, SRC_IP, bound, ip, port, int(t.dip[i]), int(t.dport[i]), pay)
        blob = b"".join(O.tx_fragment(frame, t.mtu)) if t.mtu else frame
        fo = int(t.fo[i])
        assert len(blob) == _span(len(pay), t.mtu), i
        want[fo:fo + len(blob)] = np.frombuffer(blob, np.uint8)
        owner[fo:fo + len(blob)] = i
        done.append((i, fo, len(blob), pay, port))
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
    for i, fo, m, pay, port in done:
        _own_check(res[fo:fo + m].tobytes(), pay, t.mtu, port, int(t.dport[i]), f"datagram {i} len {len(pay)}")
    return done


# ---- forced parts -------------------------------------------------------------------------------
@pytest.mark.parametrize("gapped", [0, 1], ids=["packed", "gaps"])
def test_parts_random(parts_ctx, gapped):
    """(a) 401 datagrams, lengths 0-100, 1457, 1458 and random below 1459: frames back to back
    from offset 5, or 1-15 untouched bytes between them."""
    rng = np.random.default_rng(20 + gapped)
    n = 64 * 6 + 17
    lens = rng.integers(0, 1459, n)
    lens[:103] = list(range(101)) + [1457, 1458]
    t = TxCase(rng, lens, frame_start=5, frame_gap=(lambda i: 1 + i % 15) if gapped else (lambda i: 0))
    _check(t, _run(parts_ctx, t), list(range(n)))


@pytest.mark.parametrize("L", [1458, 22])
def test_parts_uniform(parts_ctx, L):
    """(b) the shapes bench.py's tx_line times, by their bytes: 512 equal datagrams, payload_off =
    i * len, frames back to back, one socket."""
    rng = np.random.default_rng(L)
    n = 64 * 8
    t = TxCase(rng, [L] * n, pay_gap=lambda i: 0, slots=[(0, 10000, 1)])
    assert np.array_equal(t.po, np.arange(n) * L) and np.array_equal(t.fo, np.arange(n) * (L + 42))
    _check(t, _run(parts_ctx, t), list(range(n)))


def test_parts_fragments(parts_ctx):
    """(c) MTU 1500: unfragmented, single-fragment, 2-, 3- and 45-fragment datagrams in one batch."""
    rng = np.random.default_rng(31)
    n = 200
    lens = rng.integers(0, 4000, n)
    lens[[0, 7, 64, 65, 100, 127, 128, 199]] = [0, 1458, 1459, 2952, 2953, 65507, 1472, 1473]
    t = TxCase(rng, lens, mtu=1500, frame_start=3)
    _check(t, _run(parts_ctx, t), list(range(n)))


# ---- grid-stride --------------------------------------------------------------------------------
@pytest.mark.parametrize("mtu", [None, 1500])
def test_grid_stride(stride_ctx, mtu):
    """Three workgroups for 41 groups of 64 datagrams (x parts): every wave runs the group loop
    several times, all-small groups (every third) between mixed ones."""
    rng = np.random.default_rng(41 + (mtu or 0))
    n = 64 * 40 + 17
    lens = rng.integers(0, 4000 if mtu else 1459, n)
    for g in range(0, n // 64 + 1, 3):
        lens[64 * g:64 * g + 64] = rng.integers(0, 39, len(lens[64 * g:64 * g + 64]))
    t = TxCase(rng, lens, mtu=mtu, frame_start=9, frame_gap=lambda i: i % 4)
    _check(t, _run(stride_ctx, t), list(range(n)))


# ---- alignment matrix ---------------------------------------------------------------------------
SWEEP_LENS = [39, 40, 41, 54, 55, 56, 57, 58, 70, 71, 72, 73, 74, 100, 1458]
SMALL_LENS = [0, 1, 5, 6, 7, 21, 22, 23, 37, 38]


@pytest.mark.parametrize("path", ["sweep", "small"])
def test_alignment_matrix(gpu_ctx, path):
    """All 256 pairs of (frame_off mod 16, payload_off mod 16) at each length, neighbouring frames
    1-16 untouched bytes apart. 'small': every wave takes tx_small (all frames <= 80 bytes);
    'sweep': none does."""
    rng = np.random.default_rng(51)
    ls = SWEEP_LENS if path == "sweep" else SMALL_LENS
    trip = [(a, b, L) for a in range(16) for b in range(16) for L in ls]
    t = TxCase(rng, [x[2] for x in trip], frame_res=[x[0] for x in trip], pay_res=[x[1] for x in trip])
    assert all(t.fo[i] % 16 == x[0] and t.po[i] % 16 == x[1] for i, x in enumerate(trip))
    d = np.diff(t.fo) - (t.lens[:-1] + 42)
    assert d.min() >= 1 and d.max() <= 16
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


# ---- payload ends at payload_bytes --------------------------------------------------------------
END_LENS = list(range(39, 121)) + [1022, 1023, 1024, 1025, 1026, 1458]


@pytest.mark.parametrize("start", range(16))
def test_payload_ends_at_payload_bytes_sweep(gpu_ctx, start):
    """The sweep path's two 16-byte-aligned loads (sa, sa + 16) at the end of the payload range:
    the last payload starts at every residue mod 16 and ends exactly at payload_bytes, the
    allocation being payload_bytes + tailroom (0xA5). At MTU 1500 a 2953-byte payload's last
    fragment (1 byte) ends the buffer."""
    rng = np.random.default_rng(60 + start)
    for L, mtu in [(L, None) for L in END_LENS] + [(2953, 1500)]:
        lens = ([start] if start else []) + [L]
        t = TxCase(rng, lens, mtu=mtu, pay_gap=lambda i: 0, exact=True, slots=[(0, 10000, 1)])
        assert t.po[-1] % 16 == start and t.payload_bytes == start + L
        assert len(t.pay) == t.payload_bytes + abi.FRAMES_TAILROOM
        _check(t, _run(gpu_ctx, t), list(range(t.n)))


# ---- out-of-range descriptors -------------------------------------------------------------------
BAD = [0, 30, 31, 32, 63, 64]


@pytest.mark.parametrize("mtu", [None, 1500])
@pytest.mark.parametrize("kind", ["frame", "payload", "sock_neg", "sock_n"])
def test_out_of_range_sweep(gpu_ctx, kind, mtu):
    """Lanes 0 and 63 and three consecutive lanes of a sweep-path wave (payloads >= 100 bytes; at
    MTU 1500 among fragmented datagrams, one of the three itself fragmented) carry a descriptor
    one byte past its buffer or a socket outside the table: nothing is written for them and every
    other byte is exact. The last datagram is an exact fit: its frame (last fragment) ends at
    frames_bytes and its payload at payload_bytes, and it is written."""
    rng = np.random.default_rng(70 + (mtu or 0))
    n = 128
    lens = rng.integers(100, 1459, n)
    if mtu:
        lens[[5, 31, 40, 62, 70, 100, n - 1]] = [2000, 3000, 1459, 65507, 1473, 2952, 2953]
    t = TxCase(rng, lens, mtu=mtu, frame_start=11, frame_gap=lambda i: 1 + i % 7, exact=True)
    for i in BAD:
        L = int(lens[i])
        if kind == "frame":
            t.fo[i] = t.frames_bytes + 1 - _span(L, mtu)
        elif kind == "payload":
            t.po[i] = t.payload_bytes + 1 - L
        else:
            t.sock[i] = -1 if kind == "sock_neg" else len(t.slots)
    assert t.fo[-1] + _span(int(lens[-1]), mtu) == t.frames_bytes
    assert t.po[-1] + lens[-1] == t.payload_bytes
    _check(t, _run(gpu_ctx, t), [i for i in range(n) if i not in BAD])


# ---- MTU edges ----------------------------------------------------------------------------------
def test_mtu_68(gpu_ctx):
    """48-byte fragments: lengths 0-26 go out whole, 27 and up are fragmented although a wave of
    them is all <= 80 bytes (the gate in front of tx_small), with last fragments of 1-7 bytes."""
    rng = np.random.default_rng(80)
    lens = list(range(121)) + [1000] + list(rng.integers(0, 121, 6))        # two mixed waves
    lens += [27 + i % 12 for i in range(128)]                               # two waves of 27-38
    lens += [i % 27 for i in range(64)]                                     # one of 0-26: tx_small
    t = TxCase(rng, lens, mtu=68, frame_start=1, frame_gap=lambda i: 1 + i % 15)
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


def test_mtu_576(gpu_ctx):
    """576 - 20 = 556 is no multiple of 8, so 576 cannot be an MTU of this ABI (fragment offsets
    count 8-byte units; udpdk_gpu.h): the call is rejected and writes nothing, at the lengths
    around 576's would-be fragment edges. The nearest valid MTU, 572 (552-byte fragments), runs
    the same edges: the largest whole frame, the first fragmented one, exactly one, two and two
    full fragments, and one byte more."""
    rng = np.random.default_rng(81)
    t = TxCase(rng, [533, 534, 535, 548, 549, 1104, 1105] + list(rng.integers(0, 1200, 64)))
    assert np.all(_run(gpu_ctx, t, mtu_arg=576, rc_want=-errno.EINVAL) == 0xEE)
    lens = [529, 530, 531, 544, 545, 1096, 1097] + list(rng.integers(0, 1200, 64))
    t = TxCase(rng, lens, mtu=572, frame_start=2, frame_gap=lambda i: i % 5)
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


def test_mtu_65532(gpu_ctx):
    """The largest MTU the ABI takes: 65490 whole, 65491 as one 'fragment', 65507 as two."""
    rng = np.random.default_rng(82)
    t = TxCase(rng, [65490, 65491, 65507, 100, 0], mtu=65532, frame_start=6, frame_gap=lambda i: 3)
    _check(t, _run(gpu_ctx, t), list(range(t.n)))


@pytest.mark.parametrize("mtu", [67, 69, 65533])
def test_mtu_rejected(gpu_ctx, mtu):
    rng = np.random.default_rng(83)
    t = TxCase(rng, [100, 2000])
    res = _run(gpu_ctx, t, mtu_arg=mtu, rc_want=-errno.EINVAL)
    assert np.all(res == 0xEE)
