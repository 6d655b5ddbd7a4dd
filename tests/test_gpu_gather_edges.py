"""rx_gather at its edges, fed directly (no RX run: the kernel takes any lane_pkt): frames whose
payload bytes the test knows, at every start residue mod 16, with payload lengths around every
step of the kernel (the 64-byte preloaded window, the 64-byte step of the short loop, the branch
at 128 bytes, the 1024- and 2048-byte steps of the long loop with lane 63's carry dword), pairs
with an empty or missing partner, `first` and permuted or repeating lane entries, a last frame
ending at frames_bytes with the allocation exactly frames_bytes + tailroom, length fields that
disagree with the frame, packed slots, and the grid-stride loop (UDPDK_GATHER_GRID).

Expected values come from O.recv_gather and, independently, from the construction: payload =
frame[42 : 42 + min(data_len - 42, (dgram_len - 8) & 0xFFFF, cap)], source address and port as
written. The payload area is pre-filled with 0xEE and followed by a 64-byte guard that must stay
0xEE; slot bytes past len[k] are scratch (udpdk_gpu.h) and not looked at."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 64


def _rand_bytes(rng, n):
    """Never 0x00 (an out-of-range load), 0xEE (the output fill) or 0xA5 (the tailroom fill)."""
    b = rng.integers(1, 254, n, dtype=np.uint8)
    b[b == 0xA5] = 0xFE
    b[b == 0xEE] = 0xFF
    return b


class Frames:
    """Ethernet/IPv4/UDP frames at chosen start residues mod 16 in one buffer whose last frame
    ends at frames_bytes. specs: (payload bytes, padding bytes, dgram_len or None = 8 + payload)."""

    def __init__(self, rng, specs, residues, end_residue=None):
        n = len(specs)
        self.n = n
        self.offset = np.zeros(n, np.uint32)
        self.length = np.zeros(n, np.uint16)
        self.dgram_len = np.zeros(n, np.int64)
        sizes = [42 + p + pad for p, pad, _ in specs]
        pos = 0
        for i in range(n):
            pos += (int(residues[i % len(residues)]) - pos) % 16
            if i == n - 1 and end_residue is not None:
                pos += (end_residue - (pos + sizes[i])) % 16
            self.offset[i] = pos
            self.length[i] = sizes[i]
            pos += sizes[i]
        self.frames_bytes = pos
        buf = _rand_bytes(rng, pos)
        for i, (p, pad, dl) in enumerate(specs):
            dl = 8 + p if dl is None else dl
            self.dgram_len[i] = dl
            h = np.zeros(42, np.uint8)
            h[0:12] = np.frombuffer(bytes.fromhex("6805ca95fa646805ca95f8ec"), np.uint8)
            h[12:16] = [0x08, 0x00, 0x45, 0x00]
            h[16:18] = [(28 + p) >> 8 & 0xFF, (28 + p) & 0xFF]
            h[22:24] = [64, 17]
            h[26:30] = rng.integers(1, 255, 4)                       # source address
            h[30:34] = [172, 31, 100, 1]
            s = int(h[14:34].view(">u2").astype(np.uint64).sum())
            s = (s & 0xFFFF) + (s >> 16)
            s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
            h[24:26] = [s >> 8, s & 0xFF]
            h[34:36] = rng.integers(1, 255, 2)                       # source port
            h[36:38] = [0x27, 0x11]                                  # 10001
            h[38:40] = [dl >> 8 & 0xFF, dl & 0xFF]
            o = int(self.offset[i])
            buf[o:o + 42] = h
        self.buf = buf

    def expect(self, i, cap):
        o, dlen = int(self.offset[i]), int(self.length[i])
        n = min(dlen - 42, (int(self.dgram_len[i]) - 8) & 0xFFFF, cap)
        f = self.buf[o:o + dlen]
        return (f[42:42 + n], int.from_bytes(f[26:30].tobytes(), "little"),
                int.from_bytes(f[34:36].tobytes(), "little"))


def _gather(ctx, fb, lane_pkt, first, count, slot=None, caps=None):
    """One udpdk_gpu_rx_gather (slot) or udpdk_gpu_rx_gather_packed (caps) call over lane entries
    [first, first + count), checked against the oracle and the construction."""
    lane_pkt = np.asarray(lane_pkt, np.uint32)
    assert len(lane_pkt) >= first + count
    caps = np.full(count, slot, np.int64) if caps is None else np.asarray(caps, np.int64)
    so = np.concatenate([[0], np.cumsum(caps)])
    total = int(so[-1])
    # the allocation ends at frames_bytes + tailroom
    dev = np.concatenate([fb.buf, np.full(abi.FRAMES_TAILROOM, 0xA5, np.uint8)])
    bufs = [ctx.upload(dev), ctx.upload(fb.offset), ctx.upload(fb.length), ctx.upload(lane_pkt),
            ctx.alloc(total + GUARD), ctx.alloc(4 * count), ctx.alloc(4 * count), ctx.alloc(2 * count)]
    if slot is None:
        bufs.append(ctx.upload(so.astype(np.uint32)))
    abi.lib().udpdk_gpu_memset(ctx.handle, C.c_void_p(bufs[4].ptr), 0xEE, total + GUARD)
    bt = abi.RxBatch(bufs[0].ptr, fb.frames_bytes, bufs[1].ptr, bufs[2].ptr, None, fb.n)
    gt = abi.RxGather(bufs[4].ptr, slot if slot is not None else 16, bufs[5].ptr, bufs[6].ptr, bufs[7].ptr)
    if slot is not None:
        rc = abi.lib().udpdk_gpu_rx_gather(ctx.handle, C.byref(bt), C.c_void_p(bufs[3].ptr), first, count,
                                           C.byref(gt))
    else:
        rc = abi.lib().udpdk_gpu_rx_gather_packed(ctx.handle, C.byref(bt), C.c_void_p(bufs[3].ptr), first,
                                                  count, C.c_void_p(bufs[8].ptr), C.byref(gt))
    assert rc == 0
    ctx.sync()
    gp = ctx.download(bufs[4], np.uint8, total + GUARD)
    gl = ctx.download(bufs[5], np.uint32, count)
    gi = ctx.download(bufs[6], np.uint32, count)
    gs = ctx.download(bufs[7], np.uint16, count)
    for b in bufs:
        b.free()

    oslot = int(caps.max())
    wp, wl, wi, ws = O.recv_gather(fb.buf, fb.offset, fb.length, lane_pkt, first, count, oslot)
    wl = np.minimum(wl, caps)
    own = [fb.expect(int(lane_pkt[first + k]), int(caps[k])) for k in range(count)]
    assert np.array_equal(wl, [len(e[0]) for e in own]), "oracle and construction disagree"
    bad = np.nonzero(gl != wl)[0]
    assert bad.size == 0, f"len[{bad[0]}] = {gl[bad[0]]}, want {wl[bad[0]]} (frame {lane_pkt[first + bad[0]]})"
    assert np.array_equal(gi, wi) and np.array_equal(gi, [e[1] for e in own]), "source addresses"
    assert np.array_equal(gs, ws) and np.array_equal(gs, [e[2] for e in own]), "source ports"
    for k in range(count):
        n = int(wl[k])
        got = gp[so[k]:so[k] + n]
        assert np.array_equal(wp[k, :n], own[k][0]), "oracle and construction disagree"
        if not np.array_equal(got, own[k][0]):
            i = int(lane_pkt[first + k])
            b = int(np.nonzero(got != own[k][0])[0][0])
            raise AssertionError(f"entry {k} (frame {i}, offset {fb.offset[i]}, data_len {fb.length[i]}, "
                                 f"len {n}, cap {caps[k]}): byte {b} is {got[b]:#04x}, want {own[k][0][b]:#04x}")
    assert np.all(gp[total:] == 0xEE), "bytes written past the last slot"
    return gl


SWEEP = list(range(131)) + list(range(1000, 1041)) + list(range(2030, 2071)) + \
    list(range(3060, 3091)) + list(range(4090, 4101)) + [65493]
# start residue of frame i: every value, shifted against the lengths every 16 frames
RES = [(5 * i + i // 16) % 16 for i in range(256)]


def _sweep_batch(seed):
    rng = np.random.default_rng(seed)
    fb = Frames(rng, [(L, 0, None) for L in SWEEP], RES)
    n = len(SWEEP)
    # two waves of payloads <= 128 only, then long and short mixed, then everything mixed
    lane_pkt = np.concatenate([np.arange(128), 128 + rng.permutation(n - 128), rng.permutation(n)])
    return fb, lane_pkt.astype(np.uint32), rng


@pytest.mark.parametrize("slot", [16, 128, 2048, 65504])
def test_length_alignment_sweep(gpu_ctx, slot):
    """Slots of 16 and 128: every wave takes the short path (long frames truncated); 2048: the
    long path, payloads above it truncated; 65504: nothing truncated (a 65535-byte frame)."""
    fb, lane_pkt, _ = _sweep_batch(100)
    assert len(SWEEP) == 256 and sorted(set(int(o) % 16 for o in fb.offset)) == list(range(16))
    gl = _gather(gpu_ctx, fb, lane_pkt, 0, len(lane_pkt), slot=slot)
    assert int(gl.max()) == min(slot, 65493)


@pytest.mark.parametrize("caps", ["grid", "frame"])
def test_packed_slots(gpu_ctx, caps):
    """The sweep with packed slots: caps of 16 r, r in 1-260 (entries truncated at 16-byte grid
    points inside the KiB loops), or sized to each frame (nothing truncated)."""
    fb, lane_pkt, rng = _sweep_batch(101)
    if caps == "grid":
        cap = 16 * rng.integers(1, 261, len(lane_pkt))
    else:
        cap = (np.maximum(fb.length[lane_pkt].astype(np.int64) - 42, 1) + 15) // 16 * 16
    gl = _gather(gpu_ctx, fb, lane_pkt, 0, len(lane_pkt), caps=cap)
    want = np.array(SWEEP)[lane_pkt]
    if caps == "frame":
        assert np.array_equal(gl, want)
    else:
        assert np.any(gl < want) and np.any((gl == want) & (want > 128))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257])
def test_pairs_and_counts(gpu_ctx, count):
    """The long path's pairs (j, j + 1): (long, empty), (empty, long), (long, 1 byte); odd counts
    end on a long entry without a partner, and the last wave / workgroup is partial."""
    rng = np.random.default_rng(110 + count)
    longs = [129, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 3000]
    specs = [(L, 0, None) for L in longs] + [(0, 0, None), (1, 0, None), (0, 18, None)]
    fb = Frames(rng, specs, [3, 14, 9, 0, 7])
    e, b1 = len(longs), len(longs) + 1
    lane_pkt = []
    for p in range(count):
        lg = (p * 7 + p // 9) % len(longs)
        lane_pkt += [[lg, e + 2 * (p % 2)], [e, lg], [lg, b1]][p % 3]
    lane_pkt = lane_pkt[:count - 1] + [(count * 5) % len(longs)]
    _gather(gpu_ctx, fb, lane_pkt, 0, count, slot=3072)


def _mixed_specs(rng, n, top=3000):
    L = rng.integers(0, top + 1, n)
    short = rng.random(n) < 0.4
    L[short] = rng.integers(0, 129, int(short.sum()))
    return [(int(x), 0, None) for x in L]


@pytest.mark.parametrize("first", [0, 1, 63, 64, 100])
def test_first_and_permutations(gpu_ctx, first):
    """Entries from `first` on of a reversed lane_pkt and of one that names the same few frames
    many times."""
    rng = np.random.default_rng(120)
    fb = Frames(rng, _mixed_specs(rng, 300), RES)
    for lane_pkt in (np.arange(300)[::-1], rng.integers(0, 8, 300), np.repeat(rng.permutation(300)[:60], 5)):
        _gather(gpu_ctx, fb, lane_pkt, first, 300 - first, slot=2048)


END_LENS = list(range(1, 71)) + list(range(127, 133)) + list(range(1021, 1028)) + list(range(2045, 2052))


@pytest.mark.parametrize("res", range(16))
def test_frame_ends_at_frames_bytes(gpu_ctx, res):
    """The last frame ends at frames_bytes (frames_bytes mod 16 = res) and the allocation at
    frames_bytes + tailroom (0xA5): its payload, of each edge length, as lane 63 of a wave of short
    entries, as lane 63 of a wave with long ones, and alone in its wave."""
    rng = np.random.default_rng(130 + res)
    fill = [(int(x), 0, None) for x in rng.integers(0, 101, 63)] + \
        [(int(x), 0, None) for x in rng.integers(130, 1500, 8)]
    for L in END_LENS:
        fb = Frames(rng, fill + [(L, 0, None)], RES, end_residue=res)
        last = fb.n - 1
        assert fb.frames_bytes % 16 == res and fb.offset[last] + 42 + L == fb.frames_bytes
        mixed = list(rng.permutation(71)[:55]) + list(range(63, 71))
        lane_pkt = list(range(63)) + [last] + mixed + [last] + [last]
        _gather(gpu_ctx, fb, lane_pkt, 0, 129, slot=2064)


def test_length_fields(gpu_ctx):
    """Long frames whose dgram_len leaves Ethernet padding (payload trimmed), is below 8 (the
    uint16_t wrap: the frame length decides) or reaches past the frame (the frame length decides)."""
    rng = np.random.default_rng(140)
    specs = []
    for i in range(192):
        p, pad = int(rng.integers(130, 3000)), int(rng.integers(1, 47))
        specs.append([(p, pad, None), (p, pad, i % 8), (p, pad, 8 + p + pad + 1 + i), (p, 0, 65535)][i % 4])
    fb = Frames(rng, specs, RES)
    gl = _gather(gpu_ctx, fb, np.arange(192), 0, 192, slot=3072)
    assert all(gl[i] == (specs[i][0] if i % 4 == 0 else specs[i][0] + specs[i][1]) for i in range(192))


@pytest.fixture(scope="module")
def stride_ctx():
    old = os.environ.get("UDPDK_GATHER_GRID")
    os.environ["UDPDK_GATHER_GRID"] = "2"
    try:
        ctx = abi.GpuContext(0, max_frames=1 << 16, max_lanes=8)
    finally:
        if old is None:
            os.environ.pop("UDPDK_GATHER_GRID", None)
        else:
            os.environ["UDPDK_GATHER_GRID"] = old
    yield ctx
    ctx.close()


@pytest.mark.parametrize("mode", ["plain", "packed"])
def test_grid_stride(stride_ctx, mode):
    """Two workgroups for 1613 entries: each runs the entry loop four times, the last time with a
    partial workgroup (one) or nothing left (the other)."""
    rng = np.random.default_rng(150)
    fb = Frames(rng, _mixed_specs(rng, 400), RES)
    count = 2 * 256 * 3 + 77
    lane_pkt = rng.integers(0, 400, count)
    if mode == "plain":
        _gather(stride_ctx, fb, lane_pkt, 0, count, slot=2048)
    else:
        _gather(stride_ctx, fb, lane_pkt, 0, count, caps=16 * rng.integers(1, 201, count))
