"""udpdk_gpu_tx_build_neigh: frames byte for byte against the oracle's (what test_gpu_tx.py and
test_gpu_tx_cksum.py compare with: O.tx_frame, the RFC 768 sum of tx_cksum_util.py, O.tx_fragment) with bytes
0-5 of every frame, every fragment included, replaced by the datagram's own MAC. The whole output buffer is
compared, a guard past frames_bytes included."""
import ctypes as C

import numpy as np
import pytest

import tx_cksum_util as U
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
SRC_IP = abi.raw_ip("172.31.100.2")
SLOTS = [(0, 10000, 1), (abi.raw_ip("10.1.2.3"), 5353, 1), (abi.raw_ip("10.9.9.9"), 7, 0)]
GUARD = 4096
LENS = [0, 18, 38, 39, 1472, 1473, 3000]
N = 130


def _span(L, mtu):
    if mtu and L + 42 > mtu:
        return L + 8 + 34 * -(-(L + 8) // (mtu - 20))
    return L + 42


class Batch:
    """130 datagrams of the seven lengths mixed, each with a MAC of its own; payloads and frames back to back
    from odd starts, so frame ends share 16-byte chunks. Waves 0 and 1 mix both paths, the tail of 2 datagrams
    is a wave of its own; `small` makes the first wave all-small (tx_small) instead."""

    def __init__(self, seed, mtu, small=False):
        rng = np.random.default_rng(seed)
        self.mtu = mtu
        self.lens = np.array([LENS[k] for k in rng.integers(0, len(LENS), N)], np.int64)
        self.lens[:len(LENS)] = LENS
        if small:
            self.lens[:64] = rng.choice([0, 18, 38], 64)
        self.po = np.concatenate([[0], np.cumsum(self.lens + np.arange(N) % 3)[:-1]])
        self.payload_bytes = int(self.po[-1] + self.lens[-1])
        self.pay = np.concatenate([rng.integers(1, 255, self.payload_bytes, dtype=np.uint8),
                                   np.full(abi.FRAMES_TAILROOM, 0xA5, np.uint8)])
        spans = np.array([_span(int(L), mtu) for L in self.lens])
        self.fo = 5 + np.concatenate([[0], np.cumsum(spans)[:-1]])
        self.frames_bytes = int(self.fo[-1] + spans[-1])
        self.sock = rng.integers(0, len(SLOTS), N).astype(np.int32)
        self.dip = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
        self.dport = rng.integers(0, 65536, N).astype(np.uint16)
        self.macs = [bytes([0x02, 0x10 + (i >> 8), i & 0xFF, 0xC0 ^ i & 0xFF, 0x5A, 0x01 + i % 250]) for i in range(N)]
        assert len(set(self.macs)) == N
        self.dmac = np.frombuffer(b"".join(m + b"\xDE\xAD" for m in self.macs), np.uint32).copy()   # (bits 48-63 are ignored)

    def image(self, cksum, macs=None):
        want = np.full(self.frames_bytes + GUARD, 0xEE, np.uint8)
        for i in range(N):
            if self.sock[i] < 0:
                continue
            p = self.pay[self.po[i]:self.po[i] + self.lens[i]].tobytes()
            blob, frames = U.expected(SRC_MAC, DST_MAC, SRC_IP, SLOTS[self.sock[i]], int(self.dip[i]), int(self.dport[i]),
                                      p, self.mtu, cksum)
            blob, pos = bytearray(blob), 0
            assert len(blob) == _span(int(self.lens[i]), self.mtu)
            for f in frames:
                if macs is not None:
                    blob[pos:pos + 6] = macs[i]
                pos += len(f)
            want[self.fo[i]:self.fo[i] + len(blob)] = np.frombuffer(bytes(blob), np.uint8)
        return want


def _run(ctx, t, flags, dmac=True, entry="neigh"):
    ctx.upload_snapshot(abi.snapshot_from_lists({}, 1, slots=SLOTS))
    bufs = [ctx.upload(t.pay), ctx.upload(t.po.astype(np.uint32)), ctx.upload(t.lens.astype(np.uint16)),
            ctx.upload(t.sock), ctx.upload(t.dip), ctx.upload(t.dport), ctx.upload(t.fo.astype(np.uint32)),
            ctx.upload(t.dmac)]
    size = t.frames_bytes + GUARD
    out = ctx.alloc(size)
    abi.lib().udpdk_gpu_memset(ctx.handle, C.c_void_p(out.ptr), 0xEE, size)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*SRC_MAC), (C.c_uint8 * 6)(*DST_MAC), SRC_IP)
    bt = abi.TxBatch(bufs[0].ptr, t.payload_bytes, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, N)
    ot = abi.TxOut(out.ptr, t.frames_bytes, bufs[6].ptr)
    if entry == "neigh":
        rc = abi.lib().udpdk_gpu_tx_build_neigh(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot), t.mtu or 0, flags,
                                                C.c_void_p(bufs[7].ptr) if dmac else None)
    else:
        rc = abi.lib().udpdk_gpu_tx_build_flags(ctx.handle, C.byref(cfg), C.byref(bt), C.byref(ot), t.mtu or 0, flags)
    assert rc == 0
    res = ctx.download(out, np.uint8, size)
    for b in bufs + [out]:
        b.free()
    return res


def _same(t, res, want):
    bad = np.nonzero(res != want)[0]
    if bad.size:
        b = int(bad[0])
        i = int(np.searchsorted(t.fo, b, "right")) - 1
        raise AssertionError(f"{bad.size} bytes differ, the first at {b}: got {res[b]:#04x} want {want[b]:#04x}, "
                             f"datagram {i} (len {t.lens[i]}, frame_off {t.fo[i]}, byte {b - t.fo[i]})")


@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM], ids=["plain", "cksum"])
@pytest.mark.parametrize("mtu", [0, 1500])
@pytest.mark.parametrize("small", [False, True], ids=["mixed", "small_wave"])
def test_every_frame_carries_its_datagrams_mac(gpu_ctx, mtu, flags, small):
    t = Batch(400 + mtu + flags, mtu, small)
    if mtu:
        assert (t.lens == 3000).any() and (t.lens == 1473).any()      # two and three fragments each
    t.sock[[3, 64, 129]] = -1                                         # nothing is written for these
    _same(t, _run(gpu_ctx, t, flags), t.image(bool(flags), t.macs))


@pytest.mark.parametrize("flags", [0, abi.TX_UDP_CKSUM], ids=["plain", "cksum"])
@pytest.mark.parametrize("mtu", [0, 1500])
def test_null_macs_is_tx_build_flags(gpu_ctx, mtu, flags):
    t = Batch(500 + mtu + flags, mtu)
    res = _run(gpu_ctx, t, flags, dmac=False)
    _same(t, res, t.image(bool(flags)))
    assert np.array_equal(res, _run(gpu_ctx, t, flags, entry="flags"))


def test_misaligned_mac_array_is_rejected(gpu_ctx):
    t = Batch(1, 0)
    buf = gpu_ctx.upload(t.dmac)
    cfg = abi.TxConfig((C.c_uint8 * 6)(*SRC_MAC), (C.c_uint8 * 6)(*DST_MAC), SRC_IP)
    rc = abi.lib().udpdk_gpu_tx_build_neigh(gpu_ctx.handle, C.byref(cfg), C.byref(abi.TxBatch()), C.byref(abi.TxOut()),
                                            0, 0, C.c_void_p(buf.ptr + 4))
    buf.free()
    assert rc == -22
