"""Receive-side scaling restated in numpy, independent of the oracle and of the library (neither is
imported here): the Toeplitz hash straight from its definition, udpdk_gpu_rss's per-frame rules
and per-queue lists from rx_rss.hip's header comment, the key set the CPU and GPU tests share, and
a frame builder that spreads the hash input (random addresses and ports; optionally every frame
kind the rules tell apart and gaps between the frames).

Frame layout (fixed offsets, as the kernel documents): ether_type [12, 14), IPv4 version/IHL 14,
flags + fragment offset [20, 22), protocol 23, source address [26, 30), destination address
[30, 34), source port [34, 36), destination port [36, 38)."""
import json
import os
from types import SimpleNamespace

import numpy as np

_G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rss_vectors.json")))
STD_KEY = bytes.fromhex(_G["key"])


# ---- the hash ------------------------------------------------------------------------------------
def toeplitz_ref(key: bytes, inputs) -> np.ndarray:
    """Toeplitz hashes of the rows of inputs (uint8 [n, L], L <= 36) under a 40-byte key.
    Key bit b and input bit i are counted MSB first from byte 0, hash bit j from the hash's MSB:
    hash_j = XOR_i input_i . key_{i + j}."""
    x = np.ascontiguousarray(inputs, np.uint8)
    if x.ndim == 1:
        x = x[None, :]
    n, L = x.shape
    assert len(key) == 40 and 8 * L + 31 <= 320
    kb = np.unpackbits(np.frombuffer(bytes(key), np.uint8)).astype(np.float32)      # key_b
    m = kb[np.arange(8 * L)[:, None] + np.arange(32)[None, :]]                      # m[i, j] = key_{i + j}
    w = (np.uint64(1) << np.arange(31, -1, -1, dtype=np.uint64))                    # hash bit j -> value
    out = np.zeros(n, np.uint32)
    for r0 in range(0, n, 1 << 16):
        xb = np.unpackbits(x[r0:r0 + (1 << 16)], axis=1).astype(np.float32)         # input_i
        par = (xb @ m).astype(np.uint64) & np.uint64(1)                             # sums <= 288: exact
        out[r0:r0 + (1 << 16)] = (par * w).sum(1).astype(np.uint32)
    return out


def rss_ref(key: bytes, types: int, reta, n_queues: int, batch, ptype=None):
    """-> (hash u32[n], queue_off u32[n_queues + 1], queue_pkt u32[n]) for batch (.frames,
    .frames_bytes, .offset, .length) as udpdk_gpu_rss defines them:
      * a frame is hashed only if it lies inside frames_bytes and has at least 34 bytes,
      * and its ptype (given, else 0x211 for ether_type 0x0800 and 0x1 otherwise) has bit 0x10;
      * unfragmented (flags/offset & 0x3FFF == 0) UDP of at least 38 bytes: the 12 bytes [26, 38)
        when types has 2; else the 8 bytes [26, 34) when types has 1; else hash 0;
      * queue = reta[hash & (len(reta) - 1)]; queue q's list holds its frames in arrival order."""
    fr = np.asarray(batch.frames, np.uint8)
    off = np.asarray(batch.offset).astype(np.int64)
    ln = np.asarray(batch.length).astype(np.int64)
    reta = np.asarray(reta).astype(np.int64)
    n = len(off)
    h = np.zeros(n, np.uint32)
    ok = (off + ln <= int(batch.frames_bytes)) & (ln >= 34)
    idx = np.flatnonzero(ok)
    o = off[idx]
    if ptype is None:
        pt = np.where((fr[o + 12] == 0x08) & (fr[o + 13] == 0x00), 0x211, 0x1)
    else:
        pt = np.asarray(ptype).astype(np.int64)[idx]
    gate = (pt & 0x10) != 0
    ff = (fr[o + 20].astype(np.int64) << 8) | fr[o + 21]
    udp4 = gate & ((ff & 0x3FFF) == 0) & (fr[o + 23] == 17) & (ln[idx] >= 38) & bool(types & 2)
    ip2 = gate & ~udp4 & bool(types & 1)
    for sel, width in ((udp4, 12), (ip2, 8)):
        if sel.any():
            h[idx[sel]] = toeplitz_ref(key, fr[o[sel][:, None] + 26 + np.arange(width)[None, :]])
    q = reta[h.astype(np.int64) & (len(reta) - 1)]
    assert q.size == 0 or (q.min() >= 0 and q.max() < n_queues)
    queue_off = np.zeros(n_queues + 1, np.uint32)
    queue_off[1:] = np.cumsum(np.bincount(q, minlength=n_queues))
    queue_pkt = np.argsort(q, kind="stable").astype(np.uint32)
    return h, queue_off, queue_pkt


# ---- keys ----------------------------------------------------------------------------------------
def _flip(key: bytes, bit: int) -> bytes:
    k = bytearray(key)
    k[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(k)


def single_bit_key(bit: int) -> bytes:
    return _flip(bytes(40), bit)


STD_KEY_BIT127 = _flip(STD_KEY, 127)                       # differs in the first bit no 12-byte input reaches
STD_KEY_BYTE39 = STD_KEY[:39] + bytes([STD_KEY[39] ^ 0xFF])


def random_keys(n: int = 20, seed: int = 0x4B4559) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, 40, dtype=np.uint8).tobytes() for _ in range(n)]


def key_set() -> list:
    """[(name, key)]: the standard key, 20 seeded random keys, all-ones, all-zero, 6d 5a repeated,
    the 128 single-bit keys for bits 0-127, and the standard key with bit 127 / byte 39 changed."""
    ks = [("std", STD_KEY)]
    ks += [(f"rand{i}", k) for i, k in enumerate(random_keys())]
    ks += [("ones", b"\xff" * 40), ("zero", bytes(40)), ("6d5a", b"\x6d\x5a" * 20)]
    ks += [(f"bit{b}", single_bit_key(b)) for b in range(128)]
    ks += [("std^bit127", STD_KEY_BIT127), ("std^byte39", STD_KEY_BYTE39)]
    return ks


# ---- frames --------------------------------------------------------------------------------------
KINDS = ("udp", "udp_df", "mf", "fragoff", "tcp", "icmp", "noip", "noip_pt211", "ip_pt1", "pt91", "ihl6")
# kind -> bytes of hash input with types 3 when the ptype array is given / when it is derived
WIDTH_GIVEN = {"udp": 12, "udp_df": 12, "mf": 8, "fragoff": 8, "tcp": 8, "icmp": 8, "noip": 0,
               "noip_pt211": 12, "ip_pt1": 0, "pt91": 12, "ihl6": 12}
WIDTH_DERIVED = dict(WIDTH_GIVEN, noip_pt211=0, ip_pt1=12)


def sweep_tuples(seed: int) -> np.ndarray:
    """uint8 [3072, 12]: row 256 p + v has byte value v at input position p, the rest random."""
    t = np.random.default_rng(seed).integers(0, 256, (3072, 12), dtype=np.uint8)
    k = np.arange(3072)
    t[k, k // 256] = k % 256
    return t


def tuple_frames(n: int, seed: int, size=64, kinds=None, gaps: bool = False, tuples=None, fill=None):
    """n frames of `size` bytes (an int or one per frame, >= 38) with uniformly random source and
    destination addresses and ports (or the rows of tuples, uint8 [n, 12]), headers only: RSS reads
    no checksum. Unfragmented IPv4 UDP unless kinds names some of KINDS, which are then dealt
    round-robin in a seeded random order; gaps puts 0-3 bytes between the frames. Every other byte
    is random (or `fill`). Returns .frames (exactly frames_bytes long), .offset, .length,
    .frames_bytes, .n, .ptype (what a driver would report: 0x211 for ether_type IPv4, 0x1
    otherwise, and the kind's own value for the three ptype kinds) and .kind (indices into KINDS)."""
    rng = np.random.default_rng(seed)
    sizes = np.broadcast_to(np.asarray(size, np.int64), (n,)).copy()
    assert n > 0 and sizes.min() >= 38 and sizes.max() <= 65535
    gap = rng.integers(0, 4, n) if gaps else np.zeros(n, np.int64)
    off = np.cumsum(gap + np.concatenate(([0], sizes[:-1])))
    total = int(off[-1] + sizes[-1])
    if fill is None:
        fr = rng.integers(0, 256, total, dtype=np.uint8)
    else:
        fr = np.full(total, fill, np.uint8)
        hdr = off[:, None] + np.arange(38)[None, :]
        fr[hdr] = rng.integers(0, 256, (n, 38), dtype=np.uint8)
    kind = np.zeros(n, np.int64)
    if kinds:
        ki = np.array([KINDS.index(k) for k in kinds])
        kind = ki[np.arange(n) % len(ki)][rng.permutation(n)]
    is_ = lambda name: kind == KINDS.index(name)
    fr[off + 12], fr[off + 13], fr[off + 14] = 0x08, 0x00, 0x45
    fr[off + 20], fr[off + 21], fr[off + 23] = 0, 0, 17
    if tuples is not None:
        fr[off[:, None] + 26 + np.arange(12)[None, :]] = np.asarray(tuples, np.uint8)
    fr[off[is_("udp_df")] + 20] = 0x40
    fr[off[is_("mf")] + 20] = 0x20
    k = is_("fragoff")
    fo = rng.integers(1, 0x2000, int(k.sum()))                  # 13-bit offset != 0, MF on every other
    fo |= (np.arange(len(fo)) & 1) << 13
    fr[off[k] + 20], fr[off[k] + 21] = fo >> 8, fo & 0xFF
    fr[off[is_("tcp")] + 23] = 6
    fr[off[is_("icmp")] + 23] = 1
    k = is_("noip") | is_("noip_pt211")
    fr[off[k] + 12], fr[off[k] + 13] = 0x86, 0xDD
    fr[off[is_("ihl6")] + 14] = 0x46
    ptype = np.where(k, 0x1, 0x211).astype(np.uint32)
    ptype[is_("noip_pt211")] = 0x211
    ptype[is_("ip_pt1")] = 0x1
    ptype[is_("pt91")] = 0x91
    return SimpleNamespace(frames=fr, offset=off.astype(np.uint32), length=sizes.astype(np.uint16),
                           frames_bytes=total, n=n, ptype=ptype, kind=kind)


def frame_tuples(b, width: int = 12) -> np.ndarray:
    """uint8 [n, width]: bytes [26, 26 + width) of every frame of a tuple_frames batch."""
    return b.frames[b.offset.astype(np.int64)[:, None] + 26 + np.arange(width)[None, :]]
