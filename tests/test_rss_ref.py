"""The tests' own statement of receive-side scaling (tests/rss_util.py: numpy, from the
definitions, importing neither the oracle nor the library) against the oracle's bit-serial one on
the whole key set and on a batch with every frame kind, and against answers derived by hand from
the formula hash_j = XOR_i input_i . key_{i + j} (bits counted MSB first)."""
import json
import os
import socket

import numpy as np
import pytest

import oracle as O
import rss_util as R

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rss_vectors.json")))
KEYS = R.key_set()


def test_key_set():
    names = [n for n, _ in KEYS]
    assert len(KEYS) == 1 + 20 + 3 + 128 + 2 and len(set(names)) == len(names)
    assert len({k for _, k in KEYS}) == len(KEYS) and all(len(k) == 40 for _, k in KEYS)
    for b in range(128):
        k = dict(KEYS)[f"bit{b}"]
        assert sum(bin(x).count("1") for x in k) == 1 and k[b >> 3] == 0x80 >> (b & 7)
    diff = bytes(a ^ b for a, b in zip(R.STD_KEY, R.STD_KEY_BIT127))
    assert diff == bytes(15) + b"\x01" + bytes(24)
    assert R.STD_KEY_BYTE39[:39] == R.STD_KEY[:39] and R.STD_KEY_BYTE39[39] != R.STD_KEY[39]


def test_verification_vectors():
    for v in G["ipv4"]:
        a = socket.inet_aton(v["src"]) + socket.inet_aton(v["dst"])
        p = v["sport"].to_bytes(2, "big") + v["dport"].to_bytes(2, "big")
        assert int(R.toeplitz_ref(R.STD_KEY, np.frombuffer(a, np.uint8))[0]) == int(v["ipv4"], 16)
        assert int(R.toeplitz_ref(R.STD_KEY, np.frombuffer(a + p, np.uint8))[0]) == int(v["ipv4_l4"], 16)


@pytest.mark.parametrize("width", [8, 12])
def test_toeplitz_ref_equals_oracle_on_every_key(width):
    rng = np.random.default_rng(width)
    for name, key in KEYS:
        x = rng.integers(0, 256, (24, width), dtype=np.uint8)
        x[0], x[1] = 0, 0xFF
        got = R.toeplitz_ref(key, x)
        want = [O.toeplitz(key, r.tobytes()) for r in x]
        assert got.tolist() == want, name


def test_rss_ref_equals_oracle_on_every_kind():
    b = R.tuple_frames(6000, 5, size=64, kinds=R.KINDS, gaps=True)
    assert set(b.kind.tolist()) == set(range(len(R.KINDS)))
    rng = np.random.default_rng(1)
    for types in (3, 1, 2, 0):
        for pt in (None, b.ptype):
            reta = rng.integers(0, 11, 256)
            for key in (R.STD_KEY, R.random_keys()[3]):
                want = O.rss(key, types, reta, 11, b.frames, b.frames_bytes, b.offset, b.length, pt)
                got = R.rss_ref(key, types, reta, 11, b, pt)
                for w, g in zip(want, got):
                    assert np.array_equal(w, g), (types, pt is None)


def test_rss_ref_descriptor_rules():
    """Frames out of bounds or shorter than 34 bytes hash to 0; 34-37 bytes take the addresses."""
    b = R.tuple_frames(64, 9, size=64)
    t = R.frame_tuples(b)
    b.length = b.length.copy()
    b.offset = b.offset.copy()
    b.length[:8] = [0, 13, 14, 33, 34, 37, 38, 39]
    b.offset[8] = b.frames_bytes - 63
    b.offset[9] = 0xFFFFFFFF
    h, qo, qp = R.rss_ref(R.STD_KEY, 3, np.arange(128) % 4, 4, b)
    assert h[:4].tolist() == [0, 0, 0, 0] and h[8] == 0 and h[9] == 0
    assert h[4:6].tolist() == R.toeplitz_ref(R.STD_KEY, t[4:6, :8]).tolist()
    assert h[6:8].tolist() == R.toeplitz_ref(R.STD_KEY, t[6:8]).tolist()
    assert h[10:].tolist() == R.toeplitz_ref(R.STD_KEY, t[10:]).tolist()
    want = O.rss(R.STD_KEY, 3, np.arange(128) % 4, 4, b.frames, b.frames_bytes, b.offset, b.length)
    assert np.array_equal(want[0], h) and np.array_equal(want[1], qo) and np.array_equal(want[2], qp)


# ---- known answers derived by hand -----------------------------------------------------------------
def _bits(x: np.ndarray) -> list:
    return [(int(x[i >> 3]) >> (7 - (i & 7))) & 1 for i in range(8 * len(x))]


@pytest.mark.parametrize("width", [8, 12])
def test_single_bit_keys(width):
    """A key with only bit b set has key_{i + j} = 1 exactly when i = b - j, so hash_j =
    input_{b - j} (0 where b - j is no input bit): the hash is the 32 input bits ending at bit b,
    reversed: input bit b lands in the hash's MSB, input bit b - 31 in its LSB."""
    rng = np.random.default_rng(100 + width)
    for b in range(128):
        x = rng.integers(0, 256, width, dtype=np.uint8)
        xb = _bits(x)
        want = 0
        for j in range(32):
            if 0 <= b - j < 8 * width and xb[b - j]:
                want |= 1 << (31 - j)
        key = R.single_bit_key(b)
        assert int(R.toeplitz_ref(key, x)[0]) == want, b
        assert O.toeplitz(key, x.tobytes()) == want, b


def test_single_bit_key_literals():
    """Worked by hand. Input 80 00 00 00 | 00 00 00 00 | 00 00 | 00 01: input bits 0 and 95 set.
    Key bit 0: hash_j = input_{-j}: only j = 0, input bit 0 = 1 -> 0x80000000.
    Key bit 31: hash_j = input_{31 - j}: input bit 0 at j = 31 -> 0x00000001.
    Key bit 95: input bit 95 at j = 0 -> 0x80000000 (input bit 64..94 are clear).
    Key bit 126: i + j = 126 with i <= 95, j <= 31 only at i = 95, j = 31: it reaches only the
    hash's LSB, and only through input bit 95, the destination port's LSB -> 0x00000001.
    Key bit 127: i + j <= 126: reaches nothing -> 0."""
    x = np.array([0x80, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8)
    for b, want in ((0, 0x80000000), (31, 1), (95, 0x80000000), (126, 1), (127, 0), (1, 0x40000000),
                    (96, 0x40000000), (64, 0)):
        assert int(R.toeplitz_ref(R.single_bit_key(b), x)[0]) == want, b
        assert O.toeplitz(R.single_bit_key(b), x.tobytes()) == want, b
    # the same input without the destination port's LSB: key bit 126 gives 0
    y = x.copy()
    y[11] = 0xFE
    assert int(R.toeplitz_ref(R.single_bit_key(126), y)[0]) == 0
    # an 8-byte input: i <= 63, so key bits 95 and above reach nothing; bit 94 only via input bit 63
    z = np.full(8, 0xFF, np.uint8)
    for b in range(95, 128):
        assert int(R.toeplitz_ref(R.single_bit_key(b), z)[0]) == 0
    assert int(R.toeplitz_ref(R.single_bit_key(94), z)[0]) == 1


def test_unreachable_key_bits():
    """Key bit 127 and key bytes 16-39 reach no 12-byte input, key bits 95-127 no 8-byte one:
    keys that differ only there give equal hashes."""
    rng = np.random.default_rng(77)
    x12 = rng.integers(0, 256, (500, 12), dtype=np.uint8)
    x8 = x12[:, :8]
    for key in (R.STD_KEY, R.random_keys()[0], b"\xff" * 40):
        other = bytearray(key)
        other[15] ^= 0x01
        other[16:] = rng.integers(0, 256, 24, dtype=np.uint8).tobytes()
        assert np.array_equal(R.toeplitz_ref(key, x12), R.toeplitz_ref(bytes(other), x12))
        o8 = bytearray(other)
        o8[11] ^= 0x01                                   # bit 95
        o8[12:16] = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
        assert np.array_equal(R.toeplitz_ref(key, x8), R.toeplitz_ref(bytes(o8), x8))
        near = bytearray(key)
        near[15] ^= 0x02                                 # bit 126 does reach: some hash changes
        assert not np.array_equal(R.toeplitz_ref(key, x12), R.toeplitz_ref(bytes(near), x12))
    for k in (R.STD_KEY_BIT127, R.STD_KEY_BYTE39):
        assert np.array_equal(R.toeplitz_ref(k, x12), R.toeplitz_ref(R.STD_KEY, x12))
        assert [O.toeplitz(k, r.tobytes()) for r in x12[:50]] == R.toeplitz_ref(R.STD_KEY, x12[:50]).tolist()


def test_zero_key_and_linearity():
    x = np.random.default_rng(3).integers(0, 256, (200, 12), dtype=np.uint8)
    assert not R.toeplitz_ref(bytes(40), x).any()
    k = R.random_keys()
    kx = bytes(a ^ b for a, b in zip(k[1], k[2]))
    assert np.array_equal(R.toeplitz_ref(kx, x), R.toeplitz_ref(k[1], x) ^ R.toeplitz_ref(k[2], x))
