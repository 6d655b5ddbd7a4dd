"""The host's statement of the RSS hash (udpdk_amd/csrc/rss_host.h: the key-window table that
udpdk_gpu_rss_config uploads and the per-frame hash behind [gpu] dispatch = rss), checked without a
GPU: build/rss_host_check (tools/rss_host_check.c: both functions behind a main()) prints the hash
of a row `key types ptype frame`, compared with tests/rss_util.py's independent reference.

UDPDK_RSS_HOST_CHECK names another build of the program to run instead (`make rss-asan` gives
build/rss_host_check_asan, the same source under the address and undefined-behaviour sanitizers:
a stand-alone host binary)."""
import os
import subprocess

import numpy as np
import pytest

import rss_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.environ.get("UDPDK_RSS_HOST_CHECK") or os.path.join(ROOT, "build", "rss_host_check")


@pytest.fixture(scope="module")
def check():
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/rss_host_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)

    def run(rows):
        text = "\n".join(f"{key.hex()} {types} {'-' if pt is None else hex(pt)} {bytes(fr).hex()}"
                         for key, types, pt, fr in rows) + "\n"
        out = subprocess.run([CHECK], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(rows), out.stdout[-500:]
        return np.array([int(x, 16) for x in lines], np.uint32)
    return run


def _frames(tuples: np.ndarray, seed: int) -> np.ndarray:
    """uint8 [n, 38]: unfragmented IPv4 UDP headers around the given 12-byte hash inputs."""
    f = np.random.default_rng(seed).integers(0, 256, (len(tuples), 38), dtype=np.uint8)
    f[:, 12], f[:, 13], f[:, 14], f[:, 20], f[:, 21], f[:, 23] = 0x08, 0x00, 0x45, 0, 0, 17
    f[:, 26:38] = tuples
    return f


def test_every_key(check):
    """Every key of the key set on random tuples, 4-tuple (types 3) and 2-tuple (types 1)."""
    rng = np.random.default_rng(11)
    rows, want = [], []
    for name, key in R.key_set():
        t = rng.integers(0, 256, (16, 12), dtype=np.uint8)
        t[0], t[1] = 0, 0xFF
        for types, width in ((3, 12), (1, 8)):
            rows += [(key, types, None, f) for f in _frames(t, 1)]
            want.append(R.toeplitz_ref(key, t[:, :width]))
    got = check(rows)
    assert np.array_equal(got, np.concatenate(want))
    zero = [i for i, r in enumerate(rows) if r[0] == bytes(40)]
    assert len(zero) == 32 and not got[zero].any()


@pytest.mark.parametrize("k", range(4))
def test_every_byte_at_every_position(check, k):
    """All 3072 (position, byte value) pairs of the 12 input bytes, the other bytes random: every
    entry of the 12 x 256 table, under the standard key and three random keys."""
    key = ([R.STD_KEY] + R.random_keys()[:3])[k]
    t = R.sweep_tuples(20 + k)
    for p in range(12):
        assert sorted(t[256 * p:256 * p + 256, p].tolist()) == list(range(256))
    got = check([(key, 3, None, f) for f in _frames(t, 2)])
    assert np.array_equal(got, R.toeplitz_ref(key, t))
    got = check([(key, 1, None, f) for f in _frames(t, 2)])
    assert np.array_equal(got, R.toeplitz_ref(key, t[:, :8]))


@pytest.mark.parametrize("types", [3, 1, 2, 0])
def test_every_kind(check, types):
    """Every frame kind, ptype given and derived: rss_ref's hash, and the input width the kind names."""
    b = R.tuple_frames(1100, 31, size=64, kinds=R.KINDS)
    key = R.random_keys()[5]
    frames = [b.frames[o:o + 64] for o in b.offset.astype(np.int64)]
    for given, widths in ((True, R.WIDTH_GIVEN), (False, R.WIDTH_DERIVED)):
        pt = b.ptype if given else None
        got = check([(key, types, int(b.ptype[i]) if given else None, f) for i, f in enumerate(frames)])
        want, _, _ = R.rss_ref(key, types, [0], 1, b, pt)
        assert np.array_equal(got, want)
        t = R.frame_tuples(b)
        for ki, name in enumerate(R.KINDS):
            sel = b.kind == ki
            assert sel.sum() == 100
            w = widths[name]
            w = w if (w == 12 and types & 2) else (8 if w and types & 1 else 0)
            exp = R.toeplitz_ref(key, t[sel][:, :w]) if w else np.zeros(100, np.uint32)
            assert np.array_equal(got[sel], exp), (name, given)


@pytest.mark.parametrize("types", [3, 1, 2, 0])
def test_lengths(check, types):
    """Lengths 0, 13, 14, 33 hash to 0; 34 and 37 take the addresses only (UDP or not); 38 and 39
    the ports too. Each frame is handed over in an allocation of exactly its length."""
    key = R.STD_KEY
    t = np.random.default_rng(5).integers(0, 256, (8, 12), dtype=np.uint8)
    full = _frames(t, 3)
    full = np.concatenate([full, np.zeros((8, 2), np.uint8)], axis=1)
    lens = [0, 13, 14, 33, 34, 37, 38, 39]
    for pt in (None, 0x211):
        got = check([(key, types, pt, full[i, :n]) for i, n in enumerate(lens)])
        want = np.zeros(8, np.uint32)
        if types & 1:
            want[4:6] = R.toeplitz_ref(key, t[4:6, :8])
        if types & 2:
            want[6:8] = R.toeplitz_ref(key, t[6:8])
        elif types & 1:
            want[6:8] = R.toeplitz_ref(key, t[6:8, :8])
        assert np.array_equal(got, want), pt
    # a short frame whose ptype is given never has its ether_type read
    assert check([(key, 3, 0x211, full[0, :12])])[0] == 0
