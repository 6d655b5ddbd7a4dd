"""Receive-side scaling away from the benchmark's one source address and port and its one key:
udpdk_gpu_rss, bit-exact in hash, queue_off and queue_pkt against both the oracle and the tests'
own numpy statement (tests/rss_util.py), on uniformly random tuples with every byte value at every
input position, every frame kind the hash rules tell apart, the whole key set alternating on one
context, redirection tables of every size, frames ending exactly at frames_bytes in an allocation
of frames_bytes + the ABI's tailroom, and the three queue-base forms (fused into rss_hash, one
rss_base workgroup, the three-pass column scan) at their smallest shapes, the form each call took
read from UDPDK_RSS_TRACE."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
import rss_util as R
from udpdk_amd import abi

pytestmark = pytest.mark.gpu

TAIL = abi.FRAMES_TAILROOM


def _upload(ctx, b, ptype=None):
    """Device copies; the frames allocation is exactly frames_bytes + the tailroom, filled 0xFF."""
    buf = np.concatenate([np.asarray(b.frames[:b.frames_bytes], np.uint8), np.full(TAIL, 0xFF, np.uint8)])
    fb = ctx.upload(buf)
    assert fb.nbytes == b.frames_bytes + TAIL
    return abi.RxDeviceBatch(fb, b.frames_bytes, ctx.upload(np.asarray(b.offset, np.uint32)),
                             ctx.upload(np.asarray(b.length, np.uint16)),
                             ctx.upload(np.asarray(ptype, np.uint32)) if ptype is not None else None, len(b.offset))


def _free(db):
    for x in (db.frames, db.offset, db.length, db.ptype):
        if x is not None:
            x.free()


def _reta(rng, size, nq):
    """A random table that uses every queue it can."""
    return rng.permutation(np.arange(size) % nq)


def _want(key, types, reta, nq, b, ptype=None):
    """The oracle's answer, equal to the independent reference's."""
    wo = O.rss(key, types, reta, nq, b.frames, b.frames_bytes, b.offset, b.length, ptype)
    wr = R.rss_ref(key, types, reta, nq, b, ptype)
    for x, y, what in zip(wo, wr, ("hash", "queue_off", "queue_pkt")):
        assert np.array_equal(x, y), f"oracle and reference differ in {what}"
    return wo


def _same(want, got, what=""):
    for x, y, name in zip(want, got, ("hash", "queue_off", "queue_pkt")):
        assert np.array_equal(x, y), f"{name} {what}"


def _run(ctx, db, b, key, types, reta, nq, ptype=None, what=""):
    got = abi.rss_run(ctx, db, abi.rss_conf(nq, reta=reta, key=key, hash_types=types))
    _same(_want(key, types, reta, nq, b, ptype), got, what)
    return got


# ---- 1. spread tuples ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _spread():
    rng = np.random.default_rng(2024)
    t = np.concatenate([rng.integers(0, 256, (8192, 12), dtype=np.uint8), R.sweep_tuples(7)])
    return R.tuple_frames(8192 + 3072, 2024, size=64, gaps=True, tuples=t), _reta(rng, 512, 64)


@pytest.mark.parametrize("types", [3, 1, 2, 0])
def test_spread_tuples(gpu_ctx, types):
    """8192 frames with uniformly random addresses and ports, then the 3072 frames that put every
    byte value at every one of the 12 input positions, 0-3 bytes between the frames; 64 queues,
    every one of them non-empty under types 3."""
    b, reta = _spread()
    assert len(set((b.offset & 3).tolist())) == 4
    t = R.frame_tuples(b)[8192:]
    for p in range(12):
        assert sorted(t[256 * p:256 * p + 256, p].tolist()) == list(range(256))
    db = _upload(gpu_ctx, b)
    h, qo, _ = _run(gpu_ctx, db, b, R.STD_KEY, types, reta, 64)
    _free(db)
    if types == 3:
        assert np.all(np.diff(qo.astype(np.int64)) > 0)
        assert np.array_equal(h, R.toeplitz_ref(R.STD_KEY, R.frame_tuples(b)))
    if types == 0:
        assert not h.any() and qo[int(reta[0]) + 1] - qo[int(reta[0])] == b.n


# ---- 2. kinds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("types", [3, 1, 2, 0])
def test_kinds(gpu_ctx, types):
    """200 frames of every kind, the ptype array given and derived: the hash is the Toeplitz
    hash of the width the kind names (12 bytes, 8 bytes, or nothing), whatever else the frame holds."""
    b = R.tuple_frames(200 * len(R.KINDS), 77, size=64, kinds=R.KINDS, gaps=True)
    key = R.random_keys()[7]
    reta = _reta(np.random.default_rng(types), 128, 8)
    t = R.frame_tuples(b)
    db = {True: _upload(gpu_ctx, b, b.ptype), False: _upload(gpu_ctx, b)}
    for given, widths in ((True, R.WIDTH_GIVEN), (False, R.WIDTH_DERIVED)):
        h, _, _ = _run(gpu_ctx, db[given], b, key, types, reta, 8, b.ptype if given else None, f"given {given}")
        for ki, name in enumerate(R.KINDS):
            sel = b.kind == ki
            assert sel.sum() == 200, name                      # the batch cannot lose a kind
            w = widths[name]
            w = w if (w == 12 and types & 2) else (8 if w and types & 1 else 0)
            want = R.toeplitz_ref(key, t[sel][:, :w]) if w else np.zeros(200, np.uint32)
            assert np.array_equal(h[sel], want), (name, given)
            assert (np.count_nonzero(h[sel]) >= 199) == (w != 0), (name, given)
    for d in db.values():
        _free(d)


# ---- 3. keys ---------------------------------------------------------------------------------------
def _key_sweep(ctx, names):
    """The named keys of the key set over one 512-frame batch on one context, the standard key
    again after every fifth, with reta_size, n_queues and hash_types changing between the calls."""
    b = R.tuple_frames(512, 99, size=64, gaps=True)
    keys = dict(R.key_set())
    order = []
    for i, nm in enumerate(names):
        order.append(nm)
        if i % 5 == 4:
            order.append("std")
    db = _upload(ctx, b)
    rng = np.random.default_rng(len(names))
    std = []
    for i, nm in enumerate(order):
        nq = (64, 1, 7, 16, 3, 33)[i % 6]
        size = 1 << (i % 10)
        types = (3, 3, 1, 2, 3, 0, 3)[i % 7]
        got = _run(ctx, db, b, keys[nm], types, _reta(rng, size, nq), nq, None, f"{nm} at {i}")
        if nm == "std" and types == 3:
            std.append(got[0])
    _free(db)
    assert len(std) >= 2 and all(np.array_equal(std[0], s) for s in std)


def test_keys(gpu_ctx):
    """The standard, random, all-ones, all-zero, 6d5a and irrelevant-bit keys."""
    _key_sweep(gpu_ctx, [n for n, _ in R.key_set() if not n.startswith("bit")])


@pytest.mark.parametrize("half", [0, 1])
def test_single_bit_keys(gpu_ctx, half):
    """Key bits 0-63 and 64-127, one at a time: each key window in each table row on its own."""
    _key_sweep(gpu_ctx, [f"bit{b}" for b in range(64 * half, 64 * half + 64)])


def test_key_properties_without_a_reference(gpu_ctx):
    """The GPU against itself: the hash is linear in the key (hashes under k1 ^ k2 = the XOR of
    the hashes under k1 and k2), and key bit 127 and byte 39 reach no input bit."""
    b = R.tuple_frames(512, 98, size=64, gaps=True)
    db = _upload(gpu_ctx, b)
    reta = _reta(np.random.default_rng(8), 256, 64)
    run = lambda key: abi.rss_run(gpu_ctx, db, abi.rss_conf(64, reta=reta, key=key))
    ks = R.random_keys()
    for i in range(5):
        k1, k2 = ks[2 * i], ks[2 * i + 1]
        hx = run(bytes(x ^ y for x, y in zip(k1, k2)))[0]
        assert np.array_equal(hx, run(k1)[0] ^ run(k2)[0]) and hx.any()
    std = run(R.STD_KEY)
    for k in (R.STD_KEY_BIT127, R.STD_KEY_BYTE39):
        _same(std, run(k))
    _free(db)


# ---- 4. redirection tables -------------------------------------------------------------------------
def test_reta_sizes(gpu_ctx):
    """Every power of two from 1 to 512 entries, 64 queues."""
    b = R.tuple_frames(3000, 55, size=64, gaps=True)
    db = _upload(gpu_ctx, b)
    rng = np.random.default_rng(55)
    for lg in list(range(10)) + [0, 9, 3]:
        _run(gpu_ctx, db, b, R.STD_KEY, 3, rng.integers(0, 64, 1 << lg), 64, None, f"reta_size {1 << lg}")
    _free(db)


def test_reta_sparse_and_single_queue(gpu_ctx):
    """64 queues of which the table uses 0, 31 and 63 (the empty queues between them start where
    their neighbour does), and the all-zero key, under which every frame lands in reta[0] = 63."""
    b = R.tuple_frames(3000, 56, size=64, gaps=True)
    db = _upload(gpu_ctx, b)
    rng = np.random.default_rng(56)
    reta = np.array([0, 31, 63])[rng.integers(0, 3, 512)]
    _, qo, _ = _run(gpu_ctx, db, b, R.STD_KEY, 3, reta, 64)
    cnt = np.diff(qo.astype(np.int64))
    assert set(np.flatnonzero(cnt).tolist()) == {0, 31, 63}
    assert len(set(qo[1:32].tolist())) == 1 and len(set(qo[32:64].tolist())) == 1 and qo[64] == b.n
    reta = rng.integers(0, 63, 512)
    reta[0] = 63
    h, qo, qp = _run(gpu_ctx, db, b, bytes(40), 3, reta, 64)
    assert not h.any() and not qo[:64].any() and qo[64] == b.n and np.array_equal(qp, np.arange(b.n))
    _free(db)


def test_reta_entries_past_reta_size_are_never_read(gpu_ctx):
    """A configuration whose table entries past reta_size name queues that do not exist."""
    b = R.tuple_frames(3000, 57, size=64, gaps=True)
    db = _upload(gpu_ctx, b)
    reta = _reta(np.random.default_rng(57), 8, 4)
    cf = abi.rss_conf(4, reta=reta)
    for i in range(8, 512):
        cf.reta[i] = 0xFFFF
    assert cf.reta_size == 8
    assert abi.lib().udpdk_gpu_rss_config(gpu_ctx.handle, C.byref(cf)) == 0
    got = abi.rss_run(gpu_ctx, db, cf)
    _same(_want(R.STD_KEY, 3, reta, 4, b), got)
    assert np.all(np.diff(got[1].astype(np.int64)) > 0)
    _free(db)


# ---- 5. the load window's edges --------------------------------------------------------------------
EDGE_LENS = (34, 35, 37, 38, 39, 42)


def _edge_batch(r, length, frag, first, seed):
    """frames_bytes = 180 + r bytes of 0xFF holding a 64-byte frame at offset `first`, one at 72,
    and a `length`-byte frame ending exactly at frames_bytes; the descriptors around them."""
    rng = np.random.default_rng(seed)
    fb = 180 + r
    fr = np.full(fb, 0xFF, np.uint8)
    starts = [first, 72, fb - length]
    tup = rng.integers(0, 256, (3, 12), dtype=np.uint8)
    for o, ln, t in zip(starts, (64, 64, length), tup):
        f = rng.integers(0, 256, ln, dtype=np.uint8)
        f[12], f[13], f[14], f[20], f[21], f[23] = 0x08, 0x00, 0x45, 0, 0, 17
        k = min(12, ln - 26)                        # a 34-byte frame holds the addresses only
        f[26:26 + k] = t[:k]
        fr[o:o + ln] = f
    if frag:
        fr[fb - length + 20] = 0x20
    desc = [(first, 64), (72, 64), (fb - length, length),
            (fb - length + 1, length),              # the same frame one byte further: past the end
            (0xFFFFFFFF, 65535), (0xFFFFFFF0, 34), (fb - 33, 34),
            (72, 33),                               # too short, inside the buffer
            (72, 64), (fb - length, length)]        # two descriptors alias one frame
    off = np.array([d[0] for d in desc], np.uint32)
    ln = np.array([d[1] for d in desc], np.uint16)
    return SimpleNamespace(frames=fr, offset=off, length=ln, frames_bytes=fb, n=len(desc)), tup


@pytest.mark.parametrize("r", range(4))
def test_window_edges(gpu_ctx, r):
    """The last frame of 34-42 bytes ends exactly at frames_bytes, for this residue of frames_bytes
    mod 4, as UDP and as a fragment, the first frame at offset 0-3; allocation = frames_bytes + 16
    bytes of 0xFF: the two 16-byte loads of the last frame reach up to 10 bytes past frames_bytes."""
    key = R.random_keys()[9]
    reta = _reta(np.random.default_rng(r), 64, 5)
    firsts = set()
    for li, length in enumerate(EDGE_LENS):
        for frag in (False, True):
            first = (li + r + int(frag)) % 4
            firsts.add(first)
            b, tup = _edge_batch(r, length, frag, first, 1000 * r + 10 * li + frag)
            assert b.frames_bytes % 4 == r and int(b.offset[2]) + length == b.frames_bytes
            db = _upload(gpu_ctx, b)
            h, _, _ = _run(gpu_ctx, db, b, key, 3, reta, 5, None, f"len {length} frag {frag}")
            _free(db)
            width = 12 if length >= 38 and not frag else 8
            assert h[0] == R.toeplitz_ref(key, tup[0])[0] and h[1] == R.toeplitz_ref(key, tup[1])[0]
            assert h[2] == R.toeplitz_ref(key, tup[2][:width])[0] != 0
            assert h[3:8].tolist() == [0] * 5
            assert h[8] == h[1] and h[9] == h[2]
    assert firsts == {0, 1, 2, 3}


# ---- 6. the queue-base forms at their smallest shapes ----------------------------------------------
FORMS = [
    # n, queues, tiles, form
    (131072, 64, 128, "fused"),      # 128 x 64 = 8192: the fused scan's largest input, rows of 128
    (131073, 64, 129, "one"),        # first past the fused bound, the last tile holds 1 frame
    (300001, 37, 293, "one"),        # odd rows, 10 841 entries = 1 mod 4: the partial 16-byte load and store
    (524288, 64, 512, "one"),        # 32 768 entries: every rss_base thread's 32 entries live
    (524289, 64, 513, "3pass"),      # 17 chunks, the last one tile of one frame
    (540001, 63, 528, "3pass"),      # odd queue count, half-full last chunk
    (1126000, 30, 1100, "3pass"),    # 35 chunks: rx_scan_top's second 32-chunk batch, 3 live
]


@functools.lru_cache(maxsize=2)
def _form_case(n, nq):
    b = R.tuple_frames(n, n, size=64)
    reta = _reta(np.random.default_rng(n), 512, nq)
    return b, reta, _want(R.STD_KEY, 3, reta, nq, b)


def _form_run(ctx, capfd, n, nq, tiles, form):
    b, reta, want = _form_case(n, nq)
    db = _upload(ctx, b)
    capfd.readouterr()
    got = abi.rss_run(ctx, db, abi.rss_conf(nq, reta=reta))
    err = capfd.readouterr().err
    _free(db)
    lines = [ln for ln in err.splitlines() if ln.startswith("rss tiles ")]
    assert lines == [f"rss tiles {tiles} queues {nq} base {form}"], err
    _same(want, got)
    assert got[1][-1] == n and np.all(np.diff(got[1].astype(np.int64)) > 0)      # every queue fills


@pytest.mark.parametrize("n,nq,tiles,form", FORMS, ids=[f"{f[0]}x{f[1]}-{f[3]}" for f in FORMS])
def test_base_forms(gpu_ctx, monkeypatch, capfd, n, nq, tiles, form):
    """Each queue-base form at the smallest shapes that reach it, on both sides of the 8192- and
    32 768-entry bounds; UDPDK_RSS_TRACE names the form the call took."""
    assert tiles == -(-n // 1024)
    assert form == ("fused" if tiles * nq <= 8192 else "one" if tiles * nq <= 32768 else "3pass")
    monkeypatch.setenv("UDPDK_RSS_TRACE", "1")
    monkeypatch.delenv("UDPDK_RSS_FUSE", raising=False)
    _form_run(gpu_ctx, capfd, n, nq, tiles, form)


@pytest.mark.parametrize("n,nq,tiles", [(131072, 64, 128), (40000, 64, 40)])
def test_fused_shapes_without_fusing(gpu_ctx, monkeypatch, capfd, n, nq, tiles):
    """UDPDK_RSS_FUSE=0 sends the fused shapes to the rss_base launch."""
    monkeypatch.setenv("UDPDK_RSS_TRACE", "1")
    monkeypatch.setenv("UDPDK_RSS_FUSE", "0")
    _form_run(gpu_ctx, capfd, n, nq, tiles, "one")
    monkeypatch.delenv("UDPDK_RSS_FUSE")
    _form_run(gpu_ctx, capfd, n, nq, tiles, "fused")
