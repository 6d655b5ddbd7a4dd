"""The memory policy of rx_classify's streams (rx_common.h: `nt` beside `sc1` on the fused form's
verdict-word and lane-entry stores, `nt` on the long-frame form's frame loads) never changes a
value: every case runs on both arms of UDPDK_RX_POLICY (1 = the policy constants, 0 = default
policy on every stream; read at context creation) and equals the oracle bit for bit. The shapes
are the small ones where a policy could go wrong: the fused completion's repair reading other
workgroups' written-through words, recycled output buffers rewritten at pipeline depths 1 and 3,
range-checked window / tail / sweep loads at every offset residue with the last frame ending at
the buffer's last byte, and the multi-lane scan and scatter reading what classify wrote."""
import os

import numpy as np
import pytest

import oracle as O
from udpdk_amd import abi, frames as F

pytestmark = pytest.mark.gpu

ENV = ("UDPDK_RX_POLICY", "UDPDK_RX_FUSE", "UDPDK_RX_TAILG", "UDPDK_RX_SPAN")
LISTS1 = {abi.raw_port(10001): [(0, 0, 0)]}
_ctxs = {}


def _ctx(policy, fuse=None, tailg=None, span=None):
    """A context of the given policy arm and forced kernel form, made once per module."""
    key = (policy, fuse, tailg, span)
    if key not in _ctxs:
        old = {k: os.environ.get(k) for k in ENV}
        for k, v in zip(ENV, key):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        try:
            _ctxs[key] = abi.GpuContext(0, max_frames=1 << 16, max_lanes=64)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _ctxs[key]


@pytest.fixture(scope="module", params=[1, 0], ids=["policy1", "policy0"])
def policy(request):
    yield request.param
    for key in [k for k in _ctxs if k[0] == request.param]:
        _ctxs.pop(key).close()


def _want(b, lists, n_lanes):
    return O.rx(O.bindtable_from_lists(lists), b.frames, b.frames_bytes, b.offset, b.length, None,
                n_lanes, 0xFFFFFFFF)


def _same(want, got, what):
    wm, wl, wp, wc = want
    gm, gl, gp, gc, rc = got
    assert rc == 0, what
    assert np.array_equal(wm, gm), f"{what}: verdict words"
    assert np.array_equal(wl, gl), f"{what}: lane_off {wl} vs {gl}"
    assert np.array_equal(wp, gp), f"{what}: lane entries"
    assert np.array_equal(wc, gc), f"{what}: counters"


def _run(ctx, b, lists=LISTS1, n_lanes=1, want=None):
    ctx.upload_snapshot(abi.snapshot_from_lists(lists, n_lanes))
    want = want or _want(b, lists, n_lanes)
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    out = abi.rx_alloc_out(ctx, b.n, n_lanes, b.n)
    got = abi.rx_run(ctx, db, out)
    for x in (db.frames, db.offset, db.length, out.meta, out.lane_off, out.lane_pkt):
        x.free()
    return want, got


N1 = 3 * 1024 + 17              # three full tiles and a partial last one


def _batch64(no_bind=None):
    b = F.build_frames(np.full(N1, 64, np.uint32), np.full(N1, 10001, np.uint32), 11)
    if no_bind is not None:
        v = b.frames[:N1 * 64].reshape(N1, 64)
        v[no_bind, 36] = 0x4E                                # dst port 20000: not bound
        v[no_bind, 37] = 0x20
    return b


@pytest.fixture(scope="module")
def clean():
    b = _batch64()
    return b, _want(b, LISTS1, 1)


def test_fused_repair(policy, clean):
    """Clean, then one NO_BIND frame in tile 0 (the last workgroup rewrites tiles 1-3 from the
    other workgroups' written-through verdict words and counts), then clean again on the same
    context (the fan-in words are back at zero)."""
    ctx = _ctx(policy, fuse=1, tailg=1)
    b, want = clean
    _same(*_run(ctx, b, want=want), "clean")
    d = _batch64(no_bind=5)
    wd, gd = _run(ctx, d)
    assert int(wd[1][1]) == N1 - 1
    _same(wd, gd, "one NO_BIND frame in tile 0")
    _same(*_run(ctx, b, want=want), "clean again")


@pytest.mark.parametrize("depth", [1, 3])
def test_recycled_outputs(policy, clean, depth):
    """Six consecutive calls on the same batch over two output sets: every set is rewritten by a
    later call, on another stream at depth 3."""
    ctx = _ctx(policy, fuse=1, tailg=1)
    b, want = clean
    ctx.upload_snapshot(abi.snapshot_from_lists(LISTS1, 1))
    db = abi.rx_upload(ctx, b.frames, b.offset, b.length)
    db.frames_bytes = b.frames_bytes
    outs = [abi.rx_alloc_out(ctx, b.n, 1, b.n) for _ in range(2)]
    ctx.pipeline(depth)
    try:
        for i in range(6):
            assert abi.rx_enqueue(ctx, db, outs[i % 2]) == 0
        rc, st = abi.rx_stats(ctx)
        assert rc == 0
        ctx.sync()
        wm, wl, wp, wc = want
        for out in outs:
            assert np.array_equal(ctx.download(out.meta, np.uint32, b.n), wm)
            assert np.array_equal(ctx.download(out.lane_off, np.uint32, 2), wl)
            assert np.array_equal(ctx.download(out.lane_pkt, np.uint32, len(wp)), wp)
        assert np.array_equal(np.array(st.counters[:], np.uint64), wc)
    finally:
        ctx.pipeline(1)
        for x in [db.frames, db.offset, db.length] + [y for o in outs for y in (o.meta, o.lane_off, o.lane_pkt)]:
            x.free()


def _residues(n, size, seed):
    """n frames of `size` bytes (even), one byte apart: the odd stride takes the offsets through
    every residue mod 4; the host array ends with the last frame's last byte."""
    src = F.build_frames(np.full(n, size, np.uint32), np.full(n, 10001, np.uint32), seed)
    off = np.arange(n, dtype=np.int64) * (size + 1)
    end = int(off[-1]) + size
    fr = np.full(end, 0x5A, np.uint8)
    rows = off[:, None] + np.arange(size)[None, :]
    fr[rows] = src.frames[:n * size].reshape(n, size)
    assert set(off % 4) == {0, 1, 2, 3} and len(fr) == end
    return F.Batch(fr, off.astype(np.uint32), np.full(n, size, np.uint16), end)


@pytest.mark.parametrize("n,size,form", [(2048, 64, dict(tailg=1)), (1024, 106, dict(tailg=2, span=0)),
                                         (1024, 1500, dict(tailg=2, span=1))],
                         ids=["64B-window", "106B-tail", "1500B-sweep"])
def test_offset_residues_to_the_last_byte(policy, n, size, form):
    """Window loads (64 B), the G = 2 tail pass (106 B) and the span sweep (1500 B frames one byte
    apart) at offsets of every residue mod 4, the last frame ending at the buffer's last byte."""
    b = _residues(n, size, 100 + size)
    want, got = _run(_ctx(policy, **form), b)
    assert int(want[1][1]) == n                             # every frame valid and delivered
    _same(want, got, f"{n} x {size} B")


def test_multi_lane(policy):
    """4096 frames over 64 ports, four 1024-frame tiles: the column scan reads classify's
    histogram rows, the scatter its verdict words."""
    n, lanes = 4096, 64
    assert abi.geometry(n, lanes)[0] == 1024
    rng = np.random.default_rng(5)
    b = F.build_frames(np.full(n, 64, np.uint32), 10000 + rng.integers(0, lanes, n, dtype=np.uint32), 12)
    lists = {abi.raw_port(10000 + i): [(0, i, 0)] for i in range(lanes)}
    _same(*_run(_ctx(policy), b, lists, lanes), "64 lanes")
