"""The reply plan's model (tests/tx_reply_util.py) pinned to the oracle, and the host-only parts of
the reply path, without a GPU:

- on frames.mixed_batch batches run through oracle.rx, the model's payload, source address and
  source port of every lane entry are oracle.recv_gather's, its lanes the oracle's lanes;
- its spans are udpdk_gpu_tx_span's, its out-of-room entries a tail, its offsets the prefix;
- udpdk_gpu_tx_reply_geometry, and the -EINVAL / -ENOENT answers that need no device;
- the frame-table expansion of udpdk_poll_echo (csrc/host/echo_expand.h) through
  build/echo_expand_check, a stand-alone program. UDPDK_ECHO_EXPAND_CHECK names another build of it
  to run instead (`make echo-asan` gives build/echo_expand_check_asan, the same source under the
  address and undefined-behaviour sanitizers: a stand-alone host binary)."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import tx_reply_util as R
from udpdk_amd import abi, frames as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.environ.get("UDPDK_ECHO_EXPAND_CHECK") or os.path.join(ROOT, "build", "echo_expand_check")

IP1 = "172.31.100.1"
LISTS = {abi.raw_port(10001): [(0, 0, 0)],
         abi.raw_port(10002): [(abi.raw_ip(IP1), 2, 1), (abi.raw_ip(IP1), 5, 1)],
         abi.raw_port(10003): [(0, 6, 0)]}
N_LANES = 8


def _mixed(seed, n=400):
    b = F.mixed_batch(seed, n, [10001, 10002, 10003], [7], [IP1, "172.31.100.9"])
    _, loff, lpkt, _ = O.rx(O.bindtable_from_lists(LISTS), b.frames, b.frames_bytes, b.offset, b.length, None, N_LANES)
    return b, loff, lpkt


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_matches_recv_gather(seed):
    b, loff, lpkt = _mixed(seed)
    D = int(loff[N_LANES])
    assert D > 100 and len(lpkt) == D
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, D)
    pay, ln, sip, spt = O.recv_gather(b.frames, b.offset, b.length, lpkt, 0, D, 2048)
    assert np.all(P.sockfd >= 0) and P.stats["replied"] == D and P.stats["no_room"] == 0
    assert np.array_equal(P.payload_len, ln.astype(np.uint16))
    assert np.array_equal(P.dst_ip, sip) and np.array_equal(P.dst_port, spt)
    for k in range(D):
        o, L = int(P.payload_off[k]), int(P.payload_len[k])
        assert b.frames[o:o + L].tobytes() == pay[k, :L].tobytes(), k
        # the answering socket is the lane the oracle put the entry in
        assert loff[P.sockfd[k]] <= k < loff[P.sockfd[k] + 1]
    assert len({int(x) for x in P.sockfd}) >= 4              # fan-out lanes 2 and 5 among them
    # a sub-range: the same entries, offsets restarting at 0
    Q = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 37, 101)
    assert np.array_equal(Q.sockfd, P.sockfd[37:138]) and np.array_equal(Q.payload_off, P.payload_off[37:138])
    assert np.array_equal(Q.frame_off.astype(np.int64), P.frame_off[37:139].astype(np.int64) - int(P.frame_off[37]))


@pytest.mark.parametrize("mtu", [0, 68, 1500])
def test_spans_are_tx_span(mtu):
    nf = C.c_uint32()
    for L in [0, 1, 17, 18, 25, 26, 27, 1457, 1458, 1459, 1472, 1473, 2952, 2953, 3000, 65507, 65535]:
        got = abi.lib().udpdk_gpu_tx_span(L, mtu, C.byref(nf))
        assert (got, nf.value) == R.span(L, mtu), L
    b, loff, lpkt = _mixed(4, 200)
    D = int(loff[N_LANES])
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, D, mtu=mtu)
    want = np.cumsum([0] + [abi.lib().udpdk_gpu_tx_span(int(L), mtu, None) for L in P.payload_len])
    assert np.array_equal(P.frame_off.astype(np.int64), want)
    assert P.stats["bytes_needed"] == want[-1]


def test_out_of_room_is_a_tail():
    b, loff, lpkt = _mixed(5, 300)
    D = int(loff[N_LANES])
    full = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, D)
    for kc in (1, D // 2, D - 1):
        cap = int(full.frame_off[kc + 1]) - 1                # entry kc misses by one byte
        P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, D, out_cap=cap)
        assert np.all(P.sockfd[:kc] >= 0) and np.all(P.sockfd[kc:] == -1) and not P.payload_len[kc:].any()
        assert np.array_equal(P.frame_off[:kc + 1], full.frame_off[:kc + 1])
        assert np.all(P.frame_off[kc:] == full.frame_off[kc]) and int(P.frame_off[-1]) <= cap
        assert P.stats["no_room"] == D - kc and P.stats["bytes_needed"] == full.stats["bytes_needed"]
        assert P.stats["replied"] + P.stats["skipped"] == D
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, lpkt, 0, D,
                     out_cap=full.stats["bytes_needed"])
    assert P.stats["no_room"] == 0 and np.array_equal(P.frame_off, full.frame_off)


def test_model_skip_rules_and_lane_lookup():
    b, loff, lpkt = _mixed(6, 120)
    D = int(loff[N_LANES])
    # empty lanes are passed over; an offset beyond D counts as D
    assert R.lane_of([0, 0, 0, 5, 5, 9], 5, 9, 0) == 2 and R.lane_of([0, 0, 0, 5, 5, 9], 5, 9, 5) == 4
    assert R.lane_of([0, 4, 100, 100], 3, 6, 5) == 1
    bad = lpkt.copy()
    bad[3], bad[7] = b.n, 0xFFFFFFFF
    sel = np.array([1, 0] * (N_LANES // 2), np.uint8)
    P = R.plan_model(b.frames, b.frames_bytes, b.offset, b.length, loff, bad, 0, D + 5, lane_sel=sel)
    assert P.reason[3] == P.reason[7] == "bad_index" and P.reason[D:] == ["past"] * 5
    assert P.stats["bad_index"] == 2 and P.stats["unselected"] == P.reason.count("unselected") > 0
    assert all(sel[s] for s in P.sockfd if s >= 0)
    assert P.stats["skipped"] == sum(1 for r in P.reason if r)


def test_geometry_and_argument_errors_without_a_device():
    L = abi.lib()
    e, k = abi.tx_reply_geometry(1)
    assert e >= 64 and e % 64 == 0 and k == 1
    for count in (0, 1, e - 1, e, e + 1, 3 * e + 1, 1 << 20, 0xFFFFFFFF):
        assert abi.tx_reply_geometry(count) == (e, max(1, -(-count // e)))
    x = C.c_uint32()
    assert L.udpdk_gpu_tx_reply_geometry(5, None, C.byref(x)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_reply_geometry(5, C.byref(x), None) == -errno.EINVAL
    bt, ln, pl, cfg = abi.RxBatch(), abi.RxLanes(), abi.TxReplyPlan(), abi.TxConfig()
    st = abi.TxReplyStats()
    assert L.udpdk_gpu_tx_reply_plan(None, C.byref(bt), C.byref(ln), 0, 1, None, 0, 1 << 20, C.byref(pl)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_reply(None, C.byref(cfg), C.byref(bt), C.byref(ln), 0, 1, None, 0, 0, None, 1 << 20,
                                C.byref(pl)) == -errno.EINVAL
    assert L.udpdk_gpu_tx_reply_stats(None, C.byref(st)) == -errno.EINVAL


def test_poll_echo_without_a_context(host_api):
    if abi.lib().udpdk_gpu_context():                       # (a session some other test left up)
        return
    fr = np.zeros(256, np.uint8)
    rc, err, frames, _, n_out = host_api.poll_echo(fr, 64, np.zeros(1, np.uint32), np.full(1, 64, np.uint16))
    assert rc == -1 and err == errno.ENODEV and n_out == 0 and frames == []
    assert abi.lib().udpdk_poll_echo(None, 0, None, None, None, 0, None, 0, None, None, 0, None, None) == -1
    assert host_api.errno() == errno.EINVAL


# ---- the frame-table expansion, stand-alone ------------------------------------------------------
@pytest.fixture(scope="module")
def expand():
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/echo_expand_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)

    def run(cases):
        text = "".join(f"{mtu} {mx} {ob} {len(ent)} " + " ".join(f"{a} {s} {f}" for a, s, f in ent) + "\n"
                       for mtu, mx, ob, ent in cases)
        out = subprocess.run([CHECK], input=text, capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        res = []
        for line in out.stdout.splitlines():
            t = line.split()
            res.append((int(t[0]), int(t[1]), [tuple(int(x) for x in p.split(":")) for p in t[2:]]))
        assert len(res) == len(cases)
        return res
    return run


def _entries(lens, socks, mtu):
    ent, pos, want = [], 0, []
    for L, s in zip(lens, socks):
        ent.append((L if s >= 0 else 0, s, pos))
        if s < 0:
            continue
        sp, nf = R.span(L, mtu)
        for f in range(nf):
            want.append((pos + f * (mtu + 14), mtu + 14 if f + 1 < nf else sp - (nf - 1) * (mtu + 14)))
        pos += sp
    return ent, want, pos


@pytest.mark.parametrize("mtu", [0, 68, 1500])
def test_expand_frames(expand, mtu):
    rng = np.random.default_rng(50 + mtu)
    # (out_len is 16 bits, as in udpdk_tx_drain: unfragmented, a frame is at most 65535 bytes)
    lens = [0, 1, 18, 25, 26, 27, 1458, 1459, 1472, 1473, 3000, 65507 if mtu else 65493]
    lens += rng.integers(0, 4000, 40).tolist()
    socks = [int(s) for s in rng.integers(0, 4, len(lens))]
    for k in (2, 7, 20, 21):                                 # skipped entries in the middle
        socks[k] = -1
    ent, want, pos = _entries(lens, socks, mtu)
    tail = ent + [(0, -1, pos)] * 5                          # a truncated tail: entries out of room
    nf = len(want)
    got = expand([(mtu, nf, pos, ent), (mtu, nf + 3, pos, tail), (mtu, nf - 1, pos, ent), (mtu, 0, pos, ent),
                  (mtu, nf, pos - 1, ent), (mtu, 0, 0, []), (mtu, 4, 0, [(0, -1, 0)] * 3)])
    assert got[0] == (0, nf, want) and got[1] == (0, nf, want)
    assert got[2] == (-errno.ENOBUFS, nf, []) and got[3] == (-errno.ENOBUFS, nf, [])
    assert got[4] == (-errno.EINVAL, nf, [])
    assert got[5] == (0, 0, []) and got[6] == (0, 0, [])
    # the frames tile the output exactly
    assert sum(l for _, l in want) == pos and all(want[j][0] + want[j][1] == want[j + 1][0] for j in range(nf - 1))
