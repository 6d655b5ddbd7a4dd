"""The ICMP stage's model (tests/icmp_util.py) pinned down without a GPU, and the host-only parts of the
feature:

- the model's sum against tests/golden/checksum_vectors.json, its IPv4 header against oracle.ipv4_cksum;
- the model against a second, independent per-frame implementation written with struct below;
- the model's own replies: NOT_UDP with a good IPv4 checksum for the oracle's RX, unanswered when
  run through the model again, every ICMP checksum verifying; the two checksum edge cases by hand;
- exported symbols, the geometry helper, the -EINVAL answers that need no device (-ENOENT needs a
  context: tests/test_gpu_icmp.py);
- udpdk_config_icmp / udpdk_config_icmp_burst and the ini keys;
- the host queue (csrc/host/icmp_queue.h) through build/icmp_queue_check, a stand-alone program.
  UDPDK_ICMP_QUEUE_CHECK names another build of it to run instead (`make icmp-asan` gives
  build/icmp_queue_check_asan, the same source under the address and undefined-behaviour
  sanitizers: a stand-alone host binary)."""
import ctypes as C
import errno
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import icmp_util as U
import oracle as O
from udpdk_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.environ.get("UDPDK_ICMP_QUEUE_CHECK") or os.path.join(ROOT, "build", "icmp_queue_check")
OUR = abi.raw_ip(U.OUR_IP)


def _meta(buf, nb, off, ln):
    return O.rx(O.bindtable_from_lists(U.LISTS), buf, nb, off, ln, None, U.N_LANES)[0]


def test_sum_against_golden_vectors_and_the_oracle():
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "checksum_vectors.json")))
    seen = 0
    for v in vec:
        b = bytes.fromhex(v["bytes"])
        le = U.fold(U.word_sum(b))
        be = ((le & 0xFF) << 8) | (le >> 8)
        if "sum_be" in v:
            assert be == v["sum_be"], v["id"]
            seen += 1
        if "cksum_be" in v and len(b) != 20:
            assert (~be & 0xFFFF) == v["cksum_be"], v["id"]
        if len(b) == 20:                                     # an IPv4 header with a zero checksum field
            assert O.ipv4_cksum(b) == (le if le == 0xFFFF else ~le & 0xFFFF), v["id"]
            seen += 1
    assert seen >= 2
    rng = np.random.default_rng(3)
    for tl in (28, 56, 84, 1500, 0xFFEB):
        src, dst = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32))
        h = U.ipv4_header(tl, 1, src, dst)
        assert struct.unpack("<H", h[10:12])[0] == O.ipv4_cksum(h[:10] + b"\0\0" + h[12:])
    assert U.word_sum(b"\x01") == 1 and U.word_sum(b"\x01\x02\x03") == 0x0201 + 3 and U.cksum(bytes(8)) == 0xFFFF


# ---- a second implementation: one frame at a time, struct only ----------------------------------
def _be_sum(b: bytes) -> int:
    if len(b) & 1:
        b += b"\0"
    s = sum(struct.unpack(f">{len(b) // 2}H", b))
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def _reply_one(f: bytes, m: int, flags: int, mtu: int):
    """('echo' | 'unreach' | 'echo_bad' | 'bad_frame' | None, reply bytes or None) for one frame."""
    v, ip_ok, csum, len_bad, ihl_ne5 = m & 15, (m >> 4) & 1, (m >> 5) & 3, (m >> 7) & 1, (m >> 8) & 1
    if not ip_ok or ihl_ne5:
        return None, None
    echo = v == abi.V_NOT_UDP and flags & 1
    unr = v in (abi.V_NO_BIND, abi.V_NO_MATCH) and flags & 2 and csum != abi.UDP_BAD and not len_bad
    if not (echo or unr):
        return None, None
    if len(f) < 42:
        return "bad_frame", None
    tl, proto = struct.unpack(">H", f[16:18])[0], f[23]
    if f[30:34] != struct.pack("<I", OUR) or f[26] in (0, 127) or f[26] >= 224:
        return None, None
    eth = U.DST_MAC + U.SRC_MAC + b"\x08\x00"

    def ip(total):
        h = struct.pack(">BBHHHBBH", 0x45, 0, total, 0, 0, 64, 1, 0) + f[30:34] + f[26:30]
        c = _be_sum(h)
        return h[:10] + struct.pack(">H", c if c == 0xFFFF else 0xFFFF - c) + h[12:]
    if unr:
        body = b"\x03\x03\0\0\0\0\0\0" + f[14:42]
        return "unreach", eth + ip(56) + body[:2] + struct.pack(">H", 0xFFFF - _be_sum(body)) + body[4:]
    if proto != 1 or f[34] != 8 or f[35] != 0:
        return None, None
    if tl < 28 or 14 + tl > len(f) or (mtu and tl > mtu) or _be_sum(f[34:14 + tl]) != 0xFFFF:
        return "echo_bad", None
    body = b"\0\0\0\0" + f[38:14 + tl]
    return "echo", eth + ip(tl) + body[:2] + struct.pack(">H", 0xFFFF - _be_sum(body)) + body[4:]


@pytest.mark.parametrize("seed,flags,mtu", [(1, 3, 0), (2, 3, 1500), (3, 1, 0), (4, 2, 572)])
def test_model_against_the_per_frame_implementation(seed, flags, mtu):
    buf, nb, off, ln, kinds = U.mixed(seed, 1500)
    meta = _meta(buf, nb, off, ln)
    R = U.model(buf, nb, off, ln, meta, flags=flags, mtu=mtu)
    if flags == 3:
        U.assert_mixed_counts(R)
    want, what = [], {"echo": 0, "unreach": 0, "echo_bad": 0}
    for i in range(len(off)):
        r, b = _reply_one(bytes(buf[int(off[i]):int(off[i]) + int(ln[i])]), int(meta[i]), flags, mtu)
        if r in what:
            what[r] += 1
        assert (r or "") == (R.reason[i] if R.reason[i] in ("echo", "unreach", "echo_bad", "bad_frame") else ""), (i, kinds[i])
        if b is not None:
            want.append((i, b))
    assert [b for _, b in want] == R.frames_out and [i for i, _ in want] == list(R.origin)
    assert (what["echo"], what["unreach"], what["echo_bad"]) == (R.stats["echo_replied"], R.stats["unreach_sent"],
                                                                 R.stats["echo_bad"])
    assert b"".join(R.frames_out) == R.out.tobytes() and list(R.reply_off) == list(np.cumsum([0] + [len(b) for b in R.frames_out]))
    if flags & 1:
        assert what["echo"] >= 20 and what["echo_bad"] >= 20
    if flags & 2:
        assert what["unreach"] >= 20
    # the limit and the room, against the unlimited run
    elig = [i for i, r in enumerate(R.reason) if r == "unreach"]
    if len(elig) > 30:
        Lm = U.model(buf, nb, off, ln, meta, flags=flags, mtu=mtu, err_limit=25)
        assert [i for i, r in enumerate(Lm.reason) if r == "limited"] == elig[25:] and Lm.stats["limited"] == len(elig) - 25
        assert Lm.frames_out == [b for i, b in want if i not in set(elig[25:])]
    cut = U.model(buf, nb, off, ln, meta, flags=flags, mtu=mtu, out_cap=int(R.reply_off[30]) + 3, max_replies=40)
    assert cut.stats["replies"] == 30 and cut.stats["no_room"] == R.stats["replies"] - 30
    assert cut.stats["bytes_needed"] == R.stats["bytes_needed"] and cut.frames_out == R.frames_out
    assert U.model(buf, nb, off, ln, meta, flags=flags, mtu=mtu, max_replies=12).stats["replies"] == 12


def test_the_models_replies_are_not_answered():
    buf, nb, off, ln, kinds = U.mixed(9, 1200)
    R = U.model(buf, nb, off, ln, _meta(buf, nb, off, ln))
    U.assert_mixed_counts(R)
    # the replies as a batch addressed to whoever asked: seen from there they are unicast to "us"
    rb, rnb, roff, rln = U.pack(R.frames_out)
    m2 = _meta(rb, rnb, roff, rln)
    assert np.all((m2 & 0xF) == abi.V_NOT_UDP) and np.all((m2 >> 4) & 1 == 1) and np.all((m2 >> 8) & 1 == 0)
    for j, b in enumerate(R.frames_out):
        assert U.fold(U.word_sum(b[34:])) == 0xFFFF and b[34] in (0, 3) and b[23] == 1
        assert b[26:30] == struct.pack("<I", OUR)
        R2 = U.model(*U.pack([b]), m2[j:j + 1], src_ip=struct.unpack("<I", b[30:34])[0])
        assert R2.stats["replies"] == 0 and R2.reason == ["other"]


def test_checksum_edge_cases_by_hand():
    rng = np.random.default_rng(0)
    zero = U.echo_request(rng, 40, ident=0, seq=0, data=bytes(32))
    assert zero[34:38] == b"\x08\x00\xf7\xff"
    ones = U.echo_request(rng, 8, ident=0xFFFF, seq=0)
    assert ones[34:42] == b"\x08\x00\xf7\xff\xff\xff\x00\x00"
    bt = U.pack([zero, ones])
    R = U.model(*bt, _meta(*bt))
    assert R.frames_out[0][34:] == b"\x00\x00\xff\xff" + bytes(36)          # an all-zero reply carries FF FF
    assert R.frames_out[1][34:] == b"\x00\x00\x00\x00\xff\xff\x00\x00"      # a sum of 0xFFFF carries 00 00
    assert R.frames_out[0][:34] == U.DST_MAC + U.SRC_MAC + b"\x08\x00" + U.ipv4_header(60, 1, OUR, abi.raw_ip("172.31.100.2"))


def test_symbols_geometry_and_argument_errors_without_a_device():
    L = abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = {"udpdk_gpu_icmp_reply", "udpdk_gpu_icmp_stats", "udpdk_gpu_icmp_geometry", "udpdk_gpu_pipe_icmp_reply",
             "udpdk_gpu_pipe_icmp_stats", "udpdk_config_icmp", "udpdk_config_icmp_burst", "udpdk_icmp_counts"}
    assert names <= exported and names <= set(abi.declared_symbols())
    hdr = open(os.path.join(ROOT, "include", "udpdk_gpu.h")).read() + open(os.path.join(ROOT, "include", "udpdk_api.h")).read()
    assert all(n + "(" in hdr for n in names)
    assert (abi.ICMP_ECHO, abi.ICMP_UNREACH, abi.ICMP_ALL, abi.ICMP_UNREACH_BYTES) == (1, 2, 3, 70)
    assert "#define UDPDK_ICMP_UNREACH_BYTES 70u" in hdr
    e, k = abi.icmp_geometry(1)
    assert e >= 64 and e % 64 == 0 and k == 1
    for n in (0, 1, e - 1, e, e + 1, 2 * e + 1, 1 << 20, 0xFFFFFFFF):
        assert abi.icmp_geometry(n) == (e, max(1, -(-n // e)))
    x = C.c_uint32()
    assert L.udpdk_gpu_icmp_geometry(5, None, C.byref(x)) == -errno.EINVAL
    assert L.udpdk_gpu_icmp_geometry(5, C.byref(x), None) == -errno.EINVAL
    bt, o, cfg, st = abi.RxBatch(), abi.IcmpOut(), abi.TxConfig(), abi.IcmpStats()
    assert L.udpdk_gpu_icmp_reply(None, C.byref(cfg), C.byref(bt), None, 3, 0, 0, C.byref(o)) == -errno.EINVAL
    assert L.udpdk_gpu_pipe_icmp_reply(None, 1, C.byref(cfg), C.byref(bt), None, 3, 0, 0, C.byref(o)) == -errno.EINVAL
    assert L.udpdk_gpu_icmp_stats(None, C.byref(st)) == -errno.EINVAL
    assert L.udpdk_gpu_pipe_icmp_stats(None, 1, C.byref(st)) == -errno.EINVAL
    assert L.udpdk_icmp_counts(None) == -1


def test_config_semantics(host_api):
    assert host_api.config_icmp(-1) == 0 and host_api.config_icmp_burst(-2) == 64        # the defaults
    assert host_api.config_icmp(abi.ICMP_ECHO) == 0 and host_api.config_icmp(-5) == abi.ICMP_ECHO
    assert host_api.config_icmp(abi.ICMP_ALL) == abi.ICMP_ECHO
    for bad in (4, 7, 1 << 20):
        assert host_api.config_icmp(bad) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_icmp(-1) == abi.ICMP_ALL
    assert host_api.config_icmp_burst(0) == 64 and host_api.config_icmp_burst(-1) == 0
    assert host_api.config_icmp_burst(-7) == -1 and host_api.config_icmp_burst(1000) == -1
    assert host_api.config_icmp_burst(-2) == 1000
    c = host_api.icmp_counts()
    assert (c.echo_replied, c.unreach_sent, c.echo_bad, c.limited, c.queue_dropped) == (0, 0, 0, 0, 0)
    host_api.reset()
    assert host_api.config_icmp(-1) == 0 and host_api.config_icmp_burst(-2) == 64 and host_api.tx_pending() == 0


@pytest.mark.parametrize("lines,flags,burst", [
    ("", 0, 64), ("icmp = none\n", 0, 64), ("icmp = all\n", 3, 64), ("icmp = echo\n", 1, 64),
    ("icmp = unreach\nicmp_burst = 0\n", 2, 0), ("icmp = unreach , echo\nicmp_burst = -1\n", 3, -1),
    ("icmp = echo,unreach\nicmp_burst = 5\n", 3, 5),
    ("icmp = ping\n", None, None), ("icmp = echo,\n", None, None), ("icmp = \n", None, None),
    ("icmp_burst = -2\n", None, None), ("icmp_burst = many\n", None, None), ("icmp_burst = 3x\n", None, None),
    ("icmp = all\ndevices = 0,0\n", None, None)])
def test_ini_keys(tmp_path, host_api, lines, flags, burst):
    """udpdk_init reads the whole file before it looks for a GPU: a bad value is EINVAL either way, a
    good one leaves ENODEV here (or a session, on a machine with a GPU) and the parsed settings."""
    if abi.lib().udpdk_gpu_context():                        # (a session some other test left up)
        return
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.1\n[gpu]\n" + lines)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    rc = abi.lib().udpdk_init(3, argv)
    try:
        if flags is None:
            assert rc == -1 and host_api.errno() == errno.EINVAL
        else:
            assert rc == 0 or host_api.errno() == errno.ENODEV
            assert host_api.config_icmp(-1) == flags and host_api.config_icmp_burst(-2) == burst
    finally:
        abi.lib().udpdk_cleanup()


# ---- the queue, stand-alone -----------------------------------------------------------------------
def _queue(script: str):
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/icmp_queue_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([CHECK], input=script, capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


def test_queue_order_wrap_and_limits():
    got = _queue("init 1000\n"
                 "push 400 1\npush 400 2\npush 300 3\n"          # the third does not fit the byte ring
                 "stat\n"
                 "drain 1 4096\n"                                # max: one leaves
                 "push 300 4\n"                                  # wraps to the front (400 free there)
                 "push 200 5\n"                                  # 100 left at the front: dropped
                 "drain 8 399\n"                                 # out_cap one byte short: stays queued
                 "drain 8 400\n"
                 "drain 0 4096\n"
                 "push 600 6\n"                                  # [300, 900) is free again behind frame 4
                 "drain 8 899\n"                                 # 300 fits, then 600 does not
                 "stat\ndrain 8 600\nstat\n"
                 "push 0 7\npush 1001 8\npush 1000 9\nstat\n"    # empty, larger than the ring, exactly the ring
                 "reset\nstat\ndrain 8 4096\n")
    assert got == ["init", "push 0", "push 0", "push -1", "stat 2 1", "drain 1 400:1", "push 0", "push -1",
                   "drain 0", "drain 1 400:2", "drain 0", "push 0", "drain 1 300:4", "stat 1 2", "drain 1 600:6",
                   "stat 0 2", "push -1", "push -1", "push 0", "stat 1 4", "reset", "stat 0 4", "drain 0"]


def test_queue_full_frame_ring_and_long_run():
    n = 4096
    script = "init 1048576\n" + "".join(f"push {1 + k % 60} {k % 251}\n" for k in range(n + 5)) + "stat\ndrain 5000 1048576\nstat\n"
    got = _queue(script)
    assert got[1:n + 1] == ["push 0"] * n and got[n + 1:n + 6] == ["push -1"] * 5 and got[n + 6] == f"stat {n} 5"
    assert got[n + 7].split()[:2] == ["drain", str(n)]
    assert got[n + 7].split()[2:] == [f"{1 + k % 60}:{k % 251}" for k in range(n)] and got[n + 8] == "stat 0 5"
    # a long run of pushes and partial drains: every frame comes out once, in order, intact
    rng = np.random.default_rng(8)
    script, sent, want = "init 5000\n", [], []
    for k in range(3000):
        ln = int(rng.integers(1, 700))
        script += f"push {ln} {k % 256}\n"
        sent.append((ln, k % 256))
        if k % 3 == 2:
            script += f"drain {int(rng.integers(0, 6))} {int(rng.integers(0, 2500))}\n"
    script += "drain 100 100000\nstat\n"
    got = _queue(script)[1:]
    pushed = [s for s, g in zip(sent, [g for g in got if g.startswith("push")]) if g == "push 0"]
    drained = [tuple(int(x) for x in t.split(":")) for g in got if g.startswith("drain") for t in g.split()[2:]]
    assert "bad" not in " ".join(got) and drained == pushed and 500 < len(pushed) < 3000
    assert got[-1] == f"stat 0 {3000 - len(pushed)}"
