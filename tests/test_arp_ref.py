"""ARP without a GPU:
- the model of udpdk_gpu_arp_reply (tests/arp_util.py) against request / reply pairs written out by
  hand from RFC 826 and RFC 5227 (tests/golden/arp_vectors.json);
- the host's announcement builder (csrc/host/arp_frame.h) through build/arp_frame_check, a stand-alone
  program. UDPDK_ARP_FRAME_CHECK names another build of it to run instead (`make arp-asan` gives
  build/arp_frame_check_asan, the same source under the address and undefined-behaviour sanitizers);
- udpdk_config_arp / udpdk_arp_announce / udpdk_arp_counts, the ini keys and the symbols."""
import ctypes as C
import errno
import json
import os
import subprocess

import pytest

import arp_util as U
from udpdk_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.environ.get("UDPDK_ARP_FRAME_CHECK") or os.path.join(ROOT, "build", "arp_frame_check")
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "arp_vectors.json")))
MAC, IP = bytes.fromhex(VEC["our_mac"]), VEC["our_ip"]


def _run_model(frame_list, **kw):
    buf, nb, off, ln = U.pack(frame_list, aligns=[3 * k + 1 for k in range(len(frame_list))])
    return U.model(buf, nb, off, ln, U.host_meta(buf, off, ln), mac=MAC, ip=abi.raw_ip(IP), **kw)


def test_model_against_hand_written_vectors():
    cases = VEC["cases"]
    R = _run_model([bytes.fromhex(c["request"]) for c in cases])
    assert R["reason"] == [c["counter"] for c in cases]
    want = [bytes.fromhex(c["reply"]) for c in cases if c["reply"]]
    assert len(want) >= 2 and R["stats"]["replies"] == len(want)
    for r, b in enumerate(want):
        assert bytes(R["slots"][r, :42]) == b and not R["slots"][r, 42:].any()
    assert list(R["origin"]) == [i for i, c in enumerate(cases) if c["reply"]]
    assert R["stats"]["arp"] == len(cases) and R["stats"]["bad_frame"] == 0
    for k in ("other_op", "not_ours", "conflict", "own", "malformed", "sender_bad"):
        assert R["stats"][k] == 1, k
    # one case alone, with no room: counted, nothing written
    R = _run_model([bytes.fromhex(cases[0]["request"])], max_replies=0)
    assert R["stats"]["eligible"] == 1 and R["stats"]["replies"] == 0 and R["stats"]["no_room"] == 1


def test_model_over_every_kind():
    buf, nb, off, ln, kinds = U.mixed(3, 1200)
    R = U.model(buf, nb, off, ln, U.host_meta(buf, off, ln))
    for i, k in enumerate(kinds):
        assert R["reason"][i] == (None if k == "udp" else U.KINDS[k]), (i, k, R["reason"][i])
    assert {int(o) % 16 for o in off} == set(range(16))
    # a reply is itself an ARP frame with opcode 2: the model does not answer its own output
    R2 = _run_model(R["frames_out"][:50])
    assert R2["stats"]["other_op"] == 50 and R2["stats"]["replies"] == 0


def _announce_tool(mac: bytes, ip: str) -> bytes:
    if not os.path.exists(CHECK):   # the driver's build() makes it (`make`: part of `all`)
        subprocess.run(["make", "build/arp_frame_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([CHECK, ":".join(f"{b:02x}" for b in mac), ip], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    return bytes.fromhex(out.stdout.strip())


def test_announcement_builder_against_the_hand_written_vector():
    want = bytes.fromhex(VEC["announcement"])
    assert len(want) == 42 and _announce_tool(MAC, IP) == want
    other = _announce_tool(bytes.fromhex("02a1b2c3d4e5"), "10.1.2.3")
    assert other == bytes.fromhex("ffffffffffff02a1b2c3d4e50806000108000604000102a1b2c3d4e50a0102030000000000000a010203")
    # on the wire the stack's own announcement is `own`, another host's is `not_ours` (or `conflict`)
    assert _run_model([want, other])["reason"] == ["own", "not_ours"]


def test_symbols_geometry_and_argument_errors_without_a_device():
    L = abi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    names = {"udpdk_gpu_arp_reply", "udpdk_gpu_arp_stats", "udpdk_gpu_arp_geometry", "udpdk_gpu_pipe_arp_reply",
             "udpdk_gpu_pipe_arp_stats", "udpdk_config_arp", "udpdk_arp_announce", "udpdk_arp_counts"}
    assert names <= exported
    T, nb = abi.arp_geometry(1)
    assert T >= 64 and T % 64 == 0 and nb == 1
    assert abi.arp_geometry(0) == (T, 1) and abi.arp_geometry(T + 1) == (T, 2) and abi.arp_geometry(5 * T) == (T, 5)
    assert L.udpdk_gpu_arp_geometry(1, None, None) == -errno.EINVAL
    st = abi.ArpStats()
    assert L.udpdk_gpu_arp_stats(None, C.byref(st)) == -errno.EINVAL
    assert L.udpdk_gpu_arp_reply(None, None, None, None, None) == -errno.EINVAL
    assert L.udpdk_arp_counts(None) == -1
    assert C.sizeof(abi.ArpStats) == 44 and C.sizeof(abi.ArpCounts) == 96 and C.sizeof(abi.ArpOut) == 24


def test_config_semantics(host_api):
    assert host_api.config_arp(-1) == 0                                   # the default
    assert host_api.config_arp(1) == 0 and host_api.config_arp(-7) == 1
    for bad in (2, 3, 1 << 20):
        assert host_api.config_arp(bad) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_arp(-1) == 1
    assert host_api.config_arp(0) == 1 and host_api.config_arp(1) == 0
    host_api.reset()
    assert host_api.config_arp(-1) == 0


def _counts(api) -> dict:
    c = api.arp_counts()
    return {k: int(getattr(c, k)) for k, _ in abi.ArpCounts._fields_}


def test_announce_and_counts(host_api):
    zero = {k: 0 for k, _ in abi.ArpCounts._fields_}
    assert _counts(host_api) == zero
    assert host_api.config_set(MAC, U.PEER_MAC, "0.0.0.0") == 0
    assert host_api.arp_announce() == -1 and host_api.errno() == errno.EADDRNOTAVAIL
    assert host_api.tx_pending() == 0 and _counts(host_api) == zero
    assert host_api.config_set(MAC, U.PEER_MAC, IP) == 0
    for k in (1, 2, 3):
        assert host_api.arp_announce() == 0
        assert host_api.tx_pending() == k and _counts(host_api) == dict(zero, announced=k)
    host_api.reset()
    assert host_api.tx_pending() == 0 and _counts(host_api) == zero


def test_announce_into_a_full_queue(host_api):
    assert host_api.config_set(MAC, U.PEER_MAC, IP) == 0
    for _ in range(4096):
        assert host_api.arp_announce() == 0
    assert host_api.arp_announce() == -1 and host_api.errno() == errno.ENOBUFS
    assert host_api.tx_pending() == 4096 and _counts(host_api)["announced"] == 4096
    assert host_api.icmp_counts().queue_dropped == 1


@pytest.mark.parametrize("lines,arp", [
    ("", 0), ("arp = 0\n", 0), ("arp = 1\n", 1), ("arp = 1\narp_announce = 0\n", 1),
    ("arp = 2\n", None), ("arp = on\n", None), ("arp = \n", None), ("arp_announce = 2\n", None),
    ("arp = 1\ndevices = 0,0\n", None)])
def test_ini_keys(tmp_path, host_api, lines, arp):
    """udpdk_init reads the whole file before it looks for a GPU: a bad value is EINVAL either way, a
    good one leaves ENODEV here (or a session, on a machine with a GPU) and the parsed settings."""
    if abi.lib().udpdk_gpu_context():                        # (a session some other test left up)
        return
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.1\n[gpu]\n" + lines)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    rc = abi.lib().udpdk_init(3, argv)
    try:
        if arp is None:
            assert rc == -1 and host_api.errno() == errno.EINVAL
        else:
            assert rc == 0 or host_api.errno() == errno.ENODEV
            assert host_api.config_arp(-1) == arp
    finally:
        abi.lib().udpdk_cleanup()
