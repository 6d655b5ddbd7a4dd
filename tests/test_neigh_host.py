"""The neighbour switch of the socket layer without a GPU: udpdk_config_neigh's modes, the ini keys, what needs
the session's GPU and what sharded polls refuse."""
import ctypes as C
import errno

import pytest

from udpdk_amd import abi

MAC = bytes.fromhex("02aa00000001")


def test_config_semantics(host_api):
    assert host_api.config_neigh(-1) == 0                                 # the default
    assert host_api.config_neigh(1) == 0 and host_api.config_neigh(-7) == 1
    assert host_api.config_neigh(2) == 1 and host_api.config_neigh(-1) == 2
    for bad in (3, 4, 1 << 20):
        assert host_api.config_neigh(bad) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_neigh(-1) == 2
    assert host_api.config_neigh(0) == 2 and host_api.config_neigh(1) == 0
    host_api.reset()
    assert host_api.config_neigh(-1) == 0


def test_counts_and_what_needs_the_gpu(host_api):
    if abi.lib().udpdk_gpu_context():                        # (a session some other test left up)
        return
    assert set(host_api.neigh_counts().values()) == {0}
    assert len(host_api.neigh_counts()) == 26 and C.sizeof(abi.NeighCounts) == 26 * 8
    assert abi.lib().udpdk_neigh_counts(None) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.neigh_add("10.0.0.1", MAC) == -1 and host_api.errno() == errno.ENODEV
    assert host_api.neigh_add(0, MAC) == -1 and host_api.errno() == errno.EINVAL
    assert abi.lib().udpdk_neigh_add(1, None) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.neigh_flush() == -1 and host_api.errno() == errno.ENODEV


def _init(tmp_path, gpu_lines, port0_lines=""):
    ini = tmp_path / "udpdk.ini"
    ini.write_text("[port0]\nmac_addr = 68:05:ca:95:f8:ec\nip_addr = 172.31.100.1\n" + port0_lines + "[gpu]\n" + gpu_lines)
    argv = (C.c_char_p * 4)(b"prog", b"-c", str(ini).encode(), None)
    return abi.lib().udpdk_init(3, argv)


@pytest.mark.parametrize("lines,port0,mode", [
    ("", "", 0), ("neigh = 0\n", "", 0), ("neigh = 1\n", "", 1), ("neigh = fallback\n", "", 2),
    ("neigh = 1\nneigh_entries = 8\nneigh_ttl_ms = 0\nneigh_retrans_ms = 4294967295\n", "", 1),
    ("neigh = 1\nneigh_entries = 65536\n", "netmask = 255.255.255.0\ngateway = 172.31.100.254\n", 1),
    ("neigh = fallback\n", "netmask = 0.0.0.0\n", 2),
    ("neigh = 2\n", "", None), ("neigh = on\n", "", None), ("neigh = \n", "", None), ("neigh = strict\n", "", None),
    ("neigh_entries = 0\n", "", None), ("neigh_entries = 7\n", "", None), ("neigh_entries = 12\n", "", None),
    ("neigh_entries = 131072\n", "", None), ("neigh_entries = many\n", "", None),
    ("neigh_ttl_ms = soon\n", "", None), ("neigh_ttl_ms = 4294967296\n", "", None), ("neigh_retrans_ms = 1s\n", "", None),
    ("", "netmask = /24\n", None), ("", "gateway = router\n", None),
    ("neigh = 1\ndevices = 0,0\n", "", None)])
def test_ini_keys(tmp_path, host_api, lines, port0, mode):
    """udpdk_init reads the whole file before it looks for a GPU: a bad value is EINVAL either way, a good one
    leaves ENODEV here (or a session, on a machine with a GPU) and the parsed mode. [port0_dst] is not needed."""
    if abi.lib().udpdk_gpu_context():                        # (a session some other test left up)
        return
    rc = _init(tmp_path, lines, port0)
    try:
        if mode is None:
            assert rc == -1 and host_api.errno() == errno.EINVAL
        else:
            assert rc == 0 or host_api.errno() == errno.ENODEV
            assert host_api.config_neigh(-1) == mode
    finally:
        abi.lib().udpdk_cleanup()


def test_sharded_polls_refuse_the_switch(tmp_path, host_api):
    """[gpu] devices with two entries: the modes above 0 are ENOTSUP, as for udpdk_config_arp."""
    if abi.lib().udpdk_gpu_context():
        return
    rc = _init(tmp_path, "devices = 0,0\n")
    try:
        assert rc == 0 or host_api.errno() == errno.ENODEV
        for mode in (1, 2):
            assert host_api.config_neigh(mode) == -1 and host_api.errno() == errno.ENOTSUP
        assert host_api.config_neigh(0) == 0 and host_api.config_neigh(-1) == 0
        assert host_api.config_neigh(3) == -1 and host_api.errno() == errno.EINVAL
    finally:
        abi.lib().udpdk_cleanup()
    # the next session's ini is not sharded: the switch works again
    rc = _init(tmp_path, "")
    try:
        assert rc == 0 or host_api.errno() == errno.ENODEV
        assert host_api.config_neigh(1) == 0
    finally:
        abi.lib().udpdk_cleanup()
