"""UDP checksum on TX, the parts that need no GPU: the tests' own RFC 768 helper
(tx_cksum_util.py) is pinned against the oracle's RX verification, which the GPU tests then use
as the expected image; the new entry points are exported, declared and reject bad arguments; the
socket layer's switch round-trips."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

import oracle as O
import tx_cksum_util as U
from udpdk_amd import abi

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
SRC_IP = abi.raw_ip("172.31.100.2")
LENS = [0, 1, 2, 21, 22, 38, 39, 1458]


def _frame(L, seed=0, slot=(abi.raw_ip("10.1.2.3"), 5353, 1)):
    rng = np.random.default_rng(100 + L + seed)
    pay = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
    ip, port, bound = slot
    return O.tx_frame(SRC_MAC, DST_MAC, SRC_IP, bound, ip, port, int(rng.integers(1, 2**32)),
                      int(rng.integers(0, 65536)), pay)


@pytest.mark.parametrize("L", LENS)
def test_helper_verifies_in_oracle_rx(L):
    """O.tx_frame output is CSUM_NONE as built and CSUM_OK once patched by the helper; a patched
    frame with one payload (or, at L = 0, header) bit flipped is CSUM_BAD."""
    f = _frame(L)
    assert f[40:42] == b"\0\0"
    p = U.patch(f)
    assert p[:40] == f[:40] and p[42:] == f[42:] and p[40:42] != b"\0\0"
    flip = bytearray(p)
    flip[-1 if L else 37] ^= 0x10
    assert U.rx_csum_states([f, p, bytes(flip)]) == [abi.UDP_NONE, abi.UDP_OK, abi.UDP_BAD]


@pytest.mark.parametrize("L", [2, 22, 38, 40, 1458])
def test_zero_sum_goes_out_as_ffff(L):
    """A payload whose last word makes the complemented sum 0: the field is 0xFFFF, and the
    oracle's RX accepts that form."""
    f = _frame(L, seed=7)
    f = f[:-2] + U.zero_sum_word(f)
    assert U.rfc768_sum(f) == 0xFFFF and U.rfc768_cksum(f) == 0xFFFF
    p = U.patch(f)
    assert p[40:42] == b"\xff\xff"
    assert U.rx_csum_states([p]) == [abi.UDP_OK]


@pytest.mark.parametrize("L,mtu", [(1458, 1500), (1459, 1500), (2952, 1500), (100, 68)])
def test_fragment_zero_carries_the_field(L, mtu):
    """O.tx_fragment copies the patched field into fragment 0 (frame bytes 40-41) and changes
    nothing else against the unpatched datagram's fragments."""
    f = _frame(L, seed=3)
    p = U.patch(f)
    a = O.tx_fragment(f, mtu) if len(f) > mtu else [f]
    b = O.tx_fragment(p, mtu) if len(p) > mtu else [p]
    assert len(a) == len(b)
    assert b[0][40:42] == p[40:42] and b[0][:40] == a[0][:40] and b[0][42:] == a[0][42:]
    assert a[1:] == b[1:]


def test_expected_uses_the_header_source_address():
    """The pseudo-header's source is the address the IPv4 header carries: the slot's when bound
    to a specific address, else the configuration's."""
    for slot in [(0, 10000, 1), (abi.raw_ip("10.1.2.3"), 5353, 1), (abi.raw_ip("10.9.9.9"), 7, 0)]:
        blob, frames = U.expected(SRC_MAC, DST_MAC, SRC_IP, slot, abi.raw_ip("172.31.100.1"), 0x1127, b"abcde")
        want_src = slot[0] if slot[2] and slot[0] else SRC_IP
        assert int.from_bytes(blob[26:30], "little") == want_src
        assert U.rx_csum_states(frames) == [abi.UDP_OK]


def test_new_symbols_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in ("udpdk_gpu_tx_build_flags", "udpdk_config_tx_cksum"):
        assert name in exported and name in abi.declared_symbols()
        assert getattr(abi.lib(), name).argtypes is not None
    assert abi.TX_UDP_CKSUM == 1
    assert abi.lib().udpdk_gpu_abi_version() == 3


def test_tx_build_flags_null_arguments():
    L = abi.lib()
    cfg, bt, ot = abi.TxConfig(), abi.TxBatch(), abi.TxOut()
    for flags in (0, abi.TX_UDP_CKSUM, 2):
        assert L.udpdk_gpu_tx_build_flags(None, C.byref(cfg), C.byref(bt), C.byref(ot), 0, flags) == -errno.EINVAL
    assert L.udpdk_gpu_tx_build_flags(None, None, None, None, 1500, abi.TX_UDP_CKSUM) == -errno.EINVAL


def test_config_tx_cksum_round_trips(host_api):
    """Off by default; the call returns the previous setting, a negative argument only reads,
    anything above 1 is rejected, and udpdk_host_reset turns it off again."""
    assert host_api.config_tx_cksum(-1) == 0
    assert host_api.config_tx_cksum(1) == 0
    assert host_api.config_tx_cksum(-1) == 1
    assert host_api.config_tx_cksum(2) == -1 and host_api.errno() == errno.EINVAL
    assert host_api.config_tx_cksum(-1) == 1
    assert host_api.config_tx_cksum(0) == 1
    assert host_api.config_tx_cksum(-1) == 0
    host_api.config_tx_cksum(1)
    host_api.reset()
    assert host_api.config_tx_cksum(-1) == 0
