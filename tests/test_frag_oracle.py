"""CPU checks of the TX fragmentation restatement (oracle_tx_fragment, the poller's
udpdk_poller.c:461-501 + DPDK 20.05 rte_ipv4_fragment_packet) and of the span helper the GPU
path's callers use. DPDK is not in the container and the reference holds no fragment vectors, so
the fragment bytes are pinned by restatement only ("parity unpinned" beyond the properties below:
an independent pure-Python restatement of one case, reassembly round trips, header checksums)."""
import numpy as np
import pytest

import oracle as O
from udpdk_amd import abi

SRC_MAC = bytes.fromhex("6805ca95f8ec")
DST_MAC = bytes.fromhex("6805ca95fa64")
SRC_IP = abi.raw_ip("172.31.100.2")
DST_IP = abi.raw_ip("172.31.100.1")


def _sum16(b):
    s = sum(b[i] | (b[i + 1] << 8) for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def _frame(L, seed=0):
    pay = bytes((i * 13 + seed) & 0xFF for i in range(L))
    return O.tx_frame(SRC_MAC, DST_MAC, SRC_IP, 1, 0, abi.raw_port(10000), DST_IP,
                      abi.raw_port(10001), pay), pay


@pytest.mark.parametrize("mtu", [1500, 1020, 68])
@pytest.mark.parametrize("L", [0, 1, 1457, 1458, 1459, 1472, 1473, 2006, 2952, 2953, 9000, 65507])
def test_fragment_round_trip(L, mtu):
    fr, pay = _frame(L, L)
    frags = O.tx_fragment(fr, mtu)
    span = abi.lib().udpdk_gpu_tx_span(L, mtu, None)
    assert sum(len(f) for f in frags) == span
    if len(fr) <= mtu:
        assert frags == [fr]
        return
    fpl = mtu - 20
    assert len(frags) == -(-(L + 8) // fpl)
    ip_payload = bytearray()
    for k, f in enumerate(frags):
        assert f[:14] == fr[:14]
        h = f[14:34]
        assert _sum16(h) == 0xFFFF                              # the NIC-filled checksum verifies
        assert h[0] == 0x45 and h[8] == 64 and h[9] == 17 and h[4:6] == b"\0\0"
        assert h[12:20] == fr[26:34]
        tl = (h[2] << 8) | h[3]
        assert tl == len(f) - 14
        fo = (h[6] << 8) | h[7]
        assert (fo & 0x1FFF) * 8 == len(ip_payload)
        assert bool(fo & 0x2000) == (k + 1 < len(frags)) and not fo & 0x4000
        if k + 1 < len(frags):
            assert tl - 20 == fpl
        ip_payload += f[34:]
    assert bytes(ip_payload) == fr[34:]                         # UDP header + payload


# the lengths tests/test_gpu_tx_edges.py compares the GPU with the oracle at, per MTU
MTU_EDGES = {68: list(range(121)) + [1000],
             572: [529, 530, 531, 544, 545, 1096, 1097],
             65532: [65490, 65491, 65507]}


@pytest.mark.parametrize("mtu", sorted(MTU_EDGES))
def test_fragment_mtu_edges(mtu):
    """The ends of the MTU range (68, 65532) and a small one between, rebuilt from the inputs with
    no oracle in between: the fragments' IPv4 payloads concatenate to the UDP header + payload,
    every fragment header sums to 0xFFFF (RFC 1071), MF is set on all but the last, the fragment
    offsets are contiguous, and fragment k starts k * (mtu + 14) bytes into the span."""
    fpl = mtu - 20
    for L in MTU_EDGES[mtu]:
        fr, pay = _frame(L, L)
        frags = O.tx_fragment(fr, mtu)
        blob = b"".join(frags)
        assert len(blob) == abi.lib().udpdk_gpu_tx_span(L, mtu, None)
        if L + 42 <= mtu:
            assert blob == fr and fr[42:] == pay
            continue
        ipp = fr[34:42] + pay
        assert fr[38:40] == (L + 8).to_bytes(2, "big") and fr[40:42] == b"\0\0"
        nf = -(-len(ipp) // fpl)
        assert len(frags) == nf
        off = 0
        for k in range(nf):
            m = min(fpl, len(ipp) - off)
            f = blob[k * (mtu + 14):k * (mtu + 14) + 34 + m]
            assert f == frags[k]
            h = f[14:34]
            assert _sum16(h) == 0xFFFF
            assert (h[2] << 8 | h[3]) == 20 + m
            ff = h[6] << 8 | h[7]
            assert (ff & 0x1FFF) * 8 == off and bool(ff & 0x2000) == (k + 1 < nf) and not ff & 0xC000
            assert f[34:] == ipp[off:off + m]
            off += m
        assert off == len(ipp)


def test_mtu_576_is_no_mtu_of_the_abi():
    """576 - 20 is no multiple of 8 (fragment offsets count 8-byte units): the span helper treats
    it like every MTU udpdk_gpu_tx_build_mtu rejects, one unfragmented frame."""
    n = abi.C.c_uint32()
    for L in (533, 534, 535, 548, 549, 1104, 1105):
        assert abi.lib().udpdk_gpu_tx_span(L, 576, abi.C.byref(n)) == L + 42 and n.value == 1


def test_fragment_known_answer_2006():
    """Independent restatement of one case: the largest sendto that fits a 2048 B mbuf
    (RTE_MBUF_DEFAULT_BUF_SIZE data room, udpdk_init.c:78-99) at IPV4_MTU_DEFAULT."""
    fr, pay = _frame(2006)
    frags = O.tx_fragment(fr, 1500)
    assert [len(f) for f in frags] == [1514, 34 + 534]

    def hdr(tl, fo):
        h = bytearray.fromhex("4500") + tl.to_bytes(2, "big") + b"\0\0" + fo.to_bytes(2, "big") + \
            bytes([64, 17, 0, 0]) + fr[26:34]
        ck = (~_sum16(h)) & 0xFFFF
        h[10:12] = ck.to_bytes(2, "little")
        return bytes(h)
    assert frags[0] == fr[:14] + hdr(1500, 0x2000) + fr[34:34 + 1480]
    assert frags[1] == fr[:14] + hdr(554, 185) + fr[34 + 1480:]


def test_span_helper():
    n = abi.C.c_uint32()
    assert abi.lib().udpdk_gpu_tx_span(1458, 1500, abi.C.byref(n)) == 1500 and n.value == 1
    assert abi.lib().udpdk_gpu_tx_span(1459, 1500, abi.C.byref(n)) == 1501 and n.value == 1
    assert abi.lib().udpdk_gpu_tx_span(1473, 1500, abi.C.byref(n)) == 1481 + 68 and n.value == 2
    assert abi.lib().udpdk_gpu_tx_span(65507, 1500, abi.C.byref(n)) == 65515 + 34 * 45 and n.value == 45
    assert abi.lib().udpdk_gpu_tx_span(3000, 0, abi.C.byref(n)) == 3042 and n.value == 1
