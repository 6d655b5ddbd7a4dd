"""The expected image of a datagram sent with UDPDK_TX_UDP_CKSUM, for test_tx_cksum_ref.py and
test_gpu_tx_cksum.py: O.tx_frame's frame, bytes 40-41 patched with the RFC 768 checksum computed
here from the frame's own bytes (big-endian words, no code shared with the library or the
oracle), then O.tx_fragment when an MTU is set."""
import numpy as np

import oracle as O
from udpdk_amd import abi


def _fold(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def rfc768_sum(frame: bytes) -> int:
    """One's-complement sum, folded, of what the UDP checksum of an unfragmented Eth/IPv4/UDP
    frame covers, the checksum field taken as zero: pseudo-header (source and destination
    address, zero, protocol 17, UDP length), UDP header, payload zero-padded to even length."""
    udp = bytearray(frame[34:])
    ulen = (udp[4] << 8) | udp[5]
    assert ulen == len(udp) and frame[23] == 17
    udp[6:8] = b"\0\0"
    data = frame[26:34] + bytes([0, 17]) + bytes(udp[4:6]) + bytes(udp) + (b"\0" if ulen & 1 else b"")
    return _fold(int(np.frombuffer(data, ">u2").astype(np.uint64).sum()))


def rfc768_cksum(frame: bytes) -> int:
    """The checksum field's value as transmitted: the complement, 0 sent as 0xFFFF."""
    return (~rfc768_sum(frame) & 0xFFFF) or 0xFFFF


def patch(frame: bytes) -> bytes:
    c = rfc768_cksum(frame)
    return frame[:40] + bytes([c >> 8, c & 0xFF]) + frame[42:]


def zero_sum_word(frame: bytes) -> bytes:
    """For a frame with an even payload of >= 2 bytes: the value of the payload's last 16-bit
    word that makes the complemented sum 0 (so 0xFFFF goes on the wire)."""
    assert len(frame) >= 44 and len(frame) % 2 == 0
    s = rfc768_sum(frame[:-2] + b"\0\0")              # 1 .. 0xFFFF: the pseudo-header is not zero
    x = 0xFFFF - s
    return bytes([x >> 8, x & 0xFF])


def expected(src_mac, dst_mac, cfg_ip, slot, dst_ip, dst_port, payload: bytes, mtu=None, cksum=True):
    """(the datagram's output bytes, its frames): slot = (ip, port, bound)."""
    ip, port, bound = slot
    frame = O.tx_frame(src_mac, dst_mac, cfg_ip, bound, ip, port, dst_ip, dst_port, payload)
    if cksum:
        frame = patch(frame)
    frames = O.tx_fragment(frame, mtu) if mtu and len(frame) > mtu else [frame]
    return b"".join(frames), frames


def rx_csum_states(frames: list[bytes]) -> list[int]:
    """O.rx's UDP checksum state (verdict-word bits 5-6) of each frame, no bindings needed."""
    off = np.cumsum([0] + [len(f) for f in frames[:-1]]).astype(np.uint32)
    ln = np.array([len(f) for f in frames], np.uint16)
    buf = np.frombuffer(b"".join(frames) + b"\0" * 16, np.uint8).copy()
    meta = O.rx(O.BindTable(), buf, len(buf) - 16, off, ln, None, 1)[0]
    return [int(x) for x in abi.meta_udp(meta)]
