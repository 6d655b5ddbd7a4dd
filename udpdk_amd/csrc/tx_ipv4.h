// tx_ipv4.h — the IPv4 header sum and checksum every frame this stack sends is built with (tx_build,
// icmp_build). Device-only, inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave.h"

namespace udpdk {

// Sum of the 20-byte IPv4 header the TX kernels build (checksum field zero) as LE 16-bit words:
// version/IHL 0x45, tos 0, total length tl, id 0, fragment field ff (host order), ttl 64,
// protocol (17 unless given), src, dst (raw).
__device__ __forceinline__ uint32_t ipv4_raw(uint32_t tl, uint32_t ff, uint32_t src, uint32_t dst,
                                             uint32_t proto = 17u)
{
    uint32_t s = 0x0045u + bswap16(tl) + bswap16(ff) + (0x0040u | (proto << 8)) + (src & 0xFFFFu) + (src >> 16) +
                 (dst & 0xFFFFu) + (dst >> 16);
    s = (s >> 16) + (s & 0xFFFFu);
    s = (s >> 16) + (s & 0xFFFFu);
    return s & 0xFFFFu;
}

// rte_ipv4_cksum of DPDK 20.05: raw == 0xffff is returned unchanged.
__device__ __forceinline__ uint32_t ipv4_cksum(uint32_t raw) { return raw == 0xFFFFu ? raw : (~raw & 0xFFFFu); }

// The checksum a NIC computes for PKT_TX_IP_CKSUM (fragments, rte_ipv4_fragment_packet leaves 0).
__device__ __forceinline__ uint32_t ipv4_cksum_nic(uint32_t raw) { return ~raw & 0xFFFFu; }

} // namespace udpdk
