/* rss_host.h — the host side of receive-side scaling, stated once: the 12 x 256 key-window
 * table that rss_hash (rx_rss.hip) stages into LDS, and the per-frame hash by that table as the
 * host computes it for [gpu] dispatch = rss (rx_poll.c). Plain C, static inline, no project
 * state: udpdk_gpu_rss_config and h_rss_setup / h_rss_queue call these, and
 * tools/rss_host_check.c puts them behind a main() for a machine without a GPU
 * (tests/test_rss_host.py). */
#ifndef UDPDK_RSS_HOST_H
#define UDPDK_RSS_HOST_H

#include <stddef.h>
#include <stdint.h>

/* key bits [b, b + 32), MSB first, b < 96 (reads key bytes up to 15 of the 40) */
static inline uint32_t rss_key_window(const uint8_t *key, uint32_t b)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < 5; k++) w = (w << 8) | key[(b >> 3) + k];
    return (uint32_t)(w >> (8u - (b & 7u)));
}

/* tab[p][v] = XOR of the key windows at input bits 8 p + j over the set bits j, MSB first, of
 * byte value v at input position p: the Toeplitz hash of a 12-byte input is the XOR of 12 entries */
static inline void rss_key_table(const uint8_t *key, uint32_t tab[12][256])
{
    for (uint32_t p = 0; p < 12; p++)
        for (uint32_t v = 0; v < 256; v++) {
            uint32_t t = 0;
            for (uint32_t j = 0; j < 8; j++)
                if (v & (0x80u >> j)) t ^= rss_key_window(key, 8u * p + j);
            tab[p][v] = t;
        }
}

/* The hash of the frame f[0, len) (the caller has checked that it lies inside its buffer):
 * nothing (0) below 34 bytes or when the IPv4 gate rejects it (ptype given, else, with ptype =
 * NULL, derived from ether_type as rx_classify does); source + destination address + ports
 * (frame bytes [26, 38)) for unfragmented UDP of at least 38 bytes when types has
 * UDPDK_RSS_NONFRAG_IPV4_UDP (2); else the addresses (bytes [26, 34)) when types has
 * UDPDK_RSS_IPV4 (1); else 0. Fixed offsets, as the reference parses. */
static inline uint32_t rss_frame_hash(const uint8_t *f, uint32_t len, const uint32_t *ptype, uint32_t types,
                                      const uint32_t (*tab)[256])
{
    uint32_t hash = 0;
    if (len < 34u) return 0;
    const uint32_t pt = ptype ? *ptype : (f[12] == 0x08 && f[13] == 0x00 ? 0x211u : 0x1u);
    if (!(pt & 0x10u)) return 0;
    const uint32_t ff = ((uint32_t)f[20] << 8) | f[21];
    const int udp4 = !(ff & 0x3FFFu) && f[23] == 17 && len >= 38u && (types & 2u);
    if (udp4 || (types & 1u))
        for (uint32_t b = 0; b < (udp4 ? 12u : 8u); b++) hash ^= tab[b][f[26 + b]];
    return hash;
}

#endif
