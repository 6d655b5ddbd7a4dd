/*
 * igmp_frame.h — the IGMPv2 frames the host builds itself: the unsolicited membership report of a
 * join and the leave of the last drop (RFC 2236), byte for byte what the device writes in answer to
 * a query (igmp_reply.hip). Header-only and free of the library's state so that it can be tested
 * alone (tools/igmp_frame_check.c).
 */
#ifndef UDPDK_IGMP_FRAME_H
#define UDPDK_IGMP_FRAME_H

#include <stdint.h>
#include <string.h>

#define H_IGMP_FRAME_BYTES 46u           /* UDPDK_IGMP_FRAME_BYTES: 14 Ethernet + 24 IPv4 + 8 IGMP */
#define H_IGMP_REPORT 0x16u              /* version 2 membership report, sent to the group */
#define H_IGMP_LEAVE  0x17u              /* leave group, sent to 224.0.0.2 */
#define H_IGMP_ALL_HOSTS   0x010000E0u   /* 224.0.0.1, raw */
#define H_IGMP_ALL_ROUTERS 0x020000E0u   /* 224.0.0.2, raw */

/* the RFC 1071 checksum of n bytes (n even), as the two bytes to store */
static inline void h_igmp_cksum(const uint8_t *p, uint32_t n, uint8_t out[2])
{
    uint32_t s = 0;
    for (uint32_t k = 0; k < n; k += 2) s += (uint32_t)p[k] << 8 | p[k + 1];
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    s = ~s & 0xFFFFu;
    out[0] = (uint8_t)(s >> 8);
    out[1] = (uint8_t)s;
}

/* out[0, 46): 01 00 5e + the destination's low 23 bits, mac, 08 00,
 * 46 c0 00 20 00 00 40 00 01 02 <cksum> <src> <dst> 94 04 00 00 (Router Alert), <type> 00 <cksum> <group>.
 * A report goes to the group, a leave to 224.0.0.2 (addresses raw: as on the wire). */
static inline void h_igmp_build(uint8_t out[H_IGMP_FRAME_BYTES], const uint8_t mac[6], uint32_t src_raw,
                                uint32_t type, uint32_t group_raw)
{
    static const uint8_t ip0[10] = {0x46, 0xC0, 0x00, 0x20, 0x00, 0x00, 0x40, 0x00, 0x01, 0x02};
    static const uint8_t ra[4] = {0x94, 0x04, 0x00, 0x00};
    const uint32_t dst_raw = type == H_IGMP_LEAVE ? H_IGMP_ALL_ROUTERS : group_raw;
    uint8_t d[4];
    memcpy(d, &dst_raw, 4);
    out[0] = 0x01; out[1] = 0x00; out[2] = 0x5E;
    out[3] = d[1] & 0x7F; out[4] = d[2]; out[5] = d[3];
    memcpy(out + 6, mac, 6);
    out[12] = 0x08; out[13] = 0x00;
    memcpy(out + 14, ip0, 10);
    out[24] = out[25] = 0;
    memcpy(out + 26, &src_raw, 4);
    memcpy(out + 30, d, 4);
    memcpy(out + 34, ra, 4);
    h_igmp_cksum(out + 14, 24, out + 24);
    out[38] = (uint8_t)type; out[39] = 0; out[40] = out[41] = 0;
    memcpy(out + 42, &group_raw, 4);
    h_igmp_cksum(out + 38, 8, out + 40);
}

#endif
