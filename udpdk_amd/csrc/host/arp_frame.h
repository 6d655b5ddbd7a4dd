/*
 * arp_frame.h — the one ARP frame the host builds itself: the RFC 5227 §2.3 announcement (a request
 * whose sender and target protocol addresses are both ours, broadcast). Header-only and free of the
 * library's state so that it can be tested alone (tools/arp_frame_check.c). The replies are built on
 * the device (arp_reply.hip).
 */
#ifndef UDPDK_ARP_FRAME_H
#define UDPDK_ARP_FRAME_H

#include <stdint.h>
#include <string.h>

#define H_ARP_FRAME_BYTES 42u            /* UDPDK_ARP_FRAME_BYTES: 14 Ethernet + 28 ARP */

/* out[0, 42): ff x 6, mac, 08 06 00 01 08 00 06 04 00 01, mac, ip, 00 x 6, ip (ip raw: as on the wire) */
static inline void h_arp_announce_build(uint8_t out[H_ARP_FRAME_BYTES], const uint8_t mac[6], uint32_t ip_raw)
{
    static const uint8_t hdr[10] = {0x08, 0x06, 0x00, 0x01, 0x08, 0x00, 0x06, 0x04, 0x00, 0x01};
    memset(out, 0xFF, 6);
    memcpy(out + 6, mac, 6);
    memcpy(out + 12, hdr, 10);
    memcpy(out + 22, mac, 6);
    memcpy(out + 28, &ip_raw, 4);
    memset(out + 32, 0, 6);
    memcpy(out + 38, &ip_raw, 4);
}

#endif
