/*
 * arp_frame_check — the host's ARP announcement builder (udpdk_amd/csrc/host/arp_frame.h) behind a
 * main(): host code only, links no project library, runs on a machine without a GPU
 * (tests/test_arp_ref.py). `make arp-asan` builds the same program under the address and
 * undefined-behaviour sanitizers.
 *
 *   arp_frame_check MAC IP     MAC as aa:bb:cc:dd:ee:ff, IP dotted -> the 42 bytes as hex on one line
 * The frame is built into a heap block of exactly 42 bytes.
 */
#include <stdio.h>
#include <stdlib.h>

#include "host/arp_frame.h"

int main(int argc, char **argv)
{
    unsigned m[6], a[4];
    if (argc != 3 || sscanf(argv[1], "%x:%x:%x:%x:%x:%x", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5]) != 6 ||
        sscanf(argv[2], "%u.%u.%u.%u", &a[0], &a[1], &a[2], &a[3]) != 4)
        return 3;
    uint8_t mac[6], ipb[4];
    for (int i = 0; i < 6; i++) mac[i] = (uint8_t)m[i];
    for (int i = 0; i < 4; i++) ipb[i] = (uint8_t)a[i];
    uint32_t ip;
    memcpy(&ip, ipb, 4);
    uint8_t *f = malloc(H_ARP_FRAME_BYTES);
    if (!f) return 2;
    h_arp_announce_build(f, mac, ip);
    for (unsigned i = 0; i < H_ARP_FRAME_BYTES; i++) printf("%02x", f[i]);
    printf("\n");
    free(f);
    return 0;
}
