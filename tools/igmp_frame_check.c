/*
 * igmp_frame_check — the host's IGMP report and leave builder (udpdk_amd/csrc/host/igmp_frame.h)
 * behind a main(): host code only, links no project library, runs on a machine without a GPU
 * (tests/test_mcast_ref.py). `make igmp-asan` builds the same program under the address and
 * undefined-behaviour sanitizers.
 *
 *   igmp_frame_check report|leave MAC IP GROUP     MAC as aa:bb:cc:dd:ee:ff, addresses dotted
 *                                                  -> the 46 bytes as hex on one line
 * The frame is built into a heap block of exactly 46 bytes.
 */
#include <stdio.h>
#include <stdlib.h>

#include "host/igmp_frame.h"

static int quad(const char *s, uint32_t *raw)
{
    unsigned a[4];
    if (sscanf(s, "%u.%u.%u.%u", &a[0], &a[1], &a[2], &a[3]) != 4) return -1;
    uint8_t b[4];
    for (int i = 0; i < 4; i++) b[i] = (uint8_t)a[i];
    memcpy(raw, b, 4);
    return 0;
}

int main(int argc, char **argv)
{
    unsigned m[6];
    uint32_t ip, group;
    if (argc != 5 || (strcmp(argv[1], "report") && strcmp(argv[1], "leave")) ||
        sscanf(argv[2], "%x:%x:%x:%x:%x:%x", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5]) != 6 || quad(argv[3], &ip) ||
        quad(argv[4], &group))
        return 3;
    uint8_t mac[6];
    for (int i = 0; i < 6; i++) mac[i] = (uint8_t)m[i];
    uint8_t *f = malloc(H_IGMP_FRAME_BYTES);
    if (!f) return 2;
    h_igmp_build(f, mac, ip, argv[1][0] == 'l' ? H_IGMP_LEAVE : H_IGMP_REPORT, group);
    for (unsigned i = 0; i < H_IGMP_FRAME_BYTES; i++) printf("%02x", f[i]);
    printf("\n");
    free(f);
    return 0;
}
