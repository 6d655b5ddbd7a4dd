/*
 * echo_expand_check — the host half of udpdk_poll_echo's output format (udpdk_amd/csrc/host/
 * echo_expand.h) behind a main(): host code only, links no project library, runs on a machine
 * without a GPU (tests/test_tx_reply_ref.py). `make echo-asan` builds the same program under the
 * address and undefined-behaviour sanitizers.
 *
 * stdin, one case per line:  mtu max out_bytes count  then count triples  payload_len sockfd frame_off
 * stdout, one line per case: rc n_frames  then, when rc is 0, n_frames pairs off:len
 * Every array is a heap block of exactly the size the function may touch.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "host/echo_expand.h"

int main(void)
{
    unsigned mtu, max, count;
    unsigned long long out_bytes;
    while (scanf("%u %u %llu %u", &mtu, &max, &out_bytes, &count) == 4) {
        uint16_t *len = malloc(sizeof(*len) * (count ? count : 1));
        int32_t *sock = malloc(sizeof(*sock) * (count ? count : 1));
        uint32_t *foff = malloc(sizeof(*foff) * (count ? count : 1));
        uint32_t *off = malloc(sizeof(*off) * (max ? max : 1));
        uint16_t *ol = malloc(sizeof(*ol) * (max ? max : 1));
        if (!len || !sock || !foff || !off || !ol) return 2;
        for (unsigned k = 0; k < count; k++) {
            unsigned l, f;
            int s;
            if (scanf("%u %d %u", &l, &s, &f) != 3) return 3;
            len[k] = (uint16_t)l;
            sock[k] = s;
            foff[k] = f;
        }
        uint32_t nf = 0;
        const int rc = h_echo_expand(len, sock, foff, count, mtu, out_bytes, max, off, ol, &nf);
        printf("%d %" PRIu32, rc, nf);
        for (uint32_t j = 0; rc == 0 && j < nf; j++) printf(" %" PRIu32 ":%u", off[j], (unsigned)ol[j]);
        printf("\n");
        free(len); free(sock); free(foff); free(off); free(ol);
    }
    return 0;
}
