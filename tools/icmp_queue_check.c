/*
 * icmp_queue_check — the host ICMP queue (udpdk_amd/csrc/host/icmp_queue.h) behind a main(): host
 * code only, links no project library, runs on a machine without a GPU (tests/test_icmp_ref.py).
 * `make icmp-asan` builds the same program under the address and undefined-behaviour sanitizers.
 *
 * stdin, one command per line:
 *   init CAP          a queue with a byte ring of CAP bytes
 *   push LEN SEED     a frame of LEN bytes, byte j = (SEED + j) & 0xff        -> "push RC"
 *   drain MAX CAP     udpdk_tx_drain's loop with these limits                   -> "drain N LEN:SEED ..."
 *                     (SEED read back from the frame; "bad" if a byte is wrong)
 *   reset                                                                       -> "reset"
 *   stat                                                                        -> "stat COUNT DROPPED"
 * The drain's output arrays are heap blocks of exactly the size the call may touch.
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host/icmp_queue.h"

int main(void)
{
    static struct h_icmpq q;
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "init")) {
            unsigned cap;
            if (scanf("%u", &cap) != 1) return 3;
            if (h_icmpq_init(&q, cap)) return 2;
            q.dropped = 0;
            printf("init\n");
        } else if (!strcmp(cmd, "push")) {
            unsigned len, seed;
            if (scanf("%u %u", &len, &seed) != 2) return 3;
            uint8_t *f = malloc(len ? len : 1);
            if (!f) return 2;
            for (unsigned j = 0; j < len; j++) f[j] = (uint8_t)(seed + j);
            printf("push %d\n", h_icmpq_push(&q, f, len));
            free(f);
        } else if (!strcmp(cmd, "drain")) {
            unsigned max;
            unsigned long long cap;
            if (scanf("%u %llu", &max, &cap) != 2) return 3;
            uint8_t *out = malloc(cap ? cap : 1);
            uint32_t *off = malloc(sizeof(*off) * (max ? max : 1));
            uint16_t *len = malloc(sizeof(*len) * (max ? max : 1));
            if (!out || !off || !len) return 2;
            uint32_t k = 0;
            uint64_t bytes = 0;
            h_icmpq_drain(&q, out, cap, off, len, max, &k, &bytes);
            printf("drain %" PRIu32, k);
            uint64_t pos = 0;
            for (uint32_t i = 0; i < k; i++) {
                int ok = off[i] == pos;
                for (uint32_t j = 0; j < len[i]; j++) ok = ok && out[off[i] + j] == (uint8_t)(out[off[i]] + j);
                if (ok) printf(" %u:%u", (unsigned)len[i], (unsigned)out[off[i]]);
                else printf(" bad");
                pos += len[i];
            }
            printf("%s\n", pos == bytes ? "" : " badbytes");
            free(out); free(off); free(len);
        } else if (!strcmp(cmd, "reset")) {
            h_icmpq_reset(&q);
            printf("reset\n");
        } else if (!strcmp(cmd, "stat")) {
            printf("stat %" PRIu32 " %" PRIu64 "\n", q.count, q.dropped);
        } else {
            return 3;
        }
    }
    h_icmpq_free(&q);
    return 0;
}
