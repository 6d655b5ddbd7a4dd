/* rss_host_check — prints the hash the host computes for a frame, on a machine without a GPU:
 * rss_host.h's key-window table builder and per-frame hash behind a main(), no HIP call, no
 * project library (tests/test_rss_host.py compares the output with an independent reference).
 *
 * Rows on stdin, one per line, `#` starts a comment:
 *   <key: 80 hex digits> <types: 0-3> <ptype: - to derive it, or a number> [<frame bytes in hex>]
 *     -> the hash, 8 hex digits
 * A row without the last field is a frame of length 0. The frame is copied into an allocation of
 * exactly its length, so a sanitizer build sees any read past it. The table is rebuilt when the
 * key differs from the previous row's. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

#include "rss_host.h"

static int hexval(int c)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

/* s[0, 2 n) -> out[0, n); 0 on success */
static int unhex(const char *s, size_t n, uint8_t *out)
{
    for (size_t i = 0; i < n; i++) {
        const int a = hexval(s[2 * i]), b = hexval(s[2 * i + 1]);
        if (a < 0 || b < 0) return -1;
        out[i] = (uint8_t)(a * 16 + b);
    }
    return 0;
}

static int bad(const char *why, const char *line)
{
    fprintf(stderr, "rss_host_check: %s: %.100s\n", why, line);
    return 2;
}

int main(void)
{
    static uint32_t tab[12][256];
    uint8_t key[40], have[40];
    int have_key = 0;
    char *line = NULL;
    size_t cap = 0;
    ssize_t got;
    while ((got = getline(&line, &cap, stdin)) >= 0) {
        char *hash = strchr(line, '#');
        if (hash) *hash = 0;
        char *save = NULL;
        char *w[4];
        int nw = 0;
        for (char *t = strtok_r(line, " \t\r\n", &save); t && nw < 4; t = strtok_r(NULL, " \t\r\n", &save)) w[nw++] = t;
        if (!nw) continue;
        if (nw < 3) return bad("bad row", line);
        if (strlen(w[0]) != 80 || unhex(w[0], 40, key)) return bad("bad key", w[0]);
        const uint32_t types = (uint32_t)strtoul(w[1], NULL, 0);
        uint32_t ptype = 0;
        const int derive = !strcmp(w[2], "-");
        if (!derive) ptype = (uint32_t)strtoul(w[2], NULL, 0);
        const size_t hexlen = nw > 3 ? strlen(w[3]) : 0;
        if (hexlen & 1) return bad("odd frame hex", w[3]);
        const size_t len = hexlen / 2;
        uint8_t *f = malloc(len ? len : 1);
        if (!f) return 3;
        if (len && unhex(w[3], len, f)) {
            free(f);
            return bad("bad frame hex", w[3]);
        }
        if (!have_key || memcmp(have, key, 40)) {
            rss_key_table(key, tab);
            memcpy(have, key, 40);
            have_key = 1;
        }
        const uint32_t (*T)[256] = tab;
        printf("%08x\n", rss_frame_hash(f, (uint32_t)len, derive ? NULL : &ptype, types, T));
        free(f);
    }
    free(line);
    return 0;
}
