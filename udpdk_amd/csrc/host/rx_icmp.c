/*
 * rx_icmp.c — the socket layer's ICMP answers: udpdk_config_icmp / udpdk_config_icmp_burst /
 * udpdk_icmp_counts, and the stage udpdk_poll_rx runs after a batch's RX when flags are set
 * (udpdk_gpu_icmp_reply on the staged device batch, the built frames copied back and appended to the
 * host ICMP queue that udpdk_tx_drain empties first). The reference has no ICMP; off by default.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_state.h"

#define H_ICMP_OUT_MIN (1u << 20)        /* first size of the device output; grown to bytes_needed */

int udpdk_config_icmp(int flags)
{
    const int was = (int)g_udpdk.icmp_flags;
    if (flags < 0) return was;
    if ((uint32_t)flags & ~UDPDK_ICMP_ALL) { errno = EINVAL; return -1; }
    if (flags && g_udpdk.n_shards > 1) { errno = ENOTSUP; return -1; }   /* sharded polls: not answered */
    g_udpdk.icmp_flags = (uint32_t)flags;
    return was;
}

int udpdk_config_icmp_burst(int n)
{
    const int was = g_udpdk.icmp_burst;
    if (n >= -1) g_udpdk.icmp_burst = n;     /* below -1: only reads */
    return was;
}

int udpdk_icmp_counts(udpdk_icmp_counts_t *c)
{
    if (!c) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    *c = g_udpdk.icmp_counts;
    c->queue_dropped = g_udpdk.icmpq.dropped;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

void h_icmp_reset(void)                   /* under tx_lock */
{
    h_icmpq_reset(&g_udpdk.icmpq);
    g_udpdk.icmpq.dropped = 0;
    memset(&g_udpdk.icmp_counts, 0, sizeof(g_udpdk.icmp_counts));
}

void h_icmp_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.ic_out_d && g) udpdk_gpu_free(g, g_udpdk.ic_out_d);
    if (g_udpdk.ic_idx_d && g) udpdk_gpu_free(g, g_udpdk.ic_idx_d);
    if (g_udpdk.ic_h && g) udpdk_gpu_host_free(g, g_udpdk.ic_h);
    g_udpdk.ic_out_d = g_udpdk.ic_idx_d = g_udpdk.ic_h = NULL;
    g_udpdk.ic_out_d_cap = g_udpdk.ic_idx_d_cap = g_udpdk.ic_h_cap = 0;
    pthread_mutex_lock(&g_udpdk.tx_lock);
    h_icmp_reset();
    h_icmpq_free(&g_udpdk.icmpq);
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

/* The errors one poll may still answer: [gpu] icmp_burst at the start of a poll (rx_poll.c). */
uint32_t h_icmp_budget(void)
{
    return g_udpdk.icmp_burst < 0 ? 0xFFFFFFFFu : (uint32_t)g_udpdk.icmp_burst;
}

/* The stage for one staged batch (pipe 0: the one-piece poll on the context stream; 1 .. 3: a chunk
 * on its pipe, whose RX has completed). Synchronous: the replies are queued when it returns.
 * *budget: the errors the poll may still answer; what this batch answered is taken off it, so the
 * limit counts across the chunks of one poll (they run this stage one after another, in order).
 * Returns 0, or -1 with errno. */
int h_icmp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev,
                 uint32_t *budget)
{
    const uint32_t flags = g_udpdk.icmp_flags, n = b->n;
    if (!flags || !n) return 0;
    int rc;
    const uint64_t o_org = ((4ull * n + 4) + 15u) & ~15ull;
    if (h_grow_dev(&g_udpdk.ic_idx_d, &g_udpdk.ic_idx_d_cap, o_org + 4ull * n + 16) ||
        h_grow_dev(&g_udpdk.ic_out_d, &g_udpdk.ic_out_d_cap, H_ICMP_OUT_MIN))
        return -1;
    udpdk_tx_config_t cfg;
    memcpy(cfg.src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg.dst_mac, g_udpdk.dst_mac, 6);
    cfg.src_ip = g_udpdk.src_ip;
    udpdk_icmp_stats_t st;
    for (int attempt = 0;; attempt++) {
        uint64_t cap = g_udpdk.ic_out_d_cap & ~15ull;
        if (cap > 0xFFFFFFF0ull) cap = 0xFFFFFFF0ull;
        const udpdk_icmp_out_t o = {g_udpdk.ic_out_d, cap, (uint32_t *)g_udpdk.ic_idx_d,
                                    (uint32_t *)((uint8_t *)g_udpdk.ic_idx_d + o_org), n};
        if (pipe) {
            if ((rc = udpdk_gpu_pipe_icmp_reply(g, pipe, &cfg, b, meta_dev, flags, g_udpdk.mtu, *budget, &o)) ||
                (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
            rc = udpdk_gpu_pipe_icmp_stats(g, pipe, &st);
        } else {
            if ((rc = udpdk_gpu_icmp_reply(g, &cfg, b, meta_dev, flags, g_udpdk.mtu, *budget, &o))) { errno = -rc; return -1; }
            rc = udpdk_gpu_icmp_stats(g, &st);
        }
        if (rc == -ENOSPC && !attempt && st.bytes_needed <= 0xFFFFFFF0ull) {
            /* more reply bytes than the output holds: once more with what they need (meta is only
             * read, so the stage can run again) */
            if (h_grow_dev(&g_udpdk.ic_out_d, &g_udpdk.ic_out_d_cap, st.bytes_needed + 64)) return -1;
            continue;
        }
        if (rc) { errno = -rc; return -1; }
        break;
    }
    if (st.replies) {
        /* reply_off, then the frames (origin stays on the device: the queue keeps arrival order) */
        const uint64_t o_fr = ((4ull * st.replies + 4) + 15u) & ~15ull;
        if (h_grow_pinned(&g_udpdk.ic_h, &g_udpdk.ic_h_cap, o_fr + st.bytes_needed + 16)) return -1;
        uint8_t *h = g_udpdk.ic_h;
        if (pipe) {
            if ((rc = udpdk_gpu_pipe_d2h(g, pipe, h, g_udpdk.ic_idx_d, 4ull * st.replies + 4)) ||
                (rc = udpdk_gpu_pipe_d2h(g, pipe, h + o_fr, g_udpdk.ic_out_d, st.bytes_needed)) ||
                (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
        } else {
            if ((rc = udpdk_gpu_d2h(g, h, g_udpdk.ic_idx_d, 4ull * st.replies + 4)) ||
                (rc = udpdk_gpu_d2h(g, h + o_fr, g_udpdk.ic_out_d, st.bytes_needed)) ||
                (rc = udpdk_gpu_sync(g))) { errno = -rc; return -1; }
        }
        const uint32_t *ro = (const uint32_t *)h;
        pthread_mutex_lock(&g_udpdk.tx_lock);
        if (!g_udpdk.icmpq.buf && h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES)) {
            pthread_mutex_unlock(&g_udpdk.tx_lock);
            errno = ENOMEM;
            return -1;
        }
        for (uint32_t r = 0; r < st.replies; r++) {
            if (ro[r + 1] < ro[r] || ro[r + 1] > st.bytes_needed) break;     /* (never: the device's prefix) */
            (void)h_icmpq_push(&g_udpdk.icmpq, h + o_fr + ro[r], ro[r + 1] - ro[r]);
        }
        pthread_mutex_unlock(&g_udpdk.tx_lock);
    }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    g_udpdk.icmp_counts.echo_replied += st.echo_replied;
    g_udpdk.icmp_counts.unreach_sent += st.unreach_sent;
    g_udpdk.icmp_counts.echo_bad += st.echo_bad;
    g_udpdk.icmp_counts.limited += st.limited;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    if (*budget != 0xFFFFFFFFu) *budget -= st.unreach_sent < *budget ? st.unreach_sent : *budget;
    return 0;
}
