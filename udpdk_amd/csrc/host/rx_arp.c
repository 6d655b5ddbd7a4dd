/*
 * rx_arp.c — the socket layer's ARP: udpdk_config_arp / udpdk_arp_announce / udpdk_arp_counts, and the
 * stage udpdk_poll_rx runs after a batch's RX when the switch is on and the batch held a frame that
 * is not IPv4 (udpdk_gpu_arp_reply on the staged device batch, the built replies copied back and
 * appended to the host queue that udpdk_tx_drain empties first, ahead of the batch's ICMP answers).
 * The reference has no ARP; off by default.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "arp_frame.h"
#include "host_state.h"

#define H_ARP_FIRST 32u                  /* slots copied back behind the stage, before the counts are known */
#define H_ARP_OUT_BYTES ((uint64_t)H_ICMPQ_FRAMES * UDPDK_ARP_SLOT_BYTES)

int udpdk_config_arp(int on)
{
    const int was = (int)g_udpdk.arp_on;
    if (on < 0) return was;
    if (on > 1) { errno = EINVAL; return -1; }
    if (on && g_udpdk.n_shards > 1) { errno = ENOTSUP; return -1; }   /* sharded polls: not answered */
    g_udpdk.arp_on = (uint32_t)on;
    return was;
}

int udpdk_arp_counts(udpdk_arp_counts_t *c)
{
    if (!c) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    *c = g_udpdk.arp_counts;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

void h_arp_reset(void)                    /* under tx_lock */
{
    memset(&g_udpdk.arp_counts, 0, sizeof(g_udpdk.arp_counts));
}

void h_arp_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.ar_out_d && g) udpdk_gpu_free(g, g_udpdk.ar_out_d);
    if (g_udpdk.ar_h && g) udpdk_gpu_host_free(g, g_udpdk.ar_h);
    g_udpdk.ar_out_d = g_udpdk.ar_h = NULL;
    g_udpdk.ar_out_d_cap = g_udpdk.ar_h_cap = 0;
    pthread_mutex_lock(&g_udpdk.tx_lock);
    h_arp_reset();
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

int udpdk_arp_announce(void)
{
    if (!g_udpdk.src_ip) { errno = EADDRNOTAVAIL; return -1; }
    uint8_t f[H_ARP_FRAME_BYTES];
    h_arp_announce_build(f, g_udpdk.src_mac, g_udpdk.src_ip);
    pthread_mutex_lock(&g_udpdk.tx_lock);
    int rc = !g_udpdk.icmpq.buf && h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES) ? -1 : 0;
    if (!rc) rc = h_icmpq_push(&g_udpdk.icmpq, f, H_ARP_FRAME_BYTES);
    if (!rc) g_udpdk.arp_counts.announced++;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    if (rc) { errno = ENOBUFS; return -1; }
    return 0;
}

/* The stage for one staged batch (pipe 0: the one-piece poll on the context stream; 1 .. 3: a chunk
 * on its pipe, whose RX has completed). not_ipv4: the batch's NOT_IPV4 verdict count; a batch of
 * pure IPv4 enqueues nothing. Synchronous: the replies are queued when it returns. The output is one
 * fixed allocation of H_ICMPQ_FRAMES slots (more could not be queued); the first H_ARP_FIRST come
 * back behind the stage in the same wait as the counts, the rest by a second copy.
 * Returns 0, or -1 with errno. */
int h_arp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_ipv4)
{
    if (!g_udpdk.arp_on || !b->n || !not_ipv4 || !g_udpdk.src_ip) return 0;
    int rc;
    /* the slots, then the origin entries (they stay on the device: the queue keeps arrival order) */
    if (h_grow_dev(&g_udpdk.ar_out_d, &g_udpdk.ar_out_d_cap, H_ARP_OUT_BYTES + 4ull * H_ICMPQ_FRAMES) ||
        h_grow_pinned(&g_udpdk.ar_h, &g_udpdk.ar_h_cap, H_ARP_OUT_BYTES))
        return -1;
    udpdk_tx_config_t cfg;
    memcpy(cfg.src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg.dst_mac, g_udpdk.dst_mac, 6);
    cfg.src_ip = g_udpdk.src_ip;
    uint8_t *out_d = g_udpdk.ar_out_d, *h = g_udpdk.ar_h;
    const udpdk_arp_out_t o = {out_d, (uint32_t *)(out_d + H_ARP_OUT_BYTES), H_ICMPQ_FRAMES};
    const uint64_t first = (uint64_t)H_ARP_FIRST * UDPDK_ARP_SLOT_BYTES;
    udpdk_arp_stats_t st;
    if (pipe) {
        if ((rc = udpdk_gpu_pipe_arp_reply(g, pipe, &cfg, b, meta_dev, &o)) ||
            (rc = udpdk_gpu_pipe_d2h(g, pipe, h, out_d, first)) ||
            (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
        rc = udpdk_gpu_pipe_arp_stats(g, pipe, &st);
    } else {
        if ((rc = udpdk_gpu_arp_reply(g, &cfg, b, meta_dev, &o)) ||
            (rc = udpdk_gpu_d2h(g, h, out_d, first))) { errno = -rc; return -1; }
        rc = udpdk_gpu_arp_stats(g, &st);
    }
    if (rc && rc != -ENOSPC) { errno = -rc; return -1; }     /* (-ENOSPC: the excess is no_room) */
    if (st.replies > H_ICMPQ_FRAMES) { errno = EIO; return -1; }
    if (st.replies > H_ARP_FIRST) {
        const uint64_t rest = (uint64_t)(st.replies - H_ARP_FIRST) * UDPDK_ARP_SLOT_BYTES;
        if (pipe) {
            if ((rc = udpdk_gpu_pipe_d2h(g, pipe, h + first, out_d + first, rest)) ||
                (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
        } else {
            if ((rc = udpdk_gpu_d2h(g, h + first, out_d + first, rest)) ||
                (rc = udpdk_gpu_sync(g))) { errno = -rc; return -1; }
        }
    }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    if (st.replies && !g_udpdk.icmpq.buf && h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES)) {
        pthread_mutex_unlock(&g_udpdk.tx_lock);
        errno = ENOMEM;
        return -1;
    }
    for (uint32_t r = 0; r < st.replies; r++)
        (void)h_icmpq_push(&g_udpdk.icmpq, h + (uint64_t)r * UDPDK_ARP_SLOT_BYTES, UDPDK_ARP_FRAME_BYTES);
    udpdk_arp_counts_t *c = &g_udpdk.arp_counts;
    c->scanned++;
    c->arp += st.arp;
    c->malformed += st.malformed;
    c->other_op += st.other_op;
    c->own += st.own;
    c->sender_bad += st.sender_bad;
    c->not_ours += st.not_ours;
    c->conflict += st.conflict;
    c->eligible += st.eligible;
    c->replies += st.replies;
    c->no_room += st.no_room;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}
