/*
 * neigh.c — the socket layer's neighbour cache: udpdk_config_neigh / udpdk_neigh_add / udpdk_neigh_flush /
 * udpdk_neigh_counts, the learn stage udpdk_poll_rx runs after a batch's RX when the switch is on and
 * the batch held a frame that is not IPv4 (udpdk_gpu_neigh_learn on the staged device batch, behind
 * the ARP replies and on the same pipe), and what udpdk_tx_drain needs to resolve its datagrams
 * (tx_drain.c: the configuration, the table, the work buffers, the counts). The table lives in the main
 * context and is created on first use; time is CLOCK_MONOTONIC in milliseconds. The reference has no
 * neighbour cache; off by default.
 */
#include <errno.h>
#include <string.h>
#include <time.h>

#include "host_state.h"

int udpdk_config_neigh(int mode)
{
    const int was = (int)g_udpdk.neigh_mode;
    if (mode < 0) return was;
    if (mode > UDPDK_NEIGH_MODE_FALLBACK) { errno = EINVAL; return -1; }
    if (mode && g_udpdk.n_shards > 1) { errno = ENOTSUP; return -1; }   /* sharded polls: nothing is learned */
    g_udpdk.neigh_mode = (uint32_t)mode;
    return was;
}

int udpdk_neigh_counts(udpdk_neigh_counts_t *c)
{
    if (!c) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    *c = g_udpdk.neigh_counts;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

void h_neigh_reset(void)                  /* under tx_lock */
{
    memset(&g_udpdk.neigh_counts, 0, sizeof(g_udpdk.neigh_counts));
}

void h_neigh_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.ng_d && g) udpdk_gpu_free(g, g_udpdk.ng_d);
    if (g_udpdk.ng_h && g) udpdk_gpu_host_free(g, g_udpdk.ng_h);
    g_udpdk.ng_d = g_udpdk.ng_h = NULL;
    g_udpdk.ng_d_cap = g_udpdk.ng_h_cap = 0;
    g_udpdk.neigh_ready = 0;              /* the table goes with the context */
    pthread_mutex_lock(&g_udpdk.tx_lock);
    h_neigh_reset();
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

uint32_t h_neigh_now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint32_t)((uint64_t)ts.tv_sec * 1000u + (uint64_t)ts.tv_nsec / 1000000u);
}

void h_neigh_cfg(udpdk_neigh_cfg_t *cfg)
{
    memset(cfg, 0, sizeof(*cfg));
    cfg->src_ip = g_udpdk.src_ip;
    cfg->netmask = g_udpdk.netmask;
    cfg->gateway = g_udpdk.gateway;
    memcpy(cfg->src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg->fallback_mac, g_udpdk.dst_mac, 6);
    cfg->ttl_ms = g_udpdk.neigh_ttl_ms;
    cfg->retrans_ms = g_udpdk.neigh_retrans_ms;
    cfg->flags = g_udpdk.neigh_mode == UDPDK_NEIGH_MODE_FALLBACK ? UDPDK_NEIGH_FALLBACK : 0u;
}

/* The main context's table, created on first use. 0, or -1 with errno. */
int h_neigh_table(void)
{
    if (!g_udpdk.gpu) { errno = ENODEV; return -1; }
    if (g_udpdk.neigh_ready) return 0;
    const int rc = udpdk_gpu_neigh_create(g_udpdk.gpu, g_udpdk.neigh_entries);
    if (rc) { errno = -rc; return -1; }
    g_udpdk.neigh_ready = 1;
    return 0;
}

int udpdk_neigh_add(uint32_t ip, const uint8_t mac[6])
{
    if (!ip || !mac) { errno = EINVAL; return -1; }
    if (h_neigh_table()) return -1;
    udpdk_neigh_entry_t e;
    memset(&e, 0, sizeof(e));
    e.ip = ip;
    memcpy(e.mac, mac, 6);
    e.state = UDPDK_NEIGH_STATIC;
    const int rc = udpdk_gpu_neigh_set(g_udpdk.gpu, &e, 1);
    if (rc) { errno = -rc; return -1; }
    return 0;
}

int udpdk_neigh_flush(void)
{
    if (!g_udpdk.gpu) { errno = ENODEV; return -1; }
    if (!g_udpdk.neigh_ready) return 0;
    const int rc = udpdk_gpu_neigh_flush(g_udpdk.gpu, 0);
    if (rc) { errno = -rc; return -1; }
    return 0;
}

/* The learn stage for one staged batch (pipe 0: the one-piece poll on the context stream; 1 .. 3: a
 * chunk on its pipe, whose RX has completed), with h_arp_stage's gate: a batch of pure IPv4 enqueues
 * nothing. Synchronous, so the table has no writer when it returns. Returns 0, or -1 with errno. */
int h_neigh_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_ipv4)
{
    if (!g_udpdk.neigh_mode || !b->n || !not_ipv4 || !g_udpdk.src_ip) return 0;
    if (h_neigh_table()) return -1;
    udpdk_neigh_cfg_t cfg;
    h_neigh_cfg(&cfg);
    udpdk_neigh_learn_stats_t st;
    int rc;
    if (pipe) {
        if ((rc = udpdk_gpu_pipe_neigh_learn(g, pipe, &cfg, b, meta_dev, h_neigh_now())) ||
            (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
        rc = udpdk_gpu_pipe_neigh_learn_stats(g, pipe, &st);
    } else {
        if ((rc = udpdk_gpu_neigh_learn(g, &cfg, b, meta_dev, h_neigh_now()))) { errno = -rc; return -1; }
        rc = udpdk_gpu_neigh_learn_stats(g, &st);
    }
    if (rc) { errno = -rc; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    udpdk_neigh_counts_t *c = &g_udpdk.neigh_counts;
    c->arp += st.arp;
    c->malformed += st.malformed;
    c->bad_frame += st.bad_frame;
    c->other_op += st.other_op;
    c->sender_bad += st.sender_bad;
    c->updated += st.updated;
    c->refreshed += st.refreshed;
    c->static_kept += st.static_kept;
    c->created += st.created;
    c->full += st.full;
    c->ignored += st.ignored;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

void h_neigh_count_resolve(const udpdk_neigh_resolve_stats_t *st)   /* under tx_lock */
{
    udpdk_neigh_counts_t *c = &g_udpdk.neigh_counts;
    c->skipped += st->skipped;
    c->bcast += st->bcast;
    c->mcast += st->mcast;
    c->no_route += st->no_route;
    c->self += st->self;
    c->hit += st->hit;
    c->expired += st->expired;
    c->incomplete += st->incomplete;
    c->inserted += st->inserted;
    c->table_full += st->table_full;
    c->fallback += st->fallback;
    c->unresolved += st->unresolved;
    c->no_room += st->no_room;
}
