/*
 * rx_icmp_err.c — the socket layer's received ICMP errors: udpdk_config_icmp_errors /
 * udpdk_sock_error_post / udpdk_icmp_err_counts, and the stage udpdk_poll_rx runs after a batch's RX
 * when the switch is on and a socket is connected (udpdk_gpu_icmp_errors on the staged device batch
 * against the peer table h_peer_apply uploaded; the words of the lanes that carry an error are
 * copied back and posted as the sockets' pending errors, which the socket calls of sock_api.c report
 * the way Linux reports sk_err). The reference has no ICMP and no connect; off by default.
 */
#include <errno.h>
#include <string.h>

#include "host_state.h"

int udpdk_config_icmp_errors(int on)
{
    const int was = (int)g_udpdk.icmp_errors;
    if (on < 0) return was;
    if (on > 1) { errno = EINVAL; return -1; }
    if (on && g_udpdk.n_shards > 1) { errno = ENOTSUP; return -1; }      /* sharded polls: not reported */
    g_udpdk.icmp_errors = (uint32_t)on;
    return was;
}

int udpdk_icmp_err_counts(udpdk_icmp_err_counts_t *c)
{
    if (!c) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.lock);
    *c = g_udpdk.icmp_err_counts;
    pthread_mutex_unlock(&g_udpdk.lock);
    return 0;
}

void h_icmp_err_reset(void)               /* under g_udpdk.lock */
{
    memset(&g_udpdk.icmp_err_counts, 0, sizeof(g_udpdk.icmp_err_counts));
}

void h_icmp_err_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.ie_d && g) udpdk_gpu_free(g, g_udpdk.ie_d);
    if (g_udpdk.ie_h && g) udpdk_gpu_host_free(g, g_udpdk.ie_h);
    g_udpdk.ie_d = g_udpdk.ie_h = NULL;
    g_udpdk.ie_d_cap = g_udpdk.ie_h_cap = 0;
}

/* One word per lane on the device and, once something was reported, pinned: sized once for the
 * contexts' lane limit, 8 * max_lanes bytes each, so they never grow past that. */
static int h_ie_buffer(void **p, uint64_t *cap, uint64_t need, int pinned)
{
    if (*p && *cap >= need) return 0;
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (*p) (void)(pinned ? udpdk_gpu_host_free(g, *p) : udpdk_gpu_free(g, *p));
    *p = NULL;
    *cap = 0;
    const uint64_t nc = 8ull * g_udpdk.gpu_max_lanes > need ? 8ull * g_udpdk.gpu_max_lanes : need;
    const int rc = pinned ? udpdk_gpu_host_alloc(g, nc, p) : udpdk_gpu_alloc(g, nc, p);
    if (rc) { errno = -rc; return -1; }
    *cap = nc;
    return 0;
}

/* g_udpdk.lock held. */
int h_sock_error_post_locked(int s, uint32_t peer_ip, uint16_t peer_port, uint32_t code)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) return 0;
    struct h_slot *sl = &g_udpdk.slots[s];
    int hard = 0;
    const int e = udpdk_gpu_icmp_errno(code, &hard);
    if (!sl->used || !sl->connected || sl->peer_ip != peer_ip || sl->peer_port != peer_port || !hard || !e)
        return 0;
    atomic_store(&sl->so_error, e);            /* a later error overwrites (Linux: sk_err) */
    g_udpdk.icmp_err_counts.posted++;
    return 1;
}

int udpdk_sock_error_post(int s, uint32_t peer_ip, uint16_t peer_port, uint32_t code)
{
    pthread_mutex_lock(&g_udpdk.lock);
    const int r = h_sock_error_post_locked(s, peer_ip, peer_port, code);
    pthread_mutex_unlock(&g_udpdk.lock);
    return r;
}

/* The socket's pending error, cleared: what the next socket call reports. One relaxed load on the
 * calls' fast path (no error). */
int h_sock_error_take(int s)
{
    atomic_int *p = &g_udpdk.slots[s].so_error;
    if (!atomic_load_explicit(p, memory_order_relaxed)) return 0;
    return atomic_exchange(p, 0);
}

/* The stage for one staged batch (pipe 0: the one-piece poll on the context stream; 1 .. 3: a chunk
 * on its pipe, whose RX has completed), g_udpdk.lock held by the poll. Synchronous: the errors are
 * posted when it returns. The words are copied back only when the device reported something.
 * Returns 0, or -1 with errno. */
int h_icmp_err_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev)
{
    if (!g_udpdk.icmp_errors || !g_udpdk.peer_applied || !b->n) return 0;
    const uint32_t lanes = g_udpdk.snap_lanes < UDPDK_MAX_SOCKETS ? g_udpdk.snap_lanes : UDPDK_MAX_SOCKETS;
    if (!lanes) return 0;
    int rc;
    if (h_ie_buffer(&g_udpdk.ie_d, &g_udpdk.ie_d_cap, 8ull * lanes, 0)) return -1;
    uint64_t *err_d = g_udpdk.ie_d;
    udpdk_icmp_err_stats_t st;
    if (pipe) {
        if ((rc = udpdk_gpu_pipe_icmp_errors(g, pipe, g_udpdk.src_ip, b, meta_dev, NULL, lanes, err_d)) ||
            (rc = udpdk_gpu_pipe_wait(g, pipe)) || (rc = udpdk_gpu_pipe_icmp_err_stats(g, pipe, &st))) {
            errno = -rc;
            return -1;
        }
    } else {
        if ((rc = udpdk_gpu_icmp_errors(g, g_udpdk.src_ip, b, meta_dev, NULL, lanes, err_d)) ||
            (rc = udpdk_gpu_icmp_err_stats(g, &st))) {
            errno = -rc;
            return -1;
        }
    }
    udpdk_icmp_err_counts_t *c = &g_udpdk.icmp_err_counts;
    c->errors += st.errors;
    c->msg_bad += st.msg_bad;
    c->quote_bad += st.quote_bad;
    c->soft += st.soft;
    c->no_socket += st.no_socket;
    c->reported += st.reported;
    if (!st.reported) return 0;
    if (h_ie_buffer(&g_udpdk.ie_h, &g_udpdk.ie_h_cap, 8ull * lanes, 1)) return -1;
    const uint64_t *w = g_udpdk.ie_h;
    if (pipe) {
        if ((rc = udpdk_gpu_pipe_d2h(g, pipe, g_udpdk.ie_h, err_d, 8ull * lanes)) ||
            (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
    } else {
        if ((rc = udpdk_gpu_d2h(g, g_udpdk.ie_h, err_d, 8ull * lanes)) ||
            (rc = udpdk_gpu_sync(g))) { errno = -rc; return -1; }
    }
    /* against the records the device matched: a socket that changed its peer since is left alone */
    for (uint32_t s = 0; s < lanes; s++)
        if (w[s])
            (void)h_sock_error_post_locked((int)s, g_udpdk.peer_up[s].ip, g_udpdk.peer_up[s].port,
                                           (uint32_t)(w[s] & 0xFFu));
    return 0;
}
