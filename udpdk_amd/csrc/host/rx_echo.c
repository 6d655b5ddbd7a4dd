/*
 * rx_echo.c — udpdk_poll_echo: one poller turn that answers instead of delivering (the server
 * side of apps/pingpong, recvfrom + sendto back to the source, for a whole batch on the device).
 *
 * The frames and their descriptors go to the GPU in one pinned H2D; udpdk_gpu_rx makes the lanes
 * ([gpu] rx_drop, [gpu] reuseport and the peers of connected sockets apply through the context's
 * sticky stages, as in udpdk_poll_rx);
 * udpdk_gpu_tx_reply turns every lane entry into a reply built straight from the received frame's
 * bytes (headers from the slot table of the uploaded snapshot, the library's MACs, source IP, MTU
 * and tx_udp_cksum); the built bytes and the plan's payload_len / sockfd / frame_off come back and
 * are expanded into udpdk_tx_drain's per-frame table on the host (echo_expand.h). No payload
 * gather, no ring, no host loop over datagrams on the way. Main context only.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "echo_expand.h"
#include "host_state.h"

void h_echo_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.ec_h && g) udpdk_gpu_host_free(g, g_udpdk.ec_h);
    if (g_udpdk.ec_rb_h && g) udpdk_gpu_host_free(g, g_udpdk.ec_rb_h);
    if (g_udpdk.ec_in_d && g) udpdk_gpu_free(g, g_udpdk.ec_in_d);
    if (g_udpdk.ec_ws_d && g) udpdk_gpu_free(g, g_udpdk.ec_ws_d);
    if (g_udpdk.ec_out_d && g) udpdk_gpu_free(g, g_udpdk.ec_out_d);
    g_udpdk.ec_h = g_udpdk.ec_rb_h = g_udpdk.ec_in_d = g_udpdk.ec_ws_d = g_udpdk.ec_out_d = NULL;
    g_udpdk.ec_h_cap = g_udpdk.ec_rb_h_cap = g_udpdk.ec_in_d_cap = g_udpdk.ec_ws_d_cap = g_udpdk.ec_out_d_cap = 0;
}

static inline uint64_t a16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

int udpdk_poll_echo(const uint8_t *frames, uint64_t frames_bytes, const uint32_t *offset,
                    const uint16_t *length, const uint32_t *ptype, uint32_t n,
                    uint8_t *out, uint64_t out_cap, uint32_t *out_off, uint16_t *out_len,
                    uint32_t max, uint32_t *n_out, udpdk_rx_stats_t *stats)
{
    if (!n_out || (max && (!out || !out_off || !out_len))) { errno = EINVAL; return -1; }
    *n_out = 0;
    if (!g_udpdk.gpu) { errno = ENODEV; return -1; }
    if ((n && (!frames || !offset || !length)) || frames_bytes >= (1ull << 32)) { errno = EINVAL; return -1; }
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    /* the bind snapshot and the slot table the replies' source addresses come from: refreshed
     * under the table lock, tx_lock taken before anything is built (udpdk_tx_drain's order) */
    pthread_mutex_lock(&g_udpdk.lock);
    if (h_snapshot_refresh() || h_rx_drop_apply() || h_reuseport_apply() || h_peer_apply()) {
        pthread_mutex_unlock(&g_udpdk.lock);
        return -1;
    }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    int ret = -1, rc;
    udpdk_rx_stats_t st;
    memset(&st, 0, sizeof(st));
    if (!n) { ret = 0; goto done; }
    const uint32_t lanes = g_udpdk.snap_lanes, maxfan = g_udpdk.snap_maxfan;
    const uint32_t mtu = g_udpdk.mtu;
    const uint32_t txf = g_udpdk.tx_udp_cksum ? UDPDK_TX_UDP_CKSUM : 0u;
    const uint64_t cap64 = (uint64_t)n * maxfan;
    const uint32_t cap = cap64 > 0xFFFFFFFEu ? 0xFFFFFFFEu : (uint32_t)cap64;
    /* the most the replies can take: every delivery of every frame answered in full */
    uint64_t need_max = 0;
    for (uint32_t i = 0; i < n; i++)
        need_max += h_echo_span(length[i] > 42u ? length[i] - 42u : 0u, mtu, NULL);
    need_max *= maxfan;
    uint64_t dev_cap = out_cap < need_max ? out_cap : need_max;
    if (dev_cap > 0xFFFFFFF0ull) dev_cap = 0xFFFFFFF0ull;
    /* 1. host staging (pinned) and the device buffers */
    const uint64_t i_fr = 0, i_off = a16(frames_bytes + UDPDK_GPU_FRAMES_TAILROOM), i_len = i_off + a16(4ull * n),
                   i_pt = i_len + a16(2ull * n), i_tot = i_pt + (ptype ? a16(4ull * n) : 0);
    const uint64_t w_meta = 0, w_loff = a16(4ull * n), w_lpkt = w_loff + a16(4ull * (lanes + 1)),
                   w_poff = w_lpkt + a16(4ull * cap), w_dip = w_poff + a16(4ull * cap),
                   w_foff = w_dip + a16(4ull * cap), w_sock = w_foff + a16(4ull * cap + 4),
                   w_plen = w_sock + a16(4ull * cap), w_dport = w_plen + a16(2ull * cap),
                   w_tot = w_dport + a16(2ull * cap);
    if (h_grow_pinned(&g_udpdk.ec_h, &g_udpdk.ec_h_cap, i_tot) ||
        h_grow_dev(&g_udpdk.ec_in_d, &g_udpdk.ec_in_d_cap, i_tot + 64) ||
        h_grow_dev(&g_udpdk.ec_ws_d, &g_udpdk.ec_ws_d_cap, w_tot + 64) ||
        h_grow_dev(&g_udpdk.ec_out_d, &g_udpdk.ec_out_d_cap, dev_cap + 64))
        goto done;
    uint8_t *h = g_udpdk.ec_h, *di = g_udpdk.ec_in_d, *dw = g_udpdk.ec_ws_d;
    memcpy(h + i_fr, frames, frames_bytes);
    memset(h + i_fr + frames_bytes, 0, i_off - frames_bytes);
    memcpy(h + i_off, offset, 4ull * n);
    memcpy(h + i_len, length, 2ull * n);
    if (ptype) memcpy(h + i_pt, ptype, 4ull * n);
    /* 2. GPU: one H2D, RX, the replies */
    const udpdk_rx_batch_t b = {di + i_fr, frames_bytes, (const uint32_t *)(di + i_off),
                                (const uint16_t *)(di + i_len), ptype ? (const uint32_t *)(di + i_pt) : NULL, n};
    const udpdk_rx_out_t ro = {(uint32_t *)(dw + w_meta), (uint32_t *)(dw + w_loff), (uint32_t *)(dw + w_lpkt), cap};
    const udpdk_rx_lanes_t ln = {ro.meta_dev, n, ro.lane_off_dev, ro.lane_pkt_dev, cap, lanes};
    const udpdk_tx_reply_plan_t pl = {(uint32_t *)(dw + w_poff), (uint16_t *)(dw + w_plen), (int32_t *)(dw + w_sock),
                                      (uint32_t *)(dw + w_dip), (uint16_t *)(dw + w_dport), (uint32_t *)(dw + w_foff)};
    udpdk_tx_config_t cfg;
    memcpy(cfg.src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg.dst_mac, g_udpdk.dst_mac, 6);
    cfg.src_ip = g_udpdk.src_ip;
    udpdk_tx_reply_stats_t rs;
    if ((rc = udpdk_gpu_h2d(g, di, h, i_tot)) || (rc = udpdk_gpu_rx(g, &b, &ro)) ||
        (rc = udpdk_gpu_tx_reply(g, &cfg, &b, &ln, 0, cap, NULL, mtu, txf, g_udpdk.ec_out_d, dev_cap, &pl))) {
        errno = -rc;
        goto done;
    }
    rc = udpdk_gpu_tx_reply_stats(g, &rs);
    if (rc && rc != -ENOSPC) { errno = -rc; goto done; }
    if ((rc = udpdk_gpu_rx_stats(g, &st))) { errno = -rc; goto done; }
    h_rx_drop_count(g, &st);
    /* nothing has been published anywhere: the caller may come back with more room */
    if (rs.no_room || rs.frames > max || rs.bytes_needed > out_cap) { errno = ENOBUFS; goto done; }
    /* 3. the built bytes and the plan's per-datagram arrays back, then the frame table */
    const uint32_t D = st.deliveries < cap ? st.deliveries : cap;
    const uint64_t r_foff = 0, r_sock = a16(4ull * D + 4), r_plen = r_sock + a16(4ull * D), r_tot = r_plen + a16(2ull * D);
    if (h_grow_pinned(&g_udpdk.ec_rb_h, &g_udpdk.ec_rb_h_cap, r_tot)) goto done;
    uint8_t *r = g_udpdk.ec_rb_h;
    if ((rs.bytes_needed && (rc = udpdk_gpu_d2h(g, out, g_udpdk.ec_out_d, rs.bytes_needed))) ||
        (rc = udpdk_gpu_d2h(g, r + r_foff, dw + w_foff, 4ull * D + 4)) ||
        (D && (rc = udpdk_gpu_d2h(g, r + r_sock, dw + w_sock, 4ull * D))) ||
        (D && (rc = udpdk_gpu_d2h(g, r + r_plen, dw + w_plen, 2ull * D))) || (rc = udpdk_gpu_sync(g))) {
        errno = -rc;
        goto done;
    }
    uint32_t nf = 0;
    rc = h_echo_expand((const uint16_t *)(r + r_plen), (const int32_t *)(r + r_sock), (const uint32_t *)(r + r_foff),
                       D, mtu, rs.bytes_needed, max, out_off, out_len, &nf);
    if (rc || nf != rs.frames) { errno = rc ? -rc : EIO; goto done; }
    *n_out = nf;
    ret = 0;
done:
    if (ret == 0 && stats) *stats = st;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    pthread_mutex_unlock(&g_udpdk.lock);
    return ret;
}
