/*
 * tx_drain.c — udpdk_tx_drain: the poller's TX half (udpdk_poller.c:453-514) on the GPU.
 *
 * Selection follows the poller loop: sockets in index order, each socket's TX ring dequeued
 * while the burst holds fewer than BURST_SIZE frames (a datagram longer than the MTU counts as
 * its fragments, :461-501), the burst flushed when it reaches BURST_SIZE, and the loop repeated
 * until the rings are empty or the caller's frame / byte limits stop it. The selected
 * datagrams' payloads go to the GPU in one pinned H2D, udpdk_gpu_tx_build_flags builds every frame
 * (Ethernet/IPv4/UDP headers from the slot table of the uploaded bind snapshot, rte_ipv4_cksum,
 * payload copy, fragmentation at the MTU, the UDP checksum with [gpu] tx_udp_cksum = 1) and one
 * D2H returns them.
 *
 * ARP and ICMP frames a poll built (rx_arp.c, rx_icmp.c) and the ARP announcement leave first, oldest
 * first, copied from their host queue; the socket datagrams follow in what room is left. A queued frame that does not fit the caller's
 * limits stays queued, and the datagrams wait behind it for the next drain.
 *
 * With [gpu] neigh on, the build is preceded by udpdk_gpu_neigh_resolve on the same stream and done by
 * udpdk_gpu_tx_build_neigh: every datagram's frames carry its next hop's MAC. The resolved sockets and
 * the first who-has requests come back behind the frames and the counts in the same wait. A datagram
 * that came out without a socket (no MAC in strict mode, no route) is left out of the frame table,
 * dequeued and counted like the others the drain cannot send; its span in the output is a gap. The
 * requests go onto the host queue and leave first in the next drain. Off, the drain calls what it
 * always called.
 *
 * A send queued with a segment size (UDP_SEGMENT, sock_api.c) is selected as a unit: its frames and
 * bytes come from udpdk_gpu_tx_segment_span, the burst counter advances by its frames, and the drop
 * rule applies to the whole send. A drain that selected one stages the sends with their sizes instead
 * of per-datagram frame offsets, and udpdk_gpu_tx_segment_plan expands them on the device into one
 * descriptor per segment (max_segs = the host's own count) in front of the resolve and the build; the
 * frame table comes from the closed form. A drain that selected none stages and launches what it
 * always did.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "host_state.h"

void h_tx_buffers_free(void)
{
    if (g_udpdk.tx_h && g_udpdk.gpu) udpdk_gpu_host_free(g_udpdk.gpu, g_udpdk.tx_h);
    if (g_udpdk.tx_d && g_udpdk.gpu) udpdk_gpu_free(g_udpdk.gpu, g_udpdk.tx_d);
    if (g_udpdk.tx_fr_d && g_udpdk.gpu) udpdk_gpu_free(g_udpdk.gpu, g_udpdk.tx_fr_d);
    g_udpdk.tx_h = g_udpdk.tx_d = g_udpdk.tx_fr_d = NULL;
    g_udpdk.tx_h_cap = g_udpdk.tx_d_cap = g_udpdk.tx_fr_d_cap = 0;
    free(g_udpdk.tx_sel);
    g_udpdk.tx_sel = NULL;
    g_udpdk.tx_sel_cap = 0;
}

int h_grow_pinned(void **p, uint64_t *cap, uint64_t need)
{
    if (*p && *cap >= need) return 0;
    if (*p) udpdk_gpu_host_free(g_udpdk.gpu, *p);
    *p = NULL;
    *cap = 0;
    const uint64_t nc = need < (1u << 16) ? (1u << 16) : need + need / 4;
    const int rc = udpdk_gpu_host_alloc(g_udpdk.gpu, nc, p);
    if (rc) { errno = -rc; return -1; }
    *cap = nc;
    return 0;
}

static inline uint64_t a16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

int udpdk_tx_drain(uint8_t *out, uint64_t out_cap, uint32_t *out_off, uint16_t *out_len,
                   uint32_t max, uint32_t *n_out)
{
    if (!n_out || (max && (!out || !out_off || !out_len))) { errno = EINVAL; return -1; }
    *n_out = 0;
    if (!g_udpdk.gpu) { errno = ENODEV; return -1; }
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    const uint32_t mtu = g_udpdk.mtu;
    const uint32_t txf = g_udpdk.tx_udp_cksum ? UDPDK_TX_UDP_CKSUM : 0u;
    const int neigh = g_udpdk.neigh_mode != UDPDK_NEIGH_MODE_OFF;
    /* the slot table the TX kernel reads (source port and address per socket). tx_lock is taken
     * before the table lock is dropped (the order udpdk_close uses): a sendto that auto-binds, or
     * a close + socket + bind, either lands before the refresh (and is in the uploaded table) or
     * queues its datagram only after this drain has released tx_lock, so no datagram selected
     * below is built from a slot row older than its socket's binding. */
    pthread_mutex_lock(&g_udpdk.lock);
    const int src = h_snapshot_refresh();
    if (src) {
        pthread_mutex_unlock(&g_udpdk.lock);
        return -1;
    }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    pthread_mutex_unlock(&g_udpdk.lock);
    int ret = -1, rc;
    /* 0. the queued ARP and ICMP frames */
    uint32_t k0 = 0;
    uint64_t b0 = 0;
    h_icmpq_drain(&g_udpdk.icmpq, out, out_cap, out_off, out_len, max, &k0, &b0);
    *n_out = k0;
    if (g_udpdk.icmpq.count) { ret = 0; goto out; }
    const uint32_t max_s = max - k0;
    const uint64_t cap_s = out_cap - b0;
    /* 1. selection in the poller's order */
    uint32_t nsel = 0, nframes = 0, burst = 0, ndg = 0, n_gso = 0;   /* ndg: datagrams (a send's segments) */
    uint64_t bytes = 0, pay = 0;
    int progress = 1, full = 0;
    uint32_t taken[UDPDK_MAX_SOCKETS];
    memset(taken, 0, sizeof(taken));
    while (progress && !full) {
        progress = 0;
        for (int s = 0; s < UDPDK_MAX_SOCKETS && !full; s++) {
            struct h_txq *q = &g_udpdk.slots[s].tx;
            if (!g_udpdk.slots[s].used || !q->e) continue;
            while (burst < H_BURST_SIZE && q->head + taken[s] != q->tail) {
                const struct h_txd *t = &q->e[(q->head + taken[s]) % UDPDK_RX_RING_SIZE];
                uint32_t nf = 1, nseg = 1;
                const uint64_t span = udpdk_gpu_tx_segment_span(t->len, t->gso, mtu, &nseg, &nf);
                if (nframes + nf > max_s || bytes + span > cap_s) {
                    if (nframes == 0 && taken[s] == 0 && (nf > max || span > out_cap)) {
                        /* larger than any drain with these limits can carry: it would block
                         * the ring's head forever. Dropped and counted (udpdk_tx_dropped), as
                         * the reference's poller drops a burst it cannot send. */
                        q->head++;
                        g_udpdk.tx_queued--;
                        g_udpdk.tx_dropped++;
                        continue;
                    }
                    full = 1;
                    break;
                }
                if (nsel + 1 > g_udpdk.tx_sel_cap) {
                    const uint64_t nc = g_udpdk.tx_sel_cap ? 2 * g_udpdk.tx_sel_cap : 4096;
                    void *ns = realloc(g_udpdk.tx_sel, nc * sizeof(*g_udpdk.tx_sel));
                    if (!ns) { errno = ENOMEM; goto out; }
                    g_udpdk.tx_sel = ns;
                    g_udpdk.tx_sel_cap = nc;
                }
                g_udpdk.tx_sel[nsel].s = s;
                g_udpdk.tx_sel[nsel].nf = nf;
                g_udpdk.tx_sel[nsel].foff = bytes;
                nsel++;
                ndg += nseg;
                n_gso += t->gso != 0;
                taken[s]++;
                nframes += nf;
                bytes += span;
                pay += t->len;
                burst += nf;
                progress = 1;
            }
            if (burst >= H_BURST_SIZE) burst = 0;           /* flush_tx_table */
        }
        burst = 0;                                           /* end of the loop's TX half */
    }
    if (!nsel) {
        if (!g_udpdk.tx_queued) g_udpdk.txp_bytes = 0;   /* only dropped ones were left */
        ret = 0;
        goto out;
    }
    /* 2. host staging (pinned): payloads packed, then the per-datagram arrays */
    /* (with a segmented send: its size in place of the frame offset, which the plan computes, and
     * behind the staged bytes, device only, the plan's arrays: one descriptor per segment, frame_off,
     * seg_off) */
    const uint64_t o_pay = 0, o_poff = a16(pay), o_len = o_poff + a16(4ull * nsel),
                   o_sock = o_len + a16(2ull * nsel), o_ip = o_sock + a16(4ull * nsel),
                   o_port = o_ip + a16(4ull * nsel), o_foff = o_port + a16(2ull * nsel),
                   tot = o_foff + a16(n_gso ? 2ull * nsel : 4ull * nsel);
    const uint64_t p_poff = tot, p_len = p_poff + a16(4ull * ndg), p_sock = p_len + a16(2ull * ndg),
                   p_ip = p_sock + a16(4ull * ndg), p_port = p_ip + a16(4ull * ndg), p_foff = p_port + a16(2ull * ndg),
                   p_soff = p_foff + a16(4ull * ndg + 4), p_tot = p_soff + a16(4ull * nsel + 4);
    if (h_grow_pinned(&g_udpdk.tx_h, &g_udpdk.tx_h_cap, tot) ||
        h_grow_dev(&g_udpdk.tx_d, &g_udpdk.tx_d_cap, (n_gso ? p_tot : tot) + 64) ||
        h_grow_dev(&g_udpdk.tx_fr_d, &g_udpdk.tx_fr_d_cap, bytes + 64))
        goto out;
    uint8_t *h = g_udpdk.tx_h;
    uint32_t *poff = (uint32_t *)(h + o_poff), *sock = (uint32_t *)(h + o_sock);
    uint32_t *ip = (uint32_t *)(h + o_ip), *foff = (uint32_t *)(h + o_foff);
    uint16_t *len = (uint16_t *)(h + o_len), *port = (uint16_t *)(h + o_port), *gsz = (uint16_t *)(h + o_foff);
    memset(taken, 0, sizeof(taken));
    uint64_t pp = 0;
    for (uint32_t i = 0; i < nsel; i++) {
        const int s = g_udpdk.tx_sel[i].s;
        const struct h_txq *q = &g_udpdk.slots[s].tx;
        const struct h_txd *t = &q->e[(q->head + taken[s]++) % UDPDK_RX_RING_SIZE];
        memcpy(h + o_pay + pp, g_udpdk.txp + t->pay, t->len);
        poff[i] = (uint32_t)pp;
        len[i] = (uint16_t)t->len;
        sock[i] = (uint32_t)s;
        ip[i] = t->dst_ip;
        port[i] = (uint16_t)t->dst_port;
        if (n_gso) gsz[i] = (uint16_t)t->gso;
        else foff[i] = (uint32_t)g_udpdk.tx_sel[i].foff;
        pp += t->len;
    }
    /* 3. GPU: one H2D, the build, one D2H */
    uint8_t *d = g_udpdk.tx_d;
    udpdk_tx_config_t cfg;
    memcpy(cfg.src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg.dst_mac, g_udpdk.dst_mac, 6);
    cfg.src_ip = g_udpdk.src_ip;
    udpdk_tx_batch_t b = {d + o_pay, pay, (const uint32_t *)(d + o_poff), (const uint16_t *)(d + o_len),
                          (const int32_t *)(d + o_sock), (const uint32_t *)(d + o_ip),
                          (const uint16_t *)(d + o_port), nsel};
    udpdk_tx_out_t o = {g_udpdk.tx_fr_d, bytes + 64, (const uint32_t *)(d + o_foff)};
    const int32_t *sock_out = NULL;
    /* what the resolve and the build see: the staged datagrams, or the plan's segments */
    const uint32_t *ip_d = (const uint32_t *)(d + o_ip);
    const int32_t *sock_d = (const int32_t *)(d + o_sock);
    if (n_gso) {
        const udpdk_tx_sends_t sd = {d + o_pay, pay, (const uint32_t *)(d + o_poff), (const uint16_t *)(d + o_len),
                                     (const uint16_t *)(d + o_foff), (const int32_t *)(d + o_sock),
                                     (const uint32_t *)(d + o_ip), (const uint16_t *)(d + o_port), nsel};
        const udpdk_tx_segment_plan_t pl = {(uint32_t *)(d + p_poff), (uint16_t *)(d + p_len), (int32_t *)(d + p_sock),
                                            (uint32_t *)(d + p_ip), (uint16_t *)(d + p_port), (uint32_t *)(d + p_foff),
                                            (uint32_t *)(d + p_soff), ndg};
        if ((rc = udpdk_gpu_h2d(g, d, h, tot)) || (rc = udpdk_gpu_tx_segment_plan(g, &sd, mtu, 0u, bytes, &pl))) {
            errno = -rc;
            goto out;
        }
        g_udpdk.gso_counts.plans++;
        const udpdk_tx_batch_t bp = {d + o_pay, pay, pl.payload_off_dev, pl.payload_len_dev, pl.sockfd_dev,
                                     pl.dst_ip_dev, pl.dst_port_dev, ndg};
        b = bp;
        o.frame_off_dev = pl.frame_off_dev;
        ip_d = pl.dst_ip_dev;
        sock_d = pl.sockfd_dev;
    }
    if (neigh) {
        /* device: MACs, resolved sockets, states, request slots, origins; pinned: sockets, slots */
        const uint64_t n_mac = 0, n_sock = a16(8ull * ndg), n_state = n_sock + a16(4ull * ndg),
                       n_req = n_state + a16(ndg), n_org = n_req + (uint64_t)H_NEIGH_REQ_CAP * UDPDK_ARP_SLOT_BYTES,
                       n_tot = n_org + 4ull * H_NEIGH_REQ_CAP;
        const uint64_t hq = a16(4ull * ndg), first = (uint64_t)H_NEIGH_REQ_FIRST * UDPDK_ARP_SLOT_BYTES;
        if (h_neigh_table() || h_grow_dev(&g_udpdk.ng_d, &g_udpdk.ng_d_cap, n_tot) ||
            h_grow_pinned(&g_udpdk.ng_h, &g_udpdk.ng_h_cap, hq + (uint64_t)H_NEIGH_REQ_CAP * UDPDK_ARP_SLOT_BYTES))
            goto out;
        uint8_t *nd = g_udpdk.ng_d, *nh = g_udpdk.ng_h;
        udpdk_neigh_cfg_t ncfg;
        h_neigh_cfg(&ncfg);
        const udpdk_neigh_out_t no = {(uint32_t *)(nd + n_mac), (int32_t *)(nd + n_sock), nd + n_state, nd + n_req,
                                      (uint32_t *)(nd + n_org), H_NEIGH_REQ_CAP};
        udpdk_neigh_resolve_stats_t nst;
        b.sockfd_dev = no.sockfd_out_dev;
        if ((!n_gso && (rc = udpdk_gpu_h2d(g, d, h, tot))) ||
            (rc = udpdk_gpu_neigh_resolve(g, &ncfg, ip_d, sock_d, ndg, h_neigh_now(), &no)) ||
            (rc = udpdk_gpu_tx_build_neigh(g, &cfg, &b, &o, mtu, txf, no.dmac_dev)) ||
            (rc = udpdk_gpu_d2h(g, out + b0, g_udpdk.tx_fr_d, bytes)) ||
            (rc = udpdk_gpu_d2h(g, nh, no.sockfd_out_dev, 4ull * ndg)) ||
            (rc = udpdk_gpu_d2h(g, nh + hq, no.req_dev, first))) {
            errno = -rc;
            goto out;
        }
        rc = udpdk_gpu_neigh_resolve_stats(g, &nst);               /* (waits for all of the above) */
        if (rc && rc != -ENOSPC) { errno = -rc; goto out; }       /* (-ENOSPC: the excess is no_room) */
        if (nst.requests > H_NEIGH_REQ_CAP) { errno = EIO; goto out; }
        if (nst.requests > H_NEIGH_REQ_FIRST &&
            ((rc = udpdk_gpu_d2h(g, nh + hq + first, no.req_dev + first,
                                 (uint64_t)(nst.requests - H_NEIGH_REQ_FIRST) * UDPDK_ARP_SLOT_BYTES)) ||
             (rc = udpdk_gpu_sync(g)))) {
            errno = -rc;
            goto out;
        }
        if (nst.requests && !g_udpdk.icmpq.buf && h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES)) { errno = ENOMEM; goto out; }
        for (uint32_t r = 0; r < nst.requests; r++)
            if (!h_icmpq_push(&g_udpdk.icmpq, nh + hq + (uint64_t)r * UDPDK_ARP_SLOT_BYTES, UDPDK_ARP_FRAME_BYTES))
                g_udpdk.neigh_counts.requests++;
        h_neigh_count_resolve(&nst);
        sock_out = (const int32_t *)nh;
    } else if ((!n_gso && (rc = udpdk_gpu_h2d(g, d, h, tot))) || (rc = udpdk_gpu_tx_build_flags(g, &cfg, &b, &o, mtu, txf)) ||
        (rc = udpdk_gpu_d2h(g, out + b0, g_udpdk.tx_fr_d, bytes)) || (rc = udpdk_gpu_sync(g))) {
        errno = -rc;
        goto out;
    }
    /* 4. frame table, dequeue, payload store compaction */
    uint32_t k = k0, m = 0;
    for (uint32_t i = 0; i < nsel; i++) {
        /* the send's segments by the closed form (one for an ordinary datagram), back to back */
        const uint32_t gs = n_gso ? gsz[i] : 0u;
        uint32_t nseg = 1;
        udpdk_gpu_tx_segment_span(len[i], gs, mtu, &nseg, NULL);
        uint64_t so = g_udpdk.tx_sel[i].foff;
        for (uint32_t t = 0; t < nseg; t++, m++) {
            const uint32_t sl = nseg > 1 && t + 1 < nseg ? gs : len[i] - t * gs;
            uint32_t nf = 1;
            const uint64_t span = udpdk_gpu_tx_span(sl, mtu, &nf);
            const uint64_t fo = so;
            so += span;
            if (sock_out && sock_out[m] < 0) {              /* unresolved: nothing was built for it */
                g_udpdk.neigh_counts.tx_unresolved++;
                continue;
            }
            for (uint32_t f = 0; f < nf; f++) {
                out_off[k] = (uint32_t)(b0 + fo) + f * (mtu + 14u);
                out_len[k] = (uint16_t)(f + 1 < nf ? mtu + 14u : span - (uint64_t)(nf - 1) * (mtu + 14u));
                k++;
            }
        }
    }
    for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) g_udpdk.slots[s].tx.head += taken[s];
    g_udpdk.tx_queued -= nsel;
    if (!g_udpdk.tx_queued) {
        g_udpdk.txp_bytes = 0;
    } else if (g_udpdk.txp_bytes > (1u << 24)) {
        /* compact: the remaining datagrams' payloads to the front, in store order */
        uint64_t w = 0, lo = UINT64_MAX;
        for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
            const struct h_txq *q = &g_udpdk.slots[s].tx;
            for (uint32_t j = q->head; q->e && j != q->tail; j++)
                if (q->e[j % UDPDK_RX_RING_SIZE].pay < lo) lo = q->e[j % UDPDK_RX_RING_SIZE].pay;
        }
        if (lo != UINT64_MAX && lo > 0) {
            w = g_udpdk.txp_bytes - lo;
            memmove(g_udpdk.txp, g_udpdk.txp + lo, w);
            for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
                struct h_txq *q = &g_udpdk.slots[s].tx;
                for (uint32_t j = q->head; q->e && j != q->tail; j++) q->e[j % UDPDK_RX_RING_SIZE].pay -= lo;
            }
            g_udpdk.txp_bytes = w;
        }
    }
    *n_out = k;
    ret = 0;
out:
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return ret;
}
