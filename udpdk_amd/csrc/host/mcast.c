/*
 * mcast.c — the socket layer's multicast: IP_ADD_MEMBERSHIP / IP_DROP_MEMBERSHIP (per socket, Linux
 * with IP_MULTICAST_ALL = 0), udpdk_config_mcast / udpdk_mcast_counts / udpdk_rx_not_member, what a
 * poll uploads for the device membership filter (h_mcast_apply: udpdk_gpu_rx_mcast) and the stage
 * udpdk_poll_rx runs after a batch's RX when the switch is on, a group is joined and the batch held
 * a frame that is IPv4 but not UDP (udpdk_gpu_igmp_reply on the staged device batch, the reports
 * copied back and appended to the host queue that udpdk_tx_drain empties first). The unsolicited
 * report of a group's first join and the leave of its last drop are built on the host
 * (igmp_frame.h). The reference has no multicast; off by default.
 */
#include <errno.h>
#include <netinet/in.h>
#include <stdlib.h>
#include <string.h>

#include "igmp_frame.h"
#include "host_state.h"

#define H_IGMP_OUT_BYTES ((uint64_t)UDPDK_IGMP_MAX_GROUPS * UDPDK_IGMP_SLOT_BYTES)

static int h_is_group(uint32_t raw) { return (raw & 0xF0u) == 0xE0u; }

/* how many sockets hold the group (g_udpdk.lock held) */
static uint32_t h_mcast_holders(uint32_t group)
{
    uint32_t n = 0;
    for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
        const struct h_slot *sl = &g_udpdk.slots[s];
        for (uint32_t k = 0; sl->used && k < sl->n_mc; k++) n += sl->mc_group[k] == group;
    }
    return n;
}

/* One report or leave onto the queue udpdk_tx_drain empties first. Nothing is sent with the switch
 * off, for 224.0.0.1 (RFC 2236 section 6: never reported) or without a source address. */
static void h_mcast_send(uint32_t type, uint32_t group)
{
    if (!g_udpdk.mcast_on || group == H_IGMP_ALL_HOSTS || !g_udpdk.src_ip) return;
    uint8_t f[H_IGMP_FRAME_BYTES];
    h_igmp_build(f, g_udpdk.src_mac, g_udpdk.src_ip, type, group);
    pthread_mutex_lock(&g_udpdk.tx_lock);
    if ((g_udpdk.icmpq.buf || !h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES)) &&
        !h_icmpq_push(&g_udpdk.icmpq, f, H_IGMP_FRAME_BYTES)) {
        if (type == H_IGMP_LEAVE) g_udpdk.mcast_counts.leaves_sent++;
        else g_udpdk.mcast_counts.reports_sent++;
    }
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

static void h_mcast_count(int leave)
{
    pthread_mutex_lock(&g_udpdk.tx_lock);
    if (leave) g_udpdk.mcast_counts.leaves++;
    else g_udpdk.mcast_counts.joins++;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

/* socket s leaves entry k of its list (g_udpdk.lock held): the last holder's drop sends the leave */
static void h_mcast_drop_at(struct h_slot *sl, uint32_t k)
{
    const uint32_t group = sl->mc_group[k];
    sl->mc_group[k] = sl->mc_group[--sl->n_mc];
    g_udpdk.mcast_version++;
    h_mcast_count(1);
    if (!h_mcast_holders(group)) h_mcast_send(H_IGMP_LEAVE, group);
}

void h_mcast_close_locked(int s)
{
    struct h_slot *sl = &g_udpdk.slots[s];
    while (sl->n_mc) h_mcast_drop_at(sl, sl->n_mc - 1u);
}

/* udpdk_setsockopt(s, IPPROTO_IP, ...): struct ip_mreq or struct ip_mreqn (the same two addresses
 * first; an interface index must be 0) */
int h_mcast_sockopt(int s, int optname, const void *optval, socklen_t optlen)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = EBADF; return -1; }
    if (optname != IP_ADD_MEMBERSHIP && optname != IP_DROP_MEMBERSHIP) { errno = ENOPROTOOPT; return -1; }
    if (!optval) { errno = EFAULT; return -1; }
    if (optlen < sizeof(struct ip_mreq)) { errno = EINVAL; return -1; }
    struct ip_mreqn mr;
    memset(&mr, 0, sizeof(mr));
    memcpy(&mr, optval, optlen < sizeof(mr) ? sizeof(struct ip_mreq) : sizeof(mr));
    const uint32_t group = mr.imr_multiaddr.s_addr, ifa = mr.imr_address.s_addr;
    pthread_mutex_lock(&g_udpdk.lock);
    struct h_slot *sl = &g_udpdk.slots[s];
    int err = 0;
    uint32_t at = 0;
    if (!sl->used) err = EBADF;
    else if (!h_is_group(group)) err = EINVAL;
    else if ((ifa != 0u && ifa != g_udpdk.src_ip) || mr.imr_ifindex != 0) err = ENODEV;
    if (!err) {
        while (at < sl->n_mc && sl->mc_group[at] != group) at++;
        if (optname == IP_ADD_MEMBERSHIP) {
            if (at < sl->n_mc) err = EADDRINUSE;
            else if (sl->n_mc == H_MCAST_MAX) err = ENOBUFS;
        } else if (at == sl->n_mc) {
            err = EADDRNOTAVAIL;
        }
    }
    if (!err && optname == IP_ADD_MEMBERSHIP) {
        const int first = !h_mcast_holders(group);
        sl->mc_group[sl->n_mc++] = group;
        g_udpdk.mcast_version++;
        h_mcast_count(0);
        if (first) h_mcast_send(H_IGMP_REPORT, group);
    } else if (!err) {
        h_mcast_drop_at(sl, at);
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    if (err) { errno = err; return -1; }
    return 0;
}

/* The distinct groups held, in socket order, 224.0.0.1 left out: out[cap]. Returns how many there are
 * (possibly more than cap: only the first cap are written). g_udpdk.lock held. */
static uint32_t h_mcast_groups(uint32_t *out, uint32_t cap)
{
    uint32_t n = 0;
    for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
        const struct h_slot *sl = &g_udpdk.slots[s];
        for (uint32_t k = 0; sl->used && k < sl->n_mc; k++) {
            const uint32_t g = sl->mc_group[k];
            uint32_t j = 0;
            const uint32_t seen = n < cap ? n : cap;
            while (j < seen && out[j] != g) j++;
            if (j < seen || g == H_IGMP_ALL_HOSTS) continue;
            if (n < cap) out[n] = g;
            n++;
        }
    }
    return n;
}

int udpdk_config_mcast(int on)
{
    pthread_mutex_lock(&g_udpdk.lock);
    const int was = (int)g_udpdk.mcast_on;
    int err = 0;
    if (on > 1) err = EINVAL;
    else if (on > 0 && g_udpdk.n_shards > 1) err = ENOTSUP;            /* sharded polls: no filter, no IGMP */
    else if (on >= 0) g_udpdk.mcast_on = (uint32_t)on;
    if (!err && on == 1 && !was) {
        /* the groups joined while the switch was off are announced now */
        uint32_t *groups = malloc(4u * UDPDK_IGMP_MAX_GROUPS);
        if (groups) {
            uint32_t n = h_mcast_groups(groups, UDPDK_IGMP_MAX_GROUPS);
            if (n > UDPDK_IGMP_MAX_GROUPS) n = UDPDK_IGMP_MAX_GROUPS;
            for (uint32_t k = 0; k < n; k++) h_mcast_send(H_IGMP_REPORT, groups[k]);
            free(groups);
        }
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    if (err) { errno = err; return -1; }
    return was;
}

int udpdk_mcast_counts(udpdk_mcast_counts_t *c)
{
    if (!c) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    *c = g_udpdk.mcast_counts;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

uint64_t udpdk_rx_not_member(void) { return __atomic_load_n(&g_udpdk.rx_not_member, __ATOMIC_RELAXED); }

void h_mcast_reset(void)                  /* under tx_lock */
{
    memset(&g_udpdk.mcast_counts, 0, sizeof(g_udpdk.mcast_counts));
    __atomic_store_n(&g_udpdk.rx_not_member, 0, __ATOMIC_RELAXED);
    g_udpdk.mcast_version++;              /* (the slots' groups went with the sockets) */
}

void h_mcast_buffers_free(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    if (g_udpdk.mc_out_d && g) udpdk_gpu_free(g, g_udpdk.mc_out_d);
    if (g_udpdk.mc_groups_d && g) udpdk_gpu_free(g, g_udpdk.mc_groups_d);
    if (g_udpdk.mc_h && g) udpdk_gpu_host_free(g, g_udpdk.mc_h);
    free(g_udpdk.mc_members);
    g_udpdk.mc_out_d = g_udpdk.mc_groups_d = g_udpdk.mc_h = NULL;
    g_udpdk.mc_members = NULL;
    g_udpdk.mc_out_d_cap = g_udpdk.mc_groups_d_cap = g_udpdk.mc_h_cap = g_udpdk.mc_members_cap = 0;
    g_udpdk.mc_n_groups = 0;
    g_udpdk.mcast_applied = 0;
    pthread_mutex_lock(&g_udpdk.tx_lock);
    h_mcast_reset();
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

/* [gpu] mcast / udpdk_config_mcast, as h_peer_apply: while the switch is on the main context holds
 * the lanes' checked flags (a lane is a socket; a socket bound to a specific unicast address is
 * exempt: the demux proved the destination), the (group, socket) members and, for the IGMP stage,
 * the distinct groups; all three are uploaded again whenever a membership or the bind table changed.
 * With the switch off the stage is off. After h_snapshot_refresh, g_udpdk.lock held. */
int h_mcast_apply(void)
{
    udpdk_gpu_ctx *g = g_udpdk.gpu;
    int rc;
    if (!g_udpdk.mcast_on) {
        if (!g_udpdk.mcast_applied) return 0;
        if ((rc = udpdk_gpu_rx_mcast(g, NULL, 0, NULL, 0))) { errno = -rc; return -1; }
        g_udpdk.mcast_applied = 0;
        return 0;
    }
    if (g_udpdk.mcast_applied && g_udpdk.mcast_version_applied == g_udpdk.mcast_version &&
        g_udpdk.mcast_snap_version == g_udpdk.snap_version)
        return 0;
    const uint32_t lanes = g_udpdk.snap_lanes < UDPDK_MAX_SOCKETS ? g_udpdk.snap_lanes : UDPDK_MAX_SOCKETS;
    const uint64_t need = (uint64_t)UDPDK_MAX_SOCKETS * H_MCAST_MAX * sizeof(udpdk_mcast_member_t) +
                          4ull * UDPDK_IGMP_MAX_GROUPS + UDPDK_MAX_SOCKETS;
    if (h_grow_host(&g_udpdk.mc_members, &g_udpdk.mc_members_cap, need)) return -1;
    udpdk_mcast_member_t *mem = g_udpdk.mc_members;
    uint32_t *groups = (uint32_t *)(mem + (uint64_t)UDPDK_MAX_SOCKETS * H_MCAST_MAX);
    uint8_t *mc = (uint8_t *)(groups + UDPDK_IGMP_MAX_GROUPS);
    uint32_t nm = 0;
    for (uint32_t s = 0; s < lanes; s++) {
        const struct h_slot *sl = &g_udpdk.slots[s];
        mc[s] = sl->used && sl->bound && (sl->ip == 0u || h_is_group(sl->ip));
        for (uint32_t k = 0; sl->used && k < sl->n_mc; k++) {
            mem[nm].group = sl->mc_group[k];
            mem[nm++].lane = s;
        }
    }
    uint32_t ng = h_mcast_groups(groups, UDPDK_IGMP_MAX_GROUPS);
    if (ng > UDPDK_IGMP_MAX_GROUPS) ng = UDPDK_IGMP_MAX_GROUPS;      /* (queries for the rest: not_member) */
    if (lanes == 0) {
        rc = udpdk_gpu_rx_mcast(g, NULL, 0, NULL, 0);
    } else {
        rc = udpdk_gpu_rx_mcast(g, mc, lanes, nm ? mem : NULL, nm);
    }
    if (!rc && ng) {
        if (h_grow_dev(&g_udpdk.mc_groups_d, &g_udpdk.mc_groups_d_cap, 4ull * UDPDK_IGMP_MAX_GROUPS)) return -1;
        if (!(rc = udpdk_gpu_h2d(g, g_udpdk.mc_groups_d, groups, 4ull * ng))) rc = udpdk_gpu_sync(g);
    }
    if (rc) { errno = -rc; return -1; }
    g_udpdk.mc_n_groups = ng;
    g_udpdk.mcast_applied = 1;
    g_udpdk.mcast_version_applied = g_udpdk.mcast_version;
    g_udpdk.mcast_snap_version = g_udpdk.snap_version;
    return 0;
}

/* The IGMP stage for one staged batch (pipe 0: the one-piece poll on the context stream; 1 .. 3: a
 * chunk on its pipe, whose RX has completed). not_udp: the batch's NOT_UDP verdict count; a batch
 * of pure UDP enqueues nothing, and neither does a stack that joined no group. Synchronous: the
 * reports are queued when it returns. Returns 0, or -1 with errno. */
int h_igmp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_udp)
{
    if (!g_udpdk.mcast_on || !b->n || !not_udp || !g_udpdk.src_ip || !g_udpdk.mc_n_groups) return 0;
    int rc;
    /* the slots, then the group indices (they stay on the device: a report names its group) */
    if (h_grow_dev(&g_udpdk.mc_out_d, &g_udpdk.mc_out_d_cap, H_IGMP_OUT_BYTES + 4ull * UDPDK_IGMP_MAX_GROUPS) ||
        h_grow_pinned(&g_udpdk.mc_h, &g_udpdk.mc_h_cap, H_IGMP_OUT_BYTES))
        return -1;
    udpdk_tx_config_t cfg;
    memcpy(cfg.src_mac, g_udpdk.src_mac, 6);
    memcpy(cfg.dst_mac, g_udpdk.dst_mac, 6);
    cfg.src_ip = g_udpdk.src_ip;
    uint8_t *out_d = g_udpdk.mc_out_d, *h = g_udpdk.mc_h;
    const uint32_t ng = g_udpdk.mc_n_groups;
    const udpdk_igmp_out_t o = {out_d, (uint32_t *)(out_d + H_IGMP_OUT_BYTES), ng};
    udpdk_igmp_stats_t st;
    if (pipe) {
        if ((rc = udpdk_gpu_pipe_igmp_reply(g, pipe, &cfg, b, meta_dev, g_udpdk.mc_groups_d, ng, &o)) ||
            (rc = udpdk_gpu_pipe_wait(g, pipe))) { errno = -rc; return -1; }
        rc = udpdk_gpu_pipe_igmp_stats(g, pipe, &st);
    } else {
        if ((rc = udpdk_gpu_igmp_reply(g, &cfg, b, meta_dev, g_udpdk.mc_groups_d, ng, &o))) { errno = -rc; return -1; }
        rc = udpdk_gpu_igmp_stats(g, &st);
    }
    if (rc) { errno = -rc; return -1; }                      /* (room for every group: no -ENOSPC) */
    if (st.reports > ng) { errno = EIO; return -1; }
    if (st.reports) {
        const uint64_t bytes = (uint64_t)st.reports * UDPDK_IGMP_SLOT_BYTES;
        if (pipe) {
            if ((rc = udpdk_gpu_pipe_d2h(g, pipe, h, out_d, bytes)) || (rc = udpdk_gpu_pipe_wait(g, pipe))) {
                errno = -rc;
                return -1;
            }
        } else if ((rc = udpdk_gpu_d2h(g, h, out_d, bytes)) || (rc = udpdk_gpu_sync(g))) {
            errno = -rc;
            return -1;
        }
    }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    if (st.reports && !g_udpdk.icmpq.buf && h_icmpq_init(&g_udpdk.icmpq, H_ICMPQ_BYTES)) {
        pthread_mutex_unlock(&g_udpdk.tx_lock);
        errno = ENOMEM;
        return -1;
    }
    udpdk_mcast_counts_t *c = &g_udpdk.mcast_counts;
    for (uint32_t r = 0; r < st.reports; r++)
        if (!h_icmpq_push(&g_udpdk.icmpq, h + (uint64_t)r * UDPDK_IGMP_SLOT_BYTES, UDPDK_IGMP_FRAME_BYTES))
            c->reports_sent++;
    c->scanned++;
    c->igmp += st.igmp;
    c->malformed += st.malformed;
    c->bad_cksum += st.bad_cksum;
    c->other_type += st.other_type;
    c->bad_dst += st.bad_dst;
    c->general += st.general;
    c->not_member += st.not_member;
    c->specific += st.specific;
    c->reports += st.reports;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}
