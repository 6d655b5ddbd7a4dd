/*
 * sock_api.c — the socket calls of udpdk_api.h, the RX rings and payload slabs, the TX rings.
 *
 * Argument validation, errno values and slot state transitions follow udpdk_syscall.c
 * (socket :23-81, get/setsockopt :83-192, bind :194-245, sendto :247-368, recvfrom :370-488,
 * close :490-521). Deliberate fixes: close decrements the active count (the reference
 * increments it, :519), and sendto accepts payloads up to 65507 bytes, which
 * the poller's TX fragmentation carries (the reference writes past its 2048-byte mbuf above
 * 2006 bytes, §8 Q14); larger ones get EMSGSIZE.
 *
 * Beyond the reference: udpdk_sendmsg and the UDP_SEGMENT socket option and control message
 * (udpdk_api.h). Every send call ends in h_send_queue; a send with a segment size in force and more
 * bytes than one segment is one ring entry with its size, cut on the GPU by udpdk_tx_drain.
 *
 * sendto does what the reference's sendto does short of building the frame: validate, auto-bind,
 * queue the datagram on the socket's TX ring (ENOBUFS when full, :356-365). The frame is built
 * on the GPU by the poller's TX half (udpdk_tx_drain). recvfrom pops the socket's RX ring and
 * copies the payload out of the pinned slab the poller gathered it into on the GPU.
 */
#include <errno.h>
#include <netinet/in.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>
#include <sys/uio.h>

#include "host_state.h"

#ifndef UDPDK_RECV_PREFETCH
#define UDPDK_RECV_PREFETCH 4096u      /* bytes of the next datagram prefetched by recvfrom */
#endif

struct h_state g_udpdk;

static int h_valid_fd(int s) { return s >= 0 && s < UDPDK_MAX_SOCKETS; }

/* ---- RX rings: single producer (the poller), single consumer (recvfrom) ------------------- */
static void h_ring_clear(struct h_ring *r)
{
    h_arena_release(r->rel_arena, r->rel_n);
    r->rel_arena = NULL;
    r->rel_n = 0;
    if (r->e) {
        const uint32_t t = atomic_load_explicit(&r->tail, memory_order_acquire);
        for (uint32_t i = atomic_load_explicit(&r->head, memory_order_relaxed); i != t; i++)
            h_arena_release(r->e[i % UDPDK_RX_RING_SIZE].arena, 1);
        free(r->e);
    }
    r->e = NULL;
    atomic_store_explicit(&r->head, 0, memory_order_relaxed);
    atomic_store_explicit(&r->tail, 0, memory_order_relaxed);
}

/* Entries the producer may still add (usable size = size - 1, as rte_ring). */
uint32_t h_ring_free(const struct h_ring *r)
{
    const uint32_t h = atomic_load_explicit(&r->head, memory_order_acquire);
    const uint32_t t = atomic_load_explicit(&r->tail, memory_order_relaxed);
    return (UDPDK_RX_RING_SIZE - 1) - (t - h);
}

/* All-or-nothing append of n datagrams (rte_ring_enqueue_bulk, poller.c:287-290): the entries
 * are written first, then published by a release store of tail that recvfrom acquires. */
int h_ring_push_bulk(struct h_ring *r, const struct h_dgram *d, uint32_t n)
{
    if (!r->e) {
        r->e = calloc(UDPDK_RX_RING_SIZE, sizeof(*r->e));
        if (!r->e) return -1;
    }
    if (n > h_ring_free(r)) return -1;
    const uint32_t t = atomic_load_explicit(&r->tail, memory_order_relaxed);
    for (uint32_t i = 0; i < n; i++) r->e[(t + i) % UDPDK_RX_RING_SIZE] = d[i];
    atomic_store_explicit(&r->tail, t + n, memory_order_release);
    return 0;
}

/* One datagram into socket s's ring from caller-owned bytes (udpdk_api.h: poller internals). */
int udpdk_sock_rx_inject(int s, const void *data, uint32_t len, uint32_t src_ip, uint16_t src_port)
{
    if (!h_valid_fd(s)) { errno = ENOTSOCK; return -1; }
    pthread_mutex_lock(&g_udpdk.lock);                 /* the poller's lock: one producer at a time */
    int rc = -1;
    if (!g_udpdk.slots[s].used) {
        errno = EBADF;
    } else {
        const struct h_dgram d = {data, len, src_ip, src_port, NULL};
        rc = h_ring_push_bulk(&g_udpdk.slots[s].rx, &d, 1);
        if (rc) errno = ENOBUFS;
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    return rc;
}

/* ---- payload slabs ------------------------------------------------------------------------ */
#define H_ARENA_FREE_KEEP 32     /* free slabs kept for reuse; the rest go back to the runtime
                                  * (a pipelined poll makes a slab per chunk: with 8 kept, every
                                  * 1 M x 1500 B poll freed and re-pinned three 140 MB slabs) */

/* frees a slab's memory; the budget accounting is the caller's */
static void h_arena_destroy(struct h_arena *a)
{
    if (!a) return;
    void *p[] = {a->payload, a->len, a->src_ip, a->src_port};
    for (unsigned k = 0; k < 4; k++)
        if (p[k] && g_udpdk.gpu) udpdk_gpu_host_free(g_udpdk.gpu, p[k]);
    free(a);
}

static uint64_t h_arena_footprint(uint64_t cb, uint32_t cn) { return cb + 10ull * cn; }

/* A slab for n datagrams in `need` bytes of packed slots: the first free one that is large
 * enough, else a new one (pinned, so the gather's D2H is a straight DMA) if the slab budget
 * allows it after the free slabs that do not fit have been released. NULL + ENOBUFS when the
 * budget is exhausted by slabs that queued datagrams still hold (the reference's mbuf pool
 * exhausted: the burst is not received). */
struct h_arena *h_arena_get(uint32_t n, uint64_t need)
{
    pthread_mutex_lock(&g_udpdk.arena_lock);
    /* the smallest free slab that fits (a pipelined poll asks for one slab per chunk, of
     * similar sizes: first fit handed a chunk a larger one that a later chunk then missed) */
    struct h_arena **best = NULL, *a = NULL;
    for (struct h_arena **pp = &g_udpdk.arena_free; *pp; pp = &(*pp)->next)
        if ((*pp)->cap_bytes >= need && (*pp)->cap_n >= n && (!best || (*pp)->cap_bytes < (*best)->cap_bytes))
            best = pp;
    if (best) {
        a = *best;
        *best = a->next;
        g_udpdk.arena_free_n--;
    }
    /* a new slab's capacity rounded up to 1/8 of its power of two (<= 12.5 % more), so the next
     * poll's slightly larger chunk still fits it */
    const uint32_t cn0 = n < 4096 ? 4096 : n;
    const uint32_t cn = cn0 > (1u << 16) ? (cn0 + 8191u) & ~8191u : cn0;
    uint64_t cb = need < ((uint64_t)cn * 64) ? (uint64_t)cn * 64 : need;
    if (cb > (1ull << 20)) {
        uint64_t p2 = 1ull << 20;
        while (p2 <= cb / 2) p2 <<= 1;
        const uint64_t g = p2 / 8;
        cb = (cb + g - 1) / g * g;
    }
    if (!a) {
        const uint64_t fp = h_arena_footprint(cb, cn);
        /* release free slabs (none fits) until the new one fits the budget */
        while ((g_udpdk.arena_bytes + fp > g_udpdk.arena_bytes_max ||
                g_udpdk.arena_count + 1 > g_udpdk.arena_count_max) && g_udpdk.arena_free) {
            struct h_arena *f = g_udpdk.arena_free;
            g_udpdk.arena_free = f->next;
            g_udpdk.arena_free_n--;
            g_udpdk.arena_bytes -= h_arena_footprint(f->cap_bytes, f->cap_n);
            g_udpdk.arena_count--;
            h_arena_destroy(f);
        }
        if (g_udpdk.arena_bytes + fp > g_udpdk.arena_bytes_max ||
            g_udpdk.arena_count + 1 > g_udpdk.arena_count_max) {
            pthread_mutex_unlock(&g_udpdk.arena_lock);
            errno = ENOBUFS;
            return NULL;
        }
        g_udpdk.arena_bytes += fp;         /* reserved before the allocation */
        g_udpdk.arena_count++;
    }
    pthread_mutex_unlock(&g_udpdk.arena_lock);
    if (!a) {
        a = calloc(1, sizeof(*a));
        if (a && (udpdk_gpu_host_alloc(g_udpdk.gpu, cb, (void **)&a->payload) ||
                  udpdk_gpu_host_alloc(g_udpdk.gpu, 4ull * cn, (void **)&a->len) ||
                  udpdk_gpu_host_alloc(g_udpdk.gpu, 4ull * cn, (void **)&a->src_ip) ||
                  udpdk_gpu_host_alloc(g_udpdk.gpu, 2ull * cn, (void **)&a->src_port))) {
            h_arena_destroy(a);
            a = NULL;
        }
        if (!a) {
            pthread_mutex_lock(&g_udpdk.arena_lock);
            g_udpdk.arena_bytes -= h_arena_footprint(cb, cn);
            g_udpdk.arena_count--;
            pthread_mutex_unlock(&g_udpdk.arena_lock);
            errno = ENOMEM;
            return NULL;
        }
        a->cap_bytes = cb;
        a->cap_n = cn;
    }
    a->next = NULL;
    atomic_store_explicit(&a->refs, 0, memory_order_relaxed);
    return a;
}

/* Back to the pool; beyond H_ARENA_FREE_KEEP free slabs the largest goes back to the runtime,
 * so one burst of huge polls does not keep its slabs pinned forever. */
void h_arena_put(struct h_arena *a)
{
    pthread_mutex_lock(&g_udpdk.arena_lock);
    a->next = g_udpdk.arena_free;
    g_udpdk.arena_free = a;
    g_udpdk.arena_free_n++;
    struct h_arena *victim = NULL;
    if (g_udpdk.arena_free_n > H_ARENA_FREE_KEEP) {
        struct h_arena **vp = &g_udpdk.arena_free;
        for (struct h_arena **pp = &g_udpdk.arena_free; *pp; pp = &(*pp)->next)
            if ((*pp)->cap_bytes > (*vp)->cap_bytes) vp = pp;
        victim = *vp;
        *vp = victim->next;
        g_udpdk.arena_free_n--;
        g_udpdk.arena_bytes -= h_arena_footprint(victim->cap_bytes, victim->cap_n);
        g_udpdk.arena_count--;
    }
    pthread_mutex_unlock(&g_udpdk.arena_lock);
    h_arena_destroy(victim);
}

/* Drop refs references (recvfrom of one datagram, or a ring cleared by close); the last one
 * returns the slab to the pool. */
void h_arena_release(struct h_arena *a, uint32_t refs)
{
    if (a && refs && atomic_fetch_sub_explicit(&a->refs, refs, memory_order_acq_rel) == refs)
        h_arena_put(a);
}

void h_arenas_free_all(void)
{
    pthread_mutex_lock(&g_udpdk.arena_lock);
    struct h_arena *a = g_udpdk.arena_free;
    g_udpdk.arena_free = NULL;
    g_udpdk.arena_free_n = 0;
    while (a) {
        struct h_arena *n = a->next;
        g_udpdk.arena_bytes -= h_arena_footprint(a->cap_bytes, a->cap_n);
        g_udpdk.arena_count--;
        h_arena_destroy(a);
        a = n;
    }
    pthread_mutex_unlock(&g_udpdk.arena_lock);
}

uint64_t udpdk_rx_nobufs(void) { return __atomic_load_n(&g_udpdk.rx_nobufs, __ATOMIC_RELAXED); }

uint64_t udpdk_rx_dropped(void) { return __atomic_load_n(&g_udpdk.rx_dropped, __ATOMIC_RELAXED); }
uint64_t udpdk_rx_balanced(void) { return __atomic_load_n(&g_udpdk.rx_balanced, __ATOMIC_RELAXED); }
uint64_t udpdk_rx_refused(void) { return __atomic_load_n(&g_udpdk.rx_refused, __ATOMIC_RELAXED); }

/* ---- TX rings ----------------------------------------------------------------------------- */
void h_tx_reset(void)
{
    pthread_mutex_lock(&g_udpdk.tx_lock);
    for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
        free(g_udpdk.slots[s].tx.e);
        g_udpdk.slots[s].tx.e = NULL;
        g_udpdk.slots[s].tx.head = g_udpdk.slots[s].tx.tail = 0;
    }
    free(g_udpdk.txp);
    g_udpdk.txp = NULL;
    g_udpdk.txp_bytes = g_udpdk.txp_cap = 0;
    g_udpdk.tx_queued = 0;
    g_udpdk.tx_dropped = 0;
    memset(&g_udpdk.gso_counts, 0, sizeof(g_udpdk.gso_counts));
    pthread_mutex_unlock(&g_udpdk.tx_lock);
}

uint64_t udpdk_tx_pending(void)
{
    pthread_mutex_lock(&g_udpdk.tx_lock);
    const uint64_t q = g_udpdk.tx_queued + g_udpdk.icmpq.count;   /* (the poller gates its drain on this) */
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return q;
}

uint64_t udpdk_tx_dropped(void)
{
    pthread_mutex_lock(&g_udpdk.tx_lock);
    const uint64_t q = g_udpdk.tx_dropped;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return q;
}

int udpdk_gso_counts(udpdk_gso_counts_t *counts)
{
    if (!counts) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.tx_lock);
    *counts = g_udpdk.gso_counts;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return 0;
}

void h_sockets_reset(void)
{
    for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {
        h_ring_clear(&g_udpdk.slots[s].rx);
        free(g_udpdk.slots[s].tx.e);
        memset(&g_udpdk.slots[s], 0, sizeof(g_udpdk.slots[s]));
        g_udpdk.slots[s].prev = g_udpdk.slots[s].next = -1;
    }
    g_udpdk.n_active = 0;
    free(g_udpdk.txp);
    g_udpdk.txp = NULL;
    g_udpdk.txp_bytes = g_udpdk.txp_cap = 0;
    g_udpdk.tx_queued = 0;
    g_udpdk.tx_dropped = 0;
    memset(&g_udpdk.gso_counts, 0, sizeof(g_udpdk.gso_counts));
    __atomic_store_n(&g_udpdk.rx_nobufs, 0, __ATOMIC_RELAXED);   /* per library session */
    __atomic_store_n(&g_udpdk.rx_dropped, 0, __ATOMIC_RELAXED);
    __atomic_store_n(&g_udpdk.rx_balanced, 0, __ATOMIC_RELAXED);
    __atomic_store_n(&g_udpdk.rx_refused, 0, __ATOMIC_RELAXED);
    g_udpdk.mcast_version++;                   /* (the slots' groups went with the memset too) */
    g_udpdk.n_connected = 0;                   /* (the slots' peers went with the memset) */
    g_udpdk.peer_version++;
    g_udpdk.version++;
}

/* ---- socket calls ------------------------------------------------------------------------- */
int udpdk_socket(int domain, int type, int protocol)
{
    if (domain != AF_INET) { errno = EAFNOSUPPORT; return -1; }
    if (type != SOCK_DGRAM) { errno = EPROTONOSUPPORT; return -1; }
    if (protocol != 0 && protocol != IPPROTO_UDP) { errno = EINVAL; return -1; }
    pthread_mutex_lock(&g_udpdk.lock);
    int ret = -1;
    if (g_udpdk.n_active >= UDPDK_MAX_SOCKETS) {
        errno = ENOBUFS;
    } else {
        for (int s = 0; s < UDPDK_MAX_SOCKETS; s++) {   /* lowest free slot */
            struct h_slot *sl = &g_udpdk.slots[s];
            if (sl->used) continue;
            sl->used = 1;
            sl->bound = 0;
            sl->so_options = 0;
            sl->ip = 0;
            sl->udp_port = 0;
            sl->connected = 0;
            sl->gso_size = 0;
            sl->n_mc = 0;
            atomic_store(&sl->so_error, 0);
            sl->prev = sl->next = -1;
            g_udpdk.n_active++;
            ret = s;
            break;
        }
        if (ret < 0) errno = ENOBUFS;
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    return ret;
}

static int h_sockopt_check(int s, int level, int optname, const void *optval, const void *optlen)
{
    if (!h_valid_fd(s) || !g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (level != SOL_SOCKET) { errno = EINVAL; return -1; }
    if (optname != SO_REUSEADDR && optname != SO_REUSEPORT) { errno = ENOPROTOOPT; return -1; }
    if (!optval || !optlen) { errno = EFAULT; return -1; }
    return 0;
}

/* IPPROTO_UDP / UDP_SEGMENT of a socket in use: the segment size of the socket's later sends (any
 * other option of that level keeps the answer every unknown level gets, EINVAL). set: optval is the
 * new value, else it receives the stored one. */
static int h_udp_sockopt(int s, void *optval, socklen_t *optlen, int set)
{
    if (!optval || !optlen) { errno = EFAULT; return -1; }
    if (set) {
        if (*optlen < sizeof(int)) { errno = EINVAL; return -1; }
        const int v = *(const int *)optval;
        if (v < 0 || v > 65535) { errno = EINVAL; return -1; }
        g_udpdk.slots[s].gso_size = (uint16_t)v;
        return 0;
    }
    *(int *)optval = g_udpdk.slots[s].gso_size;
    *optlen = sizeof(int);
    return 0;
}

int udpdk_getsockopt(int s, int level, int optname, void *optval, socklen_t *optlen)
{
    if (level == IPPROTO_UDP && optname == UDP_SEGMENT && h_valid_fd(s) && g_udpdk.slots[s].used)
        return h_udp_sockopt(s, optval, optlen, 0);
    if (optname == SO_ERROR && level == SOL_SOCKET && h_valid_fd(s) && g_udpdk.slots[s].used) {
        /* the pending ICMP error (udpdk_config_icmp_errors), cleared by the read; 0: none */
        if (!optval || !optlen) { errno = EFAULT; return -1; }
        *(int *)optval = h_sock_error_take(s);
        *optlen = sizeof(int);
        return 0;
    }
    if (h_sockopt_check(s, level, optname, optval, optlen)) return -1;
    /* bitwise test of the option value: SO_REUSEPORT (15) contains SO_REUSEADDR (2), so
     * setting REUSEPORT reads back REUSEADDR = 1 as in the reference */
    *(int *)optval = (g_udpdk.slots[s].so_options & optname) != 0;
    return 0;
}

int udpdk_setsockopt(int s, int level, int optname, const void *optval, socklen_t optlen)
{
    /* IP_ADD_MEMBERSHIP / IP_DROP_MEMBERSHIP (mcast.c); any other IPPROTO_IP option: ENOPROTOOPT */
    if (level == IPPROTO_IP && h_valid_fd(s) && g_udpdk.slots[s].used) return h_mcast_sockopt(s, optname, optval, optlen);
    if (level == IPPROTO_UDP && optname == UDP_SEGMENT && h_valid_fd(s) && g_udpdk.slots[s].used)
        return h_udp_sockopt(s, (void *)optval, &optlen, 1);
    if (h_sockopt_check(s, level, optname, optval, &optlen)) return -1;
    struct h_slot *sl = &g_udpdk.slots[s];
    const int was = sl->so_options & optname;
    const int want = *(const int *)optval != 0;
    if (want && !was) sl->so_options |= optname;
    else if (!want && was) sl->so_options &= ~optname;
    return 0;
}

static int h_bind_locked(int s, const struct sockaddr *addr, socklen_t addrlen)
{
    if (!h_valid_fd(s) || !g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (g_udpdk.slots[s].bound) { errno = EINVAL; return -1; }
    if (!addr || addr->sa_family != AF_INET) { errno = EINVAL; return -1; }
    if (addrlen != sizeof(struct sockaddr_in)) { errno = EINVAL; return -1; }
    const struct sockaddr_in *in = (const struct sockaddr_in *)addr;
    const uint32_t port = in->sin_port;            /* raw network-order value */
    const uint32_t ip = in->sin_addr.s_addr;
    if (h_btable_add(s, ip, port, g_udpdk.slots[s].so_options) < 0) { errno = EADDRINUSE; return -1; }
    g_udpdk.slots[s].bound = 1;
    g_udpdk.slots[s].udp_port = port;
    g_udpdk.slots[s].ip = ip;
    return 0;
}

int udpdk_bind(int s, const struct sockaddr *addr, socklen_t addrlen)
{
    pthread_mutex_lock(&g_udpdk.lock);
    const int rc = h_bind_locked(s, addr, addrlen);
    pthread_mutex_unlock(&g_udpdk.lock);
    return rc;
}

int udpdk_close(int s)
{
    pthread_mutex_lock(&g_udpdk.lock);
    if (!h_valid_fd(s) || !g_udpdk.slots[s].used) {
        pthread_mutex_unlock(&g_udpdk.lock);
        errno = EBADF;
        return -1;
    }
    struct h_slot *sl = &g_udpdk.slots[s];
    /* a recvfrom blocked on this socket in another thread leaves with EBADF before the ring's
     * entries and storage go (it would otherwise read freed entries) */
    atomic_store(&sl->rx.closing, 1);
    while (atomic_load(&sl->rx.busy)) sched_yield();
    if (sl->bound) h_btable_del(s, sl->udp_port);
    h_ring_clear(&sl->rx);
    pthread_mutex_lock(&g_udpdk.tx_lock);
    if (sl->tx.e) {
        g_udpdk.tx_queued -= sl->tx.tail - sl->tx.head;   /* queued sends die with the socket */
        free(sl->tx.e);
    }
    sl->tx.e = NULL;
    sl->tx.head = sl->tx.tail = 0;
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    atomic_store(&sl->so_error, 0);
    h_mcast_close_locked(s);                   /* the groups go with the socket (the last holder's: a leave) */
    if (sl->connected) {                       /* the peer goes with the socket */
        sl->connected = 0;
        g_udpdk.n_connected--;
        g_udpdk.peer_version++;
    }
    sl->bound = 0;
    sl->used = 0;
    sl->so_options = 0;
    sl->gso_size = 0;
    g_udpdk.n_active--;
    g_udpdk.version++;
    atomic_store(&sl->rx.closing, 0);          /* later calls see used == 0 */
    pthread_mutex_unlock(&g_udpdk.lock);
    return 0;
}

/* Auto-bind an unbound socket to ANY on the lowest free raw port (udpdk_syscall.c:294-304). */
static int h_autobind_locked(int s)
{
    if (g_udpdk.slots[s].bound) return 0;
    struct sockaddr_in a;
    memset(&a, 0, sizeof(a));
    a.sin_family = AF_INET;
    a.sin_addr.s_addr = INADDR_ANY;
    const int p = h_btable_free_port();
    if (p < 0) { errno = EADDRINUSE; return -1; }
    a.sin_port = (uint16_t)p;
    return h_bind_locked(s, (const struct sockaddr *)&a, sizeof(a));
}

/* The socket's peer as a sockaddr_in; returns whether it has one. g_udpdk.lock held. */
static int h_peer_locked(int s, struct sockaddr_in *a)
{
    const struct h_slot *sl = &g_udpdk.slots[s];
    memset(a, 0, sizeof(*a));
    if (!sl->used || !sl->connected) return 0;
    a->sin_family = AF_INET;
    a->sin_port = sl->peer_port;
    a->sin_addr.s_addr = sl->peer_ip;
    return 1;
}

/* What every send call ends in: the payload is the iovecs gathered in order, gso the segment size a
 * control message gave (-1: the socket's), bad_cmsg whether the control messages were refused
 * (reported where Linux reports it, after the pending error). Validates, auto-binds and queues one
 * ring entry; returns the payload's length or -1 with errno. */
static ssize_t h_send_queue(int s, const struct iovec *iov, size_t iovcnt, int flags, const struct sockaddr *dest,
                            socklen_t addrlen, int gso, int bad_cmsg)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (flags != 0) { errno = EINVAL; return -1; }
    { const int e = h_sock_error_take(s); if (e) { errno = e; return -1; } }   /* pending ICMP error */
    if (bad_cmsg) { errno = EINVAL; return -1; }
    struct sockaddr_in peer;
    if (!dest) {
        /* a connected socket's peer (udpdk_connect); unconnected: EINVAL as ever */
        pthread_mutex_lock(&g_udpdk.lock);
        const int conn = h_peer_locked(s, &peer);
        pthread_mutex_unlock(&g_udpdk.lock);
        if (!conn) { errno = EINVAL; return -1; }
        dest = (const struct sockaddr *)&peer;
        addrlen = sizeof(peer);
    }
    if (addrlen == 0) { errno = EINVAL; return -1; }
    if (iovcnt && !iov) { errno = EFAULT; return -1; }
    uint64_t len = 0;
    for (size_t i = 0; i < iovcnt; i++) {
        len += iov[i].iov_len < (1u << 20) ? iov[i].iov_len : (1u << 20);    /* (anything above 65507 is too long) */
        if (len > (1u << 20)) len = 1u << 20;
    }
    const uint32_t g = gso >= 0 ? (uint32_t)gso : g_udpdk.slots[s].gso_size;
    if (g && (28u + g > g_udpdk.mtu || len > (uint64_t)g * UDPDK_GSO_MAX_SEGS)) {
        /* udp_send_skb: a segment must fit the MTU, a send at most UDP_MAX_SEGMENTS segments */
        pthread_mutex_lock(&g_udpdk.tx_lock);
        g_udpdk.gso_counts.refused++;
        pthread_mutex_unlock(&g_udpdk.tx_lock);
        errno = EINVAL;
        return -1;
    }
    if (len > H_UDP_MAX_PAYLOAD) { errno = EMSGSIZE; return -1; }
    for (size_t i = 0; i < iovcnt; i++)
        if (iov[i].iov_len && !iov[i].iov_base) { errno = EFAULT; return -1; }
    pthread_mutex_lock(&g_udpdk.lock);
    const int rc = h_autobind_locked(s);
    pthread_mutex_unlock(&g_udpdk.lock);
    if (rc) return -1;
    const struct sockaddr_in *d = (const struct sockaddr_in *)dest;
    pthread_mutex_lock(&g_udpdk.tx_lock);
    struct h_txq *q = &g_udpdk.slots[s].tx;
    ssize_t ret = -1;
    if (!q->e && !(q->e = malloc(UDPDK_RX_RING_SIZE * sizeof(*q->e)))) {
        errno = ENOMEM;
    } else if (q->tail - q->head >= UDPDK_RX_RING_SIZE - 1) {
        errno = ENOBUFS;                           /* rte_ring_enqueue failed (:356-365) */
    } else {
        const uint64_t need = g_udpdk.txp_bytes + len;
        if (need > g_udpdk.txp_cap) {
            uint64_t nc = g_udpdk.txp_cap ? g_udpdk.txp_cap * 2 : (1u << 20);
            while (nc < need) nc *= 2;
            uint8_t *np = realloc(g_udpdk.txp, nc);
            if (!np) { errno = ENOMEM; goto out; }
            g_udpdk.txp = np;
            g_udpdk.txp_cap = nc;
        }
        struct h_txd *t = &q->e[q->tail % UDPDK_RX_RING_SIZE];
        t->pay = g_udpdk.txp_bytes;
        t->len = (uint32_t)len;
        t->dst_ip = d->sin_addr.s_addr;
        t->dst_port = d->sin_port;
        t->gso = g && len > g ? g : 0u;            /* (len <= g: an ordinary datagram) */
        for (size_t i = 0; i < iovcnt; i++) {      /* stored once, contiguously */
            if (iov[i].iov_len) memcpy(g_udpdk.txp + g_udpdk.txp_bytes, iov[i].iov_base, iov[i].iov_len);
            g_udpdk.txp_bytes += iov[i].iov_len;
        }
        if (t->gso) {
            g_udpdk.gso_counts.sends++;
            g_udpdk.gso_counts.segments += (len + g - 1u) / g;
        }
        q->tail++;
        g_udpdk.tx_queued++;
        ret = (ssize_t)len;
    }
out:
    pthread_mutex_unlock(&g_udpdk.tx_lock);
    return ret;
}

ssize_t udpdk_sendto(int s, const void *buf, size_t len, int flags,
                     const struct sockaddr *dest, socklen_t addrlen)
{
    const struct iovec v = {(void *)buf, len};
    return h_send_queue(s, &v, 1, flags, dest, addrlen, -1, 0);
}

ssize_t udpdk_sendmsg(int s, const struct msghdr *msg, int flags)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (!msg) { errno = EFAULT; return -1; }
    /* the control messages: SOL_UDP / UDP_SEGMENT with a uint16_t is this call's segment size */
    int gso = -1, bad = 0;
    if (msg->msg_control && msg->msg_controllen) {
        for (struct cmsghdr *c = CMSG_FIRSTHDR((struct msghdr *)msg); c; c = CMSG_NXTHDR((struct msghdr *)msg, c)) {
            if (c->cmsg_level != SOL_UDP || c->cmsg_type != UDP_SEGMENT || c->cmsg_len != CMSG_LEN(sizeof(uint16_t))) {
                bad = 1;
                break;
            }
            uint16_t v;
            memcpy(&v, CMSG_DATA(c), sizeof(v));
            gso = v;
        }
    }
    return h_send_queue(s, msg->msg_iov, msg->msg_iovlen, flags, msg->msg_name ? (const struct sockaddr *)msg->msg_name : NULL,
                        msg->msg_name ? msg->msg_namelen : 0, gso, bad);
}

ssize_t udpdk_recvfrom(int s, void *buf, size_t len, int flags,
                       struct sockaddr *src_addr, socklen_t *addrlen)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (flags != 0) { errno = EINVAL; return -1; }
    if (buf == NULL && addrlen != NULL) { errno = EINVAL; return -1; }
    struct h_ring *r = &g_udpdk.slots[s].rx;
    atomic_fetch_add(&r->busy, 1);             /* seq_cst: see udpdk_close */
    if (atomic_load(&r->closing) || !g_udpdk.slots[s].used) {
        atomic_fetch_sub_explicit(&r->busy, 1, memory_order_release);
        errno = EBADF;
        return -1;
    }
    const uint32_t h = atomic_load_explicit(&r->head, memory_order_relaxed);
    /* a pending ICMP error is reported before ring data, which stays queued for the next call */
    int perr = h_sock_error_take(s);
    /* busy wait like udpdk_syscall.c:424-426; datagrams arrive from the poller (udpdk_poll_rx) */
    while (!perr && atomic_load_explicit(&r->tail, memory_order_acquire) == h) {
        const int intr = atomic_load_explicit(&g_udpdk.interrupted, memory_order_relaxed);
        if (intr || atomic_load_explicit(&r->closing, memory_order_relaxed)) {
            atomic_fetch_sub_explicit(&r->busy, 1, memory_order_release);
            errno = intr ? EINTR : EBADF;
            return -1;
        }
        sched_yield();
        perr = h_sock_error_take(s);
    }
    if (perr) {
        atomic_fetch_sub_explicit(&r->busy, 1, memory_order_release);
        errno = perr;
        return -1;
    }
    const struct h_dgram d = r->e[h % UDPDK_RX_RING_SIZE];
    if (src_addr && addrlen) {
        struct sockaddr_in a;
        memset(&a, 0, sizeof(a));
        a.sin_family = AF_INET;
        a.sin_port = (uint16_t)d.src_port;
        a.sin_addr.s_addr = d.src_ip;
        const socklen_t n = sizeof(a) <= *addrlen ? (socklen_t)sizeof(a) : *addrlen;
        memcpy(src_addr, &a, n);
        *addrlen = n;
    }
    const uint32_t t = atomic_load_explicit(&r->tail, memory_order_acquire);
    if (t != h + 1) {
        /* the next datagram's bytes are fetched while this one is copied: recvfrom at 1500 B is
         * one memcpy out of host memory per call, bound by the core's cache misses (two entries
         * ahead measured even at 1500 B and 8 % slower at IMIX). Only the first
         * UDPDK_RECV_PREFETCH bytes: a 64 KiB datagram would otherwise issue 1024 prefetches
         * competing with this call's own copy (the hardware prefetcher follows the memcpy's
         * stream past them) */
        const struct h_dgram *nx = &r->e[(h + 1) % UDPDK_RX_RING_SIZE];
        const char *np = (const char *)nx->data;
        const uint32_t pf = nx->len < UDPDK_RECV_PREFETCH ? nx->len : UDPDK_RECV_PREFETCH;
        for (uint32_t o = 0; o < pf; o += 64) __builtin_prefetch(np + o);
    }
    const size_t n = d.len < len ? d.len : len;
    if (n) memcpy(buf, d.data, n);
    /* the slab reference goes back once per run of one slab's entries: when the next entry is
     * another slab's or the ring is drained (a consumed entry never holds its slab longer than an
     * unconsumed one would) */
    if (d.arena != r->rel_arena) {
        h_arena_release(r->rel_arena, r->rel_n);
        r->rel_arena = d.arena;
        r->rel_n = 0;
    }
    r->rel_n++;
    const bool run_ends = t == h + 1 || r->e[(h + 1) % UDPDK_RX_RING_SIZE].arena != d.arena;
    atomic_store_explicit(&r->head, h + 1, memory_order_release);
    if (run_ends) {
        h_arena_release(r->rel_arena, r->rel_n);
        r->rel_arena = NULL;
        r->rel_n = 0;
    }
    atomic_fetch_sub_explicit(&r->busy, 1, memory_order_release);
    return (ssize_t)n;
}

/* ---- connected sockets -------------------------------------------------------------------- */
int udpdk_connect(int s, const struct sockaddr *addr, socklen_t addrlen)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (!addr || addrlen < sizeof(sa_family_t)) { errno = EINVAL; return -1; }
    if (addr->sa_family != AF_INET && addr->sa_family != AF_UNSPEC) { errno = EAFNOSUPPORT; return -1; }
    if (addr->sa_family == AF_INET && addrlen < sizeof(struct sockaddr_in)) { errno = EINVAL; return -1; }
    int ret = -1;
    pthread_mutex_lock(&g_udpdk.lock);
    struct h_slot *sl = &g_udpdk.slots[s];
    if (!sl->used) {
        errno = EBADF;
    } else if (addr->sa_family == AF_UNSPEC) {             /* dissolve the association */
        atomic_store(&sl->so_error, 0);                    /* an error about the old peer goes with it */
        if (sl->connected) {
            sl->connected = 0;
            g_udpdk.n_connected--;
            g_udpdk.peer_version++;
        }
        ret = 0;
    } else if (h_autobind_locked(s) == 0) {
        const struct sockaddr_in *in = (const struct sockaddr_in *)addr;
        if (!sl->connected) g_udpdk.n_connected++;
        sl->connected = 1;
        sl->peer_ip = in->sin_addr.s_addr;
        sl->peer_port = in->sin_port;                      /* raw network-order value */
        atomic_store(&sl->so_error, 0);
        g_udpdk.peer_version++;                            /* the next poll uploads the table */
        ret = 0;
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    return ret;
}

ssize_t udpdk_send(int s, const void *buf, size_t len, int flags)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    struct sockaddr_in peer;
    pthread_mutex_lock(&g_udpdk.lock);
    const int conn = h_peer_locked(s, &peer);
    pthread_mutex_unlock(&g_udpdk.lock);
    if (!conn) { errno = ENOTCONN; return -1; }
    return udpdk_sendto(s, buf, len, flags, (const struct sockaddr *)&peer, sizeof(peer));
}

ssize_t udpdk_recv(int s, void *buf, size_t len, int flags)
{
    return udpdk_recvfrom(s, buf, len, flags, NULL, NULL);
}

static int h_name_out(const struct sockaddr_in *a, struct sockaddr *addr, socklen_t *addrlen)
{
    const socklen_t n = sizeof(*a) <= *addrlen ? (socklen_t)sizeof(*a) : *addrlen;
    memcpy(addr, a, n);
    *addrlen = n;
    return 0;
}

int udpdk_getpeername(int s, struct sockaddr *addr, socklen_t *addrlen)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (!addr || !addrlen) { errno = EINVAL; return -1; }
    struct sockaddr_in a;
    pthread_mutex_lock(&g_udpdk.lock);
    const int conn = h_peer_locked(s, &a);
    pthread_mutex_unlock(&g_udpdk.lock);
    if (!conn) { errno = ENOTCONN; return -1; }
    return h_name_out(&a, addr, addrlen);
}

int udpdk_getsockname(int s, struct sockaddr *addr, socklen_t *addrlen)
{
    if (s < 0 || s >= UDPDK_MAX_SOCKETS) { errno = ENOTSOCK; return -1; }
    if (!g_udpdk.slots[s].used) { errno = EBADF; return -1; }
    if (!addr || !addrlen) { errno = EINVAL; return -1; }
    struct sockaddr_in a;
    memset(&a, 0, sizeof(a));
    a.sin_family = AF_INET;
    pthread_mutex_lock(&g_udpdk.lock);
    const struct h_slot *sl = &g_udpdk.slots[s];
    if (sl->used && sl->bound) {                           /* unbound: 0.0.0.0:0 */
        a.sin_port = (uint16_t)sl->udp_port;
        a.sin_addr.s_addr = sl->ip;
    }
    pthread_mutex_unlock(&g_udpdk.lock);
    return h_name_out(&a, addr, addrlen);
}

int udpdk_peer_lanes(udpdk_peer_t *peers, uint32_t n)
{
    if (!peers && n) return -EINVAL;
    int cnt = 0;
    pthread_mutex_lock(&g_udpdk.lock);
    for (uint32_t s = 0; s < UDPDK_MAX_SOCKETS; s++) {
        const struct h_slot *sl = &g_udpdk.slots[s];
        const int on = sl->used && sl->connected;
        if (s < n) {
            peers[s].ip = on ? sl->peer_ip : 0u;
            peers[s].port = on ? sl->peer_port : 0u;
            peers[s].on = (uint16_t)on;
        }
        cnt += on;
    }
    for (uint32_t s = UDPDK_MAX_SOCKETS; s < n; s++) memset(&peers[s], 0, sizeof(peers[s]));
    pthread_mutex_unlock(&g_udpdk.lock);
    return cnt;
}

int udpdk_slot_table(udpdk_slot_t *slots, uint32_t n_slots)
{
    if (!slots) { errno = EINVAL; return -1; }
    for (uint32_t s = 0; s < n_slots; s++) {
        const struct h_slot *sl = s < UDPDK_MAX_SOCKETS ? &g_udpdk.slots[s] : NULL;
        slots[s].ip = sl ? sl->ip : 0u;
        slots[s].udp_port = sl ? sl->udp_port : 0u;
        slots[s].bound = sl ? (uint32_t)sl->bound : 0u;
    }
    return 0;
}
