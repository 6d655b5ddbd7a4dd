/*
 * host_state.h — process-wide state of the host layer behind udpdk_api.h (internal).
 *
 * The reference keeps this state in DPDK memzones shared by the app and the forked poller
 * (exch_zone_desc, exch_slots, sock_bind_table: udpdk_globals.c:9-37, udpdk_init.c:226-279).
 * Here the application and the poller are threads of one process: plain static memory, one lock
 * for the bind table / socket slots (taken by socket, bind, close and by the poller while it
 * reads the table and fills rings), one for the TX queues, and lock-free single-producer /
 * single-consumer RX rings between the poller and recvfrom (rte_ring SP/SC, init.c:270-272).
 */
#ifndef UDPDK_HOST_STATE_H
#define UDPDK_HOST_STATE_H

#include <pthread.h>
#include <stdatomic.h>
#include <stdint.h>
#include <sys/types.h>

#include "udpdk_api.h"
#include "icmp_queue.h"

/* Linux values the reference relies on (udpdk_syscall.c:102-105, :167, :174). */
#define H_SO_REUSEADDR 2
#define H_SO_REUSEPORT 15

#define H_BURST_SIZE     128     /* BURST_SIZE, udpdk_constants.h:41 */
#define H_MAX_WORKERS    31      /* poll worker threads beyond the caller's ([gpu] poll_threads) */
#define H_POLL_THREADS_DEFAULT 8
#define H_UDP_MAX_PAYLOAD 65507  /* 65535 - 20 - 8: the largest datagram fragmentation can carry */
#define H_MCAST_MAX      20      /* groups a socket can join: Linux's igmp_max_memberships default */

/* A pinned host slab of gathered payloads: one per rx_gather of a poll. Ring entries point into
 * it; the last recvfrom of its datagrams returns it to the pool (the mbuf pool's role). */
struct h_arena {
    uint8_t  *payload;           /* cap_bytes: the datagrams' packed slots (16-byte aligned)     */
    uint32_t *len;               /* [cap_n] payload bytes                                        */
    uint32_t *src_ip;            /* [cap_n] raw                                                  */
    uint16_t *src_port;          /* [cap_n] raw                                                  */
    uint64_t  cap_bytes;
    uint32_t  cap_n;
    atomic_uint refs;            /* queued datagrams still pointing into this slab               */
    struct h_arena *next;        /* free list                                                    */
};

struct h_dgram {                 /* one queued datagram (the mbuf a ring entry would point to)   */
    const uint8_t *data;
    uint32_t len;                /* payload bytes after Ethernet-padding trim                    */
    uint32_t src_ip;             /* raw */
    uint32_t src_port;           /* raw */
    struct h_arena *arena;
};

struct h_ring {                  /* SP/SC ring of EXCH_RING_SIZE entries (udpdk_init.c:268-277)  */
    struct h_dgram *e;
    _Atomic uint32_t head;       /* consumer (recvfrom) */
    _Atomic uint32_t tail;       /* producer (the poller); tail - head = entries */
    /* consumer only: entries of one slab consumed and not yet released to it (one atomic release
     * per run of a slab's entries instead of one per recvfrom) */
    struct h_arena *rel_arena;
    uint32_t rel_n;
    /* close vs a recvfrom blocked on another thread: recvfrom counts itself in busy for its whole
     * call and leaves with EBADF once closing is set; close sets closing and waits for busy to
     * reach 0 before it clears the ring (both seq_cst, so one of the two sees the other). busy
     * is a count, so close also waits for every one of several callers; the ring itself stays
     * single-consumer like the reference's SP/SC rx_q (udpdk_init.c:270-272): one reading thread
     * per socket at a time. */
    atomic_int busy;
    atomic_int closing;
};

struct h_txd {                   /* one sendto waiting for the poller's TX half                  */
    uint64_t pay;                /* offset of its payload in g_udpdk.txp                         */
    uint32_t len;
    uint32_t dst_ip;             /* raw */
    uint32_t dst_port;           /* raw */
    uint32_t gso;                /* segment size the drain cuts it at (UDP_SEGMENT), 0: one datagram */
};

struct h_txq {                   /* per-socket TX ring (exch_slots[s].tx_q, EXCH_RING_SIZE)      */
    struct h_txd *e;
    uint32_t head, tail;         /* under tx_lock */
};

struct h_slot {                  /* exch_slot_info (udpdk_types.h:40-47) + bind list links        */
    int      used;
    int      bound;
    uint32_t udp_port;           /* raw */
    uint32_t ip;                 /* raw */
    int      so_options;
    /* binding (at most one per socket): node of its port's list */
    int32_t  prev, next;
    uint8_t  reuse_addr, reuse_port;
    uint8_t  rp_member;          /* bound with every bit of SO_REUSEPORT set (h_slot_balanced)      */
    uint8_t  connected;          /* udpdk_connect: the socket has a peer (always bound then)        */
    uint16_t peer_port;          /* raw */
    uint32_t peer_ip;            /* raw */
    atomic_int so_error;         /* pending ICMP error (udpdk_sock_error_post): an errno, 0 = none     */
    uint16_t gso_size;           /* UDP_SEGMENT socket option: segment size of later sends, 0 = off   */
    uint8_t  n_mc;               /* groups joined (IP_ADD_MEMBERSHIP), raw addresses, in no order       */
    uint32_t mc_group[H_MCAST_MAX];
    struct h_ring rx;
    struct h_txq  tx;
};

/* Whether a balancing poll treats the socket as a member of its port's reuse-port group: bound with
 * every bit of SO_REUSEPORT set. (The reference's option values overlap, SO_REUSEADDR = 2 inside
 * SO_REUSEPORT = 15, and its bind path tests `opts & SO_REUSEPORT`, so reuse_port is also set for a
 * socket that only asked for SO_REUSEADDR: such a socket keeps its clone of every datagram.) Like
 * reuse_port, fixed by the options in force at bind. */
static inline uint8_t h_slot_balanced(const struct h_slot *sl)
{
    return sl->used && sl->bound && sl->rp_member;
}

/* Device buffers of one context's payload gather (the gather list + the kernel's outputs). */
struct h_gbuf {
    void     *acc, *pay, *len, *sip, *spt;
    uint64_t  acc_cap, pay_cap, len_cap, sip_cap, spt_cap;
};

#define H_MAX_DEVS 16            /* [gpu] devices: RX shard contexts */

/* One RX shard of a multi-device poll ([gpu] devices = 0-7): a contiguous range of the poll's
 * frames processed by its own GPU context (one pool thread drives each). */
struct h_shard {
    udpdk_gpu_ctx *g;
    int       device;
    uint32_t  i0, n;             /* frames [i0, i0 + n) of the poll (contiguous dispatch)        */
    /* RSS dispatch ([gpu] dispatch = rss): the poll indices of the shard's frames (arrival
     * order) and their bytes packed back to back, with their lengths and ptypes */
    uint32_t *idx;  uint64_t idx_cap;
    uint8_t  *pack; uint64_t pack_cap;
    uint16_t *plen; uint64_t plen_cap;
    uint32_t *ppt;  uint64_t ppt_cap;
    uint64_t  lo, bytes;         /* the frame bytes they span (lo 16-byte aligned)              */
    uint32_t *off;  uint64_t off_cap;                 /* offsets rebased to lo                  */
    uint32_t *meta, *loff, *lpkt;
    uint64_t  meta_cap, loff_cap, lpkt_cap;
    udpdk_rx_stats_t st;
    int       err;               /* errno of a failed step, 0 = fine                             */
    /* payload gather of the accepted entries that are this shard's frames */
    uint32_t  nacc;
    uint64_t  acc_bytes;
    uint32_t *acc, *acco;  uint64_t acc_cap, acco_cap;  /* local frame index, packed slot offset */
    struct h_gbuf gb;
    struct h_arena *arena;
};

struct h_state {
    struct h_slot slots[UDPDK_MAX_SOCKETS];
    int32_t  port_head[65536], port_tail[65536];
    uint16_t port_len[65536];
    uint64_t n_active;
    uint64_t version;
    atomic_int interrupted;
    pthread_mutex_t lock;        /* bind table + socket slots + the poller's use of them        */
    pthread_mutex_t tx_lock;     /* TX rings + payload store                                    */
    pthread_mutex_t arena_lock;  /* arena free list                                             */
    uint8_t  src_mac[6], dst_mac[6];
    uint32_t src_ip;
    uint32_t mtu;                /* IPV4_MTU_DEFAULT = RTE_ETHER_MTU (udpdk_constants.h:37)      */
    uint32_t tx_udp_cksum;       /* [gpu] tx_udp_cksum / udpdk_config_tx_cksum: udpdk_tx_drain builds
                                    with UDPDK_TX_UDP_CKSUM (0: checksum 0, udpdk_syscall.c:343) */
    uint32_t rx_drop;            /* [gpu] rx_drop / udpdk_config_rx_drop: UDPDK_RX_DROP_* flags the next
                                    poll sets on every context (udpdk_gpu_rx_drop)                 */
    uint32_t rx_drop_applied;    /* ... and what the contexts hold (fresh contexts: 0)           */
    uint64_t rx_dropped;         /* deliveries removed that way (udpdk_rx_dropped)                */
    uint32_t reuseport;          /* [gpu] reuseport / udpdk_config_reuseport: UDPDK_REUSEPORT_*     */
    uint32_t reuseport_applied;  /* ... what the contexts hold (fresh contexts: fanout), and the    */
    uint64_t reuseport_version;  /* snapshot version their lane flags were built from             */
    uint64_t rx_balanced;        /* reuse-port clones removed (udpdk_rx_balanced)                  */
    uint32_t n_connected;        /* sockets with a peer (udpdk_connect)                             */
    uint32_t peer_applied;       /* the contexts hold a peer table (fresh contexts: none), built    */
    uint64_t peer_version;       /* ... moves with every change of a socket's peer                  */
    uint64_t peer_version_applied, peer_snap_version;   /* from these versions of peers and snapshot */
    uint64_t rx_refused;         /* deliveries the peer filter removed (udpdk_rx_refused)           */
    udpdk_gpu_ctx *gpu;
    int      gpu_device;
    uint32_t gpu_max_frames, gpu_max_lanes;
    /* bind snapshot as uploaded to the GPU: rebuilt only when the table's version moves */
    uint64_t snap_version;       /* version uploaded (UINT64_MAX = none)                        */
    int      snap_compat;
    uint32_t snap_lanes, snap_maxfan;
    /* fragments (udpdk_poller.c:338-361): the device reassembly table, created on the first
     * FRAG frame; geometry from the [gpu] frag_* ini keys (defaults: the poller's table) */
    int      frag_ready;
    uint32_t frag_buckets, frag_entries, frag_max_dgram;
    uint32_t frag_max_entries, frag_flags;    /* 0: NUM_FLOWS_MAX; [gpu] reasm_cksum = dpdk */
    uint64_t frag_ttl_ms;
    uint32_t poll_threads;       /* [gpu] poll_threads: threads of udpdk_poll_rx's socket loops  */
    uint32_t host_copy_min;      /* [gpu] host_copy_min: mean payload bytes from which a poll copies
                                  * its payloads on the host instead of gathering them on the GPU
                                  * (0: always the GPU gather)                                     */
    /* RX work buffers (poller thread only), grow-only */
    uint32_t *rx_meta, *rx_loff, *rx_lpkt;
    uint64_t  rx_meta_cap, rx_loff_cap, rx_lpkt_cap;
    uint32_t *fr_loff, *fr_lpkt, *fr_org;        /* reassembled datagrams: lanes, origins     */
    uint16_t *fr_len;
    uint64_t  fr_loff_cap, fr_lpkt_cap, fr_org_cap, fr_len_cap;
    uint32_t *acc_d, *acc_f;                     /* accepted entries: frame / datagram index   */
    uint32_t *acc_do, *acc_fo;                   /* their packed slot offsets (+ the total)    */
    uint32_t *acc_sock;                          /* per accepted entry: socket | from-frag<<31 */
    uint64_t  acc_d_cap, acc_f_cap, acc_do_cap, acc_fo_cap, acc_sock_cap;
    struct h_gbuf gb;                            /* device: gather list + outputs (context 0)  */
    /* udpdk_poll_rx's pipelined form (h_poll_chunked): pinned verdict words, per-chunk lanes and
     * the gather lists of the chunk in flight; [gpu] poll_chunk_mb = chunk size (0: one piece) */
    uint32_t *pc_meta, *pc_loff, *pc_lpkt, *pc_acc;
    uint64_t  pc_meta_cap, pc_loff_cap, pc_lpkt_cap, pc_acc_cap;
    uint32_t  poll_chunk_mb;
    uint32_t  poll_chunk_min_avg;                /* ... for batches of at least this mean frame size */
    /* multi-device RX ([gpu] devices): n_shards > 1 splits every poll into contiguous shards over
     * the shard contexts; the context above (g_udpdk.gpu) keeps TX and the reassembly table */
    uint32_t  n_shards;
    int       shard_dev[H_MAX_DEVS];
    /* [gpu] dispatch = rss: frames go to shard reta[Toeplitz hash] (the NIC's RSS queue, one
     * queue per device, udpdk_gpu_rss's hash and default key/RETA) instead of contiguous ranges;
     * lanes are merged back in arrival order */
    int       dispatch_rss;
    uint32_t  rss_tab[12][256];
    uint16_t  rss_reta[UDPDK_RSS_RETA_MAX];
    uint32_t  rss_reta_size, rss_types, rss_ready;
    uint8_t  *rss_sh;  uint64_t rss_sh_cap;      /* per poll frame: its shard                   */
    uint32_t *rss_loc; uint64_t rss_loc_cap;     /* ... and its index in that shard             */
    struct h_shard shard[H_MAX_DEVS];
    uint8_t  *acc_dk;                            /* per accepted direct entry: its shard        */
    uint32_t *acc_di;                            /* ... and its index in that shard's slab      */
    uint64_t  acc_dk_cap, acc_di_cap;
    uint8_t  *fb_frames;                         /* FRAG frames of a sharded poll, host copy    */
    uint32_t *fb_off, *fb_idx, *fb_meta, *fb_loff, *fb_lpkt, *fb_pt;
    uint16_t *fb_len;
    uint64_t  fb_frames_cap, fb_off_cap, fb_idx_cap, fb_meta_cap, fb_loff_cap, fb_lpkt_cap, fb_pt_cap,
              fb_len_cap;
    void     *dv_meta2, *dv_loff2, *dv_lpkt2;              /* device: RX of reassembled batch */
    uint64_t  dv_meta2_cap, dv_loff2_cap, dv_lpkt2_cap;
    struct h_arena *arena_free;
    /* pinned slab budget (the mbuf pool's fixed size, udpdk_init.c:78-79): bytes and slabs held
     * by live + free slabs, capped by [gpu] slab_bytes_max / slab_count_max; a poll whose payloads
     * find no slab within the budget drops its bursts (rx_nobufs), as rte_eth_rx_burst does when
     * the mempool is exhausted */
    uint64_t  arena_bytes, arena_bytes_max, rx_nobufs;
    uint32_t  arena_count, arena_count_max, arena_free_n;
    /* TX: per-socket rings of struct h_txd + the payload store they point into */
    uint8_t  *txp;
    uint64_t  txp_bytes, txp_cap;
    uint64_t  tx_queued;                         /* datagrams in all TX rings                   */
    uint64_t  tx_dropped;                        /* too large for the drain's limits (tx_drain)  */
    /* TX work buffers (tx_drain), grow-only: host pinned staging + device */
    void     *tx_h, *tx_d, *tx_fr_d;
    uint64_t  tx_h_cap, tx_d_cap, tx_fr_d_cap;
    struct h_txsel { int32_t s; uint32_t nf; uint64_t foff; } *tx_sel;   /* nf, foff: of the whole send */
    uint64_t  tx_sel_cap;
    udpdk_gso_counts_t gso_counts;               /* segmented sends (udpdk_gso_counts), under tx_lock */
    /* udpdk_poll_echo work buffers (rx_echo.c), grow-only: pinned staging of the batch, its device
     * copy, the device lanes + reply plan, the built replies, the pinned readback of the plan */
    void     *ec_h, *ec_in_d, *ec_ws_d, *ec_out_d, *ec_rb_h;
    uint64_t  ec_h_cap, ec_in_d_cap, ec_ws_d_cap, ec_out_d_cap, ec_rb_h_cap;
    /* ICMP answers (rx_icmp.c): [gpu] icmp / udpdk_config_icmp flags (0: a poll enqueues what it always
     * did), [gpu] icmp_burst (errors answered per poll, -1: no limit), the queue udpdk_tx_drain empties
     * first and the session's counts (both under tx_lock); work buffers, grow-only: the device
     * output, reply_off + origin, the pinned readback */
    uint32_t  icmp_flags;
    int32_t   icmp_burst;
    struct h_icmpq icmpq;
    udpdk_icmp_counts_t icmp_counts;
    void     *ic_out_d, *ic_idx_d, *ic_h;
    uint64_t  ic_out_d_cap, ic_idx_d_cap, ic_h_cap;
    /* ARP (rx_arp.c): [gpu] arp / udpdk_config_arp (0: a poll enqueues what it always did), the
     * session's counts (under tx_lock; the replies and the announcement share the ICMP queue); work
     * buffers of a fixed size: the device slots + origin, the pinned readback */
    uint32_t  arp_on, arp_announce;
    udpdk_arp_counts_t arp_counts;
    void     *ar_out_d, *ar_h;
    uint64_t  ar_out_d_cap, ar_h_cap;
    /* Neighbours (neigh.c): [gpu] neigh / udpdk_config_neigh (UDPDK_NEIGH_MODE_*; off: a poll and a drain
     * enqueue what they always did), the table's size and timers, [port0] netmask / gateway (raw; 0: all
     * on-link / none), whether the main context has its table yet, the session's counts (under tx_lock);
     * udpdk_tx_drain's work buffers, grow-only: the device MACs + sockets + states + requests + origins
     * and the pinned readback */
    uint32_t  neigh_mode, neigh_entries, neigh_ttl_ms, neigh_retrans_ms;
    uint32_t  netmask, gateway;
    int       neigh_ready;
    udpdk_neigh_counts_t neigh_counts;
    void     *ng_d, *ng_h;
    uint64_t  ng_d_cap, ng_h_cap;
    /* ICMP errors received (rx_icmp_err.c): [gpu] icmp_errors / udpdk_config_icmp_errors (0: a poll
     * enqueues what it always did), the session's counts (under lock) and the peer records the
     * contexts hold (h_peer_apply: what an error is posted against); work buffers, grow-only, one
     * word per lane: the device output and its pinned readback */
    uint32_t  icmp_errors;
    udpdk_icmp_err_counts_t icmp_err_counts;
    udpdk_peer_t peer_up[UDPDK_MAX_SOCKETS];
    void     *ie_d, *ie_h;
    uint64_t  ie_d_cap, ie_h_cap;
    /* Multicast (mcast.c): [gpu] mcast / udpdk_config_mcast (0: a poll and a drain enqueue what they
     * always did; memberships are recorded either way), whether the main context holds the membership
     * filter and from which versions of the memberships and the snapshot it was built, the session's
     * counts (mcast_counts under tx_lock; the reports and leaves share the ICMP queue); work buffers: the
     * host lists a poll uploads (members, then the distinct groups, then the lanes' flags), the device
     * copy of the distinct groups, the IGMP stage's device slots + group indices and their pinned
     * readback */
    uint32_t  mcast_on, mcast_applied;
    uint64_t  mcast_version, mcast_version_applied, mcast_snap_version;
    uint64_t  rx_not_member;     /* deliveries the membership filter removed (udpdk_rx_not_member)   */
    udpdk_mcast_counts_t mcast_counts;
    uint32_t  mc_n_groups;
    void     *mc_members, *mc_groups_d, *mc_out_d, *mc_h;
    uint64_t  mc_members_cap, mc_groups_d_cap, mc_out_d_cap, mc_h_cap;
    /* poller thread (udpdk_port_attach) */
    pthread_t poller;
    atomic_int poller_run;
    int       poller_started;
    udpdk_port_ops_t port;
    /* [gpu] port / port_peer: the port udpdk_init attaches the poller thread to (port_udp.c) */
    char      port_spec[128], port_peer[128];
};

extern struct h_state g_udpdk;

/* port_table.c */
void h_btable_reset(void);
int  h_btable_add(int sockfd, uint32_t ip, uint32_t port, int opts);
void h_btable_del(int sockfd, uint32_t port);
int  h_btable_free_port(void);

/* tx_drain.c: grow-only pinned host buffer (g_udpdk.gpu's allocator) */
int  h_grow_pinned(void **p, uint64_t *cap, uint64_t need);

/* sock_api.c */
void h_sockets_reset(void);
uint32_t h_ring_free(const struct h_ring *r);
int  h_ring_push_bulk(struct h_ring *r, const struct h_dgram *d, uint32_t n);
struct h_arena *h_arena_get(uint32_t n, uint64_t bytes);
void h_arena_put(struct h_arena *a);
void h_arena_release(struct h_arena *a, uint32_t refs);
void h_arenas_free_all(void);
void h_tx_reset(void);

/* h_pool.c: fork-join workers; h_pool_run calls fn(ctx, part, parts) for every part < parts
 * (part 0 on the caller) and returns when all have returned */
typedef void (*h_job_fn)(void *ctx, uint32_t part, uint32_t parts);
uint32_t h_pool_parts(void);
void h_pool_run(h_job_fn fn, void *ctx);
void h_pool_stop(void);

/* rx_poll.c */
int  h_snapshot_refresh(void);            /* under g_udpdk.lock */
void h_rx_buffers_free(void);
void h_shards_destroy(void);
void udpdk_poll_profile_dump(void);   /* -DUDPDK_POLL_PROFILE builds: phase times to stderr */
int  h_grow_dev(void **p, uint64_t *cap, uint64_t need);
int  h_grow_dev_on(udpdk_gpu_ctx *g, void **p, uint64_t *cap, uint64_t need);
int  h_rss_setup(void);
int  h_rx_drop_apply(void);               /* under g_udpdk.lock */
int  h_reuseport_apply(void);             /* under g_udpdk.lock, after h_snapshot_refresh */
int  h_peer_apply(void);                  /* under g_udpdk.lock, after h_snapshot_refresh */
void h_rx_drop_count(udpdk_gpu_ctx *g, const udpdk_rx_stats_t *st);
int  h_grow_host(void **p, uint64_t *cap, uint64_t need);

/* port_udp.c: the UDP test wire */
int  h_wire_open(const char *local, const char *peer, udpdk_port_ops_t *ops);
void h_wire_close(void);

/* tx_drain.c */
void h_tx_buffers_free(void);

/* rx_echo.c */
void h_echo_buffers_free(void);

/* rx_icmp.c */
#define H_ICMP_BURST_DEFAULT 64   /* a policy default in the spirit of Linux's icmp_msgs_burst, not measured */
void h_icmp_reset(void);                  /* under tx_lock */
void h_icmp_buffers_free(void);
uint32_t h_icmp_budget(void);
int  h_icmp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev,
                  uint32_t *budget);


/* rx_arp.c */
void h_arp_reset(void);                   /* under tx_lock */
void h_arp_buffers_free(void);
int  h_arp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_ipv4);

/* mcast.c */
void h_mcast_reset(void);                 /* under tx_lock */
void h_mcast_buffers_free(void);
int  h_mcast_sockopt(int s, int optname, const void *optval, socklen_t optlen);
void h_mcast_close_locked(int s);         /* under g_udpdk.lock */
int  h_mcast_apply(void);                 /* under g_udpdk.lock, after h_snapshot_refresh */
int  h_igmp_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_udp);

/* neigh.c */
#define H_NEIGH_ENTRIES_DEFAULT 1024u
#define H_NEIGH_TTL_MS_DEFAULT 30000u
#define H_NEIGH_RETRANS_MS_DEFAULT 1000u
#define H_NEIGH_REQ_CAP 256u              /* who-has frames one drain can queue (the rest: no_room) */
#define H_NEIGH_REQ_FIRST 32u             /* ... copied back behind the stage, before the counts are known */
void h_neigh_reset(void);                 /* under tx_lock */
void h_neigh_buffers_free(void);
uint32_t h_neigh_now(void);
void h_neigh_cfg(udpdk_neigh_cfg_t *cfg);
int  h_neigh_table(void);
int  h_neigh_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev, uint64_t not_ipv4);
void h_neigh_count_resolve(const udpdk_neigh_resolve_stats_t *st);   /* under tx_lock */

/* rx_icmp_err.c */
void h_icmp_err_reset(void);              /* under g_udpdk.lock */
void h_icmp_err_buffers_free(void);
int  h_sock_error_post_locked(int s, uint32_t peer_ip, uint16_t peer_port, uint32_t code);
int  h_sock_error_take(int s);            /* the pending error, cleared (0: none) */
int  h_icmp_err_stage(udpdk_gpu_ctx *g, int pipe, const udpdk_rx_batch_t *b, const uint32_t *meta_dev);

#endif
