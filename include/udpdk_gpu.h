/*
 * udpdk_gpu.h — C ABI of the MI355X (gfx950) batch datapath.
 *
 * This is the drop-in boundary for UDPDK's per-packet hot path. The reference has no plugin
 * registry (udpdk/Makefile:72-81 localises every non-API symbol), so the replacement points are
 * the two function bodies the hot path lives in:
 *
 *   RX  udpdk_poller.c:516-545 (burst loop) + :316-413 reassemble() + :274-298 enqueue/flush
 *       -> udpdk_gpu_rx(): one launch sequence over N frames instead of N reassemble() calls,
 *          producing a verdict word per frame and stable per-socket output lanes (the
 *          equivalent of exch_slots[s].rx_buffer flushed into exch_slots[s].rx_q).
 *   TX  udpdk_syscall.c:314-356 (udpdk_sendto header build + rte_ipv4_cksum)
 *       -> udpdk_gpu_tx_build(): header build + IPv4 checksum + payload copy for N datagrams.
 *
 * The bind table walked by reassemble() (udpdk_bind_table.c:152 btable_get_bindings + the list
 * iterator, list_iterator.c:19-55) is replaced by an immutable flattened snapshot uploaded with
 * udpdk_gpu_bind_snapshot_upload(); the host bind table (see udpdk_api.h) builds it in list order.
 *
 * Conventions
 *   - Plain C types only; no HIP/torch types cross the boundary. Streams are opaque (void*).
 *   - Every entry point returns 0 on success or a negative errno (-EINVAL bad arguments,
 *     -ENOMEM allocation failure, -ENOSPC output capacity exceeded, -EIO HIP failure; the HIP
 *     error code of the last failure is kept in the context, see udpdk_gpu_last_hip_error()).
 *     Nothing aborts. (Reference convention: API calls return -1 + errno, udpdk_syscall.c:23-520;
 *     the datapath itself never reports errors, it logs and drops.)
 *   - Ports and IPv4 addresses are "raw": the 2/4 wire bytes read as a little-endian host
 *     integer, exactly how the reference compares and indexes them (udpdk_poller.c:372-373,
 *     udpdk_bind_table.c:152, udpdk_syscall.c:230).
 *   - Buffers named *_dev are device pointers (from udpdk_gpu_alloc or any hipMalloc on the
 *     context's device); buffers named *_host are host pointers.
 *   - Calls on one context are asynchronous on that context's stream unless stated otherwise.
 *     One host thread per context; contexts on different devices are independent.
 */
#ifndef UDPDK_GPU_H
#define UDPDK_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: udpdk_reasm_out_t stats grew to UDPDK_RS_N = 11 (RS_SERIAL, RS_SORTED);
 *    udpdk_gpu_rx_gather_packed; TX payloads need UDPDK_GPU_FRAMES_TAILROOM readable bytes
 * 3: udpdk_frag_table_cfg_t grew max_entries (the table's LRU limit) and flags (32 bytes)
 *    (still 3: udpdk_gpu_tx_build_flags / UDPDK_TX_UDP_CKSUM, then udpdk_gpu_rx_filter /
 *    udpdk_gpu_rx_drop / udpdk_gpu_rx_drop_stats were added; a new symbol breaks no caller)
 *    (still 3: udpdk_gpu_tx_reply_plan / udpdk_gpu_tx_reply / udpdk_gpu_tx_reply_stats /
 *    udpdk_gpu_tx_reply_geometry were added)
 *    (still 3: udpdk_gpu_rx_balance_select / udpdk_gpu_rx_balance / udpdk_gpu_rx_balance_stats /
 *    udpdk_gpu_rx_balance_rank / udpdk_gpu_rx_removed were added)
 *    (still 3: udpdk_gpu_rx_peer_select / udpdk_gpu_rx_peer / udpdk_gpu_rx_peer_stats /
 *    udpdk_gpu_rx_peer_removed were added)
 *    (still 3: udpdk_gpu_icmp_reply / udpdk_gpu_icmp_stats / udpdk_gpu_icmp_geometry /
 *    udpdk_gpu_pipe_icmp_reply / udpdk_gpu_pipe_icmp_stats were added)
 *    (still 3: udpdk_gpu_icmp_errors / udpdk_gpu_icmp_err_stats / udpdk_gpu_pipe_icmp_errors /
 *    udpdk_gpu_pipe_icmp_err_stats / udpdk_gpu_icmp_errno were added)
 *    (still 3: udpdk_gpu_arp_reply / udpdk_gpu_arp_stats / udpdk_gpu_arp_geometry /
 *    udpdk_gpu_pipe_arp_reply / udpdk_gpu_pipe_arp_stats were added)
 *    (still 3: udpdk_gpu_neigh_create / _set / _dump / _flush / _learn / _learn_stats / _resolve /
 *    _resolve_stats / _geometry / _class, udpdk_gpu_pipe_neigh_learn / _learn_stats and
 *    udpdk_gpu_tx_build_neigh were added)
 *    (still 3: udpdk_gpu_rx_mcast_select / udpdk_gpu_rx_mcast / udpdk_gpu_rx_mcast_stats /
 *    udpdk_gpu_rx_mcast_removed / udpdk_gpu_mcast_table_build, udpdk_gpu_igmp_reply / _stats /
 *    _geometry and udpdk_gpu_pipe_igmp_reply / _stats were added)
 *    (still 3: udpdk_gpu_tx_segment_plan / udpdk_gpu_tx_segment / udpdk_gpu_tx_segment_stats /
 *    udpdk_gpu_tx_segment_span / udpdk_gpu_tx_segment_geometry were added) */
#define UDPDK_GPU_ABI_VERSION 3

/* ---------------------------------------------------------------------------------------------
 * Per-frame verdict word (one uint32 per frame, written by udpdk_gpu_rx)
 *
 *   bits  0..3   verdict (enum udpdk_verdict)
 *   bit   4      IPv4 header checksum verifies (RFC 1071 over the fixed 20 B at frame offset 14)
 *   bits  5..6   UDP checksum state (enum udpdk_udp_csum)
 *   bit   7      UDP length bad: dgram_len < 8 or 34 + dgram_len > frame length
 *   bit   8      IHL != 5 (the reference parses at fixed offsets regardless, poller.c:336,:372)
 *   bits  9..15  number of deliveries (fan-out), saturating at 127
 *   bits 16..31  sockfd of the first delivery (the original mbuf's socket; clones follow it)
 * ------------------------------------------------------------------------------------------- */
enum udpdk_verdict {
    UDPDK_V_DELIVERED = 0, /* >= 1 socket matched (poller.c:391-403)                            */
    UDPDK_V_NOT_IPV4  = 1, /* !RTE_ETH_IS_IPV4_HDR(ptype) (poller.c:334, :362-366)               */
    UDPDK_V_FRAG      = 2, /* rte_ipv4_frag_pkt_is_fragmented (poller.c:338); host slow path      */
    UDPDK_V_NOT_UDP   = 3, /* next_proto_id != 17 (poller.c:368-371)                             */
    UDPDK_V_NO_BIND   = 4, /* empty bind list for the raw dst port (poller.c:376-380)            */
    UDPDK_V_NO_MATCH  = 5, /* bind list present, no IP matched (poller.c:406-411)                */
    UDPDK_V_TRUNC     = 6, /* IPv4 by ptype but shorter than the 42 B Eth/IPv4/UDP header, and
                              not a fragment of >= 34 B (those are FRAG: a fragment needs only
                              its IPv4 header); the reference would read past data_len        */
    UDPDK_V_BAD_DESC  = 7  /* offset + length beyond frames_bytes: nothing was read              */
};
#define UDPDK_N_VERDICTS 8

enum udpdk_udp_csum {
    UDPDK_UDP_CSUM_NONE = 0, /* dgram_cksum == 0 (RFC 768 "no checksum") or not a UDP verdict */
    UDPDK_UDP_CSUM_OK   = 1,
    UDPDK_UDP_CSUM_BAD  = 2
};

#define UDPDK_META_VERDICT(m)  ((unsigned)(m) & 0xFu)
#define UDPDK_META_IP_OK(m)    (((unsigned)(m) >> 4) & 1u)
#define UDPDK_META_UDP_CSUM(m) (((unsigned)(m) >> 5) & 3u)
#define UDPDK_META_LEN_BAD(m)  (((unsigned)(m) >> 7) & 1u)
#define UDPDK_META_IHL_NE5(m)  (((unsigned)(m) >> 8) & 1u)
#define UDPDK_META_FANOUT(m)   (((unsigned)(m) >> 9) & 0x7Fu)
#define UDPDK_META_SOCKFD(m)   ((unsigned)(m) >> 16)

/* Counters reduced over a whole udpdk_gpu_rx call (replace the per-drop RTE_LOG WARNINGs,
 * poller.c:363, :369, :378, :410). */
enum udpdk_rx_counter {
    UDPDK_C_VERDICT0   = 0,  /* 0..7: frames per verdict                                     */
    UDPDK_C_DELIVERIES = 8,  /* total (frame, socket) deliveries = lane entries               */
    UDPDK_C_IP_BAD     = 9,  /* IPv4-gated frames whose header checksum fails                 */
    UDPDK_C_UDP_OK     = 10,
    UDPDK_C_UDP_BAD    = 11,
    UDPDK_C_UDP_NONE   = 12, /* UDP-verdict frames carrying dgram_cksum == 0                  */
    UDPDK_C_LEN_BAD    = 13,
    UDPDK_C_IHL_NE5    = 14,
    UDPDK_C_BYTES      = 15, /* sum of frame lengths                                         */
    UDPDK_N_COUNTERS   = 16
};

/* Limits of the GPU path. NUM_SOCKETS_MAX is 1024 in the reference (udpdk_constants.h:12); the
 * lane count is widened here and bounded by the per-workgroup LDS histogram. */
#define UDPDK_GPU_MAX_LANES        16384u
#define UDPDK_GPU_MAX_BINDS        (1u << 20)
#define UDPDK_GPU_MAX_PORT_BINDS   4095u
#define UDPDK_UDP_PORTS            65536u     /* UDP_MAX_PORT, udpdk_constants.h:13 */
/* Readable bytes the RX kernels need after frames_bytes (byte-aligned dword loads of a batch's
 * last frame may end up to 3 bytes past it). */
#define UDPDK_GPU_FRAMES_TAILROOM  16u

/* ---------------------------------------------------------------------------------------------
 * Context
 * ------------------------------------------------------------------------------------------- */
typedef struct udpdk_gpu_ctx udpdk_gpu_ctx;

/* Create a context on `device` with its own stream and workspace sized for batches of up to
 * max_frames frames and up to max_lanes per-socket lanes. Called from udpdk_init(). */
int  udpdk_gpu_ctx_create(int device, uint32_t max_frames, uint32_t max_lanes,
                          udpdk_gpu_ctx **out);
/* Synchronise and free everything. Called from udpdk_cleanup(). NULL is a no-op. */
int  udpdk_gpu_ctx_destroy(udpdk_gpu_ctx *ctx);
int  udpdk_gpu_sync(udpdk_gpu_ctx *ctx);
int  udpdk_gpu_last_hip_error(const udpdk_gpu_ctx *ctx);
int  udpdk_gpu_device_count(int *count);
int  udpdk_gpu_abi_version(void);
/* The context's HIP stream (hipStream_t) as an opaque pointer. */
void *udpdk_gpu_stream(udpdk_gpu_ctx *ctx);

/* Device / pinned-host memory helpers on the context's device (so callers need no HIP). */
int  udpdk_gpu_alloc(udpdk_gpu_ctx *ctx, size_t bytes, void **dev);
int  udpdk_gpu_free(udpdk_gpu_ctx *ctx, void *dev);
int  udpdk_gpu_host_alloc(udpdk_gpu_ctx *ctx, size_t bytes, void **host); /* pinned */
int  udpdk_gpu_host_free(udpdk_gpu_ctx *ctx, void *host);
int  udpdk_gpu_memset(udpdk_gpu_ctx *ctx, void *dev, int value, size_t bytes);       /* async */
int  udpdk_gpu_h2d(udpdk_gpu_ctx *ctx, void *dev, const void *host, size_t bytes);   /* async */
int  udpdk_gpu_d2h(udpdk_gpu_ctx *ctx, void *host, const void *dev, size_t bytes);   /* async */

/* ---------------------------------------------------------------------------------------------
 * Bind snapshot (replaces sock_bind_table[65536] of list<bind_info>, udpdk_bind_table.c:17-18,
 * walked at poller.c:376-405). Bindings of one raw port are contiguous and in list order
 * (head -> tail: ANY bindings lpush'ed, specific ones rpush'ed, udpdk_bind_table.c:119-124).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t ip;      /* raw IPv4 (bind_info.ip_addr.s_addr, udpdk_types.h:33); 0 = INADDR_ANY */
    int32_t  sockfd;  /* bind_info.sockfd (udpdk_types.h:32), 0..65535                         */
    uint32_t reuse;   /* bind_info.reuse_addr || bind_info.reuse_port (poller.c:396)            */
} udpdk_binding_t;

/* Socket slot state needed by TX header build (exch_slot_info, udpdk_types.h:40-47). */
typedef struct {
    uint32_t ip;       /* raw bound IPv4, 0 = ANY                                              */
    uint32_t udp_port; /* raw bound UDP port (low 16 bits)                                     */
    uint32_t bound;    /* slot did bind (explicitly or by sendto auto-bind)                    */
} udpdk_slot_t;

typedef struct {
    const uint32_t        *port_first;  /* [65536] index of the port's first binding          */
    const uint16_t        *port_count;  /* [65536] bindings on the port (0 = none)            */
    const udpdk_binding_t *binds;       /* [n_binds]                                          */
    uint32_t               n_binds;
    uint32_t               n_lanes;     /* > max(sockfd & lane_mask) over all bindings        */
    uint32_t               lane_mask;   /* 0xFFFFFFFF: lanes keyed by full sockfd;
                                           0xFF: compat mode, the reference's (uint8_t) slot
                                           index (poller.c:294, :393)           */
    const udpdk_slot_t    *slots;       /* [n_slots] for TX, may be NULL                      */
    uint32_t               n_slots;
    uint64_t               version;     /* bumped by every bind/close on the host             */
} udpdk_bind_snapshot_t;

/* Upload (host arrays -> device, synchronous on the context stream). */
int udpdk_gpu_bind_snapshot_upload(udpdk_gpu_ctx *ctx, const udpdk_bind_snapshot_t *snap);

/* ---------------------------------------------------------------------------------------------
 * RX: parse + validate + checksum + port demux + per-socket lanes
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const uint8_t  *frames_dev;   /* frame bytes (rte_pktmbuf_mtod, Ethernet first, no FCS),
                                     16-byte aligned base, readable for frames_bytes +
                                     UDPDK_GPU_FRAMES_TAILROOM bytes (tailroom, as every DPDK
                                     mbuf data room has); bytes past frames_bytes never
                                     affect a result                                          */
    uint64_t        frames_bytes; /* < 2^32                                                    */
    const uint32_t *offset_dev;   /* [n] byte offset of each frame in frames_dev               */
    const uint16_t *length_dev;   /* [n] data_len of each frame                                */
    const uint32_t *ptype_dev;    /* [n] mbuf packet_type, or NULL: derived from ether_type
                                     (0x0800 -> L2_ETHER|L3_IPV4|L4_UDP, else L2_ETHER)        */
    uint32_t        n;
} udpdk_rx_batch_t;

typedef struct {
    uint32_t *meta_dev;      /* [n] verdict words                                             */
    uint32_t *lane_off_dev;  /* [n_lanes + 1] exclusive prefix of per-lane delivery counts    */
    uint32_t *lane_pkt_dev;  /* [lane_cap] frame indices grouped by lane, arrival order kept  */
    uint32_t  lane_cap;
} udpdk_rx_out_t;

typedef struct {
    uint64_t counters[UDPDK_N_COUNTERS];
    uint32_t deliveries;     /* == lane_off[n_lanes]                                           */
    uint32_t overflow;       /* deliveries > lane_cap: lane_pkt holds only the first lane_cap  */
} udpdk_rx_stats_t;

/* Enqueue the RX pipeline for one batch on the context stream (async): rx_classify, then, with
 * one lane and no fan-out in the snapshot, nothing more (the last classify workgroup completes
 * the lane) or rx_compact1, else rx_scan + rx_scatter. meta, lane_off and lane_pkt are complete
 * when the stream reaches the end of the sequence. Which single-lane form runs (and how many
 * tail chunk groups classify keeps in flight) follows hints the kernels leave in pinned host
 * memory about the context's recent calls; every form gives the same results for any batch.
 * A fresh context starts on the two-launch form.
 *
 * Tailroom contract: batch->frames_dev must be readable for frames_bytes +
 * UDPDK_GPU_FRAMES_TAILROOM bytes. The kernels read frame bytes with byte-aligned dword loads
 * that are range-checked against frames_bytes rounded up to a dword, so the last frame of a batch
 * whose frames_bytes % 4 != 0 may be read up to 3 bytes past frames_bytes (never used in a
 * result). The library cannot check the allocation size behind a device pointer: a buffer that
 * ends exactly at frames_bytes may fault (tests/test_gpu_rx.py::test_tailroom_exact_allocation). */
int udpdk_gpu_rx(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch, const udpdk_rx_out_t *out);
/* Pipelining: with depth d in 2..4, consecutive udpdk_gpu_rx calls rotate over d internal
 * streams with their own workspaces, so one batch's launch, prologue and compaction overlap the
 * other batches' streaming (3 is fastest for 1 M x 64 B batches). Calls must then not share
 * output buffers with the d - 1 previous calls still in flight. Depth 1 (default): every call in
 * order on the context stream. Synchronises. */
int udpdk_gpu_pipeline_depth(udpdk_gpu_ctx *ctx, int depth);
/* Make the context stream (udpdk_gpu_stream) wait, on the device, for all work enqueued so far on
 * the other pipes (no host wait). memset/h2d/d2h/tx_build/rx_host join implicitly. */
int udpdk_gpu_join(udpdk_gpu_ctx *ctx);
/* Counters of the last udpdk_gpu_rx (reduced from its per-tile counter rows by one small kernel
 * launched here, so batches nobody asks statistics for pay nothing), then wait for the stream.
 * Returns -ENOSPC on lane overflow. */
int udpdk_gpu_rx_stats(udpdk_gpu_ctx *ctx, udpdk_rx_stats_t *stats);

/* End-to-end variant for host-resident batches (the real poller's situation: frames arrive in
 * host mbufs): pinned staging, H2D, the RX pipeline, D2H of meta and lanes (lane_pkt: only the
 * min(deliveries, lane_cap) entries made). Synchronous. frames_host etc. follow
 * udpdk_rx_batch_t; outputs are host arrays. */
int udpdk_gpu_rx_host(udpdk_gpu_ctx *ctx,
                      const uint8_t *frames_host, uint64_t frames_bytes,
                      const uint32_t *offset_host, const uint16_t *length_host,
                      const uint32_t *ptype_host, uint32_t n,
                      uint32_t *meta_host, uint32_t *lane_off_host,
                      uint32_t *lane_pkt_host, uint32_t lane_cap,
                      udpdk_rx_stats_t *stats);

/* Device view of the batch the last udpdk_gpu_rx_host call staged (frames, descriptors) and its
 * verdict words, valid until the next udpdk_gpu_rx_host[_async] call: for udpdk_gpu_rx_gather
 * and udpdk_gpu_rx_reassemble on frames already on the device (the socket layer's poller). */
int udpdk_gpu_rx_host_batch(udpdk_gpu_ctx *ctx, udpdk_rx_batch_t *batch, const uint32_t **meta_dev);

/* Asynchronous form of udpdk_gpu_rx_host for a stream of host-resident batches: the staging,
 * H2D, RX pipeline, counter reduction and D2H of meta, lane_off and lane_pkt[0, lane_cap) are
 * enqueued on the next pipe (udpdk_gpu_pipeline_depth) with its own staging buffers, and the
 * call returns; with depth 2 one batch's PCIe copies overlap the other's kernels and copies in
 * the opposite direction. At most `depth` calls are outstanding (a call first completes the one
 * that used its pipe). Host inputs must stay untouched, and outputs and *stats are valid, only
 * once udpdk_gpu_rx_host_wait returns (or a later call reuses the pipe). */
int udpdk_gpu_rx_host_async(udpdk_gpu_ctx *ctx,
                            const uint8_t *frames_host, uint64_t frames_bytes,
                            const uint32_t *offset_host, const uint16_t *length_host,
                            const uint32_t *ptype_host, uint32_t n,
                            uint32_t *meta_host, uint32_t *lane_off_host,
                            uint32_t *lane_pkt_host, uint32_t lane_cap,
                            udpdk_rx_stats_t *stats);
/* Complete every outstanding udpdk_gpu_rx_host_async call (oldest first). */
int udpdk_gpu_rx_host_wait(udpdk_gpu_ctx *ctx);

/* Poller internals, for udpdk_poll_rx's pipelined form (a large host batch cut into chunks at
 * burst boundaries, each chunk's RX, gather and payload copy on its own pipe): the same host RX
 * as udpdk_gpu_rx_host_async on an explicit pipe (1 .. 3), and the device view, gather and
 * copies of that chunk on that pipe's stream with no joins across pipes, so one chunk's payload
 * D2H overlaps the next chunk's frame H2D. udpdk_gpu_pipe_wait completes the pipe's stream and
 * the stats of its RX. offset_base: subtracted from every offset_host entry (a chunk of a larger
 * buffer whose frames_host points offset_base bytes into it). Not needed by an application;
 * reference: udpdk_poller.c:516-545 (the burst loop these chunks stand for). */
int udpdk_gpu_pipe_rx_host(udpdk_gpu_ctx *ctx, int pipe,
                           const uint8_t *frames_host, uint64_t frames_bytes,
                           const uint32_t *offset_host, uint32_t offset_base,
                           const uint16_t *length_host,
                           const uint32_t *ptype_host, uint32_t n,
                           uint32_t *meta_host, uint32_t *lane_off_host,
                           uint32_t *lane_pkt_host, uint32_t lane_cap,
                           udpdk_rx_stats_t *stats);
int udpdk_gpu_pipe_wait(udpdk_gpu_ctx *ctx, int pipe);
int udpdk_gpu_pipe_batch(udpdk_gpu_ctx *ctx, int pipe, udpdk_rx_batch_t *batch, const uint32_t **meta_dev);
int udpdk_gpu_pipe_h2d(udpdk_gpu_ctx *ctx, int pipe, void *dev, const void *host, size_t bytes);
int udpdk_gpu_pipe_d2h(udpdk_gpu_ctx *ctx, int pipe, void *host, const void *dev, size_t bytes);

/* ---------------------------------------------------------------------------------------------
 * RX drop filter: deliveries whose checksums or lengths fail are taken out of the lanes (RFC 1122
 * §4.1.3.4 has a UDP stack discard a datagram with a failed checksum; the reference delivers it).
 * rx_classify only flags such frames in their verdict word; this optional stage after the lanes
 * are complete removes every lane entry e = lane_pkt[p] whose meta[e] shows a selected reason.
 * Arrival order inside each lane is kept; the new lane_off[l] is the number of kept entries before
 * position lane_off[l]. Off by default: with no flags set udpdk_gpu_rx enqueues what it always did.
 *
 * An entry is removed when any selected reason applies. (A bad UDP length also makes the UDP
 * checksum state BAD: UDPDK_RX_DROP_UDP_LEN alone selects a subset of UDPDK_RX_DROP_UDP_CKSUM.)
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_RX_DROP_IP_CKSUM  1u   /* UDPDK_META_IP_OK(m) == 0                            */
#define UDPDK_RX_DROP_UDP_CKSUM 2u   /* UDPDK_META_UDP_CSUM(m) == UDPDK_UDP_CSUM_BAD        */
#define UDPDK_RX_DROP_UDP_LEN   4u   /* UDPDK_META_LEN_BAD(m)                               */
#define UDPDK_RX_DROP_IHL       8u   /* UDPDK_META_IHL_NE5(m)                               */
#define UDPDK_RX_DROP_ALL       15u

typedef struct {
    const uint32_t *meta_dev;      /* [n] */
    uint32_t        n;
    const uint32_t *lane_off_dev;  /* [n_lanes + 1] */
    const uint32_t *lane_pkt_dev;  /* entries [0, min(lane_off[n_lanes], lane_cap)) are read */
    uint32_t        lane_cap;
    uint32_t        n_lanes;       /* 1..UDPDK_GPU_MAX_LANES, need not be the snapshot's */
} udpdk_rx_lanes_t;

/* The filter as an explicit call on any lane set: out of place, async on the context stream; the
 * outputs (lane_off_out_dev[n_lanes + 1], lane_pkt_out_dev[out_cap]) must not alias the inputs.
 * flags == 0 is a valid identity copy (only entries >= n are removed); bits outside
 * UDPDK_RX_DROP_ALL give -EINVAL. meta is only read. Bounds, whatever the inputs hold: an offset
 * beyond min(lane_off[n_lanes], lane_cap) counts as that, an entry >= n is removed without a meta
 * read (bad_index), nothing past lane_cap is read and nothing past out_cap written; when more
 * than out_cap entries are kept only the first out_cap are written, lane_off_out is complete and
 * udpdk_gpu_rx_drop_stats returns -ENOSPC. */
int udpdk_gpu_rx_filter(udpdk_gpu_ctx *ctx, const udpdk_rx_lanes_t *in, uint32_t flags,
                        uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap);

/* Sticky mode: with nonzero flags every later udpdk_gpu_rx / udpdk_gpu_rx_host /
 * udpdk_gpu_rx_host_async / udpdk_gpu_pipe_rx_host call on this context filters its lanes, on the
 * call's own stream, before anything reads them (the caller's lane_off and lane_pkt hold the
 * filtered set; pipeline depths 2-4 work as before); with flags 0 (default) no filter stage is
 * enqueued at all. Returns the previous flags; a negative argument only queries; bits outside
 * UDPDK_RX_DROP_ALL give -EINVAL.
 *   - meta is never rewritten: it still says what classify found, fan-out and sockfd included.
 *   - udpdk_rx_stats_t: counters[] (UDPDK_C_DELIVERIES too) stay classify's; deliveries becomes
 *     the kept count, so it still equals lane_off[n_lanes]; overflow and -ENOSPC are still decided
 *     by the pre-filter total against lane_cap, and after an overflow the filtered lanes are those
 *     of the truncated input.
 *   - udpdk_gpu_rx_gather* and reassembly are unchanged: they consume the lanes they are given. */
int udpdk_gpu_rx_drop(udpdk_gpu_ctx *ctx, int flags);

typedef struct {
    uint64_t dropped[4];   /* entries per reason (ip, udp, len, ihl); an entry counts under every
                              selected reason that applies */
    uint32_t kept, removed;
    uint32_t bad_index;    /* entries >= n: removed, meta never read */
    uint32_t truncated;    /* input lane_off[n_lanes] > lane_cap: only the first lane_cap seen */
} udpdk_rx_drop_stats_t;
/* Of the last filter run on the context (explicit or sticky; -ENOENT when there was none).
 * Synchronises. -ENOSPC if kept > out_cap (sticky mode: the call's lane_cap, which cannot
 * happen). The filter launches are not event-timed (udpdk_gpu_timing_read). */
int udpdk_gpu_rx_drop_stats(udpdk_gpu_ctx *ctx, udpdk_rx_drop_stats_t *stats);

/* ---------------------------------------------------------------------------------------------
 * RX reuse-port balance: of a frame's deliveries to sockets that set SO_REUSEPORT one stays, chosen
 * by the frame's flow hash. The reference clones a datagram to every socket bound with
 * SO_REUSEADDR or SO_REUSEPORT and marks that as unfinished (udpdk_poller.c:387-389: "if dest
 * unicast and SO_REUSEPORT, should load balance; if dest broadcast and SO_REUSEADDR or
 * SO_REUSEPORT, should deliver to all"). This optional stage after the lanes are complete is that
 * rule. Off by default: then udpdk_gpu_rx enqueues what it always did.
 *
 * The uploaded snapshot must have lane_mask == 0xFFFFFFFF (a lane is a sockfd, as for
 * udpdk_gpu_tx_reply). lane_rp[l] != 0 says lane l's socket has SO_REUSEPORT; a sockfd >= n_lanes
 * counts as unflagged. D = min(lane_off[n_lanes], lane_cap).
 *   - For a DELIVERED frame i, its deliveries are those of the demux walk (the bindings of the raw
 *     dst port at frame byte 36 in list order, a match when ip == the raw dst address at byte 30
 *     or ip == 0, ended by the first match without reuse). G = the deliveries to flagged lanes in
 *     that order, g = |G| (counted by the walk itself: UDPDK_META_FANOUT saturates at 127 and only
 *     tells fan-out < 2, which needs no frame read).
 *   - g <= 1, or the destination is 255.255.255.255 or multicast (first address byte 224-239):
 *     every delivery stays. (Directed broadcast would need a netmask the stack does not have.)
 *   - Otherwise deliveries to unflagged lanes stay (SO_REUSEADDR-only sockets still fan out) and of
 *     G only member udpdk_gpu_rx_balance_rank(hash_i, g) = (uint64(hash_i) * g) >> 32 stays (the
 *     reciprocal_scale rule Linux's reuseport_select_sock uses).
 *   - hash_i = hash_dev[i] when the caller gives hashes (a NIC's mbuf.hash.rss, or an earlier
 *     udpdk_gpu_rss output), else what udpdk_gpu_rss writes for the frame under the context's RSS
 *     configuration (udpdk_gpu_rss_default_conf when udpdk_gpu_rss_config was never called): the
 *     4-tuple hash with UDPDK_RSS_NONFRAG_IPV4_UDP, else the 2-tuple hash with UDPDK_RSS_IPV4, else 0.
 *   - Entry p of lane l with frame i = lane_pkt[p] is removed iff i >= n (bad_index: no meta or
 *     frame byte of it is read) or lane_rp[l] != 0 and frame i chose a lane other than l.
 *   - The output is the drop filter's: a stable compaction, lane_off_out[l] = kept entries before
 *     min(lane_off[l], D), nothing past lane_cap read, nothing past out_cap written.
 * meta is never rewritten: fan-out and first sockfd stay classify's.
 * ------------------------------------------------------------------------------------------- */
/* The balance as an explicit call on any lane set (lanes->meta_dev required; lanes->n ==
 * batch->n): out of place, async on the context stream. lane_rp_dev is [n_lanes]; hash_dev is [n]
 * or NULL. An all-zero lane_rp is a valid identity copy (only entries >= n are removed). -EINVAL
 * with nothing enqueued: a NULL pointer (hash_dev excepted), n_lanes outside
 * 1..UDPDK_GPU_MAX_LANES, no snapshot uploaded or one with lane_mask != 0xFFFFFFFF, outputs that
 * overlap the input lanes. The frames buffer keeps the tailroom contract of udpdk_gpu_rx. */
int udpdk_gpu_rx_balance_select(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                                const udpdk_rx_lanes_t *lanes, const uint8_t *lane_rp_dev,
                                const uint32_t *hash_dev, uint32_t *lane_off_out_dev,
                                uint32_t *lane_pkt_out_dev, uint32_t out_cap);
/* Sticky mode: uploads lane_rp_host[n_lanes] (n_lanes <= the context's max_lanes; lanes past it
 * are unflagged); NULL or n_lanes == 0 turns the stage off (default: no stage is enqueued).
 * Synchronises the context. Afterwards every udpdk_gpu_rx / udpdk_gpu_rx_host /
 * udpdk_gpu_rx_host_async / udpdk_gpu_pipe_rx_host call on this context balances its lanes, on the
 * call's own stream, before anything reads them (pipeline depths 2-4 work as before), with the
 * hash computed by the stage. With udpdk_gpu_rx_drop flags set as well, the drop filter runs first;
 * the two commute. A call under a snapshot with lane_mask != 0xFFFFFFFF returns -EINVAL.
 *   - udpdk_rx_stats_t: counters[] (UDPDK_C_DELIVERIES too) stay classify's; deliveries becomes
 *     the kept count, so it still equals lane_off[n_lanes]; overflow and -ENOSPC are still decided
 *     by the pre-stage total against lane_cap: lane_cap must still hold the fan-out total. */
int udpdk_gpu_rx_balance(udpdk_gpu_ctx *ctx, const uint8_t *lane_rp_host, uint32_t n_lanes);

typedef struct {
    uint32_t kept, removed;
    uint32_t balanced;     /* frames for which a choice among >= 2 members was made */
    uint32_t bad_index;    /* entries >= n: removed, nothing of theirs read */
    uint32_t truncated;    /* input lane_off[n_lanes] > lane_cap: only the first lane_cap seen */
} udpdk_rx_balance_stats_t;
/* Of the last balance run on the context (explicit or sticky; -ENOENT when there was none).
 * Synchronises. -ENOSPC if kept > out_cap. The launches are not event-timed. */
int udpdk_gpu_rx_balance_stats(udpdk_gpu_ctx *ctx, udpdk_rx_balance_stats_t *stats);
/* (uint64(hash) * g) >> 32: the member of a group of g that a flow hash picks. Host only. */
uint32_t udpdk_gpu_rx_balance_rank(uint32_t hash, uint32_t g);
/* Poller internals: the lane entries each sticky stage removed in the call whose results were
 * last written to *stats (-ENOENT when no call's were). */
int udpdk_gpu_rx_removed(udpdk_gpu_ctx *ctx, const udpdk_rx_stats_t *stats, uint32_t *dropped,
                         uint32_t *balanced);

/* ---------------------------------------------------------------------------------------------
 * RX peer filter: the lane of a connected socket keeps only its peer's datagrams (udpdk_connect,
 * udpdk_api.h). The reference has no connect: its socket calls stop at sendto / recvfrom and every
 * application checks src_addr by hand. This optional stage after the lanes are complete applies
 * POSIX's rule for a connected UDP socket before anything reads the lanes (ring admission, payload
 * gather, replies). Off by default: then udpdk_gpu_rx enqueues what it always did.
 *
 * The uploaded snapshot must have lane_mask == 0xFFFFFFFF (a lane is a sockfd, as for
 * udpdk_gpu_tx_reply). peer[l] is lane l's record. D = min(lane_off[n_lanes], lane_cap). Entry p of
 * lane l with frame i = lane_pkt[p]:
 *   - i >= n: removed (bad_index); no descriptor or frame byte of it is read.
 *   - peer[l].on == 0: kept; no descriptor and no frame byte is read for the entry.
 *   - otherwise length[i] < 42 or offset[i] + length[i] > frames_bytes (summed in 64 bits): removed
 *     (bad_frame); no frame byte is read.
 *   - otherwise kept iff the raw u32 at frame bytes 26-29 == peer[l].ip and the raw u16 at frame
 *     bytes 34-35 == peer[l].port (what udpdk_gpu_rx_gather reports as src_ip / src_port); else
 *     removed (refused).
 *   - The rule is per entry: a frame that fans out to a connected and an unconnected lane stays in
 *     the second whatever its source is.
 *   - The output is the drop filter's: a stable compaction, lane_off_out[l] = kept entries before
 *     min(lane_off[l], D), nothing past lane_cap read, nothing past out_cap written.
 * meta is never read (lanes->meta_dev may be NULL, as for udpdk_gpu_tx_reply_plan) or rewritten.
 * ------------------------------------------------------------------------------------------- */
typedef struct { uint32_t ip; uint16_t port; uint16_t on; } udpdk_peer_t;   /* raw ip / port; 8 bytes */

/* The peer filter as an explicit call on any lane set (lanes->n == batch->n): out of place, async
 * on the context stream. peer_dev is [lanes->n_lanes], 8-byte aligned. An all-off peer table is a
 * valid identity copy (only entries >= n are removed). -EINVAL with nothing enqueued: a NULL
 * pointer, n_lanes outside 1..UDPDK_GPU_MAX_LANES, no snapshot uploaded or one with lane_mask !=
 * 0xFFFFFFFF (in compat mode a lane is not a sockfd), outputs that overlap the input lanes,
 * lanes->n != batch->n. The frames buffer keeps the tailroom contract of udpdk_gpu_rx. */
int udpdk_gpu_rx_peer_select(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                             const udpdk_rx_lanes_t *lanes, const udpdk_peer_t *peer_dev,
                             uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap);
/* Sticky mode: uploads peer_host[n_lanes] (n_lanes <= the context's max_lanes; lanes past it are
 * off); NULL, n_lanes == 0 or no record with on != 0 turns the stage off (default: no stage is
 * enqueued). Synchronises the context. Afterwards every udpdk_gpu_rx / udpdk_gpu_rx_host /
 * udpdk_gpu_rx_host_async / udpdk_gpu_pipe_rx_host call on this context filters its lanes, on the
 * call's own stream, before anything reads them (pipeline depths 2-4 work as before). With
 * udpdk_gpu_rx_drop flags or udpdk_gpu_rx_balance on as well, the drop filter runs first, the
 * balance second and this stage last; all three are per-entry predicates that do not depend on
 * what else the lanes hold, so they commute. (With the balance on, the hash may pick a group member
 * connected to somebody else: that delivery is then removed, not re-steered.) A call under a
 * snapshot with lane_mask != 0xFFFFFFFF returns -EINVAL.
 *   - udpdk_rx_stats_t: counters[] (UDPDK_C_DELIVERIES too) stay classify's; deliveries becomes
 *     the kept count, so it still equals lane_off[n_lanes]; overflow and -ENOSPC are still decided
 *     by the pre-stage total against lane_cap. */
int udpdk_gpu_rx_peer(udpdk_gpu_ctx *ctx, const udpdk_peer_t *peer_host, uint32_t n_lanes);

typedef struct {
    uint32_t kept, removed;
    uint32_t refused;      /* entries of connected lanes from another source                      */
    uint32_t bad_frame;    /* ... whose frame is shorter than 42 bytes or out of range: not read  */
    uint32_t bad_index;    /* entries >= n: removed, nothing of theirs read                       */
    uint32_t truncated;    /* input lane_off[n_lanes] > lane_cap: only the first lane_cap seen    */
} udpdk_rx_peer_stats_t;
/* Of the last peer filter run on the context (explicit or sticky; -ENOENT when there was none).
 * Synchronises. -ENOSPC if kept > out_cap. The launches are not event-timed. */
int udpdk_gpu_rx_peer_stats(udpdk_gpu_ctx *ctx, udpdk_rx_peer_stats_t *stats);
/* Poller internals, the sibling of udpdk_gpu_rx_removed: the lane entries the sticky peer filter
 * removed in the call whose results were last written to *stats (-ENOENT when no call's were). */
int udpdk_gpu_rx_peer_removed(udpdk_gpu_ctx *ctx, const udpdk_rx_stats_t *stats, uint32_t *refused);

/* ---------------------------------------------------------------------------------------------
 * RX multicast membership filter: a socket's lane keeps a multicast datagram only if the socket
 * joined the datagram's group (IP_ADD_MEMBERSHIP, udpdk_api.h). udpdk_gpu_rx matches a frame's
 * destination against a binding's address or INADDR_ANY, so without this stage a datagram to
 * 239.1.2.3:5000 lands in every ANY:5000 socket. The reference has no multicast; the rule is RFC
 * 1112's host group model with per-socket membership (Linux with IP_MULTICAST_ALL = 0). Off by
 * default: then udpdk_gpu_rx enqueues what it always did.
 *
 * The uploaded snapshot must have lane_mask == 0xFFFFFFFF (a lane is a sockfd). lane_mc is a
 * uint8[n_lanes] table. D = min(lane_off[n_lanes], lane_cap). Entry p of lane l with frame
 * i = lane_pkt[p] is handled by the first rule that applies:
 *   - i >= n: removed (bad_index); no descriptor or frame byte of it is read.
 *   - lane_mc[l] == 0: kept; no descriptor and no frame byte is read for the entry. (The socket
 *     layer clears lane_mc for sockets bound to a specific non-multicast address: the demux already
 *     proved the destination equals that address.)
 *   - length[i] < 42 or offset[i] + length[i] > frames_bytes (summed in 64 bits): removed
 *     (bad_frame); no frame byte is read.
 *   - dst = the raw u32 at frame bytes 30-33. If its first byte (dst & 0xFF) is outside 224..239 the
 *     entry is kept: unicast and 255.255.255.255.
 *   - otherwise kept iff (dst, l) is in the membership table (member), else removed (not_member).
 *   - The rule is per entry: a frame that fans out to a joined and an unjoined lane stays in the
 *     first only.
 *   - The output is the drop filter's: a stable compaction, lane_off_out[l] = kept entries before
 *     min(lane_off[l], D), nothing past lane_cap read, nothing past out_cap written.
 * meta is never read (lanes->meta_dev may be NULL) or rewritten.
 *
 * The membership table is read-only on the device: the caller builds it (udpdk_gpu_mcast_table_build)
 * and the stage never writes it. `slots` records, slots a power of two in 2..2^20; group == 0 marks
 * an empty slot. Open addressing, linear probing: the probe of (group, lane) starts at index
 * h >> (32 - log2(slots)), h = (group ^ (lane * 0x9E3779B1u)) * 0x85EBCA6Bu in uint32 arithmetic,
 * steps by one (wrapping past the last slot) and ends at a match, at an empty slot, or after
 * `slots` probes: a table with no empty slot is valid and its probes are bounded.
 * ------------------------------------------------------------------------------------------- */
typedef struct { uint32_t group; uint32_t lane; } udpdk_mcast_member_t;   /* raw group; 8 bytes */

/* Host only, pure: the table of members[n] in table_out[slots], inserted in the caller's order
 * (every slot is written: the ones not taken are zeroed). -EINVAL: a NULL pointer (members may be
 * NULL when n == 0), slots not a power of two in 2..2^20, a member with group == 0, a pair given
 * twice. -ENOSPC: n > slots. */
int udpdk_gpu_mcast_table_build(const udpdk_mcast_member_t *members, uint32_t n,
                                udpdk_mcast_member_t *table_out, uint32_t slots);

/* The filter as an explicit call on any lane set (lanes->n == batch->n): out of place, async on the
 * context stream. lane_mc_dev is [lanes->n_lanes]; table_dev is [slots], 8-byte aligned. An
 * all-zero lane_mc is a valid identity copy (only entries >= n are removed). -EINVAL with nothing
 * enqueued: the cases of udpdk_gpu_rx_peer_select (a NULL pointer, n_lanes outside
 * 1..UDPDK_GPU_MAX_LANES, no snapshot uploaded or one with lane_mask != 0xFFFFFFFF, outputs that
 * overlap the input lanes, lanes->n != batch->n, table_dev not 8-byte aligned), and slots not a
 * power of two in 2..2^20. The frames buffer keeps the tailroom contract of udpdk_gpu_rx. */
int udpdk_gpu_rx_mcast_select(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                              const udpdk_rx_lanes_t *lanes, const uint8_t *lane_mc_dev,
                              const udpdk_mcast_member_t *table_dev, uint32_t slots,
                              uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap);
/* Sticky mode: uploads lane_mc_host[n_lanes] (n_lanes <= the context's max_lanes; lanes past it are
 * exempt) and the table of members_host[n_members] (n_members <= 2^19; every member's lane <
 * n_lanes), built with slots = the smallest power of two >= 2 * n_members (minimum 2). NULL
 * lane_mc_host or n_lanes == 0 turns the stage off (default: no stage is enqueued); members_host may
 * be NULL when n_members == 0 (then checked lanes lose every multicast entry). -EINVAL for a pair
 * given twice, a group == 0, a lane >= n_lanes. Synchronises the context. Afterwards every
 * udpdk_gpu_rx / udpdk_gpu_rx_host / udpdk_gpu_rx_host_async / udpdk_gpu_pipe_rx_host call on this
 * context filters its lanes, on the call's own stream, before anything reads them. The stage runs
 * after the drop filter, the balance and the peer filter; all four are per-entry predicates that do
 * not depend on what else the lanes hold, so they commute. A call under a snapshot with lane_mask
 * != 0xFFFFFFFF returns -EINVAL.
 *   - udpdk_rx_stats_t: counters[] (UDPDK_C_DELIVERIES too) stay classify's; deliveries becomes
 *     the kept count, so it still equals lane_off[n_lanes]; overflow and -ENOSPC are still decided
 *     by the pre-stage total against lane_cap. */
int udpdk_gpu_rx_mcast(udpdk_gpu_ctx *ctx, const uint8_t *lane_mc_host, uint32_t n_lanes,
                       const udpdk_mcast_member_t *members_host, uint32_t n_members);

typedef struct {
    uint32_t kept, removed;
    uint32_t member;       /* multicast entries of checked lanes kept: the lane joined the group  */
    uint32_t not_member;   /* ... removed: it did not                                             */
    uint32_t bad_frame;    /* entries of checked lanes whose frame is shorter than 42 bytes or out
                              of range: not read                                                  */
    uint32_t bad_index;    /* entries >= n: removed, nothing of theirs read                       */
    uint32_t truncated;    /* input lane_off[n_lanes] > lane_cap: only the first lane_cap seen    */
} udpdk_rx_mcast_stats_t;
/* Of the last membership filter run on the context (explicit or sticky; -ENOENT when there was
 * none). Synchronises. -ENOSPC if kept > out_cap. The launches are not event-timed. */
int udpdk_gpu_rx_mcast_stats(udpdk_gpu_ctx *ctx, udpdk_rx_mcast_stats_t *stats);
/* Poller internals, the sibling of udpdk_gpu_rx_peer_removed: the lane entries the sticky
 * membership filter removed in the call whose results were last written to *stats (-ENOENT when no
 * call's were). */
int udpdk_gpu_rx_mcast_removed(udpdk_gpu_ctx *ctx, const udpdk_rx_stats_t *stats, uint32_t *not_member);

/* ---------------------------------------------------------------------------------------------
 * RX payload delivery: the batch form of udpdk_recvfrom (udpdk_syscall.c:401-488) over the lane
 * entries [first, first + count) of an RX output (e.g. one socket's lane, lane_off[s] ..
 * lane_off[s + 1], or all of them). Entry k = frame lane_pkt[first + k]: its UDP payload, frame
 * bytes [42, 42 + min(data_len - 42, dgram_len - 8)) (Ethernet padding trimmed, :459-466),
 * truncated to slot_bytes (recvfrom's len), goes to payload_dev + k * slot_bytes; len_dev[k] =
 * bytes copied (recvfrom's return value); src_ip_dev[k] / src_port_dev[k] = ip_hdr->src_addr /
 * udp_hdr->src_port as raw network-order values (sin_addr / sin_port, :446-447). Slot bytes past
 * len_dev[k] are scratch. Async on the context stream; the batch must be the one lane_pkt_dev
 * was computed from.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint8_t  *payload_dev;    /* [count * slot_bytes], 16-byte aligned                         */
    uint32_t  slot_bytes;     /* per-datagram buffer (recvfrom len), multiple of 16, >= 16      */
    uint32_t *len_dev;        /* [count]                                                       */
    uint32_t *src_ip_dev;     /* [count]                                                       */
    uint16_t *src_port_dev;   /* [count]                                                       */
} udpdk_rx_gather_t;

int udpdk_gpu_rx_gather(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                        const uint32_t *lane_pkt_dev, uint32_t first, uint32_t count,
                        const udpdk_rx_gather_t *out);
/* The same with packed slots: entry k's buffer is payload_dev + slot_off_dev[k], of
 * slot_off_dev[k + 1] - slot_off_dev[k] bytes (multiples of 16, ascending, count + 1 offsets);
 * out->slot_bytes is not used. A poller sizing each slot to its frame (data_len - 42, rounded up
 * to 16) hands the application every payload with one copy of only the bytes that exist. */
int udpdk_gpu_rx_gather_packed(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                               const uint32_t *lane_pkt_dev, uint32_t first, uint32_t count,
                               const uint32_t *slot_off_dev, const udpdk_rx_gather_t *out);
/* The packed gather on pipe `pipe`'s stream (poller internals, above). */
int udpdk_gpu_pipe_gather_packed(udpdk_gpu_ctx *ctx, int pipe, const udpdk_rx_batch_t *batch,
                                 const uint32_t *lane_pkt_dev, uint32_t first, uint32_t count,
                                 const uint32_t *slot_off_dev, const udpdk_rx_gather_t *out);

/* ---------------------------------------------------------------------------------------------
 * RX reassembly of IPv4 fragments (udpdk_poller.c:338-361: FRAG frames go through
 * rte_ipv4_frag_reassemble_packet on the table of udpdk_poller.c:130, and a completed datagram
 * continues through the demux at the position of the fragment that completed it)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t bucket_num;      /* NUM_FLOWS_DEF = 0x1000 (udpdk_constants.h:32)                  */
    uint32_t bucket_entries;  /* IP_FRAG_TBL_BUCKET_ENTRIES = 16 (power of two, <= 32)          */
    uint64_t max_cycles;      /* flow lifetime in the unit of the tms argument (frag_cycles =
                                 MAX_FLOW_TTL = 1 s of TSC cycles in the reference)              */
    uint32_t max_dgram;       /* IPv4 payload bytes one flow can hold, <= 65515; device memory is
                                 about entries x (max_dgram + 34) bytes                           */
    uint32_t max_entries;     /* NUM_FLOWS_MAX = 65535 (udpdk_constants.h:34): ip_frag_find adds a
                                 flow to a free entry only while fewer than max_entries are in
                                 use; at the limit it deletes the least recently added (or reused)
                                 entry if that one has expired, else drops the fragment (no
                                 space). 0: the table's entry count (the limit never applies).  */
    uint32_t flags;           /* UDPDK_FRAG_CKSUM_DPDK                                          */
    uint32_t reserved;        /* 0                                                              */
} udpdk_frag_table_cfg_t;

/* A reassembled datagram's IPv4 header checksum is left 0, as DPDK 20.05's ipv4_frag_reassemble
 * writes it and the reference delivers it ("TODO must fix the IP header checksum",
 * udpdk_poller.c:355-360), instead of the RFC 1071 value. */
#define UDPDK_FRAG_CKSUM_DPDK 1u

enum udpdk_rs_stat {
    UDPDK_RS_FRAGS      = 0, /* FRAG-verdict frames of the batch                                */
    UDPDK_RS_DROP_LEN   = 1, /* total_length <= 20 (rte_ipv4_frag_reassemble_packet drops it)    */
    UDPDK_RS_DROP_SHORT = 2, /* IP data past the frame or past max_dgram (divergence) */
    UDPDK_RS_NO_SPACE   = 3, /* no free or expired entry in the key's two buckets                */
    UDPDK_RS_ERRORS     = 4, /* flows dropped: duplicate first/last, > 4 fragments, bad size     */
    UDPDK_RS_HOLES      = 5, /* flows dropped: size complete but the fragments do not chain      */
    UDPDK_RS_EXPIRED    = 6, /* flows freed on timeout                                           */
    UDPDK_RS_DONE       = 7, /* datagrams reassembled                                             */
    UDPDK_RS_STORED     = 8, /* fragments of this batch held by the table for later batches      */
    UDPDK_RS_SERIAL     = 9, /* diagnostic: fragments that went through the table one at a time
                                in arrival order (flows that share buckets with an overlapping
                                flow, stay pending, or meet an existing or expired entry)       */
    UDPDK_RS_SORTED     = 10, /* diagnostic: 1 if the batch's flow keys needed the sorts (a key
                                 with fragments in several runs of the batch), 0 if every key's
                                 fragments were already one run in arrival order                */
    UDPDK_RS_N          = 11
};

typedef struct {
    udpdk_rx_batch_t batch;   /* reassembled frames (context-owned, valid until the next call):
                                 first fragment's Ethernet/IPv4 header with total length, DF-only
                                 fragment field and a valid checksum, then the IPv4 payload;
                                 ptype 0x211. Feed it to udpdk_gpu_rx for the demux.           */
    const uint32_t *origin_dev; /* [batch.n] index (in the input batch) of the fragment that
                                 completed each datagram; the datagrams are in this order       */
    uint64_t stats[UDPDK_RS_N];
} udpdk_reasm_out_t;

/* rte_ip_frag_table_create (udpdk_poller.c:130) on the device; replaces an existing table. */
int udpdk_gpu_frag_table_create(udpdk_gpu_ctx *ctx, const udpdk_frag_table_cfg_t *cfg);
/* Reassembly step for one batch whose udpdk_gpu_rx verdicts are in meta_dev (FRAG frames are
 * consumed; state persists across calls). tms is the batch's timestamp (the poller's cur_tsc).
 * Synchronous. Every output, count and table entry equals one-fragment-at-a-time processing in
 * arrival order (rte_ipv4_frag_reassemble_packet per fragment, udpdk_poller.c:338-361): flows
 * that cannot meet another flow in the table run in parallel, the rest in arrival order. */
int udpdk_gpu_rx_reassemble(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                            const uint32_t *meta_dev, uint64_t tms, udpdk_reasm_out_t *out);
/* As udpdk_gpu_rx_reassemble, consuming the FRAG frames' bytes the way DPDK chains the fragment
 * mbufs instead of copying them: when every datagram the call completes has its fragments back
 * to back in batch->frames_dev, in data order, each exactly 34 header bytes + its data (a
 * fragmenting sender's frames received in order), the first fragment's frame is extended over its
 * followers (each later fragment's data moves back over the headers before it, the header is
 * patched) and out->batch.frames_dev is batch->frames_dev, with the datagrams at their first
 * fragment's offset. Otherwise the call copies, exactly as udpdk_gpu_rx_reassemble. The frame
 * buffer must be writable and its frames must not overlap; other frames are not touched. */
int udpdk_gpu_rx_reassemble_inplace(udpdk_gpu_ctx *ctx, udpdk_rx_batch_t *batch,
                                    const uint32_t *meta_dev, uint64_t tms, udpdk_reasm_out_t *out);

/* ---------------------------------------------------------------------------------------------
 * Receive-side scaling: the reference configures ETH_MQ_RX_RSS with a single
 * RX ring ("TODO add RSS support", udpdk_init.c:112-137) and polls queue 0 (udpdk_poller.c:516).
 * udpdk_gpu_rss computes, per frame, the Toeplitz hash a NIC computes for rss_hf = IPv4 |
 * non-fragmented IPv4 UDP and the redirection-table queue, and lists each queue's frames in
 * arrival order: the split of one ingress batch over several pollers or GPUs by flow.
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_RSS_KEY_BYTES   40u
#define UDPDK_RSS_RETA_MAX    512u
#define UDPDK_RSS_MAX_QUEUES  64u
enum udpdk_rss_type {
    UDPDK_RSS_IPV4            = 1u, /* 2-tuple (src, dst address) for IPv4 frames              */
    UDPDK_RSS_NONFRAG_IPV4_UDP = 2u /* 4-tuple (+ src, dst port) for unfragmented UDP          */
};
typedef struct {
    uint8_t  key[UDPDK_RSS_KEY_BYTES];  /* rss_key, byte 0 first                                */
    uint32_t hash_types;                /* udpdk_rss_type bits                                   */
    uint32_t n_queues;                  /* RX queues, 1..UDPDK_RSS_MAX_QUEUES                    */
    uint32_t reta_size;                 /* power of two, 1..UDPDK_RSS_RETA_MAX                   */
    uint16_t reta[UDPDK_RSS_RETA_MAX];  /* queue of entry hash & (reta_size - 1)                 */
} udpdk_rss_conf_t;

typedef struct {
    uint32_t *hash_dev;       /* [n] the frame's RSS hash (mbuf hash.rss); 0 when no type applies */
    uint32_t *queue_off_dev;  /* [n_queues + 1] exclusive prefix of per-queue frame counts        */
    uint32_t *queue_pkt_dev;  /* [n] frame indices grouped by queue, arrival order kept           */
} udpdk_rss_out_t;

/* The widely used 40-byte Toeplitz key (the RSS verification suite's), both hash types, and a
 * 128-entry redirection table spreading entries round-robin over n_queues. Host only. */
int udpdk_gpu_rss_default_conf(udpdk_rss_conf_t *conf, uint32_t n_queues);
/* rte_eth_dev_rss_hash_update + rte_eth_dev_rss_reta_update: the context's RSS configuration. */
int udpdk_gpu_rss_config(udpdk_gpu_ctx *ctx, const udpdk_rss_conf_t *conf);
/* Hash, queue and per-queue lists for one batch (async on the context stream). Frames the IPv4
 * gate rejects (the rx_classify ptype rule) or with descriptors past frames_bytes get hash 0. */
int udpdk_gpu_rss(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch, const udpdk_rss_out_t *out);

/* ---------------------------------------------------------------------------------------------
 * TX: Eth/IPv4/UDP header build + rte_ipv4_cksum + payload copy (udpdk_syscall.c:314-356)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint8_t  src_mac[6];     /* config.src_mac_addr ([port0] mac_addr, udpdk_args.c:21-49)     */
    uint8_t  dst_mac[6];     /* config.dst_mac_addr ([port0_dst] mac_addr)                     */
    uint32_t src_ip;         /* config.src_ip_addr, raw                                        */
} udpdk_tx_config_t;

typedef struct {
    const uint8_t  *payload_dev;     /* payload bytes, followed by UDPDK_GPU_FRAMES_TAILROOM
                                        readable bytes (a payload ending at payload_bytes is
                                        read with dword loads up to 3 bytes past it)           */
    uint64_t        payload_bytes;
    const uint32_t *payload_off_dev; /* [n]                                                    */
    const uint16_t *payload_len_dev; /* [n] sendto len, <= 65507                               */
    const int32_t  *sockfd_dev;      /* [n] sending socket (slot table from the snapshot)      */
    const uint32_t *dst_ip_dev;      /* [n] raw dest_addr->sin_addr                            */
    const uint16_t *dst_port_dev;    /* [n] raw dest_addr->sin_port                            */
    uint32_t        n;
} udpdk_tx_batch_t;

typedef struct {
    uint8_t        *frames_dev;      /* output frames                                          */
    uint64_t        frames_bytes;    /* capacity                                               */
    const uint32_t *frame_off_dev;   /* [n] where datagram i's frame(s) start (len_i + 42
                                        bytes, or udpdk_gpu_tx_span() with fragmentation)    */
} udpdk_tx_out_t;

int udpdk_gpu_tx_build(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                       const udpdk_tx_batch_t *batch, const udpdk_tx_out_t *out);

/* TX with the poller's IPv4 fragmentation (udpdk_poller.c:461-501: a frame of pkt_len =
 * len + 42 > IPV4_MTU_DEFAULT goes through rte_ipv4_fragment_packet(pkt, ..., mtu) and gets its
 * Ethernet header back per fragment). mtu = 1500 reproduces the reference (IPV4_MTU_DEFAULT =
 * RTE_ETHER_MTU, udpdk_constants.h:37); mtu = 0 is udpdk_gpu_tx_build. (mtu - 20) must be a
 * multiple of 8 and mtu >= 68. Every fragment carries mtu - 20 bytes of the IPv4 payload (the
 * UDP header + data), the last the remainder; fragment k of datagram i starts at
 * frame_off[i] + k * (mtu + 14), so datagram i occupies udpdk_gpu_tx_span(len_i, mtu) bytes.
 * Fragment headers: total length 20 + fragment payload, fragment offset (8-byte units) + MF on
 * all but the last, id 0 (as sent), and the IPv4 checksum a NIC fills for PKT_TX_IP_CKSUM
 * (~RFC 1071 sum; DPDK leaves 0 in the mbuf). Unfragmented frames are exactly tx_build's. */
int udpdk_gpu_tx_build_mtu(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                           const udpdk_tx_batch_t *batch, const udpdk_tx_out_t *out,
                           uint32_t mtu);
/* udpdk_gpu_tx_build_mtu with options. flags == 0 is udpdk_gpu_tx_build_mtu exactly (same kernel,
 * same launch form); bits outside the ones below give -EINVAL and write nothing.
 *
 * UDPDK_TX_UDP_CKSUM: every written datagram carries its RFC 768 checksum at bytes 40-41 of its
 * first frame instead of the reference's 0 ("UDP checksum is optional", udpdk_syscall.c:343):
 * the one's-complement sum of the pseudo-header (the source address the IPv4 header got,
 * destination address, zero, 17, UDP length), the UDP header with a zero checksum field and the
 * payload zero-padded to even length, complemented, 0 sent as 0xFFFF. With an MTU the checksum
 * covers the whole datagram and is in fragment 0 only (later fragments carry no UDP header).
 * Every other byte of every frame is what flags == 0 writes. The checksum is computed from the
 * payload bytes the kernel already holds on their way to the frame (no extra memory traffic);
 * one wave then builds a whole group of 64 datagrams, so UDPDK_TX_PARTS does not apply. */
#define UDPDK_TX_UDP_CKSUM 1u
int udpdk_gpu_tx_build_flags(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                             const udpdk_tx_batch_t *batch, const udpdk_tx_out_t *out,
                             uint32_t mtu, uint32_t flags);
/* Output bytes of one datagram of `len` payload bytes and its frame count (host helper). */
uint64_t udpdk_gpu_tx_span(uint32_t len, uint32_t mtu, uint32_t *n_frames);

/* ---------------------------------------------------------------------------------------------
 * TX reply: answer received datagrams on the device (the server side of apps/pingpong: recvfrom,
 * then sendto back to the source; the reference has no batch form of it). Everything tx_build needs
 * is already in device memory after udpdk_gpu_rx: the payload is at frame byte 42, the peer's
 * address in frame bytes 26-35 and the answering socket is the lane an entry is in. A reply plan
 * turns the lane entries [first, first + count) into the descriptor arrays of a udpdk_tx_batch_t
 * whose payload_dev is the RX batch's frames_dev: no gather, no copy to the host, no host loop. An
 * application that rewrites payloads in place in the frame buffer between udpdk_gpu_rx and the
 * reply answers with the rewritten bytes.
 *
 * Entry k is lane entry p = first + k, frame i = lane_pkt[p], D = min(lane_off[n_lanes], lane_cap):
 *   sockfd[k]       the largest lane l < n_lanes with lane_off[l] <= p, an offset beyond D counting
 *                   as D (udpdk_gpu_rx_filter's bounds convention), so empty lanes are passed over;
 *                   lane_off must be non-decreasing from lane_off[0] = 0, as an exclusive prefix is
 *   payload_off[k]  offset[i] + 42
 *   payload_len[k]  min(length[i] - 42, (dgram_len - 8) & 0xFFFF), dgram_len the big-endian u16 at
 *                   frame byte 38: udpdk_gpu_rx_gather's rule with an unbounded slot
 *   dst_ip[k], dst_port[k]   frame bytes 26-29 and 34-35, raw
 *   frame_off[k]    exclusive prefix of udpdk_gpu_tx_span(payload_len, mtu) over the entries that
 *                   answer, summed in 64 bits; frame_off[count] = where the output ends (<= out_cap)
 * An entry does not answer when p >= D, i >= n (bad_index; no descriptor or frame byte is read),
 * length[i] < 42, offset[i] + length[i] > frames_bytes, its lane is unselected (lane_sel_dev !=
 * NULL and lane_sel_dev[l] == 0; lane_sel_dev is [n_lanes]), or its frames would end past out_cap
 * (no_room; the prefix is monotone, so these are a tail of the range and their frame_off is the
 * output's end). Such an entry gets sockfd -1, zeros in the other arrays and no output bytes;
 * tx_build writes nothing for a negative sockfd. lanes->meta_dev is not read and may be NULL.
 *
 * Both calls are asynchronous on the context stream and join the pipes as udpdk_gpu_tx_build does.
 * -EINVAL, with nothing enqueued: a NULL pointer (lane_sel_dev excepted), n_lanes outside
 * 1..UDPDK_GPU_MAX_LANES, frames_bytes or out_cap >= 2^32, a bad mtu (udpdk_gpu_tx_build_mtu's
 * rule) or flags, frames_out_dev not 16-byte aligned, first + count >= 2^32, no slot table in the
 * uploaded snapshot, or a snapshot with lane_mask != 0xFFFFFFFF (in compat mode a lane is not a
 * sockfd). count == 0 returns 0. The plan launches are not event-timed (udpdk_gpu_timing_read).
 * ------------------------------------------------------------------------------------------- */
typedef struct {                    /* all [count] except frame_off_dev [count + 1] */
    uint32_t *payload_off_dev; uint16_t *payload_len_dev; int32_t *sockfd_dev;
    uint32_t *dst_ip_dev; uint16_t *dst_port_dev; uint32_t *frame_off_dev;
} udpdk_tx_reply_plan_t;

int udpdk_gpu_tx_reply_plan(udpdk_gpu_ctx *ctx, const udpdk_rx_batch_t *batch,
                            const udpdk_rx_lanes_t *lanes, uint32_t first, uint32_t count,
                            const uint8_t *lane_sel_dev, uint32_t mtu, uint64_t out_cap,
                            const udpdk_tx_reply_plan_t *plan);
/* The plan, then udpdk_gpu_tx_build_flags over {payload_dev = batch->frames_dev, payload_bytes =
 * batch->frames_bytes, the plan's arrays, n = count} into {frames_out_dev, out_cap,
 * plan->frame_off_dev}: mtu and flags as there (that launch is timed as always). The output must
 * not overlap the RX frame buffer. Source address and port are the answering socket's slot (the
 * config IP for an ANY binding), what a sendto from that socket would send, not the request's
 * destination. */
int udpdk_gpu_tx_reply(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                       const udpdk_rx_batch_t *batch, const udpdk_rx_lanes_t *lanes,
                       uint32_t first, uint32_t count, const uint8_t *lane_sel_dev, uint32_t mtu,
                       uint32_t flags, uint8_t *frames_out_dev, uint64_t out_cap,
                       const udpdk_tx_reply_plan_t *plan);

typedef struct {
    uint64_t bytes_needed;   /* the out_cap with which no entry is out of room                  */
    uint32_t replied;        /* entries that answer                                              */
    uint32_t skipped;        /* count - replied, whatever the reason                             */
    uint32_t bad_index;      /* entries >= n                                                     */
    uint32_t unselected;     /* entries with a good frame in an unselected lane                  */
    uint32_t no_room;        /* entries out of room                                              */
    uint32_t frames;         /* output frames of the entries that answer, fragments included     */
} udpdk_tx_reply_stats_t;
/* Of the last plan on the context (-ENOENT when there was none). Synchronises. -ENOSPC when
 * no_room > 0. */
int udpdk_gpu_tx_reply_stats(udpdk_gpu_ctx *ctx, udpdk_tx_reply_stats_t *stats);
/* Entries per workgroup of the plan kernels and the workgroup count for `count` entries (host
 * only, like udpdk_gpu_rx_geometry). */
int udpdk_gpu_tx_reply_geometry(uint32_t count, uint32_t *entries_per_block, uint32_t *n_blocks);

/* ---------------------------------------------------------------------------------------------
 * TX segmentation: Linux's UDP_SEGMENT on the device. One send carries the payload of up to
 * UDPDK_GSO_MAX_SEGS datagrams plus a segment size, and the stack cuts it: a segment plan turns k
 * sends in device memory into the descriptor arrays of a udpdk_tx_batch_t with one entry per
 * segment, over the same payload buffer, and tx_build does the rest. No host loop over datagrams.
 *
 * Send j of [0, k) has nseg_j segments:
 *   0                     when it is skipped (below)
 *   1                     when gso_size == 0 or payload_len <= gso_size; a zero-length send is one
 *                         empty datagram
 *   ceil(len / gso_size)  otherwise
 * A send is skipped, with no descriptors and no output bytes, in this order of precedence:
 *   skipped    sockfd < 0
 *   too_long   payload_len > 65507
 *   bad_range  payload_off + payload_len > payload_bytes (no payload byte is read by the plan in
 *              any case)
 *   too_many   seg_limit != 0 && nseg > seg_limit
 *   no_room    its last segment index would reach max_segs, or its frames would end past out_cap,
 *              both counted over every send the rules above let through. Both prefixes are
 *              monotone, so the sends out of room are a tail. A send is all or nothing and is never
 *              split.
 * Placement:
 *   seg_off[j]      exclusive prefix of nseg; N = seg_off[k]
 *   segment m = seg_off[j] + t gets
 *   payload_off[m]  payload_off_j + t * gso_size
 *   payload_len[m]  min(gso_size, len_j - t * gso_size) (len_j for the one segment of a send that
 *                   is not cut)
 *   sockfd[m], dst_ip[m], dst_port[m]   send j's
 *   frame_off[m]    exclusive prefix of udpdk_gpu_tx_span(payload_len[m], mtu) over the segments,
 *                   summed in 64 bits; frame_off[N] = where the output ends (<= out_cap). Within a
 *                   send, frame_off = base_j + t * span(gso_size).
 * A segment may itself exceed the MTU and fragment: the span rule covers it and tx_build does the
 * rest (the socket layer never produces that case). Descriptor slots m in [N, max_segs) get
 * sockfd -1 and zeros, and frame_off[m] for m in (N, max_segs] the output's end, so tx_build over
 * n = max_segs is correct without a host synchronisation: it writes nothing for a negative sockfd.
 *
 * Both calls are asynchronous on the context stream and join the pipes as udpdk_gpu_tx_build does.
 * -EINVAL, with nothing enqueued: a NULL pointer, a bad mtu (udpdk_gpu_tx_build_mtu's rule) or
 * flags, out_cap or payload_bytes >= 2^32, max_segs == 0, k + max_segs >= 2^32, and for
 * udpdk_gpu_tx_segment what udpdk_gpu_tx_build_flags refuses (alignment, no slot table). k == 0
 * returns 0. The plan launches are not event-timed (udpdk_gpu_timing_read).
 *
 * Not part of this interface: receive-side coalescing (UDP_GRO), udpdk_poll_echo, MSG_MORE /
 * corking, recvmsg.
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_GSO_MAX_SEGS 64u      /* Linux's UDP_MAX_SEGMENTS: what the socket layer lets one send carry */

typedef struct {                    /* all [k], against one payload buffer */
    const uint8_t  *payload_dev;     /* tx_build's tailroom contract (udpdk_tx_batch_t)          */
    uint64_t        payload_bytes;
    const uint32_t *payload_off_dev;
    const uint16_t *payload_len_dev;
    const uint16_t *gso_size_dev;
    const int32_t  *sockfd_dev;
    const uint32_t *dst_ip_dev;
    const uint16_t *dst_port_dev;
    uint32_t        k;
} udpdk_tx_sends_t;

typedef struct {                    /* all [max_segs] except frame_off_dev [max_segs + 1], seg_off_dev [k + 1] */
    uint32_t *payload_off_dev; uint16_t *payload_len_dev; int32_t *sockfd_dev;
    uint32_t *dst_ip_dev; uint16_t *dst_port_dev; uint32_t *frame_off_dev;
    uint32_t *seg_off_dev;
    uint32_t  max_segs;
} udpdk_tx_segment_plan_t;

int udpdk_gpu_tx_segment_plan(udpdk_gpu_ctx *ctx, const udpdk_tx_sends_t *sends, uint32_t mtu,
                              uint32_t seg_limit, uint64_t out_cap, const udpdk_tx_segment_plan_t *plan);
/* The plan, then udpdk_gpu_tx_build_flags over {sends->payload_dev, sends->payload_bytes, the plan's
 * arrays, n = max_segs} into {frames_out_dev, out_cap, plan->frame_off_dev}: mtu and flags as there
 * (that launch is timed as always). */
int udpdk_gpu_tx_segment(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg, const udpdk_tx_sends_t *sends,
                         uint32_t mtu, uint32_t flags, uint32_t seg_limit, uint8_t *frames_out_dev,
                         uint64_t out_cap, const udpdk_tx_segment_plan_t *plan);

typedef struct {
    uint64_t bytes_needed;   /* the out_cap with which no send is out of room                    */
    uint64_t segs_needed;    /* the max_segs with which no send is out of room                   */
    uint32_t sends;          /* sends that produced segments                                     */
    uint32_t segments;       /* N                                                                */
    uint32_t frames;         /* output frames of those segments, fragments included              */
    uint32_t skipped;        /* sockfd < 0                                                       */
    uint32_t too_long;
    uint32_t bad_range;
    uint32_t too_many;
    uint32_t no_room;
} udpdk_tx_segment_stats_t;
/* Of the last plan on the context (-ENOENT when there was none). Synchronises. -ENOSPC when
 * no_room > 0. */
int udpdk_gpu_tx_segment_stats(udpdk_gpu_ctx *ctx, udpdk_tx_segment_stats_t *stats);
/* Output bytes of one send of `len` payload bytes cut at `gso` and its segment and frame counts, by
 * the definition above without the skip rules (host helper, needs no GPU): with q = len / gso and
 * r = len % gso, q * span(gso) + (r ? span(r) : 0); span(len) and one segment when gso == 0 or
 * len <= gso. nseg and n_frames may be NULL. */
uint64_t udpdk_gpu_tx_segment_span(uint32_t len, uint32_t gso, uint32_t mtu, uint32_t *nseg, uint32_t *n_frames);
/* Sends and segments per workgroup of the plan kernels and the workgroup counts for k sends and
 * max_segs segments (host only, like udpdk_gpu_tx_reply_geometry). */
int udpdk_gpu_tx_segment_geometry(uint32_t k, uint32_t max_segs, uint32_t *sends_per_block,
                                  uint32_t *segs_per_block, uint32_t *send_blocks, uint32_t *seg_blocks);

/* ---------------------------------------------------------------------------------------------
 * ICMP on the device: echo replies and port-unreachable errors. The reference has no ICMP: an echo
 * request ends as UDPDK_V_NOT_UDP and a datagram for a closed port as UDPDK_V_NO_BIND / NO_MATCH, and
 * nothing looks at either again. This optional stage after udpdk_gpu_rx answers both from what is
 * already in device memory (the verdict words, the staged frames): a host that runs this stack
 * answers `ping`, and a client of a dead service gets ECONNREFUSED instead of waiting out its
 * timeout (RFC 1122 §3.2.2.1, §4.1.3.1). Parity is against RFCs 792, 1071 and 1122. Off unless called.
 *
 * All addresses are raw. m = meta[i], tl = the big-endian u16 at frame bytes 16-17.
 *
 * Candidate by meta (no descriptor and no frame byte is read for any other frame, so a batch of UDP
 * to bound ports costs the read of meta):
 *   echo     flags & UDPDK_ICMP_ECHO, verdict NOT_UDP, UDPDK_META_IP_OK(m), !UDPDK_META_IHL_NE5(m)
 *   unreach  flags & UDPDK_ICMP_UNREACH, verdict NO_BIND or NO_MATCH, IP_OK, !IHL_NE5,
 *            UDPDK_META_UDP_CSUM(m) != UDPDK_UDP_CSUM_BAD and !UDPDK_META_LEN_BAD(m) (Linux drops a
 *            datagram with a bad checksum before it reports the port)
 * A candidate then passes the common gate:
 *   - length[i] >= 42 and offset[i] + length[i] <= frames_bytes (64 bits), else it counts as
 *     bad_frame and no frame byte is read (meta need not come from this batch);
 *   - the destination address (bytes 30-33) == cfg->src_ip: unicast to us only, broadcast and
 *     multicast are never answered (RFC 1122 §3.2.2);
 *   - the first byte of the source address (byte 26) is not 0, not 127 and < 224.
 *
 * Echo request: an echo candidate past the gate with byte 23 == 1, byte 34 == 8, byte 35 == 0. It is
 * answered iff 28 <= tl, 14 + tl <= length[i], mtu == 0 || tl <= mtu, and the one's-complement sum
 * of bytes [34, 14 + tl) verifies (odd tail zero-padded; Ethernet padding past 14 + tl is neither
 * summed nor copied); else it counts as echo_bad. The reply has 14 + tl bytes: Ethernet and IPv4
 * headers as tx_build writes them for an unfragmented datagram (config MACs, 0x0800, 0x45, tos 0,
 * id 0, fragment field 0, ttl 64, the same header checksum function) with total length tl,
 * protocol 1, source cfg->src_ip, destination the request's source; then 00 00, the checksum, and
 * request bytes [38, 14 + tl). The ICMP checksum is the full RFC 1071 value ~fold(sum) & 0xFFFF with
 * no substitution: an all-zero reply carries FF FF, one summing to 0xFFFF carries 00 00.
 *
 * Port unreachable: of the unreach candidates past the gate (the eligible ones) the first err_limit
 * in arrival order are answered, the rest count as limited (0xFFFFFFFF: no limit; 0: none). The
 * reply has UDPDK_ICMP_UNREACH_BYTES: the headers as above with total length 56; 03 03, the
 * checksum, 00 00 00 00; request bytes [14, 42) (the IPv4 header as received and the UDP header).
 *
 * Replies are in frame order, echo replies and errors interleaved. reply_off is the exclusive
 * prefix (64 bits) of the lengths of the replies the limit leaves; reply r is written iff r <
 * max_replies and its end <= out_cap, so the replies cut are a tail (no_room; no byte of theirs is
 * written); reply_off[replies] is the end of the output. The limit applies before room: a cut error
 * still used a slot of it. Fragments carry the FRAG verdict and are never answered.
 *
 * Asynchronous on the context stream; joins the pipes as udpdk_gpu_tx_build does. -EINVAL with
 * nothing enqueued: a NULL pointer, flags 0 or with bits outside UDPDK_ICMP_ALL, frames_bytes or
 * out_cap >= 2^32, an mtu udpdk_gpu_tx_build_mtu rejects, out->frames_dev not 16-byte aligned, an
 * output that overlaps the frame buffer. n == 0 returns 0 with reply_off[0] = 0. The frames buffer
 * keeps the tailroom contract of udpdk_gpu_rx. meta is read and never written. No snapshot is
 * needed. The launches are not event-timed.
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_ICMP_ECHO          1u   /* answer echo requests (type 8 -> type 0)            */
#define UDPDK_ICMP_UNREACH       2u   /* answer UDP to a closed port with type 3 code 3     */
#define UDPDK_ICMP_ALL           3u
#define UDPDK_ICMP_UNREACH_BYTES 70u  /* 14 + 20 + 8 + 28                                    */

typedef struct {
    uint8_t  *frames_dev;     /* replies back to back, arrival order; 16-byte aligned base   */
    uint64_t  out_cap;        /* < 2^32                                                      */
    uint32_t *reply_off_dev;  /* [max_replies + 1]; reply r is [reply_off[r], reply_off[r+1]) */
    uint32_t *origin_dev;     /* [max_replies] index of the frame reply r answers            */
    uint32_t  max_replies;
} udpdk_icmp_out_t;

typedef struct {
    uint64_t bytes_needed;    /* out_cap with which nothing is out of room                   */
    uint32_t replies;         /* written: echo_replied + unreach_sent                        */
    uint32_t echo_replied, unreach_sent;
    uint32_t echo_bad;        /* echo requests past the gates with a bad length, checksum or tl > mtu */
    uint32_t limited;         /* eligible errors beyond err_limit                            */
    uint32_t no_room;         /* eligible replies cut by out_cap or max_replies (a tail)     */
    uint32_t bad_frame;       /* candidate by meta, but length < 42 or out of range: not read */
} udpdk_icmp_stats_t;

int udpdk_gpu_icmp_reply(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                         const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                         uint32_t flags, uint32_t mtu, uint32_t err_limit,
                         const udpdk_icmp_out_t *out);
/* Of the last udpdk_gpu_icmp_reply on the context (-ENOENT when there was none). Synchronises.
 * -ENOSPC when no_room > 0. */
int udpdk_gpu_icmp_stats(udpdk_gpu_ctx *ctx, udpdk_icmp_stats_t *stats);
/* Frames per workgroup of the scan and build kernels and the workgroup count for n frames (host
 * only, like udpdk_gpu_tx_reply_geometry). */
int udpdk_gpu_icmp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks);
/* Poller internals: the same stage on pipe `pipe`'s stream (1 .. 3) with that pipe's workspace and
 * no joins, like udpdk_gpu_pipe_gather_packed; the counts are copied to pinned memory on the same
 * stream. udpdk_gpu_pipe_icmp_stats reads them without synchronising: they are those of the pipe's
 * last stage once udpdk_gpu_pipe_wait has returned (-ENOENT: the pipe never ran one; -ENOSPC as above). */
int udpdk_gpu_pipe_icmp_reply(udpdk_gpu_ctx *ctx, int pipe, const udpdk_tx_config_t *cfg,
                              const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                              uint32_t flags, uint32_t mtu, uint32_t err_limit,
                              const udpdk_icmp_out_t *out);
int udpdk_gpu_pipe_icmp_stats(udpdk_gpu_ctx *ctx, int pipe, udpdk_icmp_stats_t *stats);

/* ---------------------------------------------------------------------------------------------
 * ICMP errors received: of a finished udpdk_gpu_rx call, the destination-unreachable messages (type
 * 3) that quote a datagram one of our connected sockets sent to its peer, as one 64-bit word per lane
 * for the last such hard error in arrival order (Linux: a later error overwrites sk_err). RFC 1122
 * §4.1.3.3: UDP MUST pass ICMP errors up to the application; this is what connect() on a UDP socket
 * gives a POSIX program beyond the peer filter (ECONNREFUSED from a dead service instead of a
 * timeout). The reference has no ICMP and no connect. One more optional stage after RX, reading the
 * verdict words, the staged frames, the uploaded bind snapshot and a peer table.
 *
 * m = meta[i]; tl = the big-endian u16 at frame bytes 16-17; addresses and ports are raw.
 *   - Candidate by meta: verdict NOT_UDP, UDPDK_META_IP_OK(m), not UDPDK_META_IHL_NE5(m). For any other
 *     frame no descriptor and no frame byte is read: a batch of UDP to bound ports costs the read
 *     of meta plus the clearing of err_dev.
 *   - Frame gate: length[i] >= 42 and offset[i] + length[i] <= frames_bytes (64 bits), else the
 *     candidate counts as bad_frame and no frame byte is read (meta need not come from this batch).
 *   - An error to us (counted under errors): byte 23 == 1, byte 34 == 3, bytes 30-33 == our_ip.
 *     Anything else (echo traffic, other ICMP types, other destinations) is counted nowhere.
 *   - Message: valid when tl >= 56, 14 + tl <= length[i] and the one's-complement sum of bytes
 *     [34, 14 + tl) verifies (odd tail zero-padded; Ethernet padding past 14 + tl is not summed);
 *     else msg_bad. Messages are 36 bytes up to a full MTU (routers quote as much as they can).
 *   - Quote: valid when byte 42 == 0x45, byte 51 == 17 and the quoted fragment offset is 0
 *     (be16(bytes 48-49) & 0x1FFF == 0); else quote_bad. The quoted header checksum is not verified
 *     (Linux does not verify it either). Quoted source: bytes 54-57, destination: 58-61, source
 *     port: 62-63, destination port: 64-65.
 *   - Code (byte 35): udpdk_gpu_icmp_errno's table, which is Linux's icmp_err_convert:
 *       0 ENETUNREACH soft, 1 EHOSTUNREACH soft, 2 ENOPROTOOPT hard, 3 ECONNREFUSED hard,
 *       4 EMSGSIZE soft (we send with DF clear), 5 EOPNOTSUPP soft, 6 ENETUNREACH hard,
 *       7 EHOSTDOWN hard, 8 ENONET hard, 9 ENETUNREACH hard, 10 EHOSTUNREACH hard, 11 ENETUNREACH
 *       soft, 12 EHOSTUNREACH soft, 13-15 EHOSTUNREACH hard, above 15: none, soft.
 *     A code that is not hard counts as soft and reports nothing.
 *   - Socket: the snapshot's bindings of the quoted source port in list order; binding b with lane
 *     l = b.sockfd matches when l < n_lanes, b.ip == the quoted source (or b.ip == 0 and the quoted
 *     source is our_ip: what an ANY socket sends), peer[l].on, peer[l].ip == the quoted
 *     destination and peer[l].port == the quoted destination port. Every match is reported: the
 *     walk does not stop at a binding without reuse (two sockets cannot both own the 5-tuple in
 *     any case). No match: no_socket.
 *   - Report: err_dev[l] = max(err_dev[l], ((uint64)(i + 1) << 8) | code) by a 64-bit atomic max,
 *     so the result does not depend on scheduling. The stage first clears err_dev[0, n_lanes) on
 *     the same stream; 0 means no error.
 * The uploaded snapshot must have lane_mask == 0xFFFFFFFF (a lane is a sockfd, as for the peer
 * filter). peer_dev is [n_lanes], 8-byte aligned; NULL means the context's sticky table from
 * udpdk_gpu_rx_peer (lanes past what it was given are off), -ENOENT when that stage is off.
 * -EINVAL with nothing enqueued: a NULL pointer (peer_dev excepted), peer_dev or err_dev not 8-byte
 * aligned, n_lanes outside 1..UDPDK_GPU_MAX_LANES, frames_bytes >= 2^32, no snapshot uploaded or one
 * in compat mode. n == 0 clears err_dev and returns 0. Asynchronous on the context stream; joins the
 * pipes as udpdk_gpu_icmp_reply does. The frames buffer keeps the tailroom contract of udpdk_gpu_rx.
 * meta is read and never written. The launches are not event-timed.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t errors;     /* type-3 messages to us past the frame gate                          */
    uint32_t msg_bad;    /* ... with a bad total length or ICMP checksum                       */
    uint32_t quote_bad;  /* ... whose quote is not an IHL-5, first-fragment IPv4/UDP header    */
    uint32_t soft;       /* ... with a code that is not a hard error                           */
    uint32_t no_socket;  /* hard errors that matched no connected socket                       */
    uint32_t reported;   /* (frame, socket) pairs reported                                     */
    uint32_t bad_frame;  /* candidate by meta, but length < 42 or out of range: not read       */
} udpdk_icmp_err_stats_t;

int udpdk_gpu_icmp_errors(udpdk_gpu_ctx *ctx, uint32_t our_ip, const udpdk_rx_batch_t *batch,
                          const uint32_t *meta_dev, const udpdk_peer_t *peer_dev, uint32_t n_lanes,
                          uint64_t *err_dev /* [n_lanes] */);
/* Of the last udpdk_gpu_icmp_errors on the context (-ENOENT when there was none). Synchronises. */
int udpdk_gpu_icmp_err_stats(udpdk_gpu_ctx *ctx, udpdk_icmp_err_stats_t *stats);
/* Poller internals: the same stage on pipe `pipe`'s stream (1 .. 3) with that pipe's workspace and
 * no joins, like udpdk_gpu_pipe_icmp_reply; the counts are copied to pinned memory on the same
 * stream. udpdk_gpu_pipe_icmp_err_stats reads them without synchronising: they are those of the
 * pipe's last stage once udpdk_gpu_pipe_wait has returned (-ENOENT: the pipe never ran one). */
int udpdk_gpu_pipe_icmp_errors(udpdk_gpu_ctx *ctx, int pipe, uint32_t our_ip,
                               const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                               const udpdk_peer_t *peer_dev, uint32_t n_lanes, uint64_t *err_dev);
int udpdk_gpu_pipe_icmp_err_stats(udpdk_gpu_ctx *ctx, int pipe, udpdk_icmp_err_stats_t *stats);
/* The errno of destination-unreachable code `code` (0: none, codes above 15) and, when hard is not
 * NULL, whether the error is hard (1) or soft (0). Host only. */
int udpdk_gpu_icmp_errno(uint32_t code, int *hard);

/* ---------------------------------------------------------------------------------------------
 * ARP on the device: answers to who-has requests for the stack's own address (RFC 826). The
 * reference has no ARP (its .ini carries the peer's MAC by hand): a request ends as
 * UDPDK_V_NOT_IPV4 and nothing looks at it again, so no on-link host can learn our MAC. This optional
 * stage after udpdk_gpu_rx answers from what is already in device memory (the verdict words, the
 * staged frames). Parity is against RFC 826 and RFC 5227. Off unless called.
 *
 * All addresses are raw. The first failing step decides the single counter a frame lands in.
 *   1. Candidate by meta: verdict UDPDK_V_NOT_IPV4. For any other frame no descriptor and no frame
 *      byte is read, so a batch of IPv4 costs the read of meta.
 *   2. Frame gate: length[i] >= 42 and offset[i] + length[i] <= frames_bytes (64 bits), else the
 *      candidate counts as bad_frame and no frame byte is read (meta need not come from this batch).
 *   3. Bytes 12-13 == 08 06, else the frame is counted nowhere (IPv6, LLDP, ...). Then arp++.
 *   4. Bytes 14-19 == 00 01 08 00 06 04 (Ethernet, IPv4, lengths 6 and 4), else malformed.
 *   5. Bytes 20-21 == 00 01 (request), else other_op.
 *   6. Sender hardware address, bytes 22-27: equal to cfg->src_mac: own; byte 22 odd (the group
 *      bit) or all six bytes zero: sender_bad.
 *   7. Target address, bytes 38-41, == cfg->src_ip, else not_ours.
 *   8. Sender address, bytes 28-31, == cfg->src_ip: conflict, not answered (defending an address,
 *      RFC 5227 §2.4, is out of scope; the counter lets an operator see it). A sender address of
 *      0.0.0.0, an RFC 5227 probe, is answered.
 *   9. Eligible. Frames longer than 42 bytes (Ethernet padding to 60) are accepted and bytes past
 *      41 ignored. The Ethernet destination, bytes 0-5, is not looked at, as in Linux.
 *
 * Reply r is the r-th eligible request in arrival order. It is written iff r < max_replies, with
 * origin[r] the request's frame index, into the UDPDK_ARP_SLOT_BYTES slot at 64 r:
 *   bytes 0-5    request bytes 22-27 (unicast to the asker)
 *         6-11   cfg->src_mac
 *         12-21  08 06 00 01 08 00 06 04 00 02
 *         22-27  cfg->src_mac
 *         28-31  cfg->src_ip
 *         32-37  request bytes 22-27
 *         38-41  request bytes 28-31
 *         42-63  zero (a caller that wants a minimum-size Ethernet frame sends 60)
 * Slots and origin entries of index >= replies are not written; the requests cut are a tail
 * (no_room). cfg->dst_mac is not used.
 *
 * Asynchronous on the context stream; joins the pipes as udpdk_gpu_icmp_reply does. -EINVAL with
 * nothing enqueued: a NULL pointer, cfg->src_ip == 0, frames_bytes >= 2^32, out->frames_dev not
 * 16-byte aligned, an output that overlaps the frame buffer. n == 0 returns 0 with all counts zero.
 * The frames buffer keeps the tailroom contract of udpdk_gpu_rx. meta and frames are read and never
 * written. No snapshot is needed. The launch is not event-timed. One launch: its last workgroup to
 * finish writes the replies, in time proportional to min(eligible, max_replies).
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_ARP_FRAME_BYTES 42u   /* 14 Ethernet + 28 ARP; what is queued and sent            */
#define UDPDK_ARP_SLOT_BYTES  64u   /* device output stride: the frame, then 22 zero bytes      */

typedef struct {
    uint8_t  *frames_dev;    /* [max_replies * 64], 16-byte aligned; reply r at 64 * r          */
    uint32_t *origin_dev;    /* [max_replies] index of the request reply r answers              */
    uint32_t  max_replies;
} udpdk_arp_out_t;

typedef struct {
    uint32_t arp;         /* candidates past the frame gate with ethertype 0x0806               */
    uint32_t malformed;   /* ... whose bytes 14-19 are not 00 01 08 00 06 04                    */
    uint32_t other_op;    /* ... with an opcode other than 1 (replies to others, RARP, ...)     */
    uint32_t own;         /* ... whose sender MAC is cfg->src_mac (our own frames coming back)  */
    uint32_t sender_bad;  /* ... whose sender MAC has the group bit set or is all zero          */
    uint32_t not_ours;    /* ... asking for another address                                     */
    uint32_t conflict;    /* ... asking for ours while claiming it as sender (spa == our ip)    */
    uint32_t eligible;    /* requests to answer                                                 */
    uint32_t replies;     /* written: min(eligible, max_replies)                                */
    uint32_t no_room;     /* eligible - replies (a tail in arrival order)                       */
    uint32_t bad_frame;   /* candidate by meta, but length < 42 or out of range: not read       */
} udpdk_arp_stats_t;

int udpdk_gpu_arp_reply(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                        const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                        const udpdk_arp_out_t *out);
/* Of the last udpdk_gpu_arp_reply on the context (-ENOENT when there was none). Synchronises.
 * -ENOSPC when no_room > 0. */
int udpdk_gpu_arp_stats(udpdk_gpu_ctx *ctx, udpdk_arp_stats_t *stats);
/* Frames per workgroup of the kernel and the workgroup count for n frames (host only, like
 * udpdk_gpu_icmp_geometry). */
int udpdk_gpu_arp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks);
/* Poller internals: the same stage on pipe `pipe`'s stream (1 .. 3) with that pipe's workspace and
 * no joins, like udpdk_gpu_pipe_icmp_reply; the counts are copied to pinned memory on the same
 * stream. udpdk_gpu_pipe_arp_stats reads them without synchronising: they are those of the pipe's
 * last stage once udpdk_gpu_pipe_wait has returned (-ENOENT: the pipe never ran one; -ENOSPC as above). */
int udpdk_gpu_pipe_arp_reply(udpdk_gpu_ctx *ctx, int pipe, const udpdk_tx_config_t *cfg,
                             const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                             const udpdk_arp_out_t *out);
int udpdk_gpu_pipe_arp_stats(udpdk_gpu_ctx *ctx, int pipe, udpdk_arp_stats_t *stats);

/* ---------------------------------------------------------------------------------------------
 * IGMPv2 on the device: membership reports in answer to membership queries (RFC 2236), so that a
 * switch with IGMP snooping or a multicast router keeps forwarding the groups the stack joined. The
 * reference has no IGMP: a query ends as UDPDK_V_NOT_UDP and nothing looks at it again. This optional
 * stage after udpdk_gpu_rx answers from what is already in device memory (the verdict words, the
 * staged frames) and the caller's list of joined groups. Off unless called.
 *
 * All addresses are raw. groups_dev[n_groups] holds distinct group addresses in the caller's order,
 * n_groups <= UDPDK_IGMP_MAX_GROUPS. The first failing step decides the single counter a frame
 * lands in.
 *   1. Candidate by meta: verdict UDPDK_V_NOT_UDP. For any other frame no descriptor and no frame
 *      byte is read, so a batch of UDP costs the read of meta.
 *   2. Frame gate: length[i] >= 34 and offset[i] + length[i] <= frames_bytes (64 bits), else the
 *      candidate counts as bad_frame and no frame byte is read.
 *   3. Byte 23 == 2 (IGMP), else the frame is counted nowhere (ICMP, TCP, ...). Then igmp++.
 *   4. IHL = the low nibble of byte 14, 5..15; the IPv4 total length (bytes 16-17) >= 4 IHL + 8;
 *      14 + total length <= length[i]; the header checksum over all 4 IHL bytes verifies (the verdict
 *      word's IP bit covers 20 bytes only, and a query carries Router Alert: IHL 6). Else malformed.
 *   5. The IGMP message is the total length - 4 IHL bytes at 14 + 4 IHL: 8 (v1, v2), 12 or more
 *      (v3), at most what the 16-bit total length allows. Its RFC 1071 checksum over the whole
 *      message verifies, an odd length padded with a zero byte. Else bad_cksum.
 *   6. The type, message byte 0, == 0x11 (membership query), else other_type: the reports and
 *      leaves of others (0x12, 0x16, 0x17, 0x22) and anything else.
 *   7. The group, message bytes 4-7. Zero: a general query, whose destination (bytes 30-33) must be
 *      224.0.0.1, else bad_dst; then general. Non-zero: a group-specific query, whose destination
 *      must equal the group, else bad_dst; a group that is not in groups_dev: not_member; then
 *      specific.
 *   8. The max response time is ignored: the answer leaves with the caller's next transmission,
 *      inside any response window; there is no random delay and no suppression on hearing another
 *      member's report. A v1 or v3 query is answered as a v2 query (RFC 2236 section 2.5).
 *
 * The answer set is a bitmap over groups_dev: a general query sets every group except 224.0.0.1, a
 * specific query its own group. Report r is for the r-th set group in index order, so each group
 * gets at most one report per call however many queries ask for it. It is written iff
 * r < max_reports, with group_index[r] the group's index in groups_dev, into the
 * UDPDK_IGMP_SLOT_BYTES slot at 64 r (g = the group's four address bytes):
 *   bytes 0-5    01 00 5e, g[1] & 0x7f, g[2], g[3]
 *         6-11   cfg->src_mac
 *         12-13  08 00
 *         14-37  46 c0 00 20 00 00 40 00 01 02 <checksum> <cfg->src_ip> <g> 94 04 00 00
 *         38-45  16 00 <checksum> <g>
 *         46-63  zero
 * Slots and index entries of r >= reports are not written; the groups cut are a tail (no_room).
 * cfg->dst_mac is not used.
 *
 * Asynchronous on the context stream; joins the pipes as udpdk_gpu_arp_reply does. -EINVAL with
 * nothing enqueued: a NULL pointer (groups_dev may be NULL when n_groups == 0), cfg->src_ip == 0,
 * n_groups > UDPDK_IGMP_MAX_GROUPS, frames_bytes >= 2^32, out->frames_dev not 16-byte aligned, an
 * output that overlaps the frame buffer. n == 0 returns 0 with all counts zero. The frames buffer
 * keeps the tailroom contract of udpdk_gpu_rx. meta, frames and groups are read and never written. No
 * snapshot is needed. The launch is not event-timed. One launch: its last workgroup to finish
 * writes the reports.
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_IGMP_FRAME_BYTES 46u  /* 14 Ethernet + 24 IPv4 with Router Alert + 8 IGMP         */
#define UDPDK_IGMP_SLOT_BYTES  64u  /* device output stride: the frame, then 18 zero bytes      */
#define UDPDK_IGMP_MAX_GROUPS  4096u

typedef struct {
    uint8_t  *frames_dev;       /* [max_reports * 64], 16-byte aligned; report r at 64 * r      */
    uint32_t *group_index_dev;  /* [max_reports] index in groups_dev of the group of report r   */
    uint32_t  max_reports;
} udpdk_igmp_out_t;

typedef struct {
    uint32_t igmp;        /* candidates past the frame gate with protocol 2                     */
    uint32_t malformed;   /* ... whose IHL, total length or header checksum is wrong            */
    uint32_t bad_cksum;   /* ... whose IGMP checksum fails                                      */
    uint32_t other_type;  /* ... of a type other than 0x11                                      */
    uint32_t bad_dst;     /* queries sent to an address that does not go with their group field */
    uint32_t general;     /* general queries answered                                           */
    uint32_t not_member;  /* group-specific queries for a group that is not in groups_dev       */
    uint32_t specific;    /* group-specific queries answered                                    */
    uint32_t reports;     /* written: min(groups to report, max_reports)                        */
    uint32_t no_room;     /* groups to report - reports (a tail in index order)                 */
    uint32_t bad_frame;   /* candidate by meta, but length < 34 or out of range: not read       */
} udpdk_igmp_stats_t;

int udpdk_gpu_igmp_reply(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg,
                         const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                         const uint32_t *groups_dev, uint32_t n_groups, const udpdk_igmp_out_t *out);
/* Of the last udpdk_gpu_igmp_reply on the context (-ENOENT when there was none). Synchronises.
 * -ENOSPC when no_room > 0. */
int udpdk_gpu_igmp_stats(udpdk_gpu_ctx *ctx, udpdk_igmp_stats_t *stats);
/* Frames per workgroup of the kernel and the workgroup count for n frames (host only, like
 * udpdk_gpu_arp_geometry). */
int udpdk_gpu_igmp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks);
/* Poller internals: the same stage on pipe `pipe`'s stream (1 .. 3) with that pipe's workspace and
 * no joins, like udpdk_gpu_pipe_arp_reply; the counts are copied to pinned memory on the same
 * stream. udpdk_gpu_pipe_igmp_stats reads them without synchronising: they are those of the pipe's
 * last stage once udpdk_gpu_pipe_wait has returned (-ENOENT: the pipe never ran one; -ENOSPC as above). */
int udpdk_gpu_pipe_igmp_reply(udpdk_gpu_ctx *ctx, int pipe, const udpdk_tx_config_t *cfg,
                              const udpdk_rx_batch_t *batch, const uint32_t *meta_dev,
                              const uint32_t *groups_dev, uint32_t n_groups, const udpdk_igmp_out_t *out);
int udpdk_gpu_pipe_igmp_stats(udpdk_gpu_ctx *ctx, int pipe, udpdk_igmp_stats_t *stats);

/* ---------------------------------------------------------------------------------------------
 * Neighbour cache on the device: a table of on-link IPv4 addresses and their MACs, learned from the
 * ARP the stack receives (udpdk_gpu_neigh_learn, after udpdk_gpu_rx) and read per datagram before
 * udpdk_gpu_tx_build_neigh (udpdk_gpu_neigh_resolve), which also writes the who-has requests for
 * what it does not know. The reference has none: every frame goes to the one MAC of its .ini. Off
 * unless called. All addresses are raw.
 *
 * The table: open addressing keyed by the address, 16-byte entries, a power of two of them in
 * 8 .. UDPDK_NEIGH_MAX_ENTRIES. Key 0 is an empty slot (0.0.0.0 is never a neighbour). Kernels never
 * delete: an entry only changes state in place, so a key, once claimed, stays where it is. Probing is
 * linear over the whole table from the key's home slot, (key * 0x9E3779B1 mod 2^32) >> (32 - log2
 * entries), so an insert fails only when no slot is empty. Time is the caller's `now` in milliseconds;
 * ages are now - stamp in uint32 arithmetic (wrap-safe); nothing reads a clock. The table has ONE
 * writer at a time: learn, resolve, set and flush are ordered by the caller (the stream forms are
 * ordered by their stream, and join the pipes as udpdk_gpu_tx_build does). Its contents as a map
 * (address -> MAC, state, stamp) are fully determined by the calls; its layout is not, with one
 * exception: when one call brings more new keys than there are empty slots, which of them got in is
 * unspecified (how many is specified).
 *
 * Learning (udpdk_gpu_neigh_learn). Candidates and the frame gate are those of udpdk_gpu_arp_reply,
 * steps 1-4 (verdict UDPDK_V_NOT_IPV4; length >= 42 and in range, else bad_frame; bytes 12-13 08 06,
 * then arp++; bytes 14-19 00 01 08 00 06 04, else malformed). Then:
 *   5. Opcode, bytes 20-21, 1 or 2, else other_op.
 *   6. sender_bad: the sender MAC, bytes 22-27, is cfg->src_mac, has the group bit or is all zero;
 *      or the sender address, bytes 28-31, is 0.0.0.0, cfg->src_ip, 255.255.255.255 or in 224/4.
 *   7. The table has an entry for the sender address: a STATIC one is never touched (static_kept);
 *      any other becomes REACHABLE with the sender's MAC and stamp = now, counted updated when its
 *      MAC or state changed and refreshed otherwise.
 *   8. No entry, and the frame is a request (opcode 1) whose target address, bytes 38-41, is
 *      cfg->src_ip: a REACHABLE entry is created (created), or there is no empty slot (full).
 *   9. Otherwise nothing is learned (ignored): replies and gratuitous ARP about addresses the stack
 *      never asked for, requests for others. This is Linux with arp_accept = 0 (RFC 826 would create
 *      from any packet addressed to us). A solicited reply finds the INCOMPLETE entry resolve left.
 * Frames are taken in frame order: the last frame of an address wins, and every count is taken
 * against the table as the frames before it left it. meta and frames are read and never written.
 * Asynchronous; -EINVAL with nothing enqueued: a NULL pointer, no table, cfg->src_ip == 0, unknown
 * flag bits, frames_bytes >= 2^32. n == 0 returns 0 with all counts zero. One launch of
 * arp_reply's shape; its last workgroup to finish applies the events, one workgroup's width at a time,
 * so a batch without ARP costs the read of meta.
 *
 * Resolution (udpdk_gpu_neigh_resolve) of datagram i from dst_ip[i] and sockfd[i]; a negative sockfd
 * passes through (skipped, MAC zero). In order:
 *   R1. dst = 255.255.255.255, or netmask != 0 and dst on-link with all host bits one:
 *       ff:ff:ff:ff:ff:ff (bcast).
 *   R2. dst in 224/4: 01:00:5e + the low 23 bits of dst (mcast).
 *   R3. The next hop h = dst when (dst ^ src_ip) & netmask == 0 (netmask 0: everything is on-link),
 *       else gateway. h == 0 (off-link without a gateway): no_route, sockfd_out = -1, no request.
 *   R4. h == src_ip: src_mac (self).
 *   R5. The entry of h: STATIC, or REACHABLE with now - stamp <= ttl_ms: its MAC (hit). REACHABLE and
 *       older: it becomes INCOMPLETE with stamp = now (expired; a miss that asks). INCOMPLETE
 *       (incomplete): a miss, which asks iff now - stamp >= retrans_ms, and then stamp = now
 *       (retrans_ms 0 is taken as 1: a next hop is asked at most once per call). None: an INCOMPLETE
 *       entry with stamp = now is inserted (inserted; a miss that asks), or no slot is empty
 *       (table_full; a miss that does not ask).
 *   A miss gets cfg->fallback_mac and keeps its sockfd with UDPDK_NEIGH_FALLBACK (fallback), else MAC
 *   zero and sockfd_out = -1 (unresolved): udpdk_gpu_tx_build_neigh writes nothing for it.
 * Datagrams are taken in index order: states and stamps afterwards and the requests are those of a
 * serial walk. state[i] is the UDPDK_NEIGH_C_* class. dmac[2 i], dmac[2 i + 1] hold the MAC in their
 * low 48 bits (bytes 0-3, then 4-5). Request r, for the r-th distinct asking next hop in the order of
 * the first datagram that asked (req_origin[r]), is written iff r < req_cap into the
 * UDPDK_ARP_SLOT_BYTES slot at 64 r:
 *   bytes 0-5 ff, 6-11 src_mac, 12-21 08 06 00 01 08 00 06 04 00 01, 22-27 src_mac, 28-31 src_ip,
 *   32-37 zero, 38-41 h, 42-63 zero.
 * The excess counts as no_room; stamps move for every asking next hop, whether its request fitted or
 * not. Nothing is written at or past the request count. dst_ip and sockfd are never written.
 * -EINVAL with nothing enqueued: a NULL pointer (req_dev and req_origin_dev may be NULL when req_cap
 * is 0), no table, src_ip == 0, unknown flag bits, dmac_dev not 8-byte or req_dev not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define UDPDK_NEIGH_MAX_ENTRIES 65536u
#define UDPDK_NEIGH_FALLBACK    1u      /* udpdk_neigh_cfg_t::flags: a miss goes to fallback_mac   */

enum udpdk_neigh_state {
    UDPDK_NEIGH_EMPTY = 0, UDPDK_NEIGH_INCOMPLETE = 1, UDPDK_NEIGH_REACHABLE = 2, UDPDK_NEIGH_STATIC = 3
};

/* the class of a datagram (udpdk_neigh_out_t::state_dev, udpdk_gpu_neigh_class) */
enum udpdk_neigh_class {
    UDPDK_NEIGH_C_SKIPPED = 0, UDPDK_NEIGH_C_BCAST = 1, UDPDK_NEIGH_C_MCAST = 2, UDPDK_NEIGH_C_NO_ROUTE = 3,
    UDPDK_NEIGH_C_SELF = 4,
    UDPDK_NEIGH_C_LOOKUP = 5,           /* udpdk_gpu_neigh_class only: rule R5 decides             */
    UDPDK_NEIGH_C_HIT = 5, UDPDK_NEIGH_C_EXPIRED = 6, UDPDK_NEIGH_C_INCOMPLETE = 7, UDPDK_NEIGH_C_INSERTED = 8,
    UDPDK_NEIGH_C_TABLE_FULL = 9
};

typedef struct {
    uint32_t ip;          /* raw; 0: an empty slot                                                  */
    uint8_t  mac[6];
    uint8_t  state;       /* enum udpdk_neigh_state                                                 */
    uint8_t  pad;
    uint32_t stamp;       /* ms: when it was learned (REACHABLE) or last asked for (INCOMPLETE)     */
} udpdk_neigh_entry_t;

typedef struct {
    uint32_t src_ip, netmask, gateway;   /* raw; netmask 0: all on-link; gateway 0: none           */
    uint8_t  src_mac[6];
    uint8_t  fallback_mac[6];
    uint32_t ttl_ms;                     /* a REACHABLE entry is used while now - stamp <= ttl_ms   */
    uint32_t retrans_ms;                 /* an INCOMPLETE one is asked for again after this long    */
    uint32_t flags;                      /* UDPDK_NEIGH_FALLBACK                                    */
} udpdk_neigh_cfg_t;

typedef struct {
    uint32_t arp, malformed, bad_frame;  /* as in udpdk_arp_stats_t                                 */
    uint32_t other_op;                   /* an opcode other than 1 and 2                            */
    uint32_t sender_bad, updated, refreshed, static_kept, created, full, ignored;   /* steps 6-9   */
} udpdk_neigh_learn_stats_t;

typedef struct {
    uint32_t *dmac_dev;        /* [2 n], 8-byte aligned                                             */
    int32_t  *sockfd_out_dev;  /* [n]                                                               */
    uint8_t  *state_dev;       /* [n] enum udpdk_neigh_class                                        */
    uint8_t  *req_dev;         /* [req_cap * 64], 16-byte aligned                                   */
    uint32_t *req_origin_dev;  /* [req_cap]                                                         */
    uint32_t  req_cap;
} udpdk_neigh_out_t;

typedef struct {
    uint32_t skipped, bcast, mcast, no_route, self, hit;          /* one per datagram, with ...     */
    uint32_t expired, incomplete, inserted, table_full;           /* ... these, the misses          */
    uint32_t fallback, unresolved;                                /* what became of the misses      */
    uint32_t requests, no_room;                                   /* written, and cut               */
} udpdk_neigh_resolve_stats_t;

/* Allocates and clears a table of `entries`, replacing an existing one (freed with the context).
 * Synchronises. -EINVAL: entries not a power of two in 8 .. UDPDK_NEIGH_MAX_ENTRIES. */
int udpdk_gpu_neigh_create(udpdk_gpu_ctx *ctx, uint32_t entries);
/* Inserts or overwrites n entries (STATIC or REACHABLE, ip != 0) from the host. Synchronous.
 * -ENOSPC when the table is full: the entries before the one that did not fit are in. */
int udpdk_gpu_neigh_set(udpdk_gpu_ctx *ctx, const udpdk_neigh_entry_t *entries_host, uint32_t n);
/* The non-empty entries, up to cap of them, in the table's order (callers sort); *n gets their
 * number (-ENOSPC when it is above cap). Synchronous. */
int udpdk_gpu_neigh_dump(udpdk_gpu_ctx *ctx, udpdk_neigh_entry_t *out_host, uint32_t cap, uint32_t *n);
/* Clears the table; keep_static != 0 keeps the STATIC entries. Synchronous. */
int udpdk_gpu_neigh_flush(udpdk_gpu_ctx *ctx, int keep_static);
int udpdk_gpu_neigh_learn(udpdk_gpu_ctx *ctx, const udpdk_neigh_cfg_t *cfg, const udpdk_rx_batch_t *batch,
                          const uint32_t *meta_dev, uint32_t now);
/* Of the last udpdk_gpu_neigh_learn on the context (-ENOENT when there was none). Synchronises. */
int udpdk_gpu_neigh_learn_stats(udpdk_gpu_ctx *ctx, udpdk_neigh_learn_stats_t *stats);
/* Poller internals: the same stage on pipe `pipe`'s stream (1 .. 3), as udpdk_gpu_pipe_arp_reply is. */
int udpdk_gpu_pipe_neigh_learn(udpdk_gpu_ctx *ctx, int pipe, const udpdk_neigh_cfg_t *cfg,
                               const udpdk_rx_batch_t *batch, const uint32_t *meta_dev, uint32_t now);
int udpdk_gpu_pipe_neigh_learn_stats(udpdk_gpu_ctx *ctx, int pipe, udpdk_neigh_learn_stats_t *stats);
int udpdk_gpu_neigh_resolve(udpdk_gpu_ctx *ctx, const udpdk_neigh_cfg_t *cfg, const uint32_t *dst_ip_dev,
                            const int32_t *sockfd_dev, uint32_t n, uint32_t now, const udpdk_neigh_out_t *out);
/* Of the last udpdk_gpu_neigh_resolve (-ENOENT when there was none; -ENOSPC when no_room > 0).
 * Synchronises. */
int udpdk_gpu_neigh_resolve_stats(udpdk_gpu_ctx *ctx, udpdk_neigh_resolve_stats_t *stats);
/* Frames per workgroup of the learn kernel and datagrams per workgroup of the resolve kernel (host
 * only, like udpdk_gpu_arp_geometry). */
int udpdk_gpu_neigh_geometry(uint32_t *learn_frames_per_block, uint32_t *resolve_per_block);
/* Rules R1-R4 on the host, the statement the kernel compiles too: returns the class of dst_ip
 * (UDPDK_NEIGH_C_BCAST, _MCAST, _NO_ROUTE, _SELF or _LOOKUP), with *next_hop (0 where the class has
 * none) and, for bcast, mcast and self, the MAC in mac_out[6] (zero otherwise). -EINVAL: a NULL pointer. */
int udpdk_gpu_neigh_class(const udpdk_neigh_cfg_t *cfg, uint32_t dst_ip, uint32_t *next_hop, uint8_t *mac_out);
/* udpdk_gpu_tx_build_flags with bytes 0-5 of every frame (every fragment) of datagram i taken from
 * dmac_dev[2 i], dmac_dev[2 i + 1] (udpdk_neigh_out_t::dmac_dev) instead of cfg->dst_mac; every other
 * byte is the same. dmac_dev == NULL is udpdk_gpu_tx_build_flags exactly. */
int udpdk_gpu_tx_build_neigh(udpdk_gpu_ctx *ctx, const udpdk_tx_config_t *cfg, const udpdk_tx_batch_t *batch,
                             const udpdk_tx_out_t *out, uint32_t mtu, uint32_t flags, const uint32_t *dmac_dev);

/* ---------------------------------------------------------------------------------------------
 * Timing (for bench.py / the roofline): on every `enable`-th udpdk_gpu_rx call (0 = off, 1 =
 * every call) each kernel is launched with start/stop events carried by its own dispatch
 * (hipExtLaunchKernelGGL), so no marker packet separates back-to-back kernels; sampling keeps the
 * host cost of the events (~10 us per timed call) off most calls. Read back the accumulated
 * device milliseconds and the number of timed launches per kernel id.
 * ------------------------------------------------------------------------------------------- */
enum udpdk_gpu_kernel_id {
    UDPDK_K_RX_CLASSIFY = 0,   /* parse + checksums + demux + tile histograms (dominant)      */
    UDPDK_K_RX_SCAN     = 1,   /* lane offsets (one or three launches)                         */
    UDPDK_K_RX_SCATTER  = 2,   /* stable per-lane compaction (rx_scatter, or rx_compact1)      */
    UDPDK_K_TX_BUILD    = 3,
    UDPDK_K_RX_GATHER   = 4,   /* payload delivery (udpdk_gpu_rx_gather)                       */
    UDPDK_N_KERNEL_IDS  = 5
};
int udpdk_gpu_timing_enable(udpdk_gpu_ctx *ctx, int enable);
/* Synchronises; ms[k] = accumulated device ms, launches[k] = number of timed calls. Resets. */
int udpdk_gpu_timing_read(udpdk_gpu_ctx *ctx, double ms[UDPDK_N_KERNEL_IDS],
                          uint32_t launches[UDPDK_N_KERNEL_IDS]);

/* Tile geometry the RX pipeline will use for (n, n_lanes): frames per tile and tile count. */
int udpdk_gpu_rx_geometry(uint32_t n, uint32_t n_lanes, uint32_t *tile_frames,
                          uint32_t *n_tiles);

#ifdef __cplusplus
}
#endif

#endif /* UDPDK_GPU_H */
