/*
 * udpdk_api.h — POSIX-like UDP socket surface, source compatible with the reference's
 * udpdk/udpdk_api.h:19-41 (same ten functions, same argument meaning, -1 + errno on error) plus
 * udpdk_dump_payload (udpdk_api.symlist:11). Applications written against the reference
 * (apps/pktgen, apps/pingpong) compile against this header and link against libudpdk_amd.so
 * unchanged (tests/test_ref_apps.py builds both from /root/reference in place).
 *
 * What changed underneath: there is no forked DPDK poller. The per-packet RX work of
 * udpdk_poller.c runs as HIP kernels on an MI355X through udpdk_gpu.h; udpdk_init() creates the
 * GPU context (and fails with ENODEV when no GPU is present), and frame batches enter through
 * udpdk_poll_rx() (the replacement of poller.c:516-545's rte_eth_rx_burst loop). Datagrams queued
 * by udpdk_sendto() leave as frames built on the GPU through udpdk_tx_drain() (the replacement of
 * the poller's TX half, poller.c:453-514). A poller thread can drive both against a port
 * (udpdk_port_attach), as the reference's forked poller drives NIC port 0.
 *
 * Extensions below the reference surface are prefixed udpdk_ too and documented in
 * INTEGRATION.md.
 */
#ifndef UDPDK_API_H
#define UDPDK_API_H

/* What the reference header supplied to applications transitively through udpdk_types.h:19-23
 * (apps/pktgen/main.c:54-58 uses bool without including <stdbool.h> itself). */
#include <netinet/in.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>

#include "udpdk_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference surface (udpdk_api.h:19-41) ------------------------------------------------ */

/* Parse "-c <file.ini>" (keys [port0] mac_addr / ip_addr, [port0_dst] mac_addr as in
 * udpdk_args.c:21-49; optional [gpu] device / devices / max_frames / max_lanes / port ...,
 * INTEGRATION.md) and create the GPU context(s). Returns 0, or -1 with errno. */
int udpdk_init(int argc, char *argv[]);

/* Make blocking calls (udpdk_recvfrom) return -1/EINTR (udpdk_init.c:374-378). */
void udpdk_interrupt(int signum);

/* Close every socket, free all queues and the GPU context (udpdk_init.c:392-424). */
void udpdk_cleanup(void);

int udpdk_socket(int domain, int type, int protocol);

int udpdk_getsockopt(int sockfd, int level, int optname, void *optval, socklen_t *optlen);

int udpdk_setsockopt(int sockfd, int level, int optname, const void *optval, socklen_t optlen);

int udpdk_bind(int s, const struct sockaddr *addr, socklen_t addrlen);

ssize_t udpdk_sendto(int sockfd, const void *buf, size_t len, int flags,
                     const struct sockaddr *dest_addr, socklen_t addrlen);

/* One reading thread per socket at a time: the socket's receive ring is single-consumer, like
 * the reference's SP/SC rx_q (udpdk_init.c:270-272). */
ssize_t udpdk_recvfrom(int s, void *buf, size_t len, int flags,
                       struct sockaddr *src_addr, socklen_t *addrlen);

int udpdk_close(int s);

void udpdk_dump_payload(const char *payload, int len);

/* ---- extensions ----------------------------------------------------------------------------- */

/* Sockets: NUM_SOCKETS_MAX is 1024 in the reference (udpdk_constants.h:12); widened here
 * (SURVEY.md §8 Q11). Per-socket RX ring: EXCH_RING_SIZE entries (udpdk_constants.h:49). */
#define UDPDK_MAX_SOCKETS  4096
#define UDPDK_RX_RING_SIZE 2048

/* RX entry point of the GPU poller (one turn of poller_body's RX half, udpdk_poller.c:516-545):
 * classify a batch of received frames (host memory, as they come off the NIC) on the GPU,
 * reassemble IPv4 fragments on the device, gather every accepted datagram's payload on the GPU
 * into pinned host slabs and append it to its socket's RX ring in arrival order. A socket's
 * deliveries are admitted per burst of BURST_SIZE = 128 frames (frame index / 128), each burst
 * all-or-nothing like the rte_ring_enqueue_bulk of flush_rx_queue (poller.c:274-292): a burst
 * whose datagrams do not fit the ring is dropped, later bursts may still fit. Reassembled
 * datagrams count at the index of the fragment that completed them. Safe to call from a poller
 * thread while application threads call the socket functions. stats may be NULL. Returns 0 or
 * -1 with errno. A batch polled in one piece publishes nothing when it fails; a large batch of
 * long frames polled in chunks ([gpu] poll_chunk_mb) may fail after its first chunks' bursts were
 * published (each chunk's bursts go to the rings before the next chunk is admitted, as the
 * reference's burst loop publishes each burst): a caller that retries such a batch receives those
 * datagrams twice, so retry only what the rings did not get, or poll with poll_chunk_mb = 0. */
int udpdk_poll_rx(const uint8_t *frames, uint64_t frames_bytes, const uint32_t *offset,
                  const uint16_t *length, const uint32_t *ptype, uint32_t n,
                  udpdk_rx_stats_t *stats);

/* Deliveries udpdk_poll_rx dropped because the pinned payload slabs ([gpu] slab_bytes_max /
 * slab_count_max, default 4 GiB / 1024 slabs) were all held by datagrams not yet received: the
 * reference's mbuf pool exhausted. */
uint64_t udpdk_rx_nobufs(void);

/* TX exit point (the poller's TX half, udpdk_poller.c:453-514): take queued datagrams in the
 * poller's order (sockets in index order, each drained while the burst holds fewer than
 * BURST_SIZE frames), build their frames on the GPU (header build, rte_ipv4_cksum, payload copy,
 * and the IPv4 fragmentation of frames longer than the MTU, udpdk_gpu_tx_build_mtu) and copy
 * them into out, back to back (out_off/out_len per frame; a datagram's fragments are
 * consecutive frames and never split across calls). At most max frames and out_cap bytes.
 * *n_out = frames written. Needs the GPU context (udpdk_init). Returns 0 or -1 with errno. */
int udpdk_tx_drain(uint8_t *out, uint64_t out_cap, uint32_t *out_off, uint16_t *out_len,
                   uint32_t max, uint32_t *n_out);

/* One poller turn that answers instead of delivering: the server side of apps/pingpong (recvfrom,
 * then sendto back to the source) for a whole batch, on the device. The frames (as for
 * udpdk_poll_rx) are classified on the GPU and every delivery is answered by its own socket with
 * its own payload, built straight from the received frame's bytes (udpdk_gpu_tx_reply): source
 * address and port are the socket's binding (the configured IP for an ANY binding), destination
 * the datagram's source, MTU and UDP checksum as udpdk_tx_drain builds them, and out / out_off /
 * out_len / *n_out are in udpdk_tx_drain's format (a datagram's fragments are consecutive frames),
 * replies in lane order: sockets in index order, each socket's datagrams in arrival order. A
 * delivery to several sockets (address reuse) is answered by each of them. [gpu] rx_drop applies as
 * in udpdk_poll_rx. The RX rings are not touched and nothing is queued for udpdk_tx_drain. FRAG
 * frames are counted in stats and not answered. If the replies need more than max frames or
 * out_cap bytes the call returns -1 with ENOBUFS and *n_out = 0, and may be repeated with more
 * room. Runs on the main context only. stats may be NULL. Returns 0 or -1 with errno (ENODEV
 * without a GPU context). */
int udpdk_poll_echo(const uint8_t *frames, uint64_t frames_bytes, const uint32_t *offset,
                    const uint16_t *length, const uint32_t *ptype, uint32_t n,
                    uint8_t *out, uint64_t out_cap, uint32_t *out_off, uint16_t *out_len,
                    uint32_t max, uint32_t *n_out, udpdk_rx_stats_t *stats);

/* Datagrams waiting in the TX rings, plus the ICMP and ARP frames queued for the next drain
 * (udpdk_config_icmp, udpdk_config_arp, udpdk_arp_announce). */
uint64_t udpdk_tx_pending(void);

/* Datagrams udpdk_tx_drain dropped because they needed more frames or bytes than a drain with
 * the caller's limits can ever carry (they would otherwise block their socket's ring). */
uint64_t udpdk_tx_dropped(void);

/* ---- the poller thread ----------------------------------------------------------------------
 * The reference forks a poller process that busy-polls NIC port 0 (udpdk_init.c:293-368,
 * poller.c:448-546). Here a port is a pair of callbacks; udpdk_port_attach starts a poller
 * thread that loops: udpdk_tx_drain -> tx_burst, rx_burst -> udpdk_poll_rx, until
 * udpdk_port_detach or udpdk_cleanup. Applications that do not attach a port drive
 * udpdk_poll_rx / udpdk_tx_drain themselves, from one thread (the poller role). */
typedef struct udpdk_port_ops {
    /* Write up to max received frames back to back into frames (cap bytes; keep
     * UDPDK_GPU_FRAMES_TAILROOM bytes of it free), offset[i] / length[i] per frame; return the
     * frame count (0: nothing now). */
    uint32_t (*rx_burst)(void *user, uint8_t *frames, uint64_t cap, uint32_t *offset,
                         uint16_t *length, uint32_t max);
    /* Transmit n frames; the callee copies what it keeps. */
    void (*tx_burst)(void *user, const uint8_t *frames, const uint32_t *offset,
                     const uint16_t *length, uint32_t n);
    void    *user;
    uint32_t batch_frames;   /* frames per RX batch (0: 4096)                                   */
} udpdk_port_ops_t;

int udpdk_port_attach(const udpdk_port_ops_t *ops);
int udpdk_port_detach(void);
/* A built-in loopback port: frames drained from TX come back on RX (tests and demos). */
int udpdk_port_loopback(udpdk_port_ops_t *ops);

/* Flatten the bind table into a snapshot in list order (valid until the next call or the next
 * bind/close). compat != 0 keys lanes by the reference's (uint8_t) slot (poller.c:294). */
int udpdk_btable_snapshot(udpdk_bind_snapshot_t *snap, int compat);

/* The GPU context created by udpdk_init (NULL before). */
udpdk_gpu_ctx *udpdk_gpu_context(void);

/* The devices polls run on: with "[gpu] devices = 0-7" (two or more entries) udpdk_init creates
 * one RX shard context per entry and udpdk_poll_rx splits every batch into that many contiguous
 * shards, each classified, demultiplexed and gathered on its own device by its own pool thread;
 * the shards' lanes are concatenated in shard order before ring admission, so the rings are those
 * of a single-context poll. Fragments go through the main context's reassembly table. Writes up
 * to max device ids and returns how many there are (1 without "devices", 0 before udpdk_init). */
int udpdk_shard_devices(int *devices, int max);

/* The same device list read from a config file without creating any context (no GPU needed):
 * what udpdk_init(-c cfg_path) would bind, in shard order. Returns the count (1 for a single
 * "[gpu] device"), -EINVAL for a malformed list, -ENOENT for a missing file. */
int udpdk_shard_plan(const char *cfg_path, int *devices, int max);

/* With "[gpu] dispatch = rss" (and two or more devices) a poll sends each frame to the shard of
 * its RSS queue instead: one RX queue per device, queue = reta[Toeplitz hash] with
 * udpdk_gpu_rss's hash definition, default key and redirection table (the NIC's ETH_MQ_RX_RSS
 * that udpdk_init.c:112-137 asks for and leaves as a TODO); the shards' lanes are merged back in
 * arrival order, so the rings are still a single-context poll's. Writes the number of frames
 * each shard took in the last poll (up to max) and returns the shard count (0 without shards). */
int udpdk_shard_frames(uint32_t *frames, int max);

/* TX header configuration (what udpdk_init reads from the .ini). Raw network-order IPv4. */
int udpdk_config_set(const uint8_t src_mac[6], const uint8_t dst_mac[6], uint32_t src_ip_raw);
int udpdk_config_get(uint8_t src_mac[6], uint8_t dst_mac[6], uint32_t *src_ip_raw);
/* IPv4 MTU of the TX fragmentation (default IPV4_MTU_DEFAULT = 1500; (mtu - 20) % 8 == 0). */
int udpdk_config_mtu(uint32_t mtu);
/* UDP checksum on sent datagrams (ini: [gpu] tx_udp_cksum = 0|1). 0 (default): the checksum
 * field is 0 as the reference sends it (udpdk_syscall.c:343); 1: udpdk_tx_drain builds every
 * datagram with its RFC 768 checksum (UDPDK_TX_UDP_CKSUM, udpdk_gpu.h), fragmented ones
 * included. One switch for the whole library, taking effect from the next drain. Returns the
 * setting in force before the call (0 or 1); a negative `on` only reads it; on > 1: -1, EINVAL. */
int udpdk_config_tx_cksum(int on);
/* Received deliveries that fail their checksums or lengths (ini: [gpu] rx_drop = none | all | a
 * comma list of ip, udp, len, ihl). flags: UDPDK_RX_DROP_* bits (udpdk_gpu.h). 0 (default): every
 * delivery reaches its socket, as the reference hands them on; otherwise udpdk_poll_rx takes the
 * deliveries with a selected failure out of the lanes on the GPU (udpdk_gpu_rx_drop) before ring
 * admission, datagrams reassembled from fragments included, and recvfrom never sees them (RFC 1122
 * §4.1.3.4). One setting for the whole library, applied to every context by the next poll. Returns
 * the flags in force before the call; a negative argument only reads them; a bit outside
 * UDPDK_RX_DROP_ALL: -1, EINVAL. */
int udpdk_config_rx_drop(int flags);
/* Deliveries removed that way, summed over polls (and their shards and chunks) of the library
 * session, like udpdk_rx_nobufs. */
uint64_t udpdk_rx_dropped(void);
/* Datagrams for several SO_REUSEPORT sockets (ini: [gpu] reuseport = fanout | balance).
 * UDPDK_REUSEPORT_FANOUT (default): every socket bound to the port with SO_REUSEADDR or
 * SO_REUSEPORT whose address matches gets a clone, as the reference delivers
 * (udpdk_poller.c:391-403). UDPDK_REUSEPORT_BALANCE: what that code's TODO asks for
 * (udpdk_poller.c:387-389): of the matching SO_REUSEPORT sockets exactly one gets a unicast
 * datagram, the same one for every datagram of a flow (the RSS 4-tuple hash scaled to the group,
 * as Linux's reuseport_select_sock ranks: udpdk_gpu_rx_balance, udpdk_gpu.h); SO_REUSEADDR-only
 * sockets, limited broadcast and multicast still fan out. udpdk_poll_rx balances on the GPU before
 * ring admission and payload gather (chunked and sharded polls, RSS dispatch and datagrams
 * reassembled from fragments included) and udpdk_poll_echo answers a balanced datagram once, from
 * the chosen socket. One setting for the whole library, applied to every context by the next
 * poll; the sockets' flags follow bind, close and setsockopt. Returns the mode in force before
 * the call; a negative argument only reads it; an unknown mode: -1, EINVAL. */
#define UDPDK_REUSEPORT_FANOUT  0
#define UDPDK_REUSEPORT_BALANCE 1
int udpdk_config_reuseport(int mode);
/* The clones removed that way, summed over the session like udpdk_rx_dropped (which does not
 * count them). */
uint64_t udpdk_rx_balanced(void);
/* The flags a balancing poll uploads: flags[s] = 1 when socket s is bound with SO_REUSEPORT set
 * (a socket that set only SO_REUSEADDR is not flagged, although the reference's overlapping option
 * values make getsockopt report SO_REUSEPORT for it), for s < n. Returns how many sockets are flagged (or -EINVAL). Host only, needs no GPU. */
int udpdk_reuseport_lanes(uint8_t *flags, uint32_t n);

/* Connected UDP sockets: what POSIX programs expect of connect / send / recv / getpeername /
 * getsockname and the reference's ten entry points do not have.
 * udpdk_connect fixes the socket's peer: afterwards udpdk_send (and udpdk_sendto with a NULL
 * dest_addr) sends to it, and the socket receives only datagrams whose source address and port are
 * the peer's. The others are removed on the GPU before ring admission and payload gather
 * (udpdk_gpu_rx_peer, udpdk_gpu.h), in one-piece, chunked and sharded polls, under dispatch = rss,
 * and for datagrams reassembled from fragments (whose frame carries the first fragment's header);
 * udpdk_poll_echo answers only the peer's datagrams from a connected socket. No ini key: connect
 * is the switch, and with no socket connected a poll enqueues what it always did.
 *   - ENOTSOCK / EBADF as udpdk_sendto gives them; EINVAL for a NULL addr or addrlen <
 *     sizeof(struct sockaddr_in) (AF_UNSPEC: < sizeof(sa_family_t)); EAFNOSUPPORT for a family other
 *     than AF_INET or AF_UNSPEC.
 *   - AF_UNSPEC dissolves the association; a second connect replaces the peer.
 *   - An unbound socket is auto-bound exactly as udpdk_sendto does it.
 *   - Datagrams already in the socket's ring stay there; the new peer applies from the next poll
 *     that starts after udpdk_connect returns.
 *   - With [gpu] reuseport = balance the flow hash may pick a group member that is connected to
 *     somebody else: that datagram is removed, not re-steered to another member.
 * udpdk_close and udpdk_host_reset clear the peer. */
int udpdk_connect(int s, const struct sockaddr *addr, socklen_t addrlen);
/* udpdk_sendto to the peer; ENOTCONN when the socket is not connected. (udpdk_sendto with a NULL
 * dest_addr sends to the peer of a connected socket and fails with EINVAL on an unconnected one;
 * with an address it sends to that address, connected or not.) */
ssize_t udpdk_send(int s, const void *buf, size_t len, int flags);
/* udpdk_recvfrom without the source address. */
ssize_t udpdk_recv(int s, void *buf, size_t len, int flags);
/* The peer as a sockaddr_in, truncated to *addrlen, which gets the length written; ENOTCONN when
 * the socket is not connected, EBADF / ENOTSOCK as above, EINVAL for a NULL argument. */
int udpdk_getpeername(int s, struct sockaddr *addr, socklen_t *addrlen);
/* The bound address and raw port the same way; 0.0.0.0:0 for an unbound socket. */
int udpdk_getsockname(int s, struct sockaddr *addr, socklen_t *addrlen);
/* Deliveries the peer filter removed, summed over the session like udpdk_rx_dropped (which does not
 * count them). */
uint64_t udpdk_rx_refused(void);
/* The records a poll uploads: peers[s] = socket s's peer (on = 1) or all zero, for s < n. Returns
 * how many sockets are connected (or -EINVAL). Host only, needs no GPU. */
int udpdk_peer_lanes(udpdk_peer_t *peers, uint32_t n);

/* ICMP answers (ini: [gpu] icmp = none | all | a comma list of echo, unreach). flags: UDPDK_ICMP_*
 * bits (udpdk_gpu.h). 0 (default): as in the reference, an echo request ends as NOT_UDP and a
 * datagram for a closed port is counted and forgotten. Otherwise udpdk_poll_rx, after a batch's RX
 * and before reassembly, builds the answers on the GPU from the staged batch (udpdk_gpu_icmp_reply
 * with the library's MACs, source address and MTU): an echo reply for every valid echo request to
 * our address (the host answers `ping`), an ICMP port-unreachable for every valid datagram to our
 * address that no socket is bound for (a client of a dead service gets ECONNREFUSED instead of a
 * timeout). The frames are queued on the host, at most 4096 of them (later ones are dropped and
 * counted), and udpdk_tx_drain emits them first, oldest first, in its usual format, the socket
 * datagrams after them; a frame that does not fit the drain's max or out_cap stays queued.
 * udpdk_tx_pending counts them. The one-piece and the chunked poll answer (a chunk on its pipe,
 * replies queued in chunk order); fragments (the FRAG verdict) and datagrams reassembled from them
 * are not answered, and neither is anything by udpdk_poll_echo. Sharded polls ([gpu] devices with
 * two or more entries) do not answer: there a nonzero flags gives -1 with ENOTSUP, and udpdk_init
 * fails on such an ini. With the loopback port the answers come back as ICMP types 0 and 3: nothing
 * answers them, and with udpdk_config_icmp_errors on a type 3 that quotes a connected socket's
 * datagram is reported to that socket (ECONNREFUSED). Returns the flags in force before the call; a
 * negative argument only reads them; a bit outside UDPDK_ICMP_ALL: -1, EINVAL. */
int udpdk_config_icmp(int flags);
/* Port-unreachable errors answered per poll (ini: [gpu] icmp_burst = N; default 64, a policy default
 * in the spirit of Linux's icmp_msgs_burst, not a measured value): the first N eligible datagrams
 * of a poll in arrival order, counted across the chunks of a chunked poll; the rest are counted as
 * limited. The limit is per poll, not per second: a poller that polls more often answers more. 0
 * answers none, -1 means no limit; echo replies are not limited. Returns the value in force before
 * the call; an argument below -1 only reads it. */
int udpdk_config_icmp_burst(int n);
/* Session sums over polls, like udpdk_rx_dropped: replies built (echo_replied, unreach_sent), echo
 * requests refused for a bad length, checksum or an MTU overrun (echo_bad), errors beyond the burst
 * (limited), and built frames the full queue dropped (queue_dropped). udpdk_host_reset zeroes them. */
typedef struct {
    uint64_t echo_replied, unreach_sent, echo_bad, limited, queue_dropped;
} udpdk_icmp_counts_t;
int udpdk_icmp_counts(udpdk_icmp_counts_t *counts);

/* ICMP errors received (ini: [gpu] icmp_errors = 0 | 1; default 0: a received ICMP error ends as
 * NOT_UDP and is forgotten, as in the reference). With 1, and while at least one socket is connected,
 * udpdk_poll_rx runs udpdk_gpu_icmp_errors (udpdk_gpu.h) after a batch's RX, next to the ICMP answers:
 * a destination-unreachable message to our address that quotes a datagram a connected socket sent to
 * its peer, with a hard code (udpdk_gpu_icmp_errno), becomes that socket's pending error, the last
 * one of a poll in arrival order (RFC 1122 §4.1.3.3; Linux's sk_err):
 *   - the next udpdk_recvfrom / udpdk_recv / udpdk_sendto / udpdk_send on the socket returns -1 with
 *     that errno (ECONNREFUSED for a port-unreachable) and clears it. Receive calls check it before
 *     the ring: datagrams already queued stay queued and the following call returns them. A
 *     udpdk_recvfrom waiting on an empty ring sees the error and returns.
 *   - udpdk_getsockopt(s, SOL_SOCKET, SO_ERROR, &int, &len) returns the value and clears it (0: none);
 *     udpdk_setsockopt of SO_ERROR stays ENOPROTOOPT.
 *   - udpdk_connect (a new peer, AF_UNSPEC), udpdk_close and udpdk_host_reset clear it.
 * The one-piece and the chunked poll report (a chunk on its pipe). Not looked at: ICMP that is itself
 * fragmented (the FRAG verdict) and reassembled datagrams, errors about fragments other than the
 * first, soft errors (counted, never reported: no IP_RECVERR, no path-MTU handling), anything in
 * udpdk_poll_echo. Sharded polls do not report: there on = 1 gives -1 with ENOTSUP and udpdk_init
 * fails on such an ini, as for udpdk_config_icmp. Returns the value in force before the call; a
 * negative argument only reads it; above 1: -1, EINVAL. */
int udpdk_config_icmp_errors(int on);
/* Poller internals (what the stage calls for every reported word; host only, needs no GPU): under
 * the socket lock, if s is in use, still connected to exactly peer_ip : peer_port (raw) and code is a
 * hard error, the socket's pending error becomes udpdk_gpu_icmp_errno(code), a later post
 * overwriting an earlier one, and the call returns 1; otherwise it changes nothing and returns 0
 * (a udpdk_connect between the poll's peer upload and the post wins). */
int udpdk_sock_error_post(int s, uint32_t peer_ip, uint16_t peer_port, uint32_t code);
/* Poller internals (host only, needs no GPU): queue one datagram on socket s's RX ring as a poll
 * would, from bytes the caller keeps alive until the datagram is received or the socket closed (no
 * slab is taken). For pollers that deliver from memory of their own and for tests of the receive
 * calls without a device. 0, or -1 with ENOTSOCK / EBADF / ENOBUFS (ring full). */
int udpdk_sock_rx_inject(int s, const void *data, uint32_t len, uint32_t src_ip, uint16_t src_port);
/* Session sums over polls, like udpdk_icmp_counts: the device stage's counts (udpdk_icmp_err_stats_t)
 * and posted, the posts that took effect. udpdk_host_reset zeroes them. */
typedef struct {
    uint64_t errors, msg_bad, quote_bad, soft, no_socket, reported, posted;
} udpdk_icmp_err_counts_t;
int udpdk_icmp_err_counts(udpdk_icmp_err_counts_t *counts);

/* ARP replies (ini: [gpu] arp = 0 | 1; default 0: as in the reference, a who-has request for our
 * address ends as NOT_IPV4 and is forgotten, so a peer needs a static neighbour entry for us). With 1,
 * udpdk_poll_rx runs udpdk_gpu_arp_reply (udpdk_gpu.h) on every staged batch whose RX counters show a
 * frame that is not IPv4, before the ICMP stage: every valid request for our address (the library's
 * source address, asked by a unicast sender that is not us and does not claim our address) is answered
 * with the library's MAC, unicast to the asker. A batch of pure IPv4 costs nothing. The replies, 42
 * bytes each in arrival order, go onto the host queue of the ICMP answers (at most 4096 frames; what a
 * full queue drops counts in udpdk_icmp_counts().queue_dropped, and requests beyond 4096 in one batch
 * as no_room), so udpdk_tx_drain emits a poll's ARP replies first, then its ICMP answers, then the
 * socket datagrams, and udpdk_tx_pending counts them. The one-piece and the chunked poll answer (a
 * chunk on its pipe, replies queued in chunk order); udpdk_poll_echo does not. Sharded polls do not
 * answer: there on = 1 gives -1 with ENOTSUP and udpdk_init fails on such an ini, as for
 * udpdk_config_icmp. With no source address configured nothing is answered. With the loopback port our
 * own replies come back as other_op and our announcement as own: nothing is answered twice. Not done:
 * defending our address, VLAN tags (the neighbour cache, requests and per-destination MACs are
 * udpdk_config_neigh's). Returns the value in force before
 * the call; a negative argument only reads it; above 1: -1, EINVAL. */
int udpdk_config_arp(int on);
/* Queue one RFC 5227 announcement of our address (a broadcast request with sender and target address
 * both ours, built on the host) for the next udpdk_tx_drain (ini: [gpu] arp_announce = 1 makes
 * udpdk_init call it once). Needs no GPU. 0, or -1 with EADDRNOTAVAIL (no source address configured)
 * or ENOBUFS (the queue dropped it). */
int udpdk_arp_announce(void);
/* Session sums over polls, like udpdk_icmp_counts: the batches or chunks the stage ran on (scanned),
 * the device stage's counts (udpdk_arp_stats_t without bad_frame) and the announcements queued.
 * udpdk_host_reset zeroes them. */
typedef struct {
    uint64_t scanned, arp, malformed, other_op, own, sender_bad, not_ours, conflict, eligible, replies, no_room,
             announced;
} udpdk_arp_counts_t;
int udpdk_arp_counts(udpdk_arp_counts_t *counts);

/* Multicast (ini: [gpu] mcast = 0 | 1; default 0: as in the reference, which has no multicast, a
 * datagram to 239.1.2.3:5000 lands in every socket bound to ANY:5000, no IGMP is sent and a query
 * ends as NOT_UDP).
 *   udpdk_setsockopt(s, IPPROTO_IP, IP_ADD_MEMBERSHIP | IP_DROP_MEMBERSHIP, struct ip_mreq | struct
 *   ip_mreqn) records a membership whether or not the switch is on. imr_interface (imr_address) must
 *   be INADDR_ANY or our address and an interface index 0, else ENODEV; a group outside 224.0.0.0/4:
 *   EINVAL; a second join of the same group on the socket: EADDRINUSE; a drop without a join:
 *   EADDRNOTAVAIL; more than 20 groups on one socket: ENOBUFS (Linux's igmp_max_memberships); any
 *   other IPPROTO_IP option: ENOPROTOOPT. udpdk_close drops the socket's groups.
 * Membership is PER SOCKET, which is Linux with IP_MULTICAST_ALL = 0 and not Linux's default: a
 * socket receives a group only if it joined the group itself, not because another socket of the
 * host did.
 * With the switch on
 *  - udpdk_poll_rx runs the membership filter (udpdk_gpu_rx_mcast, udpdk_gpu.h) as the last
 *    lane-removal stage of every RX call, the pass over reassembled datagrams included: a socket
 *    bound to INADDR_ANY or to a group address keeps a multicast datagram only if it joined the
 *    datagram's group; unicast and 255.255.255.255 pass, and a socket bound to a specific unicast
 *    address is not looked at. udpdk_rx_not_member counts what the filter removed. The tables are
 *    uploaded again whenever a membership or the bind table changed.
 *  - udpdk_poll_rx runs udpdk_gpu_igmp_reply on every staged batch whose RX counters show a frame
 *    that is IPv4 but not UDP, while at least one group is joined, before the ICMP stage: a general
 *    query is answered with one IGMPv2 report per joined group, a group-specific query with that
 *    group's. The reports, 46 bytes each, go onto the host queue of the ICMP answers, so
 *    udpdk_tx_drain emits them before the socket datagrams and udpdk_tx_pending counts them. At most
 *    4096 distinct groups are answered for.
 *  - the first join of a group queues one unsolicited report, the last drop of a group (udpdk_close
 *    included) one leave to 224.0.0.2, and turning the switch on one report per group already
 *    joined. 224.0.0.1 is never reported. Nothing is sent without a source address.
 * Not done: IGMPv3 and source filters; report suppression and the random response delay (a report
 * leaves with the next drain); the second unsolicited report; IP_MULTICAST_TTL, IP_MULTICAST_LOOP and
 * IP_MULTICAST_IF; sharded polls (there on = 1 gives -1 with ENOTSUP and udpdk_init fails on such
 * an ini, as for udpdk_config_arp); udpdk_poll_echo. Returns the value in force before the call; a
 * negative argument only reads it; above 1: -1, EINVAL. */
int udpdk_config_mcast(int on);
/* Session sums, like udpdk_arp_counts: the batches or chunks the IGMP stage ran on (scanned), the
 * device stage's counts (udpdk_igmp_stats_t without no_room and bad_frame), the memberships added
 * and dropped (joins, leaves; counted with the switch off too) and the reports and leaves queued.
 * udpdk_host_reset zeroes them. */
typedef struct {
    uint64_t scanned, igmp, malformed, bad_cksum, other_type, bad_dst, general, not_member, specific, reports,
             joins, leaves, reports_sent, leaves_sent;
} udpdk_mcast_counts_t;
int udpdk_mcast_counts(udpdk_mcast_counts_t *counts);
/* Deliveries the membership filter removed, summed over the session like udpdk_rx_refused. */
uint64_t udpdk_rx_not_member(void);

/* Neighbours (ini: [gpu] neigh = 0 | 1 | fallback; default 0: as in the reference, every frame goes to
 * the [port0_dst] MAC). With the switch on the main context keeps a neighbour table (udpdk_gpu.h; ini:
 * [gpu] neigh_entries, default 1024; neigh_ttl_ms, default 30000; neigh_retrans_ms, default 1000), and
 *  - udpdk_poll_rx runs udpdk_gpu_neigh_learn on every staged batch whose RX counters show a frame that
 *    is not IPv4, behind the ARP replies and on the same pipe: the stack learns from the ARP it
 *    receives (requests for its address, and replies and announcements about what it asked for). This
 *    does not need [gpu] arp = 1. Time is the monotonic clock in milliseconds;
 *  - udpdk_tx_drain resolves every datagram before the build (udpdk_gpu_neigh_resolve, rules R1-R5,
 *    with ini [port0] netmask, default 0: everything is on-link, and [port0] gateway) and
 *    udpdk_gpu_tx_build_neigh writes its next hop's MAC into its frames. The who-has requests for what
 *    is not known (at most 256 a drain) go onto the host queue of the ARP and ICMP frames and leave
 *    first in the next drain. A datagram without a MAC is, in mode 1 (strict), dequeued, dropped and
 *    counted (tx_unresolved; its span in the drain's output is a gap), as the drain drops what it
 *    cannot send; in mode 2 (fallback) it goes to the [port0_dst] MAC while the request is out. A
 *    destination without a route is dropped in both. In strict mode [port0_dst] is not needed.
 * Off, a poll and a drain call what they always called. Not done: the ICMP answers and udpdk_poll_echo
 * keep the configured MAC; no hold queue for unresolved datagrams; expired entries are not removed from
 * a full table; nothing is learned from IPv4 traffic; no address defence; sharded polls (there a mode
 * above 0 gives -1 with ENOTSUP and udpdk_init fails on such an ini, as for udpdk_config_arp).
 * Returns the mode in force before the call; a negative argument only reads it; above 2: -1, EINVAL. */
#define UDPDK_NEIGH_MODE_OFF      0
#define UDPDK_NEIGH_MODE_STRICT   1
#define UDPDK_NEIGH_MODE_FALLBACK 2
int udpdk_config_neigh(int mode);
/* A static entry (never learned over, never expires) for raw address ip. Needs the session's GPU
 * (ENODEV); -1 with ENOSPC when the table is full, EINVAL for address 0. udpdk_neigh_flush clears the
 * table, static entries included. */
int udpdk_neigh_add(uint32_t ip, const uint8_t mac[6]);
int udpdk_neigh_flush(void);
/* Session sums over polls and drains: the learn stage's counts (udpdk_neigh_learn_stats_t), the resolve
 * stage's (udpdk_neigh_resolve_stats_t, its `requests` aside), the datagrams a drain dropped for want
 * of a MAC or a route (tx_unresolved) and the who-has frames queued (requests). udpdk_host_reset zeroes
 * them. */
typedef struct {
    uint64_t arp, malformed, bad_frame, other_op, sender_bad, updated, refreshed, static_kept, created, full, ignored;
    uint64_t skipped, bcast, mcast, no_route, self, hit, expired, incomplete, inserted, table_full, fallback,
             unresolved, no_room;
    uint64_t tx_unresolved, requests;
} udpdk_neigh_counts_t;
int udpdk_neigh_counts(udpdk_neigh_counts_t *counts);

/* Segmented sends: Linux's UDP_SEGMENT. One send carries the payload of up to UDPDK_GSO_MAX_SEGS
 * (64, Linux's UDP_MAX_SEGMENTS) datagrams plus a segment size g, is queued as one ring entry with
 * its payload stored once, and udpdk_tx_drain cuts it on the GPU (udpdk_gpu_tx_segment_plan,
 * udpdk_gpu.h): datagrams of g bytes, the last one the remainder, all to the send's destination.
 *   - udpdk_setsockopt(s, IPPROTO_UDP (= SOL_UDP), UDP_SEGMENT, &int, len) stores the socket's size,
 *     0..65535 (0: off); a negative value, one above 65535 or optlen < sizeof(int): EINVAL.
 *     udpdk_getsockopt returns it. Any other IPPROTO_UDP option keeps the answer it always had
 *     (EINVAL, as for every level but SOL_SOCKET and IPPROTO_IP). udpdk_close and
 *     udpdk_host_reset clear it. udpdk_sendto, udpdk_send and udpdk_sendmsg honour it alike.
 *   - udpdk_sendmsg gathers msg_iov in order into one payload; msg_name is the destination, or NULL
 *     for the peer of a connected socket, by udpdk_sendto's rules (as are the pending error, the
 *     auto-bind, ENOBUFS and EMSGSIZE). A control message SOL_UDP / UDP_SEGMENT of
 *     CMSG_LEN(sizeof(uint16_t)) overrides the socket's size for this call; another length, or any
 *     other control message: EINVAL. Without a size in force it is udpdk_sendto of the gathered bytes.
 *   - with a size g > 0 in force (Linux's udp_send_skb): 28 + g > mtu (udpdk_config_mtu) gives
 *     EINVAL whatever the length, so a segment never fragments; len > g * UDPDK_GSO_MAX_SEGS gives
 *     EINVAL; len > 65507 gives EMSGSIZE; len <= g is queued as an ordinary datagram; otherwise the
 *     call queues one entry and returns len.
 *   - udpdk_tx_drain treats a send as a unit: its frames and bytes count against the drain's limits
 *     as a whole (udpdk_gpu_tx_segment_span), its segments are consecutive frames and never split
 *     across drains, a send no drain with these limits can carry is dropped and counted once in
 *     udpdk_tx_dropped, and udpdk_tx_pending counts a queued send as one. A drain that selected no
 *     such send launches what it always launched. With the neighbour cache on, every segment is
 *     resolved, and an unresolved one counts once in tx_unresolved.
 * One divergence from Linux: there segments are always checksummed and a socket with checksums off
 * is refused; here they follow udpdk_config_tx_cksum like every other datagram. The IPv4 id stays 0,
 * as in everything this stack sends. Not done: UDP_GRO, udpdk_poll_echo, MSG_MORE / corking (flags
 * must be 0), recvmsg. */
#ifndef SOL_UDP
#define SOL_UDP 17
#endif
#ifndef UDP_SEGMENT
#define UDP_SEGMENT 103
#endif
ssize_t udpdk_sendmsg(int s, const struct msghdr *msg, int flags);
/* Session sums: sends queued with more than one segment, their segments, the drains that launched
 * the segment plan, and the sends refused with EINVAL by the size rules above. udpdk_host_reset
 * zeroes them. */
typedef struct {
    uint64_t sends, segments, plans, refused;
} udpdk_gso_counts_t;
int udpdk_gso_counts(udpdk_gso_counts_t *counts);

/* Socket slot state (exch_slot_info, udpdk_types.h:40-47) for the GPU TX slot table. */
int udpdk_slot_table(udpdk_slot_t *slots, uint32_t n_slots);

/* Drop every socket, binding, queue and the interrupt flag without touching the GPU context
 * (test isolation; the reference only resets through process restart). */
void udpdk_host_reset(void);

#ifdef __cplusplus
}
#endif

#endif /* UDPDK_API_H */
