// udpdk_gpu_ctl.hip — host side of the control-plane stages of include/udpdk_gpu.h: ICMP replies
// (icmp_reply.hip), received ICMP errors (icmp_error.hip), ARP replies (arp_reply.hip), the IGMP
// responder (igmp_reply.hip) and the neighbour cache (neigh.hip).
//
// Every stage has the same four entry points around its own argument check, enqueue and stats
// functions, all through stage_form and stage_stats: on the context stream, and on a pipe's stream,
// where the counts follow the stage on the stream and are read after udpdk_gpu_pipe_wait. The
// context and what the forms stand on are gpu_ctx.h's.
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gpu_ctx.h"

using namespace udpdk;

namespace {

// What every stage over an RX batch asks of it.
int batch_check(const udpdk_rx_batch_t *bt)
{
    if (bt->frames_bytes >= (1ull << 32)) return -EINVAL;
    if (bt->n && (!bt->frames_dev || !bt->offset_dev || !bt->length_dev)) return -EINVAL;
    return 0;
}

// Whether the batch's frame buffer with its tailroom overlaps the output [p, p + bytes); an output of
// no bytes that points inside the buffer counts too.
bool frames_overlap(const udpdk_rx_batch_t *bt, const void *p, uint64_t bytes)
{
    const uintptr_t f0 = (uintptr_t)bt->frames_dev, f1 = f0 + bt->frames_bytes + UDPDK_GPU_FRAMES_TAILROOM;
    const uintptr_t o0 = (uintptr_t)p, o1 = o0 + bytes;
    return bt->frames_dev && o0 < f1 && f0 < o1;
}

// The batch as every stage's kernel arguments hold it.
template <typename A>
void batch_fill(A &a, const udpdk_rx_batch_t *bt, const uint32_t *meta_dev)
{
    a.frames = bt->frames_dev;
    a.offset = bt->offset_dev;
    a.length = bt->length_dev;
    a.meta = meta_dev;
    a.n = bt->n;
    a.frames_bytes = (uint32_t)bt->frames_bytes;
    a.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
}

// A MAC as the kernels hold it: bytes 0-3 and 4-5 as little-endian words.
void mac_words(const uint8_t *mac, uint32_t *lo, uint32_t *hi)
{
    *lo = *hi = 0u;
    memcpy(lo, mac, 4);
    memcpy(hi, mac + 4, 2);
}

// A workspace's candidates (the IGMP responder has none).
template <typename W> int cand_ensure(udpdk_gpu_ctx *c, W &ws, size_t count) { return ws.cand.ensure(c, count); }
int cand_ensure(udpdk_gpu_ctx *, IgmpQWs &, size_t) { return 0; }

// The workspace of a stage of fanin_stage.h's shape for n units in workgroups of `tile`, at least
// what max_frames needs: `row_words` words per workgroup (the row, rbase where the stage has one),
// `tile` candidates per workgroup where the workspace has them, the result, and the fan-in words,
// zeroed on stream st when they are new.
template <typename W>
int fanin_ws(udpdk_gpu_ctx *c, W &ws, hipStream_t st, uint32_t n, uint32_t tile, uint32_t row_words)
{
    const size_t rows = std::max<size_t>(ceil_div(std::max(n, c->max_frames), tile), 1);
    int rc;
    if ((rc = cand_ensure(c, ws, rows * tile)) || (rc = ws.row.ensure(c, rows * row_words)) || (rc = ws.res.ensure(c)))
        return rc;
    if (!ws.fuse) {
        if ((rc = ws.fuse.ensure(c, FUSE_BYTES / 8))) return rc;
        HIPC(c, hipMemsetAsync(ws.fuse, 0, FUSE_BYTES, st));
    }
    return 0;
}

// What a stage leaves of an empty batch: no launch, a result of zeros.
template <typename R>
int empty_result(udpdk_gpu_ctx *c, ResultSlot<R> &res, hipStream_t st)
{
    HIPC(c, hipMemsetAsync(res.dev, 0, sizeof(R), st));
    res.ran = true;
    return 0;
}

// Where an entry point runs its stage: 0 is the context stream with the context's workspace, 1 and
// up a pipe's stream with the pipe's. The pipe forms do not take 0.
int on_pipe(int pipe) { return pipe >= 1 ? pipe : -1; }

// A stage there: `checked` is what its argument check said (nothing is enqueued unless it passed),
// enqueue(c, workspace, stream, args...) the stage. On a pipe the counts follow on the stream, for
// stage_stats after udpdk_gpu_pipe_wait.
template <typename W, typename... P, typename... A>
int stage_form(udpdk_gpu_ctx *c, int pipe, W CtlWs::*ws, int checked,
               int (*enqueue)(udpdk_gpu_ctx *, W &, hipStream_t, P...), A... args)
{
    if (!c || pipe < 0 || pipe >= MAX_PIPES) return -EINVAL;
    int rc = checked;
    if (rc) return rc;
    if (!pipe) return (rc = on_ctx_stream(c)) ? rc : enqueue(c, c->ctl.*ws, c->stream, args...);
    HIPC(c, hipSetDevice(c->device));
    Pipe &pp = c->pipes[pipe];
    pp.dirty = true;
    if ((rc = enqueue(c, pp.ctl.*ws, pp.stream, args...))) return rc;
    return (pp.ctl.*ws).res.enqueue_fetch(c, pp.stream);
}

// A stage's counts: fetched and waited for on the context stream, or as the pipe form left them.
template <typename W, typename R, typename S>
int stage_stats(udpdk_gpu_ctx *c, int pipe, W CtlWs::*ws, S *st, int (*out)(const R *, S *))
{
    if (!c || !st || pipe < 0 || pipe >= MAX_PIPES) return -EINVAL;
    ResultSlot<R> &res = ((pipe ? c->pipes[pipe].ctl : c->ctl).*ws).res;
    const int rc = pipe ? (res.ran ? 0 : -ENOENT) : ctx_result(c, res);
    return rc ? rc : out(res.host, st);
}

int tile_geometry(uint32_t n, uint32_t tile, uint32_t *frames_per_block, uint32_t *n_blocks)
{
    if (!frames_per_block || !n_blocks) return -EINVAL;
    *frames_per_block = tile;
    *n_blocks = std::max<uint32_t>(1u, ceil_div(n, tile));
    return 0;
}

// Argument checks of udpdk_gpu_icmp_reply and its pipe form.
int icmp_check(const udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
               const uint32_t *meta_dev, uint32_t flags, uint32_t mtu, const udpdk_icmp_out_t *o)
{
    if (!c || !cfg || !bt || !meta_dev || !o) return -EINVAL;
    if (!flags || (flags & ~UDPDK_ICMP_ALL)) return -EINVAL;
    if (mtu && (mtu < 68u || mtu > 65535u || (mtu - 20u) % 8u)) return -EINVAL;
    if (batch_check(bt) || o->out_cap >= (1ull << 32)) return -EINVAL;
    if (!o->frames_dev || !o->reply_off_dev || !o->origin_dev) return -EINVAL;
    if ((uintptr_t)o->frames_dev & 15u) return -EINVAL;
    return frames_overlap(bt, o->frames_dev, o->out_cap) ? -EINVAL : 0;
}

// The stage (icmp_reply.hip) on stream st with workspace W: scan, base, build.
int icmp_enqueue(udpdk_gpu_ctx *c, IcmpWs &W, hipStream_t st, const udpdk_tx_config_t *cfg,
                 const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, uint32_t flags, uint32_t mtu,
                 uint32_t err_limit, const udpdk_icmp_out_t *o)
{
    const uint32_t nb = ceil_div(bt->n, ICMP_TILE);
    const size_t rows = std::max<size_t>(ceil_div(std::max(bt->n, c->max_frames), ICMP_TILE), 1);
    int rc;
    if ((rc = W.cand.ensure(c, rows * ICMP_TILE)) || (rc = W.row.ensure(c, rows * (ICMP_ROW + 2))) ||
        (rc = W.bbase.ensure(c, rows)) || (rc = W.res.ensure(c)))
        return rc;
    if (!bt->n) {
        HIPC(c, hipMemsetAsync(o->reply_off_dev, 0, 4, st));
        return empty_result(c, W.res, st);
    }
    IcmpArgs ia;
    batch_fill(ia, bt, meta_dev);
    ia.out = o->frames_dev;
    ia.reply_off = o->reply_off_dev;
    ia.origin = o->origin_dev;
    ia.cand = W.cand;
    ia.row = W.row;
    ia.ubase = W.row + (size_t)ICMP_ROW * nb;
    ia.rbase = ia.ubase + nb;
    ia.bbase = W.bbase;
    ia.res = W.res.dev;
    ia.n_blocks = nb;
    ia.flags = flags;
    ia.mtu = mtu;
    ia.err_limit = err_limit;
    ia.out_cap = (uint32_t)o->out_cap;
    ia.max_replies = o->max_replies;
    ia.src_ip = cfg->src_ip;
    uint8_t mac[12];
    memcpy(mac, cfg->dst_mac, 6);   // Ethernet d_addr first, as tx_build
    memcpy(mac + 6, cfg->src_mac, 6);
    memcpy(ia.mac_lo, mac, 12);
    hipLaunchKernelGGL(icmp_scan, dim3(nb), dim3(ICMP_BLOCK), 0, st, ia);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(icmp_base, dim3(1), dim3(ICMP_BASE_BLOCK), 0, st, ia);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(icmp_build, dim3(nb), dim3(ICMP_BLOCK), 0, st, ia);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

int icmp_stats_out(const IcmpResult *r, udpdk_icmp_stats_t *st)
{
    st->bytes_needed = r->bytes_needed;
    st->echo_replied = r->echo_replied;
    st->unreach_sent = r->unreach_sent;
    st->replies = r->echo_replied + r->unreach_sent;
    st->echo_bad = r->echo_bad;
    st->limited = r->limited;
    st->no_room = r->no_room;
    st->bad_frame = r->bad_frame;
    return st->no_room ? -ENOSPC : 0;
}

// Argument checks of udpdk_gpu_icmp_errors and its pipe form.
int icmp_err_check(const udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *meta_dev,
                   const udpdk_peer_t *peer_dev, uint32_t n_lanes, const uint64_t *err_dev)
{
    if (!c || !bt || !meta_dev || !err_dev) return -EINVAL;
    if (((uintptr_t)peer_dev & 7u) != 0 || ((uintptr_t)err_dev & 7u) != 0) return -EINVAL;
    if (n_lanes == 0 || n_lanes > UDPDK_GPU_MAX_LANES) return -EINVAL;
    if (batch_check(bt)) return -EINVAL;
    if (!c->have_snapshot || c->lane_mask != 0xFFFFFFFFu) return -EINVAL;   // compat mode: a lane is not a sockfd
    if (!peer_dev && !c->peer_on) return -ENOENT;                          // no sticky table in force
    return 0;
}

// The stage (icmp_error.hip) on stream st with result slot W: clear, scan.
int icmp_err_enqueue(udpdk_gpu_ctx *c, IcmpErrWs &W, hipStream_t st, uint32_t our_ip, const udpdk_rx_batch_t *bt,
                     const uint32_t *meta_dev, const udpdk_peer_t *peer_dev, uint32_t n_lanes, uint64_t *err_dev)
{
    int rc;
    if ((rc = W.res.ensure(c))) return rc;
    unsigned long long *err = reinterpret_cast<unsigned long long *>(err_dev);
    hipLaunchKernelGGL(icmp_err_clear, dim3(ceil_div(std::max(n_lanes, ICMP_ERR_ROW + 1u), (uint32_t)ICMP_ERR_BLOCK)),
                       dim3(ICMP_ERR_BLOCK), 0, st, err, n_lanes, W.res.dev.p);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    if (!bt->n) return 0;
    IcmpErrArgs ea;
    batch_fill(ea, bt, meta_dev);
    ea.port_tab = c->port_tab;
    ea.binds = c->binds;
    // the sticky table holds max_lanes records, off past what udpdk_gpu_rx_peer was given
    ea.peer = peer_dev ? reinterpret_cast<const uint2 *>(peer_dev) : c->peer_tab;
    ea.err = err;
    ea.res = W.res.dev;
    ea.our_ip = our_ip;
    ea.n_lanes = n_lanes;
    ea.peer_n = peer_dev ? n_lanes : c->max_lanes;
    hipLaunchKernelGGL(icmp_err_scan, dim3(ceil_div(bt->n, ICMP_ERR_TILE)), dim3(ICMP_ERR_BLOCK), 0, st, ea);
    HIPC(c, hipGetLastError());
    return 0;
}

int icmp_err_stats_out(const IcmpErrResult *r, udpdk_icmp_err_stats_t *st)
{
    st->errors = r->c[ICMP_X_ERRORS];
    st->msg_bad = r->c[ICMP_X_MSG_BAD];
    st->quote_bad = r->c[ICMP_X_QUOTE_BAD];
    st->soft = r->c[ICMP_X_SOFT];
    st->no_socket = r->c[ICMP_X_NO_SOCKET];
    st->reported = r->c[ICMP_X_REPORTED];
    st->bad_frame = r->c[ICMP_X_BAD_FRAME];
    return 0;
}

// Argument checks of udpdk_gpu_arp_reply and its pipe form.
int arp_check(const udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
              const uint32_t *meta_dev, const udpdk_arp_out_t *o)
{
    if (!c || !cfg || !bt || !meta_dev || !o) return -EINVAL;
    if (cfg->src_ip == 0u || batch_check(bt)) return -EINVAL;
    if (!o->frames_dev || !o->origin_dev) return -EINVAL;
    if ((uintptr_t)o->frames_dev & 15u) return -EINVAL;
    // the slots and the origin entries
    if (frames_overlap(bt, o->frames_dev, (uint64_t)o->max_replies * ARP_SLOT) ||
        frames_overlap(bt, o->origin_dev, (uint64_t)o->max_replies * 4u))
        return -EINVAL;
    return 0;
}

// The stage (arp_reply.hip) on stream st with workspace W: one launch.
int arp_enqueue(udpdk_gpu_ctx *c, ArpWs &W, hipStream_t st, const udpdk_tx_config_t *cfg,
                const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, const udpdk_arp_out_t *o)
{
    const uint32_t nb = ceil_div(bt->n, ARP_TILE);
    const int rc = fanin_ws(c, W, st, bt->n, ARP_TILE, ARP_ROW + 1);
    if (rc) return rc;
    if (!bt->n) return empty_result(c, W.res, st);
    ArpArgs aa;
    batch_fill(aa, bt, meta_dev);
    aa.out = o->frames_dev;
    aa.origin = o->origin_dev;
    aa.cand = W.cand;
    aa.row = W.row;
    aa.rbase = W.row + (size_t)ARP_ROW * nb;
    aa.fuse = W.fuse;
    aa.res = W.res.dev;
    aa.n_blocks = nb;
    aa.max_replies = o->max_replies;
    aa.src_ip = cfg->src_ip;
    mac_words(cfg->src_mac, &aa.mac_lo, &aa.mac_hi);
    hipLaunchKernelGGL(arp_reply, dim3(nb), dim3(ARP_BLOCK), 0, st, aa);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

int arp_stats_out(const ArpResult *r, udpdk_arp_stats_t *st)
{
    st->arp = r->c[ARP_R_ARP];
    st->malformed = r->c[ARP_R_MALFORMED];
    st->other_op = r->c[ARP_R_OTHER_OP];
    st->own = r->c[ARP_R_OWN];
    st->sender_bad = r->c[ARP_R_SENDER_BAD];
    st->not_ours = r->c[ARP_R_NOT_OURS];
    st->conflict = r->c[ARP_R_CONFLICT];
    st->eligible = r->c[ARP_R_ELIGIBLE];
    st->replies = r->replies;
    st->no_room = r->no_room;
    st->bad_frame = r->c[ARP_R_BAD_FRAME];
    return st->no_room ? -ENOSPC : 0;
}

// Argument checks of udpdk_gpu_igmp_reply and its pipe form.
int igmp_check(const udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
               const uint32_t *meta_dev, const uint32_t *groups_dev, uint32_t n_groups, const udpdk_igmp_out_t *o)
{
    if (!c || !cfg || !bt || !meta_dev || !o) return -EINVAL;
    if (cfg->src_ip == 0u || n_groups > IGMP_MAX_GROUPS || (!groups_dev && n_groups)) return -EINVAL;
    if (batch_check(bt)) return -EINVAL;
    if (!o->frames_dev || !o->group_index_dev) return -EINVAL;
    if ((uintptr_t)o->frames_dev & 15u) return -EINVAL;
    // the slots and the index entries
    if (frames_overlap(bt, o->frames_dev, (uint64_t)o->max_reports * IGMP_SLOT) ||
        frames_overlap(bt, o->group_index_dev, (uint64_t)o->max_reports * 4u))
        return -EINVAL;
    return 0;
}

// The stage (igmp_reply.hip) on stream st with workspace W: one launch.
int igmp_enqueue(udpdk_gpu_ctx *c, IgmpQWs &W, hipStream_t st, const udpdk_tx_config_t *cfg,
                 const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, const uint32_t *groups_dev, uint32_t n_groups,
                 const udpdk_igmp_out_t *o)
{
    const uint32_t nb = ceil_div(bt->n, IGMP_TILE);
    int rc = fanin_ws(c, W, st, bt->n, IGMP_TILE, IGMP_ROW);
    if (rc) return rc;
    if (!W.bits) {                               // (on its own: it may fail where the fan-in words did not)
        if ((rc = W.bits.ensure(c, IGMP_WORDS))) return rc;
        HIPC(c, hipMemsetAsync(W.bits, 0, IGMP_WORDS * sizeof(uint32_t), st));
    }
    if (!bt->n) return empty_result(c, W.res, st);
    IgmpQArgs ga;
    batch_fill(ga, bt, meta_dev);
    ga.groups = groups_dev;
    ga.out = o->frames_dev;
    ga.group_index = o->group_index_dev;
    ga.row = W.row;
    ga.bits = W.bits;
    ga.fuse = W.fuse;
    ga.res = W.res.dev;
    ga.n_blocks = nb;
    ga.n_groups = n_groups;
    ga.max_reports = o->max_reports;
    ga.src_ip = cfg->src_ip;
    mac_words(cfg->src_mac, &ga.mac_lo, &ga.mac_hi);
    hipLaunchKernelGGL(igmp_reply, dim3(nb), dim3(IGMP_BLOCK), 0, st, ga);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

int igmp_stats_out(const IgmpQResult *r, udpdk_igmp_stats_t *st)
{
    st->igmp = r->c[IGMP_R_IGMP];
    st->malformed = r->c[IGMP_R_MALFORMED];
    st->bad_cksum = r->c[IGMP_R_BAD_CKSUM];
    st->other_type = r->c[IGMP_R_OTHER_TYPE];
    st->bad_dst = r->c[IGMP_R_BAD_DST];
    st->general = r->c[IGMP_R_GENERAL];
    st->not_member = r->c[IGMP_R_NOT_MEMBER];
    st->specific = r->c[IGMP_R_SPECIFIC];
    st->reports = r->reports;
    st->no_room = r->no_room;
    st->bad_frame = r->c[IGMP_R_BAD_FRAME];
    return st->no_room ? -ENOSPC : 0;
}

uint32_t neigh_shift(uint32_t entries) { return 32u - (uint32_t)__builtin_ctz(entries); }

// The table on the host (set, dump, flush): a copy, waited for. All streams are drained first, so
// no kernel is the table's writer meanwhile.
int neigh_fetch(udpdk_gpu_ctx *c, std::vector<udpdk_neigh_entry_t> &t)
{
    if (!c || !c->neigh_entries) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    t.resize(c->neigh_entries);
    HIPC(c, hipMemcpy(t.data(), c->neigh_tab, t.size() * sizeof(t[0]), hipMemcpyDeviceToHost));
    return 0;
}

int neigh_store(udpdk_gpu_ctx *c, const std::vector<udpdk_neigh_entry_t> &t)
{
    HIPC(c, hipMemcpy(c->neigh_tab, t.data(), t.size() * sizeof(t[0]), hipMemcpyHostToDevice));
    return 0;
}

// The kernels' probe sequence on the host copy: the slot of e.ip, or the first empty one.
int neigh_put(std::vector<udpdk_neigh_entry_t> &t, const udpdk_neigh_entry_t &e)
{
    const uint32_t mask = (uint32_t)t.size() - 1u;
    uint32_t s = neigh_home(e.ip, neigh_shift((uint32_t)t.size()));
    for (uint32_t k = 0; k <= mask; ++k, s = (s + 1u) & mask) {
        if (t[s].ip != e.ip && t[s].ip != 0u) continue;
        t[s] = e;
        t[s].pad = 0;
        return 0;
    }
    return -ENOSPC;
}

int neigh_cfg_check(const udpdk_gpu_ctx *c, const udpdk_neigh_cfg_t *cfg)
{
    if (!c || !cfg || !c->neigh_entries) return -EINVAL;
    if (cfg->src_ip == 0u || (cfg->flags & ~UDPDK_NEIGH_FALLBACK)) return -EINVAL;
    return 0;
}

// Argument checks of udpdk_gpu_neigh_learn and its pipe form.
int neigh_learn_check(const udpdk_gpu_ctx *c, const udpdk_neigh_cfg_t *cfg, const udpdk_rx_batch_t *bt,
                      const uint32_t *meta_dev)
{
    const int rc = neigh_cfg_check(c, cfg);
    if (rc) return rc;
    return !bt || !meta_dev || batch_check(bt) ? -EINVAL : 0;
}

// The learn stage (neigh.hip) on stream st with workspace W: one launch.
int neigh_learn_enqueue(udpdk_gpu_ctx *c, NeighLearnWs &W, hipStream_t st, const udpdk_neigh_cfg_t *cfg,
                        const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, uint32_t now)
{
    const uint32_t nb = ceil_div(bt->n, NL_TILE);
    const int rc = fanin_ws(c, W, st, bt->n, NL_TILE, NL_ROW + 1);
    if (rc) return rc;
    if (!bt->n) return empty_result(c, W.res, st);
    NeighLearnArgs a;
    batch_fill(a, bt, meta_dev);
    a.tab = c->neigh_tab;
    a.cand = W.cand;
    a.row = W.row;
    a.rbase = W.row + (size_t)NL_ROW * nb;
    a.fuse = W.fuse;
    a.res = W.res.dev;
    a.n_blocks = nb;
    a.mask = c->neigh_entries - 1u;
    a.shift = neigh_shift(c->neigh_entries);
    a.src_ip = cfg->src_ip;
    mac_words(cfg->src_mac, &a.mac_lo, &a.mac_hi);
    a.now = now;
    hipLaunchKernelGGL(neigh_learn, dim3(nb), dim3(NL_BLOCK), 0, st, a);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

int neigh_learn_stats_out(const NeighLearnResult *r, udpdk_neigh_learn_stats_t *st)
{
    st->arp = r->c[NL_R_ARP];
    st->malformed = r->c[NL_R_MALFORMED];
    st->bad_frame = r->c[NL_R_BAD_FRAME];
    st->other_op = r->c[NL_R_OTHER_OP];
    st->sender_bad = r->c[NL_R_SENDER_BAD];
    st->updated = r->o[NL_O_UPDATED];
    st->refreshed = r->o[NL_O_REFRESHED];
    st->static_kept = r->o[NL_O_STATIC_KEPT];
    st->created = r->o[NL_O_CREATED];
    st->full = r->o[NL_O_FULL];
    st->ignored = r->o[NL_O_IGNORED];
    return 0;
}

// Argument checks of udpdk_gpu_neigh_resolve.
int neigh_resolve_check(const udpdk_gpu_ctx *c, const udpdk_neigh_cfg_t *cfg, const uint32_t *dst_ip_dev,
                        const int32_t *sockfd_dev, const udpdk_neigh_out_t *o)
{
    const int rc = neigh_cfg_check(c, cfg);
    if (rc) return rc;
    if (!dst_ip_dev || !sockfd_dev || !o || !o->dmac_dev || !o->sockfd_out_dev || !o->state_dev) return -EINVAL;
    if (o->req_cap && (!o->req_dev || !o->req_origin_dev)) return -EINVAL;
    if (((uintptr_t)o->dmac_dev & 7u) || ((uintptr_t)o->req_dev & 15u)) return -EINVAL;
    return 0;
}

// The resolve stage (neigh.hip) on stream st with workspace W: one launch.
int neigh_resolve_enqueue(udpdk_gpu_ctx *c, NeighResolveWs &W, hipStream_t st, const udpdk_neigh_cfg_t *cfg,
                          const uint32_t *dst_ip_dev, const int32_t *sockfd_dev, uint32_t n, uint32_t now,
                          const udpdk_neigh_out_t *o)
{
    const uint32_t nb = ceil_div(n, NR_TILE);
    const int rc = fanin_ws(c, W, st, n, NR_TILE, NR_ROW + 1);
    if (rc) return rc;
    if (!n) return empty_result(c, W.res, st);
    NeighResolveArgs a;
    a.dst_ip = dst_ip_dev;
    a.sockfd = sockfd_dev;
    a.dmac = o->dmac_dev;
    a.sockfd_out = o->sockfd_out_dev;
    a.state = o->state_dev;
    a.req = o->req_dev;
    a.req_origin = o->req_origin_dev;
    a.tab = c->neigh_tab;
    a.cand = W.cand;
    a.row = W.row;
    a.rbase = W.row + (size_t)NR_ROW * nb;
    a.fuse = W.fuse;
    a.res = W.res.dev;
    a.n = n;
    a.n_blocks = nb;
    a.req_cap = o->req_cap;
    a.mask = c->neigh_entries - 1u;
    a.shift = neigh_shift(c->neigh_entries);
    a.src_ip = cfg->src_ip;
    a.netmask = cfg->netmask;
    a.gateway = cfg->gateway;
    mac_words(cfg->src_mac, &a.mac_lo, &a.mac_hi);
    mac_words(cfg->fallback_mac, &a.fb_lo, &a.fb_hi);
    a.ttl_ms = cfg->ttl_ms;
    a.retrans_ms = std::max(cfg->retrans_ms, 1u);
    a.fallback = (cfg->flags & UDPDK_NEIGH_FALLBACK) ? 1u : 0u;
    a.now = now;
    hipLaunchKernelGGL(neigh_resolve, dim3(nb), dim3(NR_BLOCK), 0, st, a);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

int neigh_resolve_stats_out(const NeighResolveResult *r, udpdk_neigh_resolve_stats_t *st)
{
    st->skipped = r->c[NR_R_SKIPPED];
    st->bcast = r->c[NR_R_BCAST];
    st->mcast = r->c[NR_R_MCAST];
    st->no_route = r->c[NR_R_NO_ROUTE];
    st->self = r->c[NR_R_SELF];
    st->hit = r->c[NR_R_HIT];
    st->expired = r->o[NR_O_EXPIRED];
    st->incomplete = r->o[NR_O_INCOMPLETE];
    st->inserted = r->o[NR_O_INSERTED];
    st->table_full = r->o[NR_O_TABLE_FULL];
    st->fallback = r->fallback;
    st->unresolved = r->unresolved;
    st->requests = r->requests;
    st->no_room = r->no_room;
    return st->no_room ? -ENOSPC : 0;
}

} // namespace

extern "C" {

int udpdk_gpu_icmp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks)
{
    return tile_geometry(n, ICMP_TILE, frames_per_block, n_blocks);
}

int udpdk_gpu_icmp_reply(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
                         const uint32_t *meta_dev, uint32_t flags, uint32_t mtu, uint32_t err_limit,
                         const udpdk_icmp_out_t *o)
{
    return stage_form(c, 0, &CtlWs::icmp, icmp_check(c, cfg, bt, meta_dev, flags, mtu, o), icmp_enqueue, cfg, bt,
                      meta_dev, flags, mtu, err_limit, o);
}

int udpdk_gpu_pipe_icmp_reply(udpdk_gpu_ctx *c, int pipe, const udpdk_tx_config_t *cfg,
                              const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, uint32_t flags,
                              uint32_t mtu, uint32_t err_limit, const udpdk_icmp_out_t *o)
{
    return stage_form(c, on_pipe(pipe), &CtlWs::icmp, icmp_check(c, cfg, bt, meta_dev, flags, mtu, o), icmp_enqueue,
                      cfg, bt, meta_dev, flags, mtu, err_limit, o);
}

int udpdk_gpu_icmp_stats(udpdk_gpu_ctx *c, udpdk_icmp_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::icmp, st, icmp_stats_out);
}

int udpdk_gpu_pipe_icmp_stats(udpdk_gpu_ctx *c, int pipe, udpdk_icmp_stats_t *st)
{
    return stage_stats(c, on_pipe(pipe), &CtlWs::icmp, st, icmp_stats_out);
}

int udpdk_gpu_icmp_errors(udpdk_gpu_ctx *c, uint32_t our_ip, const udpdk_rx_batch_t *bt, const uint32_t *meta_dev,
                          const udpdk_peer_t *peer_dev, uint32_t n_lanes, uint64_t *err_dev)
{
    return stage_form(c, 0, &CtlWs::icmp_err, icmp_err_check(c, bt, meta_dev, peer_dev, n_lanes, err_dev),
                      icmp_err_enqueue, our_ip, bt, meta_dev, peer_dev, n_lanes, err_dev);
}

int udpdk_gpu_pipe_icmp_errors(udpdk_gpu_ctx *c, int pipe, uint32_t our_ip, const udpdk_rx_batch_t *bt,
                               const uint32_t *meta_dev, const udpdk_peer_t *peer_dev, uint32_t n_lanes,
                               uint64_t *err_dev)
{
    return stage_form(c, on_pipe(pipe), &CtlWs::icmp_err, icmp_err_check(c, bt, meta_dev, peer_dev, n_lanes, err_dev),
                      icmp_err_enqueue, our_ip, bt, meta_dev, peer_dev, n_lanes, err_dev);
}

int udpdk_gpu_icmp_err_stats(udpdk_gpu_ctx *c, udpdk_icmp_err_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::icmp_err, st, icmp_err_stats_out);
}

int udpdk_gpu_pipe_icmp_err_stats(udpdk_gpu_ctx *c, int pipe, udpdk_icmp_err_stats_t *st)
{
    return stage_stats(c, on_pipe(pipe), &CtlWs::icmp_err, st, icmp_err_stats_out);
}

int udpdk_gpu_icmp_errno(uint32_t code, int *hard)
{
    // Linux's icmp_err_convert (net/ipv4/icmp.c): errno and whether the error is fatal
    static const int err[16] = {ENETUNREACH, EHOSTUNREACH, ENOPROTOOPT, ECONNREFUSED, EMSGSIZE, EOPNOTSUPP,
                                ENETUNREACH, EHOSTDOWN, ENONET, ENETUNREACH, EHOSTUNREACH, ENETUNREACH,
                                EHOSTUNREACH, EHOSTUNREACH, EHOSTUNREACH, EHOSTUNREACH};
    if (hard) *hard = code < 16u ? (int)((ICMP_ERR_HARD_MASK >> code) & 1u) : 0;
    return code < 16u ? err[code] : 0;
}

int udpdk_gpu_arp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks)
{
    return tile_geometry(n, ARP_TILE, frames_per_block, n_blocks);
}

int udpdk_gpu_arp_reply(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
                        const uint32_t *meta_dev, const udpdk_arp_out_t *o)
{
    return stage_form(c, 0, &CtlWs::arp, arp_check(c, cfg, bt, meta_dev, o), arp_enqueue, cfg, bt, meta_dev, o);
}

int udpdk_gpu_pipe_arp_reply(udpdk_gpu_ctx *c, int pipe, const udpdk_tx_config_t *cfg,
                             const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, const udpdk_arp_out_t *o)
{
    return stage_form(c, on_pipe(pipe), &CtlWs::arp, arp_check(c, cfg, bt, meta_dev, o), arp_enqueue, cfg, bt,
                      meta_dev, o);
}

int udpdk_gpu_arp_stats(udpdk_gpu_ctx *c, udpdk_arp_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::arp, st, arp_stats_out);
}

int udpdk_gpu_pipe_arp_stats(udpdk_gpu_ctx *c, int pipe, udpdk_arp_stats_t *st)
{
    return stage_stats(c, on_pipe(pipe), &CtlWs::arp, st, arp_stats_out);
}

int udpdk_gpu_igmp_geometry(uint32_t n, uint32_t *frames_per_block, uint32_t *n_blocks)
{
    return tile_geometry(n, IGMP_TILE, frames_per_block, n_blocks);
}

int udpdk_gpu_igmp_reply(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
                         const uint32_t *meta_dev, const uint32_t *groups_dev, uint32_t n_groups,
                         const udpdk_igmp_out_t *o)
{
    return stage_form(c, 0, &CtlWs::igmp, igmp_check(c, cfg, bt, meta_dev, groups_dev, n_groups, o), igmp_enqueue,
                      cfg, bt, meta_dev, groups_dev, n_groups, o);
}

int udpdk_gpu_pipe_igmp_reply(udpdk_gpu_ctx *c, int pipe, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
                              const uint32_t *meta_dev, const uint32_t *groups_dev, uint32_t n_groups,
                              const udpdk_igmp_out_t *o)
{
    return stage_form(c, on_pipe(pipe), &CtlWs::igmp, igmp_check(c, cfg, bt, meta_dev, groups_dev, n_groups, o),
                      igmp_enqueue, cfg, bt, meta_dev, groups_dev, n_groups, o);
}

int udpdk_gpu_igmp_stats(udpdk_gpu_ctx *c, udpdk_igmp_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::igmp, st, igmp_stats_out);
}

int udpdk_gpu_pipe_igmp_stats(udpdk_gpu_ctx *c, int pipe, udpdk_igmp_stats_t *st)
{
    return stage_stats(c, on_pipe(pipe), &CtlWs::igmp, st, igmp_stats_out);
}

int udpdk_gpu_neigh_create(udpdk_gpu_ctx *c, uint32_t entries)
{
    if (!c || entries < 8u || entries > UDPDK_NEIGH_MAX_ENTRIES || (entries & (entries - 1u))) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    c->neigh_entries = 0;
    c->neigh_tab.release();
    if ((rc = c->neigh_tab.ensure(c, (size_t)entries * 4u))) return rc;
    HIPC(c, hipMemset(c->neigh_tab, 0, (size_t)entries * 16u));
    c->neigh_entries = entries;
    return 0;
}

int udpdk_gpu_neigh_set(udpdk_gpu_ctx *c, const udpdk_neigh_entry_t *e, uint32_t n)
{
    if (!c || (!e && n)) return -EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (e[i].ip == 0u || (e[i].state != UDPDK_NEIGH_STATIC && e[i].state != UDPDK_NEIGH_REACHABLE)) return -EINVAL;
    std::vector<udpdk_neigh_entry_t> t;
    int rc = neigh_fetch(c, t), full = 0;
    if (rc) return rc;
    for (uint32_t i = 0; i < n && !full; ++i) full = neigh_put(t, e[i]);
    rc = neigh_store(c, t);
    return rc ? rc : full;
}

int udpdk_gpu_neigh_dump(udpdk_gpu_ctx *c, udpdk_neigh_entry_t *out, uint32_t cap, uint32_t *n)
{
    if (!c || !n || (!out && cap)) return -EINVAL;
    std::vector<udpdk_neigh_entry_t> t;
    const int rc = neigh_fetch(c, t);
    if (rc) return rc;
    uint32_t k = 0;
    for (const udpdk_neigh_entry_t &e : t) {
        if (e.ip == 0u) continue;
        if (k < cap) out[k] = e;
        ++k;
    }
    *n = k;
    return k > cap ? -ENOSPC : 0;
}

int udpdk_gpu_neigh_flush(udpdk_gpu_ctx *c, int keep_static)
{
    std::vector<udpdk_neigh_entry_t> t;
    int rc = neigh_fetch(c, t);
    if (rc) return rc;
    // (the kept entries are put back by key: a probe sequence ends at the first empty slot)
    std::vector<udpdk_neigh_entry_t> u(t.size(), udpdk_neigh_entry_t{});
    if (keep_static)
        for (const udpdk_neigh_entry_t &e : t)
            if (e.ip != 0u && e.state == UDPDK_NEIGH_STATIC) (void)neigh_put(u, e);
    return neigh_store(c, u);
}

int udpdk_gpu_neigh_geometry(uint32_t *learn_frames_per_block, uint32_t *resolve_per_block)
{
    if (!learn_frames_per_block || !resolve_per_block) return -EINVAL;
    *learn_frames_per_block = NL_TILE;
    *resolve_per_block = NR_TILE;
    return 0;
}

int udpdk_gpu_neigh_class(const udpdk_neigh_cfg_t *cfg, uint32_t dst_ip, uint32_t *next_hop, uint8_t *mac_out)
{
    if (!cfg || !next_hop || !mac_out) return -EINVAL;
    uint32_t s_lo, s_hi, lo, hi;
    mac_words(cfg->src_mac, &s_lo, &s_hi);
    const uint32_t cls = neigh_class(cfg->src_ip, cfg->netmask, cfg->gateway, s_lo, s_hi, dst_ip, next_hop, &lo, &hi);
    memcpy(mac_out, &lo, 4);
    memcpy(mac_out + 4, &hi, 2);
    return (int)cls;
}

int udpdk_gpu_neigh_learn(udpdk_gpu_ctx *c, const udpdk_neigh_cfg_t *cfg, const udpdk_rx_batch_t *bt,
                          const uint32_t *meta_dev, uint32_t now)
{
    return stage_form(c, 0, &CtlWs::nlearn, neigh_learn_check(c, cfg, bt, meta_dev), neigh_learn_enqueue, cfg, bt,
                      meta_dev, now);
}

int udpdk_gpu_pipe_neigh_learn(udpdk_gpu_ctx *c, int pipe, const udpdk_neigh_cfg_t *cfg,
                               const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, uint32_t now)
{
    return stage_form(c, on_pipe(pipe), &CtlWs::nlearn, neigh_learn_check(c, cfg, bt, meta_dev), neigh_learn_enqueue,
                      cfg, bt, meta_dev, now);
}

int udpdk_gpu_neigh_learn_stats(udpdk_gpu_ctx *c, udpdk_neigh_learn_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::nlearn, st, neigh_learn_stats_out);
}

int udpdk_gpu_pipe_neigh_learn_stats(udpdk_gpu_ctx *c, int pipe, udpdk_neigh_learn_stats_t *st)
{
    return stage_stats(c, on_pipe(pipe), &CtlWs::nlearn, st, neigh_learn_stats_out);
}

int udpdk_gpu_neigh_resolve(udpdk_gpu_ctx *c, const udpdk_neigh_cfg_t *cfg, const uint32_t *dst_ip_dev,
                            const int32_t *sockfd_dev, uint32_t n, uint32_t now, const udpdk_neigh_out_t *o)
{
    return stage_form(c, 0, &CtlWs::nresolve, neigh_resolve_check(c, cfg, dst_ip_dev, sockfd_dev, o),
                      neigh_resolve_enqueue, cfg, dst_ip_dev, sockfd_dev, n, now, o);
}

int udpdk_gpu_neigh_resolve_stats(udpdk_gpu_ctx *c, udpdk_neigh_resolve_stats_t *st)
{
    return stage_stats(c, 0, &CtlWs::nresolve, st, neigh_resolve_stats_out);
}

} // extern "C"
