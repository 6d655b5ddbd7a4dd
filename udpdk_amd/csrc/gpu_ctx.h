// gpu_ctx.h — the per-device context behind the C ABI of include/udpdk_gpu.h, shared by the host
// translation units (udpdk_gpu.hip: the context itself, RX, TX; udpdk_gpu_ctl.hip: the control-plane
// stages): owning buffers, result slots, the stages' workspaces, the pipes, and the few helpers every
// stage's entry points start and end with. Internal: nothing here is exported (libudpdk_amd.map).
#pragma once
#include <hip/hip_runtime.h>

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "rx_plan.h"
#include "rx_filter.h"
#include "rx_balance.h"
#include "rx_peer.h"
#include "rx_mcast.h"
#include "icmp_reply.h"
#include "icmp_error.h"
#include "arp_reply.h"
#include "igmp_reply.h"
#include "neigh.h"

namespace udpdk {

struct DevResult {
    unsigned long long counters[UDPDK_N_COUNTERS];
    uint32_t total;
    uint32_t pad;
    // speculative single-lane compaction: word k = max of (call epoch << 32 | ~tile) over the
    // tiles t = k mod 64 that did not deliver all their frames (rx_classify); the smallest tile
    // over the 64 words is the call's first such tile (64 words: a batch with many short tiles
    // does not serialise on one address)
    unsigned long long nonfull[UDPDK_SPEC_WORDS];
};

// Per-call kernel timing: start/stop events carried by the kernel dispatches themselves
// (hipExtLaunchKernelGGL), so timing adds no marker packets between back-to-back kernels.
constexpr int TIMED_KERNELS = 3;  // classify, scan, scatter (single-lane path: compact)
struct TimingSet {
    hipEvent_t ev[2 * TIMED_KERNELS];
    bool used[TIMED_KERNELS];
};

int hip_rc(udpdk_gpu_ctx *c, hipError_t e);    // 0, or -EIO with c->last_err set

// Device (Pinned = false) or pinned host (Pinned = true) memory of `cap` elements that its holder
// owns: sized by ensure(), freed by release() (or, at the latest, with the holder). Not copyable:
// the workspaces below are held by value and pointed at (udpdk_gpu_ctx::flt_last and the like).
template <typename T, bool Pinned>
struct Buf {
    T *p = nullptr;
    size_t cap = 0;                            // elements
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    // Room for `count` elements. Nothing happens while they fit; otherwise the old memory is freed
    // (which synchronises the device, so only ever on growth) and exactly `count` are allocated,
    // not zeroed. On failure the buffer is left empty.
    int ensure(udpdk_gpu_ctx *c, size_t count, unsigned host_flags = hipHostMallocDefault)
    {
        if (cap >= count) return 0;
        T *old = p;
        p = nullptr;
        cap = 0;
        void *q = nullptr;
        int rc;
        if (old && (rc = hip_rc(c, Pinned ? hipHostFree(old) : hipFree(old)))) return rc;
        if ((rc = hip_rc(c, Pinned ? hipHostMalloc(&q, count * sizeof(T), host_flags) : hipMalloc(&q, count * sizeof(T)))))
            return rc;
        p = static_cast<T *>(q);
        cap = count;
        return 0;
    }
    void release()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

template <typename... B> void release_all(B &...b) { (b.release(), ...); }

// A stage's device result and its pinned mirror. Two ways to read it: fetch() copies and waits
// (the context-stream *_stats calls); enqueue_fetch() leaves the copy on the stage's stream, and
// the mirror is read once that stream was waited for (the pipe forms).
template <typename R>
struct ResultSlot {
    DevBuf<R> dev;
    PinnedBuf<R> host;
    bool ran = false;                          // a stage was enqueued (-ENOENT from *_stats until then)
    int ensure(udpdk_gpu_ctx *c)
    {
        const int rc = dev.ensure(c, 1);
        return rc ? rc : host.ensure(c, 1);
    }
    int enqueue_fetch(udpdk_gpu_ctx *c, hipStream_t st)
    {
        return hip_rc(c, hipMemcpyAsync(host.p, dev.p, sizeof(R), hipMemcpyDeviceToHost, st));
    }
    int fetch(udpdk_gpu_ctx *c, hipStream_t st)
    {
        const int rc = enqueue_fetch(c, st);
        return rc ? rc : hip_rc(c, hipStreamSynchronize(st));
    }
    void release() { release_all(dev, host); }
};

// Workspace of a lane-removal stage (lane_stage: the drop filter, the balance, the peer filter, the
// membership filter),
// lazily sized: per stage one per pipe for the sticky mode and one for the explicit calls.
struct FilterWs {
    DevBuf<unsigned long long> mask;
    DevBuf<uint32_t> row, base;
    DevBuf<uint32_t> pkt, off;                 // sticky mode: the filtered set before it goes back
                                               // into the caller's buffers
    ResultSlot<FilterResult> res;
    hipStream_t stream = nullptr;              // of the last run
    uint32_t out_cap = 0;
    void release() { release_all(mask, row, base, pkt, off, res); }
};

// Workspace of the reuse-port balance stage (rx_balance.hip): the compaction workspace, the
// frames' choices and the count of balanced frames.
struct BalanceWs : FilterWs {
    DevBuf<uint32_t> chosen;
    DevBuf<uint32_t> cnt;                      // frames balanced
    PinnedBuf<uint32_t> h_cnt;
    void release()
    {
        FilterWs::release();
        release_all(chosen, cnt, h_cnt);
    }
};

// Workspace of the reply plan (tx_reply.hip), lazily sized; one per context (the context stream).
struct ReplyWs {
    DevBuf<uint32_t> row;
    DevBuf<unsigned long long> base;
    ResultSlot<ReplyResult> res;
    void release() { release_all(row, base, res); }
};

// Workspace of the segment plan (tx_segment.hip), lazily sized; one per context (the context stream).
struct SegWs {
    DevBuf<uint32_t> row, send_base;
    DevBuf<unsigned long long> base;
    ResultSlot<SegResult> res;
    void release() { release_all(row, send_base, base, res); }
};

// Workspace of the ICMP reply stage (icmp_reply.hip), lazily sized by the context's max_frames: one
// for the context stream (udpdk_gpu_icmp_reply) and one per pipe (udpdk_gpu_pipe_icmp_reply).
struct IcmpWs {
    DevBuf<IcmpEntry> cand;
    DevBuf<uint32_t> row;                      // the rows, then ubase and rbase
    DevBuf<unsigned long long> bbase;
    ResultSlot<IcmpResult> res;
    void release() { release_all(cand, row, bbase, res); }
};

// The ICMP error stage (icmp_error.hip) keeps only its counters: one for the context stream
// (udpdk_gpu_icmp_errors) and one per pipe (udpdk_gpu_pipe_icmp_errors).
struct IcmpErrWs {
    ResultSlot<IcmpErrResult> res;
    void release() { res.release(); }
};

// Workspace of a stage of fanin_stage.h's shape with candidates of type E, lazily sized by the
// context's max_frames: the ARP reply stage (arp_reply.hip) and the neighbour learn stage (neigh.hip)
// have one for the context stream and one per pipe, the neighbour resolve stage one (the context
// stream).
template <typename E, typename R>
struct FaninWs {
    DevBuf<E> cand;
    DevBuf<uint32_t> row;                      // the rows, then rbase
    DevBuf<unsigned long long> fuse;           // fan-in words, zeroed once: every launch leaves zeros
    ResultSlot<R> res;
    void release() { release_all(cand, row, fuse, res); }
};
using ArpWs = FaninWs<ArpEntry, ArpResult>;
using NeighLearnWs = FaninWs<uint4, NeighLearnResult>;
using NeighResolveWs = FaninWs<uint2, NeighResolveResult>;

// Workspace of the IGMP query responder (igmp_reply.hip), lazily sized by the context's max_frames: one
// for the context stream (udpdk_gpu_igmp_reply) and one per pipe (udpdk_gpu_pipe_igmp_reply).
struct IgmpQWs {
    DevBuf<uint32_t> row;                      // the rows
    DevBuf<uint32_t> bits;                     // the answer set, zeroed once: every launch leaves zeros
    DevBuf<unsigned long long> fuse;           // fan-in words, zeroed once: every launch leaves zeros
    ResultSlot<IgmpQResult> res;
    void release() { release_all(row, bits, fuse, res); }
};

// The control-plane stages' workspaces (udpdk_gpu_ctl.hip): one set for the context stream
// (udpdk_gpu_icmp_reply, ...) and one per pipe for that pipe's stream (udpdk_gpu_pipe_icmp_reply, ...;
// the resolve stage has no pipe form and its workspace stays empty there).
struct CtlWs {
    IcmpWs icmp;
    IcmpErrWs icmp_err;
    ArpWs arp;
    IgmpQWs igmp;
    NeighLearnWs nlearn;
    NeighResolveWs nresolve;
    void release() { release_all(icmp, icmp_err, arp, igmp, nlearn, nresolve); }
};

// The sticky lane-removal stages, in the order rx_on_pipe applies them.
enum { ST_DROP, ST_BALANCE, ST_PEER, ST_MCAST, N_STICKY };

// One RX pipe = a stream and the per-call workspace. With pipelining depth d > 1, consecutive
// udpdk_gpu_rx calls rotate over d pipes, so one batch's prologue, tail and compaction overlap
// the other batches' streaming phases (the calls are independent: distinct batches and output
// buffers). Depth 3 is the measured optimum for 1 M x 64 B (tools/probe/classify_probe: classify
// + compaction 22.2 / 19.0 / 15.5 / 17.4 us per batch at 1 / 2 / 3 / 4 streams; 4 streams exceed
// the box's 4 hardware queues with the context stream's own traffic).
struct Pipe {
    hipStream_t stream = nullptr;
    DevBuf<uint32_t> hist, partial;
    DevBuf<uint32_t> base;                    // [tiles][lanes] absolute positions (rx_scan_cols)
    DevBuf<unsigned long long> agg;           // rx_scan_cols look-back words, one per lane block
    DevBuf<uint32_t> ticket;                  // rx_scan_cols lane-block tickets
    uint32_t epoch = 0;                       // rx_scan_cols calls on this pipe (look-back tag)
    uint32_t spec_epoch = 0;                  // speculative compaction calls (DevResult::nonfull tag)
    DevBuf<unsigned long long> fuse;          // rx_classify fused-completion fan-in words (zeroed)
    DevBuf<uint32_t> tile_cnt;
    ResultSlot<DevResult> res;                // counters, total; the mirror is filled by enqueue_result
    hipEvent_t tail = nullptr;                // join point for udpdk_gpu_join
    bool dirty = false;                       // work enqueued since the last join
    uint32_t last_tiles = 0;                  // tiles of this pipe's last call (counter rows)
    uint32_t last_lane_cap = 0;
    FilterWs flt;                             // sticky drop filter
    BalanceWs bal;                            // sticky reuse-port balance
    FilterWs peer;                            // sticky peer filter
    FilterWs mcast;                           // sticky membership filter
    FilterWs *const sticky[N_STICKY] = {&flt, &bal, &peer, &mcast};
    bool sticky_ran[N_STICKY] = {};           // this pipe's last call ran the stage
    const udpdk_rx_stats_t *stats_of = nullptr;   // the stats block read_result filled last, and what each
    uint32_t removed[N_STICKY] = {};              // stage removed in that call (udpdk_gpu_rx_removed,
                                                  // udpdk_gpu_rx_peer_removed, udpdk_gpu_rx_mcast_removed)
    // host-resident batches (udpdk_gpu_rx_host[_async]): staging, lazily sized
    DevBuf<uint8_t> st_frames_d, st_desc_d, st_out_d;
    PinnedBuf<uint8_t> st_frames_h, st_desc_h;
    udpdk_rx_stats_t *host_stats = nullptr;   // outstanding async host call: where its stats go
    udpdk_rx_batch_t staged{};                // device view of the last host batch staged here
    const uint32_t *staged_meta = nullptr;    // and its verdict words
    CtlWs ctl;                                // the control-plane stages on this pipe's stream
    void release()
    {
        release_all(hist, partial, base, agg, ticket, fuse, tile_cnt, res, flt, bal, peer, mcast, st_frames_d,
                    st_desc_d, st_out_d, st_frames_h, st_desc_h, ctl);
    }
};
constexpr int MAX_PIPES = 4;
constexpr size_t FUSE_BYTES = 128u * UDPDK_FUSE_LINES;   // one 128-B line per fan-in / repair word

} // namespace udpdk

struct udpdk_gpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;             // = pipes[0].stream: the context stream
    int last_err = 0;
    uint32_t max_frames = 0, max_lanes = 0;

    // bind snapshot (device)
    udpdk::DevBuf<uint4> port_tab;      // [65536]
    udpdk::DevBuf<uint2> binds;
    udpdk::DevBuf<uint4> slots;
    uint32_t n_slots = 0;
    uint32_t n_lanes = 1, lane_mask = 0xFFFFFFFFu, key_bits = 0, max_fanout = 0;
    // the bound ports when there are at most UDPDK_INLINE_PORTS (RxArgs::inl)
    uint32_t inl = 0, n_inl = 0, inl_port[UDPDK_INLINE_PORTS] = {};
    uint4 inl_ent[UDPDK_INLINE_PORTS] = {};
    udpdk::RxKnobs knobs;          // the environment knobs, parsed once at creation (rx_plan.h)
    // Kernel hints (pinned host memory the kernels write, RxArgs::hint): the call sequence number
    // of the last call that ran a tail pass / had a tile before the last not full. The single-lane
    // path takes rx_classify<1> and the fused completion while neither was seen in the last
    // UDPDK_HINT_WINDOW calls; both forms are exact for any batch, the hint only picks the faster.
    udpdk::PinnedBuf<uint32_t> hint;
    uint32_t rx_seq = 0;
    bool have_snapshot = false;

    // RX workspace, one set per pipe
    udpdk::Pipe pipes[udpdk::MAX_PIPES];
    int depth = 1;                            // udpdk_gpu_pipeline_depth
    uint64_t rx_calls = 0;
    int last_pipe = -1;                       // pipe of the last udpdk_gpu_rx (-1: none yet)
    udpdk::RxCaps caps{};                     // entries of each pipe's hist / partial / tile_cnt

    uint64_t host_calls = 0;                  // udpdk_gpu_rx_host_async calls (pipe choice)

    uint32_t drop_flags = 0;                  // udpdk_gpu_rx_drop: UDPDK_RX_DROP_* (0: no stage)
    udpdk::FilterWs xflt;                     // explicit udpdk_gpu_rx_filter calls
    udpdk::FilterWs *flt_last = nullptr;      // the last filter run (udpdk_gpu_rx_drop_stats)
    bool bal_on = false;                      // udpdk_gpu_rx_balance: the sticky balance stage
    udpdk::DevBuf<uint8_t> bal_rp;            // [max_lanes] its lane flags (zero past what was given)
    udpdk::DevBuf<uint32_t> bal_ktab;         // key windows of the default RSS configuration (no
                                              // udpdk_gpu_rss_config on this context)
    udpdk::BalanceWs xbal;                    // explicit udpdk_gpu_rx_balance_select calls
    udpdk::BalanceWs *bal_last = nullptr;     // the last balance run (udpdk_gpu_rx_balance_stats)
    bool peer_on = false;                     // udpdk_gpu_rx_peer: the sticky peer filter
    udpdk::DevBuf<uint2> peer_tab;            // [max_lanes] its records (off past what was given)
    udpdk::FilterWs xpeer;                    // explicit udpdk_gpu_rx_peer_select calls
    udpdk::FilterWs *peer_last = nullptr;     // the last peer filter run (udpdk_gpu_rx_peer_stats)
    bool mcast_on = false;                    // udpdk_gpu_rx_mcast: the sticky membership filter
    udpdk::DevBuf<uint8_t> mcast_mc;          // [max_lanes] its lane flags (zero past what was given)
    udpdk::DevBuf<uint2> mcast_tab;           // its membership table, 1 << mcast_lg slots
    uint32_t mcast_lg = 0;
    udpdk::FilterWs xmcast;                   // explicit udpdk_gpu_rx_mcast_select calls
    udpdk::FilterWs *mcast_last = nullptr;    // the last membership filter run (udpdk_gpu_rx_mcast_stats)
    udpdk::ReplyWs rpl;                       // udpdk_gpu_tx_reply_plan / udpdk_gpu_tx_reply
    udpdk::SegWs seg;                         // udpdk_gpu_tx_segment_plan / udpdk_gpu_tx_segment
    udpdk::CtlWs ctl;                         // the control-plane stages on the context stream
    udpdk::DevBuf<uint32_t> neigh_tab;        // udpdk_gpu_neigh_create: four dwords per entry
    uint32_t neigh_entries = 0;               // 0: no table

    unsigned long long *dbg = nullptr;        // diagnostic stamp buffer (UDPDK_STAMPS builds)
    udpdk::Reasm *reasm = nullptr;            // udpdk_gpu_frag_table_create
    // receive-side scaling (udpdk_gpu_rss_config)
    bool rss_ready = false;
    udpdk::RssArgs rss{};
    udpdk::DevBuf<uint16_t> rss_reta;
    udpdk::DevBuf<uint32_t> rss_ktab;         // [12][256] key windows
    udpdk::DevBuf<uint8_t> rss_qid;
    udpdk::DevBuf<uint32_t> rss_hist, rss_partial, rss_total;
    udpdk::DevBuf<unsigned long long> rss_fuse;   // rss_hash fan-in words (fused queue bases)
    bool rss_no_fuse = false;                 // UDPDK_RSS_FUSE=0 (tests, A/B): the rss_base launch
    bool rss_trace = false;                   // UDPDK_RSS_TRACE (diagnostic): the form of every call on stderr

    // timing
    uint32_t timing_every = 0;                // 0 off, N: events on every Nth call
    uint64_t timing_calls = 0;
    udpdk::TimingSet *sets = nullptr;
    int n_sets_used = 0;
    double ms[UDPDK_N_KERNEL_IDS] = {};
    uint32_t launches[UDPDK_N_KERNEL_IDS] = {};

    // All the memory above (udpdk_gpu_ctx_destroy; whatever is missing here goes with the context)
    void release()
    {
        for (udpdk::Pipe &P : pipes) P.release();
        udpdk::release_all(port_tab, binds, slots, hint, xflt, bal_rp, bal_ktab, xbal, peer_tab, xpeer, mcast_mc,
                           mcast_tab, xmcast, rpl, seg, ctl, neigh_tab,
                           rss_reta, rss_ktab, rss_qid, rss_hist, rss_partial, rss_total, rss_fuse);
    }
};

#define HIPC(ctx, expr)                                                      \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            if (ctx) (ctx)->last_err = (int)e_;                              \
            return -EIO;                                                     \
        }                                                                    \
    } while (0)

namespace udpdk {

// Range of the frames buffer resource. Buffer loads are range-checked per dword (a dword is
// returned only if it ends within the range, zero otherwise, with no memory access:
// tools/probe/range_probe.hip) and the RX kernels load at byte-aligned frame offsets, so a
// dword holding the last frame bytes may end up to 3 bytes past frames_bytes: the range is
// frames_bytes + 3 rounded up to a dword, inside the UDPDK_GPU_FRAMES_TAILROOM bytes the frames
// buffer must keep readable after frames_bytes (udpdk_gpu.h).
uint32_t frames_rsrc_bytes(uint64_t frames_bytes);

// Every stream of the context waited for.
int sync_all(udpdk_gpu_ctx *c);

// How a call that works on the context stream starts, once its arguments have passed: select the
// device and, with pipelining on, order the other pipes' work before it.
int on_ctx_stream(udpdk_gpu_ctx *c);

// The context-stream form of a *_stats call: the stage's result into its mirror, waited for.
template <typename R>
int ctx_result(udpdk_gpu_ctx *c, ResultSlot<R> &slot)
{
    if (!slot.ran) return -ENOENT;
    HIPC(c, hipSetDevice(c->device));
    return slot.fetch(c, c->stream);
}

} // namespace udpdk
