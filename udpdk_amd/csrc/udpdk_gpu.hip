// udpdk_gpu.hip — host side of the C ABI declared in include/udpdk_gpu.h.
//
// Owns the per-device context (stream, bind snapshot, workspace, pinned readback) and enqueues
// the RX and TX kernels. No hidden synchronisation on the RX/TX enqueue path: everything stays
// on the context stream, so a caller may capture udpdk_gpu_rx into a hipGraph.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "gpu_ctx.h"
#include "rss_host.h"

using namespace udpdk;

namespace {

constexpr int EVENT_SETS = 256;   // timed calls buffered between two timing reads
constexpr size_t HINT_BYTES = 192u;
constexpr uint32_t RSS_FUSE_MAX_ENTRIES = 8192u;   // rss_hash's last workgroup scans <= this many
#ifndef UDPDK_HINT_WINDOW
#define UDPDK_HINT_WINDOW 8u       // calls (as far as the GPU got) a tail pass / a not-full tile
                                   // keeps the other form on
#endif

} // namespace

// gpu_ctx.h's helpers
namespace udpdk {

uint32_t frames_rsrc_bytes(uint64_t frames_bytes)
{
    return (uint32_t)std::min<uint64_t>((frames_bytes + 3 + 3) & ~3ull, 0xFFFFFFFCull);
}

int hip_rc(udpdk_gpu_ctx *c, hipError_t e)
{
    HIPC(c, e);
    return 0;
}

int sync_all(udpdk_gpu_ctx *c)
{
    for (Pipe &P : c->pipes)
        if (P.stream) HIPC(c, hipStreamSynchronize(P.stream));
    return 0;
}

} // namespace udpdk

namespace {

int fold_timing(udpdk_gpu_ctx *c)
{
    if (!c->n_sets_used) return 0;
    for (Pipe &P : c->pipes) HIPC(c, hipStreamSynchronize(P.stream));
    static const int kid[TIMED_KERNELS] = {UDPDK_K_RX_CLASSIFY, UDPDK_K_RX_SCAN, UDPDK_K_RX_SCATTER};
    for (int i = 0; i < c->n_sets_used; ++i) {
        for (int k = 0; k < TIMED_KERNELS; ++k) {
            if (!c->sets[i].used[k]) continue;
            float ms = 0;
            HIPC(c, hipEventElapsedTime(&ms, c->sets[i].ev[2 * k], c->sets[i].ev[2 * k + 1]));
            c->ms[kid[k]] += ms;
            c->launches[kid[k]]++;
        }
    }
    c->n_sets_used = 0;
    return 0;
}

// rx_classify<g, mr, pol>: g tail chunk groups in flight (1, 2), round-ahead descriptors, memory policy
using ClassifyKernel = void (*)(RxArgs);
ClassifyKernel classify_form(int g, int mr, int pol)
{
    static const ClassifyKernel form[2][2][2] = {
        {{rx_classify<1, 0, 0>, rx_classify<1, 0, 1>}, {rx_classify<1, 1, 0>, rx_classify<1, 1, 1>}},
        {{rx_classify<2, 0, 0>, rx_classify<2, 0, 1>}, {rx_classify<2, 1, 0>, rx_classify<2, 1, 1>}}};
    return form[g - 1][mr][pol];
}

// Launch on the context stream; with a timing set, kernel k's dispatch carries the set's start
// event (first=true) and/or stop event (last=true).
template <typename K, typename... A>
hipError_t launch(hipStream_t st, TimingSet *ts, int k, bool first, bool last, K kern, dim3 grid,
                  dim3 block, uint32_t lds, A... args)
{
    if (ts) {
        ts->used[k] = true;
        hipExtLaunchKernelGGL(kern, grid, block, lds, st, first ? ts->ev[2 * k] : nullptr,
                              last ? ts->ev[2 * k + 1] : nullptr, 0u, args...);
    } else {
        hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    }
    return hipGetLastError();
}

// One kernel of a single-launch call (rx_gather, tx_build); with timing on, between two events
// the call waits for, its time added to kernel `kid`.
template <typename K, typename A>
int launch_timed(udpdk_gpu_ctx *c, hipStream_t st, int kid, K kern, dim3 grid, dim3 block, const A &args)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing_every) {
        HIPC(c, hipEventCreate(&e0));
        HIPC(c, hipEventCreate(&e1));
        HIPC(c, hipEventRecord(e0, st));
    }
    hipLaunchKernelGGL(kern, grid, block, 0, st, args);
    HIPC(c, hipGetLastError());
    if (c->timing_every) {
        HIPC(c, hipEventRecord(e1, st));
        HIPC(c, hipEventSynchronize(e1));
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, e0, e1));
        c->ms[kid] += ms;
        c->launches[kid]++;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    return 0;
}

// Order everything enqueued on the other pipes before what comes next on the context stream.
int join_pipes(udpdk_gpu_ctx *c)
{
    for (int i = 1; i < MAX_PIPES; ++i) {
        Pipe &P = c->pipes[i];
        // an event record + stream wait costs host and GPU time even on an idle stream: only
        // pipes with work since their last join
        if (!P.stream || !P.dirty) continue;
        HIPC(c, hipEventRecord(P.tail, P.stream));
        HIPC(c, hipStreamWaitEvent(c->stream, P.tail, 0));
        P.dirty = false;
    }
    return 0;
}

} // namespace

int udpdk::on_ctx_stream(udpdk_gpu_ctx *c)
{
    HIPC(c, hipSetDevice(c->device));
    return c->depth > 1 ? join_pipes(c) : 0;
}

namespace {

// One lane-removal stage over a lane set on stream st: the stage's mark kernel fills the keep masks
// and rows, then rx_filter_base and rx_filter_write compact (rx_filter.h). `mark` gets the filled
// FilterArgs, may adjust them, and enqueues whatever the stage runs before the compaction, ending
// with launch_mark of its kernel.
template <typename Mark>
int lane_stage(udpdk_gpu_ctx *c, FilterWs &W, hipStream_t st, const udpdk_rx_lanes_t *in, uint32_t *off_out,
               uint32_t *pkt_out, uint32_t out_cap, Mark mark)
{
    const uint32_t tiles = ceil_div(in->lane_cap, FLT_TILE);
    int rc;
    if ((rc = W.mask.ensure(c, (size_t)tiles * FLT_CHUNKS + 1)) || (rc = W.row.ensure(c, (size_t)tiles * FLT_ROW + 1)) ||
        (rc = W.base.ensure(c, (size_t)tiles + 1)) || (rc = W.res.ensure(c)))
        return rc;
    FilterArgs fa;
    fa.meta = in->meta_dev;
    fa.lane_off = in->lane_off_dev;
    fa.lane_pkt = in->lane_pkt_dev;
    fa.lane_off_out = off_out;
    fa.lane_pkt_out = pkt_out;
    fa.mask = W.mask;
    fa.row = W.row;
    fa.base = W.base;
    fa.res = W.res.dev;
    fa.n = in->n;
    fa.lane_cap = in->lane_cap;
    fa.n_lanes = in->n_lanes;
    fa.flags = 0;
    fa.out_cap = out_cap;
    fa.n_tiles = tiles;
    if ((rc = mark(fa))) return rc;
    hipLaunchKernelGGL(rx_filter_base, dim3(1), dim3(FLT_BASE_BLOCK), 0, st, fa);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(rx_filter_write, dim3(tiles + ceil_div(in->n_lanes + 1u, (uint32_t)FLT_BLOCK)),
                       dim3(FLT_BLOCK), 0, st, fa);
    HIPC(c, hipGetLastError());
    W.stream = st;
    W.out_cap = out_cap;
    return 0;
}

// A stage's mark kernel, one workgroup per tile of `f` (the FilterArgs inside `args`); no launch
// for an empty grid.
template <typename K, typename A>
int launch_mark(udpdk_gpu_ctx *c, hipStream_t st, K kern, const A &args, const FilterArgs &f)
{
    if (!f.n_tiles) return 0;
    hipLaunchKernelGGL(kern, dim3(f.n_tiles), dim3(FLT_BLOCK), 0, st, args);
    HIPC(c, hipGetLastError());
    return 0;
}

// One sticky stage of rx_on_pipe, on the pipe's stream: `enqueue` runs the stage from the caller's
// buffers into the workspace's off / pkt, and rx_filter_copy puts what it kept back into the
// caller's buffers.
template <typename Enqueue>
int sticky_stage(udpdk_gpu_ctx *c, Pipe &P, int stage, const udpdk_rx_out_t *o, Enqueue enqueue)
{
    FilterWs &W = *P.sticky[stage];
    const uint32_t S = c->n_lanes;
    const uint32_t tiles = ceil_div(o->lane_cap, FLT_TILE);
    int rc;
    if ((rc = W.pkt.ensure(c, (size_t)o->lane_cap + 1)) || (rc = W.off.ensure(c, (size_t)S + 1)) ||
        (rc = enqueue(W.off.p, W.pkt.p)))
        return rc;
    hipLaunchKernelGGL(rx_filter_copy, dim3(tiles + ceil_div(S + 1u, (uint32_t)FLT_BLOCK)), dim3(FLT_BLOCK), 0,
                       P.stream, (const uint32_t *)W.off, (const uint32_t *)W.pkt, (const FilterResult *)W.res.dev,
                       o->lane_off_dev, o->lane_pkt_dev, S, o->lane_cap, tiles);
    HIPC(c, hipGetLastError());
    P.sticky_ran[stage] = true;
    return 0;
}

} // namespace

extern "C" {

int udpdk_gpu_abi_version(void) { return UDPDK_GPU_ABI_VERSION; }

int udpdk_gpu_device_count(int *count)
{
    if (!count) return -EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return 0;
}

int udpdk_gpu_rx_geometry(uint32_t n, uint32_t n_lanes, uint32_t *tile_frames, uint32_t *n_tiles)
{
    if (!tile_frames || !n_tiles || n_lanes == 0) return -EINVAL;
    geometry(n, n_lanes, tile_frames, n_tiles);
    return 0;
}

int udpdk_gpu_ctx_create(int device, uint32_t max_frames, uint32_t max_lanes, udpdk_gpu_ctx **out)
{
    if (!out || max_lanes == 0 || max_lanes > UDPDK_GPU_MAX_LANES || max_frames == 0) return -EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -ENODEV;
    udpdk_gpu_ctx *c = new (std::nothrow) udpdk_gpu_ctx();
    if (!c) return -ENOMEM;
    c->device = device;
    c->max_frames = max_frames;
    c->max_lanes = max_lanes;
    c->knobs = rx_knobs_from_env();
    c->caps = rx_caps(max_frames, max_lanes, c->knobs.geo_cap);
    int rc = -EIO;
    do {
        if (hipSetDevice(device) != hipSuccess) break;
        bool ok = true;
        for (Pipe &P : c->pipes) {
            ok = ok && hipStreamCreateWithFlags(&P.stream, hipStreamNonBlocking) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&P.tail, hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) break;
        c->stream = c->pipes[0].stream;
        if (c->port_tab.ensure(c, UDPDK_UDP_PORTS)) break;
        if (hipMemset(c->port_tab, 0, UDPDK_UDP_PORTS * sizeof(uint4)) != hipSuccess) break;
        for (Pipe &P : c->pipes) {
            ok = ok && !P.hist.ensure(c, c->caps.hist_cap);
            ok = ok && !P.partial.ensure(c, c->caps.partial_cap);
            ok = ok && !P.base.ensure(c, c->caps.hist_cap);
            // one look-back word per lane block: down to one lane per block when a batch has so
            // many tiles that a column chunk holds a single lane (rx_scan_cols' lb = 0)
            ok = ok && !P.agg.ensure(c, (size_t)max_lanes + 1);
            ok = ok && hipMemset(P.agg, 0, ((size_t)max_lanes + 1) * 8) == hipSuccess;
            ok = ok && !P.ticket.ensure(c, 64 / 4);
            ok = ok && hipMemset(P.ticket, 0, 64) == hipSuccess;
            ok = ok && !P.tile_cnt.ensure(c, (size_t)c->caps.tiles_cap * UDPDK_N_COUNTERS);
            ok = ok && !P.res.dev.ensure(c, 1);
            ok = ok && hipMemset(P.res.dev, 0, sizeof(DevResult)) == hipSuccess;
            ok = ok && !P.res.host.ensure(c, 1);
            ok = ok && !P.fuse.ensure(c, FUSE_BYTES / 8);
            ok = ok && hipMemset(P.fuse, 0, FUSE_BYTES) == hipSuccess;
        }
        // fine-grained (coherent) host memory: the kernels' hint stores go straight to it
        ok = ok && !c->hint.ensure(c, HINT_BYTES / 4, hipHostMallocCoherent | hipHostMallocMapped);
        if (ok) {
            // a fresh context starts on the two-launch form (as if call 1 had a tile not full):
            // the fused completion's rewrite of a not-full call is one workgroup's work
            memset(c->hint, 0, HINT_BYTES);
            c->hint[UDPDK_HINT_NONFULL] = 1u;
        }
        if (!ok) break;
        // rx_classify needs up to 141 KiB of dynamic LDS (16384 lanes, 8192-frame tiles)
        // (+ the span sweep's ring, one-round tiles only)
        const int cls_lds = (int)std::min<uint32_t>(
            std::max(classify_lds_bytes(UDPDK_GPU_MAX_LANES, RX_TILE_MAX),
                     classify_lds_bytes(UDPDK_GPU_MAX_LANES, RX_ROUND) + SPAN_LDS_BYTES),
            160u * 1024u - 1024u);   // static LDS besides
        for (int g = 1; g <= 2 && ok; ++g)
            for (int mr = 0; mr <= 1 && ok; ++mr)
                ok = hipFuncSetAttribute((const void *)classify_form(g, mr, c->knobs.policy),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, cls_lds) == hipSuccess;
        if (!ok) break;
        if (hipFuncSetAttribute((const void *)rx_scatter, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)scatter1_lds_bytes(UDPDK_GPU_MAX_LANES)) != hipSuccess) break;
        if (hipFuncSetAttribute((const void *)rx_scatterw<SCATTER_WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                scatterw_lds_bytes(SCATTERW_MAX_LANES)) != hipSuccess) break;
        if (hipFuncSetAttribute((const void *)rx_scatterw<2 * SCATTER_WAVES>,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                scatterw_lds_bytes(SCATTERW_MAX_LANES, 2 * SCATTER_WAVES)) != hipSuccess) break;
        // rx_scan_top's lane totals: 4 B per lane, up to UDPDK_GPU_MAX_LANES (64 KiB)
        if (hipFuncSetAttribute((const void *)rx_scan_top, hipFuncAttributeMaxDynamicSharedMemorySize,
                                4 * UDPDK_GPU_MAX_LANES) != hipSuccess) break;
        rc = 0;
    } while (0);
    if (rc) {
        (void)hipGetLastError();
        udpdk_gpu_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

int udpdk_gpu_ctx_destroy(udpdk_gpu_ctx *c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    for (Pipe &P : c->pipes)
        if (P.stream) (void)hipStreamSynchronize(P.stream);
    reasm_destroy(c->reasm);
    c->reasm = nullptr;
    c->release();
    for (Pipe &P : c->pipes)
        if (P.tail) (void)hipEventDestroy(P.tail);
    if (c->sets) {
        for (int i = 0; i < EVENT_SETS; ++i)
            for (int k = 0; k < 2 * TIMED_KERNELS; ++k) (void)hipEventDestroy(c->sets[i].ev[k]);
        delete[] c->sets;
    }
    for (Pipe &P : c->pipes)
        if (P.stream) (void)hipStreamDestroy(P.stream);
    delete c;
    return 0;
}

int udpdk_gpu_sync(udpdk_gpu_ctx *c)
{
    if (!c) return -EINVAL;
    return sync_all(c);
}

int udpdk_gpu_join(udpdk_gpu_ctx *c)
{
    if (!c) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    return join_pipes(c);
}

int udpdk_gpu_pipeline_depth(udpdk_gpu_ctx *c, int depth)
{
    if (!c || depth < 1 || depth > MAX_PIPES) return -EINVAL;
    int rc = sync_all(c);
    if (rc) return rc;
    c->depth = depth;
    return 0;
}

int udpdk_gpu_last_hip_error(const udpdk_gpu_ctx *c) { return c ? c->last_err : 0; }

void *udpdk_gpu_stream(udpdk_gpu_ctx *c) { return c ? (void *)c->stream : nullptr; }

int udpdk_gpu_alloc(udpdk_gpu_ctx *c, size_t bytes, void **dev)
{
    if (!c || !dev) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    // round up so 16-byte chunk loads past the last frame stay inside the allocation
    const size_t b = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
    if (hipMalloc(dev, b) != hipSuccess) { (void)hipGetLastError(); *dev = nullptr; return -ENOMEM; }
    return 0;
}

int udpdk_gpu_free(udpdk_gpu_ctx *c, void *dev)
{
    if (!c) return -EINVAL;
    if (dev) HIPC(c, hipFree(dev));
    return 0;
}

int udpdk_gpu_host_alloc(udpdk_gpu_ctx *c, size_t bytes, void **host)
{
    if (!c || !host) return -EINVAL;
    if (hipHostMalloc(host, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *host = nullptr;
        return -ENOMEM;
    }
    return 0;
}

int udpdk_gpu_host_free(udpdk_gpu_ctx *c, void *host)
{
    if (!c) return -EINVAL;
    if (host) HIPC(c, hipHostFree(host));
    return 0;
}

int udpdk_gpu_memset(udpdk_gpu_ctx *c, void *dev, int value, size_t bytes)
{
    if (!c || (!dev && bytes)) return -EINVAL;
    if (c->depth > 1) { int rc = join_pipes(c); if (rc) return rc; }
    if (bytes) HIPC(c, hipMemsetAsync(dev, value, bytes, c->stream));
    return 0;
}

int udpdk_gpu_h2d(udpdk_gpu_ctx *c, void *dev, const void *host, size_t bytes)
{
    if (!c || ((!dev || !host) && bytes)) return -EINVAL;
    if (c->depth > 1) { int rc = join_pipes(c); if (rc) return rc; }
    if (bytes) HIPC(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

int udpdk_gpu_d2h(udpdk_gpu_ctx *c, void *host, const void *dev, size_t bytes)
{
    if (!c || ((!dev || !host) && bytes)) return -EINVAL;
    if (c->depth > 1) { int rc = join_pipes(c); if (rc) return rc; }
    if (bytes) HIPC(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

int udpdk_gpu_bind_snapshot_upload(udpdk_gpu_ctx *c, const udpdk_bind_snapshot_t *s)
{
    if (!c || !s || !s->port_first || !s->port_count || (s->n_binds && !s->binds)) return -EINVAL;
    if (s->n_lanes == 0 || s->n_lanes > c->max_lanes || s->n_binds > UDPDK_GPU_MAX_BINDS) return -EINVAL;
    if (s->n_slots && !s->slots) return -EINVAL;
    std::vector<uint4> tab(UDPDK_UDP_PORTS, make_uint4(0, 0, 0, 0));
    uint32_t maxfan = 0, nports = 0, iport[UDPDK_INLINE_PORTS] = {};
    uint4 ient[UDPDK_INLINE_PORTS] = {};
    for (uint32_t p = 0; p < UDPDK_UDP_PORTS; ++p) {
        const uint32_t cnt = s->port_count[p];
        if (!cnt) continue;
        const uint32_t first = s->port_first[p];
        if (cnt > UDPDK_GPU_MAX_PORT_BINDS || (uint64_t)first + cnt > s->n_binds) return -EINVAL;
        const udpdk_binding_t &b0 = s->binds[first];
        tab[p] = make_uint4(cnt, first, b0.ip, (uint32_t)b0.sockfd | (b0.reuse ? 0x80000000u : 0u));
        maxfan = std::max(maxfan, cnt);
        if (nports < UDPDK_INLINE_PORTS) {
            iport[nports] = p;
            ient[nports] = tab[p];
        }
        ++nports;
    }
    std::vector<uint2> b(s->n_binds ? s->n_binds : 1);
    for (uint32_t i = 0; i < s->n_binds; ++i) {
        const udpdk_binding_t &x = s->binds[i];
        if (x.sockfd < 0 || x.sockfd > 0xFFFF) return -EINVAL;
        if (((uint32_t)x.sockfd & s->lane_mask) >= s->n_lanes) return -EINVAL;
        b[i] = make_uint2(x.ip, (uint32_t)x.sockfd | (x.reuse ? 0x80000000u : 0u));
    }
    HIPC(c, hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }
    { int rc = c->binds.ensure(c, std::max<uint32_t>(s->n_binds, 1u)); if (rc) return rc; }   // (never null)
    HIPC(c, hipMemcpy(c->port_tab, tab.data(), UDPDK_UDP_PORTS * sizeof(uint4), hipMemcpyHostToDevice));
    if (s->n_binds)
        HIPC(c, hipMemcpy(c->binds, b.data(), (size_t)s->n_binds * sizeof(uint2), hipMemcpyHostToDevice));
    if (s->n_slots) {
        { int rc = c->slots.ensure(c, s->n_slots); if (rc) return rc; }
        std::vector<uint4> sl(s->n_slots);
        for (uint32_t i = 0; i < s->n_slots; ++i)
            sl[i] = make_uint4(s->slots[i].ip, s->slots[i].udp_port & 0xFFFFu, s->slots[i].bound ? 1u : 0u, 0u);
        HIPC(c, hipMemcpy(c->slots, sl.data(), (size_t)s->n_slots * sizeof(uint4), hipMemcpyHostToDevice));
    }
    c->n_slots = s->n_slots;
    c->n_lanes = s->n_lanes;
    c->lane_mask = s->lane_mask;
    uint32_t kb = 0;
    while ((1u << kb) < s->n_lanes) ++kb;
    c->key_bits = kb;
    c->max_fanout = maxfan;
    c->inl = nports <= UDPDK_INLINE_PORTS && !c->knobs.no_inline ? 1u : 0u;
    c->n_inl = c->inl ? nports : 0u;
    for (uint32_t k = 0; k < UDPDK_INLINE_PORTS; ++k) {
        c->inl_port[k] = iport[k];
        c->inl_ent[k] = ient[k];
    }
    c->have_snapshot = true;
    return 0;
}

int udpdk_gpu_timing_enable(udpdk_gpu_ctx *c, int enable)
{
    if (!c) return -EINVAL;
    if (enable && !c->sets) {
        c->sets = new (std::nothrow) TimingSet[EVENT_SETS];
        if (!c->sets) return -ENOMEM;
        for (int i = 0; i < EVENT_SETS; ++i)
            for (int k = 0; k < 2 * TIMED_KERNELS; ++k) HIPC(c, hipEventCreate(&c->sets[i].ev[k]));
    }
    c->timing_every = enable > 0 ? (uint32_t)enable : 0u;
    c->timing_calls = 0;
    return 0;
}

int udpdk_gpu_timing_read(udpdk_gpu_ctx *c, double ms[UDPDK_N_KERNEL_IDS],
                          uint32_t launches[UDPDK_N_KERNEL_IDS])
{
    if (!c) return -EINVAL;
    int rc = fold_timing(c);
    if (rc) return rc;
    for (int k = 0; k < UDPDK_N_KERNEL_IDS; ++k) {
        if (ms) ms[k] = c->ms[k];
        if (launches) launches[k] = c->launches[k];
        c->ms[k] = 0;
        c->launches[k] = 0;
    }
    return 0;
}

namespace {

// The drop filter (rx_filter.hip): entries out by verdict-word flags.
int filter_enqueue(udpdk_gpu_ctx *c, FilterWs &W, hipStream_t st, const udpdk_rx_lanes_t *in, uint32_t flags,
                   uint32_t *off_out, uint32_t *pkt_out, uint32_t out_cap)
{
    const int rc = lane_stage(c, W, st, in, off_out, pkt_out, out_cap, [&](FilterArgs &fa) {
        fa.flags = flags;
        return launch_mark(c, st, rx_filter_mark, fa, fa);
    });
    if (!rc) c->flt_last = &W;
    return rc;
}

// The key-window table the balance stage hashes with: the context's RSS configuration, or the
// default one (built on first use) when udpdk_gpu_rss_config was never called.
int balance_ktab(udpdk_gpu_ctx *c, const uint32_t **ktab, uint32_t *types)
{
    if (c->rss_ready) {
        *ktab = c->rss_ktab;
        *types = c->rss.hash_types;
        return 0;
    }
    if (!c->bal_ktab) {
        udpdk_rss_conf_t conf;
        udpdk_gpu_rss_default_conf(&conf, 1);
        std::vector<uint32_t> tab(12 * 256);
        rss_key_table(conf.key, reinterpret_cast<uint32_t(*)[256]>(tab.data()));
        const int rc = c->bal_ktab.ensure(c, tab.size());
        if (rc) return rc;
        if (hipMemcpy(c->bal_ktab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
            c->bal_ktab.release();
            return -EIO;
        }
    }
    *ktab = c->bal_ktab;
    *types = UDPDK_RSS_IPV4 | UDPDK_RSS_NONFRAG_IPV4_UDP;
    return 0;
}

// The balance stage (rx_balance.hip): every frame's choice among its reuse-port lanes by flow hash
// (pick), then the entries in lanes not chosen out.
int balance_enqueue(udpdk_gpu_ctx *c, BalanceWs &B, hipStream_t st, const udpdk_rx_batch_t *bt,
                    const udpdk_rx_lanes_t *in, const uint8_t *lane_rp, const uint32_t *hash_dev,
                    uint32_t *off_out, uint32_t *pkt_out, uint32_t out_cap)
{
    const uint32_t *ktab = nullptr;
    uint32_t types = 0;
    int rc = balance_ktab(c, &ktab, &types);
    if (rc) return rc;
    rc = lane_stage(c, B, st, in, off_out, pkt_out, out_cap, [&](FilterArgs &fa) {
        int rc;
        if ((rc = B.chosen.ensure(c, (size_t)in->n + 1)) || (rc = B.cnt.ensure(c, 1)) || (rc = B.h_cnt.ensure(c, 1)))
            return rc;
        HIPC(c, hipMemsetAsync(B.cnt, 0, 4, st));
        if (in->n) {
            BalancePickArgs pa;
            pa.frames = bt->frames_dev;
            pa.offset = bt->offset_dev;
            pa.meta = in->meta_dev;
            pa.port_tab = c->port_tab;
            pa.binds = c->binds;
            pa.lane_rp = lane_rp;
            pa.hash_in = hash_dev;
            pa.ktab = ktab;
            pa.chosen = B.chosen;
            pa.balanced = B.cnt;
            pa.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
            pa.n = in->n;
            pa.n_lanes = in->n_lanes;
            pa.hash_types = types;
            hipLaunchKernelGGL(rx_balance_pick, dim3(ceil_div(in->n, BAL_TILE)), dim3(BAL_BLOCK), 0, st, pa);
            HIPC(c, hipGetLastError());
        }
        BalanceMarkArgs ma;
        ma.f = fa;
        ma.chosen = B.chosen;
        ma.lane_rp = lane_rp;
        return launch_mark(c, st, rx_balance_mark, ma, fa);
    });
    if (!rc) c->bal_last = &B;
    return rc;
}

// The peer filter (rx_peer.hip): a connected lane's entries from anyone but its peer out.
int peer_enqueue(udpdk_gpu_ctx *c, FilterWs &W, hipStream_t st, const udpdk_rx_batch_t *bt,
                 const udpdk_rx_lanes_t *in, const uint2 *peer, uint32_t *off_out, uint32_t *pkt_out,
                 uint32_t out_cap)
{
    const int rc = lane_stage(c, W, st, in, off_out, pkt_out, out_cap, [&](FilterArgs &fa) {
        fa.meta = nullptr;
        PeerMarkArgs ma;
        ma.f = fa;
        ma.peer = peer;
        ma.frames = bt->frames_dev;
        ma.offset = bt->offset_dev;
        ma.length = bt->length_dev;
        ma.frames_bytes = (uint32_t)bt->frames_bytes;
        ma.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
        return launch_mark(c, st, rx_peer_mark, ma, fa);
    });
    if (!rc) c->peer_last = &W;
    return rc;
}

// The membership filter (rx_mcast.hip): a checked lane's multicast entries of groups it did not join out.
int mcast_enqueue(udpdk_gpu_ctx *c, FilterWs &W, hipStream_t st, const udpdk_rx_batch_t *bt,
                  const udpdk_rx_lanes_t *in, const uint8_t *lane_mc, const uint2 *table, uint32_t slots_lg,
                  uint32_t *off_out, uint32_t *pkt_out, uint32_t out_cap)
{
    const int rc = lane_stage(c, W, st, in, off_out, pkt_out, out_cap, [&](FilterArgs &fa) {
        fa.meta = nullptr;
        McastMarkArgs ma;
        ma.f = fa;
        ma.lane_mc = lane_mc;
        ma.table = table;
        ma.frames = bt->frames_dev;
        ma.offset = bt->offset_dev;
        ma.length = bt->length_dev;
        ma.slots_lg = slots_lg;
        ma.frames_bytes = (uint32_t)bt->frames_bytes;
        ma.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
        return launch_mark(c, st, rx_mcast_mark, ma, fa);
    });
    if (!rc) c->mcast_last = &W;
    return rc;
}

int rx_lanes_on_pipe(udpdk_gpu_ctx *c, int pipe, const udpdk_rx_batch_t *bt, const udpdk_rx_out_t *o);

// One batch's RX on a pipe: the launch sequence that makes the lanes (whichever form it takes),
// then the sticky stages that are on (sticky_stage), each on what the one before left, all on the
// pipe's stream. They are per-entry predicates that do not depend on what else the lanes hold, so
// they commute: one removes every entry of a frame, one picks by a hash that does not depend on
// the lanes, two look at the entry's own lane and frame.
int rx_on_pipe(udpdk_gpu_ctx *c, int pipe, const udpdk_rx_batch_t *bt, const udpdk_rx_out_t *o)
{
    int rc = rx_lanes_on_pipe(c, pipe, bt, o);
    if (rc) return rc;
    Pipe &P = c->pipes[pipe];
    for (bool &ran : P.sticky_ran) ran = false;
    if ((!c->drop_flags && !c->bal_on && !c->peer_on && !c->mcast_on) || bt->n == 0) return 0;   // (no frames: the lanes are empty)
    const udpdk_rx_lanes_t in = {o->meta_dev, bt->n, o->lane_off_dev, o->lane_pkt_dev, o->lane_cap, c->n_lanes};
    if (c->drop_flags &&
        (rc = sticky_stage(c, P, ST_DROP, o, [&](uint32_t *off, uint32_t *pkt) {
             return filter_enqueue(c, P.flt, P.stream, &in, c->drop_flags, off, pkt, o->lane_cap);
         })))
        return rc;
    if (!c->bal_on && !c->peer_on && !c->mcast_on) return 0;
    if (c->lane_mask != 0xFFFFFFFFu) return -EINVAL;           // compat mode: a lane is not a sockfd
    if (c->bal_on &&
        (rc = sticky_stage(c, P, ST_BALANCE, o, [&](uint32_t *off, uint32_t *pkt) {
             return balance_enqueue(c, P.bal, P.stream, bt, &in, c->bal_rp, nullptr, off, pkt, o->lane_cap);
         })))
        return rc;
    if (c->peer_on &&
        (rc = sticky_stage(c, P, ST_PEER, o, [&](uint32_t *off, uint32_t *pkt) {
             return peer_enqueue(c, P.peer, P.stream, bt, &in, c->peer_tab, off, pkt, o->lane_cap);
         })))
        return rc;
    if (c->mcast_on &&
        (rc = sticky_stage(c, P, ST_MCAST, o, [&](uint32_t *off, uint32_t *pkt) {
             return mcast_enqueue(c, P.mcast, P.stream, bt, &in, c->mcast_mc, c->mcast_tab, c->mcast_lg, off, pkt,
                                  o->lane_cap);
         })))
        return rc;
    return 0;
}

int rx_lanes_on_pipe(udpdk_gpu_ctx *c, int pipe, const udpdk_rx_batch_t *bt, const udpdk_rx_out_t *o)
{
    if (!c || !bt || !o || !c->have_snapshot) return -EINVAL;
    if (bt->n > c->max_frames || bt->frames_bytes >= (1ull << 32)) return -EINVAL;
    if (bt->n && (!bt->frames_dev || !bt->offset_dev || !bt->length_dev)) return -EINVAL;
    if (((uintptr_t)bt->frames_dev & 15u) != 0) return -EINVAL;
    if (!o->meta_dev && bt->n) return -EINVAL;
    if (!o->lane_off_dev || (!o->lane_pkt_dev && o->lane_cap)) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    Pipe &P = c->pipes[pipe];
    const hipStream_t st = P.stream;
    P.dirty = true;
    c->last_pipe = pipe;
    const uint32_t S = c->n_lanes;
    TimingSet *ts = nullptr;
    if (c->timing_every && (c->timing_calls++ % c->timing_every) == 0) {
        if (c->n_sets_used == EVENT_SETS) { int rc = fold_timing(c); if (rc) return rc; }
        ts = &c->sets[c->n_sets_used++];
    }
    P.last_lane_cap = o->lane_cap;
    if (bt->n == 0) {
        HIPC(c, hipMemsetAsync(o->lane_off_dev, 0, (size_t)(S + 1) * 4, st));
        HIPC(c, hipMemsetAsync(P.res.dev, 0, sizeof(DevResult), st));
        P.last_tiles = 0;
        if (ts) c->n_sets_used--;                         // nothing was launched
        return 0;
    }
    // the kernel form from the hints of the recent calls (RxArgs::hint), measured against the
    // latest call the GPU has reached (the host may run tens of calls ahead)
    const uint32_t done = __atomic_load_n(&c->hint[UDPDK_HINT_DONE], __ATOMIC_RELAXED);
    const uint32_t tail = __atomic_load_n(&c->hint[UDPDK_HINT_TAIL], __ATOMIC_RELAXED);
    const bool tail_recent = tail != 0u && (int32_t)(done - tail) <= (int32_t)UDPDK_HINT_WINDOW;
    const RxPlan p = rx_plan(bt->n, S, c->max_fanout, tail_recent, c->knobs, c->caps);
    if (p.err) return p.err;
    P.last_tiles = p.tiles;
    if (p.spec && ++P.spec_epoch == 0) P.spec_epoch = 1;       // 0: the zeroed word's tag
    if (++c->rx_seq == 0) c->rx_seq = 1;
    const uint32_t seq = c->rx_seq;
    if (c->knobs.trace) {                      // UDPDK_RX_TRACE: the classify form, then the geometry
        char cls[32], form[128];               // and the launches this call takes after classify
        rx_plan_trace(p, cls, form);
        fprintf(stderr, "udpdk_gpu_rx seq %u done %u hint tail %u nonfull %u -> %s\nudpdk_gpu_rx seq %u form %s\n",
                seq, done, tail, c->hint[UDPDK_HINT_NONFULL], cls, seq, form);
    }

    RxArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.hist16 = p.hist16 ? 1u : 0u;
    ra.frames = bt->frames_dev;
    ra.offset = bt->offset_dev;
    ra.length = bt->length_dev;
    ra.ptype = bt->ptype_dev;
    ra.port_tab = c->port_tab;
    ra.binds = c->binds;
    ra.meta = o->meta_dev;
    ra.hist = P.hist;
    ra.tile_cnt = P.tile_cnt;
    ra.dbg = c->dbg;
    ra.key_bits = c->key_bits;
    ra.frames_bytes = (uint32_t)bt->frames_bytes;
    ra.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
    ra.n = bt->n;
    ra.tile_frames = p.T;
    ra.n_tiles = p.tiles;
    ra.lane_mask = c->lane_mask;
    ra.n_lanes = S;
    ra.inl = c->inl;
    ra.n_inl = c->n_inl;
    for (uint32_t k = 0; k < UDPDK_INLINE_PORTS; ++k) {
        ra.inl_port[k] = c->inl_port[k];
        ra.inl_ent[k] = c->inl_ent[k];
    }
    ra.spec_pkt = p.spec ? o->lane_pkt_dev : nullptr;          // see RxArgs::spec_pkt
    ra.spec_cap = p.spec ? o->lane_cap : 0u;
    ra.spec_nonfull = p.spec ? P.res.dev->nonfull : nullptr;
    ra.spec_epoch = P.spec_epoch;
    ra.hint = c->hint;
    ra.seq = seq;
    ra.fuse = p.fuse ? P.fuse : nullptr;
    ra.lane_off = o->lane_off_dev;
    ra.total = &P.res.dev->total;
    ra.span = p.span ? 1u : 0u;

    if (ts) for (int k = 0; k < TIMED_KERNELS; ++k) ts->used[k] = false;
    HIPC(c, launch(st, ts, 0, true, true, classify_form(p.tailg, p.mr ? 1 : 0, c->knobs.policy), dim3(p.tiles),
                   dim3(CLS_BLOCK), p.cls_lds, ra));
    if (p.fuse) return 0;                      // the last workgroup completed the lane
    if (p.one_lane) {
        Compact1Args ca;
        ca.meta = o->meta_dev;
        ca.tile_count = P.hist;
        ca.lane_pkt = o->lane_pkt_dev;
        ca.lane_off = o->lane_off_dev;
        ca.total = &P.res.dev->total;
        ca.n = bt->n;
        ca.tile_frames = p.T;
        ca.n_tiles = p.tiles;
        ca.lane_cap = o->lane_cap;
        ca.base = p.tile_base ? P.partial : nullptr;
        ca.spec = p.spec ? 1u : 0u;
        ca.spec_nonfull = P.res.dev->nonfull;
        ca.spec_epoch = P.spec_epoch;
        ca.hint = c->hint;
        ca.seq = seq;
        if (p.tile_base) {
            hipLaunchKernelGGL(rx_tile_base, dim3(1), dim3(1024), 0, st, (const uint32_t *)P.hist,
                               P.partial.p, p.tiles);
            HIPC(c, hipGetLastError());
        }
        HIPC(c, launch(st, ts, 2, true, true, rx_compact1, dim3(p.compact_grid), dim3(RX_BLOCK), 0u, ca));
        return 0;
    }

    ScanArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.row_mask = p.cols ? p.G - 1u : 0u;
    sa.dbg = c->dbg;
    sa.hist = P.hist;
    sa.partial = P.partial;
    sa.lane_off = o->lane_off_dev;
    sa.total = &P.res.dev->total;
    sa.n_elems = S * p.tiles;
    sa.n_tiles = p.tiles;
    sa.n_lanes = S;
    sa.base = P.base;
    sa.agg = P.agg;
    sa.ticket = P.ticket;
    sa.epoch = ++P.epoch ? P.epoch : ++P.epoch;        // 0 marks a never-written look-back word
    sa.hist16 = ra.hist16;
    if (p.scan != RX_SCAN_3PASS) {
        const bool wide = p.scan == RX_SCAN_COLS1024;
        HIPC(c, launch(st, ts, 1, true, true, wide ? rx_scan_cols<1024> : rx_scan_cols<512>, dim3(p.scan_grid),
                       dim3(wide ? 1024 : 512), 0u, sa, p.lb));
    } else {
        const dim3 grid(p.nc, ceil_div(S, (uint32_t)SCAN_BLOCK));
        HIPC(c, launch(st, ts, 1, true, false, rx_scan_reduce, grid, dim3(SCAN_BLOCK), 0u, sa));
        HIPC(c, launch(st, ts, 1, false, false, rx_scan_top, dim3(1), dim3(SCAN_TOP_BLOCK), 4u * S, sa, p.nc));
        HIPC(c, launch(st, ts, 1, false, true, rx_scan_down, grid, dim3(SCAN_BLOCK), 0u, sa));
    }

    ScatterArgs xa;
    xa.meta = o->meta_dev;
    xa.base = p.cols ? P.base : P.hist;
    xa.total = &P.res.dev->total;
    xa.frames = bt->frames_dev;
    xa.offset = bt->offset_dev;
    xa.port_tab = c->port_tab;
    xa.binds = c->binds;
    xa.lane_pkt = o->lane_pkt_dev;
    xa.n = bt->n;
    xa.tile_frames = p.G * p.T;                // a scatter tile is G classify tiles (rx_scatter: G = 1)
    xa.n_tiles = ceil_div(p.tiles, p.G);
    xa.n_lanes = S;
    xa.lane_mask = c->lane_mask;
    xa.key_bits = c->key_bits;
    xa.lane_cap = o->lane_cap;
    xa.row_step = p.G;
    xa.dbg = c->dbg;
    if (!p.scatterw)
        HIPC(c, launch(st, ts, 2, true, true, rx_scatter, dim3(p.tiles), dim3(SCATTER1_BLOCK),
                       scatter1_lds_bytes(S), xa));
    else
        HIPC(c, launch(st, ts, 2, true, true,
                       p.W == SCATTER_WAVES ? rx_scatterw<SCATTER_WAVES> : rx_scatterw<2 * SCATTER_WAVES>,
                       dim3(xa.n_tiles), dim3(64 * p.W), scatterw_lds_bytes(S, p.W), xa));
    return 0;
}

} // namespace

int udpdk_gpu_rx(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_out_t *o)
{
    if (!c) return -EINVAL;
    const int pipe = c->depth > 1 ? (int)(c->rx_calls % (uint64_t)c->depth) : 0;
    const int rc = rx_on_pipe(c, pipe, bt, o);
    if (rc == 0) ++c->rx_calls;
    return rc;
}

namespace {
int enqueue_result(udpdk_gpu_ctx *c, Pipe &P);
int read_result(udpdk_gpu_ctx *c, Pipe &P, udpdk_rx_stats_t *st);
} // namespace

int udpdk_gpu_rx_stats(udpdk_gpu_ctx *c, udpdk_rx_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    if (c->last_pipe < 0) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    Pipe &P = c->pipes[c->last_pipe];
    int rc = enqueue_result(c, P);
    if (rc) return rc;
    HIPC(c, hipStreamSynchronize(P.stream));
    return read_result(c, P, st);
}

namespace {

// The counter reduction and the result row (counters, delivery total) of pipe p's last call
// into its pinned mirror, on the pipe's stream.
int enqueue_result(udpdk_gpu_ctx *c, Pipe &P)
{
    P.dirty = true;
    if (P.last_tiles) {
        hipLaunchKernelGGL(rx_counters, dim3(1), dim3(256), 0, P.stream, (const uint32_t *)P.tile_cnt,
                           P.last_tiles, P.res.dev->counters);
        HIPC(c, hipGetLastError());
    }
    int rc = P.res.enqueue_fetch(c, P.stream);
    for (int k = 0; k < N_STICKY && !rc; ++k)
        if (P.sticky_ran[k]) rc = P.sticky[k]->res.enqueue_fetch(c, P.stream);
    return rc;
}

int read_result(udpdk_gpu_ctx *c, Pipe &P, udpdk_rx_stats_t *st)
{
    const DevResult *r = P.res.host;
    for (int k = 0; k < UDPDK_N_COUNTERS; ++k) st->counters[k] = r->counters[k];
    // (with sticky stages: what the last of them kept; overflow stays the pre-filter total's)
    st->deliveries = r->total;
    for (int k = 0; k < N_STICKY; ++k) {
        const FilterResult *f = P.sticky[k]->res.host;
        if (P.sticky_ran[k]) st->deliveries = f->kept;
        P.removed[k] = P.sticky_ran[k] ? f->removed : 0u;
    }
    for (Pipe &Q : c->pipes)
        if (Q.stats_of == st) Q.stats_of = nullptr;      // (a stats block reused across pipes)
    P.stats_of = st;
    st->overflow = r->total > P.last_lane_cap ? 1u : 0u;
    return st->overflow ? -ENOSPC : 0;
}

// Wait for pipe p's outstanding host call, if any, and fill its stats.
int finish_host(udpdk_gpu_ctx *c, Pipe &P)
{
    if (!P.host_stats) return 0;
    udpdk_rx_stats_t *st = P.host_stats;
    P.host_stats = nullptr;
    HIPC(c, hipStreamSynchronize(P.stream));
    return read_result(c, P, st);
}

// One host-resident batch on pipe p, all on the pipe's stream: (pageable input: a host copy
// into pinned staging first) H2D of frames + descriptors, the RX pipeline, the counter
// reduction, D2H of the result row, meta, lane_off and lane_pkt[0, lane_cap).
int enqueue_host(udpdk_gpu_ctx *c, int pipe, const uint8_t *frames_host, uint64_t frames_bytes,
                 const uint32_t *offset_host, const uint16_t *length_host,
                 const uint32_t *ptype_host, uint32_t n, uint32_t *meta_host,
                 uint32_t *lane_off_host, uint32_t *lane_pkt_host, uint32_t lane_cap,
                 udpdk_rx_stats_t *stats, bool copy_lanes = true, uint32_t offset_base = 0)
{
    if (!stats || !lane_off_host || n > c->max_frames) return -EINVAL;
    if (n && (!frames_host || !offset_host || !length_host || !meta_host)) return -EINVAL;
    if (lane_cap && !lane_pkt_host) return -EINVAL;
    if (frames_bytes >= (1ull << 32)) return -EINVAL;
    Pipe &P = c->pipes[pipe];
    const hipStream_t s = P.stream;
    P.dirty = true;
    // frames + the tailroom the kernels may read past them (UDPDK_GPU_FRAMES_TAILROOM)
    const size_t fb = (((size_t)frames_bytes + 255) & ~(size_t)255) + UDPDK_GPU_FRAMES_TAILROOM;
    const size_t desc = (size_t)n * 10 + 64;
    const size_t outb = (size_t)n * 4 + (size_t)(c->n_lanes + 1) * 4 + (size_t)lane_cap * 4 + 64;
    int rc;
    // The frames are expected in pinned memory (DPDK hugepage mbufs registered with the
    // runtime); pageable input is copied into a pinned staging buffer first.
    // (a chunk of a larger buffer: the allocation is looked up by the buffer's own start)
    hipPointerAttribute_t attr;
    const bool pinned = n && hipPointerGetAttributes(&attr, frames_host - offset_base) == hipSuccess &&
                        attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    if ((rc = P.st_frames_d.ensure(c, fb)) || (n && !pinned && (rc = P.st_frames_h.ensure(c, fb))) ||
        (rc = P.st_desc_d.ensure(c, desc)) || (rc = P.st_desc_h.ensure(c, desc)) || (rc = P.st_out_d.ensure(c, outb)))
        return rc;
    const uint8_t *src = frames_host;
    if (n && !pinned) {
        memcpy(P.st_frames_h, frames_host, frames_bytes);
        src = P.st_frames_h;
    }
    uint8_t *dh = P.st_desc_h;
    if (offset_base) {                          // a chunk of a larger batch: offsets rebased
        uint32_t *o = (uint32_t *)dh;
        for (uint32_t i = 0; i < n; ++i) o[i] = offset_host[i] - offset_base;
    } else {
        memcpy(dh, offset_host, (size_t)n * 4);
    }
    memcpy(dh + (size_t)n * 4, length_host, (size_t)n * 2);
    const size_t pt_off = ((size_t)n * 6 + 15) & ~(size_t)15;
    if (ptype_host) memcpy(dh + pt_off, ptype_host, (size_t)n * 4);
    if (n) HIPC(c, hipMemcpyAsync(P.st_frames_d, src, frames_bytes, hipMemcpyHostToDevice, s));
    HIPC(c, hipMemcpyAsync(P.st_desc_d, dh, pt_off + (ptype_host ? (size_t)n * 4 : 0),
                           hipMemcpyHostToDevice, s));
    uint32_t *meta_d = (uint32_t *)P.st_out_d.p;
    uint32_t *off_d = meta_d + n;
    uint32_t *pkt_d = off_d + c->n_lanes + 1;
    const uint8_t *desc_d = P.st_desc_d;
    udpdk_rx_batch_t b = {P.st_frames_d, frames_bytes, (const uint32_t *)desc_d, (const uint16_t *)(desc_d + (size_t)n * 4),
                          ptype_host ? (const uint32_t *)(desc_d + pt_off) : nullptr, n};
    udpdk_rx_out_t o = {meta_d, off_d, pkt_d, lane_cap};
    if ((rc = rx_on_pipe(c, pipe, &b, &o))) return rc;
    if ((rc = enqueue_result(c, P))) return rc;
    if (n) HIPC(c, hipMemcpyAsync(meta_host, meta_d, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPC(c, hipMemcpyAsync(lane_off_host, off_d, (size_t)(c->n_lanes + 1) * 4, hipMemcpyDeviceToHost, s));
    if (lane_cap && copy_lanes)
        HIPC(c, hipMemcpyAsync(lane_pkt_host, pkt_d, (size_t)lane_cap * 4, hipMemcpyDeviceToHost, s));
    P.host_stats = stats;
    P.staged = b;
    P.staged_meta = meta_d;
    return 0;
}

int finish_all_host(udpdk_gpu_ctx *c)
{
    int rc = 0;
    const int d = std::max(1, c->depth);
    for (int k = 0; k < d; ++k) {          // oldest first
        Pipe &P = c->pipes[(c->host_calls + (uint64_t)k) % (uint64_t)d];
        const int r = finish_host(c, P);
        if (r && !rc) rc = r;
    }
    return rc;
}

} // namespace

int udpdk_gpu_rx_host(udpdk_gpu_ctx *c, const uint8_t *frames_host, uint64_t frames_bytes,
                      const uint32_t *offset_host, const uint16_t *length_host,
                      const uint32_t *ptype_host, uint32_t n, uint32_t *meta_host,
                      uint32_t *lane_off_host, uint32_t *lane_pkt_host, uint32_t lane_cap,
                      udpdk_rx_stats_t *stats)
{
    if (!c) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    int rc = finish_all_host(c);
    if (rc && rc != -ENOSPC) return rc;
    if (c->depth > 1) { int r = join_pipes(c); if (r) return r; }
    // synchronous: the lane entries come back after the counters, only as many as were made
    if ((rc = enqueue_host(c, 0, frames_host, frames_bytes, offset_host, length_host, ptype_host, n,
                           meta_host, lane_off_host, lane_pkt_host, lane_cap, stats, false))) return rc;
    Pipe &P = c->pipes[0];
    rc = finish_host(c, P);
    if (rc && rc != -ENOSPC) return rc;
    const uint32_t d = std::min(stats->deliveries, lane_cap);
    if (d) {
        const uint32_t *pkt_d = P.staged_meta + n + c->n_lanes + 1;
        HIPC(c, hipMemcpyAsync(lane_pkt_host, pkt_d, (size_t)d * 4, hipMemcpyDeviceToHost, P.stream));
        HIPC(c, hipStreamSynchronize(P.stream));
    }
    return rc;
}

namespace {

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na && nb && x < y + nb && y < x + na;
}

// What the three explicit lane-removal calls ask of the lane set and the outputs alike.
int lanes_check(const udpdk_gpu_ctx *c, const udpdk_rx_lanes_t *in, const uint32_t *off_out, const uint32_t *pkt_out,
                uint32_t out_cap)
{
    if (!c || !in || !off_out) return -EINVAL;
    if (in->n_lanes == 0 || in->n_lanes > UDPDK_GPU_MAX_LANES || !in->lane_off_dev) return -EINVAL;
    if ((in->lane_cap && !in->lane_pkt_dev) || (out_cap && !pkt_out)) return -EINVAL;
    return 0;
}

// lanes_check, and what udpdk_gpu_rx_balance_select, _peer_select and _mcast_select ask besides: the
// batch the lanes were made from, lanes that are sockets, outputs apart from the inputs.
int select_check(const udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *in,
                 const uint32_t *off_out, const uint32_t *pkt_out, uint32_t out_cap)
{
    if (!bt || lanes_check(c, in, off_out, pkt_out, out_cap)) return -EINVAL;
    if (bt->n != in->n || bt->frames_bytes >= (1ull << 32)) return -EINVAL;
    if (bt->n && (!bt->frames_dev || !bt->offset_dev)) return -EINVAL;
    if (!c->have_snapshot || c->lane_mask != 0xFFFFFFFFu) return -EINVAL;
    const size_t offb = ((size_t)in->n_lanes + 1) * 4, pktb = (size_t)in->lane_cap * 4;
    if (ranges_overlap(off_out, offb, in->lane_off_dev, offb) || ranges_overlap(off_out, offb, in->lane_pkt_dev, pktb) ||
        ranges_overlap(pkt_out, (size_t)out_cap * 4, in->lane_off_dev, offb) ||
        ranges_overlap(pkt_out, (size_t)out_cap * 4, in->lane_pkt_dev, pktb))
        return -EINVAL;
    return 0;
}

// The FilterResult of W's last run into its mirror (and, for the balance stage, the count that goes
// with it), waited for: what the four *_stats calls read.
int fetch_filter_result(udpdk_gpu_ctx *c, FilterWs *W, BalanceWs *B = nullptr)
{
    if (!W) return -ENOENT;
    HIPC(c, hipSetDevice(c->device));
    const int rc = W->res.enqueue_fetch(c, W->stream);
    if (rc) return rc;
    if (B) HIPC(c, hipMemcpyAsync(B->h_cnt.p, B->cnt.p, 4, hipMemcpyDeviceToHost, W->stream));
    HIPC(c, hipStreamSynchronize(W->stream));
    return 0;
}

} // namespace

int udpdk_gpu_rx_filter(udpdk_gpu_ctx *c, const udpdk_rx_lanes_t *in, uint32_t flags,
                        uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap)
{
    if ((flags & ~UDPDK_RX_DROP_ALL) || lanes_check(c, in, lane_off_out_dev, lane_pkt_out_dev, out_cap)) return -EINVAL;
    if (in->n && !in->meta_dev) return -EINVAL;
    const int rc = on_ctx_stream(c);
    if (rc) return rc;
    return filter_enqueue(c, c->xflt, c->stream, in, flags, lane_off_out_dev, lane_pkt_out_dev, out_cap);
}

int udpdk_gpu_rx_drop(udpdk_gpu_ctx *c, int flags)
{
    if (!c) return -EINVAL;
    const int was = (int)c->drop_flags;
    if (flags < 0) return was;
    if ((uint32_t)flags & ~UDPDK_RX_DROP_ALL) return -EINVAL;
    c->drop_flags = (uint32_t)flags;
    return was;
}

int udpdk_gpu_rx_drop_stats(udpdk_gpu_ctx *c, udpdk_rx_drop_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    const int rc = fetch_filter_result(c, c->flt_last);
    if (rc) return rc;
    const FilterResult *r = c->flt_last->res.host;
    for (int k = 0; k < 4; ++k) st->dropped[k] = r->dropped[k];
    st->kept = r->kept;
    st->removed = r->removed;
    st->bad_index = r->bad_index;
    st->truncated = r->truncated;
    return st->kept > c->flt_last->out_cap ? -ENOSPC : 0;
}

uint32_t udpdk_gpu_rx_balance_rank(uint32_t hash, uint32_t g)
{
    return (uint32_t)(((uint64_t)hash * g) >> 32);
}

int udpdk_gpu_rx_balance_select(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *in,
                                const uint8_t *lane_rp_dev, const uint32_t *hash_dev,
                                uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap)
{
    if (!lane_rp_dev || select_check(c, bt, in, lane_off_out_dev, lane_pkt_out_dev, out_cap)) return -EINVAL;
    if (!in->meta_dev) return -EINVAL;
    const int rc = on_ctx_stream(c);
    if (rc) return rc;
    return balance_enqueue(c, c->xbal, c->stream, bt, in, lane_rp_dev, hash_dev, lane_off_out_dev,
                           lane_pkt_out_dev, out_cap);
}

int udpdk_gpu_rx_balance(udpdk_gpu_ctx *c, const uint8_t *lane_rp_host, uint32_t n_lanes)
{
    if (!c || n_lanes > c->max_lanes) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }             // (calls in flight read the flags)
    if (!lane_rp_host || n_lanes == 0) {
        c->bal_on = false;
        return 0;
    }
    { int rc = c->bal_rp.ensure(c, c->max_lanes); if (rc) return rc; }
    std::vector<uint8_t> rp(c->max_lanes, 0);
    for (uint32_t l = 0; l < n_lanes; ++l) rp[l] = lane_rp_host[l] ? 1 : 0;
    HIPC(c, hipMemcpy(c->bal_rp, rp.data(), rp.size(), hipMemcpyHostToDevice));
    const uint32_t *ktab;
    uint32_t types;
    { int rc = balance_ktab(c, &ktab, &types); if (rc) return rc; }   // (built now, not inside a call)
    c->bal_on = true;
    return 0;
}

int udpdk_gpu_rx_balance_stats(udpdk_gpu_ctx *c, udpdk_rx_balance_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    BalanceWs *B = c->bal_last;
    const int rc = fetch_filter_result(c, B, B);
    if (rc) return rc;
    const FilterResult *r = B->res.host;
    st->kept = r->kept;
    st->removed = r->removed;
    st->balanced = *B->h_cnt;
    st->bad_index = r->bad_index;
    st->truncated = r->truncated;
    return st->kept > B->out_cap ? -ENOSPC : 0;
}

int udpdk_gpu_rx_removed(udpdk_gpu_ctx *c, const udpdk_rx_stats_t *stats, uint32_t *dropped, uint32_t *balanced)
{
    if (!c || !stats || !dropped || !balanced) return -EINVAL;
    for (const Pipe &P : c->pipes) {
        if (P.stats_of != stats) continue;
        *dropped = P.removed[ST_DROP];
        *balanced = P.removed[ST_BALANCE];
        return 0;
    }
    return -ENOENT;
}

int udpdk_gpu_rx_peer_select(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *in,
                             const udpdk_peer_t *peer_dev, uint32_t *lane_off_out_dev,
                             uint32_t *lane_pkt_out_dev, uint32_t out_cap)
{
    if (!peer_dev || ((uintptr_t)peer_dev & 7u) != 0) return -EINVAL;   // (the records load as 8-byte words)
    if (select_check(c, bt, in, lane_off_out_dev, lane_pkt_out_dev, out_cap)) return -EINVAL;
    if (bt->n && !bt->length_dev) return -EINVAL;
    const int rc = on_ctx_stream(c);
    if (rc) return rc;
    return peer_enqueue(c, c->xpeer, c->stream, bt, in, reinterpret_cast<const uint2 *>(peer_dev),
                        lane_off_out_dev, lane_pkt_out_dev, out_cap);
}

int udpdk_gpu_rx_peer(udpdk_gpu_ctx *c, const udpdk_peer_t *peer_host, uint32_t n_lanes)
{
    if (!c || n_lanes > c->max_lanes) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }             // (calls in flight read the records)
    bool any = false;
    for (uint32_t l = 0; peer_host && l < n_lanes; ++l) any = any || peer_host[l].on != 0;
    if (!any) {
        c->peer_on = false;
        return 0;
    }
    { int rc = c->peer_tab.ensure(c, c->max_lanes); if (rc) return rc; }
    std::vector<uint2> tab(c->max_lanes, make_uint2(0u, 0u));
    for (uint32_t l = 0; l < n_lanes; ++l)
        if (peer_host[l].on) tab[l] = make_uint2(peer_host[l].ip, (uint32_t)peer_host[l].port | (1u << 16));
    HIPC(c, hipMemcpy(c->peer_tab, tab.data(), tab.size() * sizeof(uint2), hipMemcpyHostToDevice));
    c->peer_on = true;
    return 0;
}

int udpdk_gpu_rx_peer_stats(udpdk_gpu_ctx *c, udpdk_rx_peer_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    const int rc = fetch_filter_result(c, c->peer_last);
    if (rc) return rc;
    const FilterResult *r = c->peer_last->res.host;
    st->kept = r->kept;
    st->removed = r->removed;
    st->refused = (uint32_t)r->dropped[0];
    st->bad_frame = (uint32_t)r->dropped[1];
    st->bad_index = r->bad_index;
    st->truncated = r->truncated;
    return st->kept > c->peer_last->out_cap ? -ENOSPC : 0;
}

int udpdk_gpu_rx_peer_removed(udpdk_gpu_ctx *c, const udpdk_rx_stats_t *stats, uint32_t *refused)
{
    if (!c || !stats || !refused) return -EINVAL;
    for (const Pipe &P : c->pipes) {
        if (P.stats_of != stats) continue;
        *refused = P.removed[ST_PEER];
        return 0;
    }
    return -ENOENT;
}

int udpdk_gpu_mcast_table_build(const udpdk_mcast_member_t *members, uint32_t n, udpdk_mcast_member_t *table_out,
                                uint32_t slots)
{
    const uint32_t lg = mcast_slots_log2(slots);
    if (!table_out || (!members && n) || !lg) return -EINVAL;
    if (n > slots) return -ENOSPC;
    udpdk_mcast_member_t *tab = table_out;
    memset(tab, 0, (size_t)slots * sizeof(*tab));
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t g = members[k].group, l = members[k].lane;
        if (g == 0u || mcast_probe(tab, lg, g, l)) return -EINVAL;
        uint32_t i = mcast_start(g, l, lg);
        while (tab[i].group != 0u) i = (i + 1u) & (slots - 1u);   // (k < slots members are in: a slot is empty)
        tab[i] = members[k];
    }
    return 0;
}

int udpdk_gpu_rx_mcast_select(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *in,
                              const uint8_t *lane_mc_dev, const udpdk_mcast_member_t *table_dev, uint32_t slots,
                              uint32_t *lane_off_out_dev, uint32_t *lane_pkt_out_dev, uint32_t out_cap)
{
    const uint32_t lg = mcast_slots_log2(slots);
    if (!lane_mc_dev || !table_dev || ((uintptr_t)table_dev & 7u) != 0 || !lg) return -EINVAL;   // (8-byte loads)
    if (select_check(c, bt, in, lane_off_out_dev, lane_pkt_out_dev, out_cap)) return -EINVAL;
    if (bt->n && !bt->length_dev) return -EINVAL;
    const int rc = on_ctx_stream(c);
    if (rc) return rc;
    return mcast_enqueue(c, c->xmcast, c->stream, bt, in, lane_mc_dev, reinterpret_cast<const uint2 *>(table_dev), lg,
                         lane_off_out_dev, lane_pkt_out_dev, out_cap);
}

int udpdk_gpu_rx_mcast(udpdk_gpu_ctx *c, const uint8_t *lane_mc_host, uint32_t n_lanes,
                       const udpdk_mcast_member_t *members_host, uint32_t n_members)
{
    if (!c || n_lanes > c->max_lanes || n_members > (1u << 19) || (!members_host && n_members)) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int rc = sync_all(c); if (rc) return rc; }             // (calls in flight read the flags and the table)
    if (!lane_mc_host || n_lanes == 0) {
        c->mcast_on = false;
        return 0;
    }
    for (uint32_t k = 0; k < n_members; ++k)
        if (members_host[k].lane >= n_lanes) return -EINVAL;
    uint32_t slots = MCAST_MIN_SLOTS;
    while (slots < 2u * n_members) slots <<= 1;
    std::vector<udpdk_mcast_member_t> tab(slots);
    { int rc = udpdk_gpu_mcast_table_build(members_host, n_members, tab.data(), slots); if (rc) return rc; }
    std::vector<uint8_t> mc(c->max_lanes, 0);
    for (uint32_t l = 0; l < n_lanes; ++l) mc[l] = lane_mc_host[l] ? 1 : 0;
    c->mcast_on = false;                                     // (until both uploads are in)
    int rc;
    if ((rc = c->mcast_mc.ensure(c, c->max_lanes)) || (rc = c->mcast_tab.ensure(c, slots))) return rc;
    HIPC(c, hipMemcpy(c->mcast_mc, mc.data(), mc.size(), hipMemcpyHostToDevice));
    HIPC(c, hipMemcpy(c->mcast_tab, tab.data(), (size_t)slots * sizeof(uint2), hipMemcpyHostToDevice));
    c->mcast_lg = mcast_slots_log2(slots);
    c->mcast_on = true;
    return 0;
}

int udpdk_gpu_rx_mcast_stats(udpdk_gpu_ctx *c, udpdk_rx_mcast_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    const int rc = fetch_filter_result(c, c->mcast_last);
    if (rc) return rc;
    const FilterResult *r = c->mcast_last->res.host;
    st->kept = r->kept;
    st->removed = r->removed;
    st->member = (uint32_t)r->dropped[2];
    st->not_member = (uint32_t)r->dropped[0];
    st->bad_frame = (uint32_t)r->dropped[1];
    st->bad_index = r->bad_index;
    st->truncated = r->truncated;
    return st->kept > c->mcast_last->out_cap ? -ENOSPC : 0;
}

int udpdk_gpu_rx_mcast_removed(udpdk_gpu_ctx *c, const udpdk_rx_stats_t *stats, uint32_t *not_member)
{
    if (!c || !stats || !not_member) return -EINVAL;
    for (const Pipe &P : c->pipes) {
        if (P.stats_of != stats) continue;
        *not_member = P.removed[ST_MCAST];
        return 0;
    }
    return -ENOENT;
}

int udpdk_gpu_rx_host_batch(udpdk_gpu_ctx *c, udpdk_rx_batch_t *batch, const uint32_t **meta_dev)
{
    if (!c || !batch) return -EINVAL;
    const Pipe &P = c->pipes[0];
    if (!P.staged_meta) return -ENOENT;
    *batch = P.staged;
    if (meta_dev) *meta_dev = P.staged_meta;
    return 0;
}

int udpdk_gpu_rx_host_async(udpdk_gpu_ctx *c, const uint8_t *frames_host, uint64_t frames_bytes,
                            const uint32_t *offset_host, const uint16_t *length_host,
                            const uint32_t *ptype_host, uint32_t n, uint32_t *meta_host,
                            uint32_t *lane_off_host, uint32_t *lane_pkt_host, uint32_t lane_cap,
                            udpdk_rx_stats_t *stats)
{
    if (!c) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    const int pipe = (int)(c->host_calls % (uint64_t)std::max(1, c->depth));
    Pipe &P = c->pipes[pipe];
    int rc = finish_host(c, P);                 // at most `depth` calls outstanding
    if (rc && rc != -ENOSPC) return rc;
    if ((rc = enqueue_host(c, pipe, frames_host, frames_bytes, offset_host, length_host, ptype_host,
                           n, meta_host, lane_off_host, lane_pkt_host, lane_cap, stats))) return rc;
    ++c->host_calls;
    return 0;
}

int udpdk_gpu_rx_host_wait(udpdk_gpu_ctx *c)
{
    if (!c) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    return finish_all_host(c);
}

namespace {

static int rx_gather_launch(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *lane_pkt_dev,
                     uint32_t first, uint32_t count, const uint32_t *slot_off_dev,
                     const udpdk_rx_gather_t *o, int pipe = -1)
{
    if (!c || !bt || !o) return -EINVAL;
    if (!count) return 0;
    if (!bt->n || !bt->frames_dev || !bt->offset_dev || !bt->length_dev || !lane_pkt_dev ||
        !o->payload_dev || !o->len_dev || !o->src_ip_dev || !o->src_port_dev) return -EINVAL;
    if (!slot_off_dev && (o->slot_bytes < 16u || (o->slot_bytes & 15u))) return -EINVAL;
    if ((uintptr_t)o->payload_dev & 15u) return -EINVAL;
    if (bt->frames_bytes >= (1ull << 32) || (uint64_t)first + count > 0xFFFFFFFFull) return -EINVAL;
    // pipe >= 0: on that pipe's stream, after its own work only (udpdk_gpu_pipe_gather_packed)
    if (pipe < 0) {
        const int rc = on_ctx_stream(c);
        if (rc) return rc;
    } else {
        HIPC(c, hipSetDevice(c->device));
        c->pipes[pipe].dirty = true;
    }
    const hipStream_t gst = pipe < 0 ? c->stream : c->pipes[pipe].stream;
    GatherArgs ga;
    ga.frames = bt->frames_dev;
    ga.offset = bt->offset_dev;
    ga.length = bt->length_dev;
    ga.lane_pkt = lane_pkt_dev;
    ga.payload = o->payload_dev;
    ga.len_out = o->len_dev;
    ga.src_ip = o->src_ip_dev;
    ga.src_port = o->src_port_dev;
    ga.first = first;
    ga.count = count;
    ga.slot_bytes = o->slot_bytes;
    ga.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
    ga.n = bt->n;
    ga.slot_off = slot_off_dev;
    const uint32_t grid = std::min<uint32_t>(ceil_div(count, GATHER_BLOCK), c->knobs.gather_grid);
    return launch_timed(c, gst, UDPDK_K_RX_GATHER, rx_gather, dim3(grid), dim3(GATHER_BLOCK), ga);
}

} // namespace

int udpdk_gpu_rx_gather(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *lane_pkt_dev,
                        uint32_t first, uint32_t count, const udpdk_rx_gather_t *o)
{
    return rx_gather_launch(c, bt, lane_pkt_dev, first, count, nullptr, o);
}

int udpdk_gpu_rx_gather_packed(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *lane_pkt_dev,
                               uint32_t first, uint32_t count, const uint32_t *slot_off_dev,
                               const udpdk_rx_gather_t *o)
{
    if (count && !slot_off_dev) return -EINVAL;
    return rx_gather_launch(c, bt, lane_pkt_dev, first, count, slot_off_dev, o);
}

// ---- poller internals: udpdk_poll_rx's pipelined form (explicit pipes, no cross-pipe joins) ----
int udpdk_gpu_pipe_rx_host(udpdk_gpu_ctx *c, int pipe, const uint8_t *frames_host, uint64_t frames_bytes,
                           const uint32_t *offset_host, uint32_t offset_base, const uint16_t *length_host,
                           const uint32_t *ptype_host, uint32_t n, uint32_t *meta_host,
                           uint32_t *lane_off_host, uint32_t *lane_pkt_host, uint32_t lane_cap,
                           udpdk_rx_stats_t *stats)
{
    if (!c || pipe < 1 || pipe >= MAX_PIPES) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    int rc = finish_host(c, c->pipes[pipe]);
    if (rc && rc != -ENOSPC) return rc;
    return enqueue_host(c, pipe, frames_host, frames_bytes, offset_host, length_host, ptype_host, n,
                        meta_host, lane_off_host, lane_pkt_host, lane_cap, stats, true, offset_base);
}

int udpdk_gpu_pipe_wait(udpdk_gpu_ctx *c, int pipe)
{
    if (!c || pipe < 1 || pipe >= MAX_PIPES) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    Pipe &P = c->pipes[pipe];
    const int rc = finish_host(c, P);
    HIPC(c, hipStreamSynchronize(P.stream));
    return rc;
}

int udpdk_gpu_pipe_batch(udpdk_gpu_ctx *c, int pipe, udpdk_rx_batch_t *batch, const uint32_t **meta_dev)
{
    if (!c || !batch || pipe < 1 || pipe >= MAX_PIPES) return -EINVAL;
    const Pipe &P = c->pipes[pipe];
    if (!P.staged_meta) return -ENOENT;
    *batch = P.staged;
    if (meta_dev) *meta_dev = P.staged_meta;
    return 0;
}

// (explicit directions: hipMemcpyDefault made the runtime block the caller on these D2H copies
// into pinned slabs, 8-10 ms of a pipelined poll's issue time)
static int pipe_copy(udpdk_gpu_ctx *c, int pipe, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (!c || pipe < 1 || pipe >= MAX_PIPES || ((!dst || !src) && bytes)) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    c->pipes[pipe].dirty = true;
    if (bytes) HIPC(c, hipMemcpyAsync(dst, src, bytes, kind, c->pipes[pipe].stream));
    return 0;
}

int udpdk_gpu_pipe_h2d(udpdk_gpu_ctx *c, int pipe, void *dev, const void *host, size_t bytes)
{
    return pipe_copy(c, pipe, dev, host, bytes, hipMemcpyHostToDevice);
}

int udpdk_gpu_pipe_d2h(udpdk_gpu_ctx *c, int pipe, void *host, const void *dev, size_t bytes)
{
    return pipe_copy(c, pipe, host, dev, bytes, hipMemcpyDeviceToHost);
}

int udpdk_gpu_pipe_gather_packed(udpdk_gpu_ctx *c, int pipe, const udpdk_rx_batch_t *bt,
                                 const uint32_t *lane_pkt_dev, uint32_t first, uint32_t count,
                                 const uint32_t *slot_off_dev, const udpdk_rx_gather_t *o)
{
    if (!c || pipe < 1 || pipe >= MAX_PIPES || (count && !slot_off_dev)) return -EINVAL;
    return rx_gather_launch(c, bt, lane_pkt_dev, first, count, slot_off_dev, o, pipe);
}

int udpdk_gpu_rss_default_conf(udpdk_rss_conf_t *conf, uint32_t n_queues)
{
    static const uint8_t key[UDPDK_RSS_KEY_BYTES] = {
        0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
        0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
        0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa};
    if (!conf || !n_queues || n_queues > UDPDK_RSS_MAX_QUEUES) return -EINVAL;
    memset(conf, 0, sizeof(*conf));
    memcpy(conf->key, key, sizeof(key));
    conf->hash_types = UDPDK_RSS_IPV4 | UDPDK_RSS_NONFRAG_IPV4_UDP;
    conf->n_queues = n_queues;
    conf->reta_size = 128;
    for (uint32_t i = 0; i < conf->reta_size; ++i) conf->reta[i] = (uint16_t)(i % n_queues);
    return 0;
}

int udpdk_gpu_rss_config(udpdk_gpu_ctx *c, const udpdk_rss_conf_t *conf)
{
    if (!c || !conf) return -EINVAL;
    if (!conf->n_queues || conf->n_queues > UDPDK_RSS_MAX_QUEUES || !conf->reta_size ||
        conf->reta_size > UDPDK_RSS_RETA_MAX || (conf->reta_size & (conf->reta_size - 1)) ||
        (conf->hash_types & ~3u))
        return -EINVAL;
    for (uint32_t i = 0; i < conf->reta_size; ++i)
        if (conf->reta[i] >= conf->n_queues) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int r = join_pipes(c); if (r) return r; }
    HIPC(c, hipStreamSynchronize(c->stream));
    const uint32_t tiles = ceil_div(std::max<uint32_t>(c->max_frames, 1), RSS_TILE);
    if (!c->rss_fuse) {
        int rc;
        if ((rc = c->rss_reta.ensure(c, RSS_RETA_MAX)) || (rc = c->rss_ktab.ensure(c, 12 * 256)) ||
            (rc = c->rss_qid.ensure(c, std::max<uint32_t>(c->max_frames, 1))) ||
            (rc = c->rss_hist.ensure(c, (size_t)tiles * RSS_MAX_QUEUES)) ||
            (rc = c->rss_partial.ensure(c, (size_t)ceil_div(tiles, SCAN_COL_CHUNK) * RSS_MAX_QUEUES)) ||
            (rc = c->rss_total.ensure(c, 64 / 4)) || (rc = c->rss_fuse.ensure(c, FUSE_BYTES / 8)))
            return rc;
        HIPC(c, hipMemset(c->rss_fuse, 0, FUSE_BYTES));
    }
    {
        const char *e = getenv("UDPDK_RSS_FUSE");
        c->rss_no_fuse = e && atoi(e) == 0;
        c->rss_trace = getenv("UDPDK_RSS_TRACE") != nullptr;
    }
    HIPC(c, hipMemcpy(c->rss_reta, conf->reta, conf->reta_size * sizeof(uint16_t), hipMemcpyHostToDevice));
    // Toeplitz key windows per (input byte position, byte value) (rss_host.h): the hash of a
    // 12-byte input is the XOR of 12 table entries
    {
        std::vector<uint32_t> tab(12 * 256);
        rss_key_table(conf->key, reinterpret_cast<uint32_t(*)[256]>(tab.data()));
        HIPC(c, hipMemcpy(c->rss_ktab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    RssArgs &r = c->rss;
    memset(&r, 0, sizeof(r));
    r.reta = c->rss_reta;
    r.ktab = c->rss_ktab;
    r.qid = c->rss_qid;
    r.hist = c->rss_hist;
    r.reta_size = conf->reta_size;
    r.n_queues = conf->n_queues;
    uint32_t qb = 0;
    while ((1u << qb) < conf->n_queues) ++qb;
    r.q_bits = qb;
    r.hash_types = conf->hash_types;
    c->rss_ready = true;
    return 0;
}

int udpdk_gpu_rss(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rss_out_t *o)
{
    if (!c || !bt || !o || !c->rss_ready) return -EINVAL;
    if (bt->n > c->max_frames || bt->frames_bytes >= (1ull << 32)) return -EINVAL;
    if (bt->n && (!bt->frames_dev || !bt->offset_dev || !bt->length_dev || !o->hash_dev ||
                  !o->queue_off_dev || !o->queue_pkt_dev))
        return -EINVAL;
    if (!o->queue_off_dev) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int r = join_pipes(c); if (r) return r; }
    hipStream_t st = c->stream;
    RssArgs a = c->rss;
    const uint32_t S = a.n_queues;
    if (!bt->n) {
        HIPC(c, hipMemsetAsync(o->queue_off_dev, 0, (S + 1) * sizeof(uint32_t), st));
        return 0;
    }
    a.frames = bt->frames_dev;
    a.offset = bt->offset_dev;
    a.length = bt->length_dev;
    a.ptype = bt->ptype_dev;
    a.hash = o->hash_dev;
    a.queue_pkt = o->queue_pkt_dev;
    a.frames_bytes = bt->frames_bytes;
    a.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
    a.n = bt->n;
    const uint32_t tiles = ceil_div(bt->n, RSS_TILE);
    a.n_tiles = tiles;
    a.qmajor = tiles * S <= RSS_BASE_MAX ? 1u : 0u;
    // queue-major histogram: the last rss_hash workgroup scans it (no rss_base launch)
    // (only for small histograms: at 4 M frames x 8 queues the one-workgroup tail scan of 32 K
    // entries cost more than the 1024-thread rss_base launch, 90.7 vs 84.7 us per call; at 1 M
    // frames 25.5 vs 26.0, same-box A/B)
    const bool fuse = a.qmajor && !c->rss_no_fuse && tiles * S <= RSS_FUSE_MAX_ENTRIES;
    a.fuse = fuse ? c->rss_fuse : nullptr;
    a.queue_off = o->queue_off_dev;
    a.total = c->rss_total;
    if (c->rss_trace)                          // UDPDK_RSS_TRACE: which queue-base form this call takes
        fprintf(stderr, "rss tiles %u queues %u base %s\n", tiles, S, fuse ? "fused" : a.qmajor ? "one" : "3pass");
    hipLaunchKernelGGL(rss_hash, dim3(tiles), dim3(RSS_BLOCK), 0, st, a);
    HIPC(c, hipGetLastError());
    ScanArgs sa;
    sa.hist = c->rss_hist;
    sa.partial = c->rss_partial;
    sa.lane_off = o->queue_off_dev;
    sa.total = c->rss_total;
    sa.tot = nullptr;
    sa.n_elems = tiles * S;
    sa.n_tiles = tiles;
    sa.n_lanes = S;
    if (fuse) {
        // (the bases were written by rss_hash's last workgroup)
    } else if (a.qmajor) {
        hipLaunchKernelGGL(rss_base, dim3(1), dim3(1024), 0, st, c->rss_hist.p, tiles * S, tiles,
                           o->queue_off_dev, c->rss_total.p);
    } else {
        const uint32_t nc = ceil_div(tiles, SCAN_COL_CHUNK);
        const dim3 grid(nc, ceil_div(S, (uint32_t)SCAN_BLOCK));
        hipLaunchKernelGGL(rx_scan_reduce, grid, dim3(SCAN_BLOCK), 0, st, sa);
        hipLaunchKernelGGL(rx_scan_top, dim3(1), dim3(SCAN_TOP_BLOCK), 4u * S, st, sa, nc);
        hipLaunchKernelGGL(rx_scan_down, grid, dim3(SCAN_BLOCK), 0, st, sa);
    }
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(rss_scatter, dim3(tiles), dim3(RSS_BLOCK), 0, st, a);
    HIPC(c, hipGetLastError());
    return 0;
}

int udpdk_gpu_frag_table_create(udpdk_gpu_ctx *c, const udpdk_frag_table_cfg_t *cfg)
{
    if (!c || !cfg) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int r = join_pipes(c); if (r) return r; }
    HIPC(c, hipStreamSynchronize(c->stream));
    reasm_destroy(c->reasm);
    c->reasm = nullptr;
    return reasm_create(&c->reasm, c->device, c->max_frames, cfg, &c->last_err);
}

static int reassemble(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *meta_dev, uint64_t tms,
                      udpdk_reasm_out_t *o, bool inplace)
{
    if (!c || !bt || !o) return -EINVAL;
    if (!c->reasm) return -EINVAL;
    if (bt->n && (!bt->frames_dev || !bt->offset_dev || !bt->length_dev || !meta_dev)) return -EINVAL;
    if (bt->frames_bytes >= (1ull << 32) || bt->n > c->max_frames) return -EINVAL;
    HIPC(c, hipSetDevice(c->device));
    { int r = join_pipes(c); if (r) return r; }
    return reasm_run(c->reasm, c->stream, bt, meta_dev, tms, o, &c->last_err, inplace);
}

int udpdk_gpu_rx_reassemble(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const uint32_t *meta_dev,
                            uint64_t tms, udpdk_reasm_out_t *o)
{
    return reassemble(c, bt, meta_dev, tms, o, false);
}

int udpdk_gpu_rx_reassemble_inplace(udpdk_gpu_ctx *c, udpdk_rx_batch_t *bt, const uint32_t *meta_dev,
                                    uint64_t tms, udpdk_reasm_out_t *o)
{
    return reassemble(c, bt, meta_dev, tms, o, true);
}

uint64_t udpdk_gpu_tx_span(uint32_t len, uint32_t mtu, uint32_t *n_frames)
{
    uint32_t nf = 1;
    uint64_t span = (uint64_t)len + 42u;
    if (mtu >= 68u && (mtu - 20u) % 8u == 0 && (uint64_t)len + 42u > mtu) {
        nf = (uint32_t)(((uint64_t)len + 8u + (mtu - 20u) - 1u) / (mtu - 20u));
        span = (uint64_t)len + 8u + 34ull * nf;
    }
    if (n_frames) *n_frames = nf;
    return span;
}

int udpdk_gpu_tx_build(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_tx_batch_t *bt,
                       const udpdk_tx_out_t *o)
{
    return udpdk_gpu_tx_build_mtu(c, cfg, bt, o, 0);
}

int udpdk_gpu_tx_build_mtu(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg,
                           const udpdk_tx_batch_t *bt, const udpdk_tx_out_t *o, uint32_t mtu)
{
    return udpdk_gpu_tx_build_flags(c, cfg, bt, o, mtu, 0u);
}

int udpdk_gpu_tx_build_flags(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg,
                             const udpdk_tx_batch_t *bt, const udpdk_tx_out_t *o, uint32_t mtu,
                             uint32_t flags)
{
    return udpdk_gpu_tx_build_neigh(c, cfg, bt, o, mtu, flags, nullptr);
}

int udpdk_gpu_tx_build_neigh(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg,
                             const udpdk_tx_batch_t *bt, const udpdk_tx_out_t *o, uint32_t mtu,
                             uint32_t flags, const uint32_t *dmac_dev)
{
    if (!c || !cfg || !bt || !o) return -EINVAL;
    if ((uintptr_t)dmac_dev & 7u) return -EINVAL;
    if (flags & ~UDPDK_TX_UDP_CKSUM) return -EINVAL;
    if (mtu && (mtu < 68u || mtu > 65535u || (mtu - 20u) % 8u)) return -EINVAL;
    if (!bt->n) return 0;
    if (!bt->payload_dev || !bt->payload_off_dev || !bt->payload_len_dev || !bt->sockfd_dev ||
        !bt->dst_ip_dev || !bt->dst_port_dev || !o->frames_dev || !o->frame_off_dev) return -EINVAL;
    if (!c->slots || !c->n_slots) return -EINVAL;
    if (bt->payload_bytes >= (1ull << 32) || o->frames_bytes >= (1ull << 32)) return -EINVAL;
    if (((uintptr_t)o->frames_dev & 15u) || ((uintptr_t)bt->payload_dev & 15u)) return -EINVAL;
    { int r = on_ctx_stream(c); if (r) return r; }
    TxNeighArgs ta;
    ta.dmac = dmac_dev;
    ta.payload = bt->payload_dev;
    ta.payload_off = bt->payload_off_dev;
    ta.payload_len = bt->payload_len_dev;
    ta.sockfd = bt->sockfd_dev;
    ta.dst_ip = bt->dst_ip_dev;
    ta.dst_port = bt->dst_port_dev;
    ta.frame_off = o->frame_off_dev;
    ta.slots = c->slots;
    ta.frames = o->frames_dev;
    ta.n = bt->n;
    ta.n_slots = c->n_slots;
    ta.payload_bytes = (uint32_t)bt->payload_bytes;
    // a dword comes back from a buffer load only if it ends inside the range: a
    // payload's last bytes are read by a byte-aligned load whose last dword may end up to 3
    // bytes past payload_bytes, inside the caller's UDPDK_GPU_FRAMES_TAILROOM
    ta.payload_rsrc = (uint32_t)std::min<uint64_t>((bt->payload_bytes + 3 + 3) & ~3ull, 0xFFFFFFFCull);
    ta.frames_bytes = (uint32_t)o->frames_bytes;
    ta.src_ip = cfg->src_ip;
    ta.mtu = mtu;
    uint8_t mac[12];
    memcpy(mac, cfg->dst_mac, 6);   // Ethernet d_addr first (udpdk_syscall.c:317)
    memcpy(mac + 6, cfg->src_mac, 6);
    memcpy(ta.mac_lo, mac, 12);
    const uint32_t groups = ceil_div(bt->n, 64);
    // waves per group of 64 datagrams: up to 4 while groups alone would leave the chip under
    // ~16 K waves (their chunk sweeps split between them)
    ta.parts = std::max<uint32_t>(1u, std::min<uint32_t>(4u, 16384u / std::max<uint32_t>(groups, 1u)));
    if (c->knobs.tx_parts) ta.parts = c->knobs.tx_parts;
    // the checksum form: one wave per group (a datagram's sum is kept by the wave that sweeps
    // it and patched in behind that wave's own stores); UDPDK_TX_PARTS does not apply
    if (flags & UDPDK_TX_UDP_CKSUM) ta.parts = 1u;
    const uint32_t grid = std::min<uint32_t>(ceil_div(groups * ta.parts, TX_BLOCK / 64), c->knobs.tx_grid);
    // (without MACs of their own the datagrams take the forms, and the argument block, they always took)
    if (dmac_dev) {
        if (flags & UDPDK_TX_UDP_CKSUM)
            return launch_timed(c, c->stream, UDPDK_K_TX_BUILD, tx_build<true, true>, dim3(grid), dim3(TX_BLOCK), ta);
        return launch_timed(c, c->stream, UDPDK_K_TX_BUILD, tx_build<false, true>, dim3(grid), dim3(TX_BLOCK), ta);
    }
    const TxArgs &tb = ta;
    if (flags & UDPDK_TX_UDP_CKSUM)
        return launch_timed(c, c->stream, UDPDK_K_TX_BUILD, tx_build<true, false>, dim3(grid), dim3(TX_BLOCK), tb);
    return launch_timed(c, c->stream, UDPDK_K_TX_BUILD, tx_build<false, false>, dim3(grid), dim3(TX_BLOCK), tb);
}

namespace {

// Argument checks shared by udpdk_gpu_tx_reply_plan and udpdk_gpu_tx_reply: nothing is enqueued
// unless all pass.
int reply_check(const udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *lanes,
                uint32_t first, uint32_t count, uint32_t mtu, uint64_t out_cap,
                const udpdk_tx_reply_plan_t *pl)
{
    if (!c || !bt || !lanes || !pl) return -EINVAL;
    if (mtu && (mtu < 68u || mtu > 65535u || (mtu - 20u) % 8u)) return -EINVAL;
    if (lanes->n_lanes == 0 || lanes->n_lanes > UDPDK_GPU_MAX_LANES) return -EINVAL;
    if (bt->frames_bytes >= (1ull << 32) || out_cap >= (1ull << 32)) return -EINVAL;
    if ((uint64_t)first + count > 0xFFFFFFFFull) return -EINVAL;
    if (!bt->frames_dev || !bt->offset_dev || !bt->length_dev || !lanes->lane_off_dev ||
        !lanes->lane_pkt_dev) return -EINVAL;
    if (!pl->payload_off_dev || !pl->payload_len_dev || !pl->sockfd_dev || !pl->dst_ip_dev ||
        !pl->dst_port_dev || !pl->frame_off_dev) return -EINVAL;
    if (!c->slots || !c->n_slots) return -EINVAL;
    if (c->lane_mask != 0xFFFFFFFFu) return -EINVAL;      // compat lanes are not sockets
    return 0;
}

// The reply plan (tx_reply.hip) on the context stream: descriptors, base, placement.
int reply_enqueue(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *lanes,
                  uint32_t first, uint32_t count, const uint8_t *lane_sel_dev, uint32_t mtu,
                  uint64_t out_cap, const udpdk_tx_reply_plan_t *pl)
{
    ReplyWs &W = c->rpl;
    const uint32_t nb = ceil_div(count, RPL_TILE);
    int rc;
    if ((rc = W.row.ensure(c, (size_t)nb * RPL_ROW)) || (rc = W.base.ensure(c, nb)) || (rc = W.res.ensure(c))) return rc;
    ReplyArgs ra;
    ra.frames = bt->frames_dev;
    ra.offset = bt->offset_dev;
    ra.length = bt->length_dev;
    ra.lane_off = lanes->lane_off_dev;
    ra.lane_pkt = lanes->lane_pkt_dev;
    ra.lane_sel = lane_sel_dev;
    ra.payload_off = pl->payload_off_dev;
    ra.payload_len = pl->payload_len_dev;
    ra.sockfd = pl->sockfd_dev;
    ra.dst_ip = pl->dst_ip_dev;
    ra.dst_port = pl->dst_port_dev;
    ra.frame_off = pl->frame_off_dev;
    ra.row = W.row;
    ra.base = W.base;
    ra.res = W.res.dev;
    ra.first = first;
    ra.count = count;
    ra.n = bt->n;
    ra.n_lanes = lanes->n_lanes;
    ra.lane_cap = lanes->lane_cap;
    ra.frames_bytes = (uint32_t)bt->frames_bytes;
    ra.rsrc_bytes = frames_rsrc_bytes(bt->frames_bytes);
    ra.mtu = mtu;
    ra.out_cap = (uint32_t)out_cap;
    ra.n_blocks = nb;
    hipLaunchKernelGGL(tx_reply_desc, dim3(nb), dim3(RPL_BLOCK), 0, c->stream, ra);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(tx_reply_base, dim3(1), dim3(RPL_BASE_BLOCK), 0, c->stream, ra);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(tx_reply_place, dim3((uint32_t)(((uint64_t)count + RPL_TILE) / RPL_TILE)),
                       dim3(RPL_BLOCK), 0, c->stream, ra);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

} // namespace

int udpdk_gpu_tx_reply_geometry(uint32_t count, uint32_t *entries_per_block, uint32_t *n_blocks)
{
    if (!entries_per_block || !n_blocks) return -EINVAL;
    *entries_per_block = RPL_TILE;
    *n_blocks = std::max<uint32_t>(1u, ceil_div(count, RPL_TILE));
    return 0;
}

int udpdk_gpu_tx_reply_plan(udpdk_gpu_ctx *c, const udpdk_rx_batch_t *bt, const udpdk_rx_lanes_t *lanes,
                            uint32_t first, uint32_t count, const uint8_t *lane_sel_dev, uint32_t mtu,
                            uint64_t out_cap, const udpdk_tx_reply_plan_t *pl)
{
    int rc = reply_check(c, bt, lanes, first, count, mtu, out_cap, pl);
    if (rc || !count) return rc;
    if ((rc = on_ctx_stream(c))) return rc;
    return reply_enqueue(c, bt, lanes, first, count, lane_sel_dev, mtu, out_cap, pl);
}

int udpdk_gpu_tx_reply(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_rx_batch_t *bt,
                       const udpdk_rx_lanes_t *lanes, uint32_t first, uint32_t count,
                       const uint8_t *lane_sel_dev, uint32_t mtu, uint32_t flags,
                       uint8_t *frames_out_dev, uint64_t out_cap, const udpdk_tx_reply_plan_t *pl)
{
    if (!cfg || !frames_out_dev || (flags & ~UDPDK_TX_UDP_CKSUM)) return -EINVAL;
    int rc = reply_check(c, bt, lanes, first, count, mtu, out_cap, pl);
    if (rc) return rc;
    if (((uintptr_t)frames_out_dev & 15u) || ((uintptr_t)bt->frames_dev & 15u)) return -EINVAL;
    if (!count) return 0;
    if ((rc = on_ctx_stream(c))) return rc;
    if ((rc = reply_enqueue(c, bt, lanes, first, count, lane_sel_dev, mtu, out_cap, pl))) return rc;
    const udpdk_tx_batch_t tb = {bt->frames_dev, bt->frames_bytes, pl->payload_off_dev, pl->payload_len_dev,
                                 pl->sockfd_dev, pl->dst_ip_dev, pl->dst_port_dev, count};
    const udpdk_tx_out_t to = {frames_out_dev, out_cap, pl->frame_off_dev};
    return udpdk_gpu_tx_build_flags(c, cfg, &tb, &to, mtu, flags);
}

int udpdk_gpu_tx_reply_stats(udpdk_gpu_ctx *c, udpdk_tx_reply_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    const int rc = ctx_result(c, c->rpl.res);
    if (rc) return rc;
    const ReplyResult *r = c->rpl.res.host;
    st->bytes_needed = r->bytes_needed;
    st->replied = r->replied;
    st->skipped = r->skipped;
    st->bad_index = r->bad_index;
    st->unselected = r->unselected;
    st->no_room = r->no_room;
    st->frames = r->frames;
    return st->no_room ? -ENOSPC : 0;
}

namespace {

// Argument checks shared by udpdk_gpu_tx_segment_plan and udpdk_gpu_tx_segment: nothing is enqueued
// unless all pass.
int segment_check(const udpdk_gpu_ctx *c, const udpdk_tx_sends_t *sd, uint32_t mtu, uint64_t out_cap,
                  const udpdk_tx_segment_plan_t *pl)
{
    if (!c || !sd || !pl) return -EINVAL;
    if (mtu && (mtu < 68u || mtu > 65535u || (mtu - 20u) % 8u)) return -EINVAL;
    if (sd->payload_bytes >= (1ull << 32) || out_cap >= (1ull << 32)) return -EINVAL;
    if (pl->max_segs == 0 || (uint64_t)sd->k + pl->max_segs >= (1ull << 32)) return -EINVAL;
    if (!sd->payload_dev || !sd->payload_off_dev || !sd->payload_len_dev || !sd->gso_size_dev || !sd->sockfd_dev ||
        !sd->dst_ip_dev || !sd->dst_port_dev) return -EINVAL;
    if (!pl->payload_off_dev || !pl->payload_len_dev || !pl->sockfd_dev || !pl->dst_ip_dev || !pl->dst_port_dev ||
        !pl->frame_off_dev || !pl->seg_off_dev) return -EINVAL;
    return 0;
}

// The segment plan (tx_segment.hip) on the context stream: rows, base, placement, expansion.
int segment_enqueue(udpdk_gpu_ctx *c, const udpdk_tx_sends_t *sd, uint32_t mtu, uint32_t seg_limit,
                    uint64_t out_cap, const udpdk_tx_segment_plan_t *pl)
{
    SegWs &W = c->seg;
    const uint32_t nb = ceil_div(sd->k, SEG_SEND_TILE);
    int rc;
    if ((rc = W.row.ensure(c, (size_t)nb * SEG_ROW)) || (rc = W.base.ensure(c, 2u * (size_t)nb)) ||
        (rc = W.send_base.ensure(c, sd->k)) || (rc = W.res.ensure(c))) return rc;
    SegArgs sa;
    sa.s_payload_off = sd->payload_off_dev;
    sa.s_payload_len = sd->payload_len_dev;
    sa.s_gso = sd->gso_size_dev;
    sa.s_sockfd = sd->sockfd_dev;
    sa.s_dst_ip = sd->dst_ip_dev;
    sa.s_dst_port = sd->dst_port_dev;
    sa.payload_off = pl->payload_off_dev;
    sa.payload_len = pl->payload_len_dev;
    sa.sockfd = pl->sockfd_dev;
    sa.dst_ip = pl->dst_ip_dev;
    sa.dst_port = pl->dst_port_dev;
    sa.frame_off = pl->frame_off_dev;
    sa.seg_off = pl->seg_off_dev;
    sa.send_base = W.send_base;
    sa.row = W.row;
    sa.base = W.base;
    sa.res = W.res.dev;
    sa.k = sd->k;
    sa.max_segs = pl->max_segs;
    sa.payload_bytes = (uint32_t)sd->payload_bytes;
    sa.mtu = mtu;
    sa.seg_limit = seg_limit;
    sa.out_cap = (uint32_t)out_cap;
    sa.n_blocks = nb;
    hipLaunchKernelGGL(tx_segment_rows, dim3(nb), dim3(SEG_BLOCK), 0, c->stream, sa);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(tx_segment_base, dim3(1), dim3(SEG_BASE_BLOCK), 0, c->stream, sa);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(tx_segment_place, dim3((uint32_t)(((uint64_t)sd->k + SEG_SEND_TILE) / SEG_SEND_TILE)),
                       dim3(SEG_BLOCK), 0, c->stream, sa);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(tx_segment_expand, dim3((uint32_t)(((uint64_t)pl->max_segs + SEG_TILE) / SEG_TILE)),
                       dim3(SEG_BLOCK), 0, c->stream, sa);
    HIPC(c, hipGetLastError());
    W.res.ran = true;
    return 0;
}

} // namespace

uint64_t udpdk_gpu_tx_segment_span(uint32_t len, uint32_t gso, uint32_t mtu, uint32_t *nseg, uint32_t *n_frames)
{
    uint32_t ns = 1, nf = 0;
    uint64_t span;
    if (gso == 0 || len <= gso) {
        span = udpdk_gpu_tx_span(len, mtu, &nf);
    } else {
        const uint32_t q = len / gso, r = len % gso;
        uint32_t fq = 0, fr = 0;
        span = (uint64_t)q * udpdk_gpu_tx_span(gso, mtu, &fq) + (r ? udpdk_gpu_tx_span(r, mtu, &fr) : 0);
        ns = q + (r != 0);
        nf = q * fq + fr;
    }
    if (nseg) *nseg = ns;
    if (n_frames) *n_frames = nf;
    return span;
}

int udpdk_gpu_tx_segment_geometry(uint32_t k, uint32_t max_segs, uint32_t *sends_per_block,
                                  uint32_t *segs_per_block, uint32_t *send_blocks, uint32_t *seg_blocks)
{
    if (!sends_per_block || !segs_per_block || !send_blocks || !seg_blocks) return -EINVAL;
    *sends_per_block = SEG_SEND_TILE;
    *segs_per_block = SEG_TILE;
    *send_blocks = std::max<uint32_t>(1u, ceil_div(k, SEG_SEND_TILE));
    *seg_blocks = std::max<uint32_t>(1u, ceil_div(max_segs, SEG_TILE));
    return 0;
}

int udpdk_gpu_tx_segment_plan(udpdk_gpu_ctx *c, const udpdk_tx_sends_t *sd, uint32_t mtu, uint32_t seg_limit,
                              uint64_t out_cap, const udpdk_tx_segment_plan_t *pl)
{
    int rc = segment_check(c, sd, mtu, out_cap, pl);
    if (rc || !sd->k) return rc;
    if ((rc = on_ctx_stream(c))) return rc;
    return segment_enqueue(c, sd, mtu, seg_limit, out_cap, pl);
}

int udpdk_gpu_tx_segment(udpdk_gpu_ctx *c, const udpdk_tx_config_t *cfg, const udpdk_tx_sends_t *sd, uint32_t mtu,
                         uint32_t flags, uint32_t seg_limit, uint8_t *frames_out_dev, uint64_t out_cap,
                         const udpdk_tx_segment_plan_t *pl)
{
    if (!cfg || !frames_out_dev || (flags & ~UDPDK_TX_UDP_CKSUM)) return -EINVAL;
    int rc = segment_check(c, sd, mtu, out_cap, pl);
    if (rc) return rc;
    if (((uintptr_t)frames_out_dev & 15u) || ((uintptr_t)sd->payload_dev & 15u)) return -EINVAL;
    if (!c->slots || !c->n_slots) return -EINVAL;
    if (!sd->k) return 0;
    if ((rc = on_ctx_stream(c))) return rc;
    if ((rc = segment_enqueue(c, sd, mtu, seg_limit, out_cap, pl))) return rc;
    const udpdk_tx_batch_t tb = {sd->payload_dev, sd->payload_bytes, pl->payload_off_dev, pl->payload_len_dev,
                                 pl->sockfd_dev, pl->dst_ip_dev, pl->dst_port_dev, pl->max_segs};
    const udpdk_tx_out_t to = {frames_out_dev, out_cap, pl->frame_off_dev};
    return udpdk_gpu_tx_build_flags(c, cfg, &tb, &to, mtu, flags);
}

int udpdk_gpu_tx_segment_stats(udpdk_gpu_ctx *c, udpdk_tx_segment_stats_t *st)
{
    if (!c || !st) return -EINVAL;
    const int rc = ctx_result(c, c->seg.res);
    if (rc) return rc;
    const SegResult *r = c->seg.res.host;
    st->bytes_needed = r->bytes_needed;
    st->segs_needed = r->segs_needed;
    st->sends = r->sends;
    st->segments = r->segments;
    st->frames = r->frames;
    st->skipped = r->skipped;
    st->too_long = r->too_long;
    st->bad_range = r->bad_range;
    st->too_many = r->too_many;
    st->no_room = r->no_room;
    return st->no_room ? -ENOSPC : 0;
}

#ifdef UDPDK_STAMPS
// Diagnostic builds only (not part of the ABI headers): per-workgroup phase stamps.
int udpdk_gpu_debug_buffer(udpdk_gpu_ctx *c, void *dev)
{
    if (!c) return -EINVAL;
    c->dbg = (unsigned long long *)dev;
    return 0;
}
#endif

} // extern "C"
