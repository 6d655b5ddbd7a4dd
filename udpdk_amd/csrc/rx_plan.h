// rx_plan.h — the launch form of one udpdk_gpu_rx call as a pure host function: the environment
// knobs (parsed once per context), the workspace capacities and rx_plan(), which turns a batch's
// frame and lane counts into the tile geometry, the rx_classify form and the kernels that follow.
// Host only: no HIP runtime call, no allocation. udpdk_gpu.hip fills the argument blocks and
// launches by the plan; tools/rx_plan_check.cpp prints it on a machine without a GPU.
#pragma once
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "udpdk_gpu.h"
#include "rx_common.h"

namespace udpdk {

inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

struct RxKnobs {
    uint32_t one_lane_tile = 0;    // UDPDK_ONE_LANE_TILE (diagnostic): single-lane tile override
    uint64_t geo_cap = RX_HIST_CAP; // UDPDK_RX_HIST_CAP (diagnostic): lanes x tiles bound of the geometry
    int force_fuse = -1;           // UDPDK_RX_FUSE=0/1 (tests, A/B): fused completion off / always
    int force_tailg = 0;           // UDPDK_RX_TAILG=1/2 (tests, A/B): rx_classify<G> always
    int force_mr = -1;             // UDPDK_RX_MR=0/1 (tests, A/B): the round-ahead descriptor form
    bool no_span = false;          // UDPDK_RX_SPAN=0 (tests, A/B): no span sweep (RxArgs::span)
    int policy = 1;                // UDPDK_RX_POLICY=0 (tests, A/B): rx_classify<.., 0>, default memory policy
    bool trace = false;            // UDPDK_RX_TRACE (diagnostic): the form of every call on stderr
    uint32_t scan_cols_tiles = SCAN_COLS_MAX_TILES;   // UDPDK_RX_SCAN_COLS_TILES (tests): most tiles of the
                                                      // one-launch column scan, 0 = always reduce / top / down
    bool no_inline = false;        // UDPDK_RX_NO_INLINE (tests, A/B): always the port-table loads
    uint32_t scatter_group_frames = UDPDK_SCATTER_GROUP_FRAMES;   // UDPDK_SCATTER_GROUP_FRAMES (tests, A/B)
    uint32_t scatter_min_wg = UDPDK_SCATTER_MIN_WG;               // UDPDK_SCATTER_MIN_WG (tests, A/B)
    uint32_t tx_parts = 0;         // UDPDK_TX_PARTS=1..4 (tests): TxArgs::parts, 0 = computed per batch
                                   // (not for UDPDK_TX_UDP_CKSUM, which always runs one part)
    uint32_t tx_grid = 4096;       // UDPDK_TX_GRID>=1 (tests): tx_build's workgroup cap
    uint32_t gather_grid = 16384;  // UDPDK_GATHER_GRID>=1 (tests): rx_gather's workgroup cap
};

inline RxKnobs rx_knobs_from_env()
{
    RxKnobs k;
    if (const char *e = getenv("UDPDK_ONE_LANE_TILE")) {
        const uint32_t t = (uint32_t)atoi(e);
        if (t >= RX_TILE_MIN && t <= RX_TILE_MAX && (t & (t - 1)) == 0) k.one_lane_tile = t;
    }
    if (const char *e = getenv("UDPDK_RX_HIST_CAP")) {
        const uint64_t v = strtoull(e, nullptr, 0);
        if (v >= (1u << 16) && v <= (1u << 26)) k.geo_cap = v;
    }
    if (const char *e = getenv("UDPDK_RX_FUSE")) k.force_fuse = atoi(e) ? 1 : 0;
    k.trace = getenv("UDPDK_RX_TRACE") != nullptr;
    k.no_inline = getenv("UDPDK_RX_NO_INLINE") != nullptr;
    if (const char *e = getenv("UDPDK_RX_SCAN_COLS_TILES"))
        k.scan_cols_tiles = (uint32_t)std::min<long>(std::max<long>(atol(e), 0), (long)SCAN_COLS_MAX_TILES);
    if (const char *e = getenv("UDPDK_RX_MR")) k.force_mr = atoi(e) ? 1 : 0;
    if (const char *e = getenv("UDPDK_RX_SPAN")) k.no_span = atoi(e) == 0;
    if (const char *e = getenv("UDPDK_RX_POLICY")) k.policy = atoi(e) ? 1 : 0;
    if (const char *e = getenv("UDPDK_SCATTER_GROUP_FRAMES")) k.scatter_group_frames = (uint32_t)atoi(e);
    if (const char *e = getenv("UDPDK_SCATTER_MIN_WG")) k.scatter_min_wg = (uint32_t)atoi(e);
    if (const char *e = getenv("UDPDK_RX_TAILG")) {
        const int g = atoi(e);
        if (g == 1 || g == 2) k.force_tailg = g;
    }
    // (out-of-range values are clamped)
    if (const char *e = getenv("UDPDK_TX_PARTS")) k.tx_parts = (uint32_t)std::min(std::max(atoi(e), 1), 4);
    if (const char *e = getenv("UDPDK_TX_GRID")) k.tx_grid = (uint32_t)std::max(atoi(e), 1);
    if (const char *e = getenv("UDPDK_GATHER_GRID")) k.gather_grid = (uint32_t)std::max(atoi(e), 1);
    return k;
}

// Entries of a pipe's workspace arrays: hist and base (lanes x tiles), partial (chunks x lanes;
// rx_tile_base's tile prefix on the single-lane path) and tile_cnt (counter rows).
struct RxCaps {
    size_t hist_cap, partial_cap, tiles_cap;
};

inline RxCaps rx_caps(uint32_t max_frames, uint32_t max_lanes, uint64_t geo_cap)
{
    const uint64_t e_cap = std::max<uint64_t>(std::max<uint64_t>(RX_HIST_CAP, geo_cap) + max_lanes,
                                              (uint64_t)ceil_div(max_frames, RX_TILE_MAX) * max_lanes);
    return {(size_t)e_cap, (size_t)(e_cap / SCAN_COL_CHUNK + max_lanes + 1),
            (size_t)ceil_div(max_frames, RX_TILE_MIN) + 1};
}

inline void geometry(uint32_t n, uint32_t lanes, uint32_t *T, uint32_t *tiles, uint64_t cap = RX_HIST_CAP)
{
    uint32_t t = RX_TILE_MIN;
    while (t < RX_TILE_MAX && (uint64_t)ceil_div(n, t) * lanes > cap) t *= 2;
    *T = t;
    *tiles = std::max<uint32_t>(1u, ceil_div(n, t));
}

enum RxScan { RX_SCAN_NONE, RX_SCAN_COLS512, RX_SCAN_COLS1024, RX_SCAN_3PASS };

struct RxPlan {
    int err = 0;                          // -EINVAL: the geometry does not fit the workspace (RxCaps)
    uint32_t T = 0, tiles = 0;            // frames per classify tile, tiles (rx_classify's grid)
    bool one_lane = false;                // classify (+ rx_compact1); else classify + scan + scatter
    bool cols = false, hist16 = false;    // rx_scan_cols (else reduce / top / down); u16 tile histograms
    bool spec = false, fuse = false;      // RxArgs::spec_pkt; fused completion: no launch after classify
    int tailg = 2;                        // rx_classify<G, MR, POL>'s G ...
    bool mr = false, span = false;        // ... and MR; the span sweep (RxArgs::span)
    uint32_t cls_lds = 0;                 // rx_classify's dynamic LDS bytes (the span sweep's ring included)
    bool tile_base = false;               // rx_tile_base runs before rx_compact1
    uint32_t compact_grid = 0;            // rx_compact1's workgroups
    bool scatterw = false;                // rx_scatterw<W> over scatter tiles of G classify tiles; else rx_scatter
    uint32_t G = 1, W = SCATTER_WAVES;
    RxScan scan = RX_SCAN_NONE;
    uint32_t lb = 0, scan_grid = 0, nc = 0;   // rx_scan_cols: log2 lanes per workgroup, workgroups; 3-pass: chunks per lane
};

// rx_scan_cols<block>'s lanes per workgroup (log2): as many as the chunking allows (<= 64, 256 B
// rows), then fewer until the grid has >= UDPDK_SCAN_MIN_WG workgroups, never under 8 lanes (32 B
// row segments). Wider rows beat more workgroups: at 1024 lanes x 1024 tiles, 16-lane columns
// (64 workgroups) take 8.0 us, 8-lane (128) 11.9 us, 4-lane (256) 13.0 us.
inline uint32_t pick_lb(uint32_t block, uint32_t tiles, uint32_t lanes)
{
    const uint32_t cmin = ceil_div(tiles, scan_cols_tpt(block));
    uint32_t lb = 0;
    while ((2u << lb) <= std::min<uint32_t>(64u, block / cmin)) ++lb;
    while (lb > 3 && ceil_div(lanes, 1u << lb) < UDPDK_SCAN_MIN_WG) --lb;
    return lb;
}

// The form of a call of n > 0 frames over S lanes under a bind snapshot of fan-out max_fanout.
// tail_recent: a call within the last UDPDK_HINT_WINDOW ran a tail pass (RxArgs::hint).
inline RxPlan rx_plan(uint32_t n, uint32_t S, uint32_t max_fanout, bool tail_recent, const RxKnobs &k,
                      const RxCaps &caps)
{
    RxPlan p;
    geometry(n, S, &p.T, &p.tiles, k.geo_cap);
    p.one_lane = S == 1 && max_fanout <= 1;
    if (p.one_lane && k.one_lane_tile) {   // diagnostic override
        p.T = k.one_lane_tile;
        p.tiles = std::max<uint32_t>(1u, ceil_div(n, p.T));
    }
    const uint32_t T = p.T, tiles = p.tiles;
    if ((uint64_t)S * tiles > caps.hist_cap || tiles > caps.tiles_cap) {
        p.err = -EINVAL;
        return p;
    }
    // the one-launch column scan while each thread's tile chunk fits its registers; beyond (very
    // large batches over few lanes) the reduce / top / down chain over u32 counts
    // (UDPDK_RX_SCAN_COLS_TILES lowers the bound: the chain then rescans the histogram in place and
    // the scatter reads its rows there, row G s for a scatter tile of G classify tiles, as past the bound)
    p.cols = !p.one_lane && tiles <= k.scan_cols_tiles;
    // u16 tile histograms where a lane's count per tile cannot pass 2^16 (no fan-out): half the
    // bytes classify stores at its tile ends and the scan reads
    p.hist16 = p.cols && max_fanout <= 1;
    p.spec = UDPDK_SPEC_COMPACT && p.one_lane && T == (uint32_t)RX_ROUND && CLS_BLOCK * 4 == RX_ROUND;
    // fused completion whenever it applies: a call with a short tile repairs its lane inside the
    // same launch (classify_complete), so no form switching follows a stray frame
    p.fuse = p.spec && tiles <= UDPDK_FUSE_MAX_TILES && k.force_fuse != 0;
    // the single-lane path takes rx_classify<1> while no recent call ran a tail pass; both forms
    // are exact for any batch, the hint only picks the faster
    p.tailg = k.force_tailg ? k.force_tailg : (p.one_lane && !tail_recent) ? 1 : 2;
    // tiles of several rounds (many lanes: config 5's 8192-frame tiles) take the form that loads
    // each next round's descriptors a round ahead
    p.mr = k.force_mr >= 0 ? k.force_mr == 1 : T > (uint32_t)RX_ROUND;
    // the span sweep: the long-frame form of one-round tiles (its LDS ring after the carve)
    p.cls_lds = classify_lds_bytes(S, T, p.hist16);
    p.span = p.tailg == 2 && !p.mr && T == (uint32_t)RX_ROUND && !k.no_span &&
             p.cls_lds + SPAN_LDS_BYTES <= 160u * 1024u - 1024u;
    if (p.span) p.cls_lds += SPAN_LDS_BYTES;
    if (p.fuse) return p;
    if (p.one_lane) {
        // past a few thousand tiles each workgroup's sum over its predecessors costs more than
        // one extra launch scanning the counts once
        p.tile_base = tiles > COMPACT1_DIRECT_TILES && tiles <= caps.partial_cap;
        // speculative: grid-stride over the tiles after the call's first flagged one (usually
        // none); the grid size does not change the all-full call's cost (same-box A/B: 32, 128
        // and 1024 workgroups all 4.8-5.0 us), 256 keeps a flagged call's rewrite wide
        p.compact_grid = p.spec ? std::min<uint32_t>(tiles, UDPDK_COMPACT1_SPEC_GRID) : tiles;
        return p;
    }
    // rx_scatterw: G classify tiles per scatter workgroup while the scatter tile stays within
    // UDPDK_SCATTER_GROUP_FRAMES, its (frame, position) pairs fit the LDS counter region (8 B each
    // in 2 W S bytes) and the grid keeps UDPDK_SCATTER_MIN_WG workgroups; the column scan then
    // writes only the base rows of each group's first tile
    p.scatterw = max_fanout <= 1 && S <= SCATTERW_MAX_LANES;
    while (p.scatterw && p.G < tiles) {
        const uint32_t g2 = 2 * p.G, f2 = g2 * T;
        const uint32_t w2 = f2 > 64u * SCATTER_WAVES * SCATTERW_MV ? 2 * SCATTER_WAVES : SCATTER_WAVES;
        if (f2 > k.scatter_group_frames || f2 > 64u * w2 * SCATTERW_MV || 8ull * f2 > 2ull * w2 * S ||
            (S & 1u) || ceil_div(tiles, g2) < k.scatter_min_wg)
            break;
        p.G = g2;
        p.W = w2;
    }
    if (p.cols) {
        // workgroups of 1024 threads when that still leaves >= 16-lane columns (config 5: 11.2-11.8
        // -> 7.3-7.7 us against 256 threads; more waves per CU for the column loads' latency),
        // else 512 (config 4's 1024 lanes x 1024 tiles: 10.3-10.4 -> 8.9-9.1 us)
        p.lb = pick_lb(1024u, tiles, S);
        p.scan = p.lb >= 4 ? RX_SCAN_COLS1024 : RX_SCAN_COLS512;
        if (p.lb < 4) p.lb = pick_lb(512u, tiles, S);
        p.scan_grid = ceil_div(S, 1u << p.lb);
    } else {
        p.scan = RX_SCAN_3PASS;
        p.nc = ceil_div(tiles, SCAN_COL_CHUNK);
        if ((uint64_t)p.nc * S > caps.partial_cap) p.err = -EINVAL;
    }
    return p;
}

// UDPDK_RX_TRACE's two fragments: "classify<G>[ fused]" of the first line, and what follows
// "form " on the second (the geometry and the launches the call takes after classify).
inline void rx_plan_trace(const RxPlan &p, char cls[32], char form[128])
{
    static_assert(SCATTER_WAVES == 8, "the trace line names rx_scatterw's forms by their waves");
    static const char *const scan[] = {"none", "cols512", "cols1024", "3pass"};
    const char *scatter = p.fuse ? "fused" : p.one_lane ? "compact1" : !p.scatterw ? "scatter1"
                          : p.W == SCATTER_WAVES ? "scatterw8" : "scatterw16";
    snprintf(cls, 32, "classify<%d>%s", p.tailg, p.fuse ? " fused" : "");
    snprintf(form, 128, "T %u tiles %u mr %d hist16 %d scan %s scatter %s G %u", p.T, p.tiles, p.mr ? 1 : 0,
             p.hist16 ? 1 : 0, scan[p.scan], scatter, p.G);
}

} // namespace udpdk
