// rx_filter.h — the lane filter stage (rx_filter.hip): geometry, arguments and kernels, shared
// with the host side (udpdk_gpu.hip).
#pragma once
#include <stdint.h>

namespace udpdk {

constexpr int      FLT_BLOCK = 256;                      // 4 waves
constexpr uint32_t FLT_WAVES = FLT_BLOCK / 64;
constexpr uint32_t FLT_STEPS = 4;                        // 64-entry chunks per wave
constexpr uint32_t FLT_CHUNKS = FLT_WAVES * FLT_STEPS;   // chunks (keep masks) per tile
constexpr uint32_t FLT_TILE = 64 * FLT_CHUNKS;           // entries per workgroup: 1024
constexpr int      FLT_BASE_BLOCK = 256;                 // rx_filter_base: one workgroup
// per-tile row: kept, then the entries dropped per reason (ip, udp, len, ihl), then bad indices
constexpr uint32_t FLT_ROW = 8;

// the device image of udpdk_rx_drop_stats_t
struct FilterResult {
    unsigned long long dropped[4];
    uint32_t kept, removed, bad_index, truncated;
};

struct FilterArgs {
    const uint32_t *meta;          // [n]
    const uint32_t *lane_off;      // [n_lanes + 1]
    const uint32_t *lane_pkt;      // [min(lane_off[n_lanes], lane_cap)]
    uint32_t *lane_off_out;        // [n_lanes + 1]
    uint32_t *lane_pkt_out;        // [out_cap]
    unsigned long long *mask;      // [n_tiles x FLT_CHUNKS] keep masks (rx_filter_mark)
    uint32_t *row;                 // [n_tiles][FLT_ROW]
    uint32_t *base;                // [n_tiles] kept entries before the tile (rx_filter_base)
    FilterResult *res;
    uint32_t n;
    uint32_t lane_cap;
    uint32_t n_lanes;
    uint32_t flags;                // UDPDK_RX_DROP_*
    uint32_t out_cap;
    uint32_t n_tiles;              // ceil(lane_cap / FLT_TILE): the grid covers what may exist
};

__global__ void rx_filter_mark(FilterArgs a);
__global__ void rx_filter_base(FilterArgs a);
__global__ void rx_filter_write(FilterArgs a);
__global__ void rx_filter_copy(const uint32_t *off, const uint32_t *pkt, const FilterResult *res,
                               uint32_t *off_out, uint32_t *pkt_out, uint32_t n_lanes, uint32_t cap,
                               uint32_t n_tiles);

} // namespace udpdk
