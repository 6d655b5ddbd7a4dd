// rx_balance.h — the reuse-port balance stage (rx_balance.hip): geometry, arguments and kernels,
// shared with the host side (udpdk_gpu.hip). The compaction itself is the lane filter's
// (rx_filter.h): rx_balance_mark fills the keep masks and rows rx_filter_mark would, and
// rx_filter_base / rx_filter_write / rx_filter_copy run unchanged.
#pragma once
#include <stdint.h>

#include "rx_filter.h"

namespace udpdk {

constexpr int      BAL_BLOCK = 256;                      // rx_balance_pick: 4 waves
constexpr uint32_t BAL_STEPS = 4;                        // frames per thread
constexpr uint32_t BAL_TILE = BAL_BLOCK * BAL_STEPS;     // frames per workgroup: 1024
constexpr uint32_t BAL_KEEP_ALL = 0xFFFFFFFFu;           // chosen[i]: every delivery of frame i stays

struct BalancePickArgs {
    const uint8_t  *frames;
    const uint32_t *offset;        // [n]
    const uint32_t *meta;          // [n]
    const uint4    *port_tab;      // the uploaded bind snapshot (rx_common.h, RxArgs)
    const uint2    *binds;
    const uint8_t  *lane_rp;       // [n_lanes] nonzero: the lane's socket has SO_REUSEPORT
    const uint32_t *hash_in;       // [n] caller's flow hashes, or null: computed here
    const uint32_t *ktab;          // [12][256] Toeplitz key windows (rss_host.h)
    uint32_t *chosen;              // [n] the lane that keeps frame i's reuse-port delivery, or BAL_KEEP_ALL
    uint32_t *balanced;            // += frames with a choice among >= 2 members (zeroed before the launch)
    uint32_t rsrc_bytes;
    uint32_t n;
    uint32_t n_lanes;
    uint32_t hash_types;           // udpdk_rss_type bits of the context's RSS configuration
};

// FilterArgs first, so the rows, masks and result are where rx_filter_base / _write expect them
// (FilterArgs::flags is not used; row entry 1 counts the entries the balance removes)
struct BalanceMarkArgs {
    FilterArgs f;
    const uint32_t *chosen;        // [f.n]
    const uint8_t  *lane_rp;       // [f.n_lanes]
};

__global__ void rx_balance_pick(BalancePickArgs a);
__global__ void rx_balance_mark(BalanceMarkArgs a);

} // namespace udpdk
