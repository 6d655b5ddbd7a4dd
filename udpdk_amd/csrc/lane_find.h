// lane_find.h — the lane a lane-set position lies in, for the entry-parallel kernels that need it
// (tx_reply_desc, rx_balance_mark). The entries are sorted by lane, so a wave searches lane_off
// once for its first and once for its last position (wave-uniform binary searches, <= 14 steps
// each in a table of at most 64 KiB) and only a wave that spans several lanes searches per entry,
// between those two. Device-only, inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

// The largest l in [lo, hi] with min(lane_off[l], D) <= p (lo when there is none). lane_off is an
// exclusive prefix, so non-decreasing with lane_off[0] = 0; on anything else the result is still
// some index in [lo, hi].
__device__ __forceinline__ uint32_t lane_find(const uint32_t *lane_off, uint32_t D, uint32_t p, uint32_t lo,
                                              uint32_t hi)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (min(lane_off[mid], D) <= p) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

} // namespace udpdk
