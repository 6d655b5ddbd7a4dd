// rx_mcast.h — the multicast membership filter (rx_mcast.hip): the membership table's hash and
// probe, shared by host (the builder, udpdk_gpu.hip) and device (rx_mcast_mark), then the kernel and
// its arguments. The compaction itself is the lane filter's (rx_filter.h): rx_mcast_mark fills the
// keep masks and rows rx_filter_mark would, and rx_filter_base / rx_filter_write / rx_filter_copy
// run unchanged.
#pragma once
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_filter.h"

#if defined(__HIPCC__)
#define UDPDK_MCAST_HD __host__ __device__
#else
#define UDPDK_MCAST_HD
#endif

namespace udpdk {

constexpr uint32_t MCAST_MIN_SLOTS = 2u, MCAST_MAX_SLOTS = 1u << 20;

// log2 of a valid slot count (a power of two in MCAST_MIN_SLOTS..MCAST_MAX_SLOTS), 0 for any other
inline uint32_t mcast_slots_log2(uint32_t slots)
{
    if (slots < MCAST_MIN_SLOTS || slots > MCAST_MAX_SLOTS || (slots & (slots - 1u)) != 0u) return 0u;
    uint32_t lg = 0;
    while ((1u << lg) < slots) ++lg;
    return lg;
}

// The table rule of udpdk_gpu.h: where the probe of (group, lane) starts in a table of 1 << lg slots
UDPDK_MCAST_HD inline uint32_t mcast_start(uint32_t group, uint32_t lane, uint32_t lg)
{
    const uint32_t h = (group ^ (lane * 0x9E3779B1u)) * 0x85EBCA6Bu;
    return h >> (32u - lg);
}

// a table record's fields: the host's udpdk_mcast_member_t, the device's 8-byte load of one
UDPDK_MCAST_HD inline uint32_t mcast_group(const udpdk_mcast_member_t &m) { return m.group; }
UDPDK_MCAST_HD inline uint32_t mcast_lane(const udpdk_mcast_member_t &m) { return m.lane; }
#if defined(__HIPCC__)
UDPDK_MCAST_HD inline uint32_t mcast_group(const uint2 &m) { return m.x; }
UDPDK_MCAST_HD inline uint32_t mcast_lane(const uint2 &m) { return m.y; }
#endif

// One step of the probe of (group, lane): what the record at the probe's index says. The host's
// mcast_probe and the kernel's interleaved probes (rx_mcast_mark) both walk by it.
enum { MCAST_MISS = 0, MCAST_HIT = 1, MCAST_NEXT = 2 };
template <typename T>
UDPDK_MCAST_HD inline int mcast_step(const T &m, uint32_t group, uint32_t lane)
{
    if (mcast_group(m) == group && mcast_lane(m) == lane) return MCAST_HIT;
    return mcast_group(m) == 0u ? MCAST_MISS : MCAST_NEXT;
}

// Whether (group, lane) is in the table: linear probing from mcast_start, ended by a match, by an
// empty slot (group == 0) or after `slots` probes (a table with no empty slot is valid).
template <typename T>
UDPDK_MCAST_HD inline bool mcast_probe(const T *table, uint32_t lg, uint32_t group, uint32_t lane)
{
    const uint32_t slots = 1u << lg;
    uint32_t i = mcast_start(group, lane, lg);
    for (uint32_t k = 0; k < slots; ++k) {
        const int r = mcast_step(table[i], group, lane);
        if (r != MCAST_NEXT) return r == MCAST_HIT;
        i = (i + 1u) & (slots - 1u);
    }
    return false;
}

// raw address (the wire bytes as a little-endian integer): 224.0.0.0/4
UDPDK_MCAST_HD inline bool mcast_is_group(uint32_t raw_ip) { return ((raw_ip & 0xFFu) >> 4) == 0xEu; }

#if defined(__HIPCC__)
// FilterArgs first, so the rows, masks and result are where rx_filter_base / _write expect them
// (FilterArgs::meta and ::flags are not used; row entry 1 counts the entries of groups the lane did
// not join, entry 2 the entries whose frame descriptor is out of range, entry 3 the multicast
// entries kept)
struct McastMarkArgs {
    FilterArgs f;
    const uint8_t  *lane_mc;       // [f.n_lanes] non-zero: the lane's entries are checked
    const uint2    *table;         // [1 << slots_lg] udpdk_mcast_member_t: x = raw group, y = lane
    const uint8_t  *frames;
    const uint32_t *offset;        // [f.n]
    const uint16_t *length;        // [f.n]
    uint32_t slots_lg;
    uint32_t frames_bytes;
    uint32_t rsrc_bytes;           // frames_bytes rounded up to a dword (the tailroom contract)
};

__global__ void rx_mcast_mark(McastMarkArgs a);
#endif

} // namespace udpdk
