// rx_peer.h — the connected-socket peer filter (rx_peer.hip): arguments and kernel, shared with the
// host side (udpdk_gpu.hip). The compaction itself is the lane filter's (rx_filter.h):
// rx_peer_mark fills the keep masks and rows rx_filter_mark would, and rx_filter_base /
// rx_filter_write / rx_filter_copy run unchanged.
#pragma once
#include <stdint.h>

#include "rx_filter.h"

namespace udpdk {

// FilterArgs first, so the rows, masks and result are where rx_filter_base / _write expect them
// (FilterArgs::meta and ::flags are not used; row entry 1 counts the entries refused, entry 2 the
// entries whose frame descriptor is out of range)
struct PeerMarkArgs {
    FilterArgs f;
    const uint2    *peer;          // [f.n_lanes] udpdk_peer_t: x = raw ip, y = raw port | on << 16
    const uint8_t  *frames;
    const uint32_t *offset;        // [f.n]
    const uint16_t *length;        // [f.n]
    uint32_t frames_bytes;
    uint32_t rsrc_bytes;           // frames_bytes rounded up to a dword (the tailroom contract)
};

__global__ void rx_peer_mark(PeerMarkArgs a);

} // namespace udpdk
