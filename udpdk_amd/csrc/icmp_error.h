// icmp_error.h — launch constants, the result block and the argument block shared by the ICMP error
// kernels (icmp_error.hip) and the C-ABI host code (udpdk_gpu_ctl.hip). Device-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

constexpr int      ICMP_ERR_BLOCK = 256;              // icmp_err_scan workgroup: 4 waves
constexpr uint32_t ICMP_ERR_TILE = ICMP_ERR_BLOCK;    // frames per workgroup, one per lane
// a message of at most this many bytes ([34, 14 + tl)) is summed by its own lane (four 16-byte
// loads); a longer one by the whole wave, 16 bytes per lane per step (icmp_scan's split)
constexpr uint32_t ICMP_ERR_LANE_SUM_MAX = 64;
// Linux's icmp_err_convert, the fatal column: bit c set = destination-unreachable code c is a hard
// error (2, 3, 6-10, 13-15); codes above 15 have no entry and are soft
constexpr uint32_t ICMP_ERR_HARD_MASK = 0xE7CCu;

constexpr uint32_t ICMP_ERR_LANE_BITS = 14;           // a lane < UDPDK_GPU_MAX_LANES = 2^14 (wave_peers' key)

// the device image of udpdk_icmp_err_stats_t, field for field
constexpr uint32_t ICMP_ERR_ROW = 7;
enum { ICMP_X_ERRORS = 0, ICMP_X_MSG_BAD = 1, ICMP_X_QUOTE_BAD = 2, ICMP_X_SOFT = 3, ICMP_X_NO_SOCKET = 4,
       ICMP_X_REPORTED = 5, ICMP_X_BAD_FRAME = 6 };
struct IcmpErrResult {
    uint32_t c[ICMP_ERR_ROW];
    uint32_t pad;
};

struct IcmpErrArgs {
    const uint8_t  *frames;
    const uint32_t *offset;
    const uint16_t *length;
    const uint32_t *meta;
    const uint4    *port_tab;      // [65536] the snapshot: count, first, binding 0 (ip, sockfd | reuse << 31)
    const uint2    *binds;         // ip, sockfd | reuse << 31
    const uint2    *peer;          // [peer_n] ip, port | on << 16 (udpdk_peer_t)
    unsigned long long *err;       // [n_lanes]
    IcmpErrResult  *res;
    uint32_t n;
    uint32_t frames_bytes, rsrc_bytes;
    uint32_t our_ip;
    uint32_t n_lanes, peer_n;      // a lane >= peer_n is not connected
};

__global__ void icmp_err_clear(unsigned long long *err, uint32_t n_lanes, IcmpErrResult *res);
__global__ void icmp_err_scan(IcmpErrArgs a);

} // namespace udpdk
