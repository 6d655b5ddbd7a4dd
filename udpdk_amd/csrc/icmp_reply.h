// icmp_reply.h — launch constants, workspace rows and the argument block shared by the ICMP reply
// kernels (icmp_reply.hip) and the C-ABI host code (udpdk_gpu_ctl.hip). Device-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

constexpr int      ICMP_BLOCK = 256;             // icmp_scan / icmp_build workgroup: 4 waves
constexpr uint32_t ICMP_TILE = ICMP_BLOCK;       // frames per workgroup, one per lane (udpdk_gpu_icmp_geometry)
constexpr int      ICMP_BASE_BLOCK = 256;        // icmp_base: one workgroup, a run of rows per lane
// an echo message whose bytes after the 4-byte ICMP header are at most this many is summed by its
// own lane (four 16-byte loads); a longer one by the whole wave, 16 bytes per lane per step
constexpr uint32_t ICMP_LANE_SUM_MAX = 64;
constexpr uint32_t ICMP_UNREACH_LEN = 70;        // UDPDK_ICMP_UNREACH_BYTES
constexpr uint32_t ICMP_E_UNREACH = 0x80000000u; // IcmpEntry.y: a port-unreachable error (else an echo reply)

// per-workgroup row of icmp_scan, field-major [ICMP_ROW][n_blocks]: echo requests answered, errors
// eligible, bytes of the echo replies, echo requests refused, candidates with a bad descriptor
constexpr uint32_t ICMP_ROW = 5;
enum { ICMP_R_ECHO = 0, ICMP_R_UNR = 1, ICMP_R_EBYTES = 2, ICMP_R_EBAD = 3, ICMP_R_BADF = 4 };

// the device image of udpdk_icmp_stats_t (replies = echo_replied + unreach_sent)
struct IcmpResult {
    unsigned long long bytes_needed;
    uint32_t echo_replied, unreach_sent, echo_bad, limited, no_room, bad_frame;
};

// What icmp_scan leaves per reply candidate, compacted per workgroup in frame order at
// cand[block x ICMP_TILE + rank]: x = frame index, y = reply bytes | ICMP_E_UNREACH, z = the reply's
// ICMP checksum (raw), w = the request's raw source address (the reply's destination).
typedef uint4 IcmpEntry;

struct IcmpArgs {
    const uint8_t  *frames;
    const uint32_t *offset;
    const uint16_t *length;
    const uint32_t *meta;
    uint8_t  *out;                 // replies back to back (16-byte aligned)
    uint32_t *reply_off;           // [max_replies + 1]
    uint32_t *origin;              // [max_replies]
    IcmpEntry *cand;               // [n_blocks x ICMP_TILE]
    uint32_t *row;                 // [ICMP_ROW][n_blocks]
    uint32_t *ubase;               // [n_blocks] eligible errors before the workgroup
    uint32_t *rbase;               // [n_blocks] replies before the workgroup (after the limit)
    unsigned long long *bbase;     // [n_blocks] reply bytes before the workgroup (after the limit)
    IcmpResult *res;
    uint32_t n, n_blocks;
    uint32_t frames_bytes, rsrc_bytes;
    uint32_t flags, mtu, err_limit;
    uint32_t out_cap, max_replies;
    uint32_t src_ip;
    uint32_t mac_lo[3];            // 12 MAC bytes: dst(6) src(6) as three LE dwords
};

__global__ void icmp_scan(IcmpArgs a);
__global__ void icmp_base(IcmpArgs a);
__global__ void icmp_build(IcmpArgs a);

} // namespace udpdk
