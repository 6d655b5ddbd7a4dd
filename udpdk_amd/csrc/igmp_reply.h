// igmp_reply.h — launch constants, workspace rows and the argument block shared by the IGMP query
// responder (igmp_reply.hip) and the C-ABI host code (udpdk_gpu_ctl.hip). Device-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

constexpr int      IGMP_BLOCK = 256;                        // igmp_reply workgroup: 4 waves
constexpr uint32_t IGMP_ROUNDS = 4;                         // frames per lane, one per round
constexpr uint32_t IGMP_TILE = IGMP_BLOCK * IGMP_ROUNDS;    // frames per workgroup (udpdk_gpu_igmp_geometry)
constexpr uint32_t IGMP_SLOT = 64;                          // UDPDK_IGMP_SLOT_BYTES
constexpr uint32_t IGMP_MAX_GROUPS = 4096;                  // UDPDK_IGMP_MAX_GROUPS
constexpr uint32_t IGMP_PER_LANE = IGMP_MAX_GROUPS / IGMP_BLOCK;   // groups per lane of the finish: 16
// the answer set of the specific queries: one bit per group of groups_dev (a general query needs
// no bit: its count in the rows says that every group is asked for)
constexpr uint32_t IGMP_WORDS = IGMP_MAX_GROUPS / 32;
constexpr uint32_t IGMP_ALL_HOSTS = 0x010000E0u;            // 224.0.0.1, raw

// per-workgroup row of the sweep, field-major [IGMP_ROW][n_blocks]: the counters of
// udpdk_igmp_stats_t a frame can land in, in the order of IgmpResult
constexpr uint32_t IGMP_ROW = 9;
enum { IGMP_R_IGMP = 0, IGMP_R_MALFORMED, IGMP_R_BAD_CKSUM, IGMP_R_OTHER_TYPE, IGMP_R_BAD_DST, IGMP_R_GENERAL,
       IGMP_R_NOT_MEMBER, IGMP_R_SPECIFIC, IGMP_R_BAD_FRAME };

// the device image of udpdk_igmp_stats_t: c[IGMP_R_*], then reports and no_room
struct IgmpQResult {
    uint32_t c[IGMP_ROW];
    uint32_t reports, no_room;
};

struct IgmpQArgs {
    const uint8_t  *frames;
    const uint32_t *offset;
    const uint16_t *length;
    const uint32_t *meta;
    const uint32_t *groups;        // [n_groups] distinct raw group addresses
    uint8_t  *out;                 // [max_reports x IGMP_SLOT] (16-byte aligned)
    uint32_t *group_index;         // [max_reports]
    uint32_t *row;                 // [IGMP_ROW][n_blocks]
    uint32_t *bits;                // [IGMP_WORDS] the answer set, zero between launches
    unsigned long long *fuse;      // fan-in words (fanin_stage.h), zero between launches
    IgmpQResult *res;
    uint32_t n, n_blocks;
    uint32_t frames_bytes, rsrc_bytes;
    uint32_t n_groups, max_reports;
    uint32_t src_ip;
    uint32_t mac_lo, mac_hi;       // cfg->src_mac bytes 0-3 and 4-5 as LE words
};

__global__ void igmp_reply(IgmpQArgs a);

} // namespace udpdk
