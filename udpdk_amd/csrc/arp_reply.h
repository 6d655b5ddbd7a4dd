// arp_reply.h — launch constants, workspace rows and the argument block shared by the ARP reply
// kernel (arp_reply.hip) and the C-ABI host code (udpdk_gpu_ctl.hip). Device-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

constexpr int      ARP_BLOCK = 256;                       // arp_reply workgroup: 4 waves
constexpr uint32_t ARP_ROUNDS = 4;                        // frames per lane, one per round
constexpr uint32_t ARP_TILE = ARP_BLOCK * ARP_ROUNDS;     // frames per workgroup (udpdk_gpu_arp_geometry)
constexpr uint32_t ARP_SLOT = 64;                         // UDPDK_ARP_SLOT_BYTES

// per-workgroup row of the scan, field-major [ARP_ROW][n_blocks]: the counters of
// udpdk_arp_stats_t a frame can land in, in the order of ArpResult
constexpr uint32_t ARP_ROW = 9;
enum { ARP_R_ARP = 0, ARP_R_MALFORMED, ARP_R_OTHER_OP, ARP_R_OWN, ARP_R_SENDER_BAD, ARP_R_NOT_OURS, ARP_R_CONFLICT,
       ARP_R_ELIGIBLE, ARP_R_BAD_FRAME };

// the device image of udpdk_arp_stats_t: c[ARP_R_*], then replies and no_room
struct ArpResult {
    uint32_t c[ARP_ROW];
    uint32_t replies, no_room;
};

// What the scan leaves per eligible request, compacted per workgroup in frame order at
// cand[block x ARP_TILE + rank]: x = frame index, y = sender MAC bytes 0-3, z = sender MAC bytes 4-5,
// w = the sender's raw address.
typedef uint4 ArpEntry;

struct ArpArgs {
    const uint8_t  *frames;
    const uint32_t *offset;
    const uint16_t *length;
    const uint32_t *meta;
    uint8_t  *out;                 // [max_replies x ARP_SLOT] (16-byte aligned)
    uint32_t *origin;              // [max_replies]
    ArpEntry *cand;                // [n_blocks x ARP_TILE]
    uint32_t *row;                 // [ARP_ROW][n_blocks]
    uint32_t *rbase;               // [n_blocks] eligible requests before the workgroup
    unsigned long long *fuse;      // fan-in words (fanin_stage.h), zero between launches
    ArpResult *res;
    uint32_t n, n_blocks;
    uint32_t frames_bytes, rsrc_bytes;
    uint32_t max_replies;
    uint32_t src_ip;
    uint32_t mac_lo, mac_hi;       // cfg->src_mac bytes 0-3 and 4-5 as LE words
};

__global__ void arp_reply(ArpArgs a);

} // namespace udpdk
