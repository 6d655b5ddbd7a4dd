// neigh.h — the neighbour table's layout and hash, the destination classes (rules R1-R4 of
// udpdk_gpu_neigh_resolve, one statement for the kernel and the host), launch constants and the
// argument blocks shared by the neighbour kernels (neigh.hip) and the C-ABI host code (udpdk_gpu_ctl.hip).
// Device-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"

namespace udpdk {

// An entry is four dwords (udpdk_neigh_entry_t): the key, MAC bytes 0-3, MAC bytes 4-5 | state << 16
// | pad << 24, the stamp. The home slot of a key is the top bits of a multiplicative hash; probing is
// linear and ends at an empty key (nothing is ever deleted in place).
constexpr uint32_t NEIGH_HASH_K = 0x9E3779B1u;
constexpr uint32_t NEIGH_NONE = 0xFFFFFFFFu;
constexpr uint32_t NEIGH_SLOT = 64;                       // UDPDK_ARP_SLOT_BYTES

__host__ __device__ inline uint32_t neigh_home(uint32_t ip, uint32_t shift) { return (ip * NEIGH_HASH_K) >> shift; }

// Rules R1-R4: the class of destination `dst` and, for UDPDK_NEIGH_C_LOOKUP, its next hop. For the
// classes that carry a MAC of their own (bcast, mcast, self) *lo holds its bytes 0-3 and *hi bytes 4-5.
__host__ __device__ inline uint32_t neigh_class(uint32_t src_ip, uint32_t netmask, uint32_t gateway, uint32_t smac_lo,
                                                uint32_t smac_hi, uint32_t dst, uint32_t *hop, uint32_t *lo, uint32_t *hi)
{
    *hop = 0u;
    *lo = *hi = 0u;
    const bool onlink = ((dst ^ src_ip) & netmask) == 0u;
    if (dst == 0xFFFFFFFFu || (netmask != 0u && onlink && (dst | netmask) == 0xFFFFFFFFu)) {        // R1
        *lo = 0xFFFFFFFFu;
        *hi = 0xFFFFu;
        return UDPDK_NEIGH_C_BCAST;
    }
    if ((dst & 0xF0u) == 0xE0u) {                                                                     // R2
        // 01:00:5e, then the low 23 bits of the address (raw: its octets 1-3 are bytes 1-3)
        *lo = 0x005E0001u | ((dst & 0x7F00u) << 16);
        *hi = dst >> 16;
        return UDPDK_NEIGH_C_MCAST;
    }
    const uint32_t h = onlink ? dst : gateway;                                                        // R3
    if (h == 0u) return UDPDK_NEIGH_C_NO_ROUTE;
    *hop = h;
    if (h == src_ip) {                                                                                // R4
        *lo = smac_lo;
        *hi = smac_hi;
        return UDPDK_NEIGH_C_SELF;
    }
    return UDPDK_NEIGH_C_LOOKUP;
}

// ---- neigh_learn ----------------------------------------------------------------------------------
constexpr int      NL_BLOCK = 256;                        // 4 waves
constexpr uint32_t NL_ROUNDS = 4;                         // frames per lane, one per round
constexpr uint32_t NL_TILE = NL_BLOCK * NL_ROUNDS;        // frames per workgroup (udpdk_gpu_neigh_geometry)

// per-workgroup row of the sweep, field-major [NL_ROW][n_blocks]
constexpr uint32_t NL_ROW = 6;
enum { NL_R_ARP = 0, NL_R_MALFORMED, NL_R_OTHER_OP, NL_R_SENDER_BAD, NL_R_BAD_FRAME, NL_R_EVENTS };
// what the finishing workgroup counts per event
constexpr uint32_t NL_OUT = 6;
enum { NL_O_UPDATED = 0, NL_O_REFRESHED, NL_O_STATIC_KEPT, NL_O_CREATED, NL_O_FULL, NL_O_IGNORED };

struct NeighLearnResult {
    uint32_t c[NL_ROW];
    uint32_t o[NL_OUT];
};

// An event is an ARP request or reply whose sender may be learned, compacted per workgroup in frame
// order at cand[block x NL_TILE + rank]: x = sender address, y = sender MAC bytes 0-3, z = sender MAC
// bytes 4-5 | (a request for our address) << 16, w = frame index.
struct NeighLearnArgs {
    const uint8_t  *frames;
    const uint32_t *offset;
    const uint16_t *length;
    const uint32_t *meta;
    uint32_t *tab;                 // [4 x (mask + 1)]
    uint4    *cand;                // [n_blocks x NL_TILE]
    uint32_t *row;                 // [NL_ROW][n_blocks]
    uint32_t *rbase;               // [n_blocks] events before the workgroup
    unsigned long long *fuse;      // fan-in words (fanin_stage.h), zero between launches
    NeighLearnResult *res;
    uint32_t n, n_blocks;
    uint32_t frames_bytes, rsrc_bytes;
    uint32_t mask, shift;          // entries - 1, 32 - log2(entries)
    uint32_t src_ip;
    uint32_t mac_lo, mac_hi;       // our MAC bytes 0-3 and 4-5 as LE words
    uint32_t now;
};

__global__ void neigh_learn(NeighLearnArgs a);

// ---- neigh_resolve --------------------------------------------------------------------------------
constexpr int      NR_BLOCK = 128;                        // 2 waves, one datagram per lane
constexpr uint32_t NR_TILE = NR_BLOCK;                    // datagrams per workgroup

constexpr uint32_t NR_ROW = 7;
enum { NR_R_SKIPPED = 0, NR_R_BCAST, NR_R_MCAST, NR_R_NO_ROUTE, NR_R_SELF, NR_R_HIT, NR_R_MISS };
constexpr uint32_t NR_OUT = 4;
enum { NR_O_EXPIRED = 0, NR_O_INCOMPLETE, NR_O_INSERTED, NR_O_TABLE_FULL };

struct NeighResolveResult {
    uint32_t c[NR_ROW];
    uint32_t o[NR_OUT];
    uint32_t fallback, unresolved, requests, no_room;
};

// A miss is a datagram whose next hop has no usable entry, compacted per workgroup in index order at
// cand[block x NR_TILE + rank]: x = datagram index, y = next hop.
struct NeighResolveArgs {
    const uint32_t *dst_ip;
    const int32_t  *sockfd;
    uint32_t *dmac;                // [2 n]
    int32_t  *sockfd_out;          // [n]
    uint8_t  *state;               // [n]
    uint8_t  *req;                 // [req_cap x NEIGH_SLOT] (16-byte aligned)
    uint32_t *req_origin;          // [req_cap]
    uint32_t *tab;
    uint2    *cand;                // [n_blocks x NR_TILE]
    uint32_t *row;                 // [NR_ROW][n_blocks]
    uint32_t *rbase;               // [n_blocks]
    unsigned long long *fuse;
    NeighResolveResult *res;
    uint32_t n, n_blocks;
    uint32_t req_cap;
    uint32_t mask, shift;
    uint32_t src_ip, netmask, gateway;
    uint32_t mac_lo, mac_hi;       // our MAC
    uint32_t fb_lo, fb_hi;         // cfg->fallback_mac
    uint32_t ttl_ms, retrans_ms;   // retrans_ms >= 1
    uint32_t fallback;             // UDPDK_NEIGH_FALLBACK set
    uint32_t now;
};

__global__ void neigh_resolve(NeighResolveArgs a);

} // namespace udpdk
