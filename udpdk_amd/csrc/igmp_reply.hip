// igmp_reply.hip — gfx950 IGMPv2 membership reports for a finished RX call: the membership queries
// (RFC 2236) among the frames rx_classify left as UDPDK_V_NOT_UDP, answered on the device from the
// frames still in the staged buffer. The rules are stated in udpdk_gpu.h (udpdk_gpu_igmp_reply);
// the reference has no IGMP.
//
//   igmp_reply  IGMP_TILE frames per workgroup, IGMP_ROUNDS rounds of one frame per lane, over meta.
//               A frame whose verdict word does not make it a candidate costs its 4 bytes of meta and
//               nothing else, and a wave without a candidate in a round does nothing more in it. A
//               candidate reads its descriptor and protocol byte; an IGMP frame its header fields
//               and, in a loop of its own (queries are control traffic: a handful per batch), the
//               dwords of its IPv4 header and of its IGMP message for the two RFC 1071 sums, all
//               range-checked buffer loads. A specific query that is to be answered finds its group
//               by a linear search of groups_dev and sets the group's bit in the answer set; a
//               general query only counts. The workgroup's row holds the counts.
//               The launch's last workgroup to arrive finishes (fanin_stage.h): the row sums into the
//               result, and only when a bit is set the prefix of the set bits (sixteen groups per
//               lane) and the reports in index order, one lane per report, four aligned 16-byte
//               stores of the 64-byte slot. It leaves the answer set zeroed.
// One launch: no workgroup waits for another, and a batch without a candidate ends with the row sums.
//
// Bytes per frame: 4 (meta) + 36 / IGMP_TILE (row). Per candidate: + 6 (descriptor) + the 64-byte
// request that holds byte 23. Per report: 64 (slot) + 4 (index).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "igmp_reply.h"
#include "wave.h"
#include "fanin_stage.h"

namespace udpdk {

namespace {

constexpr int NW = IGMP_BLOCK / 64;

// the four bytes at byte offset x of the frames buffer, any alignment: two dword loads
__device__ __forceinline__ uint32_t load_u32(__amdgpu_buffer_rsrc_t fr, uint32_t x)
{
    const uint32_t A = x & ~3u;
    return __builtin_amdgcn_alignbyte(load4(fr, A + 4u), load4(fr, A), x & 3u);
}

// Whether the RFC 1071 sum over buffer bytes [s, e) verifies (s < e, any alignment and parity; an
// odd length is padded with a zero byte). The sum runs over the aligned dwords that hold the range,
// bytes outside it masked: summed at an odd address it comes out byte-swapped, and the value a sum
// that verifies folds to, 0xffff, is its own swap. At most 2^14 dwords: no overflow in 32 bits.
__device__ __forceinline__ bool cksum_verifies(__amdgpu_buffer_rsrc_t fr, uint32_t s, uint32_t e)
{
    uint32_t sum = 0u;
    for (uint64_t A = s & ~3u; A < e; A += 4u) {
        const uint32_t lo = s > A ? (uint32_t)(s - A) : 0u;               // < 4: A + 4 > s
        const uint32_t hi = (uint32_t)min((uint64_t)4u, e - A);           // >= 1
        const uint32_t lm = (1u << (8u * lo)) - 1u;
        const uint32_t hm = hi >= 4u ? 0xFFFFFFFFu : (1u << (8u * hi)) - 1u;
        sum += sum16(load4(fr, (uint32_t)A) & hm & ~lm);
    }
    return fold32(sum) == 0xFFFFu;
}

} // namespace

__global__ void __launch_bounds__(IGMP_BLOCK)
igmp_reply(IgmpQArgs a)
{
    __shared__ uint32_t red[NW][IGMP_ROW];
    __shared__ uint32_t tot[IGMP_ROW];
    __shared__ uint32_t wsum[NW];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t b = blockIdx.x, nb = a.n_blocks;
    const uint64_t f0 = (uint64_t)b * IGMP_TILE + tid;
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    // the verdict word says who is a candidate: everything below is skipped by a wave without one
    uint32_t m[IGMP_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < IGMP_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * IGMP_BLOCK;
        m[k] = i64 < a.n ? a.meta[i64] : 0xFu;
    }
    uint32_t cnt[IGMP_ROW] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < IGMP_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * IGMP_BLOCK;
        const uint32_t i = (uint32_t)i64;
        const bool cand = i64 < a.n && UDPDK_META_VERDICT(m[k]) == UDPDK_V_NOT_UDP;
        if (!__ballot(cand)) continue;                               // wave-uniform
        const uint32_t o = cand ? a.offset[i] : 0u;
        const uint32_t len = cand ? (uint32_t)a.length[i] : 0u;
        const bool fok = cand && len >= 34u && (uint64_t)o + len <= a.frames_bytes;
        // bytes 20-23: the protocol is the last; lanes with nothing to read address out of range
        const uint32_t u20 = load_u32(fr, fok ? o + 20u : OOR);
        const bool igmp = fok && (u20 >> 24) == 2u;
        bool hdr_ok = false, ck_ok = false, query = false, dst_ok = false, general = false, found = false;
        if (igmp) {                                                  // divergent: control traffic
            const uint32_t u14 = load_u32(fr, o + 14u);              // version / IHL, TOS, total length
            const uint32_t ihl4 = 4u * (u14 & 0xFu), tl = bswap16(u14 >> 16);
            hdr_ok = ihl4 >= 20u && tl >= ihl4 + 8u && 14u + tl <= len && cksum_verifies(fr, o + 14u, o + 14u + ihl4);
            if (hdr_ok) {
                const uint32_t ms = o + 14u + ihl4, me = o + 14u + tl;   // the message: 8 bytes or more
                ck_ok = cksum_verifies(fr, ms, me);
                query = ck_ok && (load_u32(fr, ms) & 0xFFu) == 0x11u;
                if (query) {
                    const uint32_t grp = load_u32(fr, ms + 4u), dst = load_u32(fr, o + 30u);
                    general = grp == 0u;
                    dst_ok = dst == (general ? IGMP_ALL_HOSTS : grp);
                    if (dst_ok && !general) {
                        for (uint32_t g = 0; g < a.n_groups; ++g) {
                            if (a.groups[g] != grp) continue;
                            found = true;
                            __hip_atomic_fetch_or(&a.bits[g >> 5], 1u << (g & 31u), __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
                            break;
                        }
                    }
                }
            }
        }
        cnt[IGMP_R_IGMP] += (uint32_t)__popcll(__ballot(igmp));
        cnt[IGMP_R_MALFORMED] += (uint32_t)__popcll(__ballot(igmp && !hdr_ok));
        cnt[IGMP_R_BAD_CKSUM] += (uint32_t)__popcll(__ballot(hdr_ok && !ck_ok));
        cnt[IGMP_R_OTHER_TYPE] += (uint32_t)__popcll(__ballot(ck_ok && !query));
        cnt[IGMP_R_BAD_DST] += (uint32_t)__popcll(__ballot(query && !dst_ok));
        cnt[IGMP_R_GENERAL] += (uint32_t)__popcll(__ballot(dst_ok && general));
        cnt[IGMP_R_NOT_MEMBER] += (uint32_t)__popcll(__ballot(dst_ok && !general && !found));
        cnt[IGMP_R_SPECIFIC] += (uint32_t)__popcll(__ballot(found));
        cnt[IGMP_R_BAD_FRAME] += (uint32_t)__popcll(__ballot(cand && !fok));
    }
    wave_counts_put(red, cnt);
    __syncthreads();
    row_store<NW, IGMP_ROW>(red, a.row + b, nb);
    if (!arrive_last<true>(a.fuse, b, nb, &s_last)) return;

    // ---- the launch's last workgroup: the counts, then the reports ----
    row_sums<IGMP_BLOCK, IGMP_ROW>(a.row, nb, red, tot);
    if (tid < IGMP_ROW) a.res->c[tid] = tot[tid];
    if (tot[IGMP_R_GENERAL] + tot[IGMP_R_SPECIFIC] == 0u) {         // (the whole workgroup: no bit is set)
        if (tid == 0) a.res->reports = a.res->no_room = 0u;
        return;
    }

    // The answer set: groups [16 tid, 16 tid + 16) are this lane's, so the reports come out in index
    // order. A general query asks for every group but 224.0.0.1.
    const uint32_t g0 = tid * IGMP_PER_LANE;
    uint32_t mine = (agent_ld(&a.bits[tid >> 1]) >> (16u * (tid & 1u))) & 0xFFFFu;
    uint32_t grp[IGMP_PER_LANE];
#pragma unroll
    for (uint32_t j = 0; j < IGMP_PER_LANE; ++j) grp[j] = g0 + j < a.n_groups ? a.groups[g0 + j] : 0u;
    if (tot[IGMP_R_GENERAL]) {
#pragma unroll
        for (uint32_t j = 0; j < IGMP_PER_LANE; ++j)
            if (g0 + j < a.n_groups && grp[j] != IGMP_ALL_HOSTS) mine |= 1u << j;
    }
    uint32_t wt;
    uint32_t r = wave_excl_scan((uint32_t)__popc(mine), &wt);
    if (lane == 0) wsum[w] = wt;
    __syncthreads();
    uint32_t total = 0u;
    for (uint32_t j = 0; j < (uint32_t)NW; ++j) {
        if (j < w) r += wsum[j];
        total += wsum[j];
    }
    const uint32_t reports = min(total, a.max_reports);
    if (tid == 0) {
        a.res->reports = reports;
        a.res->no_room = total - reports;
    }
    // every lane has read its bits: the set goes back to zeros for the next launch
    if (tid < IGMP_WORDS) agent_st(&a.bits[tid], 0u);

    const uint32_t D2 = (a.mac_lo >> 16) | (a.mac_hi << 16);        // our MAC bytes 2-5
#pragma unroll
    for (uint32_t j = 0; j < IGMP_PER_LANE; ++j) {
        if (!((mine >> j) & 1u)) continue;
        if (r < reports) {
            const uint32_t g = grp[j];
            // RFC 1071 over little-endian halves gives the checksum's two bytes in memory order
            const uint32_t ip = 0xC046u + 0x2000u + 0x0040u + 0x0201u + sum16(a.src_ip) + sum16(g) + 0x0494u;
            const uint32_t ipck = ~fold32(ip) & 0xFFFFu, ick = ~fold32(0x0016u + sum16(g)) & 0xFFFFu;
            uint4 *slot = reinterpret_cast<uint4 *>(a.out + (size_t)r * IGMP_SLOT);
            // 01 00 5e + the group's low 23 bits, our MAC, 08 00 46 c0
            slot[0] = make_uint4(0x005E0001u | ((g & 0x7F00u) << 16), (g >> 16) | (a.mac_lo << 16), D2, 0xC0460008u);
            // 00 20 00 00 40 00 01 02, the checksum, our address, the group
            slot[1] = make_uint4(0x00002000u, 0x02010040u, ipck | (a.src_ip << 16), (a.src_ip >> 16) | (g << 16));
            // 94 04 00 00 (Router Alert), 16 00, the checksum, the group
            slot[2] = make_uint4((g >> 16) | 0x04940000u, 0x00160000u, ick | (g << 16), g >> 16);
            slot[3] = make_uint4(0u, 0u, 0u, 0u);
            a.group_index[r] = g0 + j;
        }
        ++r;
    }
}

} // namespace udpdk
