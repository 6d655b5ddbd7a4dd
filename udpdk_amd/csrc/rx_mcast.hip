// rx_mcast.hip — gfx950 RX datapath, optional last stage: a socket's lane keeps a multicast
// datagram only if the socket joined the datagram's group (IP_ADD_MEMBERSHIP, per socket: Linux
// with IP_MULTICAST_ALL = 0). rx_classify matches a destination against the binding's address or
// INADDR_ANY, so a datagram to 239.1.2.3:5000 reaches every ANY:5000 socket; this stage takes it
// out of the lanes that did not ask for it. The reference has no multicast.
//
// A lane is a socket (lane_mask == 0xFFFFFFFF). lane_mc[l] == 0 exempts lane l (a socket bound to
// a specific unicast address: the demux proved the destination). Otherwise entry p of lane l with
// frame i = lane_pkt[p] stays iff the raw u32 at frame bytes 30-33 (the IPv4 destination) is
// outside 224.0.0.0/4 or (that address, l) is in the membership table (rx_mcast.h). The rule is
// per ENTRY: a frame that fans out to a joined and an unjoined lane stays in the first only.
//
//   rx_mcast_mark  rx_peer_mark's geometry and outputs (a keep mask per 64-entry chunk, a row per
//                  tile). Per wave four rounds of loads, each round all in flight before the next:
//                  the entries; lane_mc of the entries' lanes (the lane of an entry: lane_find.h,
//                  bounded by the wave's first and last entries); offset / length of the entries in
//                  checked lanes; per such entry ONE dword-aligned 8-byte buffer load at
//                  (offset + 30) & ~3, funnelled by alignbyte, which holds bytes 30-33 at any
//                  alignment and ends at or before frame byte 38. lane_mc is loaded for every
//                  lane of the wave (an entry's lane index is always below n_lanes) and selected
//                  afterwards, so the round's four loads issue together. Then the table probe, for
//                  the multicast entries only: the wave's four chunks probe side by side, one
//                  8-byte buffer load each per step of a wave-uniform loop (a chunk's lanes that
//                  are done, or were never in, address out of range), so a probe costs the wave one
//                  round trip per step of its longest chain, not one per chunk (the table is
//                  L2-resident at socket-layer sizes: 8 bytes a slot). An entry >= n goes without a descriptor or
//                  frame read (bad_index); one whose frame has length < 42 or offset + length >
//                  frames_bytes goes without a frame read (bad_frame). Lanes with nothing to read
//                  address out of range (no memory request), and a wave whose entries all lie in
//                  exempt lanes issues no descriptor or frame load at all. The buffer resource
//                  spans frames_bytes rounded up to a dword: the tailroom contract of udpdk_gpu.h,
//                  unchanged.
// Then rx_filter_base and rx_filter_write (rx_filter.hip) as for the drop filter: a stable global
// compaction keeps the lane grouping and each lane's arrival order. meta is never read.
//
// Bytes. Per entry in a checked lane: 4 (lane entry) + 1 (lane_mc, L2) + 6 (offset, length;
// gathers) + the 64-byte memory request that holds frame bytes 30-33 read, 4 (the kept entry)
// written, the keep masks 1/8 B; a multicast entry adds its probes (8 bytes each, L2). Per entry in
// an exempt lane: 4 + 1 + 4 + 1/8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_mcast.h"
#include "lane_find.h"
#include "wave.h"

namespace udpdk {

// one buffer_load_dwordx2 at a byte offset (wave.h has the one- and four-dword forms)
__device__ __forceinline__ uint2 load8(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
    return make_uint2(v[0], v[1]);
}

__global__ void __launch_bounds__(FLT_BLOCK)
rx_mcast_mark(McastMarkArgs b)
{
    __shared__ uint32_t red[FLT_WAVES][5];
    const FilterArgs &a = b.f;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, tile = blockIdx.x;
    const uint32_t din = min(a.lane_off[a.n_lanes], a.lane_cap);
    if (tile * FLT_TILE >= din) return;
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(b.frames, b.rsrc_bytes);
    const uint32_t c0 = tile * FLT_CHUNKS + w * FLT_STEPS;
    uint32_t e[FLT_STEPS];
    // round 1: the wave's entries
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) e[s] = a.lane_pkt[min((c0 + s) * 64 + lane, din - 1u)];
    // the lanes: the wave's first and last entries bound them
    uint32_t l0 = 0u, l1 = 0u;
    const uint32_t pw = (uint32_t)__builtin_amdgcn_readfirstlane((int)(c0 * 64u));
    if (pw < din) {                                                  // wave-uniform
        const uint32_t pl = min(pw + 64u * FLT_STEPS - 1u, din - 1u);
        l0 = lane_find(a.lane_off, din, pw, 0u, a.n_lanes - 1u);
        l1 = lane_find(a.lane_off, din, pl, l0, a.n_lanes - 1u);
    }
    uint32_t l[FLT_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const uint32_t p = (c0 + s) * 64 + lane;
        l[s] = l0;
        if (l1 != l0 && p < din) l[s] = lane_find(a.lane_off, din, p, l0, l1);
    }
    // round 2: lane_mc of the entries' lanes
    uint32_t mc[FLT_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool valid = (c0 + s) * 64 + lane < din && e[s] < a.n;
        const uint32_t v = b.lane_mc[l[s]];              // (unpredicated: l[s] < n_lanes whatever the entry)
        mc[s] = valid ? v : 0u;
    }
    bool need[FLT_STEPS], ok[FLT_STEPS], any = false;
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        need[s] = mc[s] != 0u;                           // (an entry that is not valid is exempt)
        ok[s] = false;
        any = any || need[s];
    }
    uint2 x[FLT_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) x[s] = make_uint2(0u, 0u);
    uint32_t sh[FLT_STEPS] = {0u, 0u, 0u, 0u};
    if (__ballot(any) != 0ull) {                         // wave-uniform: some lane is checked
        // round 3: the descriptors of the entries in checked lanes
        uint32_t o[FLT_STEPS], len[FLT_STEPS];
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            o[s] = need[s] ? b.offset[e[s]] : 0u;
            len[s] = need[s] ? (uint32_t)b.length[e[s]] : 0u;
        }
        // round 4: the destination address; lanes with nothing to read address out of range
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            ok[s] = need[s] && len[s] >= 42u && (uint64_t)o[s] + len[s] <= (uint64_t)b.frames_bytes;
            sh[s] = (o[s] + 30u) & 3u;
            x[s] = load8(fr, ok[s] ? (o[s] + 30u) & ~3u : 0xFFFFFFF0u);
        }
    }
    // the probes of the multicast entries: mcast_probe's walk (rx_mcast.h), the four chunks side by side
    const uint32_t slots = 1u << b.slots_lg;
    const __amdgpu_buffer_rsrc_t tr = make_rsrc(b.table, slots * 8u);
    uint32_t dst[FLT_STEPS], at[FLT_STEPS];
    bool group[FLT_STEPS], member[FLT_STEPS], open[FLT_STEPS], some = false;
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        dst[s] = __builtin_amdgcn_alignbyte(x[s].y, x[s].x, sh[s]);                  // bytes 30-33
        group[s] = open[s] = ok[s] && mcast_is_group(dst[s]);
        member[s] = false;
        at[s] = mcast_start(dst[s], l[s], b.slots_lg);
        some = some || open[s];
    }
    for (uint32_t k = 0; k < slots && __ballot(some) != 0ull; ++k) {                 // wave-uniform
        uint2 m[FLT_STEPS];
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) m[s] = load8(tr, open[s] ? at[s] * 8u : 0xFFFFFFF0u);
        some = false;
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            if (!open[s]) continue;
            const int r = mcast_step(m[s], dst[s], l[s]);
            member[s] = r == MCAST_HIT;
            open[s] = r == MCAST_NEXT;
            at[s] = (at[s] + 1u) & (slots - 1u);
            some = some || open[s];
        }
    }
    uint32_t cnt[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool in = (c0 + s) * 64 + lane < din, valid = in && e[s] < a.n;
        const unsigned long long keep = __ballot(valid && (!need[s] || (ok[s] && (!group[s] || member[s]))));
        if (lane == 0) a.mask[c0 + s] = keep;
        cnt[0] += (uint32_t)__popcll(keep);
        cnt[1] += (uint32_t)__popcll(__ballot(group[s] && !member[s]));
        cnt[2] += (uint32_t)__popcll(__ballot(need[s] && !ok[s]));
        cnt[3] += (uint32_t)__popcll(__ballot(group[s] && member[s]));
        cnt[4] += (uint32_t)__popcll(__ballot(in && !valid));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[w][k] = cnt[k];
    }
    __syncthreads();
    if (tid < 6) {
        // the row as rx_filter_base reads it: kept, four counts (not_member, bad_frame, member, -), bad indices
        const int src = tid <= 3 ? (int)tid : tid == 5 ? 4 : -1;
        uint32_t v = 0;
        if (src >= 0) {
#pragma unroll
            for (uint32_t i = 0; i < FLT_WAVES; ++i) v += red[i][src];
        }
        a.row[tile * FLT_ROW + tid] = v;
    }
}

} // namespace udpdk
