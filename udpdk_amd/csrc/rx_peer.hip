// rx_peer.hip — gfx950 RX datapath, optional last stage: a connected socket's lane keeps only the
// datagrams of its peer (udpdk_connect: POSIX's rule for a connected UDP socket; the reference's
// socket calls stop at sendto / recvfrom and leave the check of src_addr to every application).
//
// A lane is a socket (lane_mask == 0xFFFFFFFF) and peer[l] is lane l's record: on == 0, the socket
// is not connected and its lane is left as it is; otherwise entry p of lane l with frame
// i = lane_pkt[p] stays iff the raw u32 at frame bytes 26-29 (the IPv4 source address) equals
// peer[l].ip and the raw u16 at frame bytes 34-35 (the UDP source port) equals peer[l].port: the
// fields rx_gather reports as src_ip / src_port. The rule is per ENTRY: a frame that fans out to a
// connected and an unconnected lane stays in the second whatever its source is.
//
//   rx_peer_mark   rx_filter_mark's geometry and outputs (a keep mask per 64-entry chunk, a row per
//                  tile). Per wave four rounds of loads, each round all in flight before the next:
//                  the entries; the peer records of the entries' lanes (the lane of an entry:
//                  lane_find.h, bounded by the wave's first and last entries); offset / length of
//                  the entries in connected lanes; per such entry ONE dword-aligned 16-byte buffer
//                  load at (offset + 26) & ~3, funnelled by alignbyte, which holds bytes 26-35 at
//                  any alignment and ends at or before frame byte 42. An entry >= n goes without a
//                  descriptor or frame read (bad_index); one whose frame has length < 42 or
//                  offset + length > frames_bytes goes without a frame read (bad_frame). Lanes with
//                  nothing to read address out of range (no memory request), and a wave whose
//                  entries all lie in unconnected lanes issues no descriptor or frame load at all.
//                  The buffer resource spans frames_bytes rounded up to a dword: the tailroom
//                  contract of udpdk_gpu.h, unchanged.
// Then rx_filter_base and rx_filter_write (rx_filter.hip) as for the drop filter: a stable global
// compaction keeps the lane grouping and each lane's arrival order. meta is never read.
//
// Bytes. Per entry in a connected lane: 4 (lane entry) + 6 (offset, length; gathers) + the 64-byte
// memory request that holds frame bytes 26-35 read, 4 (the kept entry) written, the keep masks
// 1/8 B; the lane's 8-byte peer record is L2-resident (32 KiB for 4096 lanes). Per entry in an
// unconnected lane: 4 + 4 + 1/8. 8 M entries, all connected: 32 MB + 48 MB + up to 512 MB of header
// requests (fewer where entries share a frame or a line) + 32 MB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_peer.h"
#include "lane_find.h"
#include "wave.h"

namespace udpdk {

__global__ void __launch_bounds__(FLT_BLOCK)
rx_peer_mark(PeerMarkArgs b)
{
    __shared__ uint32_t red[FLT_WAVES][4];
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
    // round 2: the peer records of the entries' lanes
    uint2 pr[FLT_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool valid = (c0 + s) * 64 + lane < din && e[s] < a.n;
        pr[s] = valid ? b.peer[l[s]] : make_uint2(0u, 0u);
    }
    bool need[FLT_STEPS], ok[FLT_STEPS], any = false;
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        need[s] = (pr[s].y >> 16) != 0u;                 // (an entry that is not valid has on == 0)
        ok[s] = false;
        any = any || need[s];
    }
    uint4 x[FLT_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) x[s] = make_uint4(0u, 0u, 0u, 0u);
    uint32_t sh[FLT_STEPS] = {0u, 0u, 0u, 0u};
    if (__ballot(any) != 0ull) {                         // wave-uniform: some lane is connected
        // round 3: the descriptors of the entries in connected lanes
        uint32_t o[FLT_STEPS], len[FLT_STEPS];
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            o[s] = need[s] ? b.offset[e[s]] : 0u;
            len[s] = need[s] ? (uint32_t)b.length[e[s]] : 0u;
        }
        // round 4: the header bytes; lanes with nothing to read address out of range
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            ok[s] = need[s] && len[s] >= 42u && (uint64_t)o[s] + len[s] <= (uint64_t)b.frames_bytes;
            sh[s] = (o[s] + 26u) & 3u;
            x[s] = load16(fr, ok[s] ? (o[s] + 26u) & ~3u : 0xFFFFFFF0u);
        }
    }
    uint32_t cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool in = (c0 + s) * 64 + lane < din, valid = in && e[s] < a.n;
        const uint32_t src = __builtin_amdgcn_alignbyte(x[s].y, x[s].x, sh[s]);      // bytes 26-29
        const uint32_t ports = __builtin_amdgcn_alignbyte(x[s].w, x[s].z, sh[s]);    // bytes 34-37
        const bool match = src == pr[s].x && (ports & 0xFFFFu) == (pr[s].y & 0xFFFFu);
        const unsigned long long keep = __ballot(valid && (!need[s] || (ok[s] && match)));
        if (lane == 0) a.mask[c0 + s] = keep;
        cnt[0] += (uint32_t)__popcll(keep);
        cnt[1] += (uint32_t)__popcll(__ballot(ok[s] && !match));
        cnt[2] += (uint32_t)__popcll(__ballot(need[s] && !ok[s]));
        cnt[3] += (uint32_t)__popcll(__ballot(in && !valid));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[w][k] = cnt[k];
    }
    __syncthreads();
    if (tid < 6) {
        // the row as rx_filter_base reads it: kept, four reason counts (refused, bad_frame, -, -), bad indices
        const int src = tid <= 2 ? (int)tid : tid == 5 ? 3 : -1;
        uint32_t v = 0;
        if (src >= 0) {
#pragma unroll
            for (uint32_t i = 0; i < FLT_WAVES; ++i) v += red[i][src];
        }
        a.row[tile * FLT_ROW + tid] = v;
    }
}

} // namespace udpdk
