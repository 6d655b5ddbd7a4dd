// rx_filter.hip — gfx950 RX datapath, optional last stage: a finished lane set (lane_off,
// lane_pkt) loses every entry whose verdict word matches a drop mask (failed IPv4 or UDP checksum,
// bad UDP length, IHL != 5: the bits rx_classify sets and nothing else reads).
//
// A lane set is ONE array grouped by lane, so a global stable compaction of lane_pkt keeps the
// grouping and each lane's arrival order, and the new offsets are the kept-prefix evaluated at
// the old offsets: no per-lane histogram or scatter, and the work does not depend on the lane
// count or on how the entries spread over the lanes.
//
//   rx_filter_mark   tile of FLT_TILE entries per workgroup: each wave ballots keep for 64 entries
//                    at a time (the verdict word gathered through lane_pkt) into a mask word, and
//                    the tile's row gets the kept count and the drops per reason
//   rx_filter_base   one workgroup: exclusive prefix of the tiles' kept counts, the totals
//   rx_filter_write  tile workgroups place the kept entries at base + popc(mask & lanes below);
//                    further workgroups turn the old lane offsets into the new ones (the tile's
//                    base + the masks before the offset's chunk + the chunk's mask below it)
//   rx_filter_copy   (sticky mode) the filtered set back into the caller's buffers
//
// The entry count D = min(lane_off[n_lanes], lane_cap) is only known on the device: the grids
// cover lane_cap and the tiles past D return at once. Whatever the inputs hold, loads stay within
// meta[n], lane_off[n_lanes + 1], lane_pkt[D] and stores within the outputs: an offset past D
// counts as D, an entry >= n is removed without a verdict load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_filter.h"
#include "wave.h"

namespace udpdk {

__device__ __forceinline__ uint32_t filter_entries(const FilterArgs &a)
{
    return min(a.lane_off[a.n_lanes], a.lane_cap);
}

__global__ void __launch_bounds__(FLT_BLOCK)
rx_filter_mark(FilterArgs a)
{
    __shared__ uint32_t red[FLT_WAVES][FLT_ROW];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, tile = blockIdx.x;
    const uint32_t din = filter_entries(a);
    if (tile * FLT_TILE >= din) return;
    const uint32_t c0 = tile * FLT_CHUNKS + w * FLT_STEPS;
    uint32_t e[FLT_STEPS], m[FLT_STEPS];
    // the wave's entries, then their verdict words: two rounds of loads, each all in flight
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) e[s] = a.lane_pkt[min((c0 + s) * 64 + lane, din - 1u)];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool valid = (c0 + s) * 64 + lane < din && e[s] < a.n;
        m[s] = valid ? a.meta[e[s]] : 0u;
    }
    uint32_t cnt[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool in = (c0 + s) * 64 + lane < din, valid = in && e[s] < a.n;
        const bool r_ip = (a.flags & UDPDK_RX_DROP_IP_CKSUM) && UDPDK_META_IP_OK(m[s]) == 0;
        const bool r_udp = (a.flags & UDPDK_RX_DROP_UDP_CKSUM) && UDPDK_META_UDP_CSUM(m[s]) == UDPDK_UDP_CSUM_BAD;
        const bool r_len = (a.flags & UDPDK_RX_DROP_UDP_LEN) && UDPDK_META_LEN_BAD(m[s]);
        const bool r_ihl = (a.flags & UDPDK_RX_DROP_IHL) && UDPDK_META_IHL_NE5(m[s]);
        const unsigned long long keep = __ballot(valid && !(r_ip || r_udp || r_len || r_ihl));
        if (lane == 0) a.mask[c0 + s] = keep;
        cnt[0] += (uint32_t)__popcll(keep);
        cnt[1] += (uint32_t)__popcll(__ballot(valid && r_ip));
        cnt[2] += (uint32_t)__popcll(__ballot(valid && r_udp));
        cnt[3] += (uint32_t)__popcll(__ballot(valid && r_len));
        cnt[4] += (uint32_t)__popcll(__ballot(valid && r_ihl));
        cnt[5] += (uint32_t)__popcll(__ballot(in && !valid));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[w][k] = cnt[k];
    }
    __syncthreads();
    if (tid < 6) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t i = 0; i < FLT_WAVES; ++i) v += red[i][tid];
        a.row[tile * FLT_ROW + tid] = v;
    }
}

// Exclusive prefix of the kept counts over the tiles that hold entries (a contiguous block of
// tiles per thread + a block scan, rx_tile_base's shape: any tile count), and the totals.
__global__ void __launch_bounds__(FLT_BASE_BLOCK)
rx_filter_base(FilterArgs a)
{
    constexpr uint32_t NW = FLT_BASE_BLOCK / 64;
    __shared__ uint32_t wsum[NW][6];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t full = a.lane_off[a.n_lanes], din = min(full, a.lane_cap);
    const uint32_t nt = din / FLT_TILE + (din % FLT_TILE ? 1u : 0u);        // <= a.n_tiles
    const uint32_t per = (nt + FLT_BASE_BLOCK - 1u) / FLT_BASE_BLOCK;
    const uint32_t b0 = min(nt, tid * per), b1 = min(nt, b0 + per);
    uint32_t s[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t t = b0; t < b1; ++t) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += a.row[t * FLT_ROW + k];
    }
    const uint32_t incl = wave_incl_scan(s[0]);
    uint32_t tot[6];
    tot[0] = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
#pragma unroll
    for (int k = 1; k < 6; ++k) tot[k] = wave_sum(s[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) wsum[w][k] = tot[k];
    }
    __syncthreads();
    uint32_t before = incl - s[0];
    for (uint32_t i = 0; i < w; ++i) before += wsum[i][0];
    for (uint32_t t = b0; t < b1; ++t) {
        a.base[t] = before;
        before += a.row[t * FLT_ROW];
    }
    if (tid == 0) {
        uint32_t g[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            g[k] = 0;
            for (uint32_t i = 0; i < NW; ++i) g[k] += wsum[i][k];
        }
        FilterResult r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.dropped[k] = g[1 + k];
        r.kept = g[0];
        r.removed = din - g[0];
        r.bad_index = g[5];
        r.truncated = full > a.lane_cap ? 1u : 0u;
        *a.res = r;
    }
}

__global__ void __launch_bounds__(FLT_BLOCK)
rx_filter_write(FilterArgs a)
{
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t din = filter_entries(a);
    if (blockIdx.x < a.n_tiles) {
        const uint32_t tile = blockIdx.x;
        if (tile * FLT_TILE >= din) return;
        const uint32_t c0 = tile * FLT_CHUNKS + w * FLT_STEPS;
        uint32_t run = a.base[tile];
        for (uint32_t c = tile * FLT_CHUNKS; c < c0; ++c) run += (uint32_t)__popcll(a.mask[c]);
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (uint32_t s = 0; s < FLT_STEPS; ++s) {
            const unsigned long long m = a.mask[c0 + s];
            if ((m >> lane) & 1ull) {                       // a set bit is an entry below din
                const uint32_t pos = run + (uint32_t)__popcll(m & lt);
                if (pos < a.out_cap) a.lane_pkt_out[pos] = a.lane_pkt[(c0 + s) * 64 + lane];
            }
            run += (uint32_t)__popcll(m);
        }
        return;
    }
    // the lane offsets: kept entries before the old offset
    const uint32_t j = (blockIdx.x - a.n_tiles) * FLT_BLOCK + tid;
    if (j > a.n_lanes) return;
    const uint32_t o = min(a.lane_off[j], din);
    uint32_t v;
    if (o >= din) {
        v = a.res->kept;
    } else {
        const uint32_t c = o >> 6, tile = c / FLT_CHUNKS;   // a tile that holds entries
        v = a.base[tile];
        for (uint32_t i = tile * FLT_CHUNKS; i < c; ++i) v += (uint32_t)__popcll(a.mask[i]);
        v += (uint32_t)__popcll(a.mask[c] & ((1ull << (o & 63u)) - 1ull));
    }
    a.lane_off_out[j] = v;
}

// The filtered set back into the buffers it was taken from: entries [0, min(kept, cap)) and the
// offsets (the grid of rx_filter_write).
__global__ void __launch_bounds__(FLT_BLOCK)
rx_filter_copy(const uint32_t *off, const uint32_t *pkt, const FilterResult *res, uint32_t *off_out,
               uint32_t *pkt_out, uint32_t n_lanes, uint32_t cap, uint32_t n_tiles)
{
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < n_tiles) {
        const uint32_t k = min(res->kept, cap), p0 = blockIdx.x * FLT_TILE + tid;
#pragma unroll
        for (uint32_t i = 0; i < FLT_TILE / FLT_BLOCK; ++i) {
            const uint32_t p = p0 + i * FLT_BLOCK;
            if (p < k) pkt_out[p] = pkt[p];
        }
        return;
    }
    const uint32_t j = (blockIdx.x - n_tiles) * FLT_BLOCK + tid;
    if (j <= n_lanes) off_out[j] = off[j];
}

} // namespace udpdk
