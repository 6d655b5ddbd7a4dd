// rx_balance.hip — gfx950 RX datapath, optional last stage: of a frame's deliveries to sockets
// that set SO_REUSEPORT only one stays, chosen by the frame's flow hash (the reference clones the
// datagram to every reuse socket and says so in a TODO, udpdk_poller.c:387-403: "if dest unicast and
// SO_REUSEPORT, should load balance").
//
// For a DELIVERED frame the demux walk (the raw dst port's bindings in list order, a match when
// ip == raw dst address or ip == 0, ended by the first match without reuse: rx_scatter's loop)
// makes the frame's deliveries; G = those whose lane is flagged in lane_rp, g = |G|. With g >= 2
// and a unicast destination (not 255.255.255.255, first byte not 224-239) only member
// r = (hash x g) >> 32 of G stays (the kernel's reciprocal_scale, as reuseport_select_sock ranks);
// deliveries to unflagged lanes always stay. hash = the frame's RSS hash (rss_hash's, by the same
// table, rss_toeplitz.h) or the caller's.
//
//   rx_balance_pick  BAL_TILE frames per workgroup, one per lane and step: chosen[i] = the lane that
//                    keeps frame i's reuse-port delivery, or BAL_KEEP_ALL (not DELIVERED, fan-out
//                    < 2: from the verdict word alone, no frame byte read; g <= 1; broadcast or
//                    multicast). Otherwise the frame's offset, ONE dword-aligned 16-byte load that
//                    holds frame bytes 26-37 (funnelled by offset & 3, range-checked against
//                    frames_bytes rounded up: the tailroom contract of udpdk_gpu.h, unchanged), the
//                    hash, a walk that counts g and a walk to member r. Every lane walks its own
//                    frame's bindings, four bindings (and their lanes' flags) loaded ahead, so a
//                    wave has up to 256 binding loads in flight instead of one lane's one.
//                    META_FANOUT saturates at 127: the walk counts for itself, the verdict word
//                    only tells fan-out < 2.
//   rx_balance_mark  rx_filter_mark's geometry and outputs (a keep mask per 64-entry chunk, a row per
//                    tile): entry p of lane l with frame i = lane_pkt[p] goes when i >= n (no verdict,
//                    chosen or frame read: bad_index) or lane_rp[l] != 0 and chosen[i] is another
//                    lane. The lane of an entry: lane_find.h.
// Then rx_filter_base and rx_filter_write (rx_filter.hip) as for the drop filter: a stable global
// compaction keeps the lane grouping and each lane's arrival order.
//
// Bytes. Per frame: 4 (verdict word) + 4 (chosen, written); a balanced frame adds 4 (offset), the
// 64-byte memory request that holds its bytes 26-37, 4 with a caller's hash, and the port entry
// and bindings (16 + 8 per binding, twice; L2-resident, as the lanes' flags are); the 12 KiB key
// table goes to LDS once per workgroup that hashes. Per entry: 4 (lane entry) + 4 (chosen, a
// gather) read, 4 (the kept entry) written, the keep masks 1/8 B. 8 M entries of 1 M frames: 76 MB
// for the frames, 100 MB for the entries, 28 us at 6.3 TB/s.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_balance.h"
#include "lane_find.h"
#include "rss_toeplitz.h"
#include "wave.h"

namespace udpdk {

namespace {

// The demux walk of one frame over its port's bindings (entry e; binding 0 rides in e.z / e.w),
// counting the deliveries to flagged lanes: returns their number g, and in *lane the lane of
// member `want` (when want < g). Four bindings per round, every load of a round in flight.
__device__ __forceinline__ uint32_t balance_walk(const BalancePickArgs &a, const uint4 e, uint32_t dip,
                                                 uint32_t want, uint32_t *lane)
{
    const uint32_t nb = min(e.x, UDPDK_GPU_MAX_PORT_BINDS);
    uint32_t g = 0u;
    bool done = false;
    for (uint32_t k0 = 0u; k0 < nb && !done; k0 += 4u) {
        uint2 b[4];
        uint32_t rp[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t k = min(k0 + j, nb - 1u);
            b[j] = k == 0u ? make_uint2(e.z, e.w) : a.binds[e.y + k];
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t sock = b[j].y & 0x7FFFFFFFu;
            const bool match = k0 + j < nb && (b[j].x == dip || b[j].x == 0u);
            rp[j] = match && sock < a.n_lanes ? (uint32_t)a.lane_rp[sock] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const bool match = k0 + j < nb && (b[j].x == dip || b[j].x == 0u);
            if (done || !match) continue;
            if (rp[j]) {
                if (g == want) *lane = b[j].y & 0x7FFFFFFFu;
                ++g;
            }
            if (!(b[j].y >> 31)) done = true;
        }
    }
    return g;
}

} // namespace

__global__ void __launch_bounds__(BAL_BLOCK)
rx_balance_pick(BalancePickArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab[12][256];
    __shared__ uint32_t wcnt[BAL_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    const uint32_t t0 = blockIdx.x * BAL_TILE;
    uint32_t m[BAL_STEPS];
    bool need[BAL_STEPS], any = false;
#pragma unroll
    for (uint32_t s = 0; s < BAL_STEPS; ++s) {
        const uint32_t i = t0 + s * BAL_BLOCK + tid;
        m[s] = i < a.n ? a.meta[i] : 0xFu;
        need[s] = i < a.n && UDPDK_META_VERDICT(m[s]) == UDPDK_V_DELIVERED && UDPDK_META_FANOUT(m[s]) >= 2u;
        any = any || need[s];
    }
    // a tile without fan-out reads nothing more (and stages no table)
    if (!__syncthreads_or(any ? 1 : 0)) {
#pragma unroll
        for (uint32_t s = 0; s < BAL_STEPS; ++s) {
            const uint32_t i = t0 + s * BAL_BLOCK + tid;
            if (i < a.n) a.chosen[i] = BAL_KEEP_ALL;
        }
        return;
    }
    // offsets, then the header words and the caller's hashes: each round all in flight
    uint32_t o[BAL_STEPS], hin[BAL_STEPS];
    uint4 x[BAL_STEPS];
#pragma unroll
    for (uint32_t s = 0; s < BAL_STEPS; ++s) {
        const uint32_t i = t0 + s * BAL_BLOCK + tid;
        o[s] = need[s] ? a.offset[i] : 0u;
    }
    const bool hashing = !a.hash_in && a.hash_types != 0u;         // kernel-uniform
    constexpr uint32_t KV = 12u * 256u / 4u / BAL_BLOCK;
    uint4 kv[KV];
    if (hashing) {
        const uint4 *ksrc = reinterpret_cast<const uint4 *>(a.ktab);
#pragma unroll
        for (uint32_t q = 0; q < KV; ++q) kv[q] = ksrc[q * BAL_BLOCK + tid];
    }
#pragma unroll
    for (uint32_t s = 0; s < BAL_STEPS; ++s) {
        const uint32_t i = t0 + s * BAL_BLOCK + tid;
        // lanes with nothing to read address out of range (no memory access)
        const bool rd = need[s] && o[s] <= 0xFFFFFFFFu - 64u;
        x[s] = load16(fr, rd ? (o[s] + 26u) & ~3u : 0xFFFFFFF0u);
        hin[s] = need[s] && a.hash_in ? a.hash_in[i] : 0u;
    }
    if (hashing) {
        uint4 *dst = reinterpret_cast<uint4 *>(&tab[0][0]);
#pragma unroll
        for (uint32_t q = 0; q < KV; ++q) dst[q * BAL_BLOCK + tid] = kv[q];
        __syncthreads();
    }
    uint32_t nbal = 0u;
#pragma unroll
    for (uint32_t s = 0; s < BAL_STEPS; ++s) {
        const uint32_t i = t0 + s * BAL_BLOCK + tid;
        uint32_t pick = BAL_KEEP_ALL;
        if (need[s]) {
            const uint32_t sh = (o[s] + 26u) & 3u;
            const uint32_t src = __builtin_amdgcn_alignbyte(x[s].y, x[s].x, sh);      // bytes 26-29
            const uint32_t dip = __builtin_amdgcn_alignbyte(x[s].z, x[s].y, sh);      // bytes 30-33
            const uint32_t ports = __builtin_amdgcn_alignbyte(x[s].w, x[s].z, sh);    // bytes 34-37
            const uint32_t b0 = dip & 0xFFu;
            const bool all = dip == 0xFFFFFFFFu || (b0 >= 224u && b0 <= 239u);
            if (!all) {
                const uint4 e = a.port_tab[ports >> 16];
                uint32_t unused = 0u;
                const uint32_t g = balance_walk(a, e, dip, BAL_KEEP_ALL, &unused);
                if (g >= 2u) {
                    uint32_t hash = hin[s];
                    if (hashing) hash = rss_toeplitz(tab, src, dip, ports, (a.hash_types & 2u) != 0u);
                    const uint32_t r = __umulhi(hash, g);
                    balance_walk(a, e, dip, r, &pick);
                    ++nbal;
                }
            }
        }
        if (i < a.n) a.chosen[i] = pick;
    }
    const uint32_t ws = wave_sum(nbal);
    if (lane == 0) wcnt[w] = ws;
    __syncthreads();
    if (tid == 0) {
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t j = 0; j < BAL_BLOCK / 64; ++j) v += wcnt[j];
        if (v) atomicAdd(a.balanced, v);
    }
}

__global__ void __launch_bounds__(FLT_BLOCK)
rx_balance_mark(BalanceMarkArgs b)
{
    __shared__ uint32_t red[FLT_WAVES][3];
    const FilterArgs &a = b.f;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, tile = blockIdx.x;
    const uint32_t din = min(a.lane_off[a.n_lanes], a.lane_cap);
    if (tile * FLT_TILE >= din) return;
    const uint32_t c0 = tile * FLT_CHUNKS + w * FLT_STEPS;
    uint32_t e[FLT_STEPS], ch[FLT_STEPS];
    // the wave's entries, then their frames' choices: two rounds of loads, each all in flight
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) e[s] = a.lane_pkt[min((c0 + s) * 64 + lane, din - 1u)];
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const bool valid = (c0 + s) * 64 + lane < din && e[s] < a.n;
        ch[s] = valid ? b.chosen[e[s]] : BAL_KEEP_ALL;
    }
    // the lanes: the wave's first and last entries bound them
    uint32_t l0 = 0u, l1 = 0u;
    const uint32_t pw = (uint32_t)__builtin_amdgcn_readfirstlane((int)(c0 * 64u));
    if (pw < din) {                                                  // wave-uniform
        const uint32_t pl = min(pw + 64u * FLT_STEPS - 1u, din - 1u);
        l0 = lane_find(a.lane_off, din, pw, 0u, a.n_lanes - 1u);
        l1 = lane_find(a.lane_off, din, pl, l0, a.n_lanes - 1u);
    }
    uint32_t cnt[3] = {0, 0, 0};
#pragma unroll
    for (uint32_t s = 0; s < FLT_STEPS; ++s) {
        const uint32_t p = (c0 + s) * 64 + lane;
        const bool in = p < din, valid = in && e[s] < a.n;
        uint32_t l = l0;
        if (l1 != l0 && in) l = lane_find(a.lane_off, din, p, l0, l1);
        const bool rp = valid && ch[s] != BAL_KEEP_ALL && ch[s] != l && b.lane_rp[l] != 0;
        const unsigned long long keep = __ballot(valid && !rp);
        if (lane == 0) a.mask[c0 + s] = keep;
        cnt[0] += (uint32_t)__popcll(keep);
        cnt[1] += (uint32_t)__popcll(__ballot(rp));
        cnt[2] += (uint32_t)__popcll(__ballot(in && !valid));
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) red[w][k] = cnt[k];
    }
    __syncthreads();
    if (tid < 6) {
        // the row as rx_filter_base reads it: kept, four reason counts (the first: removed here), bad indices
        const int src = tid == 0 ? 0 : tid == 1 ? 1 : tid == 5 ? 2 : -1;
        uint32_t v = 0;
        if (src >= 0) {
#pragma unroll
            for (uint32_t i = 0; i < FLT_WAVES; ++i) v += red[i][src];
        }
        a.row[tile * FLT_ROW + tid] = v;
    }
}

} // namespace udpdk
