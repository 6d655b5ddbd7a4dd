// rx_lanes.hip — gfx950 RX datapath, second stage: rx_classify's verdict words and per-tile
// delivery histogram (rx_classify.hip) become the per-socket lanes, lane_pkt = each lane's
// delivered frames in arrival order. Two completions:
//
//   single lane   rx_compact1, a second launch where rx_classify's fused form is not taken: keeps
//       the speculative entries up to the first tile that was not full, rewrites the rest
//       (rx_tile_base: the tiles' bases when a batch has many tiles).
//   several lanes rx_scan_cols + rx_scatterw: per-lane column scan of the tile-major histogram
//       (decoupled look-back over lane blocks, base rows out), then a stable per-lane scatter
//       (LDS atomic ranks, key-ordered staging, linear stores). rx_scan_reduce/top/down and
//       rx_scatter: the same past their limits (more tiles, more lanes, fan-out).
//
//   rx_counters  on demand (udpdk_gpu_rx_stats): sum of the per-tile counter rows.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "wave.h"
#include "stamps.h"

namespace udpdk {

// counters[c] = sum over tiles of tile_cnt[t][c] (64-bit). Thread (g, c) = (tid / 16, tid % 16)
// sums counter c of rows g, g + G, ... (each pass of the block reads 16 whole rows, coalesced);
// two xor-shuffles fold the 4 row groups of a wave, LDS the waves. lds: >= 16 * waves u64.
__device__ unsigned long long reduce_counters(const uint32_t *tile_cnt, uint32_t n_tiles,
                                              unsigned long long *counters, unsigned long long *lds)
{
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, nw = blockDim.x >> 6;
    const uint32_t c = tid & 15u, G = blockDim.x >> 4;
    unsigned long long s = 0;
    uint32_t t = tid >> 4;
    auto ld = [&](uint32_t row) -> uint32_t {
        const uint32_t *p = &tile_cnt[(size_t)row * UDPDK_N_COUNTERS + c];
        return *p;
    };
    for (; t + 3u * G < n_tiles; t += 4u * G) {
        const uint32_t v0 = ld(t), v1 = ld(t + G), v2 = ld(t + 2u * G), v3 = ld(t + 3u * G);
        s += (unsigned long long)v0 + v1 + v2 + v3;
    }
    for (; t < n_tiles; t += G) s += ld(t);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (lane < 16) lds[w * 16 + lane] = s;
    __syncthreads();
    unsigned long long r = 0;
    if (tid < UDPDK_N_COUNTERS) {
        for (uint32_t i = 0; i < nw; ++i) r += lds[i * 16 + tid];
        counters[tid] = r;
    }
    return r;                                               // counter tid, for tid < 16
}

// ------------------------------------------------------------------------------------------
// rx_compact1: the single-lane batch's lane (no fan-out: every delivery is a whole frame).
// Workgroup = tile (grid-stride over the tiles after the first flagged one when rx_classify
// wrote speculative entries). Each wave ballots its quarter of the tile's verdict words (delivered =
// verdict 0) into LDS masks, the tile's base is the sum of the predecessors' delivery counts
// (<= n_tiles words, read straight from the classify kernel's per-tile histogram: no scan
// kernel and no cross-workgroup waits), then every delivered frame writes its index.
// The last tile's workgroup writes lane_off[1] = total.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void compact1_tile(const Compact1Args &a, uint32_t tile, uint32_t steps,
                                              uint32_t tid, uint32_t lane, uint32_t w)
{
    constexpr uint32_t MAXS = RX_TILE_MAX / RX_BLOCK;      // steps per wave, <= 64
    __shared__ unsigned long long msk[RX_WAVES][MAXS];
    __shared__ uint32_t red[2 * RX_WAVES];
    const uint32_t t1 = min(a.n, (tile + 1) * a.tile_frames);
    const uint32_t wb = tile * a.tile_frames + w * steps * 64;
    const uint32_t plast = a.n - 1u;
    // predecessors' counts first (the first two per thread unconditionally, clamped), so they
    // are in flight together with the verdict words: one memory round trip for both
    const uint32_t tl = a.n_tiles - 1u;
    const uint32_t c0 = a.tile_count[min(tid, tl)], c1 = a.tile_count[min(tid + RX_BLOCK, tl)];
    uint32_t wcount = 0;
    for (uint32_t s0 = 0; s0 < steps; s0 += 4) {
        uint32_t mv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) mv[u] = a.meta[min(wb + (s0 + u) * 64 + lane, plast)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (s0 + u >= steps) break;                     // fewer than 4 steps per wave
            const uint32_t p = wb + (s0 + u) * 64 + lane;
            const unsigned long long m = __ballot(p < t1 && (mv[u] & 0xFu) == UDPDK_V_DELIVERED);
            if (lane == 0) msk[w][s0 + u] = m;
            wcount += (uint32_t)__popcll(m);
        }
    }
    uint32_t pre = 0;
    if (!a.base) {
        pre = (tid < tile ? c0 : 0u) + (tid + RX_BLOCK < tile ? c1 : 0u);
        for (uint32_t t = tid + 2 * RX_BLOCK; t < tile; t += RX_BLOCK) pre += a.tile_count[t];
        pre = wave_sum(pre);
    }
    if (lane == 0) { red[w] = pre; red[RX_WAVES + w] = wcount; }
    __syncthreads();
    // many tiles: the base comes from rx_tile_base (the all-predecessor sum grows with tiles^2)
    uint32_t base = a.base ? a.base[tile] : 0u, tcount = 0, before = 0;
#pragma unroll
    for (int i = 0; i < RX_WAVES; ++i) {
        base += red[i];
        tcount += red[RX_WAVES + i];
        before += (uint32_t)i < w ? red[RX_WAVES + i] : 0u;
    }
    uint32_t run = base + before;
    const uint32_t total = base + tcount;
    if (tile == a.n_tiles - 1u && tid == 0) {
        a.lane_off[0] = 0u;
        a.lane_off[1] = total;
        *a.total = total;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (uint32_t s = 0; s < steps; ++s) {
        const unsigned long long m = msk[w][s];
        if ((m >> lane) & 1ull) {
            const uint32_t pos = run + (uint32_t)__popcll(m & lt);
            if (pos < a.lane_cap) a.lane_pkt[pos] = wb + s * 64 + lane;
        }
        run += (uint32_t)__popcll(m);
    }
}

__global__ void __launch_bounds__(RX_BLOCK)
rx_compact1(Compact1Args a)
{
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t steps = a.tile_frames / RX_BLOCK;
    const uint32_t tl = a.n_tiles - 1u;
    // speculative entries: rx_classify placed every tile's entries at tile x tile_frames + rank,
    // right when every earlier tile delivered all its frames, i.e. up to and including the call's
    // first flagged tile. Every wave reads the 64 flag words (one load per lane) and takes the
    // smallest flagged tile; only the tiles after it are rewritten (grid-stride: the launch is
    // small, so the common all-full call costs one flag read and the total's store).
    uint32_t t_first = blockIdx.x;
    if (a.spec) {
        const unsigned long long nf = __hip_atomic_load(&a.spec_nonfull[lane % UDPDK_SPEC_WORDS], __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
        uint32_t first = (uint32_t)(nf >> 32) == a.spec_epoch ? 0xFFFFFFFFu - (uint32_t)nf : 0xFFFFFFFFu;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) first = min(first, (uint32_t)__shfl_xor((int)first, d, 64));
        if (first < tl && blockIdx.x == 0 && tid == 0 && a.hint)
            __hip_atomic_store(&a.hint[UDPDK_HINT_NONFULL], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (first >= tl) {
            if (blockIdx.x == 0 && tid == 0) {
                const uint32_t total = tl * a.tile_frames + a.tile_count[tl];
                a.lane_off[0] = 0u;
                a.lane_off[1] = total;
                *a.total = total;
            }
            return;
        }
        t_first = first + 1u + blockIdx.x;
    }
    for (uint32_t tile = t_first; tile < a.n_tiles; tile += gridDim.x) {
        compact1_tile(a, tile, steps, tid, lane, w);
        __syncthreads();                       // msk / red reused by the next tile
    }
}

// ------------------------------------------------------------------------------------------
// rx_tile_base: exclusive prefix of the per-tile delivery counts for rx_compact1 when a batch
// has many tiles (one workgroup: a contiguous block of tiles per thread + a block scan).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
rx_tile_base(const uint32_t *cnt, uint32_t *base, uint32_t n)
{
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t per = (n + 1023u) / 1024u, b0 = min(n, tid * per), b1 = min(n, b0 + per);
    uint32_t s = 0;
    for (uint32_t i = b0; i < b1; ++i) s += cnt[i];
    const uint32_t incl = wave_incl_scan(s);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t before = incl - s;
    for (uint32_t i = 0; i < w; ++i) before += wsum[i];
    for (uint32_t i = b0; i < b1; ++i) {
        base[i] = before;
        before += cnt[i];
    }
}

// ------------------------------------------------------------------------------------------
// rx_counters: counters[c] = sum over the last call's tiles of tile_cnt[t][c] (one workgroup,
// launched by udpdk_gpu_rx_stats only, so a batch that nobody asks statistics for pays nothing)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rx_counters(const uint32_t *tile_cnt, uint32_t n_tiles, unsigned long long *counters)
{
    __shared__ unsigned long long lcnt[16 * 4];
    reduce_counters(tile_cnt, n_tiles, counters, lcnt);
}

// ------------------------------------------------------------------------------------------
// rx_scan: the tile-major histogram hist[tile][lane] becomes each (tile, lane)'s start position
// in the lane array: pos(t, l) = lane_off[l] + sum_{t' < t} hist[t'][l], with lane_off the
// exclusive scan of the lane totals. Every access is row-contiguous (threads = lanes).
//   cols (one launch):   tiles <= SCAN_COLS_MAX_TILES, rx_scan_cols below
//   reduce / top / down: per-chunk column sums (chunks of SCAN_COL_CHUNK tiles), one workgroup
//                        scanning chunks and lanes, then the in-place rescan of every chunk.
// ------------------------------------------------------------------------------------------
// exclusive scan over a block of any wave count; lds16 >= waves words
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *lds16, uint32_t *total)
{
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == 63) lds16[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t t = lds16[i];
        if (i < w) pre += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

// Lane totals tot[] (LDS, n_lanes words) -> lane_off[] exclusive scan + total. Thread j takes the
// contiguous lanes [j * L, (j + 1) * L).
__device__ __forceinline__ void scan_lane_totals(const uint32_t *tot, uint32_t n_lanes, uint32_t *lane_off,
                                 uint32_t *total_out, uint32_t *lds16)
{
    const uint32_t tid = threadIdx.x, L = (n_lanes + blockDim.x - 1) / blockDim.x;
    const uint32_t l0 = min(n_lanes, tid * L), l1 = min(n_lanes, l0 + L);
    // the thread's lanes in registers, loaded at once with clamped indices (a loop with a
    // data-dependent trip count waited for every load in turn); LR = 4, 8 or 16 lanes per thread
    // covers UDPDK_GPU_MAX_LANES at 1024 threads
    auto regs = [&](auto lr) {
        constexpr uint32_t LR = decltype(lr)::value;
        uint32_t v[LR], s = 0;
#pragma unroll
        for (uint32_t i = 0; i < LR; ++i) {
            const uint32_t x = tot[min(l0 + i, n_lanes - 1u)];
            v[i] = l0 + i < l1 ? x : 0u;
            s += v[i];
        }
        uint32_t total;
        uint32_t run = block_excl_scan(s, lds16, &total);
#pragma unroll
        for (uint32_t i = 0; i < LR; ++i) {
            if (l0 + i < l1) lane_off[l0 + i] = run;
            run += v[i];
        }
        if (tid == 0) { lane_off[n_lanes] = total; *total_out = total; }
    };
    if (L <= 4u) return regs(std::integral_constant<uint32_t, 4>{});
    if (L <= 8u) return regs(std::integral_constant<uint32_t, 8>{});
    if (L <= 16u) return regs(std::integral_constant<uint32_t, 16>{});
    uint32_t s = 0;
    for (uint32_t l = l0; l < l1; ++l) s += tot[l];
    uint32_t total;
    uint32_t run = block_excl_scan(s, lds16, &total);
    for (uint32_t l = l0; l < l1; ++l) {
        lane_off[l] = run;
        run += tot[l];
    }
    if (tid == 0) { lane_off[n_lanes] = total; *total_out = total; }
}

// rx_scan_cols: the whole scan in one launch. Workgroup = a block of LB = 2^lb lanes x every
// tile; thread (c, l) holds lane l's counts of the c-th of B / LB contiguous tile chunks
// (<= scan_cols_tpt(B) tiles) in registers, all loaded at once (LB lanes x 2 or 4 B contiguous per
// tile row). The chunk sums meet in LDS and give the lane totals; the lane offsets (the exclusive
// scan of the totals over ALL lanes, which other workgroups hold) come from a decoupled look-back
// over the lane blocks: blocks take tickets in dispatch order, publish their total (A) at once
// and their inclusive prefix (P) once they know it, and a block sums its predecessors' words back
// to the nearest P, one 64-word window per wave load. Each thread then writes its tiles' absolute
// positions base[t][l] = lane_off[l] + sum over t' < t of hist[t'][l], so the scatter reads one
// row per tile and no launch runs between this one and it (the former rx_lane_off).
// Look-back words: epoch << 32 | flag << 30 | value, flag 1 = A, 2 = P; a word from an earlier
// call (older epoch) is not ready. Value < 2^30: deliveries <= max_frames x fan-out.
__device__ __forceinline__ unsigned long long lb_poll(unsigned long long *p, uint32_t epoch)
{
    unsigned long long v;
    for (;;) {
        v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(v >> 32) == epoch && ((v >> 30) & 3u)) return v;
        __builtin_amdgcn_s_sleep(1);
    }
}

template <uint32_t B>
__global__ void __launch_bounds__(B)
rx_scan_cols(ScanArgs a, uint32_t lb)
{
    constexpr uint32_t TPT = scan_cols_tpt(B);
#ifdef UDPDK_STAMPS
    // diagnostic: memtime at start, loads summed, look-back done, stores issued; memrealtime at
    // start and end (rows RX_TILE_MAX * 3 + ticket of a.dbg)
    unsigned long long sst[6];
    sst[0] = __builtin_amdgcn_s_memtime();
    sst[4] = __builtin_amdgcn_s_memrealtime();
#endif
    __shared__ uint32_t part[B];
    __shared__ uint32_t loff_sh[64];
    __shared__ uint32_t jb;
    const uint32_t LB = 1u << lb, C = B >> lb;
    const uint32_t l = threadIdx.x & (LB - 1u), c = threadIdx.x >> lb;
    if (threadIdx.x == 0) {
        const uint32_t j = atomicAdd(a.ticket, 1u);
        if (j == gridDim.x - 1u) atomicExch(a.ticket, 0u); // every ticket taken: reset for the next call
        jb = j;
    }
    __syncthreads();
    const uint32_t j = jb;
    const uint32_t S = a.n_lanes, lanei = j * LB + l;
    const uint32_t tpc = (a.n_tiles + C - 1u) / C;
    const uint32_t t0 = min(a.n_tiles, c * tpc), t1 = min(a.n_tiles, t0 + tpc);
    const bool ok = lanei < S;
    const uint32_t hs = a.hist16 ? ((S + 1u) & ~1u) : S;   // row stride in counts
    const uint16_t *col16 = reinterpret_cast<const uint16_t *>(a.hist) + lanei;
    const uint32_t *col32 = a.hist + lanei;
    uint32_t v[TPT];
#pragma unroll
    for (uint32_t k = 0; k < TPT; ++k) {
        const bool in = ok && t0 + k < t1;
        const size_t o = (size_t)(in ? t0 + k : 0u) * hs;
        v[k] = !in ? 0u : a.hist16 ? (uint32_t)col16[o] : col32[o];
    }
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < TPT; ++k) sum += v[k];
    part[c * LB + l] = sum;
    __syncthreads();
#ifdef UDPDK_STAMPS
    sst[1] = __builtin_amdgcn_s_memtime();
#endif
    uint32_t run = 0, tot = 0;
    for (uint32_t i = 0; i < C; ++i) {
        const uint32_t x = part[i * LB + l];
        run += i < c ? x : 0u;
        tot += x;
    }
    if (threadIdx.x < 64) {                                  // wave 0: threads (0, l), l < LB <= 64
        const uint32_t lane = lane_id();
        const uint32_t mine = lane < LB && ok ? tot : 0u;
        const uint32_t incl = wave_incl_scan(mine);
        const uint32_t btot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const unsigned long long tag = (unsigned long long)a.epoch << 32;
        if (lane == 0)
            __hip_atomic_store(&a.agg[j], tag | (1ull << 30) | btot,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // look-back: the predecessors' words, 64 at a time, down to the nearest inclusive one
        uint32_t pre = 0;
        for (uint32_t k = j; k > 0;) {
            const uint32_t idx = k - 1u - lane;                 // lane 0 = nearest predecessor
            const bool in = lane < k;
            const unsigned long long wv = in ? lb_poll(&a.agg[idx], a.epoch) : (tag | (2ull << 30));
            const unsigned long long pm = __ballot(((wv >> 30) & 3u) == 2u);
            const uint32_t stop = pm ? (uint32_t)__ffsll((long long)pm) - 1u : 64u;
            const uint32_t val = in && lane <= stop ? (uint32_t)(wv & 0x3FFFFFFFu) : 0u;
            pre += wave_sum(val);
            if (pm) break;
            k = k > 64u ? k - 64u : 0u;
        }
        if (lane == 0)
            __hip_atomic_store(&a.agg[j], tag | (2ull << 30) | (pre + btot),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < LB) {
            const uint32_t lo = pre + incl - mine;
            loff_sh[lane] = lo;
            if (ok) a.lane_off[lanei] = lo;
        }
        if (lane == 0 && (j + 1u) * LB >= S) {             // the last block: the grand total
            a.lane_off[S] = pre + btot;
            *a.total = pre + btot;
        }
    }
    __syncthreads();
#ifdef UDPDK_STAMPS
    sst[2] = __builtin_amdgcn_s_memtime();
#endif
    run += loff_sh[l];
    uint32_t *out = a.base + lanei;
#pragma unroll
    for (uint32_t k = 0; k < TPT; ++k) {
        if (ok && t0 + k < t1 && ((t0 + k) & a.row_mask) == 0u) out[(size_t)(t0 + k) * S] = run;
        run += v[k];
    }
#ifdef UDPDK_STAMPS
    sst[3] = __builtin_amdgcn_s_memtime();
    sst[5] = __builtin_amdgcn_s_memrealtime();
    if (a.dbg && threadIdx.x == 0 && j < RX_TILE_MAX) {
        unsigned long long *d = a.dbg + (size_t)(RX_TILE_MAX * 3 + j) * 16;
        d[0] = sst[1] - sst[0];
        d[1] = sst[2] - sst[1];
        d[2] = sst[3] - sst[2];
        d[3] = sst[4];
        d[4] = sst[5];
        d[5] = j;
    }
#endif
}

template __global__ void rx_scan_cols<512>(ScanArgs a, uint32_t lb);
template __global__ void rx_scan_cols<1024>(ScanArgs a, uint32_t lb);

// Pass 1, grid (chunks, ceil(lanes / SCAN_BLOCK)): partial[c][l] = column sum of chunk c.
__global__ void __launch_bounds__(SCAN_BLOCK)
rx_scan_reduce(ScanArgs a)
{
    const uint32_t S = a.n_lanes, l = blockIdx.y * SCAN_BLOCK + threadIdx.x;
    if (l >= S) return;
    const uint32_t t0 = blockIdx.x * SCAN_COL_CHUNK, t1 = min(a.n_tiles, t0 + SCAN_COL_CHUNK);
    uint32_t v[SCAN_COL_CHUNK];                            // all loads in flight at once
#pragma unroll
    for (uint32_t k = 0; k < SCAN_COL_CHUNK; ++k)
        v[k] = t0 + k < t1 ? a.hist[(size_t)(t0 + k) * S + l] : 0u;
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_COL_CHUNK; ++k) s += v[k];
    a.partial[(size_t)blockIdx.x * S + l] = s;
}

// Pass 2, one workgroup: per lane, exclusive scan of its chunk sums (in place) and its total;
// then lane_off = exclusive scan of the totals.
__global__ void __launch_bounds__(SCAN_TOP_BLOCK)
rx_scan_top(ScanArgs a, uint32_t n_chunks)
{
    extern __shared__ uint32_t tot[];                       // [n_lanes]
    __shared__ uint32_t lds16[SCAN_TOP_BLOCK / 64];
    const uint32_t S = a.n_lanes;
    for (uint32_t l = threadIdx.x; l < S; l += SCAN_TOP_BLOCK) {
        uint32_t run = 0;
        for (uint32_t c0 = 0; c0 < n_chunks; c0 += 32) {   // 32 loads in flight per batch
            uint32_t v[32];
#pragma unroll
            for (uint32_t k = 0; k < 32; ++k)
                v[k] = c0 + k < n_chunks ? a.partial[(size_t)(c0 + k) * S + l] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < 32; ++k) {
                if (c0 + k < n_chunks) a.partial[(size_t)(c0 + k) * S + l] = run;
                run += v[k];
            }
        }
        tot[l] = run;
    }
    __syncthreads();
    scan_lane_totals(tot, S, a.lane_off, a.total, lds16);
}

// Pass 3, grid (chunks, ceil(lanes / SCAN_BLOCK)): rescan chunk c from lane_off + its prefix.
__global__ void __launch_bounds__(SCAN_BLOCK)
rx_scan_down(ScanArgs a)
{
    const uint32_t S = a.n_lanes, l = blockIdx.y * SCAN_BLOCK + threadIdx.x;
    if (l >= S) return;
    const uint32_t t0 = blockIdx.x * SCAN_COL_CHUNK, t1 = min(a.n_tiles, t0 + SCAN_COL_CHUNK);
    uint32_t v[SCAN_COL_CHUNK];
#pragma unroll
    for (uint32_t k = 0; k < SCAN_COL_CHUNK; ++k)
        v[k] = t0 + k < t1 ? a.hist[(size_t)(t0 + k) * S + l] : 0u;
    uint32_t run = a.lane_off[l] + a.partial[(size_t)blockIdx.x * S + l];
#pragma unroll
    for (uint32_t k = 0; k < SCAN_COL_CHUNK; ++k) {
        if (t0 + k < t1) a.hist[(size_t)(t0 + k) * S + l] = run;
        run += v[k];
    }
}

// Tile of workgroup b out of n so that each XCD walks a contiguous run of tiles (blocks are dealt
// round-robin over the 8 XCDs, MI355X_MICROARCH.md §Workgroup dispatch; b % 8 labels the blocks
// sharing one). Bijective for any n. A lane's entries from consecutive tiles are adjacent in
// lane_pkt, so with this order the partial lines one tile leaves in a lane are completed by the
// next tiles in the SAME L2 and written back once, instead of once per XCD that touched them.
// Placement is a speed choice only: any order gives the same output.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, uint32_t n)
{
    const uint32_t x = b & 7u, q = n >> 3, r = n & 7u;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (b >> 3);
}

// Scatter prologue: cur[k] = base[tile][k], the absolute start of the tile's deliveries in lane k
// (rx_scan_cols / rx_scan_down fold lane_off in), for the S lanes, CU loads per thread in flight at
// once (clamped indices, stores guarded): a plain strided loop waited for each iteration's loads,
// one L2 / HBM round trip per NT lanes (8 at 4096 lanes and 512 threads).
__device__ __forceinline__ void lane_cursors(const ScatterArgs &a, uint32_t tile, uint32_t *cur)
{
    const uint32_t tid = threadIdx.x, NT = blockDim.x, S = a.n_lanes;
    const uint32_t *base = a.base + (size_t)tile * a.row_step * S;
    constexpr uint32_t CU = 8;
    for (uint32_t k0 = tid; k0 < S; k0 += NT * CU) {
        uint32_t vy[CU];
#pragma unroll
        for (uint32_t u = 0; u < CU; ++u) vy[u] = base[min(k0 + u * NT, S - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < CU; ++u)
            if (k0 + u * NT < S) cur[k0 + u * NT] = vy[u];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// rx_scatterw: stable per-lane compaction without fan-out, W waves per scatter tile (one or
// several consecutive classify tiles, ScatterArgs::row_step). Wave w owns the w-th contiguous
// slice of the tile. Pass 1 counts each wave's deliveries per lane key with LDS atomics, whose
// returns are each delivery's rank within its key in the slice; each key's wave offsets then
// become the exclusive prefix over the earlier slices (and the keys' starts in the tile, for
// the staged write-out); the placement puts every delivery at cursor + slice offset + rank.
//
// Stability comes from the order in which a ds_add_rtn_u32 resolves lanes of one instruction
// that hit the same word: lane order on gfx950 (tools/probe/lds_order_probe.hip: 1.3e10 same-key
// lane pairs over 1-4096 keys, none out of order), and one wave's instructions execute in
// program order, so the returns number a key's frames of the slice in arrival order. (The first
// form ranked lanes by a wave multi-split over the key bits, 12 ballots per 64 frames at 4096
// lanes: 11 us per pass at config 5, instruction-bound; the atomics make a pass a few
// instructions per 64 frames.) Counters hold two waves each, 16 bits per wave (a scatter tile
// has <= 16384 frames, so neither half can carry into the other).
// LDS: 4 x max(n_lanes, W) (cursors) + 2 x W x n_lanes bytes (scatterw_lds_bytes).
// ------------------------------------------------------------------------------------------
template <uint32_t W>
__global__ void __launch_bounds__(64 * W)
rx_scatterw(ScatterArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smw[];
    const uint32_t S = a.n_lanes;
    // cursors [max(S, W)]: the first W words carry the key scan's wave totals until pass 2 (their
    // cursors wait in registers), so the LDS stays at 80 KiB for 8 waves at 4096 lanes (two
    // workgroups per CU)
    const uint32_t SC = S > W ? S : W;
    uint32_t *cur = smw;
    uint32_t *cnt = smw + SC;                                          // [W / 2][S] packed pairs
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t tile = xcd_tile(blockIdx.x, a.n_tiles);
    const uint32_t t1 = min(a.n, (tile + 1) * a.tile_frames);
    const uint32_t q = a.tile_frames / W;
    const uint32_t wb = tile * a.tile_frames + w * q, we = min(t1, wb + q);
    const uint32_t plast = a.n - 1u;
    uint32_t *mine = cnt + (w >> 1) * S;
    const uint32_t inc = (w & 1u) ? 0x10000u : 1u, sh = (w & 1u) * 16u;
    // the wave's whole slice of verdict words in registers (<= 16 per lane: tile_frames <=
    // 64 W SCATTERW_MV, checked by the host), loaded once for both passes (no load in the
    // counting or the placing loop) and issued first, so they are in flight during the cursor
    // prologue
    constexpr uint32_t MV = SCATTERW_MV;
    uint32_t mv[MV];
#pragma unroll
    for (uint32_t i = 0; i < MV; ++i) {
        const uint32_t p = wb + i * 64 + lane;
        mv[i] = (i * 64 < q) ? a.meta[min(p, plast)] : 0u;
    }
#ifdef UDPDK_STAMPS
    unsigned long long sacc[16] = {0}, slast = __builtin_amdgcn_s_memtime();
    sacc[12] = __builtin_amdgcn_s_memrealtime();
#endif
    // the cursors' loads (up to 8 per thread) in flight while the counters are zeroed (16-byte
    // LDS stores), then one barrier (the zeroing waited behind the cursor round trip before)
    uint32_t cur_lo;
    {
        const uint32_t *brow = a.base + (size_t)tile * a.row_step * S;
        constexpr uint32_t CU = 8;
        const uint32_t NT = 64 * W;
        uint32_t vy[CU];
#pragma unroll
        for (uint32_t u = 0; u < CU; ++u) vy[u] = brow[min(tid + u * NT, S - 1u)];
        if ((SC & 3u) == 0u) {                    // cnt = smw + SC is 16-byte aligned
            uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
            for (uint32_t k = tid; k < (W / 2) * S / 4; k += NT) c4[k] = make_uint4(0, 0, 0, 0);
        } else {
            for (uint32_t k = tid; k < (W / 2) * S; k += NT) cnt[k] = 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < CU; ++u)
            if (tid + u * NT < S && (u > 0 || tid >= W)) cur[tid + u * NT] = vy[u];
        cur_lo = vy[0];
        for (uint32_t k0 = tid + NT * CU; k0 < S; k0 += NT) cur[k0] = brow[k0];   // S > 4096: none
    }
    SSTAMP(0);
    __syncthreads();
    SSTAMP(1);
    // pass 1: per-wave counts; each atomic's return is the delivery's rank within its key in the
    // wave's slice (kept with the key: the placement adds the slice's offset, a plain LDS read,
    // where it made a second atomic per delivery)
    uint32_t kr[MV];                                                   // rank | key << 16
#pragma unroll
    for (uint32_t i = 0; i < MV; ++i) {
        kr[i] = 0xFFFFFFFFu;
        if (i * 64 >= q) break;                                        // uniform
        const uint32_t p = wb + i * 64 + lane;
        if (p < we && UDPDK_META_VERDICT(mv[i]) == UDPDK_V_DELIVERED) {
            const uint32_t key = UDPDK_META_SOCKFD(mv[i]) & a.lane_mask;
            const uint32_t o = atomicAdd(&mine[key], inc);
            kr[i] = ((o >> sh) & 0xFFFFu) | key << 16;
        }
    }
    __syncthreads();
    SSTAMP(2);
    // slice offsets: each wave's counts become the sum of the earlier slices' counts. Wave w
    // takes the contiguous keys [w KW, (w + 1) KW), lane l the keys w KW + 64 j + l (conflict-
    // free LDS rows), and keeps each key's tile total: their exclusive scan in key order (a wave
    // scan per j plus the earlier waves' totals) is each key's start in the tile's key-ordered
    // staging, held in registers until pass 2 has released the counter region. (The former
    // separate pass re-read the last pair's totals with 8 consecutive keys per thread: 8-way bank
    // conflicts and two more barriers, 6000 cycles of a 16-wave workgroup at config 5.)
    constexpr uint32_t KPT = SCATTERW_MAX_LANES / (64 * W);           // keys per lane
    const uint32_t KW = (S + 64 * W - 1) / (64 * W) * 64;               // keys per wave
    uint32_t *wtot = cur;                                               // [W] wave totals
    uint32_t kt[KPT] = {};
    {
        // every count the lane needs in flight at once (clamped addresses, masked values): one
        // LDS round trip instead of one per (key, wave pair). The j loops end at the wave's keys
        // (uniform), so the reads of one j are straight-line code.
        uint32_t cv[KPT][W / 2];
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            if (j * 64 >= KW) break;
            const uint32_t k = min(w * KW + j * 64 + lane, S - 1u);
#pragma unroll
            for (uint32_t jj = 0; jj < W / 2; ++jj) cv[j][jj] = cnt[jj * S + k];
        }
        __builtin_amdgcn_sched_barrier(0);         // all reads issued before the first use
        uint32_t run = 0;
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            if (j * 64 >= KW) break;
            const uint32_t k = w * KW + j * 64 + lane;
            const bool in = k < S;
            uint32_t c = 0;
#pragma unroll
            for (uint32_t jj = 0; jj < W / 2; ++jj) {
                const uint32_t v = in ? cv[j][jj] : 0u;
                const uint32_t lo = c, hi = c + (v & 0xFFFFu);
                cv[j][jj] = lo | (hi << 16);
                c = hi + (v >> 16);
            }
            if (in) {
#pragma unroll
                for (uint32_t jj = 0; jj < W / 2; ++jj) cnt[jj * S + k] = cv[j][jj];
            }
            const uint32_t incl = wave_incl_scan(c);
            kt[j] = run + incl - c;
            run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
        if (lane == 0) wtot[w] = run;
    }
    __syncthreads();
    uint32_t nd = 0;                                                    // the tile's deliveries
    {
        uint32_t before = 0;
#pragma unroll
        for (uint32_t j = 0; j < W; ++j) {
            const uint32_t t = wtot[j];
            before += j < w ? t : 0u;
            nd += t;
        }
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) kt[j] += before;
    }
    SSTAMP(3);
    // pass 2: placement. Staged when the tile's (frame, position) pairs fit the counter region:
    // every delivery's rank within its key comes from the atomics; the tile's deliveries are then
    // laid out in LDS in key order (each key's start from the scan above) and written out
    // linearly, so a wave's 64 stores fill runs of consecutive lane_pkt words (one run per key of
    // the tile) instead of 64 scattered words (config 5: rx_scatterw 24.5 -> 22.5 us). Otherwise
    // each delivery stores its own word (and needs every cursor now).
    const uint32_t T = a.tile_frames;
    const bool staged = (S & 1u) == 0u && 8u * T <= 4u * (W / 2) * S;   // 8-byte pairs in cnt
    if (!staged) {
        __syncthreads();                                               // wave totals read
        if (tid < W && tid < S) cur[tid] = cur_lo;
        __syncthreads();
    }
#pragma unroll
    for (uint32_t i = 0; i < MV; ++i) {
        if (i * 64 >= q) break;                                        // uniform
        if (kr[i] != 0xFFFFFFFFu) {
            const uint32_t key = kr[i] >> 16;
            const uint32_t rank = (kr[i] & 0xFFFFu) + ((mine[key] >> sh) & 0xFFFFu);
            if (staged) {
                kr[i] = rank | key << 16;
            } else {
                const uint32_t pos = cur[key] + rank;
                if (pos < a.lane_cap) a.lane_pkt[pos] = wb + i * 64 + lane;
            }
        }
    }
    SSTAMP(4);
    if (staged) {
        // every wave's pass 2 is done with the counters: the key starts go where they were
        __syncthreads();
        uint32_t *lex = cnt;                                           // [S] key start in the tile
#pragma unroll
        for (uint32_t j = 0; j < KPT; ++j) {
            const uint32_t k = w * KW + j * 64 + lane;
            if (j * 64 < KW && k < S) lex[k] = kt[j];
        }
        if (tid < W && tid < S) cur[tid] = cur_lo;                     // wave totals read long ago
        __syncthreads();
        SSTAMP(6);
        // each delivery's place in key order and its lane position into registers first (lex
        // is read), then (frame, position) pairs into LDS over the whole counter region
        uint32_t li[MV], ps[MV];
#pragma unroll
        for (uint32_t i = 0; i < MV; ++i) {
            li[i] = 0xFFFFFFFFu;
            if (i * 64 >= q) break;
            if (kr[i] != 0xFFFFFFFFu) {
                const uint32_t key = kr[i] >> 16, rank = kr[i] & 0xFFFFu;
                li[i] = lex[key] + rank;
                ps[i] = cur[key] + rank;
            }
        }
        __syncthreads();
        SSTAMP(7);
        uint2 *pp = reinterpret_cast<uint2 *>(cnt);                    // [T] (frame, position)
#pragma unroll
        for (uint32_t i = 0; i < MV; ++i) {
            if (i * 64 >= q) break;
            if (li[i] != 0xFFFFFFFFu) pp[li[i]] = make_uint2(wb + i * 64 + lane, ps[i]);
        }
        __syncthreads();
        SSTAMP(8);
        for (uint32_t i = tid; i < nd; i += 64 * W) {
            const uint2 e = pp[i];
            if (e.y < a.lane_cap) a.lane_pkt[e.y] = e.x;
        }
    }
    SSTAMP(5);
#ifdef UDPDK_STAMPS
    sacc[13] = __builtin_amdgcn_s_memrealtime();
    sacc[14] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
               ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
    sacc[15] = tile;
    if (a.dbg && w == 0 && lane < 16 && tile < RX_TILE_MAX) a.dbg[(size_t)(RX_TILE_MAX * 2 + tile) * 16 + lane] = sacc[lane];
#endif
}

template __global__ void rx_scatterw<SCATTER_WAVES>(ScatterArgs a);
template __global__ void rx_scatterw<2 * SCATTER_WAVES>(ScatterArgs a);

// ------------------------------------------------------------------------------------------
// rx_scatter: stable per-lane compaction, one wave per tile
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SCATTER1_BLOCK)
rx_scatter(ScatterArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *cur = reinterpret_cast<uint32_t *>(smem);   // running position per lane
    const uint32_t lane = lane_id();
    const uint32_t tile = xcd_tile(blockIdx.x, a.n_tiles);
    // cursor of every lane for this tile: the whole workgroup runs the prologue, wave 0 the walk
    lane_cursors(a, tile, cur);
    if (threadIdx.x >= 64) return;
    const uint32_t t0 = tile * a.tile_frames;
    const uint32_t t1 = min(a.n, t0 + a.tile_frames);

    constexpr int PF = 8;                                 // verdict words prefetched per lane
    for (uint32_t g0 = t0; g0 < t1; g0 += 64 * PF) {
        uint32_t mv[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const uint32_t p = g0 + i * 64 + lane;
            mv[i] = p < t1 ? a.meta[p] : 0u;
        }
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const uint32_t f0 = g0 + i * 64;
            if (f0 >= t1) break;
            const uint32_t p = f0 + lane;
            const bool valid = p < t1;
            const uint32_t m = mv[i];
            const bool deliver = valid && UDPDK_META_VERDICT(m) == UDPDK_V_DELIVERED;
            const uint32_t fan = UDPDK_META_FANOUT(m);
            const unsigned long long multi = __ballot(deliver && fan > 1u);
            if (multi == 0ull) {
                // one delivery per frame: the LDS atomic on the lane's cursor returns the
                // position, lanes of one key numbered in lane order (see rx_scatterw)
                if (deliver) {
                    const uint32_t pos = atomicAdd(&cur[UDPDK_META_SOCKFD(m) & a.lane_mask], 1u);
                    if (pos < a.lane_cap) a.lane_pkt[pos] = p;
                }
            } else if (lane == 0) {
                // fan-out (SO_REUSEADDR/SO_REUSEPORT clones, poller.c:396-399): deliveries in
                // frame order then list order, re-derived from the frame header. Serial.
                for (uint32_t q = 0; q < 64 && f0 + q < t1; ++q) {
                    const uint32_t fp = f0 + q;
                    const uint32_t mi = a.meta[fp];
                    if (UDPDK_META_VERDICT(mi) != UDPDK_V_DELIVERED) continue;
                    const uint8_t *f = a.frames + a.offset[fp];
                    const uint32_t dport = (uint32_t)f[36] | ((uint32_t)f[37] << 8);
                    const uint32_t dip = (uint32_t)f[30] | ((uint32_t)f[31] << 8) |
                                         ((uint32_t)f[32] << 16) | ((uint32_t)f[33] << 24);
                    const uint4 e = a.port_tab[dport];
                    uint32_t bip = e.z, bsr = e.w;
                    for (uint32_t k = 0;;) {
                        if (dip == bip || bip == 0u) {
                            const uint32_t key = (bsr & 0x7FFFFFFFu) & a.lane_mask;
                            const uint32_t c = cur[key];
                            cur[key] = c + 1u;
                            if (c < a.lane_cap) a.lane_pkt[c] = fp;
                            if (!(bsr >> 31)) break;
                        }
                        if (++k >= e.x) break;
                        const uint2 b = a.binds[e.y + k];
                        bip = b.x;
                        bsr = b.y;
                    }
                }
            }
            wave_sync();
        }
    }
}

} // namespace udpdk
