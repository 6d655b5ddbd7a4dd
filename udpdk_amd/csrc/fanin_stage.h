// fanin_stage.h — the skeleton of the control-plane stages igmp_reply, neigh_learn and neigh_resolve,
// each piece defined once; the ICMP stages use its counting pieces, and every stage that loads frame
// bytes its OOR. (arp_reply has the same shape and spells it out itself.) Device-only, all inlined.
//
// The shape: every workgroup sweeps its tile and leaves a field-major row of counts (row[f * nb + b])
// and, where the stage has them, its candidates compacted in frame order. The launch's last
// workgroup to arrive (arrive_last) finishes alone: the sums of the rows (row_sums), the exclusive
// prefix of one field (row_bases), then the candidates in order (block_of finds candidate r's
// workgroup). No workgroup waits for another, and the fan-in words are left zeroed for the next
// launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rx_common.h"
#include "wave.h"

namespace udpdk {

// The buffer offset of a lane with nothing to read. A dword comes from memory only if it ends within
// the resource's range, so up to rsrc_bytes = 0xFFFFFFF0 (frames_bytes <= 0xFFFFFFED) a load here
// touches no memory and returns zeros. The host passes at most 0xFFFFFFFC: for those last few sizes
// the first one to three dwords of a load here lie inside the frames buffer's own range (readable
// memory, never past it: no site adds to OOR before a 16-byte load, which so ends at 2^32 without
// wrapping, and none adds more than 4 before a dword load). Either way the value is never used:
// every site masks what it loaded by the predicate that chose OOR.
constexpr uint32_t OOR = 0xFFFFFFF0u;

// Words the finisher reads and writes: agent scope, past the CU's L1 (a later step reads what other
// lanes of the workgroup wrote), and words a sweep writes through for the finisher (arrive_last).
__device__ __forceinline__ uint32_t agent_ld(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void agent_st(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A workgroup's N counts from its waves' (wave-uniform) counts through red[][] in LDS (N <= F): every
// wave puts its own, and after a barrier field f's sum over the NW waves is anybody's to take.
template <uint32_t N, uint32_t F>
__device__ __forceinline__ void wave_counts_put(uint32_t (*red)[F], const uint32_t (&cnt)[N])
{
    static_assert(N <= F, "red[] holds F fields per wave");
    if (lane_id() == 0) {
#pragma unroll
        for (uint32_t f = 0; f < N; ++f) red[threadIdx.x >> 6][f] = cnt[f];
    }
}
template <int NW, uint32_t F>
__device__ __forceinline__ uint32_t wave_counts_sum(const uint32_t (*red)[F], uint32_t f)
{
    uint32_t t = 0u;
#pragma unroll
    for (int j = 0; j < NW; ++j) t += red[j][f];
    return t;
}
// ... and stored by lanes [0, N): dst[f * stride] = field f's sum (a workgroup's field-major row:
// dst = row + b, stride = nb; a result's counts: stride 1). THROUGH: written through (agent_st).
template <int NW, uint32_t N, bool THROUGH = false, uint32_t F>
__device__ __forceinline__ void row_store(const uint32_t (*red)[F], uint32_t *dst, size_t stride)
{
    static_assert(N <= F, "red[] holds F fields per wave");
    const uint32_t tid = threadIdx.x;
    if (tid < N) {
        const uint32_t t = wave_counts_sum<NW>(red, tid);
        if constexpr (THROUGH) agent_st(dst + tid * stride, t);
        else dst[tid * stride] = t;
    }
}

// How a workgroup's sweep ends: every wave's stores drained, one agent release, the arrival
// (fanin_arrive). True in every lane of the launch's last workgroup, after its acquire.
// RELEASE = false: what the finisher reads of this workgroup was stored written-through (agent_st),
// so no release is needed: a sweep that also streams megabytes of output the finisher never reads
// (neigh_resolve) does not have every workgroup ask for their write-back.
template <bool RELEASE>
__device__ __forceinline__ bool arrive_last(unsigned long long *fuse, uint32_t b, uint32_t nb, uint32_t *s_last)
{
    stores_done();
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (RELEASE) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            stores_done();
        }
        unsigned long long fin;
        *s_last = fanin_arrive(fuse, b, nb, 0ull, &fin) ? 1u : 0u;
    }
    __syncthreads();
    if (!*s_last) return false;
    if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    stores_done();
    __syncthreads();
    return true;
}

// Finisher, all BLOCK lanes: the sums of the F row fields over the nb workgroups into tot[] (LDS).
template <int BLOCK, uint32_t F>
__device__ __forceinline__ void row_sums(const uint32_t *row, uint32_t nb, uint32_t (*red)[F], uint32_t *tot)
{
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    uint32_t acc[F];
#pragma unroll
    for (uint32_t f = 0; f < F; ++f) acc[f] = 0u;
    for (uint32_t t = tid; t < nb; t += BLOCK) {
#pragma unroll
        for (uint32_t f = 0; f < F; ++f) acc[f] += row[(size_t)f * nb + t];
    }
#pragma unroll
    for (uint32_t f = 0; f < F; ++f) {
        const uint32_t s = wave_sum(acc[f]);
        if (lane == 0) red[w][f] = s;
    }
    __syncthreads();
    if (tid < F) tot[tid] = wave_counts_sum<BLOCK / 64>(red, tid);
    __syncthreads();
}

// Finisher, all BLOCK lanes: rbase[g] = the sum of cnt[0 .. g) (a contiguous run of
// ceil(nb / BLOCK) rows per lane), written at agent scope and complete when this returns.
template <int BLOCK>
__device__ __forceinline__ void row_bases(const uint32_t *cnt, uint32_t *rbase, uint32_t nb, uint32_t *wsum)
{
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t per = (nb + BLOCK - 1u) / BLOCK;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    uint32_t su = 0u;
    for (uint32_t t = b0; t < b1; ++t) su += cnt[t];
    uint32_t wt;
    uint32_t u = wave_excl_scan(su, &wt);
    if (lane == 0) wsum[w] = wt;
    __syncthreads();
    for (uint32_t j = 0; j < w; ++j) u += wsum[j];
    for (uint32_t t = b0; t < b1; ++t) {
        agent_st(rbase + t, u);
        u += cnt[t];
    }
    stores_done();
    __syncthreads();
}

// The last workgroup g of [0, nb) with rbase[g] <= r (those after it with the same base are empty).
__device__ __forceinline__ uint32_t block_of(const uint32_t *rbase, uint32_t nb, uint32_t r, uint32_t *first)
{
    uint32_t lo = 0u, hi = nb, f = 0u;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t v = agent_ld(rbase + mid);
        if (v <= r) { lo = mid; f = v; } else hi = mid;
    }
    *first = f;
    return lo;
}

} // namespace udpdk
