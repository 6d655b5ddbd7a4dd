// wave.h — the wave64 device primitives the gfx950 kernels stand on, each defined once: wave
// ordering, DPP scans, the wave multi-split, byte-range masks, RFC 1071 pieces, buffer-resource
// loads and stores. Device-only, all inlined; each comment says what the primitive costs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rx_common.h"

namespace udpdk {

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// Orders LDS accesses of one wave across lanes: no instruction. The hardware executes a wave's DS
// instructions in order, so only the compiler must be kept from reordering them; a wavefront-scope
// fence would also emit vmcnt(0) and drain every prefetch in flight.
__device__ __forceinline__ void wave_sync()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Every vector-memory access this wave issued has completed, its stores included (CDNA counts
// stores in vmcnt): one s_waitcnt, as long as the slowest access in flight.
__device__ __forceinline__ void stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Inclusive prefix sum across the wave, on the DPP network (row shifts + row broadcasts: six
// VALU ops, no LDS traffic; the __shfl_up form was six ds_bpermute round trips through the LDS
// pipeline, which the LDS-bound scatter paid for in every scan). Every lane must be active.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);   // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return v;
}

// Exclusive prefix sum of v over the wave's lanes; *total gets the wave's sum: wave_incl_scan, a
// readlane and a subtraction. Called with every lane active (wave-uniform control flow).
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t *total)
{
    const uint32_t x = wave_incl_scan(v);
    *total = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    return x - v;
}

// Inclusive prefix maximum across the wave on the DPP network (the shifts of wave_incl_scan: six
// DPP moves and six v_max). Every lane must be active.
__device__ __forceinline__ uint32_t wave_max_scan(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
    return v;
}

// The wave's sum in every lane: six xor-shuffles (ds_bpermute round trips), for sums off the hot
// loops.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Wave multi-split: the active lanes of the wave holding the same key (key < 2^bits), from one
// ballot per key bit.
__device__ __forceinline__ unsigned long long wave_peers(uint32_t key, uint32_t bits, bool active)
{
    unsigned long long peers = __ballot(active);
    for (uint32_t b = 0; b < bits; ++b) {
        const bool kb = (key >> b) & 1u;
        const unsigned long long bal = __ballot(kb);
        peers &= kb ? bal : ~bal;
    }
    return peers;
}

// Bytes [a, e) of a 16-byte chunk as a dword mask for dword i (a, e clamped to [0, 16]); the
// bytes [lo, hi) of the dword at byte `base` of anything are dword_window(lo - base, hi - base, 0).
// A handful of VALU ops, folded to a constant where the range is one.
__device__ __forceinline__ uint32_t dword_window(int a, int e, int i)
{
    const int la = min(max(a - 4 * i, 0), 4);
    const int le = min(max(e - 4 * i, 0), 4);
    const uint32_t hm = le >= 4 ? 0xFFFFFFFFu : ((1u << (8 * le)) - 1u);
    const uint32_t lm = la >= 4 ? 0xFFFFFFFFu : ((1u << (8 * la)) - 1u);
    return hm & ~lm;
}

// Both 16-bit halves of v added: and / shift / add3, three VALU ops.
__device__ __forceinline__ uint32_t sum16(uint32_t v) { return (v & 0xFFFFu) + (v >> 16); }

// acc + both 16-bit halves of v in ONE instruction: v_sad_u16(v, 0, acc) = |v.lo - 0| + |v.hi - 0|
// + acc. The RFC 1071 sums are chains of these (the and/shift/add3 form of sum16 is three).
__device__ __forceinline__ uint32_t sad16(uint32_t v, uint32_t acc)
{
    return __builtin_amdgcn_sad_u16(v, 0u, acc);
}

// One's-complement fold of a 32-bit sum of 16-bit words to [0, 0xffff] (0xffff is -0: a valid
// RFC 1071 sum folds to 0xffff; only an all-zero input folds to 0).
__device__ __forceinline__ uint32_t fold32(uint32_t x)
{
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// Sum of the 16-bit halves of the bytes [a, e) of the chunk: <= 8 * 0xFFFF.
__device__ __forceinline__ uint32_t chunk_sum(const uint4 d, int a, int e)
{
    if (e <= a) return 0u;
    if (a <= 0 && e >= 16) return sum16(d.x) + sum16(d.y) + sum16(d.z) + sum16(d.w);
    return sum16(d.x & dword_window(a, e, 0)) + sum16(d.y & dword_window(a, e, 1)) +
           sum16(d.z & dword_window(a, e, 2)) + sum16(d.w & dword_window(a, e, 3));
}

// The low 16 bits of x byte-swapped (network <-> host order), bits 16-31 ignored: two or three
// VALU ops (fewer where the compiler knows x < 2^16).
__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }

// Buffer resource over [p, p + bytes): raw buffer accesses past it load zeros and store nothing,
// so a range check is an offset, not a branch. Four SGPRs, built once per kernel.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes,
                                             0x00020000);
}

// One buffer_load_dword / _dwordx4 / buffer_store_dwordx4 at a byte offset.
// AUX: the access's cache policy bits (rx_common.h, memory policy)
template <int AUX = 0>
__device__ __forceinline__ uint32_t load4(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, AUX);
}

template <int AUX = 0>
__device__ __forceinline__ uint4 load16(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

template <int AUX = 0>
__device__ __forceinline__ void store16(__amdgpu_buffer_rsrc_t r, uint32_t off, uint4 v)
{
    __attribute__((ext_vector_type(4))) uint32_t x = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(x, r, (int)off, 0, AUX);
}

// a plain pointer load under a policy: AUX_NT = the global load's nt bit
template <int AUX, typename T>
__device__ __forceinline__ T load_pol(const T *p)
{
    if constexpr ((AUX & AUX_NT) != 0) return __builtin_nontemporal_load(p);
    else return *p;
}

} // namespace udpdk
