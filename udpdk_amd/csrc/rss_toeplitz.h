// rss_toeplitz.h — the Toeplitz hash by the 12 x 256 key-window table (rss_host.h builds it), stated
// once for the kernels that hash a frame's addresses and ports: rss_hash (rx_rss.hip) and
// rx_balance_pick (rx_balance.hip). Device-only, inlined: 8 or 12 table lookups and XORs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace udpdk {

// tab[p][v]: the table, in LDS or memory. sa, da, pp: frame bytes 26-29, 30-33, 34-37 as
// little-endian dwords; the ports enter the hash only with `ports`.
template <typename Tab>
__device__ __forceinline__ uint32_t rss_toeplitz(const Tab &tab, uint32_t sa, uint32_t da, uint32_t pp, bool ports)
{
    uint32_t hash = tab[0][sa & 255u] ^ tab[1][(sa >> 8) & 255u] ^ tab[2][(sa >> 16) & 255u] ^
                    tab[3][sa >> 24] ^ tab[4][da & 255u] ^ tab[5][(da >> 8) & 255u] ^
                    tab[6][(da >> 16) & 255u] ^ tab[7][da >> 24];
    if (ports)
        hash ^= tab[8][pp & 255u] ^ tab[9][(pp >> 8) & 255u] ^ tab[10][(pp >> 16) & 255u] ^
                tab[11][pp >> 24];
    return hash;
}

} // namespace udpdk
