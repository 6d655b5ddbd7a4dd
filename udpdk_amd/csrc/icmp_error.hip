// icmp_error.hip — gfx950 ICMP errors received for connected sockets: of a finished RX call, the
// destination-unreachable messages (RFC 792 type 3) that quote a datagram one of our connected
// sockets sent to its peer, reported as one 64-bit word per lane (RFC 1122 §4.1.3.3: UDP MUST pass
// ICMP errors up to the application). The rules are stated in udpdk_gpu.h (udpdk_gpu_icmp_errors);
// the reference has no ICMP and no connect.
//
//   icmp_err_clear  err[0, n_lanes) and the counters, one launch.
//   icmp_err_scan   ICMP_ERR_TILE frames per workgroup, one per lane, over meta. A frame whose
//                   verdict word does not make it a candidate costs its 4 bytes of meta and nothing
//                   else, and a wave without a candidate does nothing more. A candidate reads its
//                   descriptor and frame bytes [14, 66) (rx_gather's byte-aligned, range-checked
//                   dword loads: the outer headers, the ICMP header, the quoted IPv4 header and
//                   the quoted ports), and a type-3 message to us has bytes [34, 14 + tl) summed: up
//                   to ICMP_ERR_LANE_SUM_MAX bytes by its own lane, a longer message (routers quote
//                   as much as they can) by the whole wave, 16 bytes per lane per step, one
//                   candidate after another (icmp_scan's split). A hard error then walks the
//                   bindings of the quoted source port with plain global loads, reads the peer
//                   record of every binding whose address fits, and reports to each match by a
//                   64-bit atomic max of (frame + 1) << 8 | code: the last hard error in arrival
//                   order wins whatever the scheduling. Of a wave's matches for one lane in one
//                   step of the walk only the last frame's issues the atomic (wave_peers).
//                   Counts: ballots per wave, the waves' counts through LDS, one atomic add per
//                   counter and workgroup that has something.
// Two launches in stream order, no second pass.
//
// Bytes per frame: 4 (meta). Per candidate: + 6 (descriptor) + the one or two 64-byte requests that
// hold bytes 14-65. Per error to us: + the message once. Per hard error: + 16 (port entry) + 8 per
// further binding + 8 per peer record read + at most one 8-byte atomic per match.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "icmp_error.h"
#include "wave.h"
#include "fanin_stage.h"

namespace udpdk {

namespace {

constexpr int NW = ICMP_ERR_BLOCK / 64;

} // namespace

__global__ void __launch_bounds__(ICMP_ERR_BLOCK)
icmp_err_clear(unsigned long long *err, uint32_t n_lanes, IcmpErrResult *res)
{
    const uint32_t t = blockIdx.x * ICMP_ERR_BLOCK + threadIdx.x;
    if (t < n_lanes) err[t] = 0ull;
    if (t < ICMP_ERR_ROW + 1u) reinterpret_cast<uint32_t *>(res)[t] = 0u;
}

__global__ void __launch_bounds__(ICMP_ERR_BLOCK)
icmp_err_scan(IcmpErrArgs a)
{
    __shared__ uint32_t red[NW][ICMP_ERR_ROW];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint64_t i64 = (uint64_t)blockIdx.x * ICMP_ERR_TILE + tid;
    const bool valid = i64 < a.n;
    const uint32_t i = (uint32_t)i64;
    // the verdict word says who is a candidate: everything below is skipped by a wave without one
    const uint32_t m = valid ? a.meta[i] : 0xFu;
    const bool cand = valid && UDPDK_META_VERDICT(m) == UDPDK_V_NOT_UDP && UDPDK_META_IP_OK(m) && !UDPDK_META_IHL_NE5(m);
    uint32_t cnt[ICMP_ERR_ROW] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (__ballot(cand)) {                                          // wave-uniform
        const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
        const uint32_t o = cand ? a.offset[i] : 0u;
        const uint32_t len = cand ? (uint32_t)a.length[i] : 0u;
        const bool fok = cand && len >= 42u && (uint64_t)o + len <= a.frames_bytes;
        // frame bytes [14, 66) as thirteen dwords; lanes with nothing to read address out of range
        const uint32_t X = o + 14u, sh = X & 3u, A = X & ~3u;
        const uint4 d0 = load16(fr, fok ? A : OOR), d1 = load16(fr, fok ? A + 16u : OOR);
        const uint4 d2 = load16(fr, fok ? A + 32u : OOR), d3 = load16(fr, fok ? A + 48u : OOR);
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d0.y, d0.x, sh);      // bytes 14-17
        const uint32_t w2 = __builtin_amdgcn_alignbyte(d0.w, d0.z, sh);      // 22-25
        const uint32_t w4 = __builtin_amdgcn_alignbyte(d1.y, d1.x, sh);      // 30-33: destination
        const uint32_t w5 = __builtin_amdgcn_alignbyte(d1.z, d1.y, sh);      // 34-37: type, code, checksum
        const uint32_t w7 = __builtin_amdgcn_alignbyte(d2.x, d1.w, sh);      // 42-45: the quote's version / IHL
        const uint32_t w8 = __builtin_amdgcn_alignbyte(d2.y, d2.x, sh);      // 46-49: its fragment field
        const uint32_t w9 = __builtin_amdgcn_alignbyte(d2.z, d2.y, sh);      // 50-53: its protocol
        const uint32_t w10 = __builtin_amdgcn_alignbyte(d2.w, d2.z, sh);     // 54-57: quoted source
        const uint32_t w11 = __builtin_amdgcn_alignbyte(d3.x, d2.w, sh);     // 58-61: quoted destination
        const uint32_t w12 = __builtin_amdgcn_alignbyte(d3.y, d3.x, sh);     // 62-65: quoted ports
        const uint32_t tl = bswap16(w0 >> 16), proto = (w2 >> 8) & 0xFFu, code = (w5 >> 8) & 0xFFu;
        const bool is_err = fok && proto == 1u && (w5 & 0xFFu) == 3u && w4 == a.our_ip;
        const bool lens_ok = is_err && tl >= 56u && 14u + tl <= len;
        // the sum of the message, frame bytes [34, 14 + tl)
        const uint32_t S = o + 34u, rl = lens_ok ? tl - 20u : 0u;
        uint32_t R = 0u;
        const bool own = lens_ok && rl <= ICMP_ERR_LANE_SUM_MAX;
#pragma unroll
        for (uint32_t k = 0; k < ICMP_ERR_LANE_SUM_MAX / 16u; ++k) {
            const bool need = own && 16u * k < rl;
            if (__ballot(need)) {
                const uint4 d = load16(fr, need ? S + 16u * k : OOR);
                R += chunk_sum(d, 0, need ? (int)(rl - 16u * k) : 0);
            }
        }
        // the long messages of the wave, one after another, each by every lane
        unsigned long long todo = __ballot(lens_ok && !own);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t Sj = __shfl(S, j, 64), rj = __shfl(rl, j, 64);
            uint32_t acc = 0u;                                      // <= 64 steps x 8 x 0xffff
            for (uint32_t b = 16u * lane; b < rj; b += 1024u) acc += chunk_sum(load16(fr, Sj + b), 0, (int)(rj - b));
            const uint32_t tot = wave_sum(fold32(acc));
            if (lane == (uint32_t)j) R = tot;
        }
        const bool msg_ok = lens_ok && fold32(R) == 0xFFFFu;
        const bool quote_ok = msg_ok && (w7 & 0xFFu) == 0x45u && ((w9 >> 8) & 0xFFu) == 17u &&
                              (bswap16(w8 >> 16) & 0x1FFFu) == 0u;
        const bool hard = quote_ok && code < 16u && ((ICMP_ERR_HARD_MASK >> code) & 1u);
        // the sockets: the bindings of the quoted source port in list order (binding 0 rides in the
        // port entry), every match reported. The walk is wave-uniform, one binding of every hard
        // error per step: of a step's matches for one lane only the last frame's goes to memory
        // (the largest word: the frame index grows with the wave's lanes), so a burst of errors
        // about one socket is one atomic per wave and step, not one per frame.
        uint32_t pairs = 0u, nb = 0u;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (hard) {
            e = a.port_tab[w12 & 0xFFFFu];
            nb = min(e.x, UDPDK_GPU_MAX_PORT_BINDS);
        }
        const uint32_t dport = w12 >> 16;
        const unsigned long long word = ((unsigned long long)(i + 1u) << 8) | code;
        for (uint32_t k = 0; __ballot(k < nb) != 0ull; ++k) {       // wave-uniform
            bool match = false;
            uint32_t l = 0u;
            if (k < nb) {
                const uint2 b = k == 0u ? make_uint2(e.z, e.w) : a.binds[e.y + k];
                l = b.y & 0x7FFFFFFFu;
                if (l < a.n_lanes && l < a.peer_n && (b.x == w10 || (b.x == 0u && w10 == a.our_ip))) {
                    const uint2 pr = a.peer[l];
                    match = (pr.y >> 16) != 0u && pr.x == w11 && (pr.y & 0xFFFFu) == dport;
                }
                if (!match) l = 0u;
            }
            if (__ballot(match) == 0ull) continue;                  // wave-uniform
            const unsigned long long same = wave_peers(l, ICMP_ERR_LANE_BITS, match);
            if (match) {
                if ((same >> lane) == 1ull) atomicMax(&a.err[l], word);   // no later frame for lane l in the wave
                ++pairs;
            }
        }
        cnt[ICMP_X_ERRORS] = (uint32_t)__popcll(__ballot(is_err));
        cnt[ICMP_X_MSG_BAD] = (uint32_t)__popcll(__ballot(is_err && !msg_ok));
        cnt[ICMP_X_QUOTE_BAD] = (uint32_t)__popcll(__ballot(msg_ok && !quote_ok));
        cnt[ICMP_X_SOFT] = (uint32_t)__popcll(__ballot(quote_ok && !hard));
        cnt[ICMP_X_NO_SOCKET] = (uint32_t)__popcll(__ballot(hard && pairs == 0u));
        cnt[ICMP_X_REPORTED] = wave_sum(pairs);
        cnt[ICMP_X_BAD_FRAME] = (uint32_t)__popcll(__ballot(cand && !fok));
    }
    wave_counts_put(red, cnt);
    __syncthreads();
    if (tid < ICMP_ERR_ROW) {
        const uint32_t t = wave_counts_sum<NW>(red, tid);
        if (t) atomicAdd(&a.res->c[tid], t);
    }
}

} // namespace udpdk
