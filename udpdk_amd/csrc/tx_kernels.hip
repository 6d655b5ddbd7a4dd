// tx_kernels.hip — gfx950 TX header build (udpdk_syscall.c:314-356) for a batch of datagrams,
// with the poller's IPv4 fragmentation (udpdk_poller.c:461-501) when an MTU is given.
//
// Per datagram: Ethernet (config MACs, type 0x0800), IPv4 (0x45, tos 0, total length, id 0,
// frag 0, ttl 64, proto 17, rte_ipv4_cksum, src = bound slot IP unless ANY else config IP,
// dst), UDP (raw src/dst ports, length, checksum 0 or, in tx_build<true>, the RFC 768 checksum
// over the pseudo-header, the UDP header and the payload), then the payload.
//
// Fragmentation (mtu != 0 and len + 42 > mtu, the poller's pkt_len > IPV4_MTU_DEFAULT test):
// the IPv4 packet is cut the way DPDK 20.05 rte_ipv4_fragment_packet does (restated in
// oracle/udpdk_oracle.c): every fragment carries mtu - 20 bytes of the IP payload (UDP header +
// data), the last the remainder; each fragment repeats the Ethernet header and the IPv4 header
// with total length = 20 + its payload, fragment offset in 8-byte units and MF on all but the
// last. DPDK leaves the fragment header checksum 0 with PKT_TX_IP_CKSUM set, so the NIC fills
// it: here it is filled as the NIC would (~fold of the RFC 1071 sum). A datagram's frames are
// contiguous from frame_off[i]: fragment k at + k * (mtu + 14), so its span is
// (len + 8) + 34 * n_frames (len + 42 unfragmented).
//
// A wave takes 64 datagrams, expands them into output frames (one per datagram unless it is
// fragmented) and handles 64 frames per round: one lane builds a frame's 42 (or 34) header
// bytes into an LDS window laid out with the output frame's 16-byte alignment; the frames are
// then written as 16-byte chunks swept across lanes (whole chunks as one 16 B store,
// frame-boundary chunks byte-masked), the payload read with two aligned 16 B loads and a funnel
// shift. Bytes per datagram: len read + span written + 4 x 4 B + 2 x 2 B descriptors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "wave.h"
#include "tx_ipv4.h"

namespace udpdk {

namespace {

// Not wave.h's wave_sync: a wavefront-scope fence, which also drains vmcnt.
__device__ __forceinline__ void wave_sync_tx()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Not wave.h's wave_excl_scan: the __shfl_up chain (ds_bpermute), not the DPP network.
__device__ __forceinline__ uint32_t excl_scan64(uint32_t v, uint32_t *total)
{
    const uint32_t lane = lane_id();
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    *total = __shfl(x, 63, 64);
    return x - v;
}

__device__ __forceinline__ uint32_t sel4(uint32_t d, uint32_t a0, uint32_t a1, uint32_t a2,
                                         uint32_t a3)
{
    return d == 0 ? a0 : (d == 1 ? a1 : (d == 2 ? a2 : a3));
}

// (ipv4_raw, ipv4_cksum, ipv4_cksum_nic: tx_ipv4.h, shared with icmp_build)

// The RFC 768 terms that are not payload, as LE 16-bit words like ipv4_raw: the pseudo-header
// (src, dst, zero, 17, UDP length) and the UDP header (raw ports, length, checksum field 0).
__device__ __forceinline__ uint32_t udp_head_sum(uint32_t src, uint32_t dst, uint32_t pt, uint32_t ul)
{
    return sad16(src, sad16(dst, sad16(pt, 0x1100u + 2u * bswap16(ul))));
}

// The checksum field for a one's-complement sum s of everything it covers: folded,
// complemented, and 0 sent as 0xffff (RFC 768: a transmitted 0 means "no checksum").
__device__ __forceinline__ uint32_t udp_cksum(uint32_t s)
{
    const uint32_t c = ~fold32(s) & 0xFFFFu;
    return c ? c : 0xFFFFu;
}

constexpr int TX_WIN = 64;  // bytes of header window per frame (16 dwords)
constexpr int TXW = TX_BLOCK / 64;

constexpr uint32_t TX_SMALL_SPAN = 80;       // frames up to this size take tx_small
constexpr uint32_t TX_SMALL_LOADS = (TX_SMALL_SPAN - 42u + 15u) / 16u;

// The frame of datagram i built in this lane's registers and stored as 16-byte pieces: for waves
// whose frames are all <= TX_SMALL_SPAN bytes and unfragmented. The payload loads go out with
// the slot lookup (byte-aligned 16-byte buffer loads; pieces past the payload are addressed out
// of range, so they cost no memory access and read as 0), so a wave's frames take one round
// trip after the descriptors instead of one per 64-chunk sweep step.
// DM: bytes 0-5 are the datagram's own (dm_lo, dm_hi: TxNeighArgs::dmac) instead of the config's.
template <bool CK, bool DM>
__device__ __forceinline__ void tx_small(const TxArgs &a, uint32_t i, uint32_t fo, uint32_t L,
                                         uint32_t po, int32_t sock, uint32_t dm_lo, uint32_t dm_hi)
{
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(a.payload, a.payload_rsrc);
    const __amdgpu_buffer_rsrc_t fw = make_rsrc(a.frames, a.frames_bytes);
    const uint32_t span = L + 42u;
    const bool ok = i < a.n && (uint64_t)fo + span <= a.frames_bytes &&
                    (uint64_t)po + L <= a.payload_bytes && sock >= 0 && (uint32_t)sock < a.n_slots;
    uint32_t P[4 * TX_SMALL_LOADS + 1];
#pragma unroll
    for (uint32_t m = 0; m < TX_SMALL_LOADS; ++m) {
        // (a piece no lane needs is not issued: its lanes would still cost address-unit cycles)
        const bool need = ok && 16u * m < L;
        P[4 * m] = P[4 * m + 1] = P[4 * m + 2] = P[4 * m + 3] = 0u;
        if (__ballot(need)) {
            const uint4 v = load16(pr, need ? po + 16u * m : 0x80000000u);
            P[4 * m] = v.x; P[4 * m + 1] = v.y; P[4 * m + 2] = v.z; P[4 * m + 3] = v.w;
        }
    }
    P[4 * TX_SMALL_LOADS] = 0u;
    if (!ok) return;
    const uint4 sl = a.slots[sock];
    const uint32_t sq = (sl.z && sl.x != 0u) ? sl.x : a.src_ip;                    // :329-334
    const uint32_t dq = a.dst_ip[i];                                               // :335
    const uint32_t ptq = (sl.y & 0xFFFFu) | ((uint32_t)a.dst_port[i] << 16);        // :341-342
    const uint32_t tl = L + 28u, ul = L + 8u;                                      // :336, :344
    uint32_t H[10];
    H[0] = a.mac_lo[0]; H[1] = a.mac_lo[1]; H[2] = a.mac_lo[2];                    // :315-317
    if constexpr (DM) {
        H[0] = dm_lo;
        H[1] = (dm_hi & 0xFFFFu) | (a.mac_lo[1] & 0xFFFF0000u);
    }
    H[3] = 0x00450008u;
    H[4] = bswap16(tl);
    H[5] = 0x11400000u;
    H[6] = ipv4_cksum(ipv4_raw(tl, 0u, sq, dq)) | ((sq & 0xFFFFu) << 16);          // :337
    H[7] = (sq >> 16) | ((dq & 0xFFFFu) << 16);
    H[8] = (dq >> 16) | ((ptq & 0xFFFFu) << 16);
    H[9] = (ptq >> 16) | (bswap16(ul) << 16);
    // RFC 768 checksum from the words already here: pseudo-header and UDP header, then the
    // payload dwords masked to [0, L) (the pieces hold whatever follows the payload; the UDP
    // header is at an even datagram offset, so payload dwords are whole 16-bit words of the sum)
    uint32_t ck = 0u;
    if constexpr (CK) {
        uint32_t s = udp_head_sum(sq, dq, ptq, ul);
#pragma unroll
        for (uint32_t d = 0; d < (TX_SMALL_SPAN - 42u + 3u) / 4u; ++d) s = sad16(P[d] & dword_window(0, (int)L, (int)d), s);
        ck = udp_cksum(s);
    }
    // frame dword d: the header for d < 10; then frame byte 42 + t = payload byte t, so dword
    // d >= 10 = payload bytes [4d - 42, 4d - 38) (bytes 40-41: UDP checksum, 0 unless CK)
    auto F = [&](uint32_t d) -> uint32_t {
        return d < 10u ? H[d] : (d == 10u ? (P[0] << 16) | ck : __builtin_amdgcn_alignbyte(P[d - 10u], P[d - 11u], 2));
    };
    // whole 16-byte pieces, then the frame's last 0-15 bytes as dword / byte stores
#pragma unroll
    for (uint32_t c = 0; c < TX_SMALL_SPAN / 16; ++c) {
        if (16u * c + 16u <= span) {
            // (the raw builtin, not store16: the braces fix the order the four words are built in)
            const __attribute__((ext_vector_type(4))) uint32_t v = {F(4 * c), F(4 * c + 1), F(4 * c + 2), F(4 * c + 3)};
            __builtin_amdgcn_raw_buffer_store_b128(v, fw, (int)(fo + 16u * c), 0, 0);
        } else if (16u * c < span) {
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t b = 16u * c + 4u * t;
                if (b + 4u <= span) {
                    __builtin_amdgcn_raw_buffer_store_b32(F(4 * c + t), fw, (int)(fo + b), 0, 0);
                } else if (b < span) {
                    for (uint32_t k = 0; b + k < span; ++k)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(F(4 * c + t) >> (8 * k)), fw, (int)(fo + b + k), 0, 0);
                }
            }
        }
    }
}

} // namespace

// CK: the RFC 768 UDP checksum of every written datagram at bytes 40-41 of its first frame
// (UDPDK_TX_UDP_CKSUM); tx_build<false> leaves them 0 as udpdk_sendto does (:343).
//
// tx_small sums the words in its registers. On the sweep path every chunk adds the one's-
// complement sum of its payload bytes (the window pm) to its datagram's accumulator, and after
// the group's last round the datagram's own lane adds the pseudo-header and UDP header terms and
// patches the two bytes. The accumulator of the datagram in lane q is win[w][q][15]: a header
// window is at most 15 + 42 = 57 bytes, so no header byte ever lies in a row's last dword, and
// the CK build never writes that dword while building headers; LDS stays 20 KiB. l_len bits
// 24-29 carry the frame's datagram lane. Byte lanes: chunks are 16-byte aligned in the output,
// the UDP header starts at frame byte 34, fragment payload offsets and mtu + 14 are even, so
// byte t of a datagram sits in an odd byte of its chunk's 16-bit words exactly when frame_off[i]
// is odd, in every frame of the datagram: the chunk's folded sum is byte-swapped then (RFC 1071
// §2(B)). One wave per group (parts is 1): the patch must follow the sweep's own zeros.
//
// DM: the destination MAC of every frame of datagram i is a.dmac[2 i], a.dmac[2 i + 1]
// (udpdk_gpu_tx_build_neigh) instead of the config's; the argument block is TxNeighArgs then, and
// the forms without it take TxArgs and compile to what they were.
template <bool CK, bool DM>
__global__ void __launch_bounds__(TX_BLOCK) __attribute__((amdgpu_waves_per_eu(6, 8)))
tx_build(TxArgsFor<DM> a)
{
    __shared__ __attribute__((aligned(16))) uint32_t win[TXW][64][TX_WIN / 4];
    // per output frame of the current round
    // (l_len bit 31: 34-byte header, a fragment after the first)
    __shared__ uint32_t l_cs[TXW][64], l_fo[TXW][64], l_len[TXW][64], l_po[TXW][64];
    // (CK: the wave index as a scalar, or the work-item id is kept in a VGPR for it and spilled)
    const uint32_t lane = lane_id();
    const uint32_t w = CK ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : threadIdx.x >> 6;
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(a.payload, a.payload_rsrc);
    const uint32_t waves_total = gridDim.x * TXW;
    const uint32_t fpl = a.mtu ? a.mtu - 20u : 0u;      // IP payload bytes per full fragment
    const uint32_t parts = CK ? 1u : a.parts;

    // a.parts waves share each group of 64 datagrams: every one builds the group's headers and
    // takes every a.parts-th 64 chunks of its sweep (few large datagrams, e.g. 256 K datagrams
    // of 2952 B, are 4096 groups: one wave per group left 4 waves per SIMD, each a long sweep)
    const uint32_t groups = (a.n + 63u) / 64u;
    for (uint32_t gp = blockIdx.x * TXW + w; gp < groups * parts; gp += waves_total) {
        const uint32_t g = gp / parts, part = gp % parts;
        const uint32_t i = g * 64 + lane;
        uint32_t nf = 0, fo = 0, L = 0, po = 0, src = 0, dst = 0, pt = 0;
        int32_t sock = -1;
        uint32_t dm_lo = 0, dm_hi = 0;
        if (i < a.n) {
            fo = a.frame_off[i];
            L = a.payload_len[i];
            po = a.payload_off[i];
            sock = a.sockfd[i];
            if constexpr (DM) {
                const uint2 dm = *reinterpret_cast<const uint2 *>(a.dmac + 2ull * i);
                dm_lo = dm.x;
                dm_hi = dm.y;
            }
        }
        // a wave of small unfragmented frames: one lane builds and stores its own frame
        if (!__ballot(i < a.n && (L + 42u > TX_SMALL_SPAN || (a.mtu && L + 42u > a.mtu)))) {
            if (part == 0u) tx_small<CK, DM>(a, i, fo, L, po, sock, dm_lo, dm_hi);
            continue;
        }
        // this group's accumulators; the first round's wave_sync_tx orders them before any add
        if constexpr (CK) win[w][lane][15] = 0u;
        if (i < a.n) {
            const bool frag = a.mtu && L + 42u > a.mtu;                    // poller.c:466
            const uint32_t n_fr = frag ? (L + 8u + fpl - 1u) / fpl : 1u;
            const uint32_t span = frag ? L + 8u + 34u * n_fr : L + 42u;
            const bool ok = (uint64_t)fo + span <= a.frames_bytes &&
                            (uint64_t)po + L <= a.payload_bytes && sock >= 0 &&
                            (uint32_t)sock < a.n_slots;
            if (ok) {
                nf = n_fr;
                const uint4 sl = a.slots[sock];
                src = (sl.z && sl.x != 0u) ? sl.x : a.src_ip;                   // :329-334
                dst = a.dst_ip[i];                                               // :335
                pt = (sl.y & 0xFFFFu) | ((uint32_t)a.dst_port[i] << 16);          // :341-342
            }
        }
        // per datagram, kept in its lane's registers and read across lanes with shuffles:
        // first frame, frame offset, length | n_frames << 16 (fragmented), payload offset, src
        // ip, dst ip, src port | dst port << 16
        uint32_t n_frames;
        const uint32_t fs = excl_scan64(nf, &n_frames);
        const uint32_t ln = L | ((a.mtu && L + 42u > a.mtu) ? nf << 16 : 0u);

        // no fragmented datagram in the wave: frame = datagram = lane, no shuffles
        const bool direct = !__ballot(nf && (ln >> 16));
        for (uint32_t r0 = 0; r0 < (direct ? 1u : n_frames); r0 += 64) {
            const uint32_t f = r0 + lane;
            uint32_t nch = 0, ffo = 0, plen = 0, ppo = 0, hl = 0;
            uint32_t k = 0, lnq = ln, sq = src, dq = dst, ptq = pt, foq = fo, poq = po;
            uint32_t mlq = dm_lo, mhq = dm_hi;
            bool act = nf != 0;
            uint32_t dl = lane;                   // the frame's datagram lane (CK)
            if (!direct) {
                // the datagram of frame f: the last q with fs[q] <= f (datagrams without frames
                // share their successor's first index); shuffles run with every lane active
                const uint32_t fc = min(f, n_frames - 1u);
                uint32_t q = 0;
#pragma unroll
                for (int sft = 32; sft >= 1; sft >>= 1) {
                    const uint32_t v = __shfl(fs, (int)(q + sft), 64);
                    if (v <= fc) q += sft;
                }
                k = fc - __shfl(fs, (int)q, 64);
                lnq = __shfl(ln, (int)q, 64);
                sq = __shfl(src, (int)q, 64);
                dq = __shfl(dst, (int)q, 64);
                ptq = __shfl(pt, (int)q, 64);
                foq = __shfl(fo, (int)q, 64);
                poq = __shfl(po, (int)q, 64);
                if constexpr (DM) {
                    mlq = __shfl(dm_lo, (int)q, 64);
                    mhq = __shfl(dm_hi, (int)q, 64);
                }
                act = f < n_frames;
                dl = q;
            }
            const uint32_t Lq = lnq & 0xFFFFu, nfq = lnq >> 16;
            if (act) {
                uint32_t tl, ff, ck;
                if (!nfq) {                       // unfragmented: udpdk_sendto's frame as built
                    tl = Lq + 28u;                                               // :336
                    ff = 0u;
                    ck = ipv4_cksum(ipv4_raw(tl, 0u, sq, dq));                   // :337
                    hl = 42u;
                    ffo = foq;
                    ppo = poq;
                    plen = Lq;
                } else {                          // fragment k of nfq (rte_ipv4_fragment_packet)
                    const uint32_t ofs = k * fpl;
                    const bool last = k + 1u == nfq;
                    const uint32_t ipp = last ? Lq + 8u - ofs : fpl;
                    tl = 20u + ipp;
                    ff = (ofs >> 3) | (last ? 0u : 0x2000u);
                    ck = ipv4_cksum_nic(ipv4_raw(tl, ff, sq, dq));
                    hl = k ? 34u : 42u;
                    ffo = foq + k * (a.mtu + 14u);
                    ppo = poq + (k ? ofs - 8u : 0u);
                    plen = k ? ipp : ipp - 8u;
                }
                const uint32_t ul = Lq + 8u;                                     // :344
                uint32_t h[12];
                h[0] = a.mac_lo[0]; h[1] = a.mac_lo[1]; h[2] = a.mac_lo[2];      // :315-317
                if constexpr (DM) {
                    h[0] = mlq;
                    h[1] = (mhq & 0xFFFFu) | (a.mac_lo[1] & 0xFFFF0000u);
                }
                h[3] = 0x00450008u;                                 // type 0x0800, 0x45, tos 0
                h[4] = bswap16(tl);                                 // total length, id 0
                h[5] = bswap16(ff) | 0x11400000u;                   // fragment field, ttl 64, 17
                h[6] = ck | ((sq & 0xFFFFu) << 16);
                h[7] = (sq >> 16) | ((dq & 0xFFFFu) << 16);
                h[8] = (dq >> 16) | ((ptq & 0xFFFFu) << 16);        // src port raw, :341
                h[9] = (ptq >> 16) | (bswap16(ul) << 16);           // dst port raw, :342, :344
                h[10] = 0u;                                         // UDP checksum 0, :343
                h[11] = 0u;
                // shift into the frame's 16-byte alignment: byte r of the header lands at
                // window byte (ffo & 15) + r
                const uint32_t sh = ffo & 15u, s3 = sh & 3u, d0 = sh >> 2;
                uint32_t *wq = win[w][lane];
                // (CK: dword 15 is a datagram's accumulator, and holds no header byte)
#pragma unroll
                for (int t = 0; t < (CK ? 15 : 16); ++t) wq[t] = 0u;
#pragma unroll
                for (int t = 0; t < 12; ++t) {
                    const uint32_t prev = t ? h[t - 1] : 0u;
                    const uint32_t gk = s3 ? ((h[t] << (8u * s3)) | (prev >> (32u - 8u * s3))) : h[t];
                    wq[d0 + t] = gk;
                }
                if (s3 && (!CK || d0 < 3u)) wq[d0 + 12] = h[11] >> (32u - 8u * s3);
                nch = ((ffo & 15u) + hl + plen + 15u) >> 4;
            }
            uint32_t total;
            const uint32_t cs = excl_scan64(nch, &total);
            l_cs[w][lane] = cs;
            l_fo[w][lane] = ffo;
            l_len[w][lane] = plen | (hl == 34u ? 0x80000000u : 0u) | (CK ? dl << 24 : 0u);
            l_po[w][lane] = ppo;
            wave_sync_tx();

            for (uint32_t k = lane + 64u * part; k < total; k += 64u * parts) {
                uint32_t q = 0;
#pragma unroll
                for (int sft = 32; sft >= 1; sft >>= 1)
                    if (l_cs[w][q + sft] <= k) q += sft;
                const uint32_t j = k - l_cs[w][q];
                const uint32_t fq = l_fo[w][q], lw = l_len[w][q], pq = l_po[w][q];
                const uint32_t Lq = lw & (CK ? 0x00FFFFFFu : 0x7FFFFFFFu);
                const int hq = (lw >> 31) ? 34 : 42;
                const uint32_t abase = (fq & ~15u) + 16u * j;
                const int r0c = (int)(abase - fq);
                // header part
                uint32_t H[4] = {0u, 0u, 0u, 0u};
                if (j < 4) {
                    const uint4 hv = *reinterpret_cast<const uint4 *>(&win[w][q][4 * j]);
                    H[0] = hv.x; H[1] = hv.y; H[2] = hv.z; H[3] = hv.w;
                }
                // payload part: bytes at payload offset pq + r0c - hq + b
                uint32_t P[4] = {0u, 0u, 0u, 0u};
                if (r0c + 16 > hq) {
                    const int64_t src0 = (int64_t)pq + r0c - hq;
                    const int64_t sa = src0 & ~(int64_t)15;
                    const uint32_t sft = (uint32_t)(src0 - sa);       // 0..15
                    const uint4 v0 = load16(pr, (uint32_t)sa), v1 = load16(pr, (uint32_t)(sa + 16));
                    const uint32_t wv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    const uint32_t d = sft >> 2, s = sft & 3u;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const uint32_t lo = sel4(d, wv[t], wv[t + 1], wv[t + 2], wv[t + 3]);
                        const uint32_t hi = sel4(d, wv[t + 1], wv[t + 2], wv[t + 3], wv[t + 4]);
                        P[t] = __builtin_amdgcn_alignbyte(hi, lo, s);
                    }
                }
                uint32_t o[4], own[4], psum = 0u;
                bool full = true;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t hm = dword_window(-r0c, hq - r0c, t);
                    const uint32_t pm = dword_window(hq - r0c, hq + (int)Lq - r0c, t);
                    o[t] = (H[t] & hm) | (P[t] & pm);
                    own[t] = hm | pm;
                    full = full && own[t] == 0xFFFFFFFFu;
                    if constexpr (CK) psum = sad16(P[t] & pm, psum);
                }
                if constexpr (CK) {
                    // The chunk's payload bytes, folded, in the datagram's byte lanes. Lanes of
                    // one frame add to one LDS word and the adds serialise; a run-wise reduction
                    // first (DPP prefix sums, one add per run of lanes) was measured slower on
                    // every shape, so the plain add stays.
                    if (psum) {
                        psum = fold32(psum);
                        if (fq & 1u) psum = bswap16(psum);
                        atomicAdd(&win[w][(lw >> 24) & 63u][15], psum);
                    }
                }
                uint8_t *dstp = a.frames + abase;
                if (full) {
                    *reinterpret_cast<uint4 *>(dstp) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (own[t] == 0xFFFFFFFFu) {
                            *reinterpret_cast<uint32_t *>(dstp + 4 * t) = o[t];
                        } else if (own[t]) {
                            for (int b = 0; b < 4; ++b)
                                if ((own[t] >> (8 * b)) & 0xFFu) dstp[4 * t + b] = (uint8_t)(o[t] >> (8 * b));
                        }
                    }
                }
            }
            wave_sync_tx();
        }
        if constexpr (CK) {
            // The datagram's own lane finishes its sum and patches bytes 40-41 of its first
            // frame (fo may be odd: two byte stores). The sweep wrote zeros there; the closing
            // wave_sync_tx of the last round drained this wave's stores and LDS adds before this
            // point, and no other wave writes this group's frames. Skipped datagrams: no patch.
            if (nf) {
                const uint32_t ck = udp_cksum(win[w][lane][15] + udp_head_sum(src, dst, pt, L + 8u));
                a.frames[fo + 40u] = (uint8_t)ck;
                a.frames[fo + 41u] = (uint8_t)(ck >> 8);
            }
        }
    }
}

template __global__ void tx_build<false, false>(TxArgs a);
template __global__ void tx_build<true, false>(TxArgs a);
template __global__ void tx_build<false, true>(TxNeighArgs a);
template __global__ void tx_build<true, true>(TxNeighArgs a);

} // namespace udpdk
