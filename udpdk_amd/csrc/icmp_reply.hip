// icmp_reply.hip — gfx950 ICMP answers for a finished RX call: echo replies (RFC 792 type 8 -> 0) and
// destination-unreachable / port-unreachable errors (type 3 code 3, RFC 1122 §3.2.2.1, §4.1.3.1), built
// on the device from the verdict words and the frames still in the staged buffer. The rules are
// stated in udpdk_gpu.h (udpdk_gpu_icmp_reply); the reference has no ICMP.
//
//   icmp_scan   ICMP_TILE frames per workgroup, one per lane, over meta. A frame whose verdict word
//               does not make it a candidate costs its 4 bytes of meta and nothing else. A candidate
//               reads its descriptor and frame bytes [14, 42) (rx_gather's byte-aligned, range-checked
//               dword loads), passes the gates, and an echo request has the bytes after its ICMP
//               header summed: up to ICMP_LANE_SUM_MAX bytes by its own lane, a longer message by the
//               whole wave, 16 bytes per lane per step, one candidate after another. The replies of
//               a workgroup are compacted in frame order into cand[]; its row holds the counts.
//   icmp_base   one workgroup: err_limit over the eligible errors in arrival order, then the
//               exclusive prefixes of replies and reply bytes (64 bits) per scan workgroup, the totals.
//   icmp_build  workgroup b takes scan workgroup b's entries (none: it leaves at once): limit,
//               reply rank and offset by block scans, max_replies and out_cap, reply_off / origin,
//               then one wave per reply writes the frame as 16-byte chunks swept across lanes: the
//               42 header bytes from an LDS window laid out with the output's 16-byte alignment, the
//               request's bytes by two aligned 16-byte loads and a funnel shift (tx_build's copy),
//               whole chunks as one 16 B store, boundary chunks byte-masked.
// Three launches in stream order: no workgroup waits for another.
//
// Sums. The request's message is verified and the reply's checksum derived from one sum R over the
// bytes after the 4-byte ICMP header, [38, 14 + tl), as LE 16-bit words with an odd tail zero-padded:
// the request verifies iff fold(R + 0x0008 + its checksum word) == 0xffff; the reply's header words
// are 0, so its checksum is ~fold(R). R is a sum of non-negative terms and fold(x) == 0 only for
// x == 0, so an all-zero reply carries ff ff and one summing to ffff carries 00 00, as the full
// RFC 1071 recomputation gives. Lane loads are 16 bytes at the message's own byte alignment, so a
// 16-bit word of the sum is a 16-bit word of every load.
//
// Bytes per frame: 4 (meta). Per candidate: + 6 (descriptor) + the one or two 64-byte requests that
// hold bytes 14-41. Per echo reply: + the message read twice (sum, copy; the second from L2 for
// anything a workgroup holds) + 16 (entry) + the reply written + 8 (reply_off, origin). Per error:
// 16 + 70 + 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "icmp_reply.h"
#include "wave.h"
#include "fanin_stage.h"
#include "tx_ipv4.h"

namespace udpdk {

namespace {

constexpr int NW = ICMP_BLOCK / 64;

__device__ __forceinline__ uint32_t sel4(uint32_t d, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3)
{
    return d == 0 ? a0 : (d == 1 ? a1 : (d == 2 ? a2 : a3));
}

// Exclusive prefix over the workgroup of three values at once (wave scans + the waves' totals in
// LDS). Every thread of the workgroup calls it.
__device__ __forceinline__ void block_excl_scan3(uint32_t (&v)[3], uint32_t (*wtot)[3], uint32_t w, uint32_t lane)
{
    uint32_t x[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        uint32_t t;
        x[q] = wave_excl_scan(v[q], &t);
        if (lane == 0) wtot[w][q] = t;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        for (uint32_t j = 0; j < w; ++j) x[q] += wtot[j][q];
        v[q] = x[q];
    }
    __syncthreads();
}

} // namespace

__global__ void __launch_bounds__(ICMP_BLOCK)
icmp_scan(IcmpArgs a)
{
    __shared__ uint32_t red[NW][ICMP_ROW];
    __shared__ uint32_t wcnt[NW];
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint64_t i64 = (uint64_t)blockIdx.x * ICMP_TILE + tid;
    const bool valid = i64 < a.n;
    const uint32_t i = (uint32_t)i64;
    // the verdict word says who is a candidate: everything below is skipped by a wave without one
    const uint32_t m = valid ? a.meta[i] : 0xFu;
    const uint32_t v = UDPDK_META_VERDICT(m);
    const bool gate1 = UDPDK_META_IP_OK(m) && !UDPDK_META_IHL_NE5(m);
    const bool c_echo = valid && (a.flags & UDPDK_ICMP_ECHO) && v == UDPDK_V_NOT_UDP && gate1;
    const bool c_unr = valid && (a.flags & UDPDK_ICMP_UNREACH) && (v == UDPDK_V_NO_BIND || v == UDPDK_V_NO_MATCH) &&
                       gate1 && UDPDK_META_UDP_CSUM(m) != UDPDK_UDP_CSUM_BAD && !UDPDK_META_LEN_BAD(m);
    const bool cand = c_echo || c_unr;
    uint32_t s_echo = 0u, s_unr = 0u, s_ebytes = 0u, s_ebad = 0u, s_badf = 0u;
    bool is_reply = false;
    IcmpEntry ent = make_uint4(0u, 0u, 0u, 0u);
    if (__ballot(cand)) {                                          // wave-uniform
        const uint32_t o = cand ? a.offset[i] : 0u;
        const uint32_t len = cand ? (uint32_t)a.length[i] : 0u;
        const bool fok = cand && len >= 42u && (uint64_t)o + len <= a.frames_bytes;
        // frame bytes [14, 42) as seven dwords; lanes with nothing to read address out of range
        const uint32_t X = o + 14u, sh = X & 3u, A = X & ~3u;
        const uint4 d0 = load16(fr, fok ? A : OOR), d1 = load16(fr, fok ? A + 16u : OOR);
        const uint32_t w0 = __builtin_amdgcn_alignbyte(d0.y, d0.x, sh);      // bytes 14-17
        const uint32_t w1 = __builtin_amdgcn_alignbyte(d0.z, d0.y, sh);
        const uint32_t w2 = __builtin_amdgcn_alignbyte(d0.w, d0.z, sh);      // 22-25
        const uint32_t w3 = __builtin_amdgcn_alignbyte(d1.x, d0.w, sh);      // 26-29: source
        const uint32_t w4 = __builtin_amdgcn_alignbyte(d1.y, d1.x, sh);      // 30-33: destination
        const uint32_t w5 = __builtin_amdgcn_alignbyte(d1.z, d1.y, sh);      // 34-37: type, code, checksum
        const uint32_t w6 = __builtin_amdgcn_alignbyte(d1.w, d1.z, sh);      // 38-41
        const uint32_t tl = bswap16(w0 >> 16), proto = (w2 >> 8) & 0xFFu, sb = w3 & 0xFFu;
        const bool gates = fok && w4 == a.src_ip && sb != 0u && sb != 127u && sb < 224u;
        const bool is_echo = c_echo && gates && proto == 1u && (w5 & 0xFFFFu) == 0x0008u;
        const bool lens_ok = is_echo && tl >= 28u && 14u + tl <= len && (a.mtu == 0u || tl <= a.mtu);
        // R: the sum of message bytes [4, tl - 20) = frame bytes [38, 14 + tl)
        const uint32_t S = o + 38u, rl = lens_ok ? tl - 24u : 0u;
        uint32_t R = 0u;
        const bool own = lens_ok && rl <= ICMP_LANE_SUM_MAX;
#pragma unroll
        for (uint32_t k = 0; k < ICMP_LANE_SUM_MAX / 16u; ++k) {
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
        const bool ok_echo = lens_ok && fold32(R + 0x0008u + (w5 >> 16)) == 0xFFFFu;
        const bool elig = c_unr && gates;
        // the error's message: 03 03, checksum, four zeros, then frame bytes [14, 42)
        const uint32_t usum = 0x0303u + sum16(w0) + sum16(w1) + sum16(w2) + sum16(w3) + sum16(w4) + sum16(w5) + sum16(w6);
        is_reply = ok_echo || elig;
        ent.x = i;
        ent.y = ok_echo ? 14u + tl : (ICMP_UNREACH_LEN | ICMP_E_UNREACH);
        ent.z = ~fold32(ok_echo ? R : usum) & 0xFFFFu;
        ent.w = w3;
        s_echo = (uint32_t)__popcll(__ballot(ok_echo));
        s_unr = (uint32_t)__popcll(__ballot(elig));
        s_ebytes = wave_sum(ok_echo ? 14u + tl : 0u);
        s_ebad = (uint32_t)__popcll(__ballot(is_echo && !ok_echo));
        s_badf = (uint32_t)__popcll(__ballot(cand && !fok));
    }
    const unsigned long long rb = __ballot(is_reply);
    if (lane == 0) {
        red[w][ICMP_R_ECHO] = s_echo;
        red[w][ICMP_R_UNR] = s_unr;
        red[w][ICMP_R_EBYTES] = s_ebytes;
        red[w][ICMP_R_EBAD] = s_ebad;
        red[w][ICMP_R_BADF] = s_badf;
        wcnt[w] = (uint32_t)__popcll(rb);
    }
    __syncthreads();
    if (is_reply) {
        uint32_t rank = (uint32_t)__popcll(rb & ((1ull << lane) - 1ull));
        for (uint32_t j = 0; j < w; ++j) rank += wcnt[j];
        a.cand[(size_t)blockIdx.x * ICMP_TILE + rank] = ent;
    }
    row_store<NW, ICMP_ROW>(red, a.row + blockIdx.x, a.n_blocks);
}

// err_limit over the rows' eligible errors in arrival order, then the exclusive prefixes of what is
// left (replies, bytes in 64 bits) and the totals. One workgroup, a contiguous run of rows per lane
// (tx_reply_base's shape: any row count); latency-bound and small: 4096 rows for 2^20 frames.
__global__ void __launch_bounds__(ICMP_BASE_BLOCK)
icmp_base(IcmpArgs a)
{
    __shared__ uint32_t pre_u[ICMP_BASE_BLOCK], pre_r[ICMP_BASE_BLOCK];
    __shared__ unsigned long long pre_b[ICMP_BASE_BLOCK];
    __shared__ uint32_t tot[2];                                    // echo_bad, bad_frame
    const uint32_t tid = threadIdx.x, nb = a.n_blocks;
    const uint32_t per = (nb + ICMP_BASE_BLOCK - 1u) / ICMP_BASE_BLOCK;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    const uint32_t *r_echo = a.row + (size_t)ICMP_R_ECHO * nb, *r_unr = a.row + (size_t)ICMP_R_UNR * nb;
    const uint32_t *r_eb = a.row + (size_t)ICMP_R_EBYTES * nb;
    if (tid < 2u) tot[tid] = 0u;
    uint32_t su = 0u;
    for (uint32_t t = b0; t < b1; ++t) su += r_unr[t];
    pre_u[tid] = su;
    uint32_t c_ebad = 0u, c_badf = 0u;
    for (uint32_t t = tid; t < nb; t += ICMP_BASE_BLOCK) {
        c_ebad += a.row[(size_t)ICMP_R_EBAD * nb + t];
        c_badf += a.row[(size_t)ICMP_R_BADF * nb + t];
    }
    __syncthreads();
    if (c_ebad) atomicAdd(&tot[0], c_ebad);
    if (c_badf) atomicAdd(&tot[1], c_badf);
    uint32_t ub = 0u;
    for (uint32_t j = 0; j < tid; ++j) ub += pre_u[j];
    // the run's replies and bytes once the limit is applied
    uint32_t sr = 0u, u = ub;
    unsigned long long sb = 0ull;
    for (uint32_t t = b0; t < b1; ++t) {
        const uint32_t e = r_unr[t];
        const uint32_t surv = min(e, a.err_limit > u ? a.err_limit - u : 0u);
        a.ubase[t] = u;
        u += e;
        sr += r_echo[t] + surv;
        sb += (unsigned long long)r_eb[t] + (unsigned long long)ICMP_UNREACH_LEN * surv;
    }
    pre_r[tid] = sr;
    pre_b[tid] = sb;
    __syncthreads();
    uint32_t rbef = 0u;
    unsigned long long bbef = 0ull;
    for (uint32_t j = 0; j < tid; ++j) { rbef += pre_r[j]; bbef += pre_b[j]; }
    u = ub;
    for (uint32_t t = b0; t < b1; ++t) {
        const uint32_t e = r_unr[t];
        const uint32_t surv = min(e, a.err_limit > u ? a.err_limit - u : 0u);
        a.rbase[t] = rbef;
        a.bbase[t] = bbef;
        u += e;
        rbef += r_echo[t] + surv;
        bbef += (unsigned long long)r_eb[t] + (unsigned long long)ICMP_UNREACH_LEN * surv;
    }
    if (tid == ICMP_BASE_BLOCK - 1) {                              // (its run is the last: u, bbef are totals)
        IcmpResult r;
        r.bytes_needed = bbef;
        r.echo_replied = 0u;                                       // counted by icmp_build
        r.unreach_sent = 0u;
        r.echo_bad = tot[0];
        r.limited = u - min(u, a.err_limit);
        r.no_room = 0u;
        r.bad_frame = tot[1];
        *a.res = r;
        a.reply_off[0] = 0u;
    }
}

__global__ void __launch_bounds__(ICMP_BLOCK)
icmp_build(IcmpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t win[NW][20];   // 15 + 42 header bytes, read as four chunks
    __shared__ uint32_t s_frame[ICMP_TILE], s_info[ICMP_TILE], s_ck[ICMP_TILE], s_ip[ICMP_TILE], s_off[ICMP_TILE];
    __shared__ uint32_t wtot[NW][3];
    const uint32_t tid = threadIdx.x, lane = lane_id();
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t b = blockIdx.x, nb = a.n_blocks;
    const uint32_t c = a.row[(size_t)ICMP_R_ECHO * nb + b] + a.row[(size_t)ICMP_R_UNR * nb + b];
    if (c == 0u) return;                                            // (the whole workgroup)
    const bool act = tid < c;
    const IcmpEntry e = act ? a.cand[(size_t)b * ICMP_TILE + tid] : make_uint4(0u, 0u, 0u, 0u);
    const bool unr = act && (e.y & ICMP_E_UNREACH);
    const uint32_t len = e.y & ~ICMP_E_UNREACH;
    // the error's rank among the eligible ones, then rank and offset among what the limit leaves
    uint32_t sc[3] = {unr ? 1u : 0u, 0u, 0u};
    block_excl_scan3(sc, wtot, w, lane);
    const bool surv = act && (!unr || a.ubase[b] + sc[0] < a.err_limit);
    sc[1] = surv ? 1u : 0u;
    sc[2] = surv ? len : 0u;                                        // <= 256 x 65535
    block_excl_scan3(sc, wtot, w, lane);
    const uint32_t r = a.rbase[b] + sc[1];
    const unsigned long long off = a.bbase[b] + sc[2];
    const bool wr = surv && r < a.max_replies && off + len <= a.out_cap;
    if (wr) {
        a.reply_off[r + 1u] = (uint32_t)(off + len);                // (reply_off[0]: icmp_base)
        a.origin[r] = e.x;
    }
    s_frame[tid] = e.x;
    s_info[tid] = wr ? e.y : 0u;
    s_ck[tid] = e.z;
    s_ip[tid] = e.w;
    s_off[tid] = (uint32_t)off;
    const uint32_t n_echo = (uint32_t)__popcll(__ballot(wr && !unr));
    const uint32_t n_unr = (uint32_t)__popcll(__ballot(wr && unr));
    const uint32_t n_cut = (uint32_t)__popcll(__ballot(surv && !wr));
    if (lane == 0) {
        if (n_echo) atomicAdd(&a.res->echo_replied, n_echo);
        if (n_unr) atomicAdd(&a.res->unreach_sent, n_unr);
        if (n_cut) atomicAdd(&a.res->no_room, n_cut);
    }
    __syncthreads();

    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    uint8_t *wb = reinterpret_cast<uint8_t *>(win[w]);
    for (uint32_t q = w; q < c; q += NW) {                          // one wave per reply
        const uint32_t info = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_info[q]);
        if (info == 0u) continue;                                   // limited or out of room
        const bool qu = (info & ICMP_E_UNREACH) != 0u;
        const uint32_t L = info & ~ICMP_E_UNREACH;
        const uint32_t fo = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_off[q]);
        const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_ip[q]);
        const uint32_t ck = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_ck[q]);
        const uint32_t o = a.offset[(uint32_t)__builtin_amdgcn_readfirstlane((int)s_frame[q])];
        // reply byte p < hl comes from the header, byte p >= hl is request byte p - delta
        const int hl = qu ? 42 : 38;
        const uint32_t delta = qu ? 28u : 0u;
        const uint32_t tl = L - 14u, src = a.src_ip;
        uint32_t h[11];
        h[0] = a.mac_lo[0]; h[1] = a.mac_lo[1]; h[2] = a.mac_lo[2];
        h[3] = 0x00450008u;                                         // type 0x0800, 0x45, tos 0
        h[4] = bswap16(tl);                                         // total length, id 0
        h[5] = 0x01400000u;                                         // fragment field 0, ttl 64, protocol 1
        h[6] = ipv4_cksum(ipv4_raw(tl, 0u, src, dst, 1u)) | ((src & 0xFFFFu) << 16);
        h[7] = (src >> 16) | ((dst & 0xFFFFu) << 16);
        h[8] = (dst >> 16) | (qu ? 0x03030000u : 0u);               // ICMP type, code
        h[9] = ck;                                                  // checksum; the error's unused bytes
        h[10] = 0u;
        const uint32_t sh = fo & 15u;
        if (lane < 11u) {
            uint32_t hv = h[0];
#pragma unroll
            for (uint32_t t = 1; t < 11; ++t) hv = lane == t ? h[t] : hv;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) wb[sh + 4u * lane + k] = (uint8_t)(hv >> (8u * k));
        }
        wave_sync();
        const uint32_t nch = (sh + L + 15u) >> 4;
        for (uint32_t k = lane; k < nch; k += 64u) {
            const uint32_t abase = (fo & ~15u) + 16u * k;
            const int r0c = (int)(16u * k) - (int)sh;               // reply byte of the chunk's first byte
            uint32_t H[4] = {0u, 0u, 0u, 0u};
            if (k < 4u) {
                const uint4 hv = *reinterpret_cast<const uint4 *>(&win[w][4u * k]);
                H[0] = hv.x; H[1] = hv.y; H[2] = hv.z; H[3] = hv.w;
            }
            uint32_t P[4] = {0u, 0u, 0u, 0u};
            if (r0c + 16 > hl) {
                const int64_t src0 = (int64_t)o + r0c - (int64_t)delta;
                const int64_t sa = src0 & ~(int64_t)15;             // (below 0: out of range, zeros)
                const uint32_t sft = (uint32_t)(src0 - sa);
                const uint4 v0 = load16(fr, (uint32_t)sa), v1 = load16(fr, (uint32_t)(sa + 16));
                const uint32_t wv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                const uint32_t d = sft >> 2, s = sft & 3u;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t lo = sel4(d, wv[t], wv[t + 1], wv[t + 2], wv[t + 3]);
                    const uint32_t hi = sel4(d, wv[t + 1], wv[t + 2], wv[t + 3], wv[t + 4]);
                    P[t] = __builtin_amdgcn_alignbyte(hi, lo, s);
                }
            }
            uint32_t ov[4], ownm[4];
            bool full = true;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t hm = dword_window(-r0c, hl - r0c, t);
                const uint32_t pm = dword_window(hl - r0c, (int)L - r0c, t);
                ov[t] = (H[t] & hm) | (P[t] & pm);
                ownm[t] = hm | pm;
                full = full && ownm[t] == 0xFFFFFFFFu;
            }
            uint8_t *dstp = a.out + abase;
            if (full) {
                *reinterpret_cast<uint4 *>(dstp) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (ownm[t] == 0xFFFFFFFFu) {
                        *reinterpret_cast<uint32_t *>(dstp + 4 * t) = ov[t];
                    } else if (ownm[t]) {
                        for (int bb = 0; bb < 4; ++bb)
                            if ((ownm[t] >> (8 * bb)) & 0xFFu) dstp[4 * t + bb] = (uint8_t)(ov[t] >> (8 * bb));
                    }
                }
            }
        }
        wave_sync();
    }
}

} // namespace udpdk
