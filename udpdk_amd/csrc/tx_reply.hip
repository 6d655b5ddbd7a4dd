// tx_reply.hip — gfx950 reply plan: the lane entries of a finished RX call become the descriptor
// arrays of a udpdk_tx_batch_t whose payload buffer is the RX frame buffer itself, so tx_build
// answers every received datagram (a pingpong server's recvfrom + sendto, apps/pingpong) without
// a payload gather, a PCIe round trip or a host loop.
//
// Entry k of [0, count) is lane entry p = first + k, frame i = lane_pkt[p]:
//   sockfd[k]       the lane p lies in (the answering socket): the largest l < n_lanes with
//                   min(lane_off[l], D) <= p, D = min(lane_off[n_lanes], lane_cap); empty lanes
//                   are thereby passed over. lane_off is an exclusive prefix, so non-decreasing
//                   with lane_off[0] = 0; on anything else the lane is still some index < n_lanes
//   payload_off[k]  offset[i] + 42, payload_len[k] = min(length[i] - 42, (dgram_len - 8) & 0xFFFF)
//                   (rx_gather's rule with an unbounded slot, udpdk_syscall.c:436, :459-466)
//   dst_ip[k], dst_port[k]  frame bytes 26-29 and 34-35, raw (the request's source)
//   frame_off[k]    exclusive prefix of udpdk_gpu_tx_span(payload_len, mtu) over the entries that
//                   answer; frame_off[count] = where the output ends
// An entry does not answer (sockfd -1, every other field 0, no output bytes) when p >= D, i >= n
// (no descriptor or frame byte is read), length[i] < 42, offset[i] + length[i] > frames_bytes, its
// lane is unselected, or its frames would end past out_cap. The prefix is monotone, so the entries
// out of room are a tail of the range; their frame_off is the end of the last entry that fits.
//
//   tx_reply_desc   RPL_TILE entries per workgroup, one per lane: the descriptors, and the
//                   workgroup's row (output bytes, replies, frames, bad indices, unselected)
//   tx_reply_base   one workgroup: exclusive prefix of the rows' bytes in 64 bits, the totals, and
//                   the one workgroup the room ends in, entry by entry
//   tx_reply_place  frame_off = the workgroup's base + a block scan of the spans; the tail out of
//                   room loses its descriptors
// Three launches in stream order: no workgroup waits for another.
//
// The lane of an entry: the entries are sorted by lane, so a wave searches lane_off once for its
// first and once for its last entry (wave-uniform binary searches, <= 14 steps each in a table of
// at most 64 KiB) and only a wave that spans several lanes searches per entry, between those two.
//
// Frame bytes [26, 42) come as in rx_gather: dword-aligned buffer loads from the dword at or below
// offset + 26 (16 bytes, and 4 more when offset & 3 != 0), funnelled by offset & 3 and range-checked
// against frames_bytes rounded up (the tailroom contract of udpdk_gpu.h, unchanged).
//
// HBM-bound. Bytes per entry, read: 4 (lane entry) + 6 (descriptor) + the 64-byte memory request
// that holds the frame's bytes 26-41 (two when they straddle one; a whole 64 B frame); written:
// 16 (descriptors) + 4 (frame_off); tx_reply_place reads back 6 of the 16 (L2 hits for batches of
// up to about a million entries). Floor: 94 B per entry, 15.7 us for 2^20 entries at 6.3 TB/s.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "lane_find.h"
#include "wave.h"

namespace udpdk {

// udpdk_gpu_tx_span for len <= 65535 and an mtu the host has checked (0, or >= 68 with
// (mtu - 20) % 8 == 0): at most 65535 + 8 + 34 x 1366 bytes
__device__ __forceinline__ uint32_t reply_span(uint32_t len, uint32_t mtu, uint32_t *n_frames)
{
    uint32_t nf = 1u, span = len + 42u;
    if (mtu && len + 42u > mtu) {
        nf = (len + 8u + (mtu - 20u) - 1u) / (mtu - 20u);
        span = len + 8u + 34u * nf;
    }
    *n_frames = nf;
    return span;
}

// The largest l in [lo, hi] with min(lane_off[l], D) <= p (lo when there is none): lane_find.h
__device__ __forceinline__ uint32_t reply_lane(const ReplyArgs &a, uint32_t D, uint32_t p, uint32_t lo, uint32_t hi)
{
    return lane_find(a.lane_off, D, p, lo, hi);
}

__global__ void __launch_bounds__(RPL_BLOCK)
tx_reply_desc(ReplyArgs a)
{
    __shared__ uint32_t red[RPL_BLOCK / 64][RPL_ROW];
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint64_t k64 = (uint64_t)blockIdx.x * RPL_TILE + tid;
    const bool valid = k64 < a.count;
    const uint32_t k = (uint32_t)k64;
    const uint32_t D = min(a.lane_off[a.n_lanes], a.lane_cap);
    const uint32_t p = a.first + (valid ? k : 0u);
    const bool in = valid && p < D;
    const uint32_t i = in ? a.lane_pkt[p] : 0xFFFFFFFFu;
    const bool idx_ok = in && i < a.n;
    const uint32_t o = idx_ok ? a.offset[i] : 0u;
    const uint32_t len = idx_ok ? (uint32_t)a.length[i] : 0u;
    const bool frame_ok = idx_ok && len >= 42u && (uint64_t)o + len <= a.frames_bytes;

    // the lane: the wave's first and last entries bound it
    uint32_t l = 0u;
    const uint64_t kw = k64 - lane;                              // the wave's first entry
    if (kw < a.count && a.first + (uint32_t)kw < D) {            // wave-uniform
        const uint32_t k0 = (uint32_t)kw, k1 = min(k0 + 63u, a.count - 1u);
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(a.first + k0));
        const uint32_t p1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(a.first + k1, D - 1u));
        const uint32_t l0 = reply_lane(a, D, p0, 0u, a.n_lanes - 1u);
        const uint32_t l1 = reply_lane(a, D, p1, l0, a.n_lanes - 1u);
        l = l0;
        if (l1 != l0 && in) l = reply_lane(a, D, p, l0, l1);
    }
    const bool sel = !a.lane_sel || !frame_ok || a.lane_sel[l] != 0;
    const bool ok = frame_ok && sel;

    // frame bytes [26, 42): lanes with nothing to read address out of range (no memory access)
    const uint32_t X = o + 26u, sh = X & 3u, A = X & ~3u;
    const uint4 x = load16(fr, ok ? A : 0x80000000u);
    const uint32_t e = load4(fr, ok && sh != 0u ? A + 16u : 0x80000000u);
    const uint32_t src_ip = __builtin_amdgcn_alignbyte(x.y, x.x, sh);        // bytes 26-29
    const uint32_t ports = __builtin_amdgcn_alignbyte(x.w, x.z, sh);         // bytes 34-37
    const uint32_t lens = __builtin_amdgcn_alignbyte(e, x.w, sh);            // bytes 38-41
    const uint32_t pl = (bswap16(lens) - 8u) & 0xFFFFu;          // uint16_t dgram_payl_len (:436)
    const uint32_t plen = ok ? min(len - 42u, pl) : 0u;
    if (valid) {
        a.payload_off[k] = ok ? o + 42u : 0u;
        a.payload_len[k] = (uint16_t)plen;
        a.sockfd[k] = ok ? (int32_t)l : -1;
        a.dst_ip[k] = ok ? src_ip : 0u;
        a.dst_port[k] = ok ? (uint16_t)(ports & 0xFFFFu) : (uint16_t)0;
    }
    uint32_t nf = 0u;
    const uint32_t span = ok ? reply_span(plen, a.mtu, &nf) : 0u;
    if (!ok) nf = 0u;
    const uint32_t s_bytes = wave_sum(span), s_frames = wave_sum(nf);
    const uint32_t s_ok = (uint32_t)__popcll(__ballot(ok));
    const uint32_t s_bad = (uint32_t)__popcll(__ballot(in && !idx_ok));
    const uint32_t s_unsel = (uint32_t)__popcll(__ballot(frame_ok && !sel));
    if (lane == 0) {
        red[w][RPL_R_BYTES] = s_bytes;
        red[w][RPL_R_OK] = s_ok;
        red[w][RPL_R_FRAMES] = s_frames;
        red[w][RPL_R_BADIDX] = s_bad;
        red[w][RPL_R_UNSEL] = s_unsel;
    }
    __syncthreads();
    if (tid < 5u) {
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t j = 0; j < RPL_BLOCK / 64; ++j) v += red[j][tid];
        a.row[(size_t)tid * a.n_blocks + blockIdx.x] = v;               // field-major rows
    }
}

// Exclusive prefix of the rows' output bytes (a contiguous run of rows per lane, rx_filter_base's
// shape: any row count), the totals, and the room: the first row whose entries do not all fit is
// gone through entry by entry (one per lane), every later row is out of room as a whole. One
// workgroup, so latency-bound: the rows are field-major, a lane's run of byte counts is loaded 16
// at a time with every load in flight, and the totals come from coalesced strided sweeps.
__global__ void __launch_bounds__(RPL_BASE_BLOCK)
tx_reply_base(ReplyArgs a)
{
    constexpr uint32_t NONE = 0xFFFFFFFFu, NW = RPL_BASE_BLOCK / 64;
    __shared__ unsigned long long pre[RPL_BASE_BLOCK], fbase[RPL_BASE_BLOCK], total;
    __shared__ uint32_t wred[NW][6];                // replies, frames, bad indices, unselected; cut replies, frames
    __shared__ uint32_t first_cut, part[3];         // part: bytes that fit, replies and frames cut
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, nb = a.n_blocks;
    const uint32_t *bytes = a.row + (size_t)RPL_R_BYTES * nb;
    const uint32_t per = (nb + RPL_BASE_BLOCK - 1u) / RPL_BASE_BLOCK;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    // the totals of the four counters
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll 4
    for (uint32_t t = tid; t < nb; t += RPL_BASE_BLOCK) {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) c[j] += a.row[(size_t)(1u + j) * nb + t];
    }
    // the lane's run of byte counts
    unsigned long long s = 0ull;
    for (uint32_t t0 = b0; t0 < b1; t0 += 16u) {
        uint32_t v[16];
#pragma unroll
        for (uint32_t u = 0; u < 16; ++u) v[u] = t0 + u < b1 ? bytes[t0 + u] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 16; ++u) s += v[u];
    }
    pre[tid] = s;
    if (tid == 0) {
        first_cut = NONE;
        part[0] = part[1] = part[2] = 0u;
    }
    __syncthreads();
    unsigned long long before = 0ull;
    for (uint32_t j = 0; j < tid; ++j) before += pre[j];
    uint32_t fc = NONE, cut_ok = 0u, cut_fr = 0u;
    unsigned long long fb = 0ull;
    for (uint32_t t0 = b0; t0 < b1; t0 += 16u) {
        uint32_t v[16];
#pragma unroll
        for (uint32_t u = 0; u < 16; ++u) v[u] = t0 + u < b1 ? bytes[t0 + u] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 16; ++u) {
            const uint32_t t = t0 + u;
            if (t < b1) {
                a.base[t] = before;
                if (before + v[u] > a.out_cap) {                 // (out of room: rows read one by one)
                    if (fc == NONE) { fc = t; fb = before; }
                    cut_ok += a.row[(size_t)RPL_R_OK * nb + t];
                    cut_fr += a.row[(size_t)RPL_R_FRAMES * nb + t];
                }
                before += v[u];
            }
        }
    }
    fbase[tid] = fb;
    if (fc != NONE) atomicMin(&first_cut, fc);
    if (tid == RPL_BASE_BLOCK - 1) total = before;
    uint32_t r6[6] = {c[0], c[1], c[2], c[3], cut_ok, cut_fr};
#pragma unroll
    for (uint32_t q = 0; q < 6; ++q) r6[q] = wave_sum(r6[q]);
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < 6; ++q) wred[w][q] = r6[q];
    }
    __syncthreads();                                 // (also: every lane has read pre[])
    const uint32_t pb = first_cut;                   // the row the room ends in, or NONE
    unsigned long long pbase = 0ull;
    if (pb != NONE) {
        pbase = fbase[pb / per];                     // rows [j x per, j x per + per) are lane j's
        const uint64_t k64 = (uint64_t)pb * RPL_TILE + tid;
        const bool valid = k64 < a.count;
        const int32_t sock = valid ? a.sockfd[k64] : -1;
        uint32_t nf = 0u;
        const uint32_t span = sock >= 0 ? reply_span(a.payload_len[k64], a.mtu, &nf) : 0u;
        pre[tid] = span;
        __syncthreads();
        unsigned long long off = pbase;
        for (uint32_t j = 0; j < tid; ++j) off += pre[j];
        if (sock >= 0) {
            if (off + span > a.out_cap) {
                atomicAdd(&part[1], 1u);
                atomicAdd(&part[2], nf);
            } else {
                atomicAdd(&part[0], span);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t g[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < NW; ++j) {
#pragma unroll
            for (uint32_t q = 0; q < 6; ++q) g[q] += wred[j][q];
        }
        uint32_t no_room = 0u, frames_cut = 0u;
        unsigned long long end = total;
        if (pb != NONE) {
            no_room = g[4] - a.row[(size_t)RPL_R_OK * nb + pb] + part[1];
            frames_cut = g[5] - a.row[(size_t)RPL_R_FRAMES * nb + pb] + part[2];
            end = pbase + part[0];
        }
        ReplyResult r;
        r.bytes_needed = total;
        r.end = end;
        r.replied = g[0] - no_room;
        r.skipped = a.count - r.replied;
        r.bad_index = g[2];
        r.unselected = g[3];
        r.no_room = no_room;
        r.frames = g[1] - frames_cut;
        *a.res = r;
    }
}

// frame_off for entries [0, count] (the grid covers count + 1); an entry out of room gets the
// output's end and loses its descriptors.
__global__ void __launch_bounds__(RPL_BLOCK)
tx_reply_place(ReplyArgs a)
{
    __shared__ uint32_t wsum[RPL_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint64_t k64 = (uint64_t)blockIdx.x * RPL_TILE + tid;
    const bool valid = k64 < a.count;
    const unsigned long long end = a.res->end;
    const int32_t sock = valid ? a.sockfd[k64] : -1;
    uint32_t nf = 0u;
    const uint32_t span = sock >= 0 ? reply_span(a.payload_len[k64], a.mtu, &nf) : 0u;
    uint32_t wt;
    const uint32_t excl = wave_excl_scan(span, &wt);
    if (lane == 0) wsum[w] = wt;
    __syncthreads();
    unsigned long long off = blockIdx.x < a.n_blocks ? a.base[blockIdx.x] : 0ull;
    for (uint32_t j = 0; j < w; ++j) off += wsum[j];
    off += excl;
    if (k64 == a.count) a.frame_off[k64] = (uint32_t)min(end, (unsigned long long)a.out_cap);
    if (!valid) return;
    a.frame_off[k64] = (uint32_t)min(min(off, end), (unsigned long long)a.out_cap);
    if (sock >= 0 && off + span > a.out_cap) {
        a.payload_off[k64] = 0u;
        a.payload_len[k64] = (uint16_t)0;
        a.sockfd[k64] = -1;
        a.dst_ip[k64] = 0u;
        a.dst_port[k64] = (uint16_t)0;
    }
}

} // namespace udpdk
