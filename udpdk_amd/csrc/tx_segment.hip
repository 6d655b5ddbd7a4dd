// tx_segment.hip — gfx950 segment plan: K sends, each a payload and a segment size (Linux's
// UDP_SEGMENT), become the descriptor arrays of a udpdk_tx_batch_t with one entry per segment, so
// tx_build cuts every send into its datagrams without a host loop over the datagrams.
//
// Send j of [0, k) has nseg_j segments (udpdk_gpu.h has the definition entry by entry):
//   0                    when it is skipped: sockfd < 0, payload_len > 65507, payload_off +
//                        payload_len > payload_bytes, seg_limit != 0 && nseg > seg_limit, or out of
//                        room, in this order of precedence (no payload byte is read in any case)
//   1                    when gso == 0 or len <= gso (a zero-length send is one empty datagram)
//   ceil(len / gso)      otherwise
// seg_off is the exclusive prefix of nseg, N = seg_off[k]. Segment m = seg_off[j] + t:
//   payload_off[m]  payload_off_j + t * gso, payload_len[m] = min(gso, len_j - t * gso)
//   sockfd[m], dst_ip[m], dst_port[m]   send j's
//   frame_off[m]    base_j + t * span(gso): the exclusive prefix of udpdk_gpu_tx_span(seg_len, mtu)
//                   over the segments, in 64 bits; frame_off[N] = where the output ends
// A send is out of room when its last segment would reach max_segs or its frames would end past
// out_cap, both counted over every send the other rules let through: the two prefixes are monotone,
// so the sends out of room are a tail, and a send is all or nothing. Slots m in [N, max_segs) get
// sockfd -1 and zeros, frame_off[m] the output's end: tx_build over n = max_segs writes nothing for
// them.
//
//   tx_segment_rows    SEG_SEND_TILE sends per workgroup, one per lane: the workgroup's row (output
//                      bytes, segments, frames, sends with segments, the four skip counts)
//   tx_segment_base    one workgroup: exclusive prefixes of the rows' bytes and segments in 64 bits,
//                      the totals, and the one workgroup the room ends in, send by send
//   tx_segment_place   seg_off and each send's first frame offset: the workgroup's bases + a block
//                      scan; the tail out of room gets N
//   tx_segment_expand  SEG_TILE segments per workgroup, one per lane, the grid sized by max_segs:
//                      the descriptors and frame_off of every segment, the padding behind them
// Four launches in stream order: no workgroup waits for another. (seg_off has to be whole before a
// segment can look its send up in it, hence a placement launch between the base and the expansion.)
//
// The send of a segment: the segments are sorted by send, so a wave searches seg_off once for its
// first and once for its last segment (wave-uniform binary searches, lane_find.h; the second one
// in doubling steps up from the first one's send, which is mostly where it ends) and only a wave
// that spans more than two sends with segments searches per lane, between those two.
//
// HBM-bound, in practice launch-bound. Bytes per send, read: 12 (offset, length, segment size,
// sockfd; tx_segment_place and tx_segment_base's one workgroup read them again, L2 hits) + 6
// (address, port) + 8 (seg_off, base; read back by every wave that holds one of its segments, L2
// hits); written: 8 (seg_off, base). Bytes per segment, written: 16 (descriptors) + 4 (frame_off);
// read: none of its own. Floor: 34 B per send + 20 B per segment, 3.4 us for 2^14 sends of 64
// segments at 6.3 TB/s. Bitwise and 32/64-bit integer work only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "lane_find.h"
#include "wave.h"

namespace udpdk {

// udpdk_gpu_tx_span for len <= 65535 and an mtu the host has checked (tx_reply.hip's reply_span)
__device__ __forceinline__ uint32_t seg_span(uint32_t len, uint32_t mtu, uint32_t *n_frames)
{
    uint32_t nf = 1u, span = len + 42u;
    if (mtu && len + 42u > mtu) {
        nf = (len + 8u + (mtu - 20u) - 1u) / (mtu - 20u);
        span = len + 8u + 34u * nf;
    }
    *n_frames = nf;
    return span;
}

// Why a send has no segments before room is looked at: the SEG_R_* field that counts it, 0 = it has
enum { SEG_OK = 0 };

// Send j by the rules that need no prefix: its segment count (0: skipped, *why says which count
// it goes to), output bytes and frames. A send is at most 65507 segments of 43 bytes, or 65507
// bytes in fragments of at least 48: everything fits 32 bits, and so does a workgroup's sum.
__device__ __forceinline__ uint32_t seg_send(const SegArgs &a, uint32_t j, uint32_t *span, uint32_t *frames,
                                             uint32_t *why)
{
    const int32_t sock = a.s_sockfd[j];
    const uint32_t len = a.s_payload_len[j], g = a.s_gso[j], off = a.s_payload_off[j];
    *span = *frames = 0u;
    *why = SEG_OK;
    if (sock < 0) { *why = SEG_R_SKIPPED; return 0u; }
    if (len > 65507u) { *why = SEG_R_TOO_LONG; return 0u; }
    if ((uint64_t)off + len > a.payload_bytes) { *why = SEG_R_BAD_RANGE; return 0u; }
    if (g == 0u || len <= g) {
        *span = seg_span(len, a.mtu, frames);
        return 1u;
    }
    const uint32_t q = len / g, r = len - q * g, nseg = q + (r != 0u);
    if (a.seg_limit && nseg > a.seg_limit) { *why = SEG_R_TOO_MANY; return 0u; }
    uint32_t fq, fr = 0u;
    const uint32_t sq = seg_span(g, a.mtu, &fq), sr = r ? seg_span(r, a.mtu, &fr) : 0u;
    *span = q * sq + sr;
    *frames = q * fq + fr;
    return nseg;
}

// Exclusive prefix of v over the workgroup's SEG_BLOCK lanes (wave scans + the waves' totals in
// LDS; one barrier). wsum: one word per wave.
__device__ __forceinline__ uint32_t seg_block_scan(uint32_t v, uint32_t *wsum)
{
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t wt;
    const uint32_t excl = wave_excl_scan(v, &wt);
    if (lane == 0) wsum[w] = wt;
    __syncthreads();
    uint32_t before = 0u;
    for (uint32_t q = 0; q < w; ++q) before += wsum[q];
    return before + excl;
}

__global__ void __launch_bounds__(SEG_BLOCK)
tx_segment_rows(SegArgs a)
{
    __shared__ uint32_t red[SEG_BLOCK / 64][SEG_ROW];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint64_t j64 = (uint64_t)blockIdx.x * SEG_SEND_TILE + tid;
    const bool valid = j64 < a.k;
    uint32_t span = 0u, nf = 0u, why = SEG_OK, nseg = 0u;
    if (valid) nseg = seg_send(a, (uint32_t)j64, &span, &nf, &why);
    uint32_t v[SEG_ROW];
    v[SEG_R_BYTES] = wave_sum(span);
    v[SEG_R_NSEG] = wave_sum(nseg);
    v[SEG_R_FRAMES] = wave_sum(nf);
    v[SEG_R_OK] = (uint32_t)__popcll(__ballot(nseg != 0u));
#pragma unroll
    for (uint32_t q = SEG_R_SKIPPED; q < SEG_ROW; ++q) v[q] = (uint32_t)__popcll(__ballot(valid && why == q));
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < SEG_ROW; ++q) red[w][q] = v[q];
    }
    __syncthreads();
    if (tid < SEG_ROW) {
        uint32_t s = 0u;
#pragma unroll
        for (uint32_t q = 0; q < SEG_BLOCK / 64; ++q) s += red[q][tid];
        a.row[(size_t)tid * a.n_blocks + blockIdx.x] = s;               // field-major rows
    }
}

// Exclusive prefixes of the rows' output bytes and segments (a contiguous run of rows per lane,
// tx_reply_base's shape: any row count), the totals, and the room: the first row whose sends do not
// all fit is gone through send by send (one per lane), every later row is out of room as a whole.
// One workgroup, so latency-bound: the rows are field-major and the totals come from coalesced
// strided sweeps.
__global__ void __launch_bounds__(SEG_BASE_BLOCK)
tx_segment_base(SegArgs a)
{
    constexpr uint32_t NONE = 0xFFFFFFFFu, NW = SEG_BASE_BLOCK / 64, NT = SEG_ROW - 2u;
    __shared__ unsigned long long pre_b[SEG_BASE_BLOCK], pre_s[SEG_BASE_BLOCK];
    __shared__ unsigned long long fb_b[SEG_BASE_BLOCK], fb_s[SEG_BASE_BLOCK], tot_b, tot_s;
    __shared__ uint32_t wred[NW][NT + 2u];          // frames .. too_many; cut sends, cut frames
    __shared__ uint32_t wsum[2][NW];
    __shared__ uint32_t first_cut, cut_send, part[4];   // part: bytes, segments, sends, frames that fit
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6, nb = a.n_blocks;
    const uint32_t *bytes = a.row + (size_t)SEG_R_BYTES * nb, *segs = a.row + (size_t)SEG_R_NSEG * nb;
    const uint32_t per = (nb + SEG_BASE_BLOCK - 1u) / SEG_BASE_BLOCK;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    // the totals of the six counters
    uint32_t c[NT];
#pragma unroll
    for (uint32_t q = 0; q < NT; ++q) c[q] = 0u;
#pragma unroll 4
    for (uint32_t t = tid; t < nb; t += SEG_BASE_BLOCK) {
#pragma unroll
        for (uint32_t q = 0; q < NT; ++q) c[q] += a.row[(size_t)(2u + q) * nb + t];
    }
    // the lane's run of rows
    unsigned long long sb = 0ull, ss = 0ull;
    for (uint32_t t = b0; t < b1; ++t) {
        sb += bytes[t];
        ss += segs[t];
    }
    pre_b[tid] = sb;
    pre_s[tid] = ss;
    if (tid == 0) {
        first_cut = NONE;
        cut_send = a.k;
        part[0] = part[1] = part[2] = part[3] = 0u;
    }
    __syncthreads();
    unsigned long long bb = 0ull, bs = 0ull;
    for (uint32_t q = 0; q < tid; ++q) {
        bb += pre_b[q];
        bs += pre_s[q];
    }
    uint32_t fc = NONE, cut_ok = 0u, cut_fr = 0u;
    unsigned long long fbb = 0ull, fbs = 0ull;
    for (uint32_t t = b0; t < b1; ++t) {
        const uint32_t vb = bytes[t], vs = segs[t];
        a.base[t] = bb;
        a.base[(size_t)nb + t] = bs;
        if (bb + vb > a.out_cap || bs + vs > a.max_segs) {              // (out of room)
            if (fc == NONE) { fc = t; fbb = bb; fbs = bs; }
            cut_ok += a.row[(size_t)SEG_R_OK * nb + t];
            cut_fr += a.row[(size_t)SEG_R_FRAMES * nb + t];
        }
        bb += vb;
        bs += vs;
    }
    fb_b[tid] = fbb;
    fb_s[tid] = fbs;
    if (fc != NONE) atomicMin(&first_cut, fc);
    if (tid == SEG_BASE_BLOCK - 1) {
        tot_b = bb;
        tot_s = bs;
    }
    uint32_t r8[NT + 2u];
#pragma unroll
    for (uint32_t q = 0; q < NT; ++q) r8[q] = wave_sum(c[q]);
    r8[NT] = wave_sum(cut_ok);
    r8[NT + 1u] = wave_sum(cut_fr);
    if (lane == 0) {
#pragma unroll
        for (uint32_t q = 0; q < NT + 2u; ++q) wred[w][q] = r8[q];
    }
    __syncthreads();                                 // (also: every lane has read pre_b, pre_s)
    const uint32_t pb = first_cut;                   // the row the room ends in, or NONE
    unsigned long long pbb = 0ull, pbs = 0ull;
    if (pb != NONE) {                                // (workgroup-uniform)
        pbb = fb_b[pb / per];                        // rows [q x per, q x per + per) are lane q's
        pbs = fb_s[pb / per];
        const uint64_t j64 = (uint64_t)pb * SEG_SEND_TILE + tid;
        uint32_t span = 0u, nf = 0u, why = SEG_OK, nseg = 0u;
        if (j64 < a.k) nseg = seg_send(a, (uint32_t)j64, &span, &nf, &why);
        const unsigned long long ob = pbb + seg_block_scan(span, wsum[0]);
        const unsigned long long os = pbs + seg_block_scan(nseg, wsum[1]);
        if (nseg) {
            if (ob + span > a.out_cap || os + nseg > a.max_segs) {
                atomicMin(&cut_send, (uint32_t)j64);
            } else {
                atomicAdd(&part[0], span);
                atomicAdd(&part[1], nseg);
                atomicAdd(&part[2], 1u);
                atomicAdd(&part[3], nf);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t g[NT + 2u];
#pragma unroll
        for (uint32_t q = 0; q < NT + 2u; ++q) {
            g[q] = 0u;
#pragma unroll
            for (uint32_t x = 0; x < NW; ++x) g[q] += wred[x][q];
        }
        SegResult r;
        r.bytes_needed = tot_b;
        r.segs_needed = tot_s;
        r.end = tot_b;
        r.segments = (uint32_t)tot_s;                // (<= max_segs when nothing is out of room)
        r.sends = g[SEG_R_OK - 2u];
        r.frames = g[SEG_R_FRAMES - 2u];
        r.no_room = 0u;
        if (pb != NONE) {
            r.end = pbb + part[0];
            r.segments = (uint32_t)pbs + part[1];
            r.no_room = g[NT] - part[2];
            r.sends -= r.no_room;
            r.frames -= g[NT + 1u] - part[3];
        }
        r.skipped = g[SEG_R_SKIPPED - 2u];
        r.too_long = g[SEG_R_TOO_LONG - 2u];
        r.bad_range = g[SEG_R_BAD_RANGE - 2u];
        r.too_many = g[SEG_R_TOO_MANY - 2u];
        r.cut_send = cut_send;
        r.pad = 0u;
        *a.res = r;
    }
}

// seg_off for sends [0, k] (the grid covers k + 1) and the first frame offset of every send with
// room; a send out of room gets N.
__global__ void __launch_bounds__(SEG_BLOCK)
tx_segment_place(SegArgs a)
{
    __shared__ uint32_t wsum[2][SEG_BLOCK / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t j64 = (uint64_t)blockIdx.x * SEG_SEND_TILE + tid;
    const bool valid = j64 < a.k;
    const uint32_t N = a.res->segments, cut = a.res->cut_send;
    uint32_t span = 0u, nf = 0u, why = SEG_OK, nseg = 0u;
    if (valid) nseg = seg_send(a, (uint32_t)j64, &span, &nf, &why);
    const bool row = blockIdx.x < a.n_blocks;
    const unsigned long long ob = (row ? a.base[blockIdx.x] : 0ull) + seg_block_scan(span, wsum[0]);
    const unsigned long long os = (row ? a.base[(size_t)a.n_blocks + blockIdx.x] : 0ull) + seg_block_scan(nseg, wsum[1]);
    if (j64 > a.k) return;
    const bool room = j64 < cut;                     // (the prefixes up to the cut are within the limits)
    a.seg_off[j64] = room ? (uint32_t)os : N;
    if (valid) a.send_base[j64] = room ? (uint32_t)ob : 0u;
}

// The largest j in [lo, hi] with min(seg_off[j], N) <= m (lo when there is none): lane_find.h. A send
// without segments shares its offset with the next one, so the largest is the one that has them.
__device__ __forceinline__ uint32_t seg_find(const SegArgs &a, uint32_t N, uint32_t m, uint32_t lo, uint32_t hi)
{
    return lane_find(a.seg_off, N, m, lo, hi);
}

// seg_find for an m whose send is lo or close behind it (seg_off[lo] <= m): doubling steps up from
// lo, then the bisection inside the last step. A wave's last segment is mostly in its first
// segment's send or the next one: one or two dependent loads where the bisection of [lo, hi] pays
// log2(k) of them.
__device__ __forceinline__ uint32_t seg_find_near(const SegArgs &a, uint32_t N, uint32_t m, uint32_t lo, uint32_t hi)
{
    uint32_t l = lo, step = 1u;
    while (l < hi) {
        const uint32_t probe = hi - l <= step ? hi : l + step;   // (l < probe <= hi)
        if (min(a.seg_off[probe], N) > m) return seg_find(a, N, m, l, probe - 1u);
        l = probe;
        step <<= 1;                                  // (< 2^32: l has moved by step - 1 already)
    }
    return l;
}

// Segment m of [0, max_segs] (the grid covers max_segs + 1): its descriptors and frame_off; the
// slots from N on are padding.
__global__ void __launch_bounds__(SEG_BLOCK)
tx_segment_expand(SegArgs a)
{
    const uint32_t lane = lane_id();
    const uint64_t m64 = (uint64_t)blockIdx.x * SEG_TILE + threadIdx.x;
    const uint32_t N = a.res->segments;
    const uint32_t end = (uint32_t)min(a.res->end, (unsigned long long)a.out_cap);
    const bool in = m64 < N;
    const uint32_t m = (uint32_t)m64;
    // the send: the wave's first and last segments bound it
    uint32_t j = 0u;
    const uint64_t mw = m64 - lane;                              // the wave's first slot
    if (mw < N) {                                                // wave-uniform
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mw);
        const uint32_t m1 = min(m0 + 63u, N - 1u);
        const uint32_t j0 = seg_find(a, N, m0, 0u, a.k - 1u);
        const uint32_t j1 = seg_find_near(a, N, m1, j0, a.k - 1u);
        j = j0;
        if (j1 != j0) {
            const uint32_t o1 = a.seg_off[j1];
            if (a.seg_off[j0 + 1u] == o1) j = m >= o1 ? j1 : j0;     // two sends with segments
            else if (in) j = seg_find(a, N, m, j0, j1);
        }
    }
    uint32_t po = 0u, pl = 0u, ip = 0u, port = 0u, fo = end;
    int32_t sock = -1;
    if (in) {
        const uint32_t t = m - a.seg_off[j], len = a.s_payload_len[j], g = a.s_gso[j];
        uint32_t nf;
        po = a.s_payload_off[j];
        pl = len;
        fo = a.send_base[j];
        if (t) {                                                 // (then g != 0 and len > g)
            po += t * g;
            pl = min(g, len - t * g);
            fo += t * seg_span(g, a.mtu, &nf);
        } else if (g && len > g) {
            pl = g;
        }
        sock = a.s_sockfd[j];
        ip = a.s_dst_ip[j];
        port = a.s_dst_port[j];
    }
    if (m64 > a.max_segs) return;
    a.frame_off[m64] = fo;
    if (m64 == a.max_segs) return;
    a.payload_off[m64] = po;
    a.payload_len[m64] = (uint16_t)pl;
    a.sockfd[m64] = sock;
    a.dst_ip[m64] = ip;
    a.dst_port[m64] = (uint16_t)port;
}

} // namespace udpdk
