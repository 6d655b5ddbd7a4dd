// arp_reply.hip — gfx950 ARP replies for a finished RX call: the who-has requests (RFC 826) for the
// stack's own address among the frames rx_classify left as UDPDK_V_NOT_IPV4, answered on the device
// from the frames still in the staged buffer. The rules are stated in udpdk_gpu.h
// (udpdk_gpu_arp_reply); the reference has no ARP.
//
//   arp_reply   ARP_TILE frames per workgroup, ARP_ROUNDS rounds of one frame per lane, over meta. A
//               frame whose verdict word does not make it a candidate costs its 4 bytes of meta and
//               nothing else, and a wave without a candidate in a round does nothing more in it. A
//               candidate reads its descriptor and frame bytes [12, 42) (rx_gather's byte-aligned,
//               range-checked loads: two of 16 bytes and one dword) and lands in one counter. The
//               eligible requests of a workgroup are compacted in frame order into cand[] (frame
//               index, sender MAC, sender address: 16 bytes); its row holds the counts.
//               The launch's last workgroup to arrive (fanin_arrive) finishes: it sums the rows into
//               the result, and only when a request is to be answered takes the exclusive prefix of
//               the eligible counts (a run of rows per lane) and writes the replies, four lanes per
//               reply, each one aligned 16-byte store of the 64-byte slot; a reply finds its
//               workgroup by bisection over the runs' bases in LDS, then over the run's rows.
// One launch: no workgroup waits for another, and a batch without a candidate ends with the row sums.
//
// Bytes per frame: 4 (meta) + 36 / ARP_TILE (row). Per candidate: + 6 (descriptor) + the one or two
// 64-byte requests that hold bytes 12-41. Per eligible request: + 16 (entry). Per reply: + 16 (entry
// read) + 64 (slot) + 4 (origin) + the bisection's log2(n / ARP_TILE / 256) dwords from L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "arp_reply.h"
#include "wave.h"
#include "fanin_stage.h"

namespace udpdk {

namespace {

constexpr int NW = ARP_BLOCK / 64;

} // namespace

__global__ void __launch_bounds__(ARP_BLOCK)
arp_reply(ArpArgs a)
{
    __shared__ uint32_t red[NW][ARP_ROW];
    __shared__ uint32_t wcnt[ARP_ROUNDS][NW];
    __shared__ uint32_t tot[ARP_ROW];
    __shared__ uint32_t wsum[NW];
    __shared__ uint32_t pre[ARP_BLOCK];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t b = blockIdx.x, nb = a.n_blocks;
    const uint64_t f0 = (uint64_t)b * ARP_TILE + tid;
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    // the verdict word says who is a candidate: everything below is skipped by a wave without one
    uint32_t m[ARP_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < ARP_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * ARP_BLOCK;
        m[k] = i64 < a.n ? a.meta[i64] : 0xFu;
    }
    uint32_t cnt[ARP_ROW] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    ArpEntry ent[ARP_ROUNDS];
    unsigned long long eb[ARP_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < ARP_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * ARP_BLOCK;
        const uint32_t i = (uint32_t)i64;
        const bool cand = i64 < a.n && UDPDK_META_VERDICT(m[k]) == UDPDK_V_NOT_IPV4;
        bool elig = false;
        ent[k] = make_uint4(0u, 0u, 0u, 0u);
        if (__ballot(cand)) {                                      // wave-uniform
            const uint32_t o = cand ? a.offset[i] : 0u;
            const uint32_t len = cand ? (uint32_t)a.length[i] : 0u;
            const bool fok = cand && len >= 42u && (uint64_t)o + len <= a.frames_bytes;
            // frame bytes [12, 44) as eight dwords; lanes with nothing to read address out of range
            const uint32_t X = o + 12u, sh = X & 3u, A = X & ~3u;
            const uint4 d0 = load16(fr, fok ? A : OOR), d1 = load16(fr, fok ? A + 16u : OOR);
            const uint32_t d2 = load4(fr, fok ? A + 32u : OOR);
            const uint32_t u0 = __builtin_amdgcn_alignbyte(d0.y, d0.x, sh);      // bytes 12-15: type, hardware type
            const uint32_t u1 = __builtin_amdgcn_alignbyte(d0.z, d0.y, sh);      // 16-19: protocol type, lengths
            const uint32_t u2 = __builtin_amdgcn_alignbyte(d0.w, d0.z, sh);      // 20-23: opcode, sender MAC 0-1
            const uint32_t u3 = __builtin_amdgcn_alignbyte(d1.x, d0.w, sh);      // 24-27: sender MAC 2-5
            const uint32_t u4 = __builtin_amdgcn_alignbyte(d1.y, d1.x, sh);      // 28-31: sender address
            const uint32_t u6 = __builtin_amdgcn_alignbyte(d1.w, d1.z, sh);      // 36-39
            const uint32_t u7 = __builtin_amdgcn_alignbyte(d2, d1.w, sh);        // 40-43
            const uint32_t s_lo = (u2 >> 16) | (u3 << 16), s_hi = u3 >> 16;       // bytes 22-25, 26-27
            const uint32_t tpa = (u6 >> 16) | (u7 << 16);                         // bytes 38-41
            const bool is_arp = fok && (u0 & 0xFFFFu) == 0x0608u;
            const bool hdr_ok = is_arp && (u0 >> 16) == 0x0100u && u1 == 0x04060008u;
            const bool req = hdr_ok && (u2 & 0xFFFFu) == 0x0100u;
            const bool own = req && s_lo == a.mac_lo && s_hi == a.mac_hi;
            const bool sbad = req && !own && ((s_lo & 1u) != 0u || (s_lo | s_hi) == 0u);
            const bool ours = req && !own && !sbad && tpa == a.src_ip;
            const bool conf = ours && u4 == a.src_ip;
            elig = ours && !conf;
            ent[k] = make_uint4(i, s_lo, s_hi, u4);
            cnt[ARP_R_ARP] += (uint32_t)__popcll(__ballot(is_arp));
            cnt[ARP_R_MALFORMED] += (uint32_t)__popcll(__ballot(is_arp && !hdr_ok));
            cnt[ARP_R_OTHER_OP] += (uint32_t)__popcll(__ballot(hdr_ok && !req));
            cnt[ARP_R_OWN] += (uint32_t)__popcll(__ballot(own));
            cnt[ARP_R_SENDER_BAD] += (uint32_t)__popcll(__ballot(sbad));
            cnt[ARP_R_NOT_OURS] += (uint32_t)__popcll(__ballot(req && !own && !sbad && !ours));
            cnt[ARP_R_CONFLICT] += (uint32_t)__popcll(__ballot(conf));
            cnt[ARP_R_ELIGIBLE] += (uint32_t)__popcll(__ballot(elig));
            cnt[ARP_R_BAD_FRAME] += (uint32_t)__popcll(__ballot(cand && !fok));
        }
        eb[k] = __ballot(elig);
        if (lane == 0) wcnt[k][w] = (uint32_t)__popcll(eb[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t f = 0; f < ARP_ROW; ++f) red[w][f] = cnt[f];
    }
    __syncthreads();
    // the workgroup's eligible requests in frame order: rounds, then waves, then lanes
#pragma unroll
    for (uint32_t k = 0; k < ARP_ROUNDS; ++k) {
        if ((eb[k] >> lane) & 1ull) {
            uint32_t rank = (uint32_t)__popcll(eb[k] & ((1ull << lane) - 1ull));
            for (uint32_t j = 0; j < k * NW + w; ++j) rank += wcnt[j / NW][j % NW];
            a.cand[(size_t)b * ARP_TILE + rank] = ent[k];
        }
    }
    if (tid < ARP_ROW) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        a.row[(size_t)tid * nb + b] = t;                            // field-major rows
    }
    // the launch's last workgroup finishes: every wave's stores drained, one agent release, the arrival
    stores_done();
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        stores_done();
        unsigned long long fin;
        s_last = fanin_arrive(a.fuse, b, nb, 0ull, &fin) ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    stores_done();
    __syncthreads();

    // the counts
    uint32_t acc[ARP_ROW] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = tid; t < nb; t += ARP_BLOCK) {
#pragma unroll
        for (uint32_t f = 0; f < ARP_ROW; ++f) acc[f] += a.row[(size_t)f * nb + t];
    }
#pragma unroll
    for (uint32_t f = 0; f < ARP_ROW; ++f) {
        const uint32_t s = wave_sum(acc[f]);
        if (lane == 0) red[w][f] = s;
    }
    __syncthreads();
    if (tid < ARP_ROW) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        tot[tid] = t;
    }
    __syncthreads();
    const uint32_t n_elig = tot[ARP_R_ELIGIBLE];
    const uint32_t replies = min(n_elig, a.max_replies);
    if (tid < ARP_ROW) a.res->c[tid] = tot[tid];
    if (tid == 0) {
        a.res->replies = replies;
        a.res->no_room = n_elig - replies;
    }
    if (replies == 0u) return;                                      // (the whole workgroup)

    // eligible requests before each workgroup: a contiguous run of rows per lane
    const uint32_t *r_el = a.row + (size_t)ARP_R_ELIGIBLE * nb;
    const uint32_t per = (nb + ARP_BLOCK - 1u) / ARP_BLOCK;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    uint32_t su = 0u;
    for (uint32_t t = b0; t < b1; ++t) su += r_el[t];
    uint32_t wt;
    uint32_t u = wave_excl_scan(su, &wt);
    if (lane == 0) wsum[w] = wt;
    __syncthreads();
    for (uint32_t j = 0; j < w; ++j) u += wsum[j];
    pre[tid] = u;                                                   // eligible requests before the lane's run
    // (agent-scope accesses: the bisection below reads what other lanes of this workgroup wrote, past
    // the CU's L1)
    if (per > 1u) {
        for (uint32_t t = b0; t < b1; ++t) {
            __hip_atomic_store(&a.rbase[t], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            u += r_el[t];
        }
    }
    stores_done();
    __syncthreads();

    // Reply r is entry r - rbase[g] of the last workgroup g with rbase[g] <= r (those after it with
    // the same base are empty): the last run whose base is <= r by bisection in LDS, then g within
    // the run's `per` rows by bisection over rbase (one row per run up to 256 workgroups: no load).
    // Lane q of a reply's four writes bytes [16 q, 16 q + 16) of the slot; only lanes 0 and 2 carry
    // bytes of the request.
    const uint32_t D2 = (a.mac_lo >> 16) | (a.mac_hi << 16);        // our MAC bytes 2-5
    for (uint64_t idx = tid; idx < 4ull * replies; idx += ARP_BLOCK) {
        const uint32_t r = (uint32_t)(idx >> 2), q = (uint32_t)idx & 3u;
        ArpEntry e = make_uint4(0u, 0u, 0u, 0u);
        if ((q & 1u) == 0u) {
            uint32_t tl = 0u, th = ARP_BLOCK;
            while (th - tl > 1u) {
                const uint32_t mid = (tl + th) >> 1;
                if (pre[mid] <= r) tl = mid; else th = mid;
            }
            uint32_t lo = tl * per, hi = min(nb, lo + per), first = pre[tl];
            while (hi - lo > 1u) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                const uint32_t v = __hip_atomic_load(&a.rbase[mid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v <= r) { lo = mid; first = v; } else hi = mid;
            }
            e = a.cand[(size_t)lo * ARP_TILE + (r - first)];
        }
        uint4 v;
        if (q == 0u)                                                // asker, our MAC, 08 06 00 01
            v = make_uint4(e.y, e.z | (a.mac_lo << 16), D2, 0x01000608u);
        else if (q == 1u)                                           // 08 00 06 04 00 02, our MAC, our address
            v = make_uint4(0x04060008u, 0x0200u | (a.mac_lo << 16), D2, a.src_ip);
        else if (q == 2u)                                           // the asker's MAC and address
            v = make_uint4(e.y, e.z | (e.w << 16), e.w >> 16, 0u);
        else
            v = make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4 *>(a.out + (size_t)r * ARP_SLOT + 16u * q) = v;
        if (q == 0u) a.origin[r] = e.x;
    }
}

} // namespace udpdk
