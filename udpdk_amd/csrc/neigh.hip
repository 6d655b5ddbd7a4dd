// neigh.hip — gfx950 neighbour cache: a device-resident table of IPv4 next hops and their MACs,
// learned from the ARP frames rx_classify left as UDPDK_V_NOT_IPV4 (neigh_learn) and read, per
// datagram of a TX batch, before tx_build (neigh_resolve). The rules are stated in udpdk_gpu.h
// (udpdk_gpu_neigh_learn, udpdk_gpu_neigh_resolve); the reference has no neighbour cache.
//
// Both kernels have the shape of fanin_stage.h: a sweep by every workgroup that only reads the table,
// and a finish by the launch's last workgroup to arrive, which is the table's one writer. What the
// sweep cannot decide alone (an ARP sender that may be learned,
// a datagram whose next hop has no usable entry) it compacts in order into cand[]; the finisher takes
// those in order, one chunk of a workgroup's width at a time with a barrier between chunks, so the
// table after the call and every count are those of a serial walk. Within a chunk the lanes of one
// key find each other by a scan over the chunk's keys in LDS: the first decides, the last writes.
//
//   neigh_learn    NL_TILE frames per workgroup over meta, arp_reply's frame gate and loads. A batch
//                  without an event ends with the row sums. Bytes per frame: 4 (meta) + 24 / NL_TILE
//                  (row); per candidate + 6 (descriptor) + the 64-byte requests holding bytes 12-41;
//                  per event + 16 written and read, one probe (16 B per slot looked at) and at most
//                  12 B of entry written.
//   neigh_resolve  one datagram per lane. Bytes per datagram: 4 + 4 read, 8 + 4 + 1 written, and one
//                  probe (16 B per slot looked at, from L2: the default table is 16 KiB) unless rules
//                  R1-R4 decide. Per miss + 8 (cand) written and read, a probe and 1 B of state; per
//                  request + 64 (slot) + 4 (origin).
// The finisher is one workgroup: its time grows with the events (misses) of a batch, which are rare by
// design; a batch of nothing but ARP, or of nothing but misses, is served at one workgroup's rate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "neigh.h"
#include "wave.h"
#include "fanin_stage.h"

namespace udpdk {

namespace {

// The slot of key ip, or NEIGH_NONE: linear probing from the key's home slot to the first empty key,
// over the whole table at most. COH: agent-scope loads (the finisher); else plain loads (the sweeps,
// during which nobody writes).
template <bool COH>
__device__ __forceinline__ uint32_t neigh_find(const uint32_t *tab, uint32_t mask, uint32_t shift, uint32_t ip)
{
    uint32_t s = neigh_home(ip, shift);
    for (uint32_t k = 0; k <= mask; ++k, s = (s + 1u) & mask) {
        const uint32_t key = COH ? agent_ld(tab + 4u * s) : tab[4u * s];
        if (key == ip) return s;
        if (key == 0u) return NEIGH_NONE;
    }
    return NEIGH_NONE;
}

// The slot of key ip, claimed when it has none (compare-and-swap on the first empty key of its probe
// sequence; words 1-3 of a slot that was never claimed are zero); NEIGH_NONE when no slot is empty.
__device__ __forceinline__ uint32_t neigh_claim(uint32_t *tab, uint32_t mask, uint32_t shift, uint32_t ip)
{
    uint32_t s = neigh_home(ip, shift);
    for (uint32_t k = 0; k <= mask; ++k, s = (s + 1u) & mask) {
        uint32_t key = agent_ld(tab + 4u * s);
        if (key == 0u) {
            key = atomicCAS(tab + 4u * s, 0u, ip);
            if (key == 0u) return s;
        }
        if (key == ip) return s;
    }
    return NEIGH_NONE;
}

} // namespace

__global__ void __launch_bounds__(NL_BLOCK)
neigh_learn(NeighLearnArgs a)
{
    constexpr int NW = NL_BLOCK / 64;
    __shared__ uint32_t red[NW][NL_ROW];
    __shared__ uint32_t wcnt[NL_ROUNDS][NW];
    __shared__ uint32_t tot[NL_ROW];
    __shared__ uint32_t wsum[NW];
    __shared__ uint32_t ek[NL_BLOCK], em_lo[NL_BLOCK], em_hi[NL_BLOCK], eslot[NL_BLOCK];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t b = blockIdx.x, nb = a.n_blocks;
    const uint64_t f0 = (uint64_t)b * NL_TILE + tid;
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    // the verdict word says who is a candidate: everything below is skipped by a wave without one
    uint32_t m[NL_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < NL_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * NL_BLOCK;
        m[k] = i64 < a.n ? a.meta[i64] : 0xFu;
    }
    uint32_t cnt[NL_ROW] = {0u, 0u, 0u, 0u, 0u, 0u};
    uint4 ent[NL_ROUNDS];
    unsigned long long eb[NL_ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < NL_ROUNDS; ++k) {
        const uint64_t i64 = f0 + (uint64_t)k * NL_BLOCK;
        const uint32_t i = (uint32_t)i64;
        const bool cand = i64 < a.n && UDPDK_META_VERDICT(m[k]) == UDPDK_V_NOT_IPV4;
        bool ev = false;
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
            const uint32_t op = u2 & 0xFFFFu;
            const bool is_arp = fok && (u0 & 0xFFFFu) == 0x0608u;
            const bool hdr_ok = is_arp && (u0 >> 16) == 0x0100u && u1 == 0x04060008u;
            const bool opk = hdr_ok && (op == 0x0100u || op == 0x0200u);
            const bool mbad = (s_lo == a.mac_lo && s_hi == a.mac_hi) || (s_lo & 1u) != 0u || (s_lo | s_hi) == 0u;
            const bool abad = u4 == 0u || u4 == a.src_ip || u4 == 0xFFFFFFFFu || (u4 & 0xF0u) == 0xE0u;
            const bool sbad = opk && (mbad || abad);
            ev = opk && !sbad;
            const uint32_t cr = (op == 0x0100u && tpa == a.src_ip) ? 0x10000u : 0u;
            ent[k] = make_uint4(u4, s_lo, s_hi | cr, i);
            cnt[NL_R_ARP] += (uint32_t)__popcll(__ballot(is_arp));
            cnt[NL_R_MALFORMED] += (uint32_t)__popcll(__ballot(is_arp && !hdr_ok));
            cnt[NL_R_OTHER_OP] += (uint32_t)__popcll(__ballot(hdr_ok && !opk));
            cnt[NL_R_SENDER_BAD] += (uint32_t)__popcll(__ballot(sbad));
            cnt[NL_R_BAD_FRAME] += (uint32_t)__popcll(__ballot(cand && !fok));
            cnt[NL_R_EVENTS] += (uint32_t)__popcll(__ballot(ev));
        }
        eb[k] = __ballot(ev);
        if (lane == 0) wcnt[k][w] = (uint32_t)__popcll(eb[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t f = 0; f < NL_ROW; ++f) red[w][f] = cnt[f];
    }
    __syncthreads();
    // the workgroup's events in frame order: rounds, then waves, then lanes
#pragma unroll
    for (uint32_t k = 0; k < NL_ROUNDS; ++k) {
        if ((eb[k] >> lane) & 1ull) {
            uint32_t rank = (uint32_t)__popcll(eb[k] & ((1ull << lane) - 1ull));
            for (uint32_t j = 0; j < k * NW + w; ++j) rank += wcnt[j / NW][j % NW];
            a.cand[(size_t)b * NL_TILE + rank] = ent[k];
        }
    }
    if (tid < NL_ROW) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        a.row[(size_t)tid * nb + b] = t;                            // field-major rows
    }
    if (!arrive_last<true>(a.fuse, b, nb, &s_last)) return;

    // ---- the launch's last workgroup: the counts, then the events in frame order ----
    row_sums<NL_BLOCK, NL_ROW>(a.row, nb, red, tot);
    const uint32_t n_ev = tot[NL_R_EVENTS];
    if (tid < NL_ROW) a.res->c[tid] = tot[tid];
    if (n_ev == 0u) {                                               // (the whole workgroup)
        if (tid < NL_OUT) a.res->o[tid] = 0u;
        return;
    }
    row_bases<NL_BLOCK>(a.row + (size_t)NL_R_EVENTS * nb, a.rbase, nb, wsum);

    uint32_t oc[NL_OUT] = {0u, 0u, 0u, 0u, 0u, 0u};                 // wave-uniform counts
    for (uint32_t base = 0; base < n_ev; base += NL_BLOCK) {
        const uint32_t r = base + tid;
        const bool valid = r < n_ev;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (valid) {
            uint32_t first;
            const uint32_t g = block_of(a.rbase, nb, r, &first);
            e = a.cand[(size_t)g * NL_TILE + (r - first)];
        }
        const uint32_t ip = e.x, mlo = e.y, mhi = e.z & 0xFFFFu;
        const bool cr = (e.z >> 16) != 0u;
        ek[tid] = ip;                                               // 0 where there is no event: no sender is 0.0.0.0
        em_lo[tid] = mlo;
        em_hi[tid] = e.z;
        eslot[tid] = NEIGH_NONE;
        // the entry as the chunks before this one left it
        uint32_t slot = valid ? neigh_find<true>(a.tab, a.mask, a.shift, ip) : NEIGH_NONE;
        const bool had = slot != NEIGH_NONE;
        uint32_t t_lo = 0u, t_w2 = 0u;
        if (had) {
            t_lo = agent_ld(a.tab + 4u * slot + 1u);
            t_w2 = agent_ld(a.tab + 4u * slot + 2u);
        }
        __syncthreads();
        // this key's events of the chunk: the one before me, whether one follows, and the first that
        // may create (a request for our address)
        uint32_t prev = NEIGH_NONE, fc = NEIGH_NONE;
        bool later = false;
        if (valid) {
            for (uint32_t j = 0; j < tid; ++j) {
                if (ek[j] != ip) continue;
                prev = j;
                if (fc == NEIGH_NONE && (em_hi[j] >> 16)) fc = j;
            }
            if (fc == NEIGH_NONE && cr) fc = tid;
            for (uint32_t j = tid + 1u; j < (uint32_t)NL_BLOCK; ++j) later = later || ek[j] == ip;
            if (!had && fc == tid) eslot[tid] = neigh_claim(a.tab, a.mask, a.shift, ip);
        }
        __syncthreads();
        uint32_t out = NL_OUT;                                      // (none)
        bool wr = false;
        if (valid) {
            const uint32_t t_state = (t_w2 >> 16) & 0xFFu;
            if (had && t_state == UDPDK_NEIGH_STATIC) {
                out = NL_O_STATIC_KEPT;
            } else if (had || (fc != NEIGH_NONE && fc < tid && eslot[fc] != NEIGH_NONE)) {
                // an entry that is there: against the event before me, or the table's
                const bool same = prev != NEIGH_NONE && (had || prev >= fc)
                                      ? (em_lo[prev] == mlo && (em_hi[prev] & 0xFFFFu) == mhi)
                                      : (t_lo == mlo && (t_w2 & 0xFFFFu) == mhi && t_state == UDPDK_NEIGH_REACHABLE);
                out = same ? NL_O_REFRESHED : NL_O_UPDATED;
                if (!had) slot = eslot[fc];
                wr = true;
            } else if (fc == tid) {
                slot = eslot[tid];
                out = slot != NEIGH_NONE ? NL_O_CREATED : NL_O_FULL;
                wr = slot != NEIGH_NONE;
            } else {
                // no entry: never asked for, or the table had no room for the request that came first
                out = (fc != NEIGH_NONE && cr) ? NL_O_FULL : NL_O_IGNORED;
            }
            if (wr && !later) {                                     // the key's last event of the chunk
                agent_st(a.tab + 4u * slot + 1u, mlo);
                agent_st(a.tab + 4u * slot + 2u, mhi | ((uint32_t)UDPDK_NEIGH_REACHABLE << 16));
                agent_st(a.tab + 4u * slot + 3u, a.now);
            }
        }
#pragma unroll
        for (uint32_t f = 0; f < NL_OUT; ++f) oc[f] += (uint32_t)__popcll(__ballot(out == f));
        stores_done();
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t f = 0; f < NL_OUT; ++f) red[w][f] = oc[f];
    }
    __syncthreads();
    if (tid < NL_OUT) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        a.res->o[tid] = t;
    }
}

__global__ void __launch_bounds__(NR_BLOCK)
neigh_resolve(NeighResolveArgs a)
{
    constexpr int NW = NR_BLOCK / 64;
    __shared__ uint32_t red[NW][NR_ROW];
    __shared__ uint32_t tot[NR_ROW];
    __shared__ uint32_t wsum[NW];
    __shared__ uint32_t ek[NR_BLOCK], eres[NR_BLOCK];
    __shared__ uint32_t s_last;
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t b = blockIdx.x, nb = a.n_blocks;
    const uint64_t i64 = (uint64_t)b * NR_TILE + tid;
    const uint32_t i = (uint32_t)i64;
    const bool in = i64 < a.n;
    const uint32_t dst = in ? a.dst_ip[i] : 0u;
    const int32_t sock = in ? a.sockfd[i] : -1;
    uint32_t cls = NR_ROW, hop = 0u, lo = 0u, hi = 0u;
    int32_t so = sock;
    if (in) {
        if (sock < 0) {
            cls = NR_R_SKIPPED;
        } else {
            const uint32_t c = neigh_class(a.src_ip, a.netmask, a.gateway, a.mac_lo, a.mac_hi, dst, &hop, &lo, &hi);
            cls = c == UDPDK_NEIGH_C_BCAST ? NR_R_BCAST : c == UDPDK_NEIGH_C_MCAST ? NR_R_MCAST
                : c == UDPDK_NEIGH_C_NO_ROUTE ? NR_R_NO_ROUTE : c == UDPDK_NEIGH_C_SELF ? NR_R_SELF : NR_R_MISS;
            if (cls == NR_R_NO_ROUTE) so = -1;
            if (cls == NR_R_MISS) {                                 // R5
                const uint32_t slot = neigh_find<false>(a.tab, a.mask, a.shift, hop);
                if (slot != NEIGH_NONE) {
                    const uint4 t = *reinterpret_cast<const uint4 *>(a.tab + 4u * slot);
                    const uint32_t st = (t.z >> 16) & 0xFFu;
                    if (st == UDPDK_NEIGH_STATIC || (st == UDPDK_NEIGH_REACHABLE && a.now - t.w <= a.ttl_ms)) {
                        cls = NR_R_HIT;
                        lo = t.y;
                        hi = t.z & 0xFFFFu;
                    }
                }
                if (cls == NR_R_MISS) {
                    if (a.fallback) { lo = a.fb_lo; hi = a.fb_hi; } else so = -1;
                }
            }
        }
        *reinterpret_cast<uint2 *>(a.dmac + 2ull * i) = make_uint2(lo, hi);
        a.sockfd_out[i] = so;
        // (a miss's class is the finisher's to say)
        if (cls != NR_R_MISS)
            a.state[i] = (uint8_t)(cls == NR_R_SKIPPED ? UDPDK_NEIGH_C_SKIPPED : cls == NR_R_BCAST ? UDPDK_NEIGH_C_BCAST
                                   : cls == NR_R_MCAST ? UDPDK_NEIGH_C_MCAST : cls == NR_R_NO_ROUTE ? UDPDK_NEIGH_C_NO_ROUTE
                                   : cls == NR_R_SELF ? UDPDK_NEIGH_C_SELF : UDPDK_NEIGH_C_HIT);
    }
    uint32_t cnt[NR_ROW];
#pragma unroll
    for (uint32_t f = 0; f < NR_ROW; ++f) cnt[f] = (uint32_t)__popcll(__ballot(cls == f));
    const unsigned long long mb = __ballot(cls == NR_R_MISS);
    if (lane == 0) {
#pragma unroll
        for (uint32_t f = 0; f < NR_ROW; ++f) red[w][f] = cnt[f];
    }
    __syncthreads();
    if (cls == NR_R_MISS) {                                         // in index order: waves, then lanes
        uint32_t rank = (uint32_t)__popcll(mb & ((1ull << lane) - 1ull));
        for (uint32_t j = 0; j < w; ++j) rank += red[j][NR_R_MISS];
        // (written through, like the row: see arrive_last)
        uint32_t *ce = reinterpret_cast<uint32_t *>(a.cand + (size_t)b * NR_TILE + rank);
        agent_st(ce, i);
        agent_st(ce + 1, hop);
    }
    if (tid < NR_ROW) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        agent_st(a.row + (size_t)tid * nb + b, t);
    }
    if (!arrive_last<false>(a.fuse, b, nb, &s_last)) return;

    // ---- the launch's last workgroup: the counts, then the misses in index order ----
    row_sums<NR_BLOCK, NR_ROW>(a.row, nb, red, tot);
    const uint32_t n_miss = tot[NR_R_MISS];
    if (tid < NR_ROW) a.res->c[tid] = tot[tid];
    if (tid == 0) {
        a.res->fallback = a.fallback ? n_miss : 0u;
        a.res->unresolved = a.fallback ? 0u : n_miss;
    }
    if (n_miss == 0u) {                                             // (the whole workgroup)
        if (tid < NR_OUT) a.res->o[tid] = 0u;
        if (tid == 0) a.res->requests = a.res->no_room = 0u;
        return;
    }
    row_bases<NR_BLOCK>(a.row + (size_t)NR_R_MISS * nb, a.rbase, nb, wsum);

    const uint32_t D2 = (a.mac_lo >> 16) | (a.mac_hi << 16);        // our MAC bytes 2-5
    uint32_t oc[NR_OUT] = {0u, 0u, 0u, 0u};                         // wave-uniform counts
    uint32_t asked = 0u;                                            // asking next hops so far (uniform)
    for (uint32_t base = 0; base < n_miss; base += NR_BLOCK) {
        const uint32_t r = base + tid;
        const bool valid = r < n_miss;
        uint2 e = make_uint2(0u, 0u);
        if (valid) {
            uint32_t first;
            const uint32_t g = block_of(a.rbase, nb, r, &first);
            e = a.cand[(size_t)g * NR_TILE + (r - first)];
        }
        const uint32_t h = e.y;
        ek[tid] = h;                                                // 0 where there is no miss: no next hop is 0.0.0.0
        eres[tid] = 0u;
        uint32_t slot = valid ? neigh_find<true>(a.tab, a.mask, a.shift, h) : NEIGH_NONE;
        uint32_t t_w2 = 0u, t_w3 = 0u;
        if (slot != NEIGH_NONE) {
            t_w2 = agent_ld(a.tab + 4u * slot + 2u);
            t_w3 = agent_ld(a.tab + 4u * slot + 3u);
        }
        __syncthreads();
        uint32_t head = tid;
        if (valid) {
            for (uint32_t j = 0; j < tid; ++j)
                if (ek[j] == h) { head = j; break; }
        }
        // the first datagram of a next hop decides for it
        uint32_t out = NR_OUT;                                      // (none)
        bool ask = false;
        if (valid && head == tid) {
            const uint32_t st = (t_w2 >> 16) & 0xFFu;
            if (slot != NEIGH_NONE && st == UDPDK_NEIGH_INCOMPLETE) {
                out = NR_O_INCOMPLETE;
                ask = a.now - t_w3 >= a.retrans_ms;
                if (ask) agent_st(a.tab + 4u * slot + 3u, a.now);
            } else {
                // an expired entry (the MAC stays, for what it is worth), or none yet
                out = slot != NEIGH_NONE ? NR_O_EXPIRED : NR_O_INSERTED;
                if (slot == NEIGH_NONE) slot = neigh_claim(a.tab, a.mask, a.shift, h);
                if (slot == NEIGH_NONE) {
                    out = NR_O_TABLE_FULL;
                } else {
                    ask = true;
                    agent_st(a.tab + 4u * slot + 2u, (t_w2 & 0xFFFFu) | ((uint32_t)UDPDK_NEIGH_INCOMPLETE << 16));
                    agent_st(a.tab + 4u * slot + 3u, a.now);
                }
            }
            eres[tid] = out;
        }
        // the requests of the chunk in index order: waves, then lanes
        const unsigned long long ab = __ballot(ask);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(ab);
        __syncthreads();
        if (valid && head != tid) out = eres[head] == NR_O_TABLE_FULL ? NR_O_TABLE_FULL : NR_O_INCOMPLETE;
        if (valid)
            a.state[e.x] = (uint8_t)(out == NR_O_EXPIRED ? UDPDK_NEIGH_C_EXPIRED : out == NR_O_INCOMPLETE ? UDPDK_NEIGH_C_INCOMPLETE
                                     : out == NR_O_INSERTED ? UDPDK_NEIGH_C_INSERTED : UDPDK_NEIGH_C_TABLE_FULL);
        uint32_t chunk_asks = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) chunk_asks += wsum[j];
        if (ask) {
            uint32_t q = asked + (uint32_t)__popcll(ab & ((1ull << lane) - 1ull));
            for (uint32_t j = 0; j < w; ++j) q += wsum[j];
            if (q < a.req_cap) {
                // ff x 6, our MAC, 08 06 00 01 | 08 00 06 04 00 01, our MAC, our address | target MAC
                // zero, the next hop | zero
                uint4 *p = reinterpret_cast<uint4 *>(a.req + (size_t)q * NEIGH_SLOT);
                p[0] = make_uint4(0xFFFFFFFFu, 0xFFFFu | (a.mac_lo << 16), D2, 0x01000608u);
                p[1] = make_uint4(0x04060008u, 0x0100u | (a.mac_lo << 16), D2, a.src_ip);
                p[2] = make_uint4(0u, h << 16, h >> 16, 0u);
                p[3] = make_uint4(0u, 0u, 0u, 0u);
                a.req_origin[q] = e.x;
            }
        }
        asked += chunk_asks;
#pragma unroll
        for (uint32_t f = 0; f < NR_OUT; ++f) oc[f] += (uint32_t)__popcll(__ballot(out == f));
        stores_done();
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t f = 0; f < NR_OUT; ++f) red[w][f] = oc[f];
    }
    __syncthreads();
    if (tid < NR_OUT) {
        uint32_t t = 0u;
#pragma unroll
        for (int j = 0; j < NW; ++j) t += red[j][tid];
        a.res->o[tid] = t;
    }
    if (tid == 0) {
        a.res->requests = min(asked, a.req_cap);
        a.res->no_room = asked - min(asked, a.req_cap);
    }
}

} // namespace udpdk
