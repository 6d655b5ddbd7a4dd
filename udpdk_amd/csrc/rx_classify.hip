// rx_classify.hip — gfx950 RX datapath, first stage: parse + validate + checksums + port demux,
// and the single-lane completion fused into it.
//
// Replaces, for a batch of N frames, N calls of reassemble() (udpdk_poller.c:316-413) from the
// burst loop (udpdk_poller.c:516-545) plus the per-socket rx_buffer appends and ring flushes
// (udpdk_poller.c:274-298). All integer/byte work, bound by HBM:
//
//   rx_classify<G, MR, POL>  one workgroup (4 waves) per tile of T frames, lane = frame, each wave
//       walking 64-frame steps in rounds of 1024 frames. The round's descriptors are staged in
//       LDS; the header window (frame bytes [12, 64), 3 x 16 B + 8 B dword-aligned loads
//       funnelled to frame-relative words) of the next step is in flight while the current one
//       is parsed. Per step: IPv4 gate, fragment / protocol tests, IPv4 header checksum, the UDP
//       checksum of datagrams that end within the window, and, with at most 8 bound ports in
//       the kernel arguments and one-round tiles, the demux (else a demux pass per round: all
//       the round's 16-byte port-table entries in flight at once). Longer datagrams: the step's
//       tail pass (frame bytes >= 64 as 64-byte chunks swept across the wave's lanes, per-frame
//       sums from a DPP prefix scan) or, for steps of back-to-back frames in the long-frame form
//       <2, 0>, the span sweep (the step's bytes read once on a line grid, windows taken from an
//       LDS ring, checksums from prefix sums over the span). Writes the verdict words, the
//       tile's per-lane delivery histogram (tile-major row hist[tile][lane]) and counter row;
//       single-lane calls also write speculative lane entries and, fused, complete the lane in
//       the last workgroup (repairing tiles that were not full). MR = 1: multi-round tiles with
//       the next round's descriptors loaded a round ahead. POL: the cache policy of each stream
//       (rx_common.h; 0 = default policy everywhere, UDPDK_RX_POLICY=0).
//
// The lanes are completed by the kernels of rx_lanes.hip where the fused form is not taken.
//
// Algorithmic bytes per frame in rx_classify: frame_len + 6 (u32 offset + u16 length) + 4
// (verdict word), + 4 per (lane, tile) histogram entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "udpdk_gpu.h"
#include "rx_common.h"
#include "wave.h"
#include "stamps.h"

namespace udpdk {

// ------------------------------------------------------------------------------------------
// Fused single-lane completion (rx_classify with a.fuse): what rx_compact1 does in a second
// launch, done by the last workgroup to finish. Each workgroup, once its written-through stores
// are drained, adds {1 arrival, not-full flag, its deliveries} to its shard's fan-in word
// (a.fuse[16 s], s = tile mod 8, 128 B apart: one word for 1024 arrivals serialises them,
// tools/probe/ticket_probe.hip); the shard's last arrival adds the shard's sums to the top word
// (a.fuse[128]) and the top's last arrival completes the call. Every word is reset by its last
// arrival, so the pipe's next call starts from zeros. When every tile before the last delivered
// all its frames (the common case of a port-bound stream) the speculative entries are the lane
// already and the completion writes lane_off and the total only.
//
// Repair (a tile before the last not full: a stray frame, a drop): every later tile's entries sit
// at tile x T + rank instead of their base + rank. A short tile raises the call's FLAG word
// (before its arrival); every workgroup loads FLAG beside its store drain, so the value costs no
// round trip. The last UDPDK_FIX_HELPERS arrivals of each shard that saw FLAG wait for the call's
// last arrival, which opens the repair (WORK = epoch << 32, then DONE = epoch) and joins it. Each
// participant takes every tile's delivery count (sc1 loads behind an agent acquire), their
// exclusive prefix in LDS, and then chunks of UDPDK_FIX_CHUNK tiles after the first short tile
// from WORK: a full tile's entries are its frame indices in order (stores only), a short tile's
// come from its verdict words. Helpers are optional (a helper that waits past UDPDK_FIX_SPIN
// leaves; the last arrival works through every chunk itself if it must), so the repair is exact
// whoever joins; with helpers it costs a few microseconds instead of a one-workgroup rewrite.
// No workgroup waits unless a tile of its call was short, and at most UDPDK_FIX_HELPERS x 8 wait,
// far fewer than the workgroups resident at once, so no workgroup waits on one that cannot start.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_scan4(uint32_t v, uint32_t *ws, uint32_t lane, uint32_t w,
                                                uint32_t *total)
{
    // exclusive scan over the CLS_WAVES x 64 threads (ws: CLS_WAVES words of LDS)
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63) ws[w] = incl;
    __syncthreads();
    uint32_t pre = incl - v, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < CLS_WAVES; ++i) {
        pre += i < w ? ws[i] : 0u;
        tot += ws[i];
    }
    __syncthreads();
    *total = tot;
    return pre;
}

__device__ __forceinline__ void classify_complete(const RxArgs &a, uint32_t tile, uint32_t tcount,
                                                  uint32_t tid, uint32_t lane, uint32_t w, uint8_t *smem)
{
    __shared__ uint32_t fz[8 + CLS_WAVES];
    const uint32_t T = a.tile_frames;
    const bool nonfull = tile + 1u < a.n_tiles && tcount != T;
    unsigned long long flag = 0;
    if (tid == 0) {
        if (nonfull) atomicMax(&a.fuse[UDPDK_FUSE_FLAG], (unsigned long long)a.spec_epoch);
        flag = __hip_atomic_load(&a.fuse[UDPDK_FUSE_FLAG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    stores_done();                                         // every wave: its stores written through
    __syncthreads();
    if (tid == 0) {
        // payload: {tiles before the last that were not full << 32 | deliveries}
        unsigned long long fin = 0;
        uint32_t left = 0;
        const bool last = fanin_arrive(a.fuse, tile, a.n_tiles, (nonfull ? 1ull << 32 : 0ull) | tcount, &fin, &left);
        fz[0] = last ? 1u : 0u;
        fz[1] = (uint32_t)fin;                              // deliveries of the call
        fz[2] = (uint32_t)(fin >> 32) & 0xFFFFu;            // tiles (not the last) not full
        fz[3] = !last && (uint32_t)flag == a.spec_epoch && left < UDPDK_FIX_HELPERS ? 1u : 0u;
    }
    __syncthreads();
    const bool last = fz[0] != 0u;
    if (last) {
        if (tid == 0) {
            a.lane_off[0] = 0u;
            a.lane_off[1] = fz[1];
            *a.total = fz[1];
            if (fz[2] != 0u) {                             // open the repair
                __hip_atomic_store(&a.fuse[UDPDK_FUSE_WORK], (unsigned long long)a.spec_epoch << 32,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&a.fuse[UDPDK_FUSE_DONE], (unsigned long long)a.spec_epoch,
                                   __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (fz[2] == 0u) return;
    } else {
        if (fz[3] == 0u) return;
        if (tid == 0) {
            uint32_t ok = 0;
            for (uint32_t it = 0; it < UDPDK_FIX_SPIN; ++it) {
                if (__hip_atomic_load(&a.fuse[UDPDK_FUSE_DONE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                    (unsigned long long)a.spec_epoch) {
                    ok = 1u;
                    break;
                }
                __builtin_amdgcn_s_sleep(4);
            }
            fz[4] = ok;
        }
        __syncthreads();
        if (fz[4] == 0u) return;
    }
    // the other workgroups' tile counts and verdict words: one acquire, then sc1 loads
    if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    stores_done();
    __syncthreads();
    const uint32_t nt = a.n_tiles;
    uint32_t *base = reinterpret_cast<uint32_t *>(smem + DSC_OFF);   // [nt + 1] tile bases
    uint32_t *ws = fz + 8;
    {
        // thread tid holds tiles [k0, k0 + per): counts, their exclusive prefix, the first
        // short tile (not the last)
        const __amdgpu_buffer_rsrc_t hr = make_rsrc(a.hist, nt * 4u);
        const uint32_t per = (nt + CLS_BLOCK - 1u) / CLS_BLOCK, k0 = tid * per;
        uint32_t sum = 0, f = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t t = k0 + k;
            const uint32_t c = t < nt ? load4<AUX_SC1>(hr, 4u * t) : 0u;
            if (t < nt) base[t] = c;                        // counts first, prefix below
            if (t + 1u < nt && c != T) f = min(f, t);
            sum += c;
        }
        uint32_t tot;
        uint32_t run = block_scan4(sum, ws, lane, w, &tot);
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t t = k0 + k;
            if (t < nt) {
                const uint32_t c = base[t];
                base[t] = run;
                run += c;
            }
        }
        if (tid == 0) base[nt] = tot;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) f = min(f, (uint32_t)__shfl_xor((int)f, d, 64));
        if (lane == 0) ws[w] = f;
        __syncthreads();
        f = ws[0];
#pragma unroll
        for (uint32_t i = 1; i < CLS_WAVES; ++i) f = min(f, ws[i]);
        __syncthreads();
        if (tid == 0) fz[6] = f;
        __syncthreads();
    }
    const uint32_t first = fz[6];                           // tiles up to it hold their entries
    const __amdgpu_buffer_rsrc_t sr =
        make_rsrc(a.spec_pkt, a.spec_cap >= 0x40000000u ? 0xFFFFFFFCu : a.spec_cap * 4u);
    const __amdgpu_buffer_rsrc_t mr = make_rsrc(a.meta, a.n * 4u);
    for (;;) {
        __syncthreads();                                    // fz[5] of the previous chunk read
        if (tid == 0) {
            const unsigned long long k = __hip_atomic_fetch_add(&a.fuse[UDPDK_FUSE_WORK], 1ull,
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            fz[5] = (uint32_t)(k >> 32) == a.spec_epoch ? (uint32_t)k : 0xFFFFFFFFu;
        }
        __syncthreads();
        const uint32_t k = fz[5];
        if (first == 0xFFFFFFFFu || k == 0xFFFFFFFFu || k >= nt) break;
        const uint32_t ta = first + 1u + k * UDPDK_FIX_CHUNK;
        if (ta >= nt) break;
        const uint32_t tb = min(nt, ta + UDPDK_FIX_CHUNK);
        for (uint32_t t = ta; t < tb; ++t) {
            const uint32_t b = base[t], c = base[t + 1u] - b, f0 = t * T;
            if (c == T) {
                // a full tile: its frames in order (stores only)
                const uint32_t j = 4u * tid, pos = b + j;
                const __attribute__((ext_vector_type(4))) uint32_t x = {f0 + j, f0 + j + 1u, f0 + j + 2u, f0 + j + 3u};
                if ((pos & 3u) == 0u) {
                    __builtin_amdgcn_raw_buffer_store_b128(x, sr, (int)(4u * pos), 0, 0);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i)
                        __builtin_amdgcn_raw_buffer_store_b32(f0 + j + i, sr, (int)(4u * (pos + i)), 0, 0);
                }
            } else {
                // a short (or the last) tile: its delivered frames from its verdict words
                const uint32_t fb = f0 + 4u * tid;
                const auto v = __builtin_amdgcn_raw_buffer_load_b128(mr, (int)(4u * fb), 0, 16);
                uint32_t bits = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
                    if ((v[i] & 0xFu) == UDPDK_V_DELIVERED && fb + i < a.n && 4u * tid + i < T) bits |= 1u << i;
                const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
                uint32_t tot;
                uint32_t pos = b + block_scan4(cnt, ws, lane, w, &tot);
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
                    if ((bits >> i) & 1u) {
                        __builtin_amdgcn_raw_buffer_store_b32(fb + i, sr, (int)(4u * pos), 0, 0);
                        ++pos;
                    }
            }
        }
    }
}

// Frame bytes [12, 64) of one frame: 14 dwords from the dword at or below frame byte 12 (3 x 16 B
// + 8 B; at 64 B frame strides a dword-aligned start costs the same as an aligned one, a byte-
// aligned one ~25 % more, tools/probe/align_probe.hip), funnelled to g[i] = frame bytes 12 + 4i ..
struct Win {
    uint4 a, b, c;
    uint2 d;
};

// 4 waves per SIMD (<= 128 VGPRs, the tail pass's two groups in flight): one tile of 1024 frames
// per workgroup puts 4 workgroups on each CU at 1 M frames. (Round 1: a 96-VGPR budget spilled
// and ran 19 % slower at 64 B; four tail groups in flight at 148 VGPRs and 3 waves per SIMD were
// no faster at 1500 B and slower at IMIX and 106 B. Round 2: three groups at 127 VGPRs, DESIGN.md
// §4.) Round 4: G = tail-pass chunk groups in flight per wave. G = 2 (122 VGPRs, 4 waves per
// SIMD) for batches with long datagrams; G = 1 (92 VGPRs, 5 waves per SIMD, the LDS limit of a
// one-round tile) lets a fifth workgroup per CU in, which is what consecutive short-frame
// batches overlapping on several streams want (config 2, --steps 20, same-box A/B with the
// compaction launch gone: 57.1 -> 63.0 Gpkt/s; config 1 (106 B, one tail chunk per frame) is
// 8 % slower at G = 1, so the host picks G by whether recent calls had tail passes).
template <int G, int MR, int POL>
__global__ void __launch_bounds__(CLS_BLOCK)
__attribute__((amdgpu_waves_per_eu(MR ? 2 : G == 1 ? 5 : UDPDK_CLS_WPE, 8)))
rx_classify(RxArgs a)
{
    static_assert(G == 1 || G == 2, "one or two tail chunk groups in flight");
    // the span sweep (RxArgs::span) is compiled into the long-frame form of one-round tiles only
    constexpr bool SPAN = G == 2 && MR == 0;
    // this form's memory policy: frame-byte loads, descriptor loads, the fused form's stores
    constexpr int PF = pol_frame(G, MR, POL), PD = pol_desc(POL);
    constexpr int PM = pol_meta(POL), PL = pol_lane(POL);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
    const uint32_t steps = a.tile_frames / 64;
    constexpr uint32_t RSTEPS = RX_ROUND / 64;              // steps per staging round
    constexpr uint32_t SPR = RSTEPS / CLS_WAVES;            // steps per wave per staging round
    static_assert(SPR >= 2, "round staging needs two steps per wave per round");
#ifdef UDPDK_STAMPS
    // (in LDS: a register array indexed by lane at the end went to scratch, and the scratch
    // allocation held workgroups back from starting)
    __shared__ unsigned long long st_acc[16];
    unsigned long long st_last = __builtin_amdgcn_s_memtime();
    if (tid < 16) st_acc[tid] = 0;
    if (tid == 0) st_acc[12] = __builtin_amdgcn_s_memrealtime();
#endif

    uint32_t *cntw = reinterpret_cast<uint32_t *>(smem + CNT_OFF);    // [wave][counter]
    // descriptors of the current (and, double-buffered, the next) round of RX_ROUND frames:
    // staged with coalesced loads by the whole workgroup, so the per-step reads are LDS reads
    // (lgkmcnt) and never make a step wait on vector-memory loads it issued for a later step
    const uint32_t nbuf = classify_dsc_bufs(a.tile_frames);
    uint32_t *d_off = reinterpret_cast<uint32_t *>(smem + DSC_OFF);  // [nbuf][RX_ROUND]
    uint32_t *d_lp = d_off + nbuf * RX_ROUND;                        // length | ptype-IPv4 << 16
    uint32_t *hist = d_lp + nbuf * RX_ROUND;                         // [n_lanes] this tile
    // The tile's verdict words are staged in LDS and stored once per tile (16 B per lane): no
    // global store inside the step loop, so no s_waitcnt there ever waits for a store (on gfx9
    // stores count in vmcnt, in order with the loads).
    uint32_t *mstage = hist + classify_hist_words(a.n_lanes, a.hist16 != 0u);   // [stage frames]
    // datagram end (34 + UDP length) of the frames whose checksum the tail pass completes
    // pending frames' datagram end | folded window part of the UDP sum << 16
    uint32_t *dgl = mstage + classify_stage_frames(a.tile_frames);   // [RX_ROUND]
    // the round's port-table lookups: raw dst port | is-UDP << 16, raw dst IPv4
    uint2 *dstash = reinterpret_cast<uint2 *>(dgl + RX_ROUND);       // [RX_ROUND]

    // (hist is only used with several lanes; its zeroing is ordered by the staging barrier)
    // hist16: two lanes per LDS word (lane k in the half k & 1), counts < 2^16 (a tile's
    // deliveries per lane, <= 8192 without fan-out), stored as a u16 row
    const uint32_t hsh = a.hist16 ? 1u : 0u;
    auto hist_add = [&](uint32_t k, uint32_t v) { atomicAdd(&hist[k >> hsh], v << ((k & hsh) << 4)); };
    // Tiles in dispatch order (consecutive tiles on different XCDs). An XCD-contiguous remap
    // (each XCD's L2 streaming one contiguous eighth of the batch) measured 1.7 us slower per
    // 1 M x 64 B launch (tools/probe/stream_probe.hip, feat4).
    const uint32_t tile = blockIdx.x;

    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.rsrc_bytes);
    const uint32_t t0 = tile * a.tile_frames;
    const uint32_t t1 = min(a.n, t0 + a.tile_frames);

    // counters: per-lane packed 8-bit fields (verdicts 0-3 / 4-7, flag counters), deliveries
    // and bytes; reduced across the wave once per tile
    uint32_t acc_v0 = 0, acc_v1 = 0, acc_f0 = 0, acc_f1 = 0, acc_fan = 0, lane_bytes = 0;

    // Loads are unconditional (clamped index / range-checked buffer offsets): a load under a
    // lane condition makes the compiler wait for it at the end of the branch, which would drain
    // the prefetch pipeline every step.
    const uint32_t plast = a.n - 1u;
    // round r's descriptors (frames t0 + RX_ROUND r + [0, RX_ROUND)) into buffer r & 1; the
    // ptype array, when given, only contributes its L3_IPV4 bit (udpdk_poller.c:334)
    // (the ptype word is loaded unconditionally, from the offset array when there is no ptype
    // array, and masked: a load under a condition makes the compiler wait for it in the branch)
    const bool has_ptype = a.ptype != nullptr;
    const uint32_t *ptw = has_ptype ? a.ptype : a.offset;
    constexpr uint32_t SPT = RX_ROUND / CLS_BLOCK;          // descriptors staged per thread
    auto stage_load = [&](uint32_t r, uint32_t (&o)[SPT], uint32_t (&l)[SPT], uint32_t (&t)[SPT]) {
#pragma unroll
        for (uint32_t i = 0; i < SPT; ++i) {
            const uint32_t pc = min(t0 + r * RX_ROUND + i * CLS_BLOCK + tid, plast);
            o[i] = load_pol<PD>(a.offset + pc);
            l[i] = load_pol<PD>(a.length + pc);
            t[i] = load_pol<PD>(ptw + pc);
        }
    };
    auto stage_store = [&](uint32_t r, const uint32_t (&o)[SPT], const uint32_t (&l)[SPT], const uint32_t (&t)[SPT]) {
        const uint32_t b = (r & (nbuf - 1u)) * RX_ROUND;
#pragma unroll
        for (uint32_t i = 0; i < SPT; ++i) {
            d_off[b + i * CLS_BLOCK + tid] = o[i];
            d_lp[b + i * CLS_BLOCK + tid] = l[i] | (has_ptype ? (t[i] & 0x10u) << 12 : 0u);
        }
    };
    auto stage = [&](uint32_t r) {
        uint32_t o[SPT], l[SPT], t[SPT];
        stage_load(r, o, l, t);
        stage_store(r, o, l, t);
    };
    // step s's descriptor for this lane (the index wraps inside the buffers for s >= steps)
    auto read_desc = [&](uint32_t s, uint32_t &o, uint32_t &lp) {
        const uint32_t i = s * 64 + lane;
        const uint32_t b = (((i / RX_ROUND) & (nbuf - 1u)) * RX_ROUND) + (i % RX_ROUND);
        o = d_off[b];
        lp = d_lp[b];
    };
    // The frame's header window, frame bytes [12, 64) (bytes 0-11, the MAC addresses, are never
    // read). One lane per frame, 14 dwords from the dword-aligned buffer offset at or below
    // offset + 12 (byte-aligned 16-byte loads cost the vector memory path ~25 %); the step
    // funnels them to frame-relative words by offset & 3. Bytes past the frame are never used
    // (parse and sums mask by length); lanes without a frame read the buffer's first bytes
    // (cached, never used).
    // (a step that sweeps its span takes its windows from the sweep: nothing loaded here)
    constexpr uint32_t OOR = 0xFFFFFFF0u;   // past any batch's range (< 4 GiB - 16)
    auto load_win = [&](uint32_t s, uint32_t o, uint32_t l, bool swept = false) -> Win {
        const uint32_t p = t0 + s * 64 + lane;
        const bool ok = s < steps && p < t1 && l >= 14u && l <= a.frames_bytes && o <= a.frames_bytes - l;
        const uint32_t b = swept ? OOR : ok ? (o + 12u) & ~3u : 0u;
        Win r;
        r.a = load16<PF>(fr, b);
        r.b = load16<PF>(fr, b + 16u);
        r.c = load16<PF>(fr, b + 32u);
        const auto d = __builtin_amdgcn_raw_buffer_load_b64(fr, (int)(b + 48u), 0, PF);
        r.d = make_uint2(d[0], d[1]);
        return r;
    };

    // Prologue, shortest chain first: the round's descriptor loads go out before anything else,
    // and the first window (step w: frames t0 + tid, this thread's own first descriptor) before
    // the descriptors are staged and the workgroup waits at the barrier. The argument-borne bind
    // table (a vector load from the kernel-argument segment) and the LDS initialisation follow,
    // off that chain (each used to cost a dependent round trip ahead of the descriptor loads).
    __shared__ uint32_t tail_any;           // some wave of the tile ran a tail pass (kernel hint)
    __shared__ uint4 inl_tab[UDPDK_INLINE_PORTS + 1];   // RxArgs::inl entries + a zero slot
    uint32_t st = __builtin_amdgcn_readfirstlane(w);             // wave-uniform step (SGPR)
    uint32_t c_off, c_lp;
    Win W;

    // ---- span sweep (SPAN forms, a.span): is step s's span [A, Ep) sweepable? ----
    // Every frame of the step in range, each starting within SPAN_MAX_GAP bytes after the previous
    // one's end (ascending, disjoint: what a NIC's back-to-back mbuf images are), and on average
    // at least SPAN_MIN_AVG bytes long (shorter frames are all window: the per-frame windows read
    // the same lines). A = the 128-byte line holding the first frame, Ep = the end of the last
    // frame or of the furthest window (windows read 56 bytes from the dword at or below offset +
    // 12). Wave-uniform.
    auto span_check = [&](uint32_t s, uint32_t o, uint32_t l, uint32_t &A, uint32_t &Ep) -> bool {
        if (!SPAN || !a.span || s >= steps) return false;
        const uint32_t p = t0 + s * 64u + lane;
        const bool v = p < t1;
        const unsigned long long vm = __ballot(v);
        if (vm == 0ull) return false;
        const uint32_t on = (uint32_t)__shfl_down((int)o, 1, 64);    // the next frame's offset
        const bool nv = lane < 63u && p + 1u < t1;
        const bool good = l <= a.frames_bytes && o <= a.frames_bytes - l;
        const bool bad = v && (!good || (nv && on - (o + l) >= SPAN_MAX_GAP));
        if (__ballot(bad)) return false;
        const uint32_t ee = v ? max(o + l, ((o + 12u) & ~3u) + 56u) : 0u;
        const uint32_t em = (uint32_t)__builtin_amdgcn_readlane((int)wave_max_scan(ee), 63);
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)o) & ~127u;
        if (em - a0 < SPAN_MIN_AVG * (uint32_t)__popcll(vm)) return false;
        A = a0;
        Ep = em;
        return true;
    };
    bool span_cur = false;                  // the current step sweeps its span (wave-uniform)
    uint32_t span_A = 0, span_E = 0;
    {
        uint32_t o[SPT], l[SPT], t[SPT];
        stage_load(0, o, l, t);
        // (issued before the window: its wait then leaves the window loads in flight)
        const uint4 ie = a.inl_ent[min(tid, UDPDK_INLINE_PORTS - 1u)];
        c_off = o[0];
        c_lp = l[0] | (has_ptype ? (t[0] & 0x10u) << 12 : 0u);
        span_cur = span_check(st, c_off, c_lp & 0xFFFFu, span_A, span_E);
        W = load_win(st, c_off, c_lp & 0xFFFFu, span_cur);
        __builtin_amdgcn_sched_barrier(0);
        const bool inl = a.inl && tid <= UDPDK_INLINE_PORTS;
        if (tid == 0) tail_any = 0u;        // (ordered by the staging barrier)
        if (a.n_lanes > 1u)
            for (uint32_t s = tid; s < ((a.n_lanes + hsh) >> hsh); s += CLS_BLOCK) hist[s] = 0;
        stage_store(0, o, l, t);
        if (inl) inl_tab[tid] = tid < a.n_inl ? ie : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    STAMP(0);

    // ---- tail pass: UDP checksums of the datagrams that extend past the header window ----
    // Run for each step right after it (while the frames' first lines are still in L2: a pass
    // per round of four steps re-fetched the line shared by a frame's header window and its
    // first tail chunk from HBM). The step's pending frames (state 3): the tail's bytes, frame
    // bytes [64, dge) at buffer offsets [S, E) = [offset + 64, offset + dge), as 64-byte
    // super-chunks from the dword-aligned Sa = S & ~3 (chunk j = [Sa + 64 j, Sa + 64 j + 64), 4
    // dword-aligned 16-byte pieces; byte-aligned pieces ran the vector memory path at 4.45
    // instead of 5.9 TB/s, tools/probe/align_probe.hip). The words are then buffer-aligned, not
    // frame-aligned: a frame at an odd offset has its tail sum byte-swapped (RFC 1071 sums are
    // byte-order independent up to that swap), and the first chunk's S - Sa lead bytes (the
    // window's) come off again. The chunks are swept across the wave's lanes: lane i of a group
    // takes chunk k0 + i of the step's chunk space, so a group is 4 KiB of dense frame bytes. A chunk's frame comes from a prefix
    // maximum over the group's lanes of the marks the frames starting inside the group leave in
    // LDS (one LDS round trip; a binary search over the chunk starts took six). Pieces at or past
    // the datagram end are addressed out of the buffer's range (no memory access, zeros); the
    // piece holding the end, when it ends inside it, has its bytes past the end subtracted from
    // the chunk sum, so every chunk is summed the same way (v_sad_u16 chains, no masked re-sum).
    // Per-frame sums are segment sums of a DPP prefix scan; two groups in flight.
    // per frame q of the step: chunk k of q starts at buffer offset B_q + 64 k and holds D_q - 64 k
    // bytes up to the datagram end (B_q = Sa - 64 cs_q, D_q = E - Sa + 64 cs_q, cs_q = the frame's
    // first chunk index in the step), so a chunk needs two LDS words of its frame (B_q's low two
    // bits carry the lead S - Sa)
    uint32_t *l_B = reinterpret_cast<uint32_t *>(smem + TP_OFF) + w * 192;   // [64]
    uint32_t *l_D = l_B + 64;                                               // [64]
    uint32_t *l_own = l_B + 128;            // [64] frame + 1 whose chunks start at k0 + slot, else 0
    l_own[lane] = 0;
    bool tailed = false;                    // this wave ran a tail pass (the host's kernel hint)
    auto tail_step = [&](uint32_t s2) {
            const uint32_t i = s2 * 64 + lane;
            const uint32_t m = mstage[i & (RX_ROUND - 1u)];
            const bool pd = t0 + i < t1 && ((m >> 5) & 3u) == 3u;
            if (!__ballot(pd)) return;
            // the frame's offset: the staged descriptor of a single-round tile, else global
            const uint32_t fo = nbuf == 1u ? d_off[i] : a.offset[min(t0 + i, plast)];
            const uint32_t dw = dgl[i & (RX_ROUND - 1u)];
            const uint32_t de = pd ? dw & 0xFFFFu : 64u;
            const uint32_t lead = (fo + 64u) & 3u;
            const uint32_t my_nt = pd ? (de - 64u + lead + 63u) >> 6 : 0u;
            const uint32_t inc = wave_incl_scan(my_nt);
            const uint32_t my_cs = inc - my_nt;
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            l_B[lane] = (fo + 64u - lead - 64u * my_cs) | lead;
            l_D[lane] = de - 64u + lead + 64u * my_cs;
            uint32_t tsum = 0, carry = 0;
            // group k0: each lane's frame (q), the chunk's bytes in the datagram (left) and its
            // four pieces in flight
            auto issue = [&](uint32_t k0, uint32_t &q, int &left, uint32_t &lead_b, uint4 (&R)[4]) {
                const uint32_t k = k0 + lane;
                if (my_nt != 0u && my_cs >= k0 && my_cs < k0 + 64u) l_own[my_cs - k0] = lane + 1u;
                wave_sync();
                const uint32_t mark = l_own[lane];
                l_own[lane] = 0u;                       // cleared for the next group (in order)
                const uint32_t own = max(wave_max_scan(mark), carry);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)own, 63);
                q = (own - 1u) & 63u;
                left = k < total ? (int)(l_D[q] - 64u * k) : 0;
                const uint32_t bq = l_B[q];
                lead_b = mark != 0u ? bq & 3u : 0u;     // a frame's first chunk: its lead bytes
                const uint32_t base = (bq & ~3u) + 64u * k;
#pragma unroll
                for (int c = 0; c < 4; ++c) R[c] = load16<PF>(fr, 16 * c < left ? base + 16u * c : OOR);
            };
            // The full-chunk sum reads every loaded register unconditionally, so the compiler's
            // wait for this group is placed here on every path.
            auto consume = [&](uint32_t k0, int left, uint32_t lead_b, const uint4 (&R)[4]) {
                uint32_t pa = 0, pb = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    pa = sad16(R[c].x, pa);
                    pb = sad16(R[c].y, pb);
                    pa = sad16(R[c].z, pa);
                    pb = sad16(R[c].w, pb);
                }
                // the piece holding the datagram end, if the end falls inside it: its bytes
                // [r, 16) are the next frame's (or padding) and come off again
                const int r = left & 15;
                const uint32_t pc = (uint32_t)left >> 4;
                const uint4 P = pc == 0u ? R[0] : pc == 1u ? R[1] : pc == 2u ? R[2] : R[3];
                const uint32_t pv[4] = {P.x, P.y, P.z, P.w};
                uint32_t ex = 0;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int keep = min(max(r - 4 * d, 0), 4);
                    ex = sad16(pv[d] & (keep >= 4 ? 0u : 0xFFFFFFFFu << (8 * keep)), ex);
                }
                // and the first chunk's lead bytes [0, lead_b) (<= 3: in the first dword)
                ex = sad16(R[0].x & ((1u << (8u * lead_b)) - 1u), ex & (left > 0 && left < 64 && r != 0 ? ~0u : 0u));
                const uint32_t part = pa + pb - ex;
                const uint32_t Pp = wave_incl_scan(part);
                const uint32_t lo = max(my_cs, k0), hi = min(my_cs + my_nt, k0 + 64u);
                const uint32_t ph = __shfl(Pp, (int)((hi > k0 ? hi - 1u - k0 : 0u) & 63u), 64);
                const uint32_t pl = __shfl(Pp, (int)((lo > k0 ? lo - 1u - k0 : 0u) & 63u), 64);
                if (lo < hi) tsum += ph - (lo > k0 ? pl : 0u);
            };
            // Two groups in flight; one back edge, after the second group is consumed (a loop
            // exit between the two halves leaves the second group's loads pending at the
            // header, which then waits for everything). Groups past the end load nothing.
            uint32_t qa, qb, ea, eb;
            int la, lb;
            uint4 Ra[4], Rb[4];
            issue(0, qa, la, ea, Ra);
            tailed = true;
            if constexpr (G == 1) {
                // one group in flight: the next group's loads are issued after this one is summed
                for (uint32_t k0 = 0;; k0 += 64) {
                    consume(k0, la, ea, Ra);
                    if (k0 + 64 >= total) break;
                    issue(k0 + 64, qa, la, ea, Ra);
                }
                (void)qb; (void)lb; (void)eb; (void)Rb;
            } else if (total <= 64u) {
                // one group (e.g. every frame's tail one chunk): no groups issued past the end
                consume(0, la, ea, Ra);
            } else {
                for (uint32_t k0 = 0;; k0 += 128) {
                    issue(k0 + 64, qb, lb, eb, Rb);
                    consume(k0, la, ea, Ra);
                    issue(k0 + 128, qa, la, ea, Ra);
                    consume(k0 + 64, lb, eb, Rb);
                    if (k0 + 128 >= total) break;
                }
            }
            wave_sync();
            if (pd) {
                uint32_t t = fold32(tsum);
                // buffer-aligned words: swap back (t < 2^16: bswap16's second mask is an instruction more)
                if (fo & 1u) t = ((t & 0xFFu) << 8) | (t >> 8);
                const bool ok = fold32(t + (dw >> 16)) == 0xFFFFu;
                mstage[i & (RX_ROUND - 1u)] = (m & ~0x60u) | ((ok ? UDPDK_UDP_CSUM_OK : UDPDK_UDP_CSUM_BAD) << 5);
                acc_f0 += ok ? 0x10000u : 0x1000000u;
            }
    };

    // ---- span sweep: the step's bytes [A, Ep) read once, each 128-byte line by one load ----
    // (tools/probe/sweep_probe.hip: loads that each cover 1 KiB of consecutive 16-byte pieces read
    // 1.004x the span's bytes from HBM; one 64-byte chunk per lane, 1.030x; the per-frame windows
    // and tail chunks, 1.13x.) Blocks of 64 pieces, four per group, two groups in flight. Per
    // block: the pieces' RFC 1071 sums (buffer-aligned words, whole pieces) and their prefix sum
    // on the DPP network give Q(k), the sum of pieces [0, k) of the span, at each frame's two
    // piece indices (the piece holding its tail start, offset + 64, and the first piece past its
    // end); the block goes to a two-block LDS ring, from which a frame takes its header window
    // (the same 14 dwords load_win reads) when the block holding its last window byte arrives,
    // and the piece holding its end. Then a frame's tail sum over [offset + 64, offset + length)
    // = Q(end) - Q(start) - the lead bytes of the start piece (in its window) - the bytes of the
    // end piece past the frame (span_tail). Sums of 16-bit words up to 65535 bytes stay below
    // 2^32, so the differences of the wrapping prefix sums are exact.
    uint32_t *ring = reinterpret_cast<uint32_t *>(
        smem + classify_lds_bytes(a.n_lanes, a.tile_frames, a.hist16 != 0u)) + w * SPAN_RING_DW;
    uint32_t sp_Qs = 0, sp_Qe = 0;          // Q at the frame's tail-start piece and past its end
    uint4 sp_EP = make_uint4(0, 0, 0, 0);   // the piece holding the frame's end
    auto span_sweep = [&](uint32_t s, uint32_t A, uint32_t Ep, uint32_t o, uint32_t l) -> Win {
        const bool v = t0 + s * 64u + lane < t1;
        const uint32_t w0 = (o + 12u) & ~3u;
        const uint32_t s_idx = v ? (o + 64u - A) >> 4 : 0u;
        const uint32_t e_idx = v ? (o + l - A + 15u) >> 4 : 0u;
        const uint32_t wblk = v ? (w0 + 52u - A) >> 10 : 0xFFFFFFFFu;
        const uint32_t eblk = v && l > 64u && ((o + l) & 15u) != 0u ? (o + l - A) >> 10 : 0xFFFFFFFFu;
        const uint32_t ep = ((o + l - A) >> 4) & 127u;     // ring piece of the frame's end
        const uint32_t rb = ((w0 - A) >> 2) & 511u;         // ring dword of the window's first
        const uint32_t nb = (Ep - A + 1023u) >> 10;          // blocks
        const uint32_t ng = (nb + 3u) >> 2;                  // groups
        uint32_t C = 0, Qs = 0, Qe = 0;
        uint32_t Dw[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) Dw[k] = 0;
        uint4 EP = make_uint4(0, 0, 0, 0);
        uint4 *rq = reinterpret_cast<uint4 *>(ring);
        auto block = [&](uint32_t b, const uint4 &R) {
            const uint32_t ps = sad16(R.x, sad16(R.z, 0u)) + sad16(R.y, sad16(R.w, 0u));
            const uint32_t P = wave_incl_scan(ps);
            const uint32_t ds = s_idx - 64u * b - 1u, de = e_idx - 64u * b - 1u;
            const uint32_t Ps = (uint32_t)__shfl((int)P, (int)(ds & 63u), 64);
            const uint32_t Pe = (uint32_t)__shfl((int)P, (int)(de & 63u), 64);
            Qs = ds < 64u ? C + Ps : Qs;
            Qe = de < 64u ? C + Pe : Qe;
            C += (uint32_t)__builtin_amdgcn_readlane((int)P, 63);
            wave_sync();                                     // the previous block's ring reads first
            rq[(b & 1u) * 64u + lane] = R;
            if ((b & 1u) == 0u && lane < 4u) rq[128u + lane] = R;
            wave_sync();
            if (__ballot(wblk == b)) {
                if (wblk == b) {
#pragma unroll
                    for (int k = 0; k < 14; ++k) Dw[k] = ring[rb + k];
                }
            }
            if (__ballot(eblk == b)) {
                if (eblk == b) EP = rq[ep];
            }
        };
        auto issue = [&](uint32_t g, uint4 (&R)[4]) {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                const uint32_t x = A + 4096u * g + 1024u * c + 16u * lane;
                R[c] = load16<PF>(fr, x < Ep ? x : OOR);
            }
        };
        auto consume = [&](uint32_t g, const uint4 (&R)[4]) {
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c)
                if (4u * g + c < nb) block(4u * g + c, R[c]);
        };
        uint4 Ra[4], Rb[4];
        issue(0, Ra);
        for (uint32_t g = 0;; g += 2) {
            issue(g + 1u, Rb);
            consume(g, Ra);
            issue(g + 2u, Ra);
            consume(g + 1u, Rb);
            if (g + 2u >= ng) break;
        }
        sp_Qs = Qs;
        sp_Qe = Qe;
        sp_EP = EP;
        Win r;
        r.a = make_uint4(Dw[0], Dw[1], Dw[2], Dw[3]);
        r.b = make_uint4(Dw[4], Dw[5], Dw[6], Dw[7]);
        r.c = make_uint4(Dw[8], Dw[9], Dw[10], Dw[11]);
        r.d = make_uint2(Dw[12], Dw[13]);
        return r;
    };
    // the swept frame's tail sum over buffer bytes [o + 64, o + l) (buffer-aligned 16-bit words):
    // D = the window's raw dwords (buffer dwords from w0 = (o + 12) & ~3)
    auto span_tail = [&](uint32_t o, uint32_t l, const uint32_t (&D)[14]) -> uint32_t {
        const int hi = (int)(o + 64u - ((o + 12u) & ~3u)), lo = hi - (int)((o + 64u) & 15u);
        uint32_t lead = 0;
#pragma unroll
        for (int k = 9; k < 14; ++k) lead = sad16(D[k] & dword_window(lo, hi, k), lead);
        const int r = (int)((o + l) & 15u);
        const uint32_t ev[4] = {sp_EP.x, sp_EP.y, sp_EP.z, sp_EP.w};
        uint32_t over = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d) over = sad16(ev[d] & dword_window(r, 16, d), over);
        return sp_Qe - sp_Qs - lead - (r != 0 ? over : 0u);
    };

    // ---- demux of one frame: btable_get_bindings + list walk, udpdk_poller.c:376-405 ----
    // i: the frame's index in the tile, m: its verdict word so far (verdict field 0xF: UDP, port
    // lookup pending), Sv: {raw dst port | is-UDP << 16, raw dst IPv4}, Ev: the port's 16-byte
    // entry (first binding inline; the binding list is walked only for ports with several).
    // Returns the final verdict word; counts the frame and adds it to the tile histogram.
    auto demux_frame = [&](uint32_t i, uint32_t m, uint2 Sv, uint4 Ev) -> uint32_t {
        const bool valid = t0 + i < t1;
        const uint4 e = (Sv.x >> 16) ? Ev : make_uint4(0, 0, 0, 0);
        const uint32_t dip = Sv.y;
        const bool match0 = e.x != 0u && (dip == e.z || e.z == 0u);     // poller.c:391
        uint32_t fan = match0 ? 1u : 0u;
        uint32_t first = match0 ? (e.w & 0x7FFFFFFFu) : 0u;
        const bool walk = e.x > 1u && !(match0 && !(e.w >> 31));        // poller.c:396-403
        if (__ballot(walk)) {
            if (walk) {
                for (uint32_t b = 1; b < e.x; ++b) {
                    const uint2 bd = a.binds[e.y + b];
                    if (dip == bd.x || bd.x == 0u) {
                        const uint32_t sock = bd.y & 0x7FFFFFFFu;
                        if (fan > 0 && a.n_lanes > 1u)
                            hist_add(sock & a.lane_mask, 1u);           // clones (rare)
                        if (fan == 0) first = sock;
                        ++fan;
                        if (!(bd.y >> 31)) break;
                    }
                }
            }
        }
        const uint32_t pre = m & 0xFu;
        const uint32_t verdict = pre != 0xFu ? pre
                               : e.x == 0u ? UDPDK_V_NO_BIND
                               : fan ? UDPDK_V_DELIVERED : UDPDK_V_NO_MATCH;
        const uint32_t fin = (m & ~0xFu) | verdict | (min(fan, 127u) << 9) | ((first & 0xFFFFu) << 16);
        // per-lane packed counters (8-bit fields; a lane sees <= 64 frames per tile)
        const uint32_t vinc = valid ? 1u << (8u * (verdict & 3u)) : 0u;
        acc_v0 += verdict < 4u ? vinc : 0u;
        acc_v1 += verdict < 4u ? 0u : vinc;
        acc_fan += fan;
        const bool delivered = valid && fan > 0u;
        // first delivery of every frame into the tile histogram; small key spaces are
        // aggregated with a wave multi-split first (all 64 lanes may share one lane)
        // (one lane: the tile's count is its delivery counter, written at the tile end)
        const uint32_t key = first & a.lane_mask;
        if (a.n_lanes == 1u) {
        } else if (a.key_bits <= 4u) {
            // (wave_peers written out: through the helper the kernel's register allocation changes)
            unsigned long long peers = __ballot(delivered);
            for (uint32_t bit = 0; bit < a.key_bits; ++bit) {
                const bool kb = (key >> bit) & 1u;
                const unsigned long long bal = __ballot(kb);
                peers &= kb ? bal : ~bal;
            }
            if (delivered && lane == (uint32_t)__ffsll((long long)peers) - 1u)
                hist_add(key, (uint32_t)__popcll(peers));
        } else if (delivered) {
            hist_add(key, 1u);
        }
        return fin;
    };
    // the argument-borne bind table (few bound ports): the port's entry from LDS (slot n_inl is
    // zero: an unbound port); one bound port, the pktgen case, is one compare
    auto inl_entry = [&](uint32_t pt) -> uint4 {
        uint32_t k = a.n_inl;
        if (a.n_inl == 1u) {
            k = pt == a.inl_port[0] ? 0u : 1u;
        } else {
#pragma unroll
            for (uint32_t q = 0; q < UDPDK_INLINE_PORTS; ++q)
                k = q < a.n_inl && pt == a.inl_port[q] ? q : k;
        }
        return inl_tab[k];
    };
    // One-round tiles with the argument-borne table demux each frame in its step (an LDS lookup,
    // no global load to batch): the tile's end no longer waits for a demux pass over the round.
    // Several rounds keep the round's pass (their verdict words are stored by it, after the
    // round's tail passes).
    const bool step_demux = a.inl && nbuf == 1u;
    uint32_t pf_o[SPT], pf_l[SPT], pf_t[SPT];             // MR: the next round's descriptors
    // rounds of RX_ROUND frames: SPR steps per wave (each followed by its tail pass when a frame
    // of the step is pending), then the round's demux pass
    for (uint32_t rnd = 0; rnd < steps / RSTEPS; ++rnd) {
#pragma unroll 1
        for (uint32_t jstep = 0; jstep < SPR; ++jstep) {
            const uint32_t p = t0 + st * 64 + lane;
            const bool valid = p < t1;
            const uint32_t off = c_off, len = c_lp & 0xFFFFu;
            const bool good = valid && len <= a.frames_bytes && off <= a.frames_bytes - len;
            // MR: the next round's descriptors go out at the round's first step, into registers,
            // and are stored to LDS at its staging step: the staging no longer waits a round trip
            // (config 5: a descriptor round trip per round was a fifth of each workgroup's time)
            if (MR && jstep == 0u && rnd + 1u < steps / RSTEPS) {
                stage_load(rnd + 1u, pf_o, pf_l, pf_t);
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t nst = st + CLS_WAVES;
            uint32_t n_off, n_lp;
            Win NW;
            // Fairness between the workgroups sharing a CU: the instruction arbiter favours higher
            // priority, then age, so the workgroups dispatched first kept winning the memory
            // pipeline and the launch waited for the last ones (config 3 stamps: workgroup
            // durations 168 / 227 / 299 us at p0 / p50 / p100, all resident from the start). A wave
            // drops a priority level each quarter of its steps, so the ones behind catch up.
            // (Long-frame forms only: config 2's G = 1 form measured even to slightly slower.)
            if constexpr (G == 2) {
                const uint32_t lv = (4u * (st / CLS_WAVES)) / (steps / CLS_WAVES);
                if (lv == 0u) __builtin_amdgcn_s_setprio(3);
                else if (lv == 1u) __builtin_amdgcn_s_setprio(2);
                else if (lv == 2u) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }
            // a step that sweeps its span reads its window from the sweep (no window was loaded)
            if (SPAN && span_cur) {
                W = span_sweep(st, span_A, span_E, off, len);
                tailed = true;
            }

            // ---- header fields from the window registers (lane = frame) ----
            const uint32_t D[14] = {W.a.x, W.a.y, W.a.z, W.a.w, W.b.x, W.b.y, W.b.z, W.b.w,
                                    W.c.x, W.c.y, W.c.z, W.c.w, W.d.x, W.d.y};
            const uint32_t sh = off & 3u;     // lanes whose window was not loaded: unused words
            uint32_t g[13];                   // g[i] = frame bytes 12+4i ..
#pragma unroll
            for (int i = 0; i < 13; ++i) g[i] = __builtin_amdgcn_alignbyte(D[i + 1], D[i], sh);
            // IPv4 gate (udpdk_poller.c:334): the ptype array's L3_IPV4 bit when given, else derived
            // from ether_type (frames shorter than an Ethernet header are not IPv4)
            const uint32_t eth_ip = (len >= 14u && (g[0] & 0xFFFFu) == 0x0008u) ? 0x10u : 0u;
            const bool ipv4 = good && ((has_ptype ? (c_lp >> 12) : eth_ip) & 0x10u);
            // (bswap16 written out: through the helper the kernel's instruction order changes)
            const uint32_t frag = ((g[2] & 0xFFu) << 8) | ((g[2] >> 8) & 0xFFu);
            const bool l3 = ipv4 && len >= 42u;
            const bool fragd = (frag & 0x3FFFu) != 0u;                // udpdk_poller.c:338
            // a fragment needs only its IPv4 header (poller.c:338-361): 34-41 B fragments reassemble
            const bool l3h = ipv4 && len >= 34u;
            const bool hdr = l3 || (l3h && fragd);                    // IPv4 flags and counters
            const bool not_udp = (g[2] >> 24) != 17u;                 // udpdk_poller.c:368-371
            const bool is_udp = l3 && !fragd && !not_udp;
            const uint32_t dport = g[6] & 0xFFFFu;                   // poller.c:372
            STAMP(1);

            // ---- everything the header window gives ----
            // IPv4 header checksum over the fixed 20 bytes at offset 14 (RFC 1071)
            const uint32_t ipraw = sad16(g[4], sad16(g[3], sad16(g[2], sad16(g[1],
                                   (g[0] >> 16) + (g[5] & 0xFFFFu)))));
            const bool ip_ok = fold32(ipraw) == 0xFFFFu;
            const bool ihl_ne5 = ((g[0] >> 16) & 0x0Fu) != 5u;
            const uint32_t dip = (g[4] >> 16) | (g[5] << 16);         // poller.c:373
            const uint32_t ulen_raw = g[6] >> 16;
            const uint32_t ulen = bswap16(ulen_raw);
            const uint32_t ucks = g[7] & 0xFFFFu;
            const bool len_bad = ulen < 8u || 34u + ulen > len;
            // UDP checksum (RFC 768 over the datagram, frame bytes [34, 34 + ulen), plus the pseudo-
            // header {src, dst, proto 17, udp length}), computed only where it decides the state:
            // a frame whose datagram ends within the window is summed here; a longer one is left to
            // the tile's tail pass (state 3 = pending until then). Ethernet padding after the
            // datagram is never summed.
            const bool need_cs = is_udp && ucks != 0u && !len_bad;
            const uint32_t dge = 34u + ulen;                          // datagram end (<= len)
            // a swept step has every frame's tail sum over [64, len): a datagram that ends there
            // (no padding) is complete now, any other pending one goes to the tail pass
            const bool swept = SPAN && span_cur && dge == len;
            const bool pend = need_cs && dge > 64u && !swept;
            const bool pend_sw = need_cs && dge > 64u && swept;
            uint32_t ws = 0, ws2 = 0;
#pragma unroll
            for (int i = 6; i < 13; i += 2) ws = sad16(g[i], ws);
#pragma unroll
            for (int i = 7; i < 13; i += 2) ws2 = sad16(g[i], ws2);
            ws += ws2;
            if (__ballot(need_cs && dge < 64u)) {                     // short or padded frames
                uint32_t wm = 0;
#pragma unroll
                for (int i = 6; i < 13; ++i) wm = sad16(g[i] & dword_window(34 - 12, (int)dge - 12, i), wm);
                ws = dge < 64u ? wm : ws;
            }
            const uint32_t us = ws + (g[5] >> 16) + (g[3] >> 16) + (g[4] & 0xFFFFu) + (dip & 0xFFFFu) +
                                (dip >> 16) + 0x1100u + ulen_raw;
            dgl[(st * 64 + lane) & (RX_ROUND - 1u)] = dge | fold32(us) << 16;
            // the swept datagrams' checksums (buffer-aligned tail words: swapped back at odd offsets)
            bool sw_ok = false;
            if (SPAN && __ballot(pend_sw)) {
                uint32_t t = fold32(span_tail(off, len, D));
                if (off & 1u) t = ((t & 0xFFu) << 8) | (t >> 8);    // (t < 2^16, as in the tail pass)
                sw_ok = fold32(t + fold32(us)) == 0xFFFFu;
            }
            STAMP(2);

            // ---- next step of this wave: window loads stay in flight across the rest of this step.
            // A step with pending frames issues them after its tail pass instead: a window's lines
            // (the one it shares with the frame's first tail chunk, and the one the previous
            // frame's tail ends in) are then still in L2 when that step's tail reads them, where a
            // window loaded a whole step earlier had left L2 by then (IMIX fetched 1.29x its bytes).
            // A next step that sweeps its span loads no window.
            read_desc(nst, n_off, n_lp);      // in range of the buffers for any s (unused past the tile)
            uint32_t n_A = 0, n_E = 0;
            const bool span_n = span_check(nst, n_off, n_lp & 0xFFFFu, n_A, n_E);
            const bool tail_now = __ballot(pend) != 0ull;
            if (!tail_now) NW = load_win(nst, n_off, n_lp & 0xFFFFu, span_n);

            // ---- what does not need the port entry: UDP state, flags, flag counters ----
            const uint32_t state = ucks == 0u ? UDPDK_UDP_CSUM_NONE
                                 : pend ? 3u
                                 : pend_sw ? (sw_ok ? UDPDK_UDP_CSUM_OK : UDPDK_UDP_CSUM_BAD)
                                 : (len_bad || fold32(us) != 0xFFFFu) ? UDPDK_UDP_CSUM_BAD
                                                                       : UDPDK_UDP_CSUM_OK;
            const uint32_t pre = !good ? UDPDK_V_BAD_DESC
                               : !ipv4 ? UDPDK_V_NOT_IPV4
                               : !l3h ? UDPDK_V_TRUNC
                               : fragd ? UDPDK_V_FRAG
                               : !l3 ? UDPDK_V_TRUNC
                               : not_udp ? UDPDK_V_NOT_UDP : 0xFFu;       // 0xFF: UDP, demux pending
            const uint32_t l3f = hdr ? ((ip_ok ? 1u : 0u) << 4 | (ihl_ne5 ? 1u : 0u) << 8) : 0u;
            const uint32_t udpf = is_udp ? (state << 5 | (len_bad ? 1u : 0u) << 7) : 0u;
            // (pending frames count their UDP state in the tail pass)
            acc_f0 += (hdr && !ip_ok ? 1u : 0u) | (hdr && ihl_ne5 ? 0x100u : 0u) |
                      (is_udp && state == UDPDK_UDP_CSUM_OK ? 0x10000u : 0u) |
                      (is_udp && state == UDPDK_UDP_CSUM_BAD ? 0x1000000u : 0u);
            acc_f1 += (is_udp && state == UDPDK_UDP_CSUM_NONE ? 1u : 0u) | (is_udp && len_bad ? 0x100u : 0u);
            if (good) lane_bytes += len;

            // the port-table lookup: now (step_demux), else in the round's demux pass (verdict
            // field 0xF until then)
            {
                const uint32_t w0 = (pre == 0xFFu ? 0xFu : pre) | l3f | udpf;
                const uint2 sv = make_uint2(dport | (is_udp ? 0x10000u : 0u), dip);
                const uint32_t si = (st * 64 + lane) & (RX_ROUND - 1u);
                if (step_demux) {
                    mstage[si] = demux_frame(st * 64 + lane, w0, sv, inl_entry(dport));
                } else {
                    mstage[si] = w0;
                    dstash[si] = sv;
                }
            }
            if (tail_now) {
                tail_step(st);
                NW = load_win(nst, n_off, n_lp & 0xFFFFu, span_n);
            }
            STAMP(6);
            // next round's descriptors into the other buffer at the wave's next-to-last step of a
            // round (its steps of round r are 16 r + w + CLS_WAVES j, j < SPR): the last reads of that
            // buffer were before the previous round's barrier, and the next round is first read at
            // j = SPR - 1.
            // Uniform across the workgroup (every wave has steps / 4 steps).
            if ((st / CLS_WAVES) % SPR == SPR - 2u && st / RSTEPS + 1u < steps / RSTEPS) {
                if constexpr (MR != 0)
                    stage_store(st / RSTEPS + 1u, pf_o, pf_l, pf_t);
                else
                    stage(st / RSTEPS + 1u);
                __syncthreads();
                STAMP(5);
            }
            W = NW;
            c_off = n_off;
            c_lp = n_lp;
            span_cur = span_n;
            span_A = n_A;
            span_E = n_E;
            st = nst;
        }
        // ---- demux pass (not step_demux): the round's port-table lookups of this wave, all SPR
        // steps' 16-byte entries in flight at once (one round trip per round instead of one
        // exposed per step) ----
        if (!step_demux) {
            uint4 E[SPR];
            uint2 S[SPR];
#pragma unroll
            for (uint32_t j = 0; j < SPR; ++j) S[j] = dstash[((st - RSTEPS + CLS_WAVES * j) * 64 + lane) & (RX_ROUND - 1u)];
            if (a.inl) {
#pragma unroll
                for (uint32_t j = 0; j < SPR; ++j) E[j] = inl_entry(S[j].x & 0xFFFFu);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SPR; ++j) E[j] = a.port_tab[S[j].x & 0xFFFFu];
            }
#pragma unroll
            for (uint32_t j = 0; j < SPR; ++j) {
                const uint32_t i = (st - RSTEPS + CLS_WAVES * j) * 64 + lane;
                const uint32_t fin = demux_frame(i, mstage[i & (RX_ROUND - 1u)], S[j], E[j]);
                mstage[i & (RX_ROUND - 1u)] = fin;
                // a tile of several rounds stores each round's verdict words here (its LDS holds
                // one round, so three workgroups fit a CU at 4096 lanes instead of two)
                if (nbuf > 1u && t0 + i < t1) a.meta[t0 + i] = fin;
            }
        }
        STAMP(3);
    }

    // The tile's stores go out first (its verdict words are all in LDS after this barrier), the
    // counter reduction after them: the fused completion's drain then finds them written.
    __syncthreads();
    auto tile_counter = [&](uint32_t c) -> uint32_t {
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < CLS_WAVES; ++i) v += cntw[i * 16 + c];
        return v;
    };
    // Fused completion (a.fuse, single lane, one-round tiles): every store another workgroup may
    // read in this launch is written through (sc1) and drained before the workgroup's arrival,
    // as cdna_hip_programming.md Guideline 16 / MI355X_MICROARCH.md "Valid forms" require.
    const bool fuse = a.fuse != nullptr;
    uint32_t tcount = 0;                                   // the tile's deliveries (spec / fuse)
    if (a.spec_pkt) {
        // Speculative lane entries (single lane, 1024-frame one-round tile, 4 frames per
        // thread): the tile's delivered frames in order at t0 + rank, which is where they belong
        // when every earlier tile delivered all its frames. rx_compact1 (or the fused completion
        // below) keeps them then and rewrites the later tiles otherwise.
        __shared__ uint32_t spec_ws[CLS_WAVES];
        const uint32_t nv = t1 - t0, j0 = 4u * tid;
        uint32_t d = 0;
        if (j0 < nv) {
            const uint4 v = reinterpret_cast<const uint4 *>(mstage)[tid];
            d = ((v.x & 0xFu) == UDPDK_V_DELIVERED ? 1u : 0u) |
                ((v.y & 0xFu) == UDPDK_V_DELIVERED && j0 + 1u < nv ? 2u : 0u) |
                ((v.z & 0xFu) == UDPDK_V_DELIVERED && j0 + 2u < nv ? 4u : 0u) |
                ((v.w & 0xFu) == UDPDK_V_DELIVERED && j0 + 3u < nv ? 8u : 0u);
        }
        const uint32_t cnt = (uint32_t)__builtin_popcount(d);
        const uint32_t incl = wave_incl_scan(cnt);
        if (lane == 63) spec_ws[w] = incl;
        __syncthreads();
        uint32_t pos = t0 + incl - cnt;
#pragma unroll
        for (uint32_t i = 0; i < CLS_WAVES; ++i) {
            pos += i < w ? spec_ws[i] : 0u;
            tcount += spec_ws[i];
        }
        // a tile short of a full tile's deliveries (the last tile never counts: nothing follows
        // it) marks its successors' entries wrong; every other word of the flag stays untouched
        if (tid == 0 && tile + 1u < a.n_tiles && tcount != a.tile_frames)
            atomicMax(&a.spec_nonfull[tile % UDPDK_SPEC_WORDS],
                      ((unsigned long long)a.spec_epoch << 32) | (0xFFFFFFFFu - tile));
        const uint32_t f = t0 + j0;
        if (fuse) {
            // written through: the completing workgroup may rewrite these words (no stale dirty
            // copy may stay behind in this XCD's L2) -- range-checked by the resource
            const __amdgpu_buffer_rsrc_t sr =
                make_rsrc(a.spec_pkt, a.spec_cap >= 0x40000000u ? 0xFFFFFFFCu : a.spec_cap * 4u);
            if (d == 0xFu && (pos & 3u) == 0u) {
                const __attribute__((ext_vector_type(4))) uint32_t x = {f, f + 1u, f + 2u, f + 3u};
                __builtin_amdgcn_raw_buffer_store_b128(x, sr, (int)(4u * pos), 0, PL);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    if ((d >> j) & 1u) {
                        __builtin_amdgcn_raw_buffer_store_b32(f + j, sr, (int)(4u * pos), 0, PL);
                        ++pos;
                    }
            }
        } else if (d == 0xFu && (pos & 3u) == 0u && pos + 4u <= a.spec_cap) {
            *reinterpret_cast<uint4 *>(a.spec_pkt + pos) = make_uint4(f, f + 1u, f + 2u, f + 3u);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if ((d >> j) & 1u) {
                    if (pos < a.spec_cap) a.spec_pkt[pos] = f + j;
                    ++pos;
                }
        }
    }
    if (nbuf == 1u) {
        const uint32_t nv = t1 - t0;
        uint32_t *dst = a.meta + t0;
        if (fuse) {
            // verdict words written through (the completing workgroup reads them back when a
            // tile was not full)
            const __amdgpu_buffer_rsrc_t mr = make_rsrc(dst, nv * 4u);
            if (((uintptr_t)dst & 15u) == 0) {
                const uint4 *s4 = reinterpret_cast<const uint4 *>(mstage);
                for (uint32_t i = tid; i < (nv + 3u) / 4u; i += CLS_BLOCK) {
                    const uint4 v = s4[i];
                    const __attribute__((ext_vector_type(4))) uint32_t x = {v.x, v.y, v.z, v.w};
                    if (4u * i + 4u <= nv)
                        __builtin_amdgcn_raw_buffer_store_b128(x, mr, (int)(16u * i), 0, PM);
                    else
                        for (uint32_t j = 4u * i; j < nv; ++j)
                            __builtin_amdgcn_raw_buffer_store_b32(mstage[j], mr, (int)(4u * j), 0, PM);
                }
            } else {
                for (uint32_t i = tid; i < nv; i += CLS_BLOCK)
                    __builtin_amdgcn_raw_buffer_store_b32(mstage[i], mr, (int)(4u * i), 0, PM);
            }
        } else if (nv == a.tile_frames && ((uintptr_t)dst & 15u) == 0) {
            uint4 *d4 = reinterpret_cast<uint4 *>(dst);
            const uint4 *s4 = reinterpret_cast<const uint4 *>(mstage);
            for (uint32_t i = tid; i < nv / 4; i += CLS_BLOCK) d4[i] = s4[i];
        } else {
            for (uint32_t i = tid; i < nv; i += CLS_BLOCK) dst[i] = mstage[i];
        }
    }
    // ---- tile counters: one row per wave (lanes 0-15), summed by the readers ----
    uint32_t sc[UDPDK_N_COUNTERS];
    {
        auto wsum = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(v), 63); };
        const uint32_t packed[4] = {acc_v0, acc_v1, acc_f0, acc_f1};
        const int field[4][4] = {{0, 1, 2, 3}, {4, 5, 6, 7},
                                 {UDPDK_C_IP_BAD, UDPDK_C_IHL_NE5, UDPDK_C_UDP_OK, UDPDK_C_UDP_BAD},
                                 {UDPDK_C_UDP_NONE, UDPDK_C_LEN_BAD, -1, -1}};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ev = wsum(packed[k] & 0x00FF00FFu);        // 16-bit sums: no carry
            const uint32_t od = wsum((packed[k] >> 8) & 0x00FF00FFu);
            if (field[k][0] >= 0) sc[field[k][0]] = ev & 0xFFFFu;
            if (field[k][1] >= 0) sc[field[k][1]] = od & 0xFFFFu;
            if (field[k][2] >= 0) sc[field[k][2]] = ev >> 16;
            if (field[k][3] >= 0) sc[field[k][3]] = od >> 16;
        }
        sc[UDPDK_C_DELIVERIES] = wsum(acc_fan);
        sc[UDPDK_C_BYTES] = wsum(lane_bytes);
    }
    {
        uint32_t row = 0;
#pragma unroll
        for (int c = 0; c < UDPDK_N_COUNTERS; ++c) row = lane == (uint32_t)c ? sc[c] : row;
        if (lane < UDPDK_N_COUNTERS) cntw[w * 16 + lane] = row;
        if (tailed && lane == 0) tail_any = 1u;
    }
    __syncthreads();
    STAMP(7);
    if (a.n_lanes == 1u) {
        if (tid == 0) {
            if (fuse)
                __hip_atomic_store(&a.hist[tile], tcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                a.hist[tile] = tile_counter(UDPDK_C_DELIVERIES);
        }
    } else {
        if (a.hist16) {           // u16 row of n_lanes (rounded up to even) counts
            const uint32_t hw = (a.n_lanes + 1u) >> 1;
            for (uint32_t s = tid; s < hw; s += CLS_BLOCK) a.hist[(size_t)tile * hw + s] = hist[s];
        } else {
            for (uint32_t s = tid; s < a.n_lanes; s += CLS_BLOCK)
                a.hist[(size_t)tile * a.n_lanes + s] = hist[s];
        }
    }
    if (tid < UDPDK_N_COUNTERS) a.tile_cnt[(size_t)tile * UDPDK_N_COUNTERS + tid] = tile_counter(tid);
    // the host's kernel choice for its next calls: this call needed tail passes. Sampled (every
    // 64th tile, one lane): a store to host memory per wave cost IMIX classify 91 -> 544 us. After
    // the fused completion: its drain would otherwise wait for these stores to cross PCIe.
    const bool hint = a.hint && (tile & 63u) == 0u && tid == 0;
    const bool tail_seen = tail_any != 0u;
    if (fuse) classify_complete(a, tile, tcount, tid, lane, w, smem);
    if (hint) {
        if (tail_seen)
            __hip_atomic_store(&a.hint[UDPDK_HINT_TAIL], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (tile == 0u)
            __hip_atomic_store(&a.hint[UDPDK_HINT_DONE], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#ifdef UDPDK_STAMPS
    STAMP(4);                                              // slot 4: fused completion
    STAMP_END();
    __syncthreads();
    if (a.dbg && w == 0 && lane < 16) a.dbg[blockIdx.x * 16 + lane] = st_acc[lane];
#endif
}
template __global__ void rx_classify<1, 0, 0>(RxArgs a);
template __global__ void rx_classify<2, 0, 0>(RxArgs a);
template __global__ void rx_classify<1, 1, 0>(RxArgs a);
template __global__ void rx_classify<2, 1, 0>(RxArgs a);
template __global__ void rx_classify<1, 0, 1>(RxArgs a);
template __global__ void rx_classify<2, 0, 1>(RxArgs a);
template __global__ void rx_classify<1, 1, 1>(RxArgs a);
template __global__ void rx_classify<2, 1, 1>(RxArgs a);

} // namespace udpdk
