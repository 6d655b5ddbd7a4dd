// Cache policy of rx_classify's streams at the config-2 launch shape (1 M x 64 B frames, one
// workgroup of 256 threads per 1024-frame tile, 4 steps per wave, lane = frame): which `aux`
// bits on the frame loads, the descriptor loads and the verdict-word / lane-entry stores make the
// launch fastest. The kernel moves the bytes the way the real one does and nothing else:
// descriptors (u32 offset + u16 length) read coalesced into LDS, per step a 3 x 16 B + 8 B
// dword-aligned buffer-load window at a 64 B stride (the next step's in flight over the current
// one's sum), one 4 B verdict word per frame staged in LDS and stored as 16-B rows at the tile
// end, and 4 B lane entries stored as 16-B rows.
//
// Arms: frame loads {default, nt} x descriptor loads {default, nt} x stores {sc1, sc1 nt, plain,
// nt}. Each arm back-to-back on one stream and round-robin on 3 streams, in two rotations:
//   all9    frames, descriptors and outputs all rotate over 9 sets (what bench.py does: 9 x 64 MB
//           of frames, 9 x 14 MB of descriptors and outputs, the latter inside the Infinity Cache)
//   out3    frames and descriptors rotate over 9 sets, outputs are one set per stream
// Arms are interleaved within a repetition (REPS of them), so drift hits every arm alike.
// Results: profiles/r07a_policy_probe.txt.
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/probe/policy_probe tools/probe/policy_probe.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CK(x)                                                                              \
    do {                                                                                   \
        const hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

constexpr uint32_t N = 1u << 20, FL = 64, TILE = 1024, BLOCK = 256, SETS = 9;
// aux bits of the gfx950 buffer instructions: 2 = nt, 16 = sc1
constexpr int AUX_NT = 2, AUX_SC1 = 16;

struct Args {
    const uint8_t *frames;
    const uint32_t *offset;
    const uint16_t *length;
    uint32_t *meta;
    uint32_t *lane_pkt;
    uint32_t frames_bytes;
    uint32_t n;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), (short)0, (int)bytes, 0x00020000);
}

struct Win {
    uint4 a, b, c;
    uint2 d;
};

template <int LF, int LD, int ST>
__global__ void __launch_bounds__(BLOCK) policy_kernel(Args a)
{
    __shared__ uint32_t d_off[TILE], d_len[TILE];
    __shared__ __attribute__((aligned(16))) uint32_t mstage[TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t t0 = blockIdx.x * TILE;
    // every access below goes through a range-checked resource of the array's exact size
    const __amdgpu_buffer_rsrc_t fr = make_rsrc(a.frames, a.frames_bytes);
    const __amdgpu_buffer_rsrc_t orr = make_rsrc(a.offset, a.n * 4u);
    const __amdgpu_buffer_rsrc_t lr = make_rsrc(a.length, a.n * 2u);
    const __amdgpu_buffer_rsrc_t mr = make_rsrc(a.meta, a.n * 4u);
    const __amdgpu_buffer_rsrc_t pr = make_rsrc(a.lane_pkt, a.n * 4u);
    uint32_t o[4], l[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t p = t0 + i * BLOCK + tid;
        o[i] = __builtin_amdgcn_raw_buffer_load_b32(orr, (int)(4u * p), 0, LD);
        l[i] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(lr, (int)(2u * p), 0, LD);
    }
    auto load_win = [&](uint32_t off, uint32_t len, bool ok) -> Win {
        const uint32_t b = ok && len >= 14u && len <= a.frames_bytes && off <= a.frames_bytes - len
                               ? (off + 12u) & ~3u : 0u;
        Win r;
        const auto x = __builtin_amdgcn_raw_buffer_load_b128(fr, (int)b, 0, LF);
        const auto y = __builtin_amdgcn_raw_buffer_load_b128(fr, (int)(b + 16u), 0, LF);
        const auto z = __builtin_amdgcn_raw_buffer_load_b128(fr, (int)(b + 32u), 0, LF);
        const auto d = __builtin_amdgcn_raw_buffer_load_b64(fr, (int)(b + 48u), 0, LF);
        r.a = make_uint4(x[0], x[1], x[2], x[3]);
        r.b = make_uint4(y[0], y[1], y[2], y[3]);
        r.c = make_uint4(z[0], z[1], z[2], z[3]);
        r.d = make_uint2(d[0], d[1]);
        return r;
    };
    // the wave's first window goes out before the staging barrier (step w = this thread's frames)
    Win W = load_win(o[0], l[0], true);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        d_off[i * BLOCK + tid] = o[i];
        d_len[i * BLOCK + tid] = l[i];
    }
    __syncthreads();
    constexpr uint32_t STEPS = TILE / 64;
    for (uint32_t st = w; st < STEPS; st += 4) {
        const uint32_t nst = st + 4u, ni = (nst * 64u + lane) & (TILE - 1u);
        const Win NW = load_win(d_off[ni], d_len[ni], nst < STEPS);
        const uint32_t sh = d_off[st * 64u + lane] & 3u;
        uint32_t s = __builtin_amdgcn_alignbyte(W.a.y, W.a.x, sh);
        s = __builtin_amdgcn_sad_u16(W.a.z, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.a.w, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.b.x ^ W.b.y, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.b.z ^ W.b.w, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.c.x ^ W.c.y, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.c.z ^ W.c.w, 0u, s);
        s = __builtin_amdgcn_sad_u16(W.d.x ^ W.d.y, 0u, s);
        mstage[st * 64u + lane] = s;
        W = NW;
    }
    __syncthreads();
    {
        const uint4 v = reinterpret_cast<const uint4 *>(mstage)[tid];
        const __attribute__((ext_vector_type(4))) uint32_t x = {v.x, v.y, v.z, v.w};
        __builtin_amdgcn_raw_buffer_store_b128(x, mr, (int)(4u * t0 + 16u * tid), 0, ST);
        const uint32_t f = t0 + 4u * tid;
        const __attribute__((ext_vector_type(4))) uint32_t y = {f, f + 1u, f + 2u, f + 3u};
        __builtin_amdgcn_raw_buffer_store_b128(y, pr, (int)(4u * t0 + 16u * tid), 0, ST);
    }
}

struct Arm {
    const char *name;
    void (*kern)(Args);
};
#define ARM(lf, ld, st, nm) {nm, policy_kernel<lf, ld, st>}
static const Arm ARMS[] = {
    ARM(0, 0, AUX_SC1, "ld default  desc default  st sc1"),        // the library's policy today
    ARM(0, 0, AUX_SC1 | AUX_NT, "ld default  desc default  st sc1 nt"),
    ARM(0, 0, 0, "ld default  desc default  st plain"),
    ARM(0, 0, AUX_NT, "ld default  desc default  st nt"),
    ARM(0, AUX_NT, AUX_SC1, "ld default  desc nt       st sc1"),
    ARM(0, AUX_NT, AUX_SC1 | AUX_NT, "ld default  desc nt       st sc1 nt"),
    ARM(0, AUX_NT, 0, "ld default  desc nt       st plain"),
    ARM(0, AUX_NT, AUX_NT, "ld default  desc nt       st nt"),
    ARM(AUX_NT, 0, AUX_SC1, "ld nt       desc default  st sc1"),
    ARM(AUX_NT, 0, AUX_SC1 | AUX_NT, "ld nt       desc default  st sc1 nt"),
    ARM(AUX_NT, 0, 0, "ld nt       desc default  st plain"),
    ARM(AUX_NT, 0, AUX_NT, "ld nt       desc default  st nt"),
    ARM(AUX_NT, AUX_NT, AUX_SC1, "ld nt       desc nt       st sc1"),
    ARM(AUX_NT, AUX_NT, AUX_SC1 | AUX_NT, "ld nt       desc nt       st sc1 nt"),
    ARM(AUX_NT, AUX_NT, 0, "ld nt       desc nt       st plain"),
    ARM(AUX_NT, AUX_NT, AUX_NT, "ld nt       desc nt       st nt"),
};
constexpr int N_ARMS = sizeof(ARMS) / sizeof(ARMS[0]);

int main()
{
    const int REPS = getenv("REPS") ? atoi(getenv("REPS")) : 5;
    const int R = getenv("LAUNCHES") ? atoi(getenv("LAUNCHES")) : 200;
    std::vector<uint8_t> hf((size_t)N * FL);
    for (size_t i = 0; i < hf.size(); ++i) hf[i] = (uint8_t)(i * 2654435761u >> 13);
    std::vector<uint32_t> ho(N);
    std::vector<uint16_t> hl(N, FL);
    for (uint32_t i = 0; i < N; ++i) ho[i] = i * FL;

    uint8_t *fr;
    uint32_t *off, *meta, *lp;
    uint16_t *len;
    CK(hipMalloc(&fr, (size_t)N * FL * SETS));
    CK(hipMalloc(&off, (size_t)N * 4 * SETS));
    CK(hipMalloc(&len, (size_t)N * 2 * SETS));
    CK(hipMalloc(&meta, (size_t)N * 4 * SETS));
    CK(hipMalloc(&lp, (size_t)N * 4 * SETS));
    for (uint32_t c = 0; c < SETS; ++c) {
        CK(hipMemcpy(fr + (size_t)c * N * FL, hf.data(), (size_t)N * FL, hipMemcpyHostToDevice));
        CK(hipMemcpy(off + (size_t)c * N, ho.data(), (size_t)N * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(len + (size_t)c * N, hl.data(), (size_t)N * 2, hipMemcpyHostToDevice));
    }
    hipStream_t ss[3];
    for (int k = 0; k < 3; ++k) CK(hipStreamCreateWithFlags(&ss[k], hipStreamNonBlocking));

    // mode bit 0: 3 streams; bit 1: outputs one set per stream (else rotating with the inputs)
    auto run = [&](const Arm &arm, int mode) -> double {
        const int ns = (mode & 1) ? 3 : 1;
        auto launch = [&](int i) {
            const uint32_t c = (uint32_t)i % SETS, oc = (mode & 2) ? (uint32_t)(i % ns) : c;
            Args a;
            a.frames = fr + (size_t)c * N * FL;
            a.offset = off + (size_t)c * N;
            a.length = len + (size_t)c * N;
            a.meta = meta + (size_t)oc * N;
            a.lane_pkt = lp + (size_t)oc * N;
            a.frames_bytes = N * FL;
            a.n = N;
            hipLaunchKernelGGL(arm.kern, dim3(N / TILE), dim3(BLOCK), 0, ss[i % ns], a);
        };
        for (int i = 0; i < 18; ++i) launch(i);
        CK(hipDeviceSynchronize());
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < R; ++i) launch(i);
        CK(hipDeviceSynchronize());
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / R;
    };

    static double us[4][N_ARMS][16];
    const int reps = std::min(REPS, 16);
    for (int rep = 0; rep < reps; ++rep)
        for (int mode = 0; mode < 4; ++mode)
            for (int k = 0; k < N_ARMS; ++k) us[mode][k][rep] = run(ARMS[k], mode);

    // every arm wrote the same words
    std::vector<uint32_t> hm(N);
    CK(hipMemcpy(hm.data(), meta, (size_t)N * 4, hipMemcpyDeviceToHost));
    unsigned long long sum = 0;
    for (uint32_t v : hm) sum += v;
    printf("verdict-word sum %llu (set 0)\n", sum);

    const char *MODE[4] = {"all9 1 stream", "all9 3 streams", "out3 1 stream", "out3 3 streams"};
    const double bytes = (double)N * (FL + 6 + 4 + 4);
    for (int mode = 0; mode < 4; ++mode) {
        printf("\n%s: us per launch, %d launches, %d interleaved reps: min / median / max   TB/s at median\n",
               MODE[mode], R, reps);
        for (int k = 0; k < N_ARMS; ++k) {
            std::sort(us[mode][k], us[mode][k] + reps);
            const double md = us[mode][k][reps / 2];
            printf("  %-38s %7.2f %7.2f %7.2f   %5.2f\n", ARMS[k].name, us[mode][k][0], md,
                   us[mode][k][reps - 1], bytes / md * 1e-6);
        }
    }
    return 0;
}
