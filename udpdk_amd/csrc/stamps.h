// stamps.h — per-phase timing stamps of the diagnostic build (make stamps, tools/stamps.py);
// empty in the product build. Stamps never feed an output (cdna_hip_programming.md §7).
//
// -DUDPDK_STAMPS: wave 0 of every workgroup accumulates s_memtime cycles per phase, written to
// a.dbg[block][16] at the kernel's end. The macros use the kernel's own locals.
//   STAMP(k), STAMP_END()  rx_classify: w, lane, tid, tile, st_acc[16] (LDS), st_last
//   SSTAMP(k)              rx_scatterw: w, sacc[16], slast
// -DUDPDK_STAMPS_LIGHT keeps only rx_classify's entry/exit realtime stamps (dispatch timeline).
#pragma once

#if defined(UDPDK_STAMPS) && !defined(UDPDK_STAMPS_LIGHT)
#define STAMP(k)                                                                 \
    do {                                                                         \
        if (w == 0) {                                                            \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();          \
            if (lane == 0) st_acc[k] += t_ - st_last;                            \
            st_last = t_;                                                        \
        }                                                                        \
    } while (0)
#else
#define STAMP(k) do {} while (0)
#endif
// slots 12-15: realtime (100 MHz, chip-synchronous) at entry and exit, HW_ID | XCC_ID << 32, tile
#ifdef UDPDK_STAMPS
#define STAMP_END()                                                                   \
    do {                                                                              \
        if (tid != 0) break;                                                          \
        st_acc[13] = __builtin_amdgcn_s_memrealtime();                                \
        st_acc[14] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |  \
                     ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32); \
        st_acc[15] = tile;                                                            \
    } while (0)
#define SSTAMP(k)                                                         \
    do {                                                                  \
        if (w == 0) {                                                     \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();   \
            sacc[k] += t_ - slast;                                        \
            slast = t_;                                                   \
        }                                                                 \
    } while (0)
#else
#define SSTAMP(k) do {} while (0)
#endif
