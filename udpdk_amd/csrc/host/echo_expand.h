/*
 * echo_expand.h — the host half of udpdk_poll_echo's output format: the per-datagram arrays a
 * reply plan leaves (payload_len, sockfd, frame_off; udpdk_gpu_tx_reply_plan) expanded into
 * udpdk_tx_drain's per-frame table (out_off / out_len, a datagram's fragments consecutive).
 * Pure functions of their arguments, no library state: rx_echo.c uses them, and
 * tools/echo_expand_check.c runs them behind a main() under the host sanitizers.
 */
#ifndef UDPDK_ECHO_EXPAND_H
#define UDPDK_ECHO_EXPAND_H

#include <errno.h>
#include <stdint.h>

/* udpdk_gpu_tx_span (udpdk_gpu.h) without the library: output bytes and frames of one datagram. */
static inline uint64_t h_echo_span(uint32_t len, uint32_t mtu, uint32_t *n_frames)
{
    uint32_t nf = 1;
    uint64_t span = (uint64_t)len + 42u;
    if (mtu >= 68u && (mtu - 20u) % 8u == 0 && (uint64_t)len + 42u > mtu) {
        nf = (uint32_t)(((uint64_t)len + 8u + (mtu - 20u) - 1u) / (mtu - 20u));
        span = (uint64_t)len + 8u + 34ull * nf;
    }
    if (n_frames) *n_frames = nf;
    return span;
}

/* Entries with sockfd < 0 answer nothing. *n_frames gets the number of frames the answering
 * entries make, whatever the result. Returns 0 with out_off / out_len filled for all of them;
 * -ENOBUFS when they are more than max (nothing written); -EINVAL when an answering entry's frames
 * would end past out_bytes (a plan never leaves one: nothing written). */
static inline int h_echo_expand(const uint16_t *payload_len, const int32_t *sockfd, const uint32_t *frame_off,
                                uint32_t count, uint32_t mtu, uint64_t out_bytes, uint32_t max,
                                uint32_t *out_off, uint16_t *out_len, uint32_t *n_frames)
{
    uint64_t need = 0;
    int bad = 0;
    for (uint32_t k = 0; k < count; k++) {
        if (sockfd[k] < 0) continue;
        uint32_t nf;
        const uint64_t span = h_echo_span(payload_len[k], mtu, &nf);
        if ((uint64_t)frame_off[k] + span > out_bytes) bad = 1;
        need += nf;
    }
    if (n_frames) *n_frames = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)need;
    if (bad) return -EINVAL;
    if (need > max) return -ENOBUFS;
    uint32_t j = 0;
    for (uint32_t k = 0; k < count; k++) {
        if (sockfd[k] < 0) continue;
        uint32_t nf;
        const uint64_t span = h_echo_span(payload_len[k], mtu, &nf);
        for (uint32_t f = 0; f < nf; f++) {
            out_off[j] = frame_off[k] + f * (mtu + 14u);
            out_len[j] = (uint16_t)(f + 1 < nf ? mtu + 14u : span - (uint64_t)(nf - 1) * (mtu + 14u));
            j++;
        }
    }
    return 0;
}

#endif
