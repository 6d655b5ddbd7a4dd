/*
 * icmp_queue.h — the host queue of ICMP and ARP frames built by a poll (and of the ARP announcement)
 * waiting for udpdk_tx_drain: a bounded ring of at most H_ICMPQ_FRAMES frames whose bytes live in one
 * ring of `cap` bytes. Every
 * frame is contiguous (a frame that does not fit before the end of the byte ring starts at 0, as
 * long as the oldest frame leaves that much room). A frame that fits neither the frame ring nor the
 * byte ring is dropped and counted. Header-only and free of the library's state so that it can be
 * tested alone (tools/icmp_queue_check.c). The callers serialise access (g_udpdk.tx_lock).
 */
#ifndef UDPDK_ICMP_QUEUE_H
#define UDPDK_ICMP_QUEUE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define H_ICMPQ_FRAMES 4096u             /* frames the queue holds */
#define H_ICMPQ_BYTES  (4u << 20)        /* bytes the library's queue holds (1 KiB a frame) */

struct h_icmpq {
    uint8_t *buf;
    uint32_t cap;
    uint32_t off[H_ICMPQ_FRAMES];
    uint16_t len[H_ICMPQ_FRAMES];
    uint32_t head, count;                /* oldest frame, frames queued */
    uint32_t wpos;                       /* where the next frame's bytes would start */
    uint64_t dropped;
};

/* 0, or -1 when the byte ring cannot be had. An initialised queue is emptied and keeps its ring
 * when the capacity is the same. */
static inline int h_icmpq_init(struct h_icmpq *q, uint32_t cap)
{
    if (!q->buf || q->cap != cap) {
        free(q->buf);
        q->buf = (uint8_t *)malloc(cap ? cap : 1);
        q->cap = q->buf ? cap : 0;
    }
    q->head = q->count = q->wpos = 0;
    return q->buf ? 0 : -1;
}

static inline void h_icmpq_reset(struct h_icmpq *q) { q->head = q->count = q->wpos = 0; }

static inline void h_icmpq_free(struct h_icmpq *q)
{
    free(q->buf);
    q->buf = NULL;
    q->cap = q->head = q->count = q->wpos = 0;
}

/* Append one frame of len bytes (1 .. 65535); 0 queued, -1 dropped (counted). */
static inline int h_icmpq_push(struct h_icmpq *q, const uint8_t *frame, uint32_t len)
{
    if (!q->buf || !len || len > 0xFFFFu || len > q->cap || q->count == H_ICMPQ_FRAMES) goto drop;
    uint32_t pos;
    if (!q->count) {
        pos = 0;
    } else {
        const uint32_t rpos = q->off[q->head];
        if (q->wpos > rpos) {                        /* the bytes in use are [rpos, wpos) */
            if (len <= q->cap - q->wpos) pos = q->wpos;
            else if (len <= rpos) pos = 0;
            else goto drop;
        } else {                                     /* wrapped: [rpos, cap) and [0, wpos) */
            if (len <= rpos - q->wpos) pos = q->wpos;
            else goto drop;
        }
    }
    memcpy(q->buf + pos, frame, len);
    const uint32_t slot = (q->head + q->count) % H_ICMPQ_FRAMES;
    q->off[slot] = pos;
    q->len[slot] = (uint16_t)len;
    q->count++;
    q->wpos = pos + len;
    return 0;
drop:
    q->dropped++;
    return -1;
}

/* The oldest frame (NULL when the queue is empty); it stays queued. */
static inline const uint8_t *h_icmpq_peek(const struct h_icmpq *q, uint32_t *len)
{
    if (!q->count) return NULL;
    *len = q->len[q->head];
    return q->buf + q->off[q->head];
}

static inline void h_icmpq_pop(struct h_icmpq *q)
{
    if (!q->count) return;
    q->head = (q->head + 1) % H_ICMPQ_FRAMES;
    if (!--q->count) q->wpos = 0;
}

/* Move frames, oldest first, into out / out_off / out_len (udpdk_tx_drain's format, frames back to
 * back from byte *bytes, frame index from *k) while another fits max frames and out_cap bytes; a
 * frame that does not fit stays queued, and so does everything behind it. */
static inline void h_icmpq_drain(struct h_icmpq *q, uint8_t *out, uint64_t out_cap, uint32_t *out_off,
                                 uint16_t *out_len, uint32_t max, uint32_t *k, uint64_t *bytes)
{
    uint32_t len = 0;
    const uint8_t *f;
    while (*k < max && (f = h_icmpq_peek(q, &len)) && *bytes + len <= out_cap) {
        memcpy(out + *bytes, f, len);
        out_off[*k] = (uint32_t)*bytes;
        out_len[*k] = (uint16_t)len;
        *bytes += len;
        (*k)++;
        h_icmpq_pop(q);
    }
}

#endif
