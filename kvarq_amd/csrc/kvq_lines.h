// kvarq_amd/csrc/kvq_lines.h -- what the kernels that walk the record index share (kernels_general.hip's trim, kernels_profile.hip,
// kernels_reads.hip, kernels_over.hip, kernels_adapt.hip, kernels_clip.hip, kernels_emit.hip, kernels_records.hip): the masked load of
// sixteen bytes of a line, the byte flags and masks on its words, the 64-bit shuffles, and the quality trim of one record by one
// wave.  One copy of each; a kernel file names what it uses by including this.
#pragma once

#include "kvq_device.h"

// the sixteen bytes [q, q + 16) of a line of `len` bytes whose terminator ('\n', or the '\r' in front of it) lies at line[len]: one
// vector where it fits into the line and its terminator, else words where they fit and bytes where the line ends (never a byte
// behind the terminator); zeros behind it
__device__ __forceinline__ void kvq_load16(const uint8_t *line, uint32_t len, uint32_t q, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (q + 16u <= len + 1u) {
#pragma unroll
        for (int d = 0; d < 4; d++) __builtin_memcpy(&w[d], line + q + 4u * d, 4);
    } else if (q < len) {
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const uint32_t qd = q + 4u * d;
            if (qd + 4u <= len + 1u) __builtin_memcpy(&w[d], line + qd, 4);
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) if (qd + j < len) w[d] |= (uint32_t)line[qd + j] << (8u * j);
            }
        }
    }
}

// 0x80 in every byte of x that equals the byte repeated in c4 (exact per byte: no carry leaves a byte)
__device__ __forceinline__ uint32_t kvq_eq_flags(uint32_t x, uint32_t c4)
{
    const uint32_t y = x ^ c4;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}
// the bytes of a 32-bit word that are among the first v (of the word and what follows it)
__device__ __forceinline__ uint32_t kvq_keep_bytes(uint32_t v) { return v >= 4u ? 0xFFFFFFFFu : (1u << (8u * v)) - 1u; }

// 64 bits from lane `src`, and from the lane whose number differs in the bits of d
__device__ __forceinline__ unsigned long long kvq_shfl64(unsigned long long v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long kvq_shfl_xor64(unsigned long long v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return (unsigned long long)hi << 32 | lo;
}

// ---------------------------------------------------------------------------
// quality trim
// ---------------------------------------------------------------------------

// running state of the longest-run search over the quality line, fed 64 bits
// at a time (bit i = score byte >= Amin).  A run only counts when a low byte
// closes it; the first of equally long runs wins (workhorse.c:1055-1068).
struct RunState { int in_run; uint32_t run_start; int best; uint32_t best_start; };

__device__ __forceinline__ void run_feed(RunState &st, uint64_t good, int nbits, uint32_t base)
{
    int pos = 0;
    while (pos < nbits) {
        if (st.in_run) {
            const uint64_t z = (~good) >> pos;
            const int d = z ? __ffsll((long long)z) - 1 : 64;
            if (pos + d >= nbits) break;                       // run continues in the next word
            const int len = (int)(base + pos + d - st.run_start);
            if (len > st.best) { st.best = len; st.best_start = st.run_start; }
            st.in_run = 0;
            pos += d + 1;
        } else {
            const uint64_t o = good >> pos;
            const int d = o ? __ffsll((long long)o) - 1 : 64;
            if (pos + d >= nbits) break;
            st.run_start = base + pos + d;
            st.in_run = 1;
            pos += d;
        }
    }
}

#define KVQ_TRIM_RPW 16   // records per wave
// the longest run of scores >= amin among line[0 .. Q) (the byte behind it closes the last run), the first of equally long
// ones, by all 64 lanes of a wave; the answer in every lane (kernels_bp.hip)
__device__ void kvq_long_line_run(const uint8_t *line, uint32_t Q, int amin, int lane, int &best, uint32_t &best_start);

// ---- a wave a record: the trim of one score line at one cutoff (kvq_profile_records, kvq_emit_size).  Both split their lines three
// ways in their own bodies -- 1024 scores and more: kvq_long_trim; 256 and more, and shorter ones: kvq_short_load and kvq_short_trim
// with sixteen and with four bytes a lane --, each for the reason its file gives ----
// a line of fewer than 64 NG - 1 bytes and its newline (qlen bytes with it): lane l holds bytes l, l + 64, ...
template <int NG>
__device__ __forceinline__ void kvq_short_load(const uint8_t *line, uint32_t qlen, int lane, uint8_t by[NG])
{
#pragma unroll
    for (int k = 0; k < NG; k++) {
        const uint32_t i = 64u * (uint32_t)k + (uint32_t)lane;
        by[k] = line[i < qlen ? i : qlen - 1u];                    // (unconditional loads travel together; qlen >= 1: the newline)
    }
}

// the engine's trim of a short score line (kvq_short_load has its bytes and its newline): kvq_trim_records' loop (the line's
// newline is fed too: it closes the last run when it is below the cutoff).  The longest run; its start in best_start
template <int NG>
__device__ __forceinline__ void kvq_short_trim(const uint8_t by[NG], uint32_t qlen, int amin, int lane, int &best, uint32_t &best_start)
{
    RunState st; st.in_run = 1; st.run_start = 0; st.best = 0; st.best_start = 0;
#pragma unroll
    for (int k = 0; k < NG; k++) {
        const uint32_t o = 64u * (uint32_t)k;
        if (o >= qlen) break;
        const uint64_t good = __ballot(o + (uint32_t)lane < qlen && (int)(int8_t)by[k] >= amin);
        run_feed(st, good, (qlen - o) < 64u ? (int)(qlen - o) : 64, o);
    }
    best = st.best; best_start = st.best_start;
}

// one behind the last byte of line[0, len) that is below amin; 0: there is none (the answer in every lane)
__device__ __forceinline__ uint32_t kvq_last_low(const uint8_t *line, uint32_t len, int amin, int lane)
{
    uint32_t last = 0;
    for (uint32_t o = 0; o < len; o += 1024u) {
        const uint32_t q = o + 16u * (uint32_t)lane;
        uint32_t w[4];
        kvq_load16(line, len, q, w);
        const uint32_t n = q < len ? (len - q < 16u ? len - q : 16u) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++)
            if (j < n && (int)(int8_t)(w[j >> 2] >> (8u * (j & 3u))) < amin) last = q + j + 1u;
    }
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)last, d, 64); last = o > last ? o : last; }
    return last;
}

// the trim of a score line of 1024 scores and more (a long read from BAM), as kvq_trim_records' long score lines go.
// kvq_long_line_run closes the last run at the end of what it is given: where the newline is no low byte, the line ends for it at
// its last low byte, which closes the last run that counts
__device__ __forceinline__ void kvq_long_trim(const uint8_t *sline, uint32_t Q, int amin, int lane, int &best, uint32_t &best_start)
{
    best = 0; best_start = 0u;
    uint32_t end = Q; bool closed = true;
    if ('\n' >= amin) { const uint32_t behind = kvq_last_low(sline, Q, amin, lane); closed = behind > 0u; end = behind - 1u; }
    if (closed) kvq_long_line_run(sline, end, amin, lane, best, best_start);
}
