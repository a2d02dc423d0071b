// kvarq_amd/csrc/kernels_records.hip -- the FastQ records of the hits (kvq_scan_set_records), gathered while the text is
// in device memory: the reference's `extract_hits` (kvarq/analyse.py:536-540) as an output of the scan instead of a second
// pass over the file.
//
// A hit's record is the bytes of the FastQ record whose bases line holds the hit's file_pos: from the first byte of its
// identifier line to the end of its quality line, that line's '\n' included (to the end of the text when it has no final
// newline).  All hits of one read share file_pos, so records are keyed by it and stored ONCE per read:
//   * kvq_gather_records, behind kvq_fold_batch over the same range of the arena: a lane per hit claims file_pos + 1 in an
//     open-addressing table (64-bit CAS, linear probing); the lane that claims a read finds its record's bounds, reserves
//     store space (one reservation per wave) and copies the bytes.  A record longer than a lane's walk or copy is handed to
//     the whole wave.
//   * kvq_record_lookup, behind the ordering (kernels_results.hip): per hit in canonical order, (offset, length) of its
//     record in the store.
//   * kvq_records_clear, wherever the arena is cleared: frees the slots the last scan claimed (the directory lists them).
// A pass that is thrown away (a batch whose speculated split failed validation, redone exhaustively) claims nothing: its
// range of the arena is closed empty by kvq_commit_batch before the gather runs.  And whatever claims a key, the key is a
// file_pos in the same text, so the bytes stored for it are the same by construction.
//
// This file is included by kvq_unity.hip after kernels_results.hip (KvqFinishState).

#include "kvq_host.h"
#include "kvq_lines.h"

#define KVQ_REC_LANE_STEPS 32u        // aligned 16-byte blocks a lane walks alone in each direction (512 bytes)
#define KVQ_REC_LANE_COPY 2048u       // records up to this many bytes a lane copies alone; longer ones the wave copies

struct KvqRecTable {
    unsigned long long *key;          // per slot: file_pos + 1, 0 = free
    unsigned long long *off;          // per slot: where the record's bytes start in the store
    unsigned int *len;                // per slot: the record's bytes
    unsigned int *dir;                // the slots claimed, in claim order (kvq_records_clear frees them)
    unsigned long long *ctr;          // [0] store bytes reserved (counts past store_cap), [1] slots claimed, [2] a probe went round the table
    uint8_t *store; unsigned long long store_cap;
    uint32_t mask;                    // slots - 1 (a power of two)
};

__device__ __forceinline__ uint32_t kvq_rec_hash(unsigned long long key, uint32_t mask)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// 16 bits: byte j of the aligned 16-byte block at data + b is '\n'
__device__ __forceinline__ uint32_t kvq_rec_nl16(const uint8_t *data, int64_t b)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(data + b);
    return kvq_flags16(kvq_nl_flags(v.x), kvq_nl_flags(v.y), kvq_nl_flags(v.z), kvq_nl_flags(v.w));
}

// One lane: the k-th newline in [lo, p).  Its offset; lo - 1 when the chunk begins first; -2 when `steps` blocks did not
// reach it.  Aligned blocks only, never in front of the batch's first byte.
__device__ int64_t kvq_rec_back(const uint8_t *data, int64_t lo, int64_t p, int k, uint32_t steps)
{
    if (p <= lo) return lo - 1;
    int64_t b = (p - 1) & ~15ll;
    uint32_t lim = (uint32_t)(p - b);
    for (uint32_t st = 0; st < steps; st++) {
        uint32_t m = kvq_rec_nl16(data, b);
        if (lim < 16u) m &= (1u << lim) - 1u;
        if (b < lo) m &= ~((1u << (uint32_t)(lo - b)) - 1u);
        while (m) { const int i = 31 - __clz(m); if (--k == 0) return b + i; m &= ~(1u << i); }
        if (b <= lo) return lo - 1;
        b -= 16; lim = 16u;
    }
    return -2;
}

// One lane: the k-th newline in [p, n).  Its offset; n when the chunk ends first; -2 when `steps` blocks did not reach it.
// Blocks that start at or behind n are not read.
__device__ int64_t kvq_rec_fwd(const uint8_t *data, int64_t n, int64_t p, int k, uint32_t steps)
{
    int64_t b = p & ~15ll;
    uint32_t skip = (uint32_t)(p - b);
    for (uint32_t st = 0; st < steps; st++) {
        if (b >= n) return n;
        uint32_t m = kvq_rec_nl16(data, b) & ~((1u << skip) - 1u);
        if (n - b < 16) m &= (1u << (uint32_t)(n - b)) - 1u;
        while (m) { const int i = __ffs(m) - 1; if (--k == 0) return b + i; m &= m - 1u; }
        b += 16; skip = 0;
    }
    return -2;
}

// The whole wave (all lanes active, same arguments): kvq_rec_back without a step limit, 1 KiB a step.
__device__ int64_t kvq_rec_back_wave(const uint8_t *data, int64_t lo, int64_t p, int k)
{
    if (p <= lo) return lo - 1;
    const int lane = kvq_lane();
    int64_t top = (p - 1) & ~15ll;
    for (;;) {
        const int64_t b = top - 16ll * lane;
        uint32_t m = 0;
        if (b + 16 > lo) {
            m = kvq_rec_nl16(data, b);
            if (b == top && p - top < 16) m &= (1u << (uint32_t)(p - top)) - 1u;
            if (b < lo) m &= ~((1u << (uint32_t)(lo - b)) - 1u);
        }
        const uint32_t c = (uint32_t)__popc(m), incl = kvq_wave_incl_scan(c);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (tot >= (uint32_t)k) {
            const bool here = incl >= (uint32_t)k && incl - c < (uint32_t)k;
            int64_t at = 0;
            if (here) {
                int r = k - (int)(incl - c);
                for (;;) { const int i = 31 - __clz(m); if (--r == 0) { at = b + i; break; } m &= ~(1u << i); }
            }
            return (int64_t)kvq_shfl64((unsigned long long)at, __ffsll((long long)__ballot(here)) - 1);
        }
        k -= (int)tot;
        if (top - 16ll * 63 <= lo) return lo - 1;
        top -= 1024;
    }
}

// The whole wave: kvq_rec_fwd without a step limit.
__device__ int64_t kvq_rec_fwd_wave(const uint8_t *data, int64_t n, int64_t p, int k)
{
    const int lane = kvq_lane();
    int64_t bot = p & ~15ll;
    for (;;) {
        if (bot >= n) return n;
        const int64_t b = bot + 16ll * lane;
        uint32_t m = 0;
        if (b < n) {
            m = kvq_rec_nl16(data, b);
            if (b <= p && p - b < 16) m &= ~((1u << (uint32_t)(p - b)) - 1u);      // (the block that holds p: only in the first step)
            if (n - b < 16) m &= (1u << (uint32_t)(n - b)) - 1u;
        }
        const uint32_t c = (uint32_t)__popc(m), incl = kvq_wave_incl_scan(c);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (tot >= (uint32_t)k) {
            const bool here = incl >= (uint32_t)k && incl - c < (uint32_t)k;
            int64_t at = 0;
            if (here) {
                int r = k - (int)(incl - c);
                for (;;) { const int i = __ffs(m) - 1; if (--r == 0) { at = b + i; break; } m &= m - 1u; }
            }
            return (int64_t)kvq_shfl64((unsigned long long)at, __ffsll((long long)__ballot(here)) - 1);
        }
        k -= (int)tot;
        bot += 1024;
    }
}

// The records of one batch's hits [*range_begin, min(*range_end, arena_cap)) of the arena, a lane per hit (see the head of
// this file).  Launched right behind kvq_fold_batch, before the batch's closing event: every guard on reusing the batch's
// text (staging slots, inflate run buffers) covers it.
extern "C" __global__ void __launch_bounds__(256)
kvq_gather_records(KvqRecTable T, const KvqHit *__restrict__ arena, uint32_t arena_cap, const uint8_t *__restrict__ data,
                   int64_t nbytes, int64_t fpos_base, const uint32_t *__restrict__ chunk_off, uint32_t nchunks,
                   const unsigned int *__restrict__ range_begin, const unsigned int *__restrict__ range_end)
{
    KVQ_BESIDE_SCAN();
    typedef uint32_t u32x4_any __attribute__((ext_vector_type(4), aligned(1)));
    const uint32_t h0 = *range_begin;
    uint32_t h1 = *range_end; if (h1 > arena_cap) h1 = arena_cap;
    const int lane = kvq_lane();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t hb = h0 + wave * 64u; hb < h1; hb += nwaves * 64u) {
        const uint32_t h = hb + (uint32_t)lane;
        bool mine = false;
        uint32_t slot = 0;
        int64_t p = 0;
        if (h < h1) {
            const int64_t fpos = arena[h].fpos;
            const unsigned long long key = (unsigned long long)fpos + 1ull;
            p = fpos - fpos_base;
            slot = kvq_rec_hash(key, T.mask);
            for (uint32_t probe = 0;; probe++) {
                if (probe > T.mask) { atomicMax(&T.ctr[2], 1ull); break; }        // (cannot happen: slots >= 2 x arena_cap)
                const unsigned long long k = T.key[slot];
                if (k == key) break;
                if (k == 0ull) {
                    const unsigned long long was = atomicCAS(&T.key[slot], 0ull, key);
                    if (was == 0ull) { mine = true; break; }
                    if (was == key) break;
                }
                slot = (slot + 1u) & T.mask;
            }
        }
        // bounds: the second newline in front of p (the end of the record before), the third at or behind it (the end of
        // the quality line), inside the chunk that holds p (chunks begin at record starts: a record never crosses one);
        // a lane walks 512 bytes each way, what is farther is the wave's
        int64_t rs = 0, re = 0, lo = 0, hi = nbytes;
        bool far = false;
        if (mine) {
            if (nchunks && p >= (int64_t)chunk_off[0] && p < (int64_t)chunk_off[nchunks]) {
                uint32_t a = 0, b = nchunks;                                     // chunk_off[a] <= p < chunk_off[b]
                while (b - a > 1u) { const uint32_t m = (a + b) >> 1; if ((int64_t)chunk_off[m] <= p) a = m; else b = m; }
                lo = chunk_off[a]; hi = chunk_off[b];
            }
            const int64_t a = kvq_rec_back(data, lo, p, 2, KVQ_REC_LANE_STEPS);
            const int64_t e = a == -2 ? -2 : kvq_rec_fwd(data, hi, p, 3, KVQ_REC_LANE_STEPS);
            far = a == -2 || e == -2;
            rs = a + 1; re = e == hi ? hi : e + 1;
        }
        for (uint64_t todo = __ballot(far); todo; todo &= todo - 1ull) {
            const int w = __ffsll((long long)todo) - 1;
            const int64_t pw = (int64_t)kvq_shfl64((unsigned long long)p, w), low = (int64_t)kvq_shfl64((unsigned long long)lo, w), hiw = (int64_t)kvq_shfl64((unsigned long long)hi, w);
            const int64_t a = kvq_rec_back_wave(data, low, pw, 2), e = kvq_rec_fwd_wave(data, hiw, pw, 3);
            if (lane == w) { rs = a + 1; re = e == hiw ? hiw : e + 1; }
        }
        // store space: short records with one reservation per wave, long ones each with its own; a directory entry each
        const uint64_t len = mine ? (uint64_t)(re - rs) : 0ull;
        const bool longrec = len > KVQ_REC_LANE_COPY;
        const uint32_t short_len = mine && !longrec ? (uint32_t)len : 0u;
        const uint32_t incl = kvq_wave_incl_scan(short_len);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint64_t claimed = __ballot(mine);
        unsigned long long base = 0, dbase = 0;
        if (lane == 0) {
            if (tot) base = atomicAdd(&T.ctr[0], (unsigned long long)tot);
            if (claimed) dbase = atomicAdd(&T.ctr[1], (unsigned long long)__popcll(claimed));
        }
        base = kvq_shfl64(base, 0);
        dbase = kvq_shfl64(dbase, 0);
        unsigned long long off = base + incl - short_len;
        if (longrec) off = atomicAdd(&T.ctr[0], (unsigned long long)len);
        const bool fits = off + len <= T.store_cap;
        if (mine) {
            T.off[slot] = off; T.len[slot] = (unsigned int)len;
            const unsigned long long d = dbase + (unsigned long long)__popcll(claimed & kvq_lanemask_lt());
            if (d <= T.mask) T.dir[d] = slot;
        }
        if (mine && !longrec && fits) {
            const uint8_t *src = data + rs;
            uint8_t *dst = T.store + off;
            uint32_t q = 0;
            for (; q + 16u <= (uint32_t)len; q += 16u) *reinterpret_cast<u32x4_any *>(dst + q) = *reinterpret_cast<const u32x4_any *>(src + q);
            for (; q < (uint32_t)len; q++) dst[q] = src[q];
        }
        for (uint64_t todo = __ballot(longrec && fits); todo; todo &= todo - 1ull) {
            const int w = __ffsll((long long)todo) - 1;
            const uint8_t *src = data + (int64_t)kvq_shfl64((unsigned long long)rs, w);
            uint8_t *dst = T.store + kvq_shfl64(off, w);
            const uint64_t n = kvq_shfl64(len, w), body = n & ~15ull;
            for (uint64_t q = 16ull * (uint64_t)lane; q < body; q += 1024ull)
                *reinterpret_cast<u32x4_any *>(dst + q) = *reinterpret_cast<const u32x4_any *>(src + q);
            if (body + (uint64_t)lane < n) dst[body + lane] = src[body + lane];
        }
    }
}

// per hit in canonical order (the file_pos column the ordering left in the result buffer): its record's place in the store
extern "C" __global__ void __launch_bounds__(256)
kvq_record_lookup(KvqRecTable T, const KvqFinishState *__restrict__ st, const uint8_t *__restrict__ res,
                  long long *__restrict__ out_off, int32_t *__restrict__ out_len)
{
    KVQ_BESIDE_SCAN();
    const uint32_t n = st->n;
    const long long *fpos = reinterpret_cast<const long long *>(res + st->L.file_pos);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long key = (unsigned long long)fpos[i] + 1ull;
        uint32_t slot = kvq_rec_hash(key, T.mask);
        long long o = -1; int32_t l = 0;
        for (uint32_t probe = 0; probe <= T.mask; probe++) {
            const unsigned long long k = T.key[slot];
            if (k == key) { o = (long long)T.off[slot]; l = (int32_t)T.len[slot]; break; }
            if (k == 0ull) break;
            slot = (slot + 1u) & T.mask;
        }
        out_off[i] = o; out_len[i] = l;
    }
}

// frees the slots the last scan claimed (the counters are zeroed behind it, on the same stream)
extern "C" __global__ void __launch_bounds__(256)
kvq_records_clear(KvqRecTable T)
{
    KVQ_BESIDE_SCAN();
    unsigned long long n = T.ctr[1];
    if (n > (unsigned long long)T.mask + 1ull) n = (unsigned long long)T.mask + 1ull;
    for (unsigned long long i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) T.key[T.dir[i]] = 0ull;
}
