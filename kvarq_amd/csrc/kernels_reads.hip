// kvarq_amd/csrc/kernels_reads.hip -- what the individual reads of a batch look like (include/kvarq_hip.h): the
// per-read GC share, mean quality and N count as three histograms, and the duplication of the reads' first 64 bases in a hash
// table on the device.  kvq_reads_records walks the record index of the exhaustive path (kvq_index_records), as
// kvq_profile_records does; it reads the text only inside its records and writes nothing but its array and the table.
// kvq_dup_plan / kvq_dup_purge settle the table behind every slice of records, kvq_dup_levels reads it out in the tail of a scan.
#include "kvq_device.h"
#include "kvq_lines.h"
#include "kvq_dup_hash.h"
#include "../../include/kvarq_hip.h"

// the table's small state block: 64-bit words
struct KvqDupState {
    enum { LEVEL = 0, NEW_LEVEL = 1, ACTIVE = 2, DISTINCT = 3, KEYED = 4, UNKEYED = 5, PLAN_DONE = 6, PURGE_DONE = 7, MOVED = 8,
           TZ = 16,                      // 65 words: keys of the table by the trailing zero bits of their hash (kvq_dup_plan's scratch)
           WORDS = 96 };
};
// two tables of 2^lg slots {hash, count} (linear probing cannot delete in place: a purge moves the keys it keeps to the other
// one), the state block.  The table that is not active is all zero.
struct KvqDupTable { unsigned long long *state, *tab[2]; uint32_t lg; };

// where the pieces lie inside a workgroup's LDS: the three histograms (32-bit bins: a batch is < 4 GiB), then the scalars
struct KvqReadsLds {
    static constexpr uint32_t GC = 0, MEANQ = 101, NCOUNT = 357, BINS = 613,
                              S_RECORDS = 613, S_GC_NONE = 614, S_MEANQ_NONE = 615, S_KEYED = 616, S_UNKEYED = 617, S_NEW = 618, WORDS = 619;
};

// the bytes of word d of a piece that are among its first `nvalid`
__device__ __forceinline__ uint32_t reads_keep(uint32_t nvalid, uint32_t d)
{
    return kvq_keep_bytes(nvalid > 4u * d ? nvalid - 4u * d : 0u);
}
// A C G T, G C and N among the bytes of a piece of a bases line (a zero, a newline and a '\r' are none of them)
__device__ __forceinline__ void reads_count_bases(const uint32_t w[4], uint32_t &a, uint32_t &g, uint32_t &c)
{
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t gc = kvq_eq_flags(w[d], 0x47474747u) | kvq_eq_flags(w[d], 0x43434343u);
        a += (uint32_t)__popc(gc | kvq_eq_flags(w[d], 0x41414141u) | kvq_eq_flags(w[d], 0x54545454u));
        g += (uint32_t)__popc(gc);
        c += (uint32_t)__popc(kvq_eq_flags(w[d], 0x4E4E4E4Eu));
    }
}
// the sum of the first nvalid bytes of a piece, as unsigned
__device__ __forceinline__ uint32_t reads_sum(const uint32_t w[4], uint32_t nvalid)
{
    uint32_t s = 0;
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        const uint32_t x = w[d] & reads_keep(nvalid, d);
        s += (x & 0x00FF00FFu) + ((x >> 8) & 0x00FF00FFu);
    }
    return (s & 0xFFFFu) + (s >> 16);
}
// the parts (kvq_dup_word) of key words 2 sub and 2 sub + 1, from bytes [16 sub, 16 sub + 16) of the bases line; sub < 4
__device__ __forceinline__ unsigned long long reads_key_parts(const uint32_t w[4], uint32_t nkey, uint32_t sub)
{
    const uint32_t kv = nkey > 16u * sub ? nkey - 16u * sub : 0u;
    const unsigned long long lo = (unsigned long long)(w[0] & reads_keep(kv, 0)) | (unsigned long long)(w[1] & reads_keep(kv, 1)) << 32;
    const unsigned long long hi = (unsigned long long)(w[2] & reads_keep(kv, 2)) | (unsigned long long)(w[3] & reads_keep(kv, 3)) << 32;
    return kvq_dup_word(lo, 2u * sub) ^ kvq_dup_word(hi, 2u * sub + 1u);
}

// `n` more copies of key h into a table of 2^lg slots: the slot from the HIGH bits of h, linear probing.  The host's slices keep the
// table at most three-quarters full, so a free slot is always met (the bound on the probes only keeps a broken table from hanging
// the device).  Returns 1 when the key is new.
__device__ __forceinline__ uint32_t dup_insert(unsigned long long *tab, uint32_t lg, unsigned long long h, unsigned long long n)
{
    const unsigned long long C = 1ull << lg;
    unsigned long long slot = h >> (64u - lg);
    for (unsigned long long probe = 0; probe < C; probe++) {
        const unsigned long long old = atomicCAS(&tab[2ull * slot], 0ull, h);
        if (old == 0ull || old == h) {
            atomicAdd(&tab[2ull * slot + 1ull], n);
            return old == 0ull ? 1u : 0u;
        }
        slot = (slot + 1ull) & (C - 1ull);
    }
    return 0u;
}

// Records [rec0, rec1) of the batch (a slice: at most a quarter of the table's slots when the duplication is on).  A QUARTER-WAVE
// A RECORD: sixteen lanes take a line 256 bytes a step, sixteen bytes a lane -- a 150-base read is one step for each of its two
// lines, and the four records of a wave have their loads in flight together.  A record with a line of 1024 bytes and more is
// walked by the whole wave, a KiB a step, as kvq_profile_records walks it.  mode: bit 0 the distributions (reads: the array of
// include/kvarq_hip.h), bit 1 the duplication (T).  Grid-stride over waves.
extern "C" __global__ void __launch_bounds__(256)
kvq_reads_records(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t rec0, uint32_t rec1, uint32_t mode,
                  unsigned long long *__restrict__ reads, KvqDupTable T)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned int lds[KvqReadsLds::WORDS];
    const bool stats = (mode & 1u) != 0u, dup = (mode & 2u) != 0u;
    for (uint32_t i = threadIdx.x; i < KvqReadsLds::WORDS; i += blockDim.x) lds[i] = 0u;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t quarter = (uint32_t)lane >> 4, sub = (uint32_t)lane & 15u;
    uint32_t level = 0; unsigned long long *tab = nullptr;
    if (dup) { level = (uint32_t)T.state[KvqDupState::LEVEL]; tab = T.tab[T.state[KvqDupState::ACTIVE] & 1ull]; }

    // (what a quarter's first lane keeps for its records)
    uint32_t mine = 0, gc_none = 0, meanq_none = 0, no_n = 0, keyed = 0, unkeyed = 0, newkeys = 0;
    unsigned long long pend_h = 0, pend_n = 0;          // equal keys in a row are counted first: one add for the run
    for (uint64_t g0 = (uint64_t)rec0 + ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; g0 < rec1; g0 += (uint64_t)gridDim.x * 16u) {
        const uint64_t g = g0 + quarter;
        const bool have = g < rec1;
        uint32_t n[4] = { 0u, 1u, 1u, 2u };              // (behind the last record: two empty lines)
        if (have) __builtin_memcpy(n, nl4 + 4u * (size_t)g, 16);
        const uint32_t boff = n[0] + 1u, L = n[1] - n[0] - 1u, soff = n[2] + 1u, Q = stats ? n[3] - n[2] - 1u : 0u;
        const bool is_long = L >= 1024u || Q >= 1024u;
        uint32_t a = 0, gc = 0, c = 0, crb = 0, crs = 0;
        unsigned long long S = 0, parts = 0;
        {
            // the quarter's own record, both lines below 1024 bytes
            const bool here = have && !is_long;
            const uint8_t *bline = data + boff, *sline = data + soff;
            const uint32_t bl = here ? L : 0u, sl = here ? Q : 0u;
            if (bl) crb = bline[bl - 1u] == '\r';
            if (sl) crs = sline[sl - 1u] == '\r';
            const uint32_t nkey = bl - crb < KVQ_DUP_KEY_BYTES ? bl - crb : KVQ_DUP_KEY_BYTES;
            const uint32_t top = bl > sl ? bl : sl;
            uint32_t s32 = 0;
            for (uint32_t o = 0; o < top; o += 256u) {
                const uint32_t q = o + 16u * sub;
                uint32_t bw[4], sw[4];
                kvq_load16(bline, bl, q, bw);
                kvq_load16(sline, sl, q, sw);
                reads_count_bases(bw, a, gc, c);
                if (dup && o == 0u && sub < 4u) parts = reads_key_parts(bw, nkey, sub);
                s32 += reads_sum(sw, q < sl ? (sl - q < 16u ? sl - q : 16u) : 0u);
            }
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                a += (uint32_t)__shfl_xor((int)a, d, 64); gc += (uint32_t)__shfl_xor((int)gc, d, 64); c += (uint32_t)__shfl_xor((int)c, d, 64);
                s32 += (uint32_t)__shfl_xor((int)s32, d, 64);
                if (dup) parts ^= kvq_shfl_xor64(parts, d);
            }
            S = s32;
        }
        // the records with a long line: the whole wave, one after the other (the same for every lane)
        unsigned long long longs = __ballot(have && is_long);
        while (longs) {
            const int l = __ffsll((long long)longs) - 1;
            longs &= ~(0xFFFFull << (l & ~15));
            const uint32_t rL = (uint32_t)__shfl((int)L, l, 64), rQ = (uint32_t)__shfl((int)Q, l, 64);
            const uint8_t *bline = data + (uint32_t)__shfl((int)boff, l, 64), *sline = data + (uint32_t)__shfl((int)soff, l, 64);
            const uint32_t cb = rL && bline[rL - 1u] == '\r', cs = rQ && sline[rQ - 1u] == '\r';
            const uint32_t nkey = rL - cb < KVQ_DUP_KEY_BYTES ? rL - cb : KVQ_DUP_KEY_BYTES;
            uint32_t a2 = 0, g2 = 0, c2 = 0;
            unsigned long long S2 = 0, p2 = 0;
            for (uint32_t o = 0; o < rL; o += 1024u) {
                const uint32_t q = o + 16u * (uint32_t)lane;
                uint32_t w[4];
                kvq_load16(bline, rL, q, w);
                reads_count_bases(w, a2, g2, c2);
                if (dup && o == 0u && lane < 4) p2 = reads_key_parts(w, nkey, (uint32_t)lane);
                if (o + 1024u < o) break;                                   // (a line that ends in the last KiB below 4 GiB)
            }
            for (uint32_t o = 0; o < rQ; o += 1024u) {
                const uint32_t q = o + 16u * (uint32_t)lane;
                uint32_t w[4];
                kvq_load16(sline, rQ, q, w);
                S2 += reads_sum(w, q < rQ ? (rQ - q < 16u ? rQ - q : 16u) : 0u);
                if (o + 1024u < o) break;
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                a2 += (uint32_t)__shfl_xor((int)a2, d, 64); g2 += (uint32_t)__shfl_xor((int)g2, d, 64); c2 += (uint32_t)__shfl_xor((int)c2, d, 64);
                S2 += kvq_shfl_xor64(S2, d);
                p2 ^= kvq_shfl_xor64(p2, d);
            }
            if (quarter == (uint32_t)l >> 4) { a = a2; gc = g2; c = c2; S = S2; parts = p2; crb = cb; crs = cs; }
        }
        if (have && sub == 0u) {
            mine++;
            if (stats) {
                // the trailing '\r' is no byte of its line: none of A C G T N, so only the scores have counted it
                const uint32_t nq = Q - crs;
                const unsigned long long Sq = S - 13ull * crs;
                if (a) {
                    const uint32_t k = a < (1u << 24) ? (200u * gc + a) / (2u * a) : (uint32_t)((200ull * gc + a) / (2ull * a));
                    atomicAdd(&lds[KvqReadsLds::GC + k], 1u);
                } else gc_none++;
                if (nq) {
                    const uint32_t b = nq < (1u << 22) ? (2u * (uint32_t)Sq + nq) / (2u * nq) : (uint32_t)((2ull * Sq + nq) / (2ull * nq));
                    atomicAdd(&lds[KvqReadsLds::MEANQ + b], 1u);
                } else meanq_none++;
                if (c) atomicAdd(&lds[KvqReadsLds::NCOUNT + (c < 255u ? c : 255u)], 1u);
                else no_n++;
            }
            if (dup) {
                const uint32_t Lk = L - crb;
                if (!Lk) unkeyed++;
                else {
                    keyed++;
                    const unsigned long long h = kvq_dup_close(Lk < KVQ_DUP_KEY_BYTES ? Lk : KVQ_DUP_KEY_BYTES, parts);
                    if (kvq_dup_tracked(h, level)) {
                        if (h == pend_h) pend_n++;
                        else {
                            if (pend_n) newkeys += dup_insert(tab, T.lg, pend_h, pend_n);
                            pend_h = h; pend_n = 1;
                        }
                    }
                }
            }
        }
    }
    if (pend_n) newkeys += dup_insert(tab, T.lg, pend_h, pend_n);
    if (sub == 0u && mine) {
        atomicAdd(&lds[KvqReadsLds::S_RECORDS], mine);
        if (gc_none) atomicAdd(&lds[KvqReadsLds::S_GC_NONE], gc_none);
        if (meanq_none) atomicAdd(&lds[KvqReadsLds::S_MEANQ_NONE], meanq_none);
        if (no_n) atomicAdd(&lds[KvqReadsLds::NCOUNT], no_n);
        if (keyed) atomicAdd(&lds[KvqReadsLds::S_KEYED], keyed);
        if (unkeyed) atomicAdd(&lds[KvqReadsLds::S_UNKEYED], unkeyed);
        if (newkeys) atomicAdd(&lds[KvqReadsLds::S_NEW], newkeys);
    }
    __syncthreads();
    // the workgroup's bins that are not zero -> the array, the table's counts -> its state block
    if (stats) {
        for (uint32_t i = threadIdx.x; i < KvqReadsLds::BINS; i += blockDim.x)
            if (lds[i]) atomicAdd(&reads[KVQ_READS_GC + i], (unsigned long long)lds[i]);
        if (threadIdx.x < 3u && lds[KvqReadsLds::S_RECORDS + threadIdx.x])
            atomicAdd(&reads[KVQ_READS_RECORDS + threadIdx.x], (unsigned long long)lds[KvqReadsLds::S_RECORDS + threadIdx.x]);
    }
    if (dup && threadIdx.x == 0) {
        if (lds[KvqReadsLds::S_KEYED]) atomicAdd(&T.state[KvqDupState::KEYED], (unsigned long long)lds[KvqReadsLds::S_KEYED]);
        if (lds[KvqReadsLds::S_UNKEYED]) atomicAdd(&T.state[KvqDupState::UNKEYED], (unsigned long long)lds[KvqReadsLds::S_UNKEYED]);
        if (lds[KvqReadsLds::S_NEW]) atomicAdd(&T.state[KvqDupState::DISTINCT], (unsigned long long)lds[KvqReadsLds::S_NEW]);
    }
}

// ---- the settle behind every slice: fixed grids that read what there is to do from the state block (no host round trip) ----
#define KVQ_DUP_GRID_MAX 1024u

// More than half the slots taken: count the table's keys by the trailing zero bits of their hash and pick the smallest level
// above the present one that leaves at most half (the keys tracked at level s are those with s trailing zero bits and more).
// Returns at once otherwise.  The workgroup that ends last decides.
extern "C" __global__ void __launch_bounds__(256)
kvq_dup_plan(KvqDupTable T)
{
    __shared__ unsigned int tz[65];
    __shared__ unsigned int last;
    unsigned long long *const st = T.state;
    const unsigned long long C = 1ull << T.lg;
    if (st[KvqDupState::DISTINCT] <= C / 2ull) return;            // (nothing in this kernel writes the word: the same for every workgroup)
    if (threadIdx.x < 65u) tz[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long *tab = T.tab[st[KvqDupState::ACTIVE] & 1ull];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long h = tab[2ull * i];
        if (h) atomicAdd(&tz[__ffsll((long long)h) - 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 65u && tz[threadIdx.x]) atomicAdd(&st[KvqDupState::TZ + threadIdx.x], (unsigned long long)tz[threadIdx.x]);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(&st[KvqDupState::PLAN_DONE], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1u : 0u;
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    const uint32_t level = (uint32_t)st[KvqDupState::LEVEL];
    unsigned long long above = 0;                                 // keys with s trailing zero bits and more (every key has `level` of them)
    for (int t = 0; t < 65; t++) above += atomicAdd(&st[KvqDupState::TZ + t], 0ull);
    uint32_t s = 0;
    while (s < 64u && (s <= level || above > C / 2ull)) { above -= atomicAdd(&st[KvqDupState::TZ + s], 0ull); s++; }
    st[KvqDupState::NEW_LEVEL] = s;
    for (int t = 0; t < 65; t++) st[KvqDupState::TZ + t] = 0ull;
    st[KvqDupState::PLAN_DONE] = 0ull;
}

// The level has moved: the keys of the new level go, with their counts, into the other table, every slot of the old one is left
// zero, and the workgroup that ends last makes the other table the active one.  Returns at once otherwise.
extern "C" __global__ void __launch_bounds__(256)
kvq_dup_purge(KvqDupTable T)
{
    __shared__ unsigned int moved;
    __shared__ unsigned int last;
    unsigned long long *const st = T.state;
    const uint32_t level = (uint32_t)st[KvqDupState::LEVEL], to = (uint32_t)st[KvqDupState::NEW_LEVEL];
    if (to == level) return;                 // (the two words change only once every other workgroup has ended: the same for all)
    const unsigned long long C = 1ull << T.lg;
    const uint32_t active = (uint32_t)(st[KvqDupState::ACTIVE] & 1ull);
    unsigned long long *const src = T.tab[active], *const dst = T.tab[active ^ 1u];
    if (threadIdx.x == 0) moved = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long h = src[2ull * i];
        if (!h) continue;
        const unsigned long long n = src[2ull * i + 1ull];
        src[2ull * i] = 0ull; src[2ull * i + 1ull] = 0ull;
        if (kvq_dup_tracked(h, to)) mine += dup_insert(dst, T.lg, h, n);
    }
    if (mine) atomicAdd(&moved, mine);
    __syncthreads();
    if (threadIdx.x == 0 && moved) atomicAdd(&st[KvqDupState::MOVED], (unsigned long long)moved);
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) last = atomicAdd(&st[KvqDupState::PURGE_DONE], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1u : 0u;
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    st[KvqDupState::DISTINCT] = atomicAdd(&st[KvqDupState::MOVED], 0ull);
    st[KvqDupState::MOVED] = 0ull;
    st[KvqDupState::LEVEL] = to;
    st[KvqDupState::ACTIVE] = active ^ 1u;
    st[KvqDupState::PURGE_DONE] = 0ull;
}

// the tail of a scan: the result array of include/kvarq_hip.h from the active table (out: zero when the kernel starts)
extern "C" __global__ void __launch_bounds__(256)
kvq_dup_levels(KvqDupTable T, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long bins[32];              // distinct[16], records[16]
    const unsigned long long *const st = T.state;
    const unsigned long long C = 1ull << T.lg;
    if (threadIdx.x < 32u) bins[threadIdx.x] = 0ull;
    __syncthreads();
    const unsigned long long *tab = T.tab[st[KvqDupState::ACTIVE] & 1ull];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256ull) {
        if (!tab[2ull * i]) continue;
        const unsigned long long n = tab[2ull * i + 1ull];
        const uint32_t b = kvq_dup_bin(n);
        atomicAdd(&bins[b], 1ull);
        atomicAdd(&bins[16u + b], n);
    }
    __syncthreads();
    if (threadIdx.x < 32u && bins[threadIdx.x]) {
        atomicAdd(&out[KVQ_DUP_DISTINCT + threadIdx.x], bins[threadIdx.x]);            // (the records' row lies behind the distinct keys')
        atomicAdd(&out[threadIdx.x < 16u ? KVQ_DUP_TRACKED_KEYS : KVQ_DUP_TRACKED_RECORDS], bins[threadIdx.x]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[KVQ_DUP_LEVEL] = st[KvqDupState::LEVEL]; out[KVQ_DUP_SLOTS] = C;
        out[KVQ_DUP_KEYED] = st[KvqDupState::KEYED]; out[KVQ_DUP_UNKEYED] = st[KvqDupState::UNKEYED];
    }
}
