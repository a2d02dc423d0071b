// kvarq_amd/csrc/kernels_over.hip -- the overrepresented sequences of an input (include/kvarq_hip.h): the keys of
// the scan's first M records are the candidates, every candidate is counted through the whole input, and the tail of a scan lists
// those with a share of 0.1 % and more.  kvq_over_records walks the record index of the exhaustive path (kvq_index_records), as
// the other input passes do; it reads the first 64 bytes and the last byte of every bases line, never a byte outside its record,
// and writes nothing but the table and its state block.  kvq_over_select reads the table out.  The key and its hash are the
// duplication's (kvq_dup_hash.h); beyond it and the line helpers of kvq_lines.h nothing is shared with kernels_reads.hip.
#include "kvq_device.h"
#include "kvq_lines.h"
#include "kvq_dup_hash.h"
#include "../../include/kvarq_hip.h"

// the table's small state block: 64-bit words
struct KvqOverState { enum { KEYED = 0, UNKEYED = 1, WORDS = 8 }; };
// 2^lg slots of KVQ_OVER_ROW_WORDS words each, laid out as a row of the result is: {hash, count, n, w0 .. w7}; hash 0: empty.
// At most M keys ever go into the 4 M slots and more: a free slot is always met, and there is no overflow path
struct KvqOverTable { unsigned long long *state, *slots; uint32_t lg; };

// INSERT: `n` more copies of candidate h.  The slot from the HIGH bits of h, linear probing; *won: the caller has taken an empty
// slot and owes it the key's length and bytes.  (The bound on the probes only keeps a broken table from hanging the device.)
__device__ __forceinline__ unsigned long long over_insert(const KvqOverTable T, unsigned long long h, unsigned long long n, uint32_t *won)
{
    const unsigned long long C = 1ull << T.lg;
    unsigned long long slot = h >> (64u - T.lg);
    for (unsigned long long probe = 0; probe < C; probe++) {
        unsigned long long *row = T.slots + slot * KVQ_OVER_ROW_WORDS;
        const unsigned long long old = atomicCAS(&row[KVQ_OVER_ROW_HASH], 0ull, h);
        if (old == 0ull || old == h) {
            atomicAdd(&row[KVQ_OVER_ROW_COUNT], n);
            *won = old == 0ull ? 1u : 0u;
            return slot;
        }
        slot = (slot + 1ull) & (C - 1ull);
    }
    *won = 0u;
    return 0ull;
}
// LOOKUP: `n` more copies of key h when it is a candidate -- probe to the hash or to the first empty slot; nothing is written otherwise
// (no hash word changes while a LOOKUP launch runs: the two modes are never on the device together)
__device__ __forceinline__ void over_count(const KvqOverTable T, unsigned long long h, unsigned long long n)
{
    const unsigned long long C = 1ull << T.lg;
    unsigned long long slot = h >> (64u - T.lg);
    for (unsigned long long probe = 0; probe < C; probe++) {
        unsigned long long *row = T.slots + slot * KVQ_OVER_ROW_WORDS;
        const unsigned long long v = row[KVQ_OVER_ROW_HASH];
        if (v == h) { atomicAdd(&row[KVQ_OVER_ROW_COUNT], n); return; }
        if (v == 0ull) return;
        slot = (slot + 1ull) & (C - 1ull);
    }
}

// Records [rec0, rec1) of the batch.  FOUR LANES A RECORD, sixteen records a wave: the key is at most four 16-byte pieces, so a
// lane loads one piece (and every lane of the four the line's last byte, for the '\r' rule), hashes the two key words it holds, the
// four XOR their parts and kvq_dup_close finishes -- the split of kvq_reads_records, without the twelve lanes of its sixteen that
// would hold nothing here.  The sixteen records of a wave have their loads and their probes in flight together.
// insert != 0: the records are among the scan's first M -- their keys become candidates (atomicCAS on the hash word; the four lanes
// of the record that took the slot store n and the key bytes; atomicAdd on the count).  insert == 0: the rest of the input -- a
// lookup, an add on a match, no store otherwise.  The records of a wave that share the key of its first keyed record are counted
// with one add, and in a lookup so are equal keys in a row of a lane's records.  Keyed and unkeyed records -> the state block, one
// atomic per word and workgroup.  Grid-stride over waves.
extern "C" __global__ void __launch_bounds__(256)
kvq_over_records(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t rec0, uint32_t rec1, uint32_t insert, KvqOverTable T)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned int lds[2];                     // keyed, unkeyed
    if (threadIdx.x < 2u) lds[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t grp = (uint32_t)lane >> 2, sub = (uint32_t)lane & 3u;
    uint32_t keyed = 0, unkeyed = 0;                    // (what a record's first lane keeps)
    unsigned long long pend_h = 0, pend_n = 0;
    for (uint64_t g0 = (uint64_t)rec0 + ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 16u; g0 < rec1; g0 += (uint64_t)gridDim.x * 64u) {
        const uint64_t g = g0 + grp;
        const bool have = g < rec1;
        uint32_t n[2] = { 0u, 1u };                      // (behind the last record: an empty line)
        if (have) __builtin_memcpy(n, nl4 + 4u * (size_t)g, 8);
        const uint8_t *line = data + n[0] + 1u;
        const uint32_t L = n[1] - n[0] - 1u;
        const uint32_t cr = L && line[L - 1u] == '\r' ? 1u : 0u;
        const uint32_t Lk = L - cr, nkey = Lk < KVQ_DUP_KEY_BYTES ? Lk : KVQ_DUP_KEY_BYTES;
        uint32_t w[4];
        kvq_load16(line, L, 16u * sub, w);
        const uint32_t kv = nkey > 16u * sub ? nkey - 16u * sub : 0u;          // key bytes in this lane's piece and behind it
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) w[d] &= kvq_keep_bytes(kv > 4u * d ? kv - 4u * d : 0u);
        const unsigned long long lo = (unsigned long long)w[0] | (unsigned long long)w[1] << 32, hi = (unsigned long long)w[2] | (unsigned long long)w[3] << 32;
        unsigned long long parts = kvq_dup_word(lo, 2u * sub) ^ kvq_dup_word(hi, 2u * sub + 1u);
        parts ^= kvq_shfl_xor64(parts, 1);
        parts ^= kvq_shfl_xor64(parts, 2);
        const bool first = have && sub == 0u, key = first && Lk != 0u;
        const unsigned long long h = kvq_dup_close(nkey, parts);
        if (first) { if (Lk) keyed++; else unkeyed++; }
        // the records of the wave with the key of its first keyed record: one add for all of them, by the first
        const unsigned long long keys = __ballot(key);
        unsigned long long mult = key ? 1ull : 0ull;
        if (keys) {
            const int l0 = __ffsll((long long)keys) - 1;
            const unsigned long long h0 = kvq_shfl64(h, l0);
            const unsigned long long same = __ballot(key && h == h0);
            if (same >> lane & 1ull) mult = lane == l0 ? (unsigned long long)__popcll(same) : 0ull;
        }
        if (insert) {
            uint32_t won = 0; unsigned long long slot = 0;
            if (mult) slot = over_insert(T, h, mult, &won);
            won = (uint32_t)__shfl((int)won, lane & ~3, 64);
            slot = kvq_shfl64(slot, lane & ~3);
            if (won) {
                unsigned long long *row = T.slots + slot * KVQ_OVER_ROW_WORDS;
                if (sub == 0u) row[KVQ_OVER_ROW_N] = nkey;
                row[KVQ_OVER_ROW_KEY + 2u * sub] = lo; row[KVQ_OVER_ROW_KEY + 2u * sub + 1u] = hi;
            }
        } else if (mult) {
            if (h == pend_h) pend_n += mult;
            else {
                if (pend_n) over_count(T, pend_h, pend_n);
                pend_h = h; pend_n = mult;
            }
        }
    }
    if (pend_n) over_count(T, pend_h, pend_n);
    if (keyed) atomicAdd(&lds[0], keyed);
    if (unkeyed) atomicAdd(&lds[1], unkeyed);
    __syncthreads();
    if (threadIdx.x < 2u && lds[threadIdx.x]) atomicAdd(&T.state[KvqOverState::KEYED + threadIdx.x], (unsigned long long)lds[threadIdx.x]);
}

#define KVQ_OVER_GRID_MAX 1024u

// the tail of a scan: the result array of include/kvarq_hip.h from the table (out: zero when the kernel starts).  The candidates
// and their records are summed, and every slot that is LISTED -- count >= 2 and 1000 count >= keyed -- appends its row: the
// counts sum to at most `keyed`, so no more than KVQ_OVER_MAX_ROWS slots can be (the bound on the index only keeps a broken
// table inside the array).  The rows land in no order: the host sorts them.  Fixed grid.
extern "C" __global__ void __launch_bounds__(256)
kvq_over_select(KvqOverTable T, unsigned long long M, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long sums[2];               // candidates, their records
    const unsigned long long C = 1ull << T.lg, keyed = T.state[KvqOverState::KEYED];
    if (threadIdx.x < 2u) sums[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long cand = 0, counted = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < C; i += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long *row = T.slots + i * KVQ_OVER_ROW_WORDS;
        if (!row[KVQ_OVER_ROW_HASH]) continue;
        const unsigned long long c = row[KVQ_OVER_ROW_COUNT];
        cand++; counted += c;
        if (c >= 2ull && 1000ull * c >= keyed) {
            const unsigned long long at = atomicAdd(&out[KVQ_OVER_LISTED], 1ull);
            if (at < (unsigned long long)KVQ_OVER_MAX_ROWS)
                for (uint32_t k = 0; k < (uint32_t)KVQ_OVER_ROW_WORDS; k++) out[KVQ_OVER_ROWS + at * KVQ_OVER_ROW_WORDS + k] = row[k];
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { cand += kvq_shfl_xor64(cand, d); counted += kvq_shfl_xor64(counted, d); }
    if (kvq_lane() == 0 && cand) { atomicAdd(&sums[0], cand); atomicAdd(&sums[1], counted); }
    __syncthreads();
    if (threadIdx.x < 2u && sums[threadIdx.x]) atomicAdd(&out[KVQ_OVER_CANDIDATES + threadIdx.x], sums[threadIdx.x]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[KVQ_OVER_M] = M; out[KVQ_OVER_SLOTS] = C;
        out[KVQ_OVER_KEYED] = keyed; out[KVQ_OVER_UNKEYED] = T.state[KvqOverState::UNKEYED];
    }
}
