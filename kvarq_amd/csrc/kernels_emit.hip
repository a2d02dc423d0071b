// kvarq_amd/csrc/kernels_emit.hip -- the reads the scan saw, as FastQ text (include/kvarq_hip.h): every record of a
// batch cut to the part the quality trim leaves of it and compacted into one store.  Three steps over the record index of the
// exhaustive path (kvq_index_records: nl4, rec_start): kvq_emit_size says per record what becomes of it and how many bytes it takes,
// an exclusive 64-bit prefix sum over those bytes (kvq_emit_block_sums, kvq_emit_scan_blocks, kvq_emit_offsets) says where, and
// kvq_emit_copy moves the three pieces of every emitted record and writes its five fixed bytes.  The batch's text is only read.
#include "kvq_device.h"
#include "kvq_lines.h"
#include "../../include/kvarq_hip.h"

// what kvq_emit_size leaves per record: the class (KVQ_EMIT_CLASS_*), start and length of the trim, the bytes of its output (0: dropped)
struct KvqEmitRec { uint32_t cls, start, length, bytes; };
#define KVQ_EMIT_CLASS_EMITTED 0u
#define KVQ_EMIT_CLASS_SHORT 1u
#define KVQ_EMIT_CLASS_MISMATCHED 2u
// records a workgroup of the prefix sum takes (a thread each); the second level takes as many block sums a step, and carries
#define KVQ_EMIT_SCAN_BLOCK 256u

// Records [0, nrec) of the batch, a wave a record, KVQ_TRIM_RPW consecutive records a wave, grid-stride over waves (the shape of
// kvq_profile_records, whose trim this is for the one cutoff amin: the same three-way split over the helpers of kvq_lines.h.  The
// split stands here and not in a function of its own: behind one, the compiler loads the index entry as one vector and the kernel
// takes 100 VGPRs for 99; profiles/record_pass_refactor.txt).  rec[g] is written for every record.  The wave keeps its records'
// share of the seven sums in registers (every lane the same), its first lane adds them to the workgroup's LDS, and the words that
// are not zero go to out[1 .. 7] with one 64-bit atomic each a workgroup.
extern "C" __global__ void __launch_bounds__(256)
kvq_emit_size(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, const uint32_t *__restrict__ rec_start, uint32_t nrec,
              int32_t amin, uint32_t min_length, KvqEmitRec *__restrict__ rec, unsigned long long *__restrict__ out)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long emit_lds[KVQ_EMIT_WORDS];
    if (threadIdx.x < (uint32_t)KVQ_EMIT_WORDS) emit_lds[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = kvq_lane();
    unsigned long long sums[KVQ_EMIT_WORDS] = { 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull };
    for (uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6); (uint64_t)wave * KVQ_TRIM_RPW < nrec; wave += gridDim.x * 4u) {
        const uint32_t g_begin = wave * KVQ_TRIM_RPW;
        for (uint32_t g = g_begin; g < g_begin + KVQ_TRIM_RPW && g < nrec; g++) {
            const uint32_t n0 = nl4[4 * (size_t)g], n1 = nl4[4 * (size_t)g + 1], n2 = nl4[4 * (size_t)g + 2], n3 = nl4[4 * (size_t)g + 3];
            const uint32_t r0 = rec_start[g];
            const uint8_t *sline = data + n2 + 1u;
            const uint32_t L = n1 - n0 - 1u, Q = n3 - n2 - 1u;
            sums[KVQ_EMIT_RECORDS]++; sums[KVQ_EMIT_BASES_IN] += L;
            KvqEmitRec e; e.cls = KVQ_EMIT_CLASS_MISMATCHED; e.start = 0u; e.length = 0u; e.bytes = 0u;
            if (L != Q) sums[KVQ_EMIT_MISMATCHED]++;
            else {
                int best; uint32_t bstart;
                if (Q >= 1024u) kvq_long_trim(sline, Q, amin, lane, best, bstart);
                else if (Q >= 256u) { uint8_t by[16]; kvq_short_load<16>(sline, Q + 1u, lane, by); kvq_short_trim<16>(by, Q + 1u, amin, lane, best, bstart); }
                else { uint8_t by[4]; kvq_short_load<4>(sline, Q + 1u, lane, by); kvq_short_trim<4>(by, Q + 1u, amin, lane, best, bstart); }
                e.start = bstart; e.length = (uint32_t)best;
                if ((uint32_t)best < min_length) { e.cls = KVQ_EMIT_CLASS_SHORT; sums[KVQ_EMIT_SHORT]++; }
                else {
                    // the name: [r0, n0) less one trailing '\r'
                    const uint32_t name = n0 - r0 - (n0 > r0 && data[n0 - 1u] == '\r' ? 1u : 0u);
                    e.cls = KVQ_EMIT_CLASS_EMITTED; e.bytes = name + 2u * (uint32_t)best + 5u;
                    sums[KVQ_EMIT_EMITTED]++; sums[KVQ_EMIT_BASES_OUT] += (uint32_t)best; sums[KVQ_EMIT_BYTES_OUT] += e.bytes;
                }
            }
            if (lane == 0) rec[g] = e;
        }
    }
    if (lane == 0 && sums[KVQ_EMIT_RECORDS]) {
#pragma unroll
        for (int i = 1; i < KVQ_EMIT_WORDS; i++) if (sums[i]) atomicAdd(&emit_lds[i], sums[i]);
    }
    __syncthreads();
    if (threadIdx.x >= 1u && threadIdx.x < (uint32_t)KVQ_EMIT_WORDS && emit_lds[threadIdx.x]) atomicAdd(&out[threadIdx.x], emit_lds[threadIdx.x]);
}

// ---- the exclusive 64-bit prefix sum of rec[].bytes ----
// the exclusive sum of v over the 256 threads of a workgroup, and their total (lds: four words; every thread calls)
__device__ __forceinline__ unsigned long long emit_block_scan(unsigned long long v, unsigned long long *lds, unsigned long long &total)
{
    const int lane = kvq_lane();
    const uint32_t wave = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(x, (unsigned int)d, 64);
        if (lane >= d) x += t;
    }
    __syncthreads();                                   // (the words may still be read from the call before)
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned long long base = 0; total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; w++) { const unsigned long long t = lds[w]; total += t; if (w < wave) base += t; }
    return base + x - v;
}

// block b: the sum of the bytes of records [256 b, 256 b + 256)
extern "C" __global__ void __launch_bounds__(256)
kvq_emit_block_sums(const KvqEmitRec *__restrict__ rec, uint32_t nrec, unsigned long long *__restrict__ bsum)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long lds[4];
    for (uint32_t b = blockIdx.x; (uint64_t)b * KVQ_EMIT_SCAN_BLOCK < nrec; b += gridDim.x) {
        const uint64_t g = (uint64_t)b * KVQ_EMIT_SCAN_BLOCK + threadIdx.x;
        unsigned long long total;
        (void)emit_block_scan(g < nrec ? (unsigned long long)rec[g].bytes : 0ull, lds, total);
        if (threadIdx.x == 0) bsum[b] = total;
    }
}

// ONE workgroup: the block sums become their exclusive prefix sums, 256 a step with the carry of the steps before; the total of
// the batch goes to *total
extern "C" __global__ void __launch_bounds__(256)
kvq_emit_scan_blocks(unsigned long long *__restrict__ bsum, uint32_t nblocks, unsigned long long *__restrict__ total_out)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long lds[4];
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += KVQ_EMIT_SCAN_BLOCK) {
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long v = b < nblocks ? bsum[b] : 0ull;
        unsigned long long total;
        const unsigned long long ex = emit_block_scan(v, lds, total);
        if (b < nblocks) bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// off[g]: where record g's output begins in the store
extern "C" __global__ void __launch_bounds__(256)
kvq_emit_offsets(const KvqEmitRec *__restrict__ rec, uint32_t nrec, const unsigned long long *__restrict__ bsum, unsigned long long *__restrict__ off)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long lds[4];
    for (uint32_t b = blockIdx.x; (uint64_t)b * KVQ_EMIT_SCAN_BLOCK < nrec; b += gridDim.x) {
        const uint64_t g = (uint64_t)b * KVQ_EMIT_SCAN_BLOCK + threadIdx.x;
        unsigned long long total;
        const unsigned long long ex = emit_block_scan(g < nrec ? (unsigned long long)rec[g].bytes : 0ull, lds, total);
        if (g < nrec) off[g] = bsum[b] + ex;
    }
}

// ---- the copy ----
// src[0, len) to dst[0, len) by the sixteen lanes of a quarter, any alignment of either.  Lane `sub` takes the 16-byte blocks sub,
// sub + 16, ... of the DESTINATION, counted from the aligned block that holds dst[0].  The bytes of a block that lie inside the
// piece come from one or two ALIGNED 16-byte blocks of the source, each of which holds at least one byte of the piece (the rule
// of kvq_load16: the batch's buffer may end with its text's last byte, and an aligned block never leaves a page); they are put
// in place with a word select and v_alignbyte.  A whole block inside the piece is one 16-byte store, an aligned word inside it one
// dword store, the bytes of the two ragged ends go one by one: nothing is read back, no byte outside dst[0, len) is written, and
// every byte has one lane.
__device__ __forceinline__ void emit_copy(const uint8_t *src, uint32_t len, uint8_t *dst, uint32_t sub)
{
    const uintptr_t S = (uintptr_t)src, A = (uintptr_t)dst, B = A + len;
    if (len == 0u) return;                               // (an empty piece has no byte a load could hold)
    for (uintptr_t blk = (A & ~(uintptr_t)15) + 16u * sub; blk < B; blk += 256u) {
        const uintptr_t da = blk > A ? blk : A, db = blk + 16u < B ? blk + 16u : B;      // the block's bytes inside the piece
        const uintptr_t sa = S + (da - A), sb = S + (db - A);                            // ... and where they come from
        const uintptr_t b0 = sa & ~(uintptr_t)15, b1 = (sb - 1u) & ~(uintptr_t)15;       // (b1 is b0 or b0 + 16)
        const uint4 x0 = *(const uint4 *)b0;
        uint4 x1 = make_uint4(0u, 0u, 0u, 0u);
        if (b1 != b0) x1 = *(const uint4 *)b1;
        // the byte of the source that belongs at blk lies `at` bytes into (16 zero bytes, x0, x1): 1 .. 31
        const uint32_t at = (uint32_t)(S + (blk - A) + 16u - b0);
        uint32_t w[12] = { 0u, 0u, 0u, 0u, x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w };
        const uint32_t wi = at >> 2, bi = at & 3u;
        if (wi & 4u) {
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = w[i + 4];
        }
        if (wi & 2u) {
#pragma unroll
            for (int i = 0; i < 6; i++) w[i] = w[i + 2];
        }
        if (wi & 1u) {
#pragma unroll
            for (int i = 0; i < 5; i++) w[i] = w[i + 1];
        }
        uint32_t v[4];
#pragma unroll
        for (int d = 0; d < 4; d++) v[d] = __builtin_amdgcn_alignbyte(w[d + 1], w[d], bi);
        if (blk >= A && blk + 16u <= B) {
            *(uint4 *)blk = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const uintptr_t p = blk + 4u * d;
            if (p >= A && p + 4u <= B) *(uint32_t *)p = v[d];
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) if (p + j >= A && p + j < B) *(uint8_t *)(p + j) = (uint8_t)(v[d] >> (8u * j));
            }
        }
    }
}

// Records [0, nrec) of the batch, A QUARTER-WAVE A RECORD (as kvq_clip_records), grid-stride over waves.  An emitted record g goes
// to store[off[g], off[g] + rec[g].bytes): its name, '\n', its bases [start, start + length), "\n+\n", its scores of the same
// range, '\n' -- three pieces through emit_copy, the five fixed bytes by the quarter's first five lanes.  The lanes of a quarter
// need nothing of each other: no shuffle, and a long piece only keeps its own sixteen lanes busy.
extern "C" __global__ void __launch_bounds__(256)
kvq_emit_copy(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, const uint32_t *__restrict__ rec_start, uint32_t nrec,
              const KvqEmitRec *__restrict__ rec, const unsigned long long *__restrict__ off, uint8_t *__restrict__ store)
{
    KVQ_BESIDE_SCAN();
    const uint32_t lane = (uint32_t)kvq_lane(), sub = lane & 15u, quarter = lane >> 4;
    const uint64_t stride = (uint64_t)gridDim.x * 16u;
    for (uint64_t g = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u + quarter; g < nrec; g += stride) {
        const KvqEmitRec e = rec[g];
        if (e.bytes == 0u) continue;                     // (dropped: short or mismatched)
        uint32_t n[4];
        __builtin_memcpy(n, nl4 + 4u * (size_t)g, 16);
        const uint32_t r0 = rec_start[g];
        const uint32_t name = e.bytes - 2u * e.length - 5u;
        uint8_t *const o = store + off[g];
        emit_copy(data + r0, name, o, sub);
        emit_copy(data + n[0] + 1u + e.start, e.length, o + name + 1u, sub);
        emit_copy(data + n[2] + 1u + e.start, e.length, o + name + e.length + 4u, sub);
        if (sub < 5u) {
            const uint32_t at = sub == 0u ? name : sub < 4u ? name + e.length + sub : e.bytes - 1u;
            o[at] = sub == 2u ? (uint8_t)'+' : (uint8_t)'\n';
        }
    }
}
