// kvarq_amd/csrc/kernels_adapt.hip -- the adapter content of an input (include/kvarq_hip.h): per record and probe
// the first full occurrence of the probe on the bases line, else the longest prefix of the probe that ends the line, and the
// length a clip at the earliest of them would leave.  kvq_adapt_records walks the record index of the exhaustive path
// (kvq_index_records), as the other input passes do; it reads the bases line of every record up to its newline, never a byte
// outside its record, and writes nothing but its array.
#include "kvq_device.h"
#include "../../include/kvarq_hip.h"

// the probes as the kernel takes them, by value: the 2-bit codes (byte >> 1) & 3 of probe k, base i at bits [2 i, 2 i + 2), the
// mask of its 2 m_k low bits (all 64 at m_k == 32: no shift by 64 anywhere) and m_k; entries k >= n are zero
struct KvqAdaptProbes { unsigned long long code[KVQ_ADAPT_MAX_PROBES], mask[KVQ_ADAPT_MAX_PROBES]; uint32_t m[KVQ_ADAPT_MAX_PROBES]; uint32_t n; };

// a workgroup's LDS: the header words and the blocks of the n probes as the result array has them, the clip histogram right behind
// the last block that is in use (32-bit bins: a batch is < 4 GiB)
struct KvqAdaptLds {
    __host__ __device__ static constexpr uint32_t clip(uint32_t n) { return (uint32_t)KVQ_ADAPT_BLOCKS + n * (uint32_t)KVQ_ADAPT_BLOCK_WORDS; }
    __host__ __device__ static constexpr uint32_t words(uint32_t n) { return clip(n) + (uint32_t)KVQ_ADAPT_CLIP_BINS; }
};

#define KVQ_ADAPT_NONE 0xFFFFFFFFu
// a round of a quarter-wave: sixteen lanes load 256 bytes, the first fourteen own the 224 positions a window of 32 can start at
#define KVQ_ADAPT_ROUND 224u

// the sixteen bytes [q, q + 16) of a line of `len` bytes whose terminator ('\n', or the '\r' in front of it) lies at line[len]: one
// vector where it fits into the line and its terminator, else words where they fit and bytes where the line ends (never a byte
// behind the terminator); zeros behind it
__device__ __forceinline__ void adapt_load16(const uint8_t *line, uint32_t len, uint32_t q, uint32_t w[4])
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
__device__ __forceinline__ uint32_t adapt_eq(uint32_t x, uint32_t c4)
{
    const uint32_t y = x ^ c4;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}
// sixteen bytes -> their sixteen 2-bit codes (byte j at bits [2 j, 2 j + 2)) and the sixteen bits "is upper-case A C G T" (a zero,
// a newline, a '\r', an 'N' and a lower-case letter are not).  The multiplies gather one field of every byte: no two partial
// products meet in a bit, so nothing carries
__device__ __forceinline__ void adapt_codes(const uint32_t w[4], uint32_t &code, uint32_t &valid)
{
    code = 0u; valid = 0u;
#pragma unroll
    for (uint32_t d = 0; d < 4u; d++) {
        const uint32_t t = (w[d] >> 1) & 0x03030303u;
        code |= ((t * 0x01041040u) >> 24) << (8u * d);
        const uint32_t v = adapt_eq(w[d], 0x41414141u) | adapt_eq(w[d], 0x43434343u) | adapt_eq(w[d], 0x47474747u) | adapt_eq(w[d], 0x54545454u);
        valid |= (((v >> 7) * 0x01020408u) >> 24) << (4u * d);
    }
}

// Records [0, nrec) of the batch, N probes (an instantiation for every N: the per-probe state is registers, and nothing is spent
// on probes that are not there).  A QUARTER-WAVE A RECORD, as kvq_reads_records: sixteen lanes take the bases line 256 bytes a
// round, sixteen bytes a lane, and turn them into 32 bits of codes and 16 bits of "is A C G T".  A lane takes the words of the two
// lanes behind it by shuffle and has the 47 bytes a window of 32 bases at any of its sixteen positions can reach; the last two
// lanes of the sixteen only supply, so a round advances by 224 positions and nothing is carried from round to round.  Per
// position the low 16 bits of the window (eight bases: no probe is shorter) are tested against every probe first; only a lane
// with such a hit compares the masked 64-bit windows and the valid bits.  Bytes behind the line load as zeros, which are not
// valid, and so is a trailing '\r': no match reaches over the line's end, and the line's loads need not wait for the byte that
// tells whether it ends in '\r'.  The rounds of a wave are those of its longest line (the shuffles stay convergent).  The tail
// test: the last 32 bytes of the line as it lies (a trailing '\r' among them), sixteen to each of the first two lanes, handed to
// all sixteen by shuffle; lane sub tests t = T + sub and T + 16 + sub.  FIRST_k and TAIL_k: min / max over the sixteen lanes.
// Lane k of the sixteen then adds probe k's words, lane 0 the record's, all into the workgroup's LDS image of the array; the
// words that are not zero go to the array with 64-bit atomics when the workgroup ends.  Grid-stride over waves, the index entry
// of a wave's next records loaded a step ahead.
template <int N> __global__ void __launch_bounds__(256)
kvq_adapt_records(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, KvqAdaptProbes P,
                  unsigned long long *__restrict__ out)
{
    KVQ_BESIDE_SCAN();
    extern __shared__ unsigned int adapt_lds[];
    constexpr uint32_t clip0 = KvqAdaptLds::clip(N), words = KvqAdaptLds::words(N);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) adapt_lds[i] = 0u;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t sub = (uint32_t)lane & 15u, quarter = (uint32_t)lane >> 4;
    const bool own = sub < 14u;
    uint32_t mine = 0, with_full = 0, tail_only = 0;     // (what a quarter's first lane keeps for its records)
    const uint64_t stride = (uint64_t)gridDim.x * 16u;
    uint64_t g0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u;
    uint32_t nn[2] = { 0u, 1u };                         // (behind the last record: an empty line)
    if (g0 + quarter < nrec) __builtin_memcpy(nn, nl4 + 4u * (size_t)(g0 + quarter), 8);
    for (; g0 < nrec; g0 += stride) {
        const bool have = g0 + quarter < nrec;
        const uint32_t n[2] = { nn[0], nn[1] };
        nn[0] = 0u; nn[1] = 1u;
        if (g0 + stride + quarter < nrec) __builtin_memcpy(nn, nl4 + 4u * (size_t)(g0 + stride + quarter), 8);
        const uint8_t *line = data + n[0] + 1u;
        const uint32_t Lraw = n[1] - n[0] - 1u;          // the line as it lies: a trailing '\r' is among its bytes
        const uint32_t cr = Lraw && line[Lraw - 1u] == '\r' ? 1u : 0u;
        uint32_t top = Lraw;
        top = max(top, (uint32_t)__shfl_xor((int)top, 16, 64));
        top = max(top, (uint32_t)__shfl_xor((int)top, 32, 64));

        uint32_t first[N], tail[N];
#pragma unroll
        for (int k = 0; k < N; k++) { first[k] = KVQ_ADAPT_NONE; tail[k] = 0u; }
        for (uint32_t o = 0; o < top; o += KVQ_ADAPT_ROUND) {
            const uint32_t q = o + 16u * sub;
            uint32_t w[4], c0, v0;
            adapt_load16(line, Lraw, q, w);
            adapt_codes(w, c0, v0);
            const uint32_t c1 = (uint32_t)__shfl((int)c0, lane + 1, 64), c2 = (uint32_t)__shfl((int)c0, lane + 2, 64);
            const unsigned long long lo = (unsigned long long)c0 | (unsigned long long)c1 << 32;
            bool any = false;
#pragma unroll
            for (uint32_t j = 0; j < 16u; j++) {
                const uint32_t x = (uint32_t)(lo >> (2u * j)) & 0xFFFFu;
#pragma unroll
                for (int k = 0; k < N; k++) any |= x == ((uint32_t)P.code[k] & 0xFFFFu);
            }
            // (in front of the branch: every lane takes part in a shuffle)
            const uint32_t v1 = (uint32_t)__shfl((int)v0, lane + 1, 64), v2 = (uint32_t)__shfl((int)v0, lane + 2, 64);
            if (any && own) {
                const unsigned long long v = (unsigned long long)v0 | (unsigned long long)v1 << 16 | (unsigned long long)v2 << 32;
#pragma unroll
                for (uint32_t j = 0; j < 16u; j++) {
                    const unsigned long long W = j ? lo >> (2u * j) | (unsigned long long)c2 << (64u - 2u * j) : lo;
                    const uint32_t nv = ~(uint32_t)(v >> j);
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const uint32_t vm = P.m[k] >= 32u ? 0xFFFFFFFFu : (1u << P.m[k]) - 1u;
                        if (((W ^ P.code[k]) & P.mask[k]) == 0ull && (nv & vm) == 0u) first[k] = min(first[k], q + j);
                    }
                }
            }
            if (o + KVQ_ADAPT_ROUND < o) break;          // (a line that ends in the last round below 4 GiB)
        }
        // the last 32 bytes of the line as it lies (all of a shorter line), for the tails: the line proper ends at offset `at` of
        // them, and its last 31 bytes are among them whether or not a '\r' is
        const uint32_t L = Lraw - cr;
        {
            const uint32_t b0 = Lraw > 32u ? Lraw - 32u : 0u, at = L - b0;
            uint32_t w[4], cp, vp;
            adapt_load16(line, Lraw, b0 + 16u * (sub & 1u), w);
            adapt_codes(w, cp, vp);
            const int q0 = lane & ~15;
            const uint32_t ca = (uint32_t)__shfl((int)cp, q0, 64), cb = (uint32_t)__shfl((int)cp, q0 + 1, 64);
            const uint32_t va = (uint32_t)__shfl((int)vp, q0, 64), vb = (uint32_t)__shfl((int)vp, q0 + 1, 64);
            const unsigned long long C = (unsigned long long)ca | (unsigned long long)cb << 32;
            const uint32_t V = va | vb << 16;
#pragma unroll
            for (uint32_t half = 0; half < 2u; half++) {
                const uint32_t t = (uint32_t)KVQ_ADAPT_MIN_TAIL + 16u * half + sub;
                if (t > 31u || t > L) continue;
                const uint32_t off = at - t;
                const unsigned long long cw = C >> (2u * off), tm = (1ull << (2u * t)) - 1ull;
                const bool valid = (~(V >> off) & ((1u << t) - 1u)) == 0u;
#pragma unroll
                for (int k = 0; k < N; k++)
                    if (t < P.m[k] && valid && ((cw ^ P.code[k]) & tm) == 0ull) tail[k] = max(tail[k], t);
            }
        }
        uint32_t my_first = KVQ_ADAPT_NONE, my_tail = 0u, clip = L;
        bool full = false, tailed = false;
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                first[k] = min(first[k], (uint32_t)__shfl_xor((int)first[k], d, 64));
                tail[k] = max(tail[k], (uint32_t)__shfl_xor((int)tail[k], d, 64));
            }
            if (first[k] != KVQ_ADAPT_NONE) { full = true; clip = min(clip, first[k]); tail[k] = 0u; }   // (TAIL_k only where FIRST_k is none)
            else if (tail[k]) { tailed = true; clip = min(clip, L - tail[k]); }
            if (sub == (uint32_t)k) { my_first = first[k]; my_tail = tail[k]; }
        }
        if (have && sub < (uint32_t)N) {
            unsigned int *blk = adapt_lds + KVQ_ADAPT_BLOCKS + sub * (uint32_t)KVQ_ADAPT_BLOCK_WORDS;
            if (my_first != KVQ_ADAPT_NONE) {
                atomicAdd(&blk[KVQ_ADAPT_B_FIRST], 1u);
                atomicAdd(&blk[my_first < (uint32_t)KVQ_ADAPT_POSITIONS ? KVQ_ADAPT_B_FIRST_BINS + my_first : (uint32_t)KVQ_ADAPT_B_BEYOND], 1u);
            } else if (my_tail) {
                atomicAdd(&blk[KVQ_ADAPT_B_TAIL], 1u);
                atomicAdd(&blk[KVQ_ADAPT_B_TAIL_BINS + my_tail], 1u);
            }
        }
        if (have && sub == 0u) {
            atomicAdd(&adapt_lds[clip0 + min(clip, (uint32_t)KVQ_ADAPT_CLIP_BINS - 1u)], 1u);
            mine++;
            if (full) with_full++;
            else if (tailed) tail_only++;
        }
    }
    if (mine) atomicAdd(&adapt_lds[KVQ_ADAPT_RECORDS], mine);
    if (with_full) atomicAdd(&adapt_lds[KVQ_ADAPT_WITH_FULL], with_full);
    if (tail_only) atomicAdd(&adapt_lds[KVQ_ADAPT_TAIL_ONLY], tail_only);
    __syncthreads();
    // the workgroup's words that are not zero -> the array (the clip histogram lies behind the eighth block there)
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x)
        if (adapt_lds[i]) atomicAdd(&out[i < clip0 ? i : i - clip0 + (uint32_t)KVQ_ADAPT_CLIP], (unsigned long long)adapt_lds[i]);
}

// the instantiation for n probes, 1 <= n <= KVQ_ADAPT_MAX_PROBES
typedef void (*KvqAdaptKernel)(const uint8_t *, const uint32_t *, uint32_t, KvqAdaptProbes, unsigned long long *);
static KvqAdaptKernel kvq_adapt_kernel(uint32_t n)
{
    switch (n) {
    case 1: return kvq_adapt_records<1>;
    case 2: return kvq_adapt_records<2>;
    case 3: return kvq_adapt_records<3>;
    case 4: return kvq_adapt_records<4>;
    case 5: return kvq_adapt_records<5>;
    case 6: return kvq_adapt_records<6>;
    case 7: return kvq_adapt_records<7>;
    default: return kvq_adapt_records<8>;
    }
}
