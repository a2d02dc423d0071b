// kvarq_amd/csrc/kernels_adapt.hip -- the adapter content of an input (include/kvarq_hip.h): per record and probe
// the first full occurrence of the probe on the bases line, else the longest prefix of the probe that ends the line, and the
// length a clip at the earliest of them would leave.  TWO SEARCHES say where a probe occurs: the exact one, and the one that
// tolerates E(len) = len / per differing positions; they are overloads of adapt_search on the probes'
// struct.  ONE SINK, kvq_adapt_records, walks the record index of the exhaustive path (kvq_index_records), as the other input
// passes do, runs the search its probes pick, and adds what it found to its array; it reads the bases line of every record up to
// its newline, never a byte outside its record, and writes nothing but its array.  The adapter clip (kernels_clip.hip) is the
// other sink of the same two searches.
#pragma once
#include "kvq_device.h"
#include "kvq_lines.h"
#include "../../include/kvarq_hip.h"
#include <type_traits>

// the probes as the exact search takes them, by value: the 2-bit codes (byte >> 1) & 3 of probe k, base i at bits [2 i, 2 i + 2), the
// mask of its 2 m_k low bits (all 64 at m_k == 32: no shift by 64 anywhere) and m_k; entries k >= n are zero
struct KvqAdaptProbes { unsigned long long code[KVQ_ADAPT_MAX_PROBES], mask[KVQ_ADAPT_MAX_PROBES]; uint32_t m[KVQ_ADAPT_MAX_PROBES]; uint32_t n; };
// the probes as the tolerant search takes them, by value: probe k as two planes of one bit a base -- bit i of lo / hi is bit 0 / bit 1
// of the 2-bit code (byte >> 1) & 3 of base i --, the mask of its m_k low bits, m_k and E(m_k); entries k >= n are zero
struct KvqAdaptProbesMm { uint32_t lo[KVQ_ADAPT_MAX_PROBES], hi[KVQ_ADAPT_MAX_PROBES], mask[KVQ_ADAPT_MAX_PROBES], m[KVQ_ADAPT_MAX_PROBES], e[KVQ_ADAPT_MAX_PROBES]; uint32_t n, per; };

// a workgroup's LDS: the header words and the blocks of the n probes as the result array has them, the clip histogram right behind
// the last block that is in use (32-bit bins: a batch is < 4 GiB)
struct KvqAdaptLds {
    __host__ __device__ static constexpr uint32_t clip(uint32_t n) { return (uint32_t)KVQ_ADAPT_BLOCKS + n * (uint32_t)KVQ_ADAPT_BLOCK_WORDS; }
    __host__ __device__ static constexpr uint32_t words(uint32_t n) { return clip(n) + (uint32_t)KVQ_ADAPT_CLIP_BINS; }
};

#define KVQ_ADAPT_NONE 0xFFFFFFFFu
// a round of a quarter-wave: sixteen lanes load 256 bytes, the first fourteen own the 224 positions a window of 32 can start at
#define KVQ_ADAPT_ROUND 224u

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
        const uint32_t v = kvq_eq_flags(w[d], 0x41414141u) | kvq_eq_flags(w[d], 0x43434343u) | kvq_eq_flags(w[d], 0x47474747u) | kvq_eq_flags(w[d], 0x54545454u);
        valid |= (((v >> 7) * 0x01020408u) >> 24) << (4u * d);
    }
}
// the sixteen even bits of x, gathered into the low half
__device__ __forceinline__ uint32_t adapt_even_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | x >> 1) & 0x33333333u;
    x = (x | x >> 2) & 0x0F0F0F0Fu;
    x = (x | x >> 4) & 0x00FF00FFu;
    return (x | x >> 8) & 0xFFFFu;
}
// sixteen bytes -> three planes of sixteen bits: the low and the high bit of every 2-bit code, packed as lo | hi << 16, and "is
// upper-case A C G T" (adapt_codes, its codes taken apart)
__device__ __forceinline__ void adapt_planes(const uint32_t w[4], uint32_t &lohi, uint32_t &valid)
{
    uint32_t code;
    adapt_codes(w, code, valid);
    lohi = adapt_even_bits(code) | adapt_even_bits(code >> 1) << 16;
}
// bits [j, j + 32) of the 64 bits b:a, j < 32
__device__ __forceinline__ uint32_t adapt_window(uint32_t a, uint32_t b, uint32_t j)
{
    return (uint32_t)(((unsigned long long)b << 32 | a) >> j);
}

// BOTH SEARCHES: for the sixteen lanes of a quarter-wave and the line of their record (Lraw bytes as it lies, a trailing '\r' among
// them; `top`: the longest line of the wave's four, which sets the rounds so that the shuffles stay convergent).  Sixteen lanes take
// the line 256 bytes a round, sixteen bytes a lane; a lane takes the words of the two lanes behind it by shuffle and has the 47
// bytes a window of 32 bases at any of its sixteen positions can reach; the last two lanes of the sixteen only supply, so a round
// advances by 224 positions and nothing is carried from round to round.  The tail test: the last 32 bytes of the line as it lies (a
// trailing '\r' among them), sixteen to each of the first two lanes, handed to all sixteen by shuffle; lane sub tests t = T + sub
// and T + 16 + sub.  Then FIRST_k (min) and TAIL_k (max; zero where there is a FIRST_k) over the sixteen lanes: all sixteen return
// with the same L (the line less a trailing '\r'), first[], dist[] and tail[].
//
// THE EXACT SEARCH.  A lane turns its bytes into 32 bits of codes and 16 bits of "is A C G T".  Per position the low 16 bits of the
// window (eight bases: no probe is shorter) are tested against every probe first; only a lane with such a hit compares the masked
// 64-bit windows and the valid bits.  Bytes behind the line load as zeros, which are not valid, and so is a trailing '\r': no match
// reaches over the line's end, and the line's loads need not wait for the byte that tells whether it ends in '\r'.  (dist[]: an
// exact occurrence differs nowhere.)
template <int N> __device__ __forceinline__ void
adapt_search(const uint8_t *line, uint32_t Lraw, uint32_t top, const KvqAdaptProbes &P, int lane, uint32_t sub,
             uint32_t &L, uint32_t first[N], uint32_t dist[N], uint32_t tail[N])
{
    const bool own = sub < 14u;
    const uint32_t cr = Lraw && line[Lraw - 1u] == '\r' ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < N; k++) { first[k] = KVQ_ADAPT_NONE; dist[k] = 0u; tail[k] = 0u; }
    for (uint32_t o = 0; o < top; o += KVQ_ADAPT_ROUND) {
        const uint32_t q = o + 16u * sub;
        uint32_t w[4], c0, v0;
        kvq_load16(line, Lraw, q, w);
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
        if (o + KVQ_ADAPT_ROUND < o) break;              // (a line that ends in the last round below 4 GiB)
    }
    // the last 32 bytes of the line as it lies (all of a shorter line), for the tails: the line proper ends at offset `at` of
    // them, and its last 31 bytes are among them whether or not a '\r' is
    L = Lraw - cr;
    {
        const uint32_t b0 = Lraw > 32u ? Lraw - 32u : 0u, at = L - b0;
        uint32_t w[4], cp, vp;
        kvq_load16(line, Lraw, b0 + 16u * (sub & 1u), w);
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
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            first[k] = min(first[k], (uint32_t)__shfl_xor((int)first[k], d, 64));
            tail[k] = max(tail[k], (uint32_t)__shfl_xor((int)tail[k], d, 64));
        }
        if (first[k] != KVQ_ADAPT_NONE) tail[k] = 0u;                              // (TAIL_k only where FIRST_k is none)
    }
}

// THE TOLERANT SEARCH.  A lane turns its sixteen bytes into three planes and has the 47 bases of its windows as three words of 32
// bits and three of 16.  A window is three funnel shifts; a probe then costs popc(((lo ^ plo) | (hi ^ phi) | ~valid) & mask_k)
// and a compare against E(m_k).  No pre-test and no branch: every position of every probe gets its count, and the smallest
// position j of the lane within the budget is kept (j runs downwards: the last one written is the smallest).  A byte that is no
// upper-case A C G T -- an 'N', a lower-case letter, the '\r', the zeros behind the line -- is not valid and so one mismatch,
// whatever its code.  THE WINDOW LIES INSIDE THE LINE: with a budget, a window that hangs over the line's end by up to E bytes
// would be within it, so a position counts only where p + m_k <= L; L needs the byte that tells whether the line ends in '\r',
// which is waited for only here, behind the counts of the first round.  The distance of the position that is kept is counted
// again for that one window (once a round and probe), and lives in a register of its own: a position keeps all its 32 bits.
// Positions rise from round to round, so a lane keeps the first one it finds.  The tails: the last 32 bytes of the line as
// three planes in every lane, tested against E(t) = t / per.  DIST_k is that of the lane that held the minimum.
template <int N> __device__ __forceinline__ void
adapt_search(const uint8_t *line, uint32_t Lraw, uint32_t top, const KvqAdaptProbesMm &P, int lane, uint32_t sub,
             uint32_t &L, uint32_t first[N], uint32_t dist[N], uint32_t tail[N])
{
    const bool own = sub < 14u;
    const uint32_t cr = Lraw && line[Lraw - 1u] == '\r' ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < N; k++) { first[k] = KVQ_ADAPT_NONE; dist[k] = 0u; tail[k] = 0u; }
    for (uint32_t o = 0; o < top; o += KVQ_ADAPT_ROUND) {
        const uint32_t q = o + 16u * sub;
        uint32_t w[4], x0, v0;
        kvq_load16(line, Lraw, q, w);
        adapt_planes(w, x0, v0);
        const uint32_t x1 = (uint32_t)__shfl((int)x0, lane + 1, 64), x2 = (uint32_t)__shfl((int)x0, lane + 2, 64);
        const uint32_t v1 = (uint32_t)__shfl((int)v0, lane + 1, 64), v2 = (uint32_t)__shfl((int)v0, lane + 2, 64);
        // positions 0 .. 31 of the lane's 48 in a, 32 .. 47 in b (what lies above them there is never reached: j + 31 <= 46)
        const uint32_t loa = (x0 & 0xFFFFu) | x1 << 16, lob = x2 & 0xFFFFu;
        const uint32_t hia = x0 >> 16 | (x1 & 0xFFFF0000u), hib = x2 >> 16;
        const uint32_t nva = ~(v0 | v1 << 16), nvb = ~v2;
        uint32_t pj[N];
#pragma unroll
        for (int k = 0; k < N; k++) pj[k] = 16u;
#pragma unroll
        for (int j = 15; j >= 0; j--) {
            const uint32_t wl = adapt_window(loa, lob, (uint32_t)j), wh = adapt_window(hia, hib, (uint32_t)j), wn = adapt_window(nva, nvb, (uint32_t)j);
#pragma unroll
            for (int k = 0; k < N; k++)
                pj[k] = (uint32_t)__popc(((wl ^ P.lo[k]) | (wh ^ P.hi[k]) | wn) & P.mask[k]) <= P.e[k] ? (uint32_t)j : pj[k];
        }
        const uint32_t Lr = Lraw - cr;
#pragma unroll
        for (int k = 0; k < N; k++) {
            // the lane's positions whose window lies inside the line: j <= jmax (none: -1)
            const uint32_t lim = Lr - P.m[k];
            const int jmax = own && Lr >= P.m[k] && q <= lim ? (int)min(lim - q, 15u) : -1;
            const bool take = (int)pj[k] <= jmax && first[k] == KVQ_ADAPT_NONE;
            const uint32_t j = pj[k] & 15u;
            const uint32_t d = (uint32_t)__popc(((adapt_window(loa, lob, j) ^ P.lo[k]) | (adapt_window(hia, hib, j) ^ P.hi[k]) | adapt_window(nva, nvb, j)) & P.mask[k]);
            first[k] = take ? q + j : first[k];
            dist[k] = take ? d : dist[k];
        }
        if (o + KVQ_ADAPT_ROUND < o) break;              // (a line that ends in the last round below 4 GiB)
    }
    // the last 32 bytes of the line as it lies (all of a shorter line), for the tails: the line proper ends at offset `at` of them
    L = Lraw - cr;
    {
        const uint32_t b0 = Lraw > 32u ? Lraw - 32u : 0u, at = L - b0;
        uint32_t w[4], xp, vp;
        kvq_load16(line, Lraw, b0 + 16u * (sub & 1u), w);
        adapt_planes(w, xp, vp);
        const int q0 = lane & ~15;
        const uint32_t xa = (uint32_t)__shfl((int)xp, q0, 64), xb = (uint32_t)__shfl((int)xp, q0 + 1, 64);
        const uint32_t va = (uint32_t)__shfl((int)vp, q0, 64), vb = (uint32_t)__shfl((int)vp, q0 + 1, 64);
        const uint32_t lo = (xa & 0xFFFFu) | xb << 16, hi = xa >> 16 | (xb & 0xFFFF0000u), nv = ~(va | vb << 16);
#pragma unroll
        for (uint32_t half = 0; half < 2u; half++) {
            const uint32_t t = (uint32_t)KVQ_ADAPT_MIN_TAIL + 16u * half + sub;
            if (t > 31u || t > L) continue;
            const uint32_t off = at - t, tm = (1u << t) - 1u;                      // (off <= 26: at <= 32, t >= 6)
            const uint32_t Et = P.per ? (t >= P.per ? 1u : 0u) + (t >= 2u * P.per ? 1u : 0u) + (t >= 3u * P.per ? 1u : 0u) : 0u;   // t / per: t <= 31, per >= 10
            const uint32_t wl = lo >> off, wh = hi >> off, wn = nv >> off;
#pragma unroll
            for (int k = 0; k < N; k++)
                if (t < P.m[k] && (uint32_t)__popc(((wl ^ P.lo[k]) | (wh ^ P.hi[k]) | wn) & tm) <= Et) tail[k] = max(tail[k], t);
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        const uint32_t mine = first[k];
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            first[k] = min(first[k], (uint32_t)__shfl_xor((int)first[k], d, 64));
            tail[k] = max(tail[k], (uint32_t)__shfl_xor((int)tail[k], d, 64));
        }
        // (a position belongs to one lane: the one that held the minimum has its distance, every other lane zero)
        dist[k] = mine == first[k] && mine != KVQ_ADAPT_NONE ? dist[k] : 0u;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) dist[k] |= (uint32_t)__shfl_xor((int)dist[k], d, 64);
        if (first[k] != KVQ_ADAPT_NONE) tail[k] = 0u;                              // (TAIL_k only where FIRST_k is none)
    }
}

// THE CONTENT SINK.  Records [0, nrec) of the batch, N probes (an instantiation for every N: the per-probe state is registers, and
// nothing is spent on probes that are not there), the search of `Probes`.  A QUARTER-WAVE A RECORD, as kvq_reads_records; the rounds
// of a wave are those of its longest line.  Lane k of the sixteen adds probe k's words -- with tolerant probes the distance bins
// +4 .. +7 among them --, lane 0 the record's, all into the workgroup's LDS image of the array (KvqAdaptLds); the words that are not
// zero go to the array with 64-bit atomics when the workgroup ends.  ([4] = per is no sum: the host sets it.)  Grid-stride over
// waves, the index entry of a wave's next records loaded a step ahead.
template <int N, class Probes> __global__ void __launch_bounds__(256)
kvq_adapt_records(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, Probes P,
                  unsigned long long *__restrict__ out)
{
    KVQ_BESIDE_SCAN();
    extern __shared__ unsigned int adapt_lds[];
    constexpr uint32_t clip0 = KvqAdaptLds::clip(N), words = KvqAdaptLds::words(N);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) adapt_lds[i] = 0u;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t sub = (uint32_t)lane & 15u, quarter = (uint32_t)lane >> 4;
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
        uint32_t top = Lraw;
        top = max(top, (uint32_t)__shfl_xor((int)top, 16, 64));
        top = max(top, (uint32_t)__shfl_xor((int)top, 32, 64));

        uint32_t L, first[N], dist[N], tail[N];
        adapt_search<N>(line, Lraw, top, P, lane, sub, L, first, dist, tail);
        uint32_t my_first = KVQ_ADAPT_NONE, my_dist = 0u, my_tail = 0u, clip = L;
        bool full = false, tailed = false;
#pragma unroll
        for (int k = 0; k < N; k++) {
            if (first[k] != KVQ_ADAPT_NONE) { full = true; clip = min(clip, first[k]); }
            else if (tail[k]) { tailed = true; clip = min(clip, L - tail[k]); }
            if (sub == (uint32_t)k) { my_first = first[k]; my_dist = dist[k]; my_tail = tail[k]; }
        }
        if (have && sub < (uint32_t)N) {
            unsigned int *blk = adapt_lds + KVQ_ADAPT_BLOCKS + sub * (uint32_t)KVQ_ADAPT_BLOCK_WORDS;
            if (my_first != KVQ_ADAPT_NONE) {
                atomicAdd(&blk[KVQ_ADAPT_B_FIRST], 1u);
                atomicAdd(&blk[my_first < (uint32_t)KVQ_ADAPT_POSITIONS ? KVQ_ADAPT_B_FIRST_BINS + my_first : (uint32_t)KVQ_ADAPT_B_BEYOND], 1u);
                if constexpr (std::is_same<Probes, KvqAdaptProbesMm>::value) atomicAdd(&blk[KVQ_ADAPT_B_DIST + min(my_dist, (uint32_t)KVQ_ADAPT_DISTS - 1u)], 1u);
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
