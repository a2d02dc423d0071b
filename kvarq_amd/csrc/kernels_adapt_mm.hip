// kvarq_amd/csrc/kernels_adapt_mm.hip -- adapter probes that tolerate mismatches (include/kvarq_hip.h): the
// adapter content and the adapter clip under the rule "at most E(len) = len / per positions differ", as kvq_adapt_records_mm
// and kvq_clip_records_mm.  ONE search (adapt_search_mm) serves both; the walk over the record index, the loads, the LDS image,
// the stores and the atomics are those of kernels_adapt.hip and kernels_clip.hip, whose helpers are used as they are.  The
// launcher picks these kernels only with per > 0: the exact kernels keep their registers and their numbers.
#include "kvq_device.h"
#include "../../include/kvarq_hip.h"

// the probes as these kernels take them, by value: probe k as two planes of one bit a base -- bit i of lo / hi is bit 0 / bit 1 of
// the 2-bit code (byte >> 1) & 3 of base i --, the mask of its m_k low bits, m_k and E(m_k); entries k >= n are zero
struct KvqAdaptProbesMm { uint32_t lo[KVQ_ADAPT_MAX_PROBES], hi[KVQ_ADAPT_MAX_PROBES], mask[KVQ_ADAPT_MAX_PROBES], m[KVQ_ADAPT_MAX_PROBES], e[KVQ_ADAPT_MAX_PROBES]; uint32_t n, per; };

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

// THE SEARCH, for the sixteen lanes of a quarter-wave and the line of their record (Lraw bytes as it lies, a trailing '\r' among
// them; `top`: the longest line of the wave's four, which sets the rounds so that the shuffles stay convergent).  Rounds of 224
// positions with nothing carried, as kvq_adapt_records: a lane turns its sixteen bytes into three planes, takes those of the two
// lanes behind it by shuffle and has the 47 bases a window of 32 at any of its sixteen positions can reach, as three words of 32
// bits and three of 16.  A window is three funnel shifts; a probe then costs popc(((lo ^ plo) | (hi ^ phi) | ~valid) & mask_k)
// and a compare against E(m_k).  No pre-test and no branch: every position of every probe gets its count, and the smallest
// position j of the lane within the budget is kept (j runs downwards: the last one written is the smallest).  A byte that is no
// upper-case A C G T -- an 'N', a lower-case letter, the '\r', the zeros behind the line -- is not valid and so one mismatch,
// whatever its code.  THE WINDOW LIES INSIDE THE LINE: with a budget, a window that hangs over the line's end by up to E bytes
// would be within it, so a position counts only where p + m_k <= L; L needs the byte that tells whether the line ends in '\r',
// which is waited for only here, behind the counts of the first round.  The distance of the position that is kept is counted
// again for that one window (once a round and probe), and lives in a register of its own: a position keeps all its 32 bits.
// Positions rise from round to round, so a lane keeps the first one it finds.  The tails: the last 32 bytes of the line as
// three planes in every lane; lane sub tests t = T + sub and T + 16 + sub against E(t) = t / per.  Then FIRST_k (min), DIST_k
// (of the lane that held the minimum) and TAIL_k (max; zero where there is a FIRST_k) over the sixteen lanes: all sixteen
// return with the same first[], dist[], tail[] and L.
template <int N> __device__ __forceinline__ void
adapt_search_mm(const uint8_t *line, uint32_t Lraw, uint32_t top, const KvqAdaptProbesMm &P, int lane, uint32_t sub,
                uint32_t &L, uint32_t first[N], uint32_t dist[N], uint32_t tail[N])
{
    const bool own = sub < 14u;
    const uint32_t cr = Lraw && line[Lraw - 1u] == '\r' ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < N; k++) { first[k] = KVQ_ADAPT_NONE; dist[k] = 0u; tail[k] = 0u; }
    for (uint32_t o = 0; o < top; o += KVQ_ADAPT_ROUND) {
        const uint32_t q = o + 16u * sub;
        uint32_t w[4], x0, v0;
        adapt_load16(line, Lraw, q, w);
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
        adapt_load16(line, Lraw, b0 + 16u * (sub & 1u), w);
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

// Records [0, nrec) of the batch, N probes: kvq_adapt_records with the search above.  A quarter-wave a record, the index entry of
// a wave's next records loaded a step ahead; lane k of the sixteen adds probe k's words -- the distance bins +4 .. +7 among
// them --, lane 0 the record's, all into the workgroup's LDS image of the array (KvqAdaptLds); the words that are not zero go to
// the array with 64-bit atomics when the workgroup ends.  ([4] = per is no sum: the host sets it.)
template <int N> __global__ void __launch_bounds__(256)
kvq_adapt_records_mm(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, KvqAdaptProbesMm P,
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
        adapt_search_mm<N>(line, Lraw, top, P, lane, sub, L, first, dist, tail);
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
                atomicAdd(&blk[KVQ_ADAPT_B_DIST + min(my_dist, (uint32_t)KVQ_ADAPT_DISTS - 1u)], 1u);
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

// Records [0, nrec) of the batch, N probes: kvq_clip_records with the search above.  The whole 16-byte index entry (n2 and n3
// bound the score line); where CLIP < L the sixteen lanes store '!' over [CLIP, S) of the score line (clip_store).  The four sums
// as there.  ([5] = per is no sum: the host sets it.)
template <int N> __global__ void __launch_bounds__(256)
kvq_clip_records_mm(uint8_t *data, const uint32_t *__restrict__ nl4, uint32_t nrec, KvqAdaptProbesMm P, unsigned long long *__restrict__ out)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long clip_lds[4];
    if (threadIdx.x < 4u) clip_lds[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t sub = (uint32_t)lane & 15u, quarter = (uint32_t)lane >> 4;
    unsigned long long mine = 0, clipped = 0, masked = 0, cut = 0;     // (what a quarter's first lane keeps for its records)
    const uint64_t stride = (uint64_t)gridDim.x * 16u;
    uint64_t g0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u;
    uint32_t nn[4] = { 0u, 1u, 1u, 2u };                 // (behind the last record: empty lines)
    if (g0 + quarter < nrec) __builtin_memcpy(nn, nl4 + 4u * (size_t)(g0 + quarter), 16);
    for (; g0 < nrec; g0 += stride) {
        const bool have = g0 + quarter < nrec;
        const uint32_t n[4] = { nn[0], nn[1], nn[2], nn[3] };
        nn[0] = 0u; nn[1] = 1u; nn[2] = 1u; nn[3] = 2u;
        if (g0 + stride + quarter < nrec) __builtin_memcpy(nn, nl4 + 4u * (size_t)(g0 + stride + quarter), 16);
        const uint8_t *line = data + n[0] + 1u;
        const uint32_t Lraw = n[1] - n[0] - 1u;          // the line as it lies: a trailing '\r' is among its bytes
        uint32_t top = Lraw;
        top = max(top, (uint32_t)__shfl_xor((int)top, 16, 64));
        top = max(top, (uint32_t)__shfl_xor((int)top, 32, 64));

        uint32_t L, first[N], dist[N], tail[N];
        adapt_search_mm<N>(line, Lraw, top, P, lane, sub, L, first, dist, tail);
        uint32_t clip = L;
#pragma unroll
        for (int k = 0; k < N; k++) {
            if (first[k] != KVQ_ADAPT_NONE) clip = min(clip, first[k]);
            else if (tail[k]) clip = min(clip, L - tail[k]);
        }
        // the mask: [CLIP, S) of the score line of a clipped record (a quarter's lanes agree on all of it: no shuffle below)
        if (have && clip < L) {
            const uint32_t Sraw = n[3] - n[2] - 1u;
            const uint32_t S = Sraw - (Sraw && data[n[2] + Sraw] == '\r' ? 1u : 0u);
            if (S > clip) clip_store(data, (uint64_t)n[2] + 1u + clip, (uint64_t)n[2] + 1u + S, sub);
            if (sub == 0u) { clipped++; masked += S > clip ? S - clip : 0u; cut += L - clip; }
        }
        if (have && sub == 0u) mine++;
    }
    if (mine) atomicAdd(&clip_lds[0], mine);
    if (clipped) { atomicAdd(&clip_lds[1], clipped); atomicAdd(&clip_lds[2], masked); atomicAdd(&clip_lds[3], cut); }
    __syncthreads();
    if (threadIdx.x < 4u && clip_lds[threadIdx.x]) atomicAdd(&out[KVQ_CLIP_RECORDS + threadIdx.x], clip_lds[threadIdx.x]);
}

// the instantiations for n probes, 1 <= n <= KVQ_ADAPT_MAX_PROBES
typedef void (*KvqAdaptMmKernel)(const uint8_t *, const uint32_t *, uint32_t, KvqAdaptProbesMm, unsigned long long *);
static KvqAdaptMmKernel kvq_adapt_mm_kernel(uint32_t n)
{
    switch (n) {
    case 1: return kvq_adapt_records_mm<1>;
    case 2: return kvq_adapt_records_mm<2>;
    case 3: return kvq_adapt_records_mm<3>;
    case 4: return kvq_adapt_records_mm<4>;
    case 5: return kvq_adapt_records_mm<5>;
    case 6: return kvq_adapt_records_mm<6>;
    case 7: return kvq_adapt_records_mm<7>;
    default: return kvq_adapt_records_mm<8>;
    }
}
typedef void (*KvqClipMmKernel)(uint8_t *, const uint32_t *, uint32_t, KvqAdaptProbesMm, unsigned long long *);
static KvqClipMmKernel kvq_clip_mm_kernel(uint32_t n)
{
    switch (n) {
    case 1: return kvq_clip_records_mm<1>;
    case 2: return kvq_clip_records_mm<2>;
    case 3: return kvq_clip_records_mm<3>;
    case 4: return kvq_clip_records_mm<4>;
    case 5: return kvq_clip_records_mm<5>;
    case 6: return kvq_clip_records_mm<6>;
    case 7: return kvq_clip_records_mm<7>;
    default: return kvq_clip_records_mm<8>;
    }
}
