// kvarq_amd/csrc/kernels_profile.hip -- the profile of a batch (include/kvarq_hip.h): what bytes the score
// and bases lines of its records hold, how long the bases lines are, and what the quality trim leaves of every record at
// up to eight cutoffs.  One kernel over the record index of the exhaustive path (kvq_index_records); it reads the text
// only inside its records and writes nothing but the profile array.
#include "kvq_device.h"
#include "kvq_lines.h"
#include "../../include/kvarq_hip.h"

// the cutoffs, a byte each (compared as signed char, like Amin)
struct KvqProfileCuts { int32_t n; unsigned long long packed; };
__device__ __forceinline__ int prof_amin(const KvqProfileCuts &C, int k) { return (int)(int8_t)(C.packed >> (8 * k)); }

// where the pieces lie inside a workgroup's LDS (32-bit bins: a batch is < 4 GiB); `spread`: KVQ_PROF_COPIES copies of the two
// byte histograms behind them, a lane adding to the copy of its number
#define KVQ_PROF_COPIES 8
struct KvqProfLds {
    static constexpr uint32_t SCORE = 0, BASE = 256, RAW = 512, TRIM = RAW + KVQ_PROF_RAW_BINS, SCALARS = 16;
    // scalars behind the last trimmed histogram: records, mismatched, longest raw line + 1, longest trimmed read + 1 per cutoff
    static constexpr uint32_t S_RECORDS = 0, S_MISMATCH = 1, S_LONGEST = 2, S_CUT_LONGEST = 3;
    __host__ __device__ static uint32_t scalars(int ncut) { return TRIM + (uint32_t)ncut * KVQ_RL_BINS; }
    __host__ __device__ static uint32_t copies(int ncut) { return scalars(ncut) + SCALARS; }
    __host__ __device__ static uint32_t words(int ncut, bool spread) { return copies(ncut) + (spread ? 2u * 256u * KVQ_PROF_COPIES : 0u); }
};

// one byte of every lane (where `valid`) into a 256-bin histogram in LDS.  Score and bases lines hold few distinct bytes,
// and 64 lanes adding to one LDS word queue up: either the wave counts its equal bytes first (the first lane's byte, the
// ballot of the lanes that hold the same one, ONE add of their number, until none is left), or the lanes spread their
// adds over KVQ_PROF_COPIES copies of the histogram
__device__ __forceinline__ void prof_byte(unsigned int *bins, unsigned int *copies, bool spread, uint32_t byte, bool valid, int lane)
{
    if (spread) {
        if (valid) atomicAdd(&copies[byte * KVQ_PROF_COPIES + ((uint32_t)lane & (KVQ_PROF_COPIES - 1u))], 1u);
        return;
    }
    unsigned long long todo = __ballot(valid);
    while (todo) {                                   // (the same for every lane)
        const int l = __ffsll((long long)todo) - 1;
        const uint32_t v = (uint32_t)__shfl((int)byte, l, 64);
        const unsigned long long same = __ballot(valid && byte == v);
        if (lane == l) atomicAdd(&bins[v], (unsigned int)__popcll(same));
        todo &= ~same;
    }
}

// a line of 1024 bytes or more (a long read from BAM): a KiB a step, sixteen bytes a lane
__device__ void prof_long_bytes(const uint8_t *line, uint32_t len, unsigned int *bins, unsigned int *copies, bool spread, int lane)
{
    for (uint32_t o = 0; o < len; o += 1024u) {
        const uint32_t q = o + 16u * (uint32_t)lane;
        uint32_t w[4];
        kvq_load16(line, len, q, w);
        const uint32_t n = q < len ? (len - q < 16u ? len - q : 16u) : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) prof_byte(bins, copies, spread, (w[j >> 2] >> (8u * (j & 3u))) & 0xFFu, j < n, lane);
    }
}

template <int NG>
__device__ __forceinline__ void prof_short_bytes(const uint8_t by[NG], uint32_t len, unsigned int *bins, unsigned int *copies, bool spread, int lane)
{
#pragma unroll
    for (int k = 0; k < NG; k++) {
        if (64u * (uint32_t)k >= len) break;
        prof_byte(bins, copies, spread, by[k], 64u * (uint32_t)k + (uint32_t)lane < len, lane);
    }
}

// Grid-stride over waves, KVQ_TRIM_RPW consecutive records a wave (a wave a record).  prof: the profile array of
// include/kvarq_hip.h.  Dynamic LDS: KvqProfLds::words(C.n, spread) words.
extern "C" __global__ void __launch_bounds__(256)
kvq_profile_records(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, KvqProfileCuts C,
                    uint32_t spread_, unsigned long long *__restrict__ prof)
{
    KVQ_BESIDE_SCAN();
    extern __shared__ unsigned int prof_lds[];
    const bool spread = spread_ != 0u;
    const int ncut = C.n;
    const uint32_t nwords = KvqProfLds::words(ncut, spread);
    for (uint32_t i = threadIdx.x; i < nwords; i += blockDim.x) prof_lds[i] = 0u;
    __syncthreads();
    unsigned int *const score = prof_lds + KvqProfLds::SCORE, *const base = prof_lds + KvqProfLds::BASE, *const raw = prof_lds + KvqProfLds::RAW;
    unsigned int *const trimmed = prof_lds + KvqProfLds::TRIM, *const sc = prof_lds + KvqProfLds::scalars(ncut);
    unsigned int *const score_copies = prof_lds + KvqProfLds::copies(ncut), *const base_copies = score_copies + 256 * KVQ_PROF_COPIES;

    const int lane = kvq_lane();
    unsigned long long nbase = 0, nscore = 0;          // bytes on the bases / score lines of this wave's records
    uint32_t mine = 0, mism = 0, longest = 0;
    for (uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6); (uint64_t)wave * KVQ_TRIM_RPW < nrec; wave += gridDim.x * 4u) {
        const uint32_t g_begin = wave * KVQ_TRIM_RPW;
        for (uint32_t g = g_begin; g < g_begin + KVQ_TRIM_RPW && g < nrec; g++) {
            const uint32_t n0 = nl4[4 * (size_t)g], n1 = nl4[4 * (size_t)g + 1], n2 = nl4[4 * (size_t)g + 2], n3 = nl4[4 * (size_t)g + 3];
            const uint8_t *bline = data + n0 + 1u, *sline = data + n2 + 1u;
            const uint32_t L = n1 - n0 - 1u, Q = n3 - n2 - 1u;
            mine++; nbase += L; nscore += Q; mism += L != Q;
            longest = L + 1u > longest ? L + 1u : longest;
            if (lane == 0) atomicAdd(&raw[L < KVQ_PROF_RAW_BINS - 1u ? L : KVQ_PROF_RAW_BINS - 1u], 1u);
            // the bases line
            if (L >= 1024u) prof_long_bytes(bline, L, base, base_copies, spread, lane);
            else if (L >= 256u) { uint8_t by[16]; kvq_short_load<16>(bline, L + 1u, lane, by); prof_short_bytes<16>(by, L, base, base_copies, spread, lane); }
            else { uint8_t by[4]; kvq_short_load<4>(bline, L + 1u, lane, by); prof_short_bytes<4>(by, L, base, base_copies, spread, lane); }
            // the score line, and what the trim leaves of it at every cutoff (add_rl: a read of 1024 and more in no bin)
            auto count = [&](int k, int rl) {
                if (lane == 0) {
                    if (rl < KVQ_RL_BINS) atomicAdd(&trimmed[(uint32_t)k * KVQ_RL_BINS + (uint32_t)rl], 1u);
                    atomicMax(&sc[KvqProfLds::S_CUT_LONGEST + k], (unsigned int)rl + 1u);
                }
            };
            // (the split by line length stands here, over the helpers of kvq_lines.h: a short line's bytes are loaded once, for the
            // histogram and for every cutoff)
            int best; uint32_t start;                  // (the run the trim keeps: only its length is counted here)
            if (Q >= 1024u) {
                prof_long_bytes(sline, Q, score, score_copies, spread, lane);
                for (int k = 0; k < ncut; k++) { kvq_long_trim(sline, Q, prof_amin(C, k), lane, best, start); count(k, best); }
            } else if (Q >= 256u) {
                uint8_t by[16]; kvq_short_load<16>(sline, Q + 1u, lane, by);
                prof_short_bytes<16>(by, Q, score, score_copies, spread, lane);
                for (int k = 0; k < ncut; k++) { kvq_short_trim<16>(by, Q + 1u, prof_amin(C, k), lane, best, start); count(k, best); }
            } else {
                uint8_t by[4]; kvq_short_load<4>(sline, Q + 1u, lane, by);
                prof_short_bytes<4>(by, Q, score, score_copies, spread, lane);
                for (int k = 0; k < ncut; k++) { kvq_short_trim<4>(by, Q + 1u, prof_amin(C, k), lane, best, start); count(k, best); }
            }
        }
    }
    if (lane == 0 && mine) {
        atomicAdd(&sc[KvqProfLds::S_RECORDS], mine);
        if (mism) atomicAdd(&sc[KvqProfLds::S_MISMATCH], mism);
        atomicMax(&sc[KvqProfLds::S_LONGEST], longest);
        atomicAdd(&prof[KVQ_PROF_BASE_LINE_BYTES], nbase);
        atomicAdd(&prof[KVQ_PROF_SCORE_LINE_BYTES], nscore);
    }
    __syncthreads();
    // the workgroup's bins that are not zero -> the profile; the maxima as maxima
    for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x) {
        unsigned int v = prof_lds[i];
        if (spread)
            for (uint32_t c = 0; c < KVQ_PROF_COPIES; c++) v += score_copies[i * KVQ_PROF_COPIES + c];      // (the bases' copies lie behind the scores')
        if (v) atomicAdd(&prof[KVQ_PROF_SCORE_BYTES + i], (unsigned long long)v);
    }
    for (uint32_t i = threadIdx.x; i < KVQ_PROF_RAW_BINS; i += blockDim.x)
        if (raw[i]) atomicAdd(&prof[KVQ_PROF_RAW_LENGTHS + i], (unsigned long long)raw[i]);
    for (uint32_t i = threadIdx.x; i < (uint32_t)ncut * KVQ_RL_BINS; i += blockDim.x)
        if (trimmed[i]) atomicAdd(&prof[KVQ_PROF_CUTOFFS + (i / KVQ_RL_BINS) * KVQ_PROF_CUT_WORDS + 1u + (i % KVQ_RL_BINS)], (unsigned long long)trimmed[i]);
    if (threadIdx.x == 0) {
        if (sc[KvqProfLds::S_RECORDS]) atomicAdd(&prof[KVQ_PROF_RECORDS], (unsigned long long)sc[KvqProfLds::S_RECORDS]);
        if (sc[KvqProfLds::S_MISMATCH]) atomicAdd(&prof[KVQ_PROF_MISMATCHED], (unsigned long long)sc[KvqProfLds::S_MISMATCH]);
        if (sc[KvqProfLds::S_LONGEST]) atomicMax(&prof[KVQ_PROF_LONGEST], (unsigned long long)sc[KvqProfLds::S_LONGEST]);
    }
    if (threadIdx.x < (uint32_t)ncut && sc[KvqProfLds::S_CUT_LONGEST + threadIdx.x])
        atomicMax(&prof[KVQ_PROF_CUTOFFS + threadIdx.x * KVQ_PROF_CUT_WORDS], (unsigned long long)sc[KvqProfLds::S_CUT_LONGEST + threadIdx.x]);
}

// ---- per-cycle counts (include/kvarq_hip.h) ----
// How often every byte value stands at every position ("cycle") of the score lines and of the bases lines, positions
// 0 .. KVQ_CYCLES - 1.  A LANE IS A POSITION: the 64 lanes of a wave hold 64 consecutive bytes of one line, so their 64 adds go
// to 64 different LDS words on 32 different banks, whatever the bytes are (the byte histograms of kvq_profile_records queue
// on a few words instead).  1024 x 256 bins do not fit LDS: the positions are cut into slabs of W (blockIdx.y), and a
// workgroup keeps the HOT columns of its slab in LDS, 32-bit bins (a batch is < 4 GiB): score bytes '!' .. '~' and the bases
// A C G T N.  Any other byte goes straight to the array with a 64-bit atomic: input made of cold bytes costs speed, never
// results.
#define KVQ_CYC_SCORE_LO 33u
#define KVQ_CYC_SCORE_COLS 94u                                  // '!' .. '~'
#define KVQ_CYC_COLS (KVQ_CYC_SCORE_COLS + 5u)                  // ... and A C G T N
#define KVQ_CYC_SLAB 64u                                        // W; profiles/cycles_rate.txt has both widths, measured
#define KVQ_CYC_SLAB_ALT 128u
#define KVQ_CYC_RECORDS 4u                                      // records of a wave whose loads travel together

// the LDS column of a byte of a bases line; -1: cold
__device__ __forceinline__ int cyc_base_col(uint32_t b)
{
    return b == 'A' ? (int)KVQ_CYC_SCORE_COLS : b == 'C' ? (int)KVQ_CYC_SCORE_COLS + 1 : b == 'G' ? (int)KVQ_CYC_SCORE_COLS + 2
         : b == 'T' ? (int)KVQ_CYC_SCORE_COLS + 3 : b == 'N' ? (int)KVQ_CYC_SCORE_COLS + 4 : -1;
}

// Grid: x over record shares (a wave takes 64 consecutive records at a time, a record index a lane; grid-stride), y over the
// slabs slab0, slab0 + 1, ...  cyc: the array of include/kvarq_hip.h; behind it (cyc[kvq_cycles_len()]) one word of the
// kernel's own: the longest line of either kind so far, a running maximum like KVQ_PROF_LONGEST but true for score lines too.
// The launch of slab 0 raises it (every record reaches slab 0 or no slab); the launch of the other slabs, behind it on the
// stream, reads it, and a workgroup whose slab no line reaches returns at once.  Static LDS: KVQ_CYC_COLS * W words, column
// by column (word col * W + position: W is a multiple of 32, so the bank is the position's whatever the column).
template <uint32_t W>
__device__ __forceinline__ void cyc_slab(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, uint32_t slab0,
                                         unsigned long long *__restrict__ cyc)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned int bins[KVQ_CYC_COLS * W];
    constexpr uint32_t NG = W / 64u;
    constexpr size_t BASE = (size_t)KVQ_CYCLES * 256u, SCRATCH = 2u * BASE;
    const uint32_t p0 = (slab0 + blockIdx.y) * W;
    if (p0 >= KVQ_CYCLES) return;
    if (p0 > 0u && (unsigned long long)p0 >= cyc[SCRATCH]) return;           // (the same for the whole workgroup)
    for (uint32_t i = threadIdx.x; i < KVQ_CYC_COLS * W; i += blockDim.x) bins[i] = 0u;
    __syncthreads();

    const int lane = kvq_lane();
    uint32_t longest = 0;
    for (uint64_t g0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; g0 < nrec; g0 += (uint64_t)gridDim.x * 256u) {
        // lane l: record g0 + l (behind the last record: two empty lines)
        uint32_t boff = 0, L = 0, soff = 0, Q = 0;
        if (g0 + (uint32_t)lane < nrec) {
            uint32_t n[4];
            __builtin_memcpy(n, nl4 + 4u * (size_t)(g0 + (uint32_t)lane), 16);
            boff = n[0] + 1u; L = n[1] - n[0] - 1u; soff = n[2] + 1u; Q = n[3] - n[2] - 1u;
        }
        const uint32_t reach = L > Q ? L : Q;
        longest = reach > longest ? reach : longest;
        const unsigned long long todo = __ballot(reach > p0);
        for (uint32_t r = 0; r < 64u; r += KVQ_CYC_RECORDS) {
            if (!((todo >> r) & ((1ull << KVQ_CYC_RECORDS) - 1ull))) continue;
            // the loads of KVQ_CYC_RECORDS records first, a byte a lane and never a byte that is not of the line; then their adds
            uint32_t sb[KVQ_CYC_RECORDS][NG], bb[KVQ_CYC_RECORDS][NG], rL[KVQ_CYC_RECORDS], rQ[KVQ_CYC_RECORDS];
#pragma unroll
            for (uint32_t j = 0; j < KVQ_CYC_RECORDS; j++) {
                const uint32_t ro = (uint32_t)__builtin_amdgcn_readlane((int)boff, (int)(r + j)), so = (uint32_t)__builtin_amdgcn_readlane((int)soff, (int)(r + j));
                rL[j] = (uint32_t)__builtin_amdgcn_readlane((int)L, (int)(r + j)); rQ[j] = (uint32_t)__builtin_amdgcn_readlane((int)Q, (int)(r + j));
#pragma unroll
                for (uint32_t k = 0; k < NG; k++) {
                    const uint32_t p = p0 + 64u * k + (uint32_t)lane;
                    bb[j][k] = p < rL[j] ? data[(size_t)ro + p] : 0u;
                    sb[j][k] = p < rQ[j] ? data[(size_t)so + p] : 0u;
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < KVQ_CYC_RECORDS; j++) {
#pragma unroll
                for (uint32_t k = 0; k < NG; k++) {
                    const uint32_t at = 64u * k + (uint32_t)lane, p = p0 + at;
                    if (p < rQ[j]) {
                        const uint32_t col = sb[j][k] - KVQ_CYC_SCORE_LO;
                        if (col < KVQ_CYC_SCORE_COLS) atomicAdd(&bins[col * W + at], 1u);
                        else atomicAdd(&cyc[(size_t)p * 256u + sb[j][k]], 1ull);
                    }
                    if (p < rL[j]) {
                        const int col = cyc_base_col(bb[j][k]);
                        if (col >= 0) atomicAdd(&bins[(uint32_t)col * W + at], 1u);
                        else atomicAdd(&cyc[BASE + (size_t)p * 256u + bb[j][k]], 1ull);
                    }
                }
            }
        }
    }
    if (p0 == 0u) {
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)longest, d, 64); longest = o > longest ? o : longest; }
        if (lane == 0 && longest) atomicMax(&cyc[SCRATCH], (unsigned long long)longest);
    }
    __syncthreads();
    // the workgroup's bins that are not zero -> the array; consecutive threads take consecutive bytes of one position, which
    // are consecutive words of the array
    for (uint32_t i = threadIdx.x; i < KVQ_CYC_COLS * W; i += blockDim.x) {
        const uint32_t at = i / KVQ_CYC_COLS, col = i % KVQ_CYC_COLS;
        const unsigned int v = bins[col * W + at];
        if (!v) continue;
        const size_t word = col < KVQ_CYC_SCORE_COLS ? (size_t)(p0 + at) * 256u + KVQ_CYC_SCORE_LO + col
                                                     : BASE + (size_t)(p0 + at) * 256u + ((0x4E54474341ull >> (8u * (col - KVQ_CYC_SCORE_COLS))) & 0xFFu);      // "ACGTN"
        atomicAdd(&cyc[word], (unsigned long long)v);
    }
}

extern "C" __global__ void __launch_bounds__(256)
kvq_profile_cycles(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, uint32_t slab0, unsigned long long *__restrict__ cyc)
{
    cyc_slab<KVQ_CYC_SLAB>(data, nl4, nrec, slab0, cyc);
}
// (measurement, tools/cycles_rate.py: the other slab width)
extern "C" __global__ void __launch_bounds__(256)
kvq_profile_cycles_alt(const uint8_t *__restrict__ data, const uint32_t *__restrict__ nl4, uint32_t nrec, uint32_t slab0, unsigned long long *__restrict__ cyc)
{
    cyc_slab<KVQ_CYC_SLAB_ALT>(data, nl4, nrec, slab0, cyc);
}
