// kvarq_amd/csrc/kernels_clip.hip -- the adapter clip of a scan (include/kvarq_hip.h): in front of a batch's scan the
// score bytes of every record from its adapter's first base on become '!' (Phred 0), so that no trim, whichever kernel does it,
// reaches into the adapter.  kvq_clip_records walks the record index (kvq_index_records), finds CLIP on the bases line as
// kvq_adapt_records does (its helpers: kernels_adapt.hip, which stays as it is) and writes nothing but the bytes [CLIP, S) of the
// score line and its four sums; it reads no byte outside the bases line and its terminator, and the last byte of the score line.
#include "kvq_device.h"
#include "../../include/kvarq_hip.h"

#define KVQ_CLIP_BYTE 0x21u                              // '!'

// '!' over data[a, b) by the sixteen lanes of a quarter, lane `sub` taking the 16-byte blocks sub, sub + 16, ... counted from the
// aligned block that holds a: a whole block inside the range is one 16-byte store, an aligned word inside it one dword store, and
// the bytes of the two ragged ends go one by one.  No byte outside [a, b) is read or written
__device__ __forceinline__ void clip_store(uint8_t *data, uint64_t a, uint64_t b, uint32_t sub)
{
    const uintptr_t base = (uintptr_t)data;
    const uintptr_t A = base + a, B = base + b;
    for (uintptr_t blk = (A & ~(uintptr_t)15) + 16u * sub; blk < B; blk += 256u) {
        if (blk >= A && blk + 16u <= B) {
            *(uint4 *)blk = make_uint4(0x21212121u, 0x21212121u, 0x21212121u, 0x21212121u);
            continue;
        }
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const uintptr_t w = blk + 4u * d;
            if (w >= A && w + 4u <= B) *(uint32_t *)w = 0x21212121u;
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) if (w + j >= A && w + j < B) *(uint8_t *)(w + j) = (uint8_t)KVQ_CLIP_BYTE;
            }
        }
    }
}

// Records [0, nrec) of the batch, N probes (an instantiation for every N, as kvq_adapt_records).  A QUARTER-WAVE A RECORD: the
// whole 16-byte index entry (n2 and n3 bound the score line), then the search of kvq_adapt_records word for word -- adapt_load16,
// adapt_codes, rounds of 224 positions with nothing carried, the 16-bit pre-test, the tail test on the last 32 bytes -- which
// leaves CLIP in all sixteen lanes.  Where CLIP < L the sixteen lanes store '!' over [CLIP, S) of the score line (clip_store), S
// its length less a trailing '\r'.  A quarter's first lane keeps the record's share of the four sums; they are reduced over the
// workgroup in LDS and go to the array with one 64-bit atomic a word that is not zero.  Grid-stride over waves, the index entry of
// a wave's next records loaded a step ahead.
template <int N> __global__ void __launch_bounds__(256)
kvq_clip_records(uint8_t *data, const uint32_t *__restrict__ nl4, uint32_t nrec, KvqAdaptProbes P, unsigned long long *__restrict__ out)
{
    KVQ_BESIDE_SCAN();
    __shared__ unsigned long long clip_lds[4];
    if (threadIdx.x < 4u) clip_lds[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = kvq_lane();
    const uint32_t sub = (uint32_t)lane & 15u, quarter = (uint32_t)lane >> 4;
    const bool own = sub < 14u;
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
        // the last 32 bytes of the line as it lies (all of a shorter line), for the tails: as kvq_adapt_records
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
        uint32_t clip = L;
#pragma unroll
        for (int k = 0; k < N; k++) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                first[k] = min(first[k], (uint32_t)__shfl_xor((int)first[k], d, 64));
                tail[k] = max(tail[k], (uint32_t)__shfl_xor((int)tail[k], d, 64));
            }
            if (first[k] != KVQ_ADAPT_NONE) clip = min(clip, first[k]);       // (TAIL_k only where FIRST_k is none)
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

// the instantiation for n probes, 1 <= n <= KVQ_ADAPT_MAX_PROBES
typedef void (*KvqClipKernel)(uint8_t *, const uint32_t *, uint32_t, KvqAdaptProbes, unsigned long long *);
static KvqClipKernel kvq_clip_kernel(uint32_t n)
{
    switch (n) {
    case 1: return kvq_clip_records<1>;
    case 2: return kvq_clip_records<2>;
    case 3: return kvq_clip_records<3>;
    case 4: return kvq_clip_records<4>;
    case 5: return kvq_clip_records<5>;
    case 6: return kvq_clip_records<6>;
    case 7: return kvq_clip_records<7>;
    default: return kvq_clip_records<8>;
    }
}
