// kvarq_amd/csrc/kernels_clip.hip -- the adapter clip of a scan (include/kvarq_hip.h): in front of a batch's scan the
// score bytes of every record from its adapter's first base on become '!' (Phred 0), so that no trim, whichever kernel does it,
// reaches into the adapter.  kvq_clip_records walks the record index (kvq_index_records), finds CLIP on the bases line with the
// search kvq_adapt_records uses (adapt_search, kernels_adapt.hip: the exact one or the tolerant one, as its probes say) and writes
// nothing but the bytes [CLIP, S) of the score line and its four sums; it reads no byte outside the bases line and its terminator,
// and the last byte of the score line.  The file ends with the one table of both sinks' instantiations.
#pragma once
#include "kernels_adapt.hip"
#include <array>
#include <utility>

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

// THE CLIP SINK.  Records [0, nrec) of the batch, N probes (an instantiation for every N, as kvq_adapt_records), the search of
// `Probes`.  A QUARTER-WAVE A RECORD: the whole 16-byte index entry (n2 and n3 bound the score line), then adapt_search, which
// leaves L, FIRST_k and TAIL_k, and so CLIP, in all sixteen lanes.  Where CLIP < L the sixteen lanes store '!' over [CLIP, S) of the
// score line (clip_store), S its length less a trailing '\r'.  A quarter's first lane keeps the record's share of the four sums;
// they are reduced over the workgroup in LDS and go to the array with one 64-bit atomic a word that is not zero.  ([5] = per is no
// sum: the host sets it.)  Grid-stride over waves, the index entry of a wave's next records loaded a step ahead.
template <int N, class Probes> __global__ void __launch_bounds__(256)
kvq_clip_records(uint8_t *data, const uint32_t *__restrict__ nl4, uint32_t nrec, Probes P, unsigned long long *__restrict__ out)
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
        adapt_search<N>(line, Lraw, top, P, lane, sub, L, first, dist, tail);
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

// THE INSTANTIATIONS of both sinks for the probes `Probes`: row n - 1 has those for n probes, 1 <= n <= KVQ_ADAPT_MAX_PROBES
template <class Probes> struct KvqProbeKernels {
    void (*adapt)(const uint8_t *, const uint32_t *, uint32_t, Probes, unsigned long long *);
    void (*clip)(uint8_t *, const uint32_t *, uint32_t, Probes, unsigned long long *);
};
template <class Probes, size_t... I>
static constexpr std::array<KvqProbeKernels<Probes>, sizeof...(I)> kvq_probe_kernel_rows(std::index_sequence<I...>)
{
    return { { { kvq_adapt_records<(int)I + 1, Probes>, kvq_clip_records<(int)I + 1, Probes> }... } };
}
template <class Probes> static const KvqProbeKernels<Probes> &kvq_probe_kernels(uint32_t n)
{
    static constexpr auto rows = kvq_probe_kernel_rows<Probes>(std::make_index_sequence<KVQ_ADAPT_MAX_PROBES>());
    return rows[n - 1u];
}
