// kvarq_amd/csrc/kernels_deflate.hip -- the emitted reads, deflated to BGZF on the device (include/kvarq_hip.h):
// kvq_deflate_blocks makes one member of every block of 65 280 bytes of a text, a workgroup a block and a lane a segment, into
// a slot of its own; the members' sizes are prefix-summed (kvq_emit_scan_blocks) and kvq_deflate_gather moves the members side by
// side.  Everything that decides a byte of the output is kvq_deflate.h's, which the CPU twin runs too (kvq_deflate_bgzf_host):
// what is added to a histogram, OR-ed into the bit buffer or XOR-ed into the CRC by atomics commutes, so no launch geometry, no
// timing and no order of lanes changes a byte.
#include "kvq_device.h"
#include "kvq_host.h"
#include "kvq_deflate.h"
#include "../../include/kvarq_hip.h"

// a member's slot: two bytes of padding (the stream, 18 bytes into the member, then lies on a word), the member, and what fills
// the slot up to a multiple of sixteen (kvq_deflate_gather reads aligned blocks of sixteen bytes)
#define KVQ_DEFLATE_SLOT_PAD   2u
#define KVQ_DEFLATE_SLOT_BYTES 65552u
#define KVQ_DEFLATE_ROUND      2048u    // members that are in their slots at a time
#define KVQ_DEFLATE_TOKENS     (KVQ_DEFLATE_SEG * KVQ_DEFLATE_SEGS)      // tokens of a block at most: token t of lane l at [256 t + l]
static_assert(KVQ_DEFLATE_SLOT_BYTES % 16u == 0 && KVQ_DEFLATE_SLOT_PAD + KVQ_DEFLATE_MEMBER_MAX <= KVQ_DEFLATE_SLOT_BYTES, "a member fits its slot");
static_assert(KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS * 2u >= KVQ_DEFLATE_BLOCK + 8u, "the two table blocks hold every dynamic stream that is shorter than the stored one");
// words of the device array behind the eight that are the result: the bytes of the text's members so far, the bytes of a round's
#define KVQ_DEFLATE_D_BASE  8
#define KVQ_DEFLATE_D_TOTAL 9
#define KVQ_DEFLATE_D_WORDS 16

struct KvqLdsOr {
    static __host__ __device__ __forceinline__ void orw(uint32_t *w, uint32_t v)
    {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(w, v);
#else
        *w |= v;
#endif
    }
};

// what a lane's parse leaves: its tokens in its column of the workgroup's token block, their symbols in the histograms
struct KvqDeflateLaneSink {
    KvqDeflatePlan *P; uint32_t *tok; uint32_t ntok, matches, maxd, maxl;
    __device__ __forceinline__ void literal(uint8_t b) { tok[(size_t)ntok++ * KVQ_DEFLATE_SEGS] = b; atomicAdd(&P->ll_freq[b], 1u); }
    __device__ __forceinline__ void match(uint32_t len, uint32_t dist)
    {
        uint32_t s, n, e;
        tok[(size_t)ntok++ * KVQ_DEFLATE_SEGS] = KVQ_DEFLATE_TOKEN_MATCH | (len << 16) | dist;
        kvq_deflate_len_sym(len, s, n, e); atomicAdd(&P->ll_freq[s], 1u);
        kvq_deflate_dist_sym(dist, s, n, e); atomicAdd(&P->d_freq[s], 1u);
        matches++; maxd = dist > maxd ? dist : maxd; maxl = len > maxl ? len : maxl;
    }
};

// Blocks [first, first + nblocks) of text[0, nbytes), a workgroup of 256 a block, grid-stride: block first + k becomes the member in
// slot k, sizes[k] and lens[k] its bytes.  The block lies in LDS (64 KB) beside the two table blocks (64 KB, which hold the bits
// once the parse is over) and the plan: ~137 KB, one workgroup a compute unit.  tokens: KVQ_DEFLATE_TOKENS words per workgroup OF
// THE GRID.  words[0, 8) take the members' sums and maxima.
extern "C" __global__ void __launch_bounds__(256)
kvq_deflate_blocks(const uint8_t *__restrict__ text, uint64_t nbytes, uint64_t first, uint32_t nblocks, uint8_t *__restrict__ slots,
                   unsigned long long *__restrict__ sizes, uint32_t *__restrict__ lens, uint32_t *__restrict__ tokens, unsigned long long *__restrict__ words)
{
    KVQ_BESIDE_SCAN();
    __shared__ uint32_t blkw[KVQ_DEFLATE_BLOCK / 4u];
    __shared__ uint32_t tabw[KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS * 2u / 4u];
    __shared__ KvqDeflatePlan P;
    __shared__ uint32_t crc_table[256];
    __shared__ unsigned long long scan_lds[4];
    __shared__ uint32_t red[4];                          // of the block: its CRC, its matches, its longest distance and match
    const uint32_t tid = threadIdx.x;
    uint8_t *const blk = (uint8_t *)blkw, *const own = (uint8_t *)tabw, *const fin = own + KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS;
    uint32_t *const tok = tokens + (size_t)blockIdx.x * KVQ_DEFLATE_TOKENS + tid;
    crc_table[tid] = kvq_crc_entry(tid);
    for (uint32_t k = blockIdx.x; k < nblocks; k += gridDim.x) {
        const uint64_t at = (first + k) * (uint64_t)KVQ_DEFLATE_BLOCK;
        const uint32_t n = (uint32_t)(nbytes - at < KVQ_DEFLATE_BLOCK ? nbytes - at : KVQ_DEFLATE_BLOCK);
        const uint8_t *src = text + at;
        // the block into LDS: whole words where the text lies on one, never a byte behind the block's last
        if (((uintptr_t)src & 3u) == 0u) {
            for (uint32_t w = tid; w < n / 4u; w += 256u) blkw[w] = ((const uint32_t *)src)[w];
            if (tid < (n & 3u)) blk[(n & ~3u) + tid] = src[(n & ~3u) + tid];
        } else {
            for (uint32_t i = tid; i < n; i += 256u) blk[i] = src[i];
        }
        for (uint32_t i = tid; i < 288u; i += 256u) P.ll_freq[i] = 0u;
        if (tid < 32u) P.d_freq[tid] = 0u;
        if (tid < 4u) red[tid] = 0u;
        __syncthreads();
        kvq_deflate_final_table(blk, n, tid, fin);
        __syncthreads();
        KvqDeflateLaneSink sink = { &P, tok, 0u, 0u, 0u, 0u };
        kvq_deflate_parse(blk, n, tid, own, fin, sink);
        {
            // the segment's own CRC, moved to the front by the bytes behind the segment
            const uint32_t sb = kvq_deflate_seg_begin(tid, n), se = kvq_deflate_seg_begin(tid + 1u, n);
            if (se > sb) atomicXor(&red[0], kvq_crc_mul(kvq_crc_shift(n - se), kvq_crc_bytes(crc_table, 0u, blk + sb, se - sb)));
            if (sink.matches) { atomicAdd(&red[1], sink.matches); atomicMax(&red[2], sink.maxd); atomicMax(&red[3], sink.maxl); }
        }
        __syncthreads();
        if (tid == 0u) { P.ll_freq[256] = 1u; kvq_deflate_plan(&P, n); }
        __syncthreads();
        const uint32_t stream = kvq_deflate_stream_bytes(&P, n), member = KVQ_BGZF_HEADER + stream + KVQ_BGZF_TRAILER;
        uint8_t *const slot = slots + (size_t)k * KVQ_DEFLATE_SLOT_BYTES + KVQ_DEFLATE_SLOT_PAD;
        uint8_t *const body = slot + KVQ_BGZF_HEADER;          // (on a word)
        if (tid < KVQ_BGZF_HEADER) slot[tid] = kvq_bgzf_header_byte(tid, member);
        if (P.stored) {
            if (tid < 5u) body[tid] = kvq_deflate_stored_byte(tid, n);
            for (uint32_t i = tid; i < n; i += 256u) body[5u + i] = blk[i];
        } else {
            // (the tables are over: their bytes are the bit buffer)
            for (uint32_t w = tid; w < KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS * 2u / 4u; w += 256u) tabw[w] = 0u;
            uint32_t bits = 0;
            for (uint32_t t = 0; t < sink.ntok; t++) bits += kvq_deflate_token_bits(&P, tok[(size_t)t * KVQ_DEFLATE_SEGS]);
            unsigned long long all;
            const uint32_t ahead = (uint32_t)emit_block_scan(bits, scan_lds, all);      // (its barriers stand behind the zeroing)
            KvqBitsOut<KvqLdsOr> o;
            if (tid == 0u) {
                o.open(tabw, 0u);
                kvq_deflate_put_header(&P, o);
                o.close();
                o.open(tabw, P.total_bits - P.ll_len[256]);
                o.put(P.ll_code[256], P.ll_len[256]);
                o.close();
            }
            o.open(tabw, P.header_bits + ahead);
            for (uint32_t t = 0; t < sink.ntok; t++) kvq_deflate_put_token(&P, tok[(size_t)t * KVQ_DEFLATE_SEGS], o);
            o.close();
            __syncthreads();
            for (uint32_t w = tid; w < (stream + 3u) / 4u; w += 256u) ((uint32_t *)body)[w] = tabw[w];
        }
        __syncthreads();                                 // (the last word of the stream may reach into the trailer's bytes)
        if (tid < 4u) body[stream + tid] = (uint8_t)(red[0] >> (8u * tid));
        else if (tid < 8u) body[stream + tid] = (uint8_t)(n >> (8u * (tid - 4u)));
        if (tid == 0u) {
            sizes[k] = member; lens[k] = member;
            unsigned long long lits = 0;
            for (uint32_t s = 0; s < 256u; s++) lits += P.ll_freq[s];
            atomicAdd(&words[KVQ_DEFLATE_MEMBERS], 1ull); atomicAdd(&words[KVQ_DEFLATE_BYTES_IN], (unsigned long long)n);
            atomicAdd(&words[KVQ_DEFLATE_BYTES_OUT], (unsigned long long)member);
            if (P.stored) atomicAdd(&words[KVQ_DEFLATE_STORED], 1ull);
            else {
                // (the parse's words count where its tokens are the stream)
                if (red[1]) atomicAdd(&words[KVQ_DEFLATE_MATCHES], (unsigned long long)red[1]);
                atomicAdd(&words[KVQ_DEFLATE_LITERALS], lits);
                atomicMax(&words[KVQ_DEFLATE_MAX_DISTANCE], (unsigned long long)red[2]); atomicMax(&words[KVQ_DEFLATE_MAX_LENGTH], (unsigned long long)red[3]);
            }
        }
        __syncthreads();                                 // (the block, the plan and the sums are the next block's)
    }
}

// The members of slots [0, nblocks) to out + *base + off[k], off the exclusive prefix sums of their sizes: sixteen lanes a piece of
// 4096 bytes through emit_copy, which writes no byte outside its piece.  A member that would reach beyond out[0, cap) stays where it is.
extern "C" __global__ void __launch_bounds__(256)
kvq_deflate_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ lens, const unsigned long long *__restrict__ off, uint32_t nblocks,
                   const unsigned long long *__restrict__ base, uint8_t *__restrict__ out, uint64_t cap)
{
    KVQ_BESIDE_SCAN();
    const uint32_t piece = (threadIdx.x >> 4) * 4096u, sub = threadIdx.x & 15u;
    for (uint32_t k = blockIdx.x; k < nblocks; k += gridDim.x) {
        const uint32_t len = lens[k];
        const unsigned long long to = *base + off[k];
        if (to + len > cap || piece >= len) continue;
        emit_copy(slots + (size_t)k * KVQ_DEFLATE_SLOT_BYTES + KVQ_DEFLATE_SLOT_PAD + piece, len - piece < 4096u ? len - piece : 4096u, out + to + piece, sub);
    }
}
// the round's bytes join the bytes so far
extern "C" __global__ void kvq_deflate_advance(unsigned long long *words)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) words[KVQ_DEFLATE_D_BASE] += words[KVQ_DEFLATE_D_TOTAL];
}

// BGZF(d_text[0, nbytes)) to d_out[0, cap) on `stream`, round after round of KVQ_DEFLATE_ROUND members; B.words is cleared first and
// holds the eight words, and the bytes of all members in word KVQ_DEFLATE_D_BASE, when the stream has run.  Waits for nothing.
int kvq_deflate_enqueue(const uint8_t *d_text, uint64_t nbytes, uint8_t *d_out, uint64_t cap, KvqDeflateBufs &B, hipStream_t stream)
{
    int rc;
    const uint64_t members = kvq_deflate_members(nbytes);
    // (KVQ_DEFLATE_ROUND, for tests: fewer members a round, so that a small text takes several)
    const char *env = getenv("KVQ_DEFLATE_ROUND");
    const long wish = env ? atol(env) : 0;
    const uint32_t round = (uint32_t)std::min<uint64_t>(members, wish >= 1 && wish < (long)KVQ_DEFLATE_ROUND ? (uint64_t)wish : KVQ_DEFLATE_ROUND);
    const uint32_t cus = std::max<uint32_t>(kvq_device_cu_count(), 1u);
    const uint32_t grid = std::max<uint32_t>(std::min<uint32_t>(round, cus), 1u);
    if ((rc = B.words.ensure(KVQ_DEFLATE_D_WORDS * 8))) return rc;
    KVQ_HIP(hipMemsetAsync(B.words.p, 0, KVQ_DEFLATE_D_WORDS * 8, stream));
    if (!members) return KVQ_OK;
    if ((rc = B.slots.ensure((size_t)round * KVQ_DEFLATE_SLOT_BYTES)) || (rc = B.sizes.ensure((size_t)round * 8)) || (rc = B.lens.ensure((size_t)round * 4)) ||
        (rc = B.tokens.ensure((size_t)grid * KVQ_DEFLATE_TOKENS * 4))) return rc;
    unsigned long long *const words = B.words.as<unsigned long long>();
    for (uint64_t first = 0; first < members; first += round) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(round, members - first);
        hipLaunchKernelGGL(kvq_deflate_blocks, dim3(std::min(nb, grid)), dim3(256), 0, stream, d_text, nbytes, first, nb, B.slots.as<uint8_t>(),
                           B.sizes.as<unsigned long long>(), B.lens.as<uint32_t>(), B.tokens.as<uint32_t>(), words);
        hipLaunchKernelGGL(kvq_emit_scan_blocks, dim3(1), dim3(256), 0, stream, B.sizes.as<unsigned long long>(), nb, words + KVQ_DEFLATE_D_TOTAL);
        hipLaunchKernelGGL(kvq_deflate_gather, dim3(std::min<uint32_t>(nb, 4096u)), dim3(256), 0, stream, (const uint8_t *)B.slots.as<uint8_t>(), (const uint32_t *)B.lens.as<uint32_t>(),
                           (const unsigned long long *)B.sizes.as<unsigned long long>(), nb, (const unsigned long long *)(words + KVQ_DEFLATE_D_BASE), d_out, cap);
        hipLaunchKernelGGL(kvq_deflate_advance, dim3(1), dim3(64), 0, stream, words);
        KVQ_HIP(hipGetLastError());
    }
    return KVQ_OK;
}
void kvq_deflate_release(KvqDeflateBufs &B) { for (DevBuf *b : { &B.slots, &B.sizes, &B.lens, &B.tokens, &B.words }) b->release(); }

extern "C" int64_t kvq_deflate_bgzf_device(const void *d_text, int64_t nbytes, void *d_out, int64_t out_cap, int64_t *out_words)
{
    kvq_clear_error();
    if (nbytes < 0 || out_cap < 0 || !out_words || (nbytes > 0 && !d_text) || (out_cap > 0 && !d_out)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_deflate_bgzf_device: bad arguments"); return -1;
    }
    KvqDeflateBufs B;
    unsigned long long h[KVQ_DEFLATE_D_WORDS];
    int rc = kvq_deflate_enqueue((const uint8_t *)d_text, (uint64_t)nbytes, (uint8_t *)d_out, (uint64_t)out_cap, B, 0);
    hipError_t e = hipSuccess;
    if (!rc && (e = hipMemcpyAsync(h, B.words.p, sizeof h, hipMemcpyDeviceToHost, 0)) == hipSuccess) e = hipStreamSynchronize(0);
    if (rc) (void)hipStreamSynchronize(0);
    kvq_deflate_release(B);
    if (rc) return -1;
    if (e != hipSuccess) { kvq_set_error(KVQ_ERR_DEVICE, "kvq_deflate_bgzf_device: %s", hipGetErrorString(e)); return -1; }
    for (int i = 0; i < KVQ_DEFLATE_WORDS; i++) out_words[i] = (int64_t)h[i];
    if (h[KVQ_DEFLATE_D_BASE] > (uint64_t)out_cap) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_deflate_bgzf_device: the text takes %llu bytes, out_cap is %lld", h[KVQ_DEFLATE_D_BASE], (long long)out_cap);
        return -1;
    }
    return (int64_t)h[KVQ_DEFLATE_D_BASE];
}
