// kvarq_amd/csrc/kernels_inflate.hip -- BGZF members inflated on the GPU, the BGZF block index of a
// file's bytes, and the host entry of the shared decoder (kvq_inflate.h).
//
// One wavefront per member: the wave runs the decoder of kvq_inflate.h together (every lane the same bit reader,
// lane 0 the literals, the wave the tables and the copies of back-references and stored blocks) into a 32 KiB ring
// in LDS -- DEFLATE's whole window: a back-reference reads bytes the wave has just written, LDS keeps that inside
// the wave -- which the wave streams to the member's place in the output whenever the next write would overwrite
// bytes not yet stored.  38 KB of LDS a member: four members in flight per CU.
#include "kvq_host.h"
#include "kvq_inflate.h"

#include <string.h>

#define KVQ_CUT_CAP 4096                  // chunk starts one launch of kvq_cut_chunks writes at most

#define KVQ_INF_RING 32768u               // DEFLATE's window: no distance reaches further back

// the device's output of kvq_inflate_core: a ring of the last 32 KiB in LDS; bytes [f, o) are in the ring only
struct KvqRingOut {
    uint8_t *ring, *dst; uint32_t f;
    template <class G> __device__ __forceinline__ void flush(const G &g, uint32_t o)
    {
        g.sync();
        for (uint32_t i = f + (uint32_t)g.lane(); i < o; i += G::width) dst[i] = ring[i & (KVQ_INF_RING - 1u)];
        f = o;
        g.sync();                                         // (the slots just stored are written again next)
    }
    template <class G> __device__ __forceinline__ void room(const G &g, uint32_t o, uint32_t len) { if (o + len - f > KVQ_INF_RING) flush(g, o); }
    template <class G> __device__ __forceinline__ void lit(const G &g, uint32_t o, uint8_t v)
    {
        room(g, o, 1);
        if (g.lane() == 0) ring[o & (KVQ_INF_RING - 1u)] = v;
    }
    template <class G> __device__ __forceinline__ void stored(const G &g, uint32_t o, const uint8_t *src, uint32_t len)
    {
        for (uint32_t a = 0; a < len; a += 4096) {
            const uint32_t m = len - a < 4096 ? len - a : 4096;
            room(g, o + a, m);
            for (uint32_t i = (uint32_t)g.lane(); i < m; i += G::width) ring[(o + a + i) & (KVQ_INF_RING - 1u)] = src[a + i];
        }
    }
    // (dist <= 32 KiB: a source byte's slot is written by this copy only at or after the lane that reads it, in the same or a later round)
    template <class G> __device__ __forceinline__ void copy(const G &g, uint32_t o, uint32_t dist, uint32_t len)
    {
        room(g, o, len);
        g.sync();
        const uint32_t s0 = o - dist;
        if (dist >= len) for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) ring[(o + i) & (KVQ_INF_RING - 1u)] = ring[(s0 + i) & (KVQ_INF_RING - 1u)];
        else for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) ring[(o + i) & (KVQ_INF_RING - 1u)] = ring[(s0 + i % dist) & (KVQ_INF_RING - 1u)];
    }
    template <class G> __device__ __forceinline__ void finish(const G &g, uint32_t o) { flush(g, o); }
};

struct KvqWaveGroup {
    static constexpr int width = KVQ_WAVE;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }      // (a workgroup is one wave)
};

// entry b of the table -> out[out_off, out_off + isize), status[b].  An entry that points outside in[0, in_bytes)
// or out[0, out_bytes), or whose isize exceeds 64 KiB, gets KVQ_INF_STREAM_ERROR and touches nothing; a member that
// does not inflate gets its status, and what it had streamed out before it failed stays in its slot (never beyond it).
extern "C" __global__ void __launch_bounds__(KVQ_WAVE)
kvq_inflate_bgzf(const uint8_t *__restrict__ in, int64_t in_bytes, const kvq_bgzf_block *__restrict__ tab, int64_t nblocks,
                 uint8_t *__restrict__ out, int64_t out_bytes, int32_t *__restrict__ status)
{
    __shared__ KvqInflateWork ws;
    __shared__ uint8_t ring[KVQ_INF_RING];
    const KvqWaveGroup g;
    const int lane = (int)threadIdx.x;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const kvq_bgzf_block e = tab[b];
        int st;
        if (e.in_off < 0 || e.out_off < 0 || e.isize > KVQ_INF_MAX_ISIZE || e.in_off > in_bytes || (int64_t)e.in_len > in_bytes - e.in_off ||
            e.out_off > out_bytes || (int64_t)e.isize > out_bytes - e.out_off)
            st = KVQ_INF_STREAM_ERROR;
        else {
            KvqRingOut w; w.ring = ring; w.dst = out + e.out_off; w.f = 0;
            st = kvq_inflate_core(g, &ws, in + e.in_off, (int64_t)e.in_len, w, e.isize);
        }
        if (lane == 0) status[b] = st;
        __syncthreads();                                  // (the ring and the tables are the next member's)
    }
}

int kvq_inflate_bgzf_launch(const uint8_t *d_in, int64_t in_bytes, const kvq_bgzf_block *d_tab, int64_t nblocks,
                            uint8_t *d_out, int64_t out_bytes, int32_t *d_status, hipStream_t stream)
{
    if (nblocks <= 0) return KVQ_OK;
    const int64_t grid = nblocks < (1 << 20) ? nblocks : (1 << 20);
    hipLaunchKernelGGL(kvq_inflate_bgzf, dim3((uint32_t)grid), dim3(KVQ_WAVE), 0, stream, d_in, in_bytes, d_tab, nblocks, d_out, out_bytes, d_status);
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

extern "C" int32_t kvq_inflate_bgzf_device(const void *d_in, int64_t in_bytes, const kvq_bgzf_block *d_blocks, int64_t nblocks,
                                           void *d_out, int64_t out_bytes, int32_t *d_status)
{
    kvq_clear_error();
    if (nblocks < 0 || in_bytes < 0 || out_bytes < 0 || (nblocks > 0 && (!d_in || !d_blocks || !d_out || !d_status))) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_inflate_bgzf_device: bad arguments"); return KVQ_ERR_RUNTIME;
    }
    int rc = kvq_inflate_bgzf_launch((const uint8_t *)d_in, in_bytes, d_blocks, nblocks, (uint8_t *)d_out, out_bytes, d_status, 0);
    if (rc) return rc;
    KVQ_HIP(hipStreamSynchronize(0));
    return KVQ_OK;
}

extern "C" int32_t kvq_inflate_raw_host(const uint8_t *in, int64_t n, uint8_t *out, int64_t isize)
{
    if (n < 0 || isize < 0 || isize > KVQ_INF_MAX_ISIZE || (!in && n > 0) || (!out && isize > 0)) return KVQ_INF_STREAM_ERROR;
    KvqInflateWork ws;
    KvqFlatOut w; w.out = out;
    return kvq_inflate_core(KvqSerialGroup(), &ws, in, n, w, (uint32_t)isize);
}

// is there a BGZF block at offset `off` of a file of `size` bytes?  read(dst, bytes, at) -> bytes read.  The host reader's
// acceptance rules (StreamSource::bgzf_peek): exactly FEXTRA, a 'BC' subfield of two bytes, ISIZE <= 64 KiB.
template <class Read>
static bool kvq_bgzf_peek(Read &&read, int64_t size, int64_t off, kvq_bgzf_entry_ *b)
{
    uint8_t h[12];
    if (off + 28 > size || read(h, 12, off) != 12) return false;
    if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || h[3] != 4) return false;
    const uint32_t xlen = h[10] | (h[11] << 8);
    if (xlen < 6 || xlen > 4096) return false;
    uint8_t x[4096];
    if (read(x, xlen, off + 12) != (int64_t)xlen) return false;
    uint32_t bsize = 0;
    for (uint32_t i = 0; i + 4 <= xlen; ) {
        const uint32_t slen = x[i + 2] | (x[i + 3] << 8);
        if (x[i] == 'B' && x[i + 1] == 'C' && slen == 2 && i + 6 <= xlen) bsize = (x[i + 4] | (x[i + 5] << 8)) + 1u;
        i += 4 + slen;
    }
    const uint32_t hdr = 12 + xlen;
    if (bsize < hdr + 8 || off + bsize > size) return false;
    uint8_t t[4];
    if (read(t, 4, off + bsize - 4) != 4) return false;
    b->off = off; b->size = bsize; b->hdr = hdr;
    b->isize = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
    return b->isize <= KVQ_INF_MAX_ISIZE;
}

// every block of a file that is BGZF to its end (at most 10 trailing bytes, as the host reader accepts); false otherwise
template <class Read>
static bool kvq_bgzf_walk(Read &&read, int64_t size, std::vector<kvq_bgzf_entry_> &blocks)
{
    blocks.clear();
    int64_t off = 0;
    do {
        kvq_bgzf_entry_ b;
        if (!kvq_bgzf_peek(read, size, off, &b)) return false;
        blocks.push_back(b); off += b.size;
    } while (size - off > 10);
    return true;
}

extern "C" int64_t kvq_bgzf_index(const uint8_t *file_bytes, int64_t n, int64_t *block_off, uint32_t *csize, uint32_t *isize, int64_t cap)
{
    if (!file_bytes || n <= 0) return -1;
    auto read = [&](uint8_t *dst, int64_t k, int64_t at) -> int64_t {
        const int64_t m = at >= n ? 0 : (k < n - at ? k : n - at);
        if (m > 0) memcpy(dst, file_bytes + at, (size_t)m);
        return m;
    };
    std::vector<kvq_bgzf_entry_> blocks;
    if (!kvq_bgzf_walk(read, n, blocks)) return -1;
    for (size_t i = 0; i < blocks.size() && (int64_t)i < cap; i++) {
        if (block_off) block_off[i] = blocks[i].off;
        if (csize) csize[i] = blocks[i].size;
        if (isize) isize[i] = blocks[i].isize;
    }
    return (int64_t)blocks.size();
}

// The chunk cuts of fastq_read (workhorse.c:696-718, 916-943; kvq_chunk_offsets on the host) over inflated text in device
// memory, by one wave: from chunk start cs, while cs + 1 MiB <= have, the next start is the line-start '@' in front of the
// last line-start '+' of text[cs + 2, cs + 1 MiB) (kvq_tail_record).  The wave walks back 64 bytes a step, a lane a byte,
// and takes both from two ballots.  Writes at most cap starts to offs; res: {chunks, cs, fill, error, want, end} -- fill is
// where the reference's buffer ends (the last cut's 1 MiB mark); error = no record start in a window, with the numbers of
// the host route's message.
extern "C" __global__ void __launch_bounds__(KVQ_WAVE)
kvq_cut_chunks(const uint8_t *__restrict__ text, int64_t have, int64_t cs, int64_t fill, int64_t *__restrict__ offs, int64_t cap,
               int64_t *__restrict__ res)
{
    const int lane = (int)threadIdx.x;
    int64_t n = 0, err = 0, want = 0, err_end = 0;
    while (cs + KVQ_SCANBUFSIZE <= have && n < cap) {
        const int64_t end = cs + KVQ_SCANBUFSIZE;
        bool plus_seen = false;
        int64_t at = -1;
        for (int64_t hi = end - 1; hi >= cs + 2 && at < 0; hi -= KVQ_WAVE) {
            const int64_t k = hi - lane;
            const bool in = k >= cs + 2;
            const uint8_t c = in ? text[k] : 0, prev = in ? text[k - 1] : 0;
            const bool ls = prev == '\n' || prev == '\r';
            const uint64_t P = __ballot(ls && c == '+');
            uint64_t A = __ballot(ls && c == '@');
            if (!plus_seen) {
                if (!P) continue;
                plus_seen = true;
                const int lp = __builtin_ctzll(P);            // the highest '+' of the window: an '@' must lie in front of it
                A = lp == 63 ? 0 : A & ~((2ull << lp) - 1ull);
            }
            if (A) at = hi - __builtin_ctzll(A);
        }
        if (at < 0) { err = 1; want = end - fill; err_end = end; break; }
        if (lane == 0) offs[n] = cs;
        n++; cs = at; fill = end;
    }
    if (lane == 0) { res[0] = n; res[1] = cs; res[2] = fill; res[3] = err; res[4] = want; res[5] = err_end; }
}

int kvq_cut_chunks_launch(const uint8_t *d_text, int64_t have, int64_t cs, int64_t fill, int64_t *d_offs, int64_t cap, int64_t *d_res, hipStream_t stream)
{
    hipLaunchKernelGGL(kvq_cut_chunks, dim3(1), dim3(KVQ_WAVE), 0, stream, d_text, have, cs, fill, d_offs, cap, d_res);
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

// kvq_chunk_offsets for text in device memory, by kvq_cut_chunks
extern "C" int64_t kvq_chunk_offsets_device(const void *d_data, int64_t nbytes, int64_t *offsets, int64_t cap)
{
    kvq_clear_error();
    int64_t *d_res = nullptr;
    if (hipMalloc((void **)&d_res, (8 + KVQ_CUT_CAP) * 8) != hipSuccess) { (void)hipGetLastError(); kvq_set_error(KVQ_ERR_DEVICE, "hipMalloc failed"); return -1; }
    std::vector<int64_t> res(8 + KVQ_CUT_CAP);
    int64_t n = 0, cs = 0, fill = 0, out = 0;
    for (;;) {
        if (kvq_cut_chunks_launch((const uint8_t *)d_data, nbytes, cs, fill, d_res + 8, KVQ_CUT_CAP, d_res, 0) ||
            hipMemcpy(res.data(), d_res, res.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); out = -1; break; }
        if (res[3]) { kvq_set_error(KVQ_ERR_RUNTIME, "could find beginning of record; read %ld bytes up to %ld", (long)res[4], (long)res[5]); out = -1; break; }
        for (int64_t i = 0; i < res[0]; i++, n++) if (n < cap) offsets[n] = res[8 + i];
        cs = res[1]; fill = res[2];
        if (res[0] < KVQ_CUT_CAP) break;
    }
    (void)hipFree(d_res);
    if (out < 0) return -1;
    if (nbytes > cs) { if (n < cap) offsets[n] = cs; n++; }
    if (n < cap + 1) offsets[n] = nbytes;
    return n;
}
