// kvarq_amd/csrc/kernels_gzip.hip -- plain gzip inflated by speculative chunk decoding: the kernels of the
// four phases, and one chunked algorithm over them that the host runs with the same decoder on the CPU (kvq_inflate_gzip_host)
// or on the GPU (kvq_inflate_gzip_device, and the device route of kvq_findseqs_ex).
//
// A run is a span of one file's compressed bytes that starts at a block boundary already known.  It is cut into chunks of
// chunk_bytes; (1) the block finder puts each chunk's start at the first bit offset behind its nominal start that carries a
// dynamic-Huffman header kvq_dyn_header accepts (a chunk without one is merged into the one before); (2) one wave per chunk
// decodes from there to the first block boundary at or past the next chunk's start, the 32 KiB in front unknown: 16-bit
// symbols, markers for the unknown window; (3) the host checks the chain -- chunk k+1 holds when decoder k ended exactly at
// its start, else it is decoded again from where decoder k ended -- until every chunk holds; (4) one workgroup resolves the
// chunks' windows one after the other; (5) a parallel pass replaces the markers and writes the bytes, packed, to the text.
#include "kvq_host.h"
#include "kvq_inflate.h"

#include <string.h>
#include <atomic>
#include <functional>
#include <limits.h>

#define KVQ_GZ_FIND_THREADS 256
#define KVQ_GZ_RES_THREADS 1024

// one chunk decode of a launch: its place in the file's bytes, its slot (cap symbols), where its result goes
struct kvq_gz_job {
    int64_t start_bit, stop_bit, cap;
    uint16_t *slot;
    KvqChunkRes *res;
    int32_t wlen, pad_;
};

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------

// (1) chunk c: the first bit offset in [lo[c], hi[c]) at which kvq_gz_candidate holds, else -1.  256 offsets a round, a lane each
extern "C" __global__ void __launch_bounds__(KVQ_GZ_FIND_THREADS)
kvq_gz_find(const uint8_t *__restrict__ in, int64_t n, const int64_t *__restrict__ lo, const int64_t *__restrict__ hi,
            int64_t *__restrict__ cand)
{
    __shared__ int first;
    const int c = (int)blockIdx.x, t = (int)threadIdx.x;
    const int64_t a = lo[c], b = hi[c];
    int64_t found = -1;
    for (int64_t base = a; base < b; base += KVQ_GZ_FIND_THREADS) {
        if (t == 0) first = INT_MAX;
        __syncthreads();
        const int64_t bit = base + t;
        if (bit < b && kvq_gz_candidate(in, n, bit)) atomicMin(&first, t);
        __syncthreads();
        const int f = first;
        __syncthreads();                                              // (first is set again by the next round)
        if (f != INT_MAX) { found = base + f; break; }
    }
    if (t == 0) cand[c] = found;
}

// the device's output of kvq_inflate_chunk: a ring of the last 32 Ki symbols in LDS, streamed to the slot; symbols [f, o) are in the ring only
struct KvqRingMarkOut {
    uint16_t *ring, *dst; int64_t f;
    template <class G> __device__ __forceinline__ void flush(const G &g, int64_t o)
    {
        g.sync();
        for (int64_t i = f + g.lane(); i < o; i += G::width) dst[i] = ring[i & (KVQ_INF_WINDOW - 1)];
        f = o;
        g.sync();
    }
    template <class G> __device__ __forceinline__ void room(const G &g, int64_t o, uint32_t len) { if (o + len - f > KVQ_INF_WINDOW) flush(g, o); }
    template <class G> __device__ __forceinline__ void lit(const G &g, int64_t o, uint8_t v)
    {
        room(g, o, 1);
        if (g.lane() == 0) ring[o & (KVQ_INF_WINDOW - 1)] = v;
    }
    template <class G> __device__ __forceinline__ void stored(const G &g, int64_t o, const uint8_t *src, uint32_t len)
    {
        for (uint32_t a = 0; a < len; a += 4096) {
            const uint32_t m = len - a < 4096 ? len - a : 4096;
            room(g, o + a, m);
            for (uint32_t i = (uint32_t)g.lane(); i < m; i += G::width) ring[(o + a + i) & (KVQ_INF_WINDOW - 1)] = src[a + i];
        }
    }
    // (as KvqRingOut::copy: a source symbol's place is written by this copy only at or after the lane that reads it; a source in
    // front of the chunk is the marker of its window byte)
    template <class G> __device__ __forceinline__ void copy(const G &g, int64_t o, uint32_t dist, uint32_t len)
    {
        room(g, o, len);
        g.sync();
        const int64_t s0 = o - (int64_t)dist;
        for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) {
            const int64_t p = s0 + (dist >= len ? i : i % dist);
            ring[(o + i) & (KVQ_INF_WINDOW - 1)] = p < 0 ? (uint16_t)(2 * KVQ_INF_MARKER + p) : ring[p & (KVQ_INF_WINDOW - 1)];
        }
    }
    template <class G> __device__ __forceinline__ void finish(const G &g, int64_t o) { flush(g, o); }
};

// (2) one wave per job: kvq_inflate_chunk into the job's slot, the result to job.res.  64 KiB ring + 6.2 KB tables of LDS: two
// decoders per CU
extern "C" __global__ void __launch_bounds__(KVQ_WAVE)
kvq_gz_decode(const uint8_t *__restrict__ in, int64_t n, int64_t file_end, const kvq_gz_job *__restrict__ jobs, int64_t njobs)
{
    __shared__ KvqInflateWork ws;
    __shared__ uint16_t ring[KVQ_INF_WINDOW];
    const KvqWaveGroup g;
    for (int64_t j = blockIdx.x; j < njobs; j += gridDim.x) {
        const kvq_gz_job e = jobs[j];
        KvqRingMarkOut w; w.ring = ring; w.dst = e.slot; w.f = 0;
        kvq_inflate_chunk(g, &ws, in, n, file_end, e.start_bit, e.stop_bit, e.wlen, w, e.cap, e.res);
        __syncthreads();
    }
}

// (4) one workgroup walks chunks 0..m-1: window k+1 (win + (k+1) * 32 KiB, its last wl[k+1] bytes valid) is the last 32 KiB of
// window k and chunk k's resolved bytes, or of chunk k's bytes since the member that starts in it.  res[0] = the first chunk that
// refers to a byte in front of its valid window (-1 none; the walk ends there), res[1] = the last window's valid bytes.
extern "C" __global__ void __launch_bounds__(KVQ_GZ_RES_THREADS)
kvq_gz_resolve(const kvq_gz_job *__restrict__ jobs, int64_t m, int32_t wl0, uint8_t *__restrict__ win, int64_t *__restrict__ res)
{
    const int t = (int)threadIdx.x;
    int64_t L = wl0, bad = -1;
    for (int64_t k = 0; k < m; k++) {
        const KvqChunkRes r = *jobs[k].res;
        if (r.lowest < -L) { bad = k; break; }
        const uint16_t *slot = jobs[k].slot;
        const uint8_t *W = win + k * KVQ_INF_WINDOW;
        uint8_t *N = win + (k + 1) * KVQ_INF_WINDOW;
        const int64_t nk = r.nsym;
        int64_t nl = r.mstart >= 0 ? nk - r.mstart : L + nk;
        if (nl > KVQ_INF_WINDOW) nl = KVQ_INF_WINDOW;
        for (int64_t j = t; j < nl; j += KVQ_GZ_RES_THREADS) {
            const int64_t q = nk - nl + j;
            uint8_t v;
            if (q >= 0) { const uint16_t s = slot[q]; v = s < 256 ? (uint8_t)s : W[s - KVQ_INF_MARKER]; }
            else v = W[KVQ_INF_WINDOW + q];
            N[KVQ_INF_WINDOW - nl + j] = v;
        }
        __syncthreads();
        L = nl;
    }
    if (t == 0) { res[0] = bad; res[1] = L; }
}

// (5) chunks blockIdx.y, + gridDim.y, ... < m: their symbols, markers replaced from their windows, to text + pre[chunk]; counts the markers
extern "C" __global__ void __launch_bounds__(256)
kvq_gz_replace(const kvq_gz_job *__restrict__ jobs, int64_t m, const int64_t *__restrict__ pre, const uint8_t *__restrict__ win,
               uint8_t *__restrict__ text, unsigned long long *__restrict__ markers)
{
    unsigned long long mk = 0;
    for (int64_t k = blockIdx.y; k < m; k += gridDim.y) {
        const uint16_t *slot = jobs[k].slot;
        const uint8_t *W = win + k * KVQ_INF_WINDOW;
        const int64_t nk = pre[k + 1] - pre[k];
        uint8_t *out = text + pre[k];
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nk; i += (int64_t)gridDim.x * 256) {
            const uint16_t s = slot[i];
            if (s < 256) out[i] = (uint8_t)s;
            else { out[i] = W[s - KVQ_INF_MARKER]; mk++; }
        }
    }
    for (int d = 32; d > 0; d >>= 1) mk += __shfl_down(mk, d);
    if ((threadIdx.x & 63) == 0 && mk) atomicAdd(markers, mk);
}

// ---------------------------------------------------------------------------------------------------------------------
// the chunked algorithm, on top of a backend (the CPU's or the GPU's)
// ---------------------------------------------------------------------------------------------------------------------

struct GzChunk {
    int64_t start = 0, stop = 0, cap = 0;
    int32_t wlen = KVQ_INF_WINDOW;
    KvqChunkRes r{};
};

// one run's outcome: chunks [0, nconf) hold; status (DATA_ERROR: at text offset err_o of the run; NEED_INPUT: the run must
// see more of the file); ended: the text of the file ends in the run; else the next run starts at next_bit
struct GzRunOut {
    int64_t nconf = 0, text = 0, err_o = 0, next_bit = 0, wl = 0;
    int64_t mbyte = -1;                  // the first DEFLATE byte of the last member that started in the run, -1 none
    int64_t end_byte = 0; int32_t end_how = 0;       // ended: as KvqChunkRes
    int32_t status = 0;
    bool ended = false;
};

static kvq_gzip_report g_gz_report;                                   // of the last call (kvq_gzip_last_report)
// test hook (kvq_gzip_slot_canaries): every slot between g_gz_pad canary symbols on each side, and how many were found overwritten
#define KVQ_GZ_CANARY 0xC5C5u
static int32_t g_gz_pad = 0;
static std::atomic<int64_t> g_gz_breaches{0};
static std::vector<int64_t> g_gz_cand, g_gz_start, g_gz_end, g_gz_nsym;     // ... its candidates and held chunks (the test hook)

static int64_t gz_cap0(int64_t start, int64_t stop, int64_t n)
{
    const int64_t hi = stop < n * 8 ? stop : n * 8;
    return (hi > start ? (hi - start) / 8 : 0) * 8 + 65536;           // (FastQ compresses 3.5-6x at levels 1-9)
}

// one run: in[0, n) of a file of file_end bytes; decode from start_bit (a block start, wl0 bytes of window known) to the first
// boundary at or past stop_bit.  The backend has the initial window in place.  Backend:
//   find(lo, hi, cand); decode(chunks, which); resolve(chunks, m, wl0, &bad, &wl); replace(chunks, m, pre) -> text
template <class B>
static int gz_run(B &be, int64_t n, int64_t file_end, int64_t start_bit, int64_t stop_bit, int32_t wl0, int64_t chunk_bytes,
                  kvq_gzip_report &rep, GzRunOut &ro, bool keep_hook)
{
    int rc;
    ro = GzRunOut();
    rep.runs++;
    const int64_t limit = stop_bit < n * 8 ? stop_bit : n * 8;
    std::vector<int64_t> lo, hi, cand;
    for (int64_t b = ((start_bit >> 3) + chunk_bytes) * 8; b < limit; b += chunk_bytes * 8) lo.push_back(b);
    for (size_t i = 0; i < lo.size(); i++) hi.push_back(i + 1 < lo.size() ? lo[i + 1] : limit);
    cand.assign(lo.size(), -1);
    double t0 = now_ms();
    if (!lo.empty() && (rc = be.find(lo, hi, cand))) return rc;
    rep.ms_find += now_ms() - t0;
    std::vector<GzChunk> ch(1);
    ch[0].start = start_bit; ch[0].wlen = wl0;
    for (size_t i = 0; i < lo.size(); i++) {
        rep.candidates_tested += cand[i] >= 0 ? cand[i] - lo[i] + 1 : hi[i] - lo[i];
        if (cand[i] >= 0) { GzChunk c; c.start = cand[i]; ch.push_back(c); }
    }
    if (keep_hook) g_gz_cand = cand;
    const size_t m = ch.size();
    rep.chunks += (int64_t)m;
    for (size_t k = 0; k < m; k++) {
        ch[k].stop = k + 1 < m ? ch[k + 1].start : stop_bit;
        ch[k].cap = gz_cap0(ch[k].start, ch[k].stop, n);
    }
    std::vector<size_t> which(m);
    for (size_t k = 0; k < m; k++) which[k] = k;
    std::vector<char> stale(m);
    size_t held = 0, term = m;                                        // term: the chunk at which the text ends or fails
    for (int pass = 0; ; pass++) {
        t0 = now_ms();
        if ((rc = be.decode(ch, which))) return rc;
        rep.ms_decode += now_ms() - t0;
        if (pass > 0) rep.redecodes += (int64_t)which.size();
        std::fill(stale.begin(), stale.end(), 0);
        for (size_t k : which)
            if (ch[k].r.status == KVQ_INF_SLOT_FULL) { ch[k].cap *= 4; stale[k] = 1; rep.slot_overflows++; }
        for (size_t k = 0; k + 1 < m; k++) {
            const KvqChunkRes &r = ch[k].r;
            if (stale[k] || r.status || r.end != 1) continue;         // (its link is not known yet)
            if (r.end_bit != ch[k + 1].start) { ch[k + 1].start = r.end_bit; stale[k + 1] = 1; rep.refuted++; }
        }
        // the chunks that hold: from chunk 0 while each ended where the next one starts
        held = 0; term = m;
        while (held < m && !stale[held]) {
            const KvqChunkRes &r = ch[held].r;
            held++;
            if (r.status || r.end == 2) { term = held - 1; break; }
        }
        if (held == m || term < m) break;
        which.clear();
        for (size_t k = 0; k < m; k++) if (stale[k]) { which.push_back(k); ch[k].cap = ch[k].cap > gz_cap0(ch[k].start, ch[k].stop, n) ? ch[k].cap : gz_cap0(ch[k].start, ch[k].stop, n); }
    }
    // a chunk that holds ran out of input: the run is repeated with more of it, so nothing of this one may be kept (the
    // windows are not resolved, the run's initial window stays where it is)
    if (term < m && ch[term].r.status == KVQ_INF_NEED_INPUT) { ro.status = KVQ_INF_NEED_INPUT; ro.nconf = (int64_t)term; return KVQ_OK; }
    // the windows, chunk after chunk; an earlier reference in front of a member (or of the file) is the first error
    int64_t bad = -1, wl = 0;
    t0 = now_ms();
    if ((rc = be.resolve(ch, held, wl0, &bad, &wl))) return rc;
    rep.ms_resolve += now_ms() - t0;
    if (bad >= 0) {
        // locate it: decoded again with exactly the window that is there
        GzChunk &c = ch[(size_t)bad];
        c.wlen = (int32_t)be.window_len((size_t)bad);
        const std::vector<size_t> one(1, (size_t)bad);
        if ((rc = be.decode(ch, one))) return rc;
        rep.redecodes++;
        term = (size_t)bad; held = term + 1;
        if (c.r.status == 0) c.r.status = KVQ_INF_DATA_ERROR, c.r.err_o = 0;          // (cannot happen: the same decoder refused it)
    }
    std::vector<int64_t> pre(held + 1, 0);
    for (size_t k = 0; k < held; k++) pre[k + 1] = pre[k] + ch[k].r.nsym;
    if (keep_hook) {
        g_gz_start.clear(); g_gz_end.clear(); g_gz_nsym.clear();
        for (size_t k = 0; k < held; k++) { g_gz_start.push_back(ch[k].start); g_gz_end.push_back(ch[k].r.end == 1 ? ch[k].r.end_bit : -1); g_gz_nsym.push_back(ch[k].r.nsym); }
    }
    if (term < m && ch[term].r.status) {
        ro.status = ch[term].r.status; ro.err_o = pre[term] + ch[term].r.err_o; ro.nconf = (int64_t)term;
        return KVQ_OK;
    }
    t0 = now_ms();
    if ((rc = be.replace(ch, held, pre, &rep.marker_symbols))) return rc;
    rep.ms_replace += now_ms() - t0;
    if ((rc = be.keep_window(held))) return rc;                       // (only now: the run's window for the run behind it)
    ro.nconf = (int64_t)held; ro.text = pre[held]; ro.wl = wl;
    ro.ended = term < m || ch[m - 1].r.end == 2;
    ro.next_bit = ch[m - 1].r.end_bit;
    for (size_t k = 0; k < held; k++) if (ch[k].r.mbyte >= 0) ro.mbyte = ch[k].r.mbyte;
    if (ro.ended) { ro.end_byte = ch[held - 1].r.end_byte; ro.end_how = ch[held - 1].r.end_how; }
    return KVQ_OK;
}

// one run's report into the call's.  repeated: the run ran out of input and is done again with more of it -- it counts once,
// as its last attempt does; this attempt only adds its decodes (as decodes again) and its time
static void gz_report_add(kvq_gzip_report &to, const kvq_gzip_report &r, bool repeated)
{
    if (repeated) { to.input_retries++; to.redecodes += r.chunks + r.redecodes; }
    else {
        to.runs += r.runs; to.chunks += r.chunks; to.candidates_tested += r.candidates_tested; to.refuted += r.refuted;
        to.redecodes += r.redecodes; to.slot_overflows += r.slot_overflows; to.marker_symbols += r.marker_symbols;
        to.input_retries += r.input_retries;
    }
    to.ms_find += r.ms_find; to.ms_decode += r.ms_decode; to.ms_resolve += r.ms_resolve; to.ms_replace += r.ms_replace;
}

// the CPU's backend: whole file in memory, a vector per slot, the windows as vectors
struct GzHostBackend {
    const uint8_t *in; int64_t n, file_end;
    std::vector<std::vector<uint16_t>> padded;                        // per chunk its slot, between g_gz_pad canaries a side
    std::vector<uint16_t *> slot;
    std::vector<uint8_t> win;                                         // window k at win[k * 32 KiB]; window 0 is the run's initial one
    std::vector<int64_t> wl;
    uint8_t *text = nullptr; int64_t text_cap = 0;

    int find(const std::vector<int64_t> &lo, const std::vector<int64_t> &hi, std::vector<int64_t> &cand)
    {
        for (size_t c = 0; c < lo.size(); c++)
            for (int64_t b = lo[c]; b < hi[c]; b++) if (kvq_gz_candidate(in, n, b)) { cand[c] = b; break; }
        return KVQ_OK;
    }
    int decode(std::vector<GzChunk> &ch, const std::vector<size_t> &which)
    {
        if (slot.size() < ch.size()) { slot.resize(ch.size()); padded.resize(ch.size()); }
        KvqInflateWork ws;
        const size_t pad = (size_t)g_gz_pad;
        for (size_t k : which) {
            GzChunk &c = ch[k];
            std::vector<uint16_t> &v = padded[k];
            v.assign((size_t)c.cap + 2 * pad, (uint16_t)KVQ_GZ_CANARY);
            KvqMarkOut w; w.slot = v.data() + pad;
            kvq_inflate_chunk(KvqSerialGroup(), &ws, in, n, file_end, c.start, c.stop, c.wlen, w, c.cap, &c.r);
            for (size_t i = 0; i < pad; i++) g_gz_breaches += (v[i] != KVQ_GZ_CANARY) + (v[pad + (size_t)c.cap + i] != KVQ_GZ_CANARY);
            slot[k] = v.data() + pad;
        }
        return KVQ_OK;
    }
    int64_t window_len(size_t k) const { return wl[k]; }
    int resolve(std::vector<GzChunk> &ch, size_t m, int32_t wl0, int64_t *bad, int64_t *wl_out)
    {
        win.resize((m + 1) * KVQ_INF_WINDOW);
        wl.assign(m + 1, 0); wl[0] = wl0;
        *bad = -1;
        for (size_t k = 0; k < m; k++) {
            const KvqChunkRes &r = ch[k].r;
            if (r.lowest < -wl[k]) { *bad = (int64_t)k; break; }
            const uint8_t *W = win.data() + k * KVQ_INF_WINDOW;
            uint8_t *N = win.data() + (k + 1) * KVQ_INF_WINDOW;
            const int64_t nk = r.nsym;
            int64_t nl = r.mstart >= 0 ? nk - r.mstart : wl[k] + nk;
            if (nl > KVQ_INF_WINDOW) nl = KVQ_INF_WINDOW;
            for (int64_t j = 0; j < nl; j++) {
                const int64_t q = nk - nl + j;
                uint8_t v;
                if (q >= 0) { const uint16_t s = slot[k][q]; v = s < 256 ? (uint8_t)s : W[s - KVQ_INF_MARKER]; }
                else v = W[KVQ_INF_WINDOW + q];
                N[KVQ_INF_WINDOW - nl + j] = v;
            }
            wl[k + 1] = nl;
        }
        *wl_out = *bad >= 0 ? 0 : wl[m];
        return KVQ_OK;
    }
    int keep_window(size_t) { return KVQ_OK; }                        // (one run: no run behind it)
    int replace(std::vector<GzChunk> &, size_t m, const std::vector<int64_t> &pre, int64_t *markers)
    {
        if (pre[m] > text_cap) return KVQ_OK;                         // (the caller only wants the length)
        for (size_t k = 0; k < m; k++) {
            const uint8_t *W = win.data() + k * KVQ_INF_WINDOW;
            for (int64_t i = 0; i < pre[k + 1] - pre[k]; i++) {
                const uint16_t s = slot[k][i];
                if (s < 256) text[pre[k] + i] = (uint8_t)s;
                else { text[pre[k] + i] = W[s - KVQ_INF_MARKER]; (*markers)++; }
            }
        }
        return KVQ_OK;
    }
};

// the GPU's backend: the file's bytes in device memory; the slots of each decode launch in a buffer of their own
struct GzDeviceBackend {
    const uint8_t *d_in; int64_t n, file_end;
    hipStream_t st = 0;
    std::vector<DevBuf> bufs;                                         // slot buffers, one per decode launch
    std::vector<uint16_t *> slot_of;                                  // chunk -> its slot
    DevBuf d_jobs, d_res, d_lohi, d_win, d_out8, d_pre;               // jobs of all chunks, their results, the finder's ranges, the windows,
                                                                      // the chunks' text offsets
    std::vector<kvq_gz_job> jobs; std::vector<KvqChunkRes> hres;
    std::vector<int64_t> wl_host; int64_t wl0 = 0;
    uint8_t *d_text = nullptr; int64_t text_cap = 0;
    const uint8_t *d_win0 = nullptr;                                  // the run's initial window (32 KiB), nullptr: none
    uint8_t *d_win_last = nullptr;                                    // where the last window goes (32 KiB), nullptr: nowhere
    std::function<int(int64_t)> grow;                                 // makes d_text hold text_cap >= need bytes (nullptr: it must fit)

    ~GzDeviceBackend() { for (auto &b : bufs) b.release(); d_jobs.release(); d_res.release(); d_lohi.release(); d_win.release(); d_out8.release(); d_pre.release(); }

    int find(const std::vector<int64_t> &lo, const std::vector<int64_t> &hi, std::vector<int64_t> &cand)
    {
        const size_t c = lo.size();
        int rc;
        if ((rc = d_lohi.ensure(c * 3 * 8))) return rc;
        int64_t *d = d_lohi.as<int64_t>();
        KVQ_HIP(hipMemcpyAsync(d, lo.data(), c * 8, hipMemcpyHostToDevice, st));
        KVQ_HIP(hipMemcpyAsync(d + c, hi.data(), c * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kvq_gz_find, dim3((uint32_t)c), dim3(KVQ_GZ_FIND_THREADS), 0, st, d_in, n, d, d + c, d + 2 * c);
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipMemcpyAsync(cand.data(), d + 2 * c, c * 8, hipMemcpyDeviceToHost, st));
        KVQ_HIP(hipStreamSynchronize(st));
        return KVQ_OK;
    }
    int decode(std::vector<GzChunk> &ch, const std::vector<size_t> &which)
    {
        int rc;
        const size_t m = ch.size();
        if (slot_of.size() < m) slot_of.resize(m, nullptr);
        if ((rc = d_res.ensure(m * sizeof(KvqChunkRes)))) { return rc; }
        if (d_jobs.cap < m * sizeof(kvq_gz_job) && (rc = d_jobs.ensure(m * sizeof(kvq_gz_job)))) return rc;
        const int64_t pad = g_gz_pad;
        int64_t total = 0;
        for (size_t k : which) total += (ch[k].cap + 2 * pad + 63) & ~63ll;
        bufs.emplace_back();
        if ((rc = bufs.back().ensure((size_t)total * 2))) return rc;
        uint16_t *base = bufs.back().as<uint16_t>();
        if (pad) KVQ_HIP(hipMemsetAsync(base, KVQ_GZ_CANARY & 0xFF, (size_t)total * 2, st));
        jobs.resize(m); hres.resize(m);
        std::vector<kvq_gz_job> launch;
        int64_t at = 0;
        for (size_t k : which) {
            slot_of[k] = base + at + pad; at += (ch[k].cap + 2 * pad + 63) & ~63ll;
            kvq_gz_job j; j.start_bit = ch[k].start; j.stop_bit = ch[k].stop; j.cap = ch[k].cap; j.slot = slot_of[k];
            j.res = d_res.as<KvqChunkRes>() + k; j.wlen = ch[k].wlen; j.pad_ = 0;
            launch.push_back(j);
        }
        // (the launch's jobs at the front of d_jobs; resolve and replace write the table of all chunks again)
        KVQ_HIP(hipMemcpyAsync(d_jobs.p, launch.data(), launch.size() * sizeof(kvq_gz_job), hipMemcpyHostToDevice, st));
        const int64_t grid = (int64_t)launch.size() < (1 << 20) ? (int64_t)launch.size() : (1 << 20);
        hipLaunchKernelGGL(kvq_gz_decode, dim3((uint32_t)grid), dim3(KVQ_WAVE), 0, st, d_in, n, file_end, d_jobs.as<kvq_gz_job>(), (int64_t)launch.size());
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipMemcpyAsync(hres.data(), d_res.p, m * sizeof(KvqChunkRes), hipMemcpyDeviceToHost, st));
        KVQ_HIP(hipStreamSynchronize(st));
        for (size_t k : which) ch[k].r = hres[k];
        if (pad) {
            std::vector<uint16_t> h((size_t)total);
            KVQ_HIP(hipMemcpy(h.data(), base, (size_t)total * 2, hipMemcpyDeviceToHost));
            for (size_t k : which) {
                const int64_t o = slot_of[k] - base;
                for (int64_t i = 0; i < pad; i++)
                    g_gz_breaches += (h[(size_t)(o - pad + i)] != KVQ_GZ_CANARY) + (h[(size_t)(o + ch[k].cap + i)] != KVQ_GZ_CANARY);
            }
        }
        return KVQ_OK;
    }
    int64_t window_len(size_t k) const { return wl_host[k]; }
    int table(size_t m)
    {
        jobs.resize(m);
        for (size_t k = 0; k < m; k++) { jobs[k] = kvq_gz_job(); jobs[k].slot = slot_of[k]; jobs[k].res = d_res.as<KvqChunkRes>() + k; }
        KVQ_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), m * sizeof(kvq_gz_job), hipMemcpyHostToDevice, st));
        return KVQ_OK;
    }
    int resolve(std::vector<GzChunk> &ch, size_t m, int32_t w0, int64_t *bad, int64_t *wl_out)
    {
        int rc;
        if ((rc = d_win.ensure((m + 1) * KVQ_INF_WINDOW))) return rc;
        if ((rc = d_out8.ensure(64))) return rc;
        if ((rc = table(m))) return rc;
        if (d_win0 && w0 > 0) KVQ_HIP(hipMemcpyAsync(d_win.p, d_win0, KVQ_INF_WINDOW, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(kvq_gz_resolve, dim3(1), dim3(KVQ_GZ_RES_THREADS), 0, st, d_jobs.as<kvq_gz_job>(), (int64_t)m, w0, d_win.as<uint8_t>(), d_out8.as<int64_t>());
        KVQ_HIP(hipGetLastError());
        int64_t res[2];
        KVQ_HIP(hipMemcpyAsync(res, d_out8.p, 16, hipMemcpyDeviceToHost, st));
        KVQ_HIP(hipStreamSynchronize(st));
        *bad = res[0]; *wl_out = res[0] >= 0 ? 0 : res[1];
        // the valid bytes of each window, as the kernel worked them out (to locate a reference in front of one)
        wl_host.assign(m + 1, 0); wl_host[0] = w0;
        for (size_t k = 0; k < m; k++) {
            int64_t nl = ch[k].r.mstart >= 0 ? ch[k].r.nsym - ch[k].r.mstart : wl_host[k] + ch[k].r.nsym;
            wl_host[k + 1] = nl > KVQ_INF_WINDOW ? KVQ_INF_WINDOW : nl;
        }
        return KVQ_OK;
    }
    // the window behind the last of m resolved chunks to d_win_last (which may be d_win0: it is read by resolve only)
    int keep_window(size_t m)
    {
        if (d_win_last) KVQ_HIP(hipMemcpyAsync(d_win_last, d_win.as<uint8_t>() + m * KVQ_INF_WINDOW, KVQ_INF_WINDOW, hipMemcpyDeviceToDevice, st));
        return KVQ_OK;
    }
    int replace(std::vector<GzChunk> &, size_t m, const std::vector<int64_t> &pre, int64_t *markers)
    {
        int rc;
        if (pre[m] > text_cap && grow && (rc = grow(pre[m]))) return rc;
        if (pre[m] > text_cap || m == 0) return KVQ_OK;
        if ((rc = table(m))) return rc;
        if ((rc = d_pre.ensure((m + 1) * 8 + 8))) return rc;
        KVQ_HIP(hipMemcpyAsync(d_pre.p, pre.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
        KVQ_HIP(hipMemsetAsync(d_pre.as<int64_t>() + m + 1, 0, 8, st));
        int64_t longest = 1;
        for (size_t k = 0; k < m; k++) longest = std::max(longest, pre[k + 1] - pre[k]);
        const uint32_t gx = (uint32_t)std::min<int64_t>((longest + 4095) / 4096, 1024);
        hipLaunchKernelGGL(kvq_gz_replace, dim3(gx, (uint32_t)std::min<size_t>(m, 65535)), dim3(256), 0, st, d_jobs.as<kvq_gz_job>(), (int64_t)m,
                           d_pre.as<int64_t>(), d_win.as<uint8_t>(),
                           d_text, (unsigned long long *)(d_pre.as<int64_t>() + m + 1));
        KVQ_HIP(hipGetLastError());
        int64_t mk = 0;
        KVQ_HIP(hipMemcpyAsync(&mk, d_pre.as<int64_t>() + m + 1, 8, hipMemcpyDeviceToHost, st));
        KVQ_HIP(hipStreamSynchronize(st));
        *markers += mk;
        return KVQ_OK;
    }
};

// the header of the file's first member (it must start at byte 0): the bit offset of its DEFLATE data, or -1 (kvq_last_error:
// the host reader's message); in[0, n) with n == file_end or enough of it
static int64_t gz_first_member(const uint8_t *in, int64_t n, int64_t file_end)
{
    int why = 0;
    const int64_t h = kvq_gz_header(in, n, file_end, 0, 0, &why);
    if (h >= 0) return h * 8;
    static const char *const msg[4] = { "", "magic bytes not found", "expected method==DEFLATED", "unsupported flags (CONTINUATION or ENCRYPTED or RESERVED)" };
    kvq_set_error(KVQ_ERR_IO, "no valid gzip header found at beginning of file : %s", h == -2 ? "magic bytes not found" : msg[why]);
    return -1;
}

// the whole file in one run, as kvq_inflate_gzip_host/_device do
template <class B>
static int64_t gz_whole(B &be, const uint8_t *host_bytes, int64_t nhost, int64_t n, int64_t chunk_bytes, int32_t *status, int64_t *err_fpos,
                        kvq_gzip_report *rep_out)
{
    g_gz_report = kvq_gzip_report();
    g_gz_cand.clear(); g_gz_start.clear(); g_gz_end.clear(); g_gz_nsym.clear();
    if (status) *status = 0;
    if (err_fpos) *err_fpos = -1;
    if (chunk_bytes < 64) { kvq_set_error(KVQ_ERR_RUNTIME, "chunk_bytes must be at least 64"); return -2; }
    const int64_t s0 = gz_first_member(host_bytes, nhost, n);
    if (s0 < 0) return -2;
    GzRunOut ro;
    const int rc = gz_run(be, n, n, s0, INT64_MAX, 0, chunk_bytes, g_gz_report, ro, true);
    if (rep_out) *rep_out = g_gz_report;
    if (rc) return -2;
    if (ro.status) {
        if (status) *status = ro.status;
        if (err_fpos) *err_fpos = ro.err_o;
        kvq_set_error(KVQ_ERR_IO, "error while inflating compressed data : status=%d fpos=%ld", ro.status, (long)ro.err_o);
        return -1;
    }
    return ro.text;
}

extern "C" int64_t kvq_inflate_gzip_host(const uint8_t *file, int64_t n, int64_t chunk_bytes, uint8_t *out, int64_t out_cap,
                                         int32_t *status, int64_t *err_fpos, kvq_gzip_report *rep)
{
    kvq_clear_error();
    if (!file || n < 0 || out_cap < 0 || (out_cap > 0 && !out)) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_inflate_gzip_host: bad arguments"); return -2; }
    GzHostBackend be; be.in = file; be.n = n; be.file_end = n; be.text = out; be.text_cap = out_cap;
    return gz_whole(be, file, n, n, chunk_bytes, status, err_fpos, rep);
}

extern "C" int64_t kvq_inflate_gzip_device(const void *d_file, int64_t n, int64_t chunk_bytes, void *d_out, int64_t out_cap,
                                           int32_t *status, int64_t *err_fpos, kvq_gzip_report *rep)
{
    kvq_clear_error();
    if (!d_file || n < 0 || out_cap < 0 || (out_cap > 0 && !d_out)) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_inflate_gzip_device: bad arguments"); return -2; }
    std::vector<uint8_t> head((size_t)std::min<int64_t>(n, 1 << 20));
    if (!head.empty() && hipMemcpy(head.data(), d_file, head.size(), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError(); kvq_set_error(KVQ_ERR_DEVICE, "device failure"); return -2;
    }
    GzDeviceBackend be; be.d_in = (const uint8_t *)d_file; be.n = n; be.file_end = n; be.d_text = (uint8_t *)d_out; be.text_cap = out_cap;
    return gz_whole(be, head.data(), (int64_t)head.size(), n, chunk_bytes, status, err_fpos, rep);
}

extern "C" void kvq_gzip_last_report(kvq_gzip_report *rep) { if (rep) *rep = g_gz_report; }

extern "C" int64_t kvq_gzip_slot_canaries(int32_t pad_symbols)
{
    g_gz_pad = pad_symbols < 0 ? 0 : (pad_symbols > 65536 ? 65536 : pad_symbols);
    return g_gz_breaches.exchange(0);
}

extern "C" int64_t kvq_gzip_last_chunks(int64_t *cand, int64_t ncand_cap, int64_t *start_bit, int64_t *end_bit, int64_t *nsym, int64_t cap,
                                        int64_t *ncand)
{
    if (ncand) *ncand = (int64_t)g_gz_cand.size();
    for (size_t i = 0; i < g_gz_cand.size() && (int64_t)i < ncand_cap; i++) cand[i] = g_gz_cand[i];
    for (size_t i = 0; i < g_gz_start.size() && (int64_t)i < cap; i++) { start_bit[i] = g_gz_start[i]; end_bit[i] = g_gz_end[i]; nsym[i] = g_gz_nsym[i]; }
    return (int64_t)g_gz_start.size();
}
