// kvarq_amd/csrc/kernels_bam.hip -- BAM records to FastQ text on the GPU, the host twin over the same
// source (kvq_bam.h), and the C entry points of both.
//
// The records of an inflated run form a serial chain (each one's block_size says where the next starts).  The run is cut
// into segments of KVQ_BAM_SEGMENT_KB; one wave per segment finds the first offset from which 4 chained records are
// well-formed (64 candidate offsets a step, a lane each), then walks the chain to the first record at or behind the
// segment's end, noting each record's offset and the offset of its text inside the segment's text.  Segment 0 starts at
// the known first record.  The host checks the chain as section 10 does: a segment holds when it began where the segment
// in front of it ended; the others are walked again from there, all of them in one pass, until every segment holds.  The
// segments' text sizes are summed on the host, and kvq_bam_emit writes the text, a wave per segment, through a window in
// LDS that leaves in aligned 16-byte stores.
#include "kvq_host.h"
#include "kvq_bam.h"

#include <string.h>

#define KVQ_BAM_WIN 4096                 // LDS window of kvq_bam_emit (a multiple of 16)

// one segment's walk (device; host-corrected after the chain check)
struct KvqBamSeg {
    int64_t start;          // the record the walk began at; -1: the segment holds no record start
    int64_t end;            // the first record at or behind the segment's end, or (flags & 1) the record the run ends inside
    int64_t err;            // the record that broke a rule (-1: none); the walk stops there
    int64_t text;           // FastQ bytes of the segment's records
    int64_t base;           // (host) where they go in the run's text: the sizes of the segments in front of it
    int32_t count, written, noqual, flags;      // records walked, records that write text, ... of those without qualities; bit 0: run end
};

static int64_t bam_segment_bytes_default()
{
    const char *e = getenv("KVQ_BAM_SEGMENT_KB");
    const long v = e ? atol(e) : 0;
    return (int64_t)(v >= 1 && v <= 1024 ? v : 64) << 10;
}
static int64_t bam_slot_cap(int64_t seg_bytes) { return seg_bytes / KVQ_BAM_MIN_RECORD + 2; }

// Segment k of p[s0, n) is [s0 + k S, s0 + (k + 1) S) cut at n; redo != nullptr: walk segment redo[2i] from redo[2i + 1]
// (a pass of the chain check).  slot[k cap + i]: offset of record i from the segment's start; toff[k cap + i]: where its text
// starts inside the segment's text.
extern "C" __global__ void __launch_bounds__(KVQ_WAVE)
kvq_bam_find(const uint8_t *__restrict__ p, int64_t n, int64_t limit, int32_t n_ref, int64_t s0, int64_t seg_bytes, int64_t nseg,
             const int64_t *__restrict__ redo, int64_t nredo, uint32_t *__restrict__ slot, uint32_t *__restrict__ toff, int64_t cap,
             KvqBamSeg *__restrict__ seg)
{
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (redo ? i >= nredo : i >= nseg) return;
    const int64_t k = redo ? redo[2 * i] : i;
    const int64_t lo = s0 + k * seg_bytes, hi = lo + seg_bytes < n ? lo + seg_bytes : n;
    int64_t start = -1;
    if (redo) start = redo[2 * i + 1];
    else if (k == 0) start = s0;
    else {
        for (int64_t b = lo; b < hi && start < 0; b += KVQ_WAVE) {
            const int64_t o = b + lane;
            const uint64_t m = __ballot(o < hi && kvq_bam_candidate(p, n, limit, n_ref, o));
            if (m) start = b + __builtin_ctzll(m);
        }
    }
    if (lane != 0) return;
    KvqBamSeg s; s.start = start; s.end = start; s.err = -1; s.text = 0; s.base = 0; s.count = 0; s.written = 0; s.noqual = 0; s.flags = 0;
    if (start >= 0) {
        int64_t o = start, t = 0;
        uint32_t *sl = slot + k * cap, *to = toff + k * cap;
        while (o < hi) {
            KvqBamRec r;
            const int v = kvq_bam_check(p, n, limit, n_ref, o, &r);
            if (v == KVQ_BAM_BAD) { s.err = o; break; }
            if (v == KVQ_BAM_SHORT) { s.flags |= 1; break; }
            if (s.count >= cap) { s.err = o; break; }                // (cannot happen: records are >= 38 bytes apart)
            sl[s.count] = (uint32_t)(o - lo); to[s.count] = (uint32_t)t;
            s.count++;
            const int64_t len = kvq_bam_out_len(r);
            if (len) { s.written++; s.noqual += kvq_bam_noqual(p, r) ? 1 : 0; }
            t += len; o = r.next;
        }
        s.end = s.err >= 0 ? -1 : o; s.text = t;
    }
    seg[k] = s;
}

// the text of every segment's records: segment k's at out[seg[k].base ...], the bytes of out[0, out_cap) only.  The wave
// writes a record's bytes (any lane any byte, kvq_bam_char) into a window of KVQ_BAM_WIN bytes in LDS aligned as out's
// 16-byte words are; a full window leaves in 16-byte stores, the partial words at the segment's two ends byte by byte.
extern "C" __global__ void __launch_bounds__(KVQ_WAVE)
kvq_bam_emit(const uint8_t *__restrict__ p, int64_t s0, int64_t seg_bytes, const KvqBamSeg *__restrict__ seg,
             const uint32_t *__restrict__ slot, const uint32_t *__restrict__ toff, int64_t cap, uint8_t *__restrict__ out, int64_t out_cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[KVQ_BAM_WIN];
    const int lane = (int)threadIdx.x;
    const int64_t k = blockIdx.x;
    const KvqBamSeg s = seg[k];
    if (s.text <= 0 || s.count <= 0) return;
    const int64_t B = s.base, E = s.base + s.text, lo = s0 + k * seg_bytes;
    const int64_t mis = (int64_t)((uintptr_t)out & 15u);
    int64_t A = ((B + mis) & ~(int64_t)15) - mis;                     // out + A is 16-byte aligned
    auto flush = [&](int64_t a, int64_t b) {                          // window bytes of [a, b) that lie in [B, E), to out
        __syncthreads();
        for (int64_t w = a + 16 * lane; w < b; w += 16 * KVQ_WAVE) {
            if (w >= B && w + 16 <= E && w + 16 <= out_cap) *(uint4 *)(out + w) = *(const uint4 *)(win + (w - A));
            else for (int64_t x = w; x < w + 16 && x < b; x++) if (x >= B && x < E && x < out_cap) out[x] = win[x - A];
        }
        __syncthreads();
    };
    for (int32_t i = 0; i < s.count; i++) {
        const KvqBamRec r = kvq_bam_parse(p, lo + slot[k * cap + i]);
        const int64_t L = kvq_bam_out_len(r), at = B + toff[k * cap + i];
        for (int64_t j0 = 0; j0 < L; ) {
            if (at + j0 >= A + KVQ_BAM_WIN) { flush(A, A + KVQ_BAM_WIN); A += KVQ_BAM_WIN; }
            const int64_t m = L - j0 < A + KVQ_BAM_WIN - (at + j0) ? L - j0 : A + KVQ_BAM_WIN - (at + j0);
            for (int64_t j = lane; j < m; j += KVQ_WAVE) win[at + j0 + j - A] = kvq_bam_char(p, r, j0 + j);
            j0 += m;
        }
    }
    flush(A, E < A + KVQ_BAM_WIN ? E : A + KVQ_BAM_WIN);
}

static kvq_bam_report g_bam_report;                                   // of the last call (kvq_bam_last_report)
extern "C" void kvq_bam_last_report(kvq_bam_report *rep) { if (rep) *rep = g_bam_report; }

// the buffers of the device runs, kept from call to call (one findseqs runs at a time)
static struct BamBufs {
    DevBuf d_seg, d_slot, d_toff, d_redo, d_bam[2];
    void *pseg = nullptr, *predo = nullptr; size_t pseg_cap = 0, predo_cap = 0;
} g_bam;

// what bam_run_find learnt of a run p[0, n)
struct BamRunOut {
    int64_t nseg = 0;
    int64_t text = 0;       // FastQ bytes of the run's records
    int64_t end = 0;        // where the chain left the run: n, or the record the run ends inside (the carry)
    int64_t err = -1;       // the first record on the chain that breaks a rule
};

// The records of p[s0, n) (device memory; limit: where the file's stream ends, relative to p): the segments found, the chain
// checked and walked again until it holds, the segments' text offsets uploaded.  Blocking (it reads the segments back); the
// text is written by bam_run_emit.
static int bam_run_find(const uint8_t *d_p, int64_t n, int64_t limit, int32_t n_ref, int64_t s0, int64_t seg_bytes, hipStream_t st,
                        kvq_bam_report &rep, BamRunOut &ro)
{
    int rc;
    ro = BamRunOut();
    ro.end = s0;
    if (s0 >= n) return KVQ_OK;
    const int64_t nseg = (n - s0 + seg_bytes - 1) / seg_bytes, cap = bam_slot_cap(seg_bytes);
    ro.nseg = nseg;
    if ((rc = g_bam.d_seg.ensure((size_t)nseg * sizeof(KvqBamSeg)))) return rc;
    if ((rc = g_bam.d_slot.ensure((size_t)(nseg * cap) * 4))) return rc;
    if ((rc = g_bam.d_toff.ensure((size_t)(nseg * cap) * 4))) return rc;
    if ((rc = pinned_grow(&g_bam.pseg, &g_bam.pseg_cap, (size_t)nseg * sizeof(KvqBamSeg)))) return rc;
    KvqBamSeg *seg = (KvqBamSeg *)g_bam.pseg;
    const double t0 = now_ms();
    hipLaunchKernelGGL(kvq_bam_find, dim3((uint32_t)nseg), dim3(KVQ_WAVE), 0, st, d_p, n, limit, n_ref, s0, seg_bytes, nseg,
                       (const int64_t *)nullptr, (int64_t)0, g_bam.d_slot.as<uint32_t>(), g_bam.d_toff.as<uint32_t>(), cap, g_bam.d_seg.as<KvqBamSeg>());
    KVQ_HIP(hipGetLastError());
    KVQ_HIP(hipMemcpyAsync(seg, g_bam.d_seg.p, (size_t)nseg * sizeof(KvqBamSeg), hipMemcpyDeviceToHost, st));
    KVQ_HIP(hipStreamSynchronize(st));
    rep.segments += nseg;
    std::vector<int64_t> redo;
    for (;;) {
        rep.check_passes++;
        // the chain in order: where the segment must begin (pos), or that it must hold no record start
        redo.clear();
        int64_t pos = s0; bool open = true;
        for (int64_t k = 0; k < nseg; k++) {
            const int64_t hi = std::min(s0 + (k + 1) * seg_bytes, n);
            if (!open || pos >= hi) {
                if (seg[k].start != -1 || seg[k].count) { seg[k] = KvqBamSeg(); seg[k].start = -1; seg[k].end = pos; seg[k].err = -1; }
                continue;
            }
            if (seg[k].start != pos) { redo.push_back(k); redo.push_back(pos); }
            if (seg[k].err >= 0 || (seg[k].flags & 1)) { open = false; pos = seg[k].err >= 0 ? -1 : seg[k].end; }
            else pos = seg[k].end;
        }
        if (redo.empty()) break;
        rep.refuted += (int64_t)redo.size() / 2;
        const int64_t nr = (int64_t)redo.size() / 2;
        if ((rc = g_bam.d_redo.ensure(redo.size() * 8))) return rc;
        if ((rc = pinned_grow(&g_bam.predo, &g_bam.predo_cap, redo.size() * 8))) return rc;
        memcpy(g_bam.predo, redo.data(), redo.size() * 8);
        KVQ_HIP(hipMemcpyAsync(g_bam.d_seg.p, seg, (size_t)nseg * sizeof(KvqBamSeg), hipMemcpyHostToDevice, st));
        KVQ_HIP(hipMemcpyAsync(g_bam.d_redo.p, g_bam.predo, redo.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kvq_bam_find, dim3((uint32_t)nr), dim3(KVQ_WAVE), 0, st, d_p, n, limit, n_ref, s0, seg_bytes, nseg,
                           (const int64_t *)g_bam.d_redo.p, nr, g_bam.d_slot.as<uint32_t>(), g_bam.d_toff.as<uint32_t>(), cap, g_bam.d_seg.as<KvqBamSeg>());
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipMemcpyAsync(seg, g_bam.d_seg.p, (size_t)nseg * sizeof(KvqBamSeg), hipMemcpyDeviceToHost, st));
        KVQ_HIP(hipStreamSynchronize(st));
    }
    // the chain holds: its first broken record, its end, the text offsets of the segments
    int64_t t = 0;
    ro.end = n;
    for (int64_t k = 0; k < nseg; k++) {
        KvqBamSeg &s = seg[k];
        if (s.start < 0) continue;
        if (s.err >= 0) { ro.err = s.err; ro.end = s.err; break; }
        s.base = t; t += s.text;
        rep.records_seen += s.count; rep.records_written += s.written; rep.records_skipped += s.count - s.written; rep.records_noqual += s.noqual;
        if (s.flags & 1) { ro.end = s.end; break; }
    }
    ro.text = t;
    if (ro.err < 0) KVQ_HIP(hipMemcpyAsync(g_bam.d_seg.p, seg, (size_t)nseg * sizeof(KvqBamSeg), hipMemcpyHostToDevice, st));
    rep.ms_find += now_ms() - t0;
    return KVQ_OK;
}

// the text of the run bam_run_find checked, to out[out_off, out_off + ro.text) (out_cap: the bytes of out); enqueued on st
static int bam_run_emit(const uint8_t *d_p, int64_t s0, int64_t seg_bytes, const BamRunOut &ro, uint8_t *d_out, int64_t out_off, int64_t out_cap,
                        hipStream_t st)
{
    if (ro.nseg <= 0 || ro.text <= 0) return KVQ_OK;
    if (out_off < 0 || out_off + ro.text > out_cap) { kvq_set_error(KVQ_ERR_RUNTIME, "BAM text does not fit its buffer"); return KVQ_ERR_RUNTIME; }
    hipLaunchKernelGGL(kvq_bam_emit, dim3((uint32_t)ro.nseg), dim3(KVQ_WAVE), 0, st, d_p, s0, seg_bytes, g_bam.d_seg.as<KvqBamSeg>(),
                       g_bam.d_slot.as<uint32_t>(), g_bam.d_toff.as<uint32_t>(), bam_slot_cap(seg_bytes), d_out + out_off, out_cap - out_off);
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

// ---- C entry points --------------------------------------------------------------------------------------------------

extern "C" int64_t kvq_bam_header_host(const uint8_t *inflated, int64_t n, int32_t *n_ref)
{
    if (!inflated || n < 0) return -1;
    int32_t nr = 0;
    const int64_t o = kvq_bam_header(inflated, n, &nr);
    if (o >= 0 && n_ref) *n_ref = nr;
    return o;
}

// One run as the route takes a file: p[0, n) a prefix of a stream that ends at limit.  The host twin walks the chain itself;
// the device run is bam_run_find and bam_run_emit as BamProducer calls them.  kvq_bam_to_fastq_* are these with limit = n.
extern "C" int64_t kvq_bam_run_host(const uint8_t *p, int64_t n, int64_t limit, int32_t n_ref, int64_t first_record, uint8_t *out, int64_t cap,
                                    int64_t *end)
{
    kvq_clear_error();
    if (!p || n < 0 || limit < n || first_record < 0 || first_record > n) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_bam_run_host: bad arguments"); return -2; }
    kvq_bam_report rep = kvq_bam_report();
    int64_t o = first_record, t = 0;
    while (o < n) {
        KvqBamRec r;
        const int v = kvq_bam_check(p, n, limit, n_ref, o, &r);
        if (v == KVQ_BAM_BAD) {
            if (end) *end = o;
            kvq_set_error(KVQ_ERR_IO, "malformed BAM record : offset=%ld", (long)o);
            return -1;
        }
        if (v == KVQ_BAM_SHORT) break;                                // the record the prefix ends inside
        const int64_t len = kvq_bam_out_len(r);
        rep.records_seen++;
        if (len) { rep.records_written++; rep.records_noqual += kvq_bam_noqual(p, r) ? 1 : 0; } else rep.records_skipped++;
        if (out && t + len <= cap) for (int64_t j = 0; j < len; j++) out[t + j] = kvq_bam_char(p, r, j);
        t += len; o = r.next;
    }
    if (end) *end = o;
    rep.bam_bytes = n; rep.text_bytes = t;
    g_bam_report = rep;
    return t;
}

extern "C" int64_t kvq_bam_to_fastq_host(const uint8_t *inflated, int64_t n, int32_t n_ref, int64_t first_record, uint8_t *out, int64_t cap,
                                         int64_t *consumed)
{
    if (!inflated || n < 0 || first_record < 0 || first_record > n) { kvq_clear_error(); kvq_set_error(KVQ_ERR_RUNTIME, "kvq_bam_to_fastq_host: bad arguments"); return -2; }
    return kvq_bam_run_host(inflated, n, n, n_ref, first_record, out, cap, consumed);
}

extern "C" int64_t kvq_bam_run_device(const void *d_p, int64_t n, int64_t limit, int32_t n_ref, int64_t first_record, void *d_out, int64_t out_off,
                                      int64_t cap, int64_t segment_bytes, int64_t *end, kvq_bam_report *rep_out)
{
    kvq_clear_error();
    if (!d_p || n < 0 || limit < n || first_record < 0 || first_record > n || out_off < 0 || cap < 0 || segment_bytes < 0 || segment_bytes > (64 << 20)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_bam_run_device: bad arguments"); return -2;
    }
    const int64_t sb = segment_bytes > 0 ? segment_bytes : bam_segment_bytes_default();
    kvq_bam_report rep = kvq_bam_report();
    BamRunOut ro;
    int rc = bam_run_find((const uint8_t *)d_p, n, limit, n_ref, first_record, sb, 0, rep, ro);
    if (rc) return -2;
    rep.runs = 1;
    if (end) *end = ro.end;
    if (ro.err >= 0) {
        g_bam_report = rep; if (rep_out) *rep_out = rep;
        kvq_set_error(KVQ_ERR_IO, "malformed BAM record : offset=%ld", (long)ro.err);
        return -1;
    }
    if (d_out && out_off + ro.text <= cap) {
        const double t0 = now_ms();
        if (bam_run_emit((const uint8_t *)d_p, first_record, sb, ro, (uint8_t *)d_out, out_off, cap, 0)) return -2;
        if (hipStreamSynchronize(0) != hipSuccess) { (void)hipGetLastError(); kvq_set_error(KVQ_ERR_DEVICE, "device failure in kvq_bam_emit"); return -2; }
        rep.ms_emit += now_ms() - t0;
    }
    rep.bam_bytes = n; rep.text_bytes = ro.text;
    g_bam_report = rep; if (rep_out) *rep_out = rep;
    return ro.text;
}

extern "C" int64_t kvq_bam_to_fastq_device(const void *d_in, int64_t n, int32_t n_ref, int64_t first_record, void *d_out, int64_t cap,
                                           int64_t segment_bytes, kvq_bam_report *rep_out)
{
    if (!d_in || n < 0 || first_record < 0 || first_record > n || cap < 0 || segment_bytes < 0 || segment_bytes > (64 << 20)) {
        kvq_clear_error(); kvq_set_error(KVQ_ERR_RUNTIME, "kvq_bam_to_fastq_device: bad arguments"); return -2;
    }
    return kvq_bam_run_device(d_in, n, n, n_ref, first_record, d_out, 0, cap, segment_bytes, nullptr, rep_out);
}
