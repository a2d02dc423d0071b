// kvarq_amd/csrc/kvq_routes.hip -- the device routes of engine.findseqs (kvq_findseqs_ex with KVQ_FIND_DEVICE_INFLATE or
// KVQ_FIND_DEVICE_GZIP, and BAM files; DESIGN sections 9, 10 and 12): one walk over a list of input files whose FastQ text
// comes to lie in device memory -- inflated from BGZF blocks, from any other gzip, or decoded from BAM records -- and is
// cut and handed to the scan where it lies.
#include "kvq_host.h"

#include <atomic>
#include <memory>
#include <string.h>
#include <zlib.h>
#include <thread>

// ---------------------------------------------------------------------------
// input files
// ---------------------------------------------------------------------------

// bytes [at, at + n) of a file into dst, by up to `nthreads` (at most `max_threads`) preads at once
static bool pread_run(int fdn, uint8_t *dst, int64_t n, int64_t at, int nthreads, int max_threads)
{
    int nt = nthreads < 1 ? 1 : (nthreads > max_threads ? max_threads : nthreads);
    if (n < (4 << 20)) nt = 1;
    std::atomic<int> bad{0};
    auto slice = [&](int t) {
        int64_t a = n * t / nt, b = n * (t + 1) / nt;
        while (a < b) {
            const ssize_t got = pread(fdn, dst + a, (size_t)(b - a), (off_t)(at + a));
            if (got <= 0) { bad = 1; return; }
            a += got;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; t++) th.emplace_back(slice, t);
    slice(0);
    for (auto &x : th) x.join();
    return !bad.load();
}

// bytes [at, at + n) of a file into the pinned buffer *pin, grown to hold them
static int pread_pinned(int fdn, void **pin, size_t *pin_cap, int64_t n, int64_t at)
{
    int rc = pinned_grow(pin, pin_cap, (size_t)std::max<int64_t>(n, 1));
    if (rc) return rc;
    kvq_config cfg; kvq_config_get(&cfg);
    if (n > 0 && !pread_run(fdn, (uint8_t *)*pin, n, at, cfg.nthreads, 16)) {
        kvq_set_error(KVQ_ERR_IO, "could not read enough bytes from .fastq.gz : I/O error"); return KVQ_ERR_IO;
    }
    return KVQ_OK;
}

// 1 when the file starts with a BGZF block whose inflated bytes begin with "BAM\1" (inflated only as far as that), 0 when not,
// -1 when the file cannot be opened
static int bam_peek(const char *name)
{
    FILE *fd = fopen(name, "rb");
    if (!fd) return -1;
    fseek(fd, 0, SEEK_END); const int64_t size = ftell(fd);
    const PreadAt read{ fileno(fd) };
    kvq_bgzf_entry_ b;
    int is = 0;
    if (kvq_bgzf_peek(read, size, 0, &b) && b.isize >= 4) {
        uint8_t in[4096], out[4];
        const int64_t k = std::min<int64_t>(b.size - b.hdr - 8, sizeof(in));
        z_stream z; memset(&z, 0, sizeof(z));
        if (read(in, k, b.hdr) == k && inflateInit2(&z, -MAX_WBITS) == Z_OK) {
            z.next_in = in; z.avail_in = (uInt)k; z.next_out = out; z.avail_out = 4;
            (void)inflate(&z, Z_SYNC_FLUSH);
            is = z.avail_out == 0 && out[0] == 'B' && out[1] == 'A' && out[2] == 'M' && out[3] == 1;
            inflateEnd(&z);
        }
    }
    fclose(fd);
    return is;
}

// an input file of the device routes: BGZF to its end (its blocks, walked with the host reader's acceptance rules) or not;
// of a BAM file also the inflated bytes of all blocks, the offset of the first record among them and the reference count
struct InputFile {
    std::string name; int64_t size = 0;
    bool bgzf = false; std::vector<kvq_bgzf_entry_> blocks;
    bool bam = false; int64_t isize = 0, first = 0; int32_t n_ref = 0;
};

// opens, sizes and walks a file.  bam: it must be BGZF to its end (else "truncated BAM file") and its header, inflated block
// after block on the host until it is whole, well-formed (else "malformed BAM header")
static int input_open(const char *name, bool bam, InputFile &f)
{
    f = InputFile(); f.name = name; f.bam = bam;
    FILE *fd = fopen(name, "rb");
    if (!fd) { kvq_set_error(KVQ_ERR_IO, "cannot open file"); return KVQ_ERR_IO; }
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{ fd };
    fseek(fd, 0, SEEK_END); f.size = ftell(fd);
    const PreadAt read{ fileno(fd) };
    f.bgzf = kvq_bgzf_walk(read, f.size, f.blocks);
    if (!bam) return KVQ_OK;
    if (!f.bgzf) { kvq_set_error(KVQ_ERR_IO, "truncated BAM file"); return KVQ_ERR_IO; }
    for (auto &b : f.blocks) f.isize += b.isize;
    std::vector<uint8_t> head, comp;
    int64_t first = -2;
    for (size_t k = 0; k < f.blocks.size() && first == -2; k++) {
        const kvq_bgzf_entry_ &b = f.blocks[k];
        comp.resize(b.size);
        if (read(comp.data(), b.size, b.off) != (int64_t)b.size) { kvq_set_error(KVQ_ERR_IO, "truncated BAM file"); return KVQ_ERR_IO; }
        const size_t at = head.size();
        head.resize(at + b.isize);
        const int st = kvq_inflate_raw_host(comp.data() + b.hdr, b.size - b.hdr - 8, head.data() + at, b.isize);
        if (st) { kvq_set_error(KVQ_ERR_IO, "error while inflating compressed data : status=%d fpos=%ld", st, (long)at); return KVQ_ERR_IO; }
        first = kvq_bam_header(head.data(), (int64_t)head.size(), &f.n_ref);
    }
    if (first < 0) { kvq_set_error(KVQ_ERR_IO, "malformed BAM header"); return KVQ_ERR_IO; }
    f.first = first;
    return KVQ_OK;
}

// ---------------------------------------------------------------------------
// buffers and settings of the routes
// ---------------------------------------------------------------------------

// kept from call to call (one findseqs runs at a time): per slot the compressed run of BGZF blocks and its block table in
// pinned and in device memory, the statuses; the two text buffers; the cut results
static struct DevRoute {
    void *pin[2] = { nullptr, nullptr }, *ptab[2] = { nullptr, nullptr }, *pstat[2] = { nullptr, nullptr }, *pcut = nullptr;
    size_t pin_cap[2] = { 0, 0 }, ptab_cap[2] = { 0, 0 }, pstat_cap[2] = { 0, 0 }, pcut_cap = 0;
    DevBuf d_comp[2], d_tab[2], d_stat[2], d_text[2], d_cut;
} g_dev;

// ... the compressed run of a plain gzip file and the window carried from run to run
static struct GzRoute { DevBuf d_comp, d_win; void *pin = nullptr; size_t pin_cap = 0; } g_gz;

// inflated bytes per device batch: 256 MiB, about 4 100 blocks of bgzip's 65 280 bytes (KVQ_INFLATE_BATCH_MB=<2..1024>)
static int64_t device_batch_bytes()
{
    const char *e = getenv("KVQ_INFLATE_BATCH_MB");
    const long v = e ? atol(e) : 0;
    return (int64_t)(v >= 2 && v <= 1024 ? v : 256) << 20;
}

// compressed bytes per run of a plain gzip file (a quarter of the text a batch holds) and per chunk (KVQ_GZIP_CHUNK_KB)
static int64_t gz_chunk_bytes()
{
    const char *e = getenv("KVQ_GZIP_CHUNK_KB");
    const long v = e ? atol(e) : 0;
    return (int64_t)(v >= 1 && v <= 65536 ? v : 128) << 10;
}

// ---------------------------------------------------------------------------
// runs of whole BGZF blocks
// ---------------------------------------------------------------------------

// One run of whole BGZF blocks [b0, b1) of a file, its compressed bytes [bl[b0].off, end of bl[b1 - 1]) in g_dev.pin[slot]:
// the block table (the inflated bytes go behind the `carry` bytes kept from the run before, copied from carry_at to the front
// of out unless they lie there), the copies and kvq_inflate_bgzf enqueued on st, the statuses on their way to g_dev.pstat[slot].
// *have: the bytes there will be.  bgzf_run_check reads the statuses once st has been synchronised.
static int bgzf_run_enqueue(const std::vector<kvq_bgzf_entry_> &bl, size_t b0, size_t b1, int slot, uint8_t *out, int64_t out_cap,
                            int64_t carry, const uint8_t *carry_at, hipStream_t st, int64_t *have)
{
    int rc;
    const int64_t nb = (int64_t)(b1 - b0), c0 = bl[b0].off, c1 = bl[b1 - 1].off + bl[b1 - 1].size;
    if ((rc = pinned_grow(&g_dev.ptab[slot], &g_dev.ptab_cap[slot], (size_t)nb * sizeof(kvq_bgzf_block)))) return rc;
    if ((rc = pinned_grow(&g_dev.pstat[slot], &g_dev.pstat_cap[slot], (size_t)nb * 4))) return rc;
    kvq_bgzf_block *tab = (kvq_bgzf_block *)g_dev.ptab[slot];
    int64_t o = carry;
    for (int64_t i = 0; i < nb; i++) {
        const kvq_bgzf_entry_ &b = bl[b0 + i];
        tab[i].in_off = b.off - c0 + b.hdr; tab[i].in_len = b.size - b.hdr - 8; tab[i].isize = b.isize; tab[i].out_off = o;
        o += b.isize;
    }
    *have = o;
    if ((rc = g_dev.d_comp[slot].ensure((size_t)(c1 - c0)))) return rc;
    if ((rc = g_dev.d_tab[slot].ensure((size_t)nb * sizeof(kvq_bgzf_block)))) return rc;
    if ((rc = g_dev.d_stat[slot].ensure((size_t)nb * 4))) return rc;
    KVQ_HIP(hipMemcpyAsync(g_dev.d_comp[slot].p, g_dev.pin[slot], (size_t)(c1 - c0), hipMemcpyHostToDevice, st));
    KVQ_HIP(hipMemcpyAsync(g_dev.d_tab[slot].p, tab, (size_t)nb * sizeof(kvq_bgzf_block), hipMemcpyHostToDevice, st));
    if (carry && carry_at != out) KVQ_HIP(hipMemcpyAsync(out, carry_at, (size_t)carry, hipMemcpyDeviceToDevice, st));
    if ((rc = kvq_inflate_bgzf_launch(g_dev.d_comp[slot].as<uint8_t>(), c1 - c0, g_dev.d_tab[slot].as<kvq_bgzf_block>(), nb,
                                      out, out_cap, g_dev.d_stat[slot].as<int32_t>(), st))) return rc;
    KVQ_HIP(hipMemcpyAsync(g_dev.pstat[slot], g_dev.d_stat[slot].p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
    return KVQ_OK;
}

// the statuses of the run bgzf_run_enqueue enqueued in `slot` (nb blocks; base: the stream offset of out's front): the first
// block that did not inflate, as the route's IOError naming that block's first byte
static int bgzf_run_check(int slot, int64_t nb, int64_t base)
{
    const int32_t *stat = (const int32_t *)g_dev.pstat[slot];
    const kvq_bgzf_block *tab = (const kvq_bgzf_block *)g_dev.ptab[slot];
    for (int64_t i = 0; i < nb; i++)
        if (stat[i] != 0) {
            kvq_set_error(KVQ_ERR_IO, "error while inflating compressed data : status=%d fpos=%ld", stat[i], (long)(base + tab[i].out_off));
            return KVQ_ERR_IO;
        }
    return KVQ_OK;
}

// The runs of the BGZF files of a list, in order: as many whole blocks as inflate to a batch (one at least), read into the
// pinned slots g_dev.pin[0] and [1] in turn -- the run behind the one the GPU works on while it does, be that the first run of
// the next file.
struct BlockRuns {
    struct Run { size_t f = (size_t)-1, b0 = 0, b1 = 0; int64_t c1 = 0, isz = 0; int slot = 0; bool eof = false; };
    const std::vector<InputFile> &files; const int64_t batch_cap;
    Run ahead;                                     // the run read ahead (f == -1: none)
    FILE *fd = nullptr; size_t fd_of = (size_t)-1;

    BlockRuns(const std::vector<InputFile> &files_, int64_t batch_cap_) : files(files_), batch_cap(batch_cap_) {}
    ~BlockRuns() { if (fd) fclose(fd); }

    // the run of file f that starts at block b0, in pinned memory
    int read(size_t f, size_t b0, int slot, Run &r)
    {
        const auto &bl = files[f].blocks;
        r = Run(); r.f = f; r.b0 = b0; r.b1 = b0; r.slot = slot;
        while (r.b1 < bl.size() && (r.b1 == b0 || r.isz + bl[r.b1].isize <= batch_cap)) r.isz += bl[r.b1++].isize;
        r.c1 = bl[r.b1 - 1].off + bl[r.b1 - 1].size; r.eof = r.b1 == bl.size();
        if (fd_of != f) {
            if (fd) fclose(fd);
            fd = fopen(files[f].name.c_str(), "rb"); fd_of = f;
            if (!fd) { kvq_set_error(KVQ_ERR_IO, "cannot open file"); return KVQ_ERR_IO; }
        }
        return pread_pinned(fileno(fd), &g_dev.pin[slot], &g_dev.pin_cap[slot], r.c1 - bl[b0].off, bl[b0].off);
    }
    // ... read ahead, or now
    int take(size_t f, size_t b0, Run &r)
    {
        if (ahead.f == f && ahead.b0 == b0) { r = ahead; ahead = Run(); return KVQ_OK; }
        return read(f, b0, 0, r);
    }
    // the run behind r into the other slot, while the GPU works on r
    int read_ahead(const Run &r)
    {
        if (!r.eof) return read(r.f, r.b1, r.slot ^ 1, ahead);
        if (r.f + 1 < files.size() && files[r.f + 1].bgzf) return read(r.f + 1, 0, r.slot ^ 1, ahead);
        return KVQ_OK;
    }
};

// ---------------------------------------------------------------------------
// the shared stage: from text in a device buffer to batches of whole chunks
// ---------------------------------------------------------------------------

// The walk of stream_batches over text that lies in device memory.  Per run a producer appends text behind the unfinished
// chunk the run before left (copied device to device to the front of the text buffer, so that the batch starts 16-byte
// aligned); kvq_cut_chunks cuts the chunks, their offsets come back to the host, and the text is handed to the scan where it
// lies.  The two text buffers alternate after every batch handed to the scan (and only then: a run that hands over nothing --
// an empty file -- must not overwrite the text of the batch in flight, which may still be scanned again from where it lies);
// the scan's stream runs a batch's kernels before the producer of the batch after the next one writes.  file_pos and parsed
// count text bytes; the estimate of the total is the host reader's, worked out from where its reader would have read to.
template <class Sink>
struct TextStage {
    Sink &sink; hipStream_t st; const int64_t size_all;
    int64_t fpos = 0, ftell0 = 0, total;
    int64_t carry = 0, carry_src = 0, fill = 0, text_fpos = 0;       // the unfinished chunk of the file, where it lies (text buffer cb)
    int tb = 0, cb = 0;                                               // the text buffer of this run
    int64_t have = 0;                                                 // text bytes of this run, the unfinished chunk included

    TextStage(Sink &sink_, hipStream_t st_, int64_t size_all_) : sink(sink_), st(st_), size_all(size_all_), total(size_all_) {}

    int init()
    {
        int rc;
        if ((rc = g_dev.d_cut.ensure((8 + KVQ_CUT_CAP) * 8))) return rc;
        return pinned_grow(&g_dev.pcut, &g_dev.pcut_cap, (8 + KVQ_CUT_CAP) * 8);
    }
    uint8_t *text() const { return g_dev.d_text[tb].as<uint8_t>(); }
    int64_t cap() const { return (int64_t)g_dev.d_text[tb].cap; }

    // the text buffer of this run grows to `bytes`; an unfinished chunk that lies in it moves along
    int grow(int64_t bytes)
    {
        DevBuf nb;
        int rc = nb.ensure((size_t)bytes);
        if (rc) return rc;
        if (cb == tb && carry) KVQ_HIP(hipMemcpyAsync(nb.p, text() + carry_src, (size_t)carry, hipMemcpyDeviceToDevice, st));
        KVQ_HIP(hipStreamSynchronize(st));
        g_dev.d_text[tb].release(); g_dev.d_text[tb] = nb;
        if (cb == tb) carry_src = 0;
        return KVQ_OK;
    }
    // the unfinished chunk to the front of this run's text buffer, unless it lies there
    int front()
    {
        const uint8_t *carry_at = g_dev.d_text[cb].as<uint8_t>() + carry_src;
        if (carry && carry_at != text()) KVQ_HIP(hipMemcpyAsync(text(), carry_at, (size_t)carry, hipMemcpyDeviceToDevice, st));
        cb = tb; carry_src = 0;
        return KVQ_OK;
    }

    // the first cuts of the run's text, `more` bytes behind the unfinished chunk: enqueued behind whatever writes them
    int enqueue(int64_t more)
    {
        int rc;
        have = carry + more;
        int64_t *d_cut = g_dev.d_cut.as<int64_t>();
        if ((rc = kvq_cut_chunks_launch(text(), have, 0, fill, d_cut + 8, KVQ_CUT_CAP, d_cut, st))) return rc;
        KVQ_HIP(hipMemcpyAsync(g_dev.pcut, d_cut, (8 + KVQ_CUT_CAP) * 8, hipMemcpyDeviceToHost, st));
        return KVQ_OK;
    }
    // ... and, the stream synchronised, the rest of them, the batch handed over, the chunk left unfinished.  consumed: the
    // compressed bytes of the file the host reader would have read by now; eof: the file's text ends with this run
    int collect(int64_t consumed, bool eof)
    {
        int rc;
        int64_t *cut = (int64_t *)g_dev.pcut, *d_cut = g_dev.d_cut.as<int64_t>();
        std::vector<int64_t> off;
        for (;;) {
            if (cut[3]) {
                kvq_set_error(KVQ_ERR_RUNTIME, "could find beginning of record; read %ld bytes up to %ld", (long)cut[4], (long)(text_fpos + cut[5]));
                return KVQ_ERR_RUNTIME;
            }
            off.insert(off.end(), cut + 8, cut + 8 + cut[0]);
            if (cut[0] < KVQ_CUT_CAP) break;
            if ((rc = kvq_cut_chunks_launch(text(), have, cut[1], cut[2], d_cut + 8, KVQ_CUT_CAP, d_cut, st))) return rc;
            KVQ_HIP(hipMemcpyAsync(cut, d_cut, (8 + KVQ_CUT_CAP) * 8, hipMemcpyDeviceToHost, st));
            KVQ_HIP(hipStreamSynchronize(st));
        }
        int64_t cs = cut[1];
        fill = cut[2];
        fpos += have - carry;
        if (ftell0 + consumed > 0)
            total = (int64_t)(size_t)((float)size_all * fpos / (ftell0 + consumed));          // the host reader's estimate (883-884)
        if (eof) { if (have > cs) off.push_back(cs); cs = have; }
        const bool handed = !off.empty();
        if (handed) {
            off.push_back(cs);
            if ((rc = sink.batch(text(), cs, off.data(), (int64_t)off.size() - 1, text_fpos, fpos, total))) return rc;
        }
        if (eof) { ftell0 += consumed; carry = 0; carry_src = 0; fill = 0; text_fpos = fpos; }          // the next file starts afresh
        else { carry = have - cs; carry_src = cs; cb = tb; fill -= cs; text_fpos += cs; }
        if (handed) tb ^= 1;
        return KVQ_OK;
    }
};

// ---------------------------------------------------------------------------
// the producers: the next run of a file's text behind the unfinished chunk
// ---------------------------------------------------------------------------

struct Produced { int64_t text = 0, consumed = 0; bool eof = false; };      // text bytes appended, compressed bytes of the file behind them, the file ended

// (S: the stage.)  open: once, before the file's first run; enqueue: the run's text is on the stream at least, and *out says
// what it will be; ahead: host work while the GPU does its part and the first cuts; check: the stream has been synchronised
template <class S>
struct Producer {
    virtual ~Producer() {}
    virtual int open() { return KVQ_OK; }
    virtual int enqueue(S &sg, Produced *out) = 0;
    virtual int ahead() { return KVQ_OK; }
    virtual int check(const S &) { return KVQ_OK; }
};

// a BGZF file: a run of whole blocks through kvq_inflate_bgzf, straight behind the unfinished chunk.  (Never more than a
// batch of text and less than a chunk in front of it: the text buffers hold that from the start.)
template <class S>
struct BgzfProducer : Producer<S> {
    BlockRuns &runs; const size_t f; size_t b0 = 0; BlockRuns::Run run;
    BgzfProducer(BlockRuns &runs_, size_t f_) : runs(runs_), f(f_) {}
    int enqueue(S &sg, Produced *out) override
    {
        int rc;
        if ((rc = runs.take(f, b0, run)) || (rc = sg.front())) return rc;
        int64_t have = 0;
        if ((rc = bgzf_run_enqueue(runs.files[f].blocks, run.b0, run.b1, run.slot, sg.text(), sg.cap(), sg.carry, sg.text(), sg.st, &have))) return rc;
        b0 = run.b1;
        out->text = run.isz; out->eof = run.eof;
        out->consumed = run.eof ? runs.files[f].size : run.c1;               // (at the end also the trailer behind the last block)
        return KVQ_OK;
    }
    int ahead() override { return runs.read_ahead(run); }
    int check(const S &sg) override { return bgzf_run_check(run.slot, (int64_t)(run.b1 - run.b0), sg.text_fpos); }
};

// any other gzip file: a run of compressed bytes through the chunked algorithm of kernels_gzip.hip, each run starting at the
// block boundary (and with the window, kept on the device) where the run before it ended; the last chunk of a run reads on
// into a margin of the bytes behind it.  Blocking.
template <class S>
struct GzipProducer : Producer<S> {
    const InputFile &F; kvq_scan *s; const int64_t chunk_bytes, run_bytes;
    FILE *fd = nullptr;
    int64_t gz_bit = 0, gz_h = 0; int32_t gz_wl = 0;      // where the next run starts, where the serial reader's reads of the member started, the window's valid bytes
    GzipProducer(const InputFile &F_, kvq_scan *s_, int64_t batch_cap) : F(F_), s(s_), chunk_bytes(gz_chunk_bytes()), run_bytes(std::max<int64_t>(batch_cap / 4, 64 << 10)) {}
    ~GzipProducer() { if (fd) fclose(fd); }
    int read(int64_t at, int64_t n) { return pread_pinned(fileno(fd), &g_gz.pin, &g_gz.pin_cap, n, at); }
    int open() override
    {
        int rc;
        if (!(fd = fopen(F.name.c_str(), "rb"))) { kvq_set_error(KVQ_ERR_IO, "cannot open file"); return KVQ_ERR_IO; }
        const int64_t k = std::min<int64_t>(F.size, 1 << 20);
        if ((rc = read(0, k))) return rc;
        gz_bit = gz_first_member((const uint8_t *)g_gz.pin, k, F.size);
        if (gz_bit < 0) return KVQ_ERR_IO;
        gz_h = gz_bit >> 3;
        s->path_bits |= 32;
        return KVQ_OK;
    }
    int enqueue(S &sg, Produced *out) override
    {
        int rc;
        if ((rc = sg.front())) return rc;
        const hipStream_t st = sg.st;
        const int64_t carry = sg.carry;
        // a run of compressed bytes [rb, re) and a margin behind it
        const int64_t rb = gz_bit >> 3, re = std::min<int64_t>(F.size, rb + run_bytes);
        GzRunOut ro;
        for (int64_t margin = 1 << 20; ; margin *= 4) {
            const int64_t n = std::min<int64_t>(F.size, re + margin) - rb;
            if ((rc = read(rb, n))) return rc;
            if ((rc = g_gz.d_comp.ensure((size_t)std::max<int64_t>(n, 1)))) return rc;
            KVQ_HIP(hipMemcpyAsync(g_gz.d_comp.p, g_gz.pin, (size_t)n, hipMemcpyHostToDevice, st));
            GzDeviceBackend be; be.d_in = g_gz.d_comp.as<uint8_t>(); be.n = n; be.file_end = F.size - rb; be.st = st;
            be.d_win0 = g_gz.d_win.as<uint8_t>(); be.d_win_last = g_gz.d_win.as<uint8_t>();
            be.d_text = sg.text() + carry; be.text_cap = sg.cap() - carry;
            be.grow = [&](int64_t need) -> int {
                int rc2 = sg.grow(carry + need + need / 4 + KVQ_SCANBUFSIZE + 64);
                if (rc2) return rc2;
                be.d_text = sg.text() + carry; be.text_cap = sg.cap() - carry;
                return KVQ_OK;
            };
            const int64_t stop = re >= F.size ? INT64_MAX : (re - rb) * 8;
            kvq_gzip_report part = kvq_gzip_report();
            if ((rc = gz_run(be, n, F.size - rb, gz_bit - rb * 8, stop, gz_wl, chunk_bytes, part, ro, false))) return rc;
            const bool again = ro.status == KVQ_INF_NEED_INPUT && rb + n < F.size;
            gz_report_add(g_gz_report, part, again);
            if (!again) break;
        }
        if (ro.status) {
            kvq_set_error(KVQ_ERR_IO, "error while inflating compressed data : status=%d fpos=%ld", ro.status == KVQ_INF_NEED_INPUT ? KVQ_INF_BUF_ERROR : ro.status,
                          (long)(sg.text_fpos + carry + ro.err_o));
            return KVQ_ERR_IO;
        }
        out->text = ro.text; out->eof = ro.ended;
        if (ro.mbyte >= 0) gz_h = rb + ro.mbyte;
        if (!ro.ended) { gz_bit = rb * 8 + ro.next_bit; gz_wl = (int32_t)ro.wl; out->consumed = std::min<int64_t>(F.size, gz_bit >> 3); }
        else if (ro.end_how == 1) {
            // GzSerial reads a member's data a KVQ_SCANBUFSIZE at a time from behind its header, up to the byte behind its final block
            const int64_t e = rb + ro.end_byte, reads = (e - gz_h + KVQ_SCANBUFSIZE - 1) / KVQ_SCANBUFSIZE;
            out->consumed = std::min<int64_t>(F.size, gz_h + reads * KVQ_SCANBUFSIZE);
        } else out->consumed = ro.end_how == 2 ? rb + ro.end_byte : F.size;
        return KVQ_OK;
    }
};

// what the BAM files of a call share: which of the two BAM buffers takes the next run, the timing events, the report
struct BamShared {
    int bb = 0;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    ~BamShared() { for (int i = 0; i < 4; i++) if (ev[i]) (void)hipEventDestroy(ev[i]); }
    int init()
    {
        g_bam_report = kvq_bam_report();
        for (int i = 0; i < 4; i++) KVQ_HIP(hipEventCreate(&ev[i]));
        return KVQ_OK;
    }
};

// a BAM file: a run of whole blocks through kvq_inflate_bgzf into a BAM buffer, behind the record the run before ended inside
// (the two BAM buffers alternate; the next run is read while the GPU inflates this one); the records found and checked
// (bam_run_find), their text written behind the unfinished chunk (bam_run_emit).  Blocking.
template <class S>
struct BamProducer : Producer<S> {
    BlockRuns &runs; const size_t f; const InputFile &F; BamShared &sh; const int64_t seg_bytes;
    size_t b0 = 0;
    int64_t bcarry = 0, bcarry_src = 0, run_base = 0, skip;          // the unfinished record (BAM buffer sh.bb ^ 1), the stream offset of the buffer's front, header bytes to skip
    BamProducer(BlockRuns &runs_, size_t f_, BamShared &sh_) : runs(runs_), f(f_), F(runs_.files[f_]), sh(sh_), seg_bytes(bam_segment_bytes_default()), skip(F.first) {}
    int enqueue(S &sg, Produced *out) override
    {
        int rc;
        const hipStream_t st = sg.st;
        kvq_bam_report &rep = g_bam_report;
        hipEvent_t *ev = sh.ev;
        const int bb = sh.bb;
        // the run into the BAM buffer, behind the unfinished record
        BlockRuns::Run run;
        if ((rc = runs.take(f, b0, run))) return rc;
        if ((rc = g_bam.d_bam[bb].ensure((size_t)(bcarry + run.isz + 64)))) return rc;
        uint8_t *bam = g_bam.d_bam[bb].as<uint8_t>();
        int64_t n = 0;
        KVQ_HIP(hipEventRecord(ev[0], st));
        if ((rc = bgzf_run_enqueue(F.blocks, run.b0, run.b1, run.slot, bam, (int64_t)g_bam.d_bam[bb].cap, bcarry, g_bam.d_bam[bb ^ 1].as<uint8_t>() + bcarry_src, st, &n))) return rc;
        KVQ_HIP(hipEventRecord(ev[1], st));
        if ((rc = runs.read_ahead(run))) return rc;
        KVQ_HIP(hipStreamSynchronize(st));
        float ms = 0; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) rep.ms_inflate += ms;
        if ((rc = bgzf_run_check(run.slot, (int64_t)(run.b1 - run.b0), run_base))) return rc;
        b0 = run.b1;
        out->eof = run.eof; out->consumed = run.eof ? F.size : run.c1;
        rep.runs++; rep.bam_bytes += run.isz;
        // the records of the run and their text's size
        const int64_t s0 = std::min(skip, n);
        skip -= s0;
        BamRunOut ro;
        if ((rc = bam_run_find(bam, n, F.isize - run_base, F.n_ref, s0, seg_bytes, st, rep, ro))) return rc;
        if (ro.err >= 0) { kvq_set_error(KVQ_ERR_IO, "malformed BAM record : offset=%ld", (long)(run_base + ro.err)); return KVQ_ERR_IO; }
        const int64_t have = sg.carry + ro.text;
        if (have > (4ll << 30) - (1 << 20)) { kvq_set_error(KVQ_ERR_RUNTIME, "BAM batch of %ld text bytes (KVQ_INFLATE_BATCH_MB)", (long)have); return KVQ_ERR_RUNTIME; }
        // the text behind the unfinished chunk (the text buffer of this run is not the one of the batch in flight)
        if (sg.cap() < have + 64 && (rc = sg.grow(have + 64))) return rc;
        if ((rc = sg.front())) return rc;
        KVQ_HIP(hipEventRecord(ev[2], st));
        if ((rc = bam_run_emit(bam, s0, seg_bytes, ro, sg.text(), sg.carry, sg.cap(), st))) return rc;
        KVQ_HIP(hipEventRecord(ev[3], st));
        rep.text_bytes += ro.text;
        out->text = ro.text;
        // the unfinished record goes to the front of the other BAM buffer with the next run
        bcarry = n - ro.end; bcarry_src = ro.end; run_base += ro.end; sh.bb ^= 1;
        return KVQ_OK;
    }
    int check(const S &) override
    {
        float ms = 0; if (hipEventElapsedTime(&ms, sh.ev[2], sh.ev[3]) == hipSuccess) g_bam_report.ms_emit += ms;
        return KVQ_OK;
    }
};

// ---------------------------------------------------------------------------
// the walk
// ---------------------------------------------------------------------------

enum Route { ROUTE_HOST, ROUTE_BGZF, ROUTE_GZIP, ROUTE_BAM };      // how a findseqs call gets its text: the host reader, or here with
                                                                   // every file BGZF to its end / every file some gzip / every file BAM

// One walk over the files, each through the producer of its kind.  Per run: the producer's text and the first cuts are
// enqueued, the producer does its host work (the all-BGZF route reads the next run from disk here, while the GPU inflates and
// cuts this one), the stream is synchronised once for both, and the stage collects.
template <class Sink>
static int stream_device(Sink &sink, kvq_scan *s, const std::vector<InputFile> &files, Route route, int64_t *parsed, int64_t *total_out)
{
    typedef TextStage<Sink> Stage;
    int rc;
    int64_t size_all = 0;
    for (auto &f : files) size_all += f.size;
    sink.begin(size_all);
    const int64_t batch_cap = device_batch_bytes();
    // (BGZF runs never need more text than this; any other gzip and BAM grow the buffer of the run when they do)
    if (route != ROUTE_BAM) for (int i = 0; i < 2; i++) if ((rc = g_dev.d_text[i].ensure((size_t)(batch_cap + KVQ_SCANBUFSIZE + 64)))) return rc;
    Stage sg(sink, s->stream, size_all);
    if ((rc = sg.init())) return rc;
    BlockRuns runs(files, batch_cap);
    BamShared bam;
    if (route == ROUTE_BAM && (rc = bam.init())) return rc;
    if (route == ROUTE_GZIP) {
        if ((rc = g_gz.d_win.ensure(KVQ_INF_WINDOW))) return rc;
        g_gz_report = kvq_gzip_report();
    }
    for (size_t f = 0; f < files.size() && !kvq_stop_requested(); f++) {
        std::unique_ptr<Producer<Stage>> p;
        if (files[f].bam) p.reset(new BamProducer<Stage>(runs, f, bam));
        else if (files[f].bgzf) p.reset(new BgzfProducer<Stage>(runs, f));
        else p.reset(new GzipProducer<Stage>(files[f], s, batch_cap));
        if ((rc = p->open())) return rc;
        Produced out;
        while (!out.eof && !kvq_stop_requested()) {
            if ((rc = p->enqueue(sg, &out)) || (rc = sg.enqueue(out.text)) || (rc = p->ahead())) return rc;
            KVQ_HIP(hipStreamSynchronize(s->stream));
            if ((rc = p->check(sg)) || (rc = sg.collect(out.consumed, out.eof))) return rc;
        }
    }
    if (route == ROUTE_BAM) s->path_bits |= 64;
    *parsed = sg.fpos; *total_out = sg.total;
    return KVQ_OK;
}
