// kvarq_amd/csrc/kvq_reader.hip -- the host reader of engine.findseqs: the concatenated inflated stream of the input
// files (plain or gzip, workhorse.c:559-629), cut into the chunks fastq_read would hand out (workhorse.c:737-956) and
// handed on batch by batch.  Everything here needs zlib and no GPU.  (A plain file is read by pread_run, which the device
// routes use too and kvq_routes.hip defines: the unity build includes that file first.)
#include "kvq_host.h"

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string.h>
#include <zlib.h>
#include <thread>
#include <sys/mman.h>
#include <unistd.h>

// ---------------------------------------------------------------------------
// fastq_rewind / fastq_read chunk cuts on an in-memory stream
// ---------------------------------------------------------------------------

// length of the trailing partial record of buf[0..n): going backwards, the
// first line start '@' met after a line start '+' (workhorse.c:696-718)
int64_t kvq_tail_record(const uint8_t *buf, int64_t n)
{
    bool plus_seen = false;
    for (int64_t k = n - 1; k >= 2; k--) {                 // i = n - k runs 1 .. n-2 (706)
        const uint8_t prev = buf[k - 1];
        if (prev != '\n' && prev != '\r') continue;
        if (buf[k] == '+') plus_seen = true;
        else if (buf[k] == '@' && plus_seen) return n - k;
    }
    return -1;
}

extern "C" int64_t kvq_chunk_offsets(const uint8_t *data, int64_t nbytes, int64_t *offsets, int64_t cap)
{
    int64_t n = 0, cs = 0, fill = 0;
    for (;;) {
        const int64_t want = KVQ_SCANBUFSIZE - (fill - cs);
        const int64_t have = nbytes - fill;
        if (have >= want) {                                // buffer filled, source not dry: cut (916-943)
            const int64_t end = fill + want;
            const int64_t keep = kvq_tail_record(data + cs, end - cs);
            if (keep < 0) return -1;
            if (n < cap) offsets[n] = cs;
            n++;
            cs = end - keep; fill = end;
        } else {                                           // short read: eof, no cut (901-910)
            if (nbytes > cs) { if (n < cap) offsets[n] = cs; n++; }
            break;
        }
    }
    if (n < cap + 1) offsets[n] = nbytes;
    return n;
}

// ---------------------------------------------------------------------------
// the inflated stream of a list of files
// ---------------------------------------------------------------------------

// Serial inflate of one .gz file, member after member (workhorse.c:482-541, 559-629, 790-884).  It owns its
// FILE and knows nothing of the stream around it, so that it can run ahead of the stream in a thread of its
// own (GzAhead): an error is kept -- code, message, position within the file's inflated bytes -- for the
// stream's thread to raise.
struct GzSerial {
    FILE *fd = nullptr; z_stream zs; bool zs_live = false; uint8_t *inbuf = nullptr;
    int64_t remaining = 0;      // compressed bytes of the file not yet read
    int64_t consumed = 0;       // compressed bytes of the file behind the read position (what ftell() says)
    int64_t produced = 0;       // inflated bytes handed out
    int err = 0; char msg[256]; int64_t err_at = -1;          // err_at >= 0: the message ends " fpos=<stream offset of the file + err_at>"

    ~GzSerial() { close(); free(inbuf); }
    void close()
    {
        if (zs_live) { inflateEnd(&zs); zs_live = false; }
        if (fd) { fclose(fd); fd = nullptr; }
    }
    int fail(int code, const char *fmt, const char *a = "", const char *b = "")
    {
        err = code; snprintf(msg, sizeof(msg), fmt, a, b); return code;
    }
    int getc_counted() { const int c = fgetc(fd); if (c != EOF) consumed++; return c; }

    // workhorse.c:482-541
    const char *skip_gz_header(int dist)
    {
        int state = 0, y = 0, c;
        for (c = getc_counted(); state != 2 && y <= dist && c != EOF; c = getc_counted()) {
            if (c == 0x1F && state == 0) state = 1;
            else if (c == 0x8B && state == 1) state = 2;
            else { state = 0; y++; }
        }
        if (state != 2) return "magic bytes not found";
        if (c != 8) return "expected method==DEFLATED";
        const int flags = getc_counted();
        if (flags & (0x02 | 0x20 | 0xC0)) return "unsupported flags (CONTINUATION or ENCRYPTED or RESERVED)";
        for (int i = 0; i < 6; i++) (void)getc_counted();
        if (flags & 0x04) { int n = getc_counted(); n |= getc_counted() << 8; while (n-- > 0) (void)getc_counted(); }
        if (flags & 0x08) { do c = getc_counted(); while (c > 0); }
        if (flags & 0x10) { do c = getc_counted(); while (c > 0); }
        return nullptr;
    }

    // takes over `f`, positioned at file offset `at` of `file_size`: at == 0 is the beginning of the file (the header
    // must start right there, workhorse.c:613-621), anything else a later member (header within 10 bytes; *no_member
    // when there is none: the stream ends, workhorse.c:851-853)
    int start(FILE *f, int64_t file_size, int64_t at, bool *no_member)
    {
        fd = f; consumed = at; produced = 0; err = 0; err_at = -1;
        if (no_member) *no_member = false;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) return fail(KVQ_ERR_RUNTIME, "cannot mz_inflateInit()");
        zs_live = true;
        if (!inbuf) inbuf = (uint8_t *)malloc(KVQ_SCANBUFSIZE);
        if (!inbuf) return fail(KVQ_ERR_MEMORY, "cannot allocate inbuf");
        fseek(fd, (long)at, SEEK_SET);
        remaining = file_size - at;
        const char *m = skip_gz_header(at == 0 ? 0 : 10);
        if (m) {
            if (at == 0) return fail(KVQ_ERR_IO, "no valid gzip header found at beginning of file : %s", m);
            *no_member = true; return KVQ_OK;
        }
        remaining -= consumed - at;
        return KVQ_OK;
    }

    // up to cap inflated bytes; *eof when the file is exhausted; -1 (and err/msg/err_at) on failure
    int64_t read(uint8_t *dst, int64_t cap, bool *eof)
    {
        *eof = false;
        zs.next_out = dst; zs.avail_out = (uInt)cap;
        bool done = false;
        while (zs.avail_out > 0 && !done) {
            if (zs.avail_in == 0) {
                if (remaining <= 0) { done = true; break; }
                const int64_t m = std::min<int64_t>(KVQ_SCANBUFSIZE, remaining);
                if ((int64_t)fread(inbuf, 1, (size_t)m, fd) != m) {
                    fail(KVQ_ERR_IO, "could not read enough bytes from .fastq.gz%s%s", ferror(fd) ? " : I/O error" : "", feof(fd) ? " : premature EOF" : "");
                    return -1;
                }
                consumed += m; remaining -= m;
                zs.next_in = inbuf; zs.avail_in = (uInt)m;
            }
            const int st = inflate(&zs, Z_SYNC_FLUSH);
            if (st != Z_OK && st != Z_STREAM_END && st != Z_BUF_ERROR) {
                err = KVQ_ERR_IO; snprintf(msg, sizeof(msg), "error while inflating compressed data : status=%d", st);
                err_at = produced + (cap - zs.avail_out);
                return -1;
            }
            if (st == Z_STREAM_END) {
                // another gzip member follows when more than a trailer is left (842-866)
                if (remaining + (int64_t)zs.avail_in > 10) {
                    fseek(fd, -(long)zs.avail_in, SEEK_CUR);
                    consumed -= zs.avail_in; remaining += zs.avail_in; zs.avail_in = 0;
                    const int64_t before = consumed;
                    const char *m = skip_gz_header(10);
                    if (m) { remaining = 0; done = true; }
                    else {
                        remaining -= consumed - before;
                        uint8_t *no = zs.next_out; const uInt ao = zs.avail_out;
                        inflateEnd(&zs); memset(&zs, 0, sizeof(zs)); inflateInit2(&zs, -MAX_WBITS);
                        zs.next_out = no; zs.avail_out = ao;
                    }
                } else done = true;
            } else if (st == Z_BUF_ERROR && zs.avail_in == 0 && remaining <= 0) done = true;
        }
        const int64_t n = cap - zs.avail_out;
        if (zs.avail_out > 0) *eof = true;
        produced += n;
        return n;
    }
};

// A GzSerial in a thread of its own, inflating into a queue of blocks for the stream to pick up.  The stream
// is strictly one file after the other (the file positions of hits count inflated bytes of every file before,
// workhorse.c:641-686), but nothing says the files must be INFLATED one after the other: the reader of the
// second file of a pair starts together with the first file's and runs up to `budget` inflated bytes ahead.
struct GzAhead {
    struct Block { uint8_t *p; int64_t n, used, consumed_after; bool eof, failed; };
    static const int64_t BLOCK = 4 << 20;
    GzSerial z; int open_err = 0;
    std::thread th; std::mutex m; std::condition_variable cv; std::deque<Block> q;
    int64_t queued = 0, budget = 0; bool quit = false;
    std::vector<uint8_t *> spare;                 // blocks handed back by the consumer, written again without page faults

    // a fresh block costs a page fault per 4 KiB written, a third of the inflate time itself: ask for huge pages
    static uint8_t *new_block()
    {
        void *p = nullptr;
        if (posix_memalign(&p, 2 << 20, (size_t)BLOCK)) return nullptr;
        (void)madvise(p, (size_t)BLOCK, MADV_HUGEPAGE);
        return (uint8_t *)p;
    }

    GzAhead(const char *name, int64_t budget_bytes) : budget(budget_bytes)
    {
        FILE *f = fopen(name, "rb");
        if (!f) { open_err = z.fail(KVQ_ERR_IO, "cannot open file"); return; }
        fseek(f, 0, SEEK_END); const int64_t size = ftell(f);
        open_err = z.start(f, size, 0, nullptr);
        if (!open_err) th = std::thread([this] { run(); });
    }
    ~GzAhead()
    {
        { std::lock_guard<std::mutex> l(m); quit = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
        for (auto &b : q) free(b.p);
        for (auto p : spare) free(p);
    }
    void run()
    {
        for (;;) {
            uint8_t *mem = nullptr;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return quit || queued < budget; });
                if (quit) return;
                if (!spare.empty()) { mem = spare.back(); spare.pop_back(); }
            }
            Block b = { mem ? mem : new_block(), 0, 0, 0, false, false };
            if (!b.p) { z.fail(KVQ_ERR_MEMORY, "cannot allocate memory for scanning"); b.failed = true; }
            else {
                const int64_t n = z.read(b.p, BLOCK, &b.eof);
                if (n < 0) b.failed = true; else b.n = n;
            }
            b.consumed_after = z.consumed;
            const bool last = b.eof || b.failed;
            {
                std::lock_guard<std::mutex> l(m);
                q.push_back(b); queued += b.n;
            }
            cv.notify_all();
            if (last) return;
        }
    }
    // the consumer's side of GzSerial::read; *consumed follows the compressed bytes behind what has been handed out.
    // Whatever is queued is copied out by up to `nthreads` threads at once: behind the first file of a pair the whole
    // second file may be waiting, and one memcpy stream would then be what the scan waits for.
    int64_t read(uint8_t *dst, int64_t cap, bool *eof, int64_t *consumed, int nthreads)
    {
        struct Span { const uint8_t *from; uint8_t *to; int64_t n; };
        *eof = false;
        int64_t n = 0;
        while (n < cap && !*eof) {
            std::vector<Span> spans;
            size_t whole = 0;                             // blocks used up by this round
            bool failed = false;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return !q.empty(); });
                for (auto &b : q) {                       // (only this thread pops, and a deque keeps its elements in place when the reader pushes)
                    const int64_t k = std::min(cap - n, b.n - b.used);
                    if (k > 0) spans.push_back({ b.p + b.used, dst + n, k });
                    n += k; b.used += k;
                    if (b.used < b.n) break;              // cap reached inside the block
                    *consumed = b.consumed_after;
                    if (b.failed) { failed = true; break; }
                    whole++;
                    if (b.eof) { *eof = true; break; }
                    if (n == cap) break;
                }
            }
            int64_t bytes = 0;
            for (auto &sp : spans) bytes += sp.n;
            const int nt = bytes < (8 << 20) ? 1 : std::max(1, std::min<int>(std::min<int>(nthreads, 8), (int)spans.size()));
            auto copy = [&](int t) { for (size_t i = (size_t)t; i < spans.size(); i += (size_t)nt) memcpy(spans[i].to, spans[i].from, (size_t)spans[i].n); };
            std::vector<std::thread> helpers;
            for (int t = 1; t < nt; t++) helpers.emplace_back(copy, t);
            copy(0);
            for (auto &h : helpers) h.join();
            if (failed) return -1;
            {
                std::lock_guard<std::mutex> l(m);
                for (; whole > 0; whole--) {
                    if (spare.size() < 4) spare.push_back(q.front().p); else free(q.front().p);
                    queued -= q.front().n; q.pop_front();
                }
            }
            cv.notify_all();
        }
        return n;
    }
};

class StreamSource {
public:
    ~StreamSource() { close_file(); }

    // workhorse.c:641-686: sizes of all files first, then the first file is opened
    int open(const char *const *files, int nfiles)
    {
        for (int i = 0; i < nfiles; i++) files_.push_back(files[i]);
        for (auto &f : files_) {
            FILE *fd = fopen(f.c_str(), "rb");
            if (!fd) { kvq_set_error(KVQ_ERR_IO, "cannot open file '%s' for getting filesize", f.c_str()); return KVQ_ERR_IO; }
            fseek(fd, 0, SEEK_END); size_ += ftell(fd); fclose(fd);
        }
        total_ = size_;
        return KVQ_OK;
    }
    bool has_next_file() const { return next_ < files_.size(); }

    // workhorse.c:559-629
    int open_next()
    {
        close_file();
        const std::string &name = files_[next_++];
        fd_ = fopen(name.c_str(), "rb");
        if (!fd_) { kvq_set_error(KVQ_ERR_IO, "cannot open file"); return KVQ_ERR_IO; }
        consumed_ = 0; file_done_ = false; opened_ = true; file_fpos0_ = fpos_; serial_fpos0_ = fpos_;
        fseek(fd_, 0, SEEK_END); file_size_ = ftell(fd_); fseek(fd_, 0, SEEK_SET);
        gz_ = gz_suffix(name);                                                       // by suffix (582)
        bgzf_ = false;
        if (gz_) {
            // a file of BGZF blocks (bgzip: gzip members of at most 64 KiB that carry their own size)
            // is inflated by `nthreads` workers, block by block; anything else by the serial path below,
            // which also takes over should a later member not be a BGZF block
            BgzfBlock first;
            const char *sw = getenv("KVQ_BGZF");                              // KVQ_BGZF=0: serial reader only (diagnostic)
            if (!(sw && sw[0] == '0') && bgzf_peek(fd_, file_size_, 0, &first)) { bgzf_ = true; boff_ = 0; total_ *= 3; start_next_ahead(); return KVQ_OK; }
            if (ahead_next_ && ahead_next_for_ == next_ - 1) ahead_ = std::move(ahead_next_);     // its reader has been running since the file before was opened
            else if (ahead_budget() > 0) ahead_.reset(new GzAhead(name.c_str(), ahead_budget()));
            if (ahead_) {
                if (ahead_->open_err) return raise(ahead_->z);
            } else {
                int rc = z_.start(fd_, file_size_, 0, nullptr);
                fd_ = nullptr;                                                        // (z_ owns the FILE now)
                if (rc) return raise(z_);
                consumed_ = z_.consumed;
            }
            total_ *= 3;                                                              // "random guess" (625)
        }
        start_next_ahead();
        return KVQ_OK;
    }

    // up to cap bytes of the current file's inflated stream; *eof when the file is exhausted
    int64_t read(uint8_t *dst, int64_t cap, bool *eof)
    {
        *eof = false;
        if (file_done_) { *eof = true; return 0; }
        int64_t n = 0;
        if (!gz_) {
            // plain file: `nthreads` readers pread() disjoint slices straight into the pinned buffer
            // (the reference's workers share one fread under a mutex, workhorse.c:746,890)
            const int64_t left = file_size_ - consumed_;
            n = left < cap ? (left < 0 ? 0 : left) : cap;
            kvq_config cfg; kvq_config_get(&cfg);
            if (!pread_run(fileno(fd_), dst, n, consumed_, cfg.nthreads, 32)) { kvq_set_error(KVQ_ERR_IO, "error while reading from file in fastq_read"); return -1; }
            if (n < cap) { *eof = true; file_done_ = true; }
            consumed_ += n;
        } else {
            if (bgzf_) {
                const int64_t got = read_bgzf(dst, cap, eof);
                if (got != -2) return got;            // -2: the next member is no BGZF block -> serial path from here on
            }
            bool end = false;
            if (ahead_) {
                kvq_config cfg; kvq_config_get(&cfg);
                n = ahead_->read(dst, cap, &end, &consumed_, cfg.nthreads);
                if (n < 0) { raise(ahead_->z); return -1; }
            } else {
                n = z_.read(dst, cap, &end);
                if (n < 0) { raise(z_); return -1; }
                consumed_ = z_.consumed;
            }
            if (end) { *eof = true; file_done_ = true; }
            // running estimate of the inflated size, float arithmetic as in 883-884
            if (ftell0_ + consumed_ > 0)
                total_ = (int64_t)(size_t)((float)size_ * (fpos_ + n) / (ftell0_ + consumed_));
        }
        fpos_ += n;
        return n;
    }

    int64_t fpos() const { return fpos_; }
    int64_t total() const { return total_; }

private:
    // ---- BGZF (SAM/BAM specification, section 4.1): gzip member with FEXTRA subfield 'B','C',2,0,BSIZE ----
    typedef kvq_bgzf_entry_ BgzfBlock;                                  // file offset, block bytes, header bytes, inflated bytes

    // is there a well-formed BGZF block at file offset `off`?  (the rules of kvq_bgzf_peek, which the device route walks too)
    static bool bgzf_peek(FILE *fd, int64_t file_size, int64_t off, BgzfBlock *b) { return kvq_bgzf_peek(PreadAt{ fileno(fd) }, file_size, off, b); }

    // inflate as many whole BGZF blocks as fit into cap bytes, nthreads workers; -2 = hand over to the serial path
    int64_t read_bgzf(uint8_t *dst, int64_t cap, bool *eof)
    {
        std::vector<BgzfBlock> blocks;
        int64_t out = 0;
        bool handover = false;
        while (true) {
            if (file_size_ - boff_ <= 10) {                                               // at most a trailer is left (workhorse.c:842)
                consumed_ += file_size_ - boff_; boff_ = file_size_;                      // (the serial reader has read those bytes too)
                *eof = true; file_done_ = true; break;
            }
            BgzfBlock b;
            if (!bgzf_peek(fd_, file_size_, boff_, &b)) { handover = true; break; }
            if (out + b.isize > cap) break;
            blocks.push_back(b); out += b.isize; boff_ += b.size;
        }
        if (handover && blocks.empty()) {
            // the serial reader continues at this member: position the file, skip its header as open_next does
            bgzf_ = false;
            bool no_member = false;
            z_.consumed = consumed_;
            serial_fpos0_ = fpos_;                                                 // (the serial reader counts what IT produces: its error positions are relative to here)
            const int rc = z_.start(fd_, file_size_, boff_, &no_member);
            fd_ = nullptr;
            if (rc) { raise(z_); return -1; }
            // (GzSerial counts file offsets; the stream's count of this file also holds what the block reader skipped)
            consumed_ += z_.consumed - boff_; z_.consumed = consumed_;
            if (no_member) { *eof = true; file_done_ = true; return 0; }          // as behind any member: no further header, the stream ends (851-853)
            return -2;
        }
        // read the compressed bytes of the whole run once, then inflate block by block in parallel
        if (!blocks.empty()) {
            const int64_t c0 = blocks.front().off, c1 = blocks.back().off + blocks.back().size;
            cbuf_.resize((size_t)(c1 - c0));
            const int fdn = fileno(fd_);
            for (int64_t a = 0; a < c1 - c0; ) {
                const ssize_t got = pread(fdn, cbuf_.data() + a, (size_t)(c1 - c0 - a), (off_t)(c0 + a));
                if (got <= 0) { kvq_set_error(KVQ_ERR_IO, "could not read enough bytes from .fastq.gz : I/O error"); return -1; }
                a += got;
            }
            std::vector<int64_t> at(blocks.size());
            int64_t o = 0;
            for (size_t i = 0; i < blocks.size(); i++) { at[i] = o; o += blocks[i].isize; }
            kvq_config cfg; kvq_config_get(&cfg);
            int nt = cfg.nthreads < 1 ? 1 : (cfg.nthreads > 32 ? 32 : cfg.nthreads);
            if ((size_t)nt > blocks.size()) nt = (int)blocks.size();
            std::atomic<int> bad{0};
            auto work = [&](int t) {
                z_stream z; memset(&z, 0, sizeof(z));
                if (inflateInit2(&z, -MAX_WBITS) != Z_OK) { bad = 1; return; }
                for (size_t i = blocks.size() * t / nt; i < blocks.size() * (t + 1) / nt; i++) {
                    const BgzfBlock &b = blocks[i];
                    z.next_in = cbuf_.data() + (b.off - c0) + b.hdr; z.avail_in = b.size - b.hdr - 8;
                    z.next_out = dst + at[i]; z.avail_out = b.isize;
                    const int st = inflate(&z, Z_FINISH);
                    if (st != Z_STREAM_END || z.avail_out != 0) { bad = (st == Z_STREAM_END || st == Z_OK || st == Z_BUF_ERROR) ? 2 : 3; break; }
                    inflateReset(&z);
                }
                inflateEnd(&z);
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nt; t++) th.emplace_back(work, t);
            work(0);
            for (auto &x : th) x.join();
            if (bad.load()) {
                kvq_set_error(KVQ_ERR_IO, "error while inflating compressed data : status=%d fpos=%ld", bad.load() == 3 ? Z_DATA_ERROR : Z_BUF_ERROR, (long)fpos_);
                return -1;
            }
            consumed_ += c1 - c0;
        }
        if (ftell0_ + consumed_ > 0)
            total_ = (int64_t)(size_t)((float)size_ * (fpos_ + out) / (ftell0_ + consumed_));      // as in the serial path (883-884)
        fpos_ += out;
        return out;
    }

    // an error met by a gzip reader, possibly in its own thread, raised in this one
    int raise(const GzSerial &z)
    {
        if (z.err_at >= 0) kvq_set_error(z.err, "%s fpos=%ld", z.msg, (long)((&z == &z_ ? serial_fpos0_ : file_fpos0_) + z.err_at));
        else kvq_set_error(z.err, "%s", z.msg);
        return z.err;
    }

    // inflated bytes a reader may run ahead of the stream, per reader (the current file's and the next file's run at once):
    // KVQ_GZ_AHEAD_MB, else 256 MiB -- the scan takes 64 MiB at a time, a few batches of look-ahead keep it fed -- and never
    // more than an eighth of the free memory; none with nthreads == 1 (one worker was asked for).  Worked out once per walk.
    int64_t ahead_budget()
    {
        if (ahead_budget_ >= 0) return ahead_budget_;
        kvq_config cfg; kvq_config_get(&cfg);
        if (cfg.nthreads <= 1) return ahead_budget_ = 0;
        if (const char *e = getenv("KVQ_GZ_AHEAD_MB")) return ahead_budget_ = (int64_t)atol(e) << 20;
        const int64_t avail = (int64_t)sysconf(_SC_AVPHYS_PAGES) * sysconf(_SC_PAGESIZE);
        return ahead_budget_ = std::max<int64_t>(64ll << 20, std::min<int64_t>(avail / 8, 256ll << 20));
    }
    int64_t ahead_budget_ = -1;

    // the file after the one just opened: when it is a plain .gz (not BGZF -- those are inflated block-parallel when
    // their turn comes), its reader starts now
    void start_next_ahead()
    {
        if (next_ >= files_.size() || ahead_next_ || ahead_budget() <= 0) return;
        const std::string &name = files_[next_];
        if (!gz_suffix(name)) return;
        const char *sw = getenv("KVQ_BGZF");
        if (!(sw && sw[0] == '0')) {
            FILE *f = fopen(name.c_str(), "rb");
            if (!f) return;                                     // (open_next reports it when the file's turn comes)
            fseek(f, 0, SEEK_END);
            BgzfBlock first;
            const bool is_bgzf = bgzf_peek(f, ftell(f), 0, &first);
            fclose(f);
            if (is_bgzf) return;
        }
        ahead_next_.reset(new GzAhead(name.c_str(), ahead_budget()));
        ahead_next_for_ = next_;
    }

    void close_file()
    {
        if (opened_) { ftell0_ += consumed_; opened_ = false; }
        if (fd_) { fclose(fd_); fd_ = nullptr; }
        z_.close(); ahead_.reset();
    }

    std::vector<std::string> files_; size_t next_ = 0;
    FILE *fd_ = nullptr; bool gz_ = false, file_done_ = true;
    bool opened_ = false; int64_t file_fpos0_ = 0;                              // a file is open / the stream offset it began at
    int64_t serial_fpos0_ = 0;                                                  // ... / the stream offset at which z_ started producing (behind a BGZF run: later than the file)
    GzSerial z_;                                                                // serial .gz reader in this thread ...
    std::unique_ptr<GzAhead> ahead_, ahead_next_; size_t ahead_next_for_ = 0;   // ... or in its own; the next file's, already running
    bool bgzf_ = false; int64_t boff_ = 0; std::vector<uint8_t> cbuf_;       // BGZF: next block's file offset, compressed run
    int64_t size_ = 0, ftell0_ = 0, consumed_ = 0, fpos_ = 0, total_ = 0, file_size_ = 0;
};

// ---------------------------------------------------------------------------
// driver
// ---------------------------------------------------------------------------

// new stream bytes per batch (KVQ_BATCH_BYTES_MB: 16..512, read once; the two pinned buffers are of this size)
static const int64_t BATCH_BYTES = [] { const char *e = getenv("KVQ_BATCH_BYTES_MB"); const long v = e ? atol(e) : 0; return (int64_t)(v >= 16 && v <= 512 ? v : 64) << 20; }();

// Walk the files once: Sink::batch(data, nbytes, chunk offsets, nchunks, fpos,
// parsed, total) is called for every run of whole chunks, in stream order.
// pin2 (optional): a second buffer of the same size; the walk then alternates between the two
// after every batch, so that the sink may still be reading the batch it was handed last (the
// sink must be done with a batch when it is handed the next one)
template <class Sink>
static int stream_batches(Sink &sink, const char *const *files, int nfiles, uint8_t *pin, int64_t pin_cap,
                          int64_t *parsed, int64_t *total, uint8_t *pin2 = nullptr)
{
    StreamSource src;
    int rc = src.open(files, nfiles);
    if (rc) return rc;
    sink.begin(src.total());
    double t_read = 0, t_cut = 0, t_sink = 0, t_carry = 0; int64_t nbatch = 0;       // (KVQ_TIMING=1: where the host's time goes)
    struct Report { double &a, &b, &c, &d; int64_t &n; ~Report() { if (g_timing) fprintf(stderr, "stream_batches: %lld batches; read %.1f  cut %.1f  sink (wait for the last batch + enqueue) %.1f  carry %.1f ms\n", (long long)n, a, b, c, d); } } report{ t_read, t_cut, t_sink, t_carry, nbatch };

    while (src.has_next_file() && !kvq_stop_requested()) {
        if ((rc = src.open_next())) return rc;
        // chunker state of this file, offsets relative to pin[0]
        int64_t have = 0;              // bytes of the file's stream sitting in pin
        int64_t pin_fpos = src.fpos(); // stream offset of pin[0]
        int64_t cs = 0, fill = 0;      // current chunk start / how far the reference has read (== cs + leftover)
        bool eof = false;
        while (!kvq_stop_requested()) {
            // top up
            const double tr0 = now_ms();
            while (!eof && have < pin_cap) {
                const int64_t n = src.read(pin + have, pin_cap - have, &eof);
                if (n < 0) return kvq_error_code();
                have += n;
                if (n == 0 && !eof) break;
            }
            const double tr1 = now_ms(); t_read += tr1 - tr0;
            // cut chunks the way fastq_read does (workhorse.c:737-956)
            std::vector<int64_t> off;
            bool file_finished = false;
            for (;;) {
                const int64_t want = KVQ_SCANBUFSIZE - (fill - cs);
                if (have - fill >= want) {
                    const int64_t end = fill + want;
                    const int64_t keep = kvq_tail_record(pin + cs, end - cs);
                    if (keep < 0) {
                        kvq_set_error(KVQ_ERR_RUNTIME, "could find beginning of record; read %ld bytes up to %ld", (long)want, (long)(pin_fpos + end));
                        return KVQ_ERR_RUNTIME;
                    }
                    off.push_back(cs);
                    cs = end - keep; fill = end;
                } else if (eof) {
                    if (have > cs) off.push_back(cs);
                    cs = fill = have; file_finished = true;
                    break;
                } else break;        // need more data
            }
            const int64_t batch_begin = off.empty() ? cs : off[0];
            const int64_t batch_end = cs;
            const double tr2 = now_ms(); t_cut += tr2 - tr1;
            if (!off.empty()) {
                off.push_back(batch_end);
                for (auto &o : off) o -= batch_begin;
                rc = sink.batch(pin + batch_begin, batch_end - batch_begin, off.data(), (int64_t)off.size() - 1,
                                pin_fpos + batch_begin, src.fpos(), src.total());
                if (rc) return rc;
                nbatch++;
            }
            const double tr3 = now_ms(); t_sink += tr3 - tr2;
            if (file_finished) {
                if (pin2 && !off.empty()) std::swap(pin, pin2);       // the next file starts in the other buffer
                break;
            }
            // carry the unfinished chunk to the front of the (other) buffer
            const int64_t carry = have - cs;
            if (carry >= pin_cap) { kvq_set_error(KVQ_ERR_RUNTIME, "buf_size < fastq->buf_size !"); return KVQ_ERR_RUNTIME; }
            if (pin2 && !off.empty()) { memcpy(pin2, pin + cs, (size_t)carry); std::swap(pin, pin2); }
            else memmove(pin, pin + cs, (size_t)carry);
            pin_fpos += cs; fill -= cs; have = carry; cs = 0;
            t_carry += now_ms() - tr3;
        }
    }
    *parsed = src.fpos(); *total = src.total();
    return KVQ_OK;
}

// host-only view of the same walk (no GPU): the chunks fastq_read would hand
// out, as (stream offset, length) pairs -- what the CPU tests compare with the oracle
struct PlanSink {
    int64_t *fpos, *len; int64_t cap, n = 0;
    void begin(int64_t) {}
    int batch(const uint8_t *, int64_t, const int64_t *off, int64_t nchunks, int64_t base, int64_t, int64_t)
    {
        for (int64_t c = 0; c < nchunks; c++, n++)
            if (n < cap) { fpos[n] = base + off[c]; len[n] = off[c + 1] - off[c]; }
        return KVQ_OK;
    }
};

extern "C" int64_t kvq_host_chunk_plan(const char *const *files, int32_t nfiles, int64_t *chunk_fpos, int64_t *chunk_len,
                                       int64_t cap, int64_t *parsed, int64_t *total, int64_t batch_bytes)
{
    kvq_clear_error();
    const int64_t pin_cap = (batch_bytes > 0 ? batch_bytes : BATCH_BYTES) + 2 * KVQ_SCANBUFSIZE;
    uint8_t *buf = (uint8_t *)malloc((size_t)pin_cap);
    if (!buf) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for scanning"); return -1; }
    PlanSink sink; sink.fpos = chunk_fpos; sink.len = chunk_len; sink.cap = cap;
    const int rc = stream_batches(sink, files, nfiles, buf, pin_cap, parsed, total);
    free(buf);
    return rc ? -1 : sink.n;
}
