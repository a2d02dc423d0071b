// kvarq_amd/csrc/kvq_findseqs.hip -- engine.findseqs (workhorse.c:1249-1464) on
// top of the scan object: the batches of the host reader (kvq_reader.hip) or of a
// device route (kvq_routes.hip) handed to the GPU one by one; live stats and
// cooperative stop (workhorse.c:1205-1244, 1469-1479).
#include "kvq_host.h"

#include <atomic>
#include <fcntl.h>
#include <mutex>
#include <signal.h>
#include <string.h>

int kvq_scan_finish_internal(kvq_scan *s);

// ---------------------------------------------------------------------------
// live state shared with engine.stats()/engine.stop()
// ---------------------------------------------------------------------------

static std::atomic<int> g_running{0}, g_stop{0}, g_sigints{0};
static struct { kvq_table *t = nullptr; kvq_scan *s = nullptr; int dev = -1; } g_kept;       // the last kvq_findseqs call's table and scan object (kvq_findseqs_free)
static std::mutex g_kept_lock;
void kvq_drop_kept_scan()
{
    std::lock_guard<std::mutex> l(g_kept_lock);
    if (g_kept.s) { kvq_table *kt = g_kept.t; kvq_scan_destroy(g_kept.s); kvq_table_destroy(kt); g_kept.t = nullptr; g_kept.s = nullptr; }
}
static std::mutex g_live_lock;
static struct {
    int64_t records = 0, parsed = 0, total = 0, longest = -1;
    int32_t nseq = 0;
    std::vector<int64_t> readlengths = std::vector<int64_t>(KVQ_MAX_READLENGTH, 0), nseqhits, nseqbasehits;
} g_live;

extern "C" void kvq_request_stop(void) { g_stop++; }
bool kvq_stop_requested() { return g_stop.load() != 0; }
extern "C" void kvq_count_sigint(void) { g_sigints++; }

// The reference installs its counting handler with signal() when the module is imported (workhorse.c:133-136,
// 1632): a C handler, so that a SIGINT is counted while the main thread sits inside findseqs (a Python-level
// handler only runs once the interpreter gets control back).  Here installing it is an explicit call, and it
// can be undone; a lock-free atomic increment is all the handler does.
static struct sigaction g_sigint_before;
static bool g_sigint_installed = false;
static void on_sigint(int) { g_sigints++; }
static_assert(std::atomic<int>::is_always_lock_free, "the SIGINT handler only touches a lock-free counter");

extern "C" int kvq_sigint_counter_install(void)
{
    if (g_sigint_installed) return KVQ_OK;
    struct sigaction sa; memset(&sa, 0, sizeof(sa));
    sa.sa_handler = on_sigint; sigemptyset(&sa.sa_mask); sa.sa_flags = SA_RESTART;
    if (sigaction(SIGINT, &sa, &g_sigint_before) != 0) { kvq_set_error(KVQ_ERR_RUNTIME, "cannot install the SIGINT handler"); return KVQ_ERR_RUNTIME; }
    g_sigint_installed = true;
    return KVQ_OK;
}

extern "C" void kvq_sigint_counter_remove(void)
{
    if (!g_sigint_installed) return;
    (void)sigaction(SIGINT, &g_sigint_before, nullptr);
    g_sigint_installed = false;
}

extern "C" void kvq_poll_stats(kvq_live_stats *out, int64_t *readlengths, int64_t *nseqhits, int64_t *nseqbasehits, int32_t nseq_cap)
{
    std::lock_guard<std::mutex> l(g_live_lock);
    if (out) {
        out->records_parsed = g_live.records; out->parsed = g_live.parsed; out->total = g_live.total;
        out->rls_longest = g_live.longest; out->nseq = g_live.nseq; out->running = g_running.load();
        out->sigints = g_sigints.load(); out->stop_requested = g_stop.load();
    }
    if (readlengths) memcpy(readlengths, g_live.readlengths.data(), KVQ_MAX_READLENGTH * sizeof(int64_t));
    const int32_t n = std::min<int32_t>(nseq_cap, g_live.nseq);
    if (nseqhits && n > 0) memcpy(nseqhits, g_live.nseqhits.data(), (size_t)n * sizeof(int64_t));
    if (nseqbasehits && n > 0) memcpy(nseqbasehits, g_live.nseqbasehits.data(), (size_t)n * sizeof(int64_t));
}

static void live_reset(int32_t nseq, int64_t total)
{
    std::lock_guard<std::mutex> l(g_live_lock);
    g_live.records = 0; g_live.parsed = 0; g_live.total = total; g_live.longest = -1; g_live.nseq = nseq;
    std::fill(g_live.readlengths.begin(), g_live.readlengths.end(), 0);
    g_live.nseqhits.assign((size_t)nseq, 0); g_live.nseqbasehits.assign((size_t)nseq, 0);
}

static void live_from_counters(const kvq_table *t, const int64_t *ctr, int64_t parsed, int64_t total)
{
    std::lock_guard<std::mutex> l(g_live_lock);
    g_live.records = ctr[KVQ_CTR_RECORDS]; g_live.longest = ctr[KVQ_CTR_LONGEST] - 1;
    g_live.parsed = parsed; g_live.total = total;
    memcpy(g_live.readlengths.data(), ctr + KVQ_CTR_READLENGTHS, KVQ_MAX_READLENGTH * sizeof(int64_t));
    if (t->nseq) {
        memcpy(g_live.nseqhits.data(), ctr + t->off_nseqhits, (size_t)t->nseq * sizeof(int64_t));
        memcpy(g_live.nseqbasehits.data(), ctr + t->off_nseqbasehits, (size_t)t->nseq * sizeof(int64_t));
    }
}

// ---------------------------------------------------------------------------
// the GPU sink: one kvq_scan_host per batch, live stats after each
struct ScanSink {
    kvq_scan *s = nullptr;
    // The live statistics (engine.stats() from another thread while findseqs runs: workhorse.c:1205-1244 reads the workers' counters
    // under their lock) are ONE consistent snapshot: the head of the counter array copied on the scan's own stream, behind the kernels
    // of the batches enqueued so far and in front of the next one's, into pinned memory -- published by the next call together with
    // the byte count that belongs to it.  (Round 3 copied on the null stream, beside the non-blocking stream's kernels: records, read
    // lengths and hits per sequence of different batches in one answer.)
    int64_t *snap = nullptr; size_t snap_cap = 0, head = 0; hipEvent_t snap_ev = nullptr;
    bool snap_pending = false; int64_t snap_parsed = 0, enq_parsed = 0, last_parsed = 0;
    bool staged = false;               // batches are device text of the device-inflate route (kvq_scan_staged), not host buffers
    ~ScanSink()
    {
        if (s && s->stream) (void)hipStreamSynchronize(s->stream);          // (the snapshot copy may still be on its way into snap)
        if (snap_ev) (void)hipEventDestroy(snap_ev);
        if (snap) pinned_give(snap, snap_cap);
    }
    void begin(int64_t total)
    {
        live_reset(s->t->nseq, total);
        // (only the head of the counter array -- scalars, read lengths, hits per sequence: 12 KB for the MTBC table -- not the
        // coverage and mutation counters behind it, 0.8 MB)
        head = std::min((size_t)std::max<int64_t>(s->t->off_nseqbasehits + s->t->nseq, KVQ_CTR_READLENGTHS + KVQ_MAX_READLENGTH), (size_t)s->t->ctr_len);
        if (!snap) snap = (int64_t *)pinned_take(head * 8, &snap_cap);
        if (!snap_ev) (void)hipEventCreateWithFlags(&snap_ev, hipEventDisableTiming);
        snap_pending = false; enq_parsed = last_parsed = 0;
    }
    int batch(const uint8_t *data, int64_t nbytes, const int64_t *off, int64_t nchunks, int64_t fpos, int64_t parsed, int64_t total)
    {
        // publish the snapshot taken behind the batches that were enqueued two calls ago (it landed while this batch was read)
        if (snap_pending) {
            if (hipEventSynchronize(snap_ev) != hipSuccess) { kvq_set_error(KVQ_ERR_DEVICE, "device failure during scan"); return KVQ_ERR_DEVICE; }
            live_from_counters(s->t, snap, snap_parsed, total);            // (it reads the head only)
            snap_pending = false;
        }
        // hand this batch over (its text sets out at once, the kernels of the batch before it are enqueued: kvq_scan_host_async) and
        // return, so that the reader fills the other host buffer while this one crosses PCIe
        const int rc = staged ? kvq_scan_staged(s, data, nbytes, off, nchunks, fpos) : kvq_scan_host_async(s, data, nbytes, off, nchunks, fpos);
        if (rc) return rc;
        // the stream now holds the kernels of every batch up to the one handed over in the call before this -- up to this one for
        // staged text, whose kernels kvq_scan_staged enqueues at once: snapshot behind them, with the byte count that belongs to it
        const int64_t behind = staged ? parsed : last_parsed;
        if (snap && snap_ev && behind > 0) {
            if (hipMemcpyAsync(snap, s->d_ctr, head * 8, hipMemcpyDeviceToHost, s->stream) == hipSuccess && hipEventRecord(snap_ev, s->stream) == hipSuccess) {
                snap_pending = true; snap_parsed = behind;
            } else (void)hipGetLastError();
        }
        last_parsed = parsed;
        return KVQ_OK;
    }
};

// one pass over the files with the current arena; KVQ_NEED_RESCAN asks for another.  route: the host reader through the two
// pinned buffers, or a device route over `in`, the files as input_open describes them
static int findseqs_pass(kvq_scan *s, Route route, const char *const *files, int nfiles, uint8_t *pin, uint8_t *pin2, int64_t pin_cap,
                         const std::vector<InputFile> &in)
{
    ScanSink sink; sink.s = s; sink.staged = route != ROUTE_HOST;
    int64_t parsed = 0, total = 0;
    const double tp0 = now_ms();
    int rc = route != ROUTE_HOST ? stream_device(sink, s, in, route, &parsed, &total)
                                 : stream_batches(sink, files, nfiles, pin, pin_cap, &parsed, &total, pin2);       // two host buffers
    if (g_timing) fprintf(stderr, "findseqs pass: stream %.1f ms\n", now_ms() - tp0);
    if (rc) return rc;
    s->parsed = parsed; s->total = total;
    {
        std::lock_guard<std::mutex> l(g_live_lock);
        g_live.parsed = parsed; g_live.total = total;
    }
    rc = kvq_scan_finish_internal(s);
    if (rc == KVQ_OK) live_from_counters(s->t, s->h_ctr.data(), parsed, total);     // stats() after the scan == the scan's stats
    return rc;
}

static kvq_scan *findseqs_impl(const char *const *files, int32_t nfiles,
                               const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, uint32_t flags, const kvq_find_opts *opts = nullptr)
{
    kvq_clear_error();
    if ((flags & KVQ_FIND_PROFILE) && (!opts || opts->n_cutoffs < 0 || opts->n_cutoffs > KVQ_PROFILE_MAX_CUTOFFS)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: at most %d cutoffs", KVQ_PROFILE_MAX_CUTOFFS);
        return nullptr;
    }
    if ((flags & KVQ_FIND_CYCLES) && !(flags & KVQ_FIND_PROFILE)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_CYCLES needs KVQ_FIND_PROFILE (the cycles ride on the profile)");
        return nullptr;
    }
    if ((flags & (KVQ_FIND_READ_STATS | KVQ_FIND_DUPLICATION)) && !(flags & KVQ_FIND_PROFILE)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_READ_STATS and KVQ_FIND_DUPLICATION need KVQ_FIND_PROFILE (the per-read statistics ride on the profile)");
        return nullptr;
    }
    if ((flags & KVQ_FIND_OVERREPRESENTED) && !(flags & KVQ_FIND_PROFILE)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_OVERREPRESENTED needs KVQ_FIND_PROFILE (the overrepresented sequences ride on the profile)");
        return nullptr;
    }
    // the probes of KVQ_FIND_ADAPTERS and KVQ_FIND_CLIP -- one block for both -- ride behind the 20 bytes of kvq_find_opts: read only with
    // one of the flags, and only when the size covers them
    const uint8_t *probes[KVQ_ADAPT_MAX_PROBES] = { nullptr }; int32_t probe_lens[KVQ_ADAPT_MAX_PROBES] = { 0 }, nprobes = 0;
    if ((flags & KVQ_FIND_ADAPTERS) && !(flags & KVQ_FIND_PROFILE)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_ADAPTERS needs KVQ_FIND_PROFILE (the adapter content rides on the profile)");
        return nullptr;
    }
    if (flags & (KVQ_FIND_ADAPTERS | KVQ_FIND_CLIP)) {
        const kvq_find_opts_adapters *oa = (const kvq_find_opts_adapters *)opts;
        if (!opts || opts->size < sizeof(kvq_find_opts_adapters)) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: bad size"); return nullptr; }
        if (oa->n_probes < 1 || oa->n_probes > KVQ_ADAPT_MAX_PROBES) {
            kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_ADAPTERS and KVQ_FIND_CLIP take 1 to %d probes", KVQ_ADAPT_MAX_PROBES);
            return nullptr;
        }
        nprobes = oa->n_probes;
        for (int32_t k = 0; k < nprobes; k++) { probes[k] = oa->probes[k]; probe_lens[k] = oa->lens[k]; }
    }
    // the mismatch rate of KVQ_FIND_ADAPTER_MISMATCHES rides behind the probes: read only with the flag, and only when the size covers it
    int32_t mismatch_per = 0;
    if (flags & KVQ_FIND_ADAPTER_MISMATCHES) {
        if (!(flags & (KVQ_FIND_ADAPTERS | KVQ_FIND_CLIP))) {
            kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_ADAPTER_MISMATCHES needs KVQ_FIND_ADAPTERS or KVQ_FIND_CLIP (it is the rule of their probes)");
            return nullptr;
        }
        if (opts->size < sizeof(kvq_find_opts_adapters_mm)) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: bad size"); return nullptr; }
        mismatch_per = ((const kvq_find_opts_adapters_mm *)opts)->mismatch_per;
        if (!adapt_per_ok("kvq_findseqs_opts", mismatch_per)) return nullptr;
    }
    // min_length and the path of KVQ_FIND_EMIT ride behind the mismatch rate: read only with the flag, and only when the size covers them
    int32_t emit_min = -1; const char *emit_path = nullptr;
    if (flags & KVQ_FIND_EMIT) {
        if (!opts || opts->size < sizeof(kvq_find_opts_emit)) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: bad size"); return nullptr; }
        emit_min = ((const kvq_find_opts_emit *)opts)->min_length; emit_path = ((const kvq_find_opts_emit *)opts)->path;
        if (!emit_path || !emit_path[0]) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_EMIT needs the path of the output"); return nullptr; }
    }
    if ((flags & KVQ_FIND_EMIT_BGZF) && !(flags & KVQ_FIND_EMIT)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: KVQ_FIND_EMIT_BGZF needs KVQ_FIND_EMIT (it is the form of its output)");
        return nullptr;
    }
    int expected = 0;
    if (!g_running.compare_exchange_strong(expected, 1)) {            // workhorse.c:1258-1263
        kvq_set_error(KVQ_ERR_RUNTIME, "findseqs() already running!");
        return nullptr;
    }
    g_stop = 0; g_sigints = 0;                                         // workhorse.c:1264-1265
    const double tf0 = now_ms();
    // the table and the scan object of the last call are kept (kvq_findseqs_free): a caller that scans file after file with
    // the same sequences and settings -- the usual case -- does not build the seed index and a dozen device buffers again
    kvq_table *t = nullptr; kvq_scan *s = nullptr;
    {
        kvq_config cfg; kvq_config_get(&cfg);
        std::lock_guard<std::mutex> l(g_kept_lock);
        int dev_now = 0; (void)hipGetDevice(&dev_now);
        if (g_kept.s && g_kept.dev == dev_now && nseq == g_kept.t->nseq && memcmp(&cfg, &g_kept.t->cfg, sizeof(cfg)) == 0) {
            bool same = true;
            for (int32_t i = 0; i < nseq && same; i++) {
                const int32_t len = g_kept.t->h_off[i + 1] - g_kept.t->h_off[i];
                same = seqlens[i] == len && memcmp(seqs[i], g_kept.t->h_tab.data() + g_kept.t->h_off[i], (size_t)len) == 0;
            }
            if (same && kvq_scan_reset(g_kept.s) == KVQ_OK) {
                t = g_kept.t; s = g_kept.s; g_kept.t = nullptr; g_kept.s = nullptr;
                s->tile_bytes = 0; s->rec_bytes = 0;                  // (another file: the tiles are sized from its own head)
            }
        }
        if (!s && g_kept.s) { kvq_table *kt = g_kept.t; kvq_scan_destroy(g_kept.s); kvq_table_destroy(kt); g_kept.t = nullptr; g_kept.s = nullptr; }
        kvq_clear_error();
    }
    if (!s) {
        t = kvq_table_create(seqs, seqlens, nseq, nullptr);
        s = t ? kvq_scan_create(t, nullptr) : nullptr;
    }
    if (s && (kvq_scan_set_records(s, (flags & KVQ_FIND_RECORDS) ? 1 : 0) ||
              kvq_scan_set_long_reads(s, (flags & KVQ_FIND_LONG_READS) ? 1 : (flags & KVQ_FIND_LONG_READS_AUTO) ? 2 : 0) ||
              kvq_scan_set_profile(s, opts ? opts->cutoffs : nullptr, (flags & KVQ_FIND_PROFILE) ? opts->n_cutoffs : -1) ||
              kvq_scan_set_cycles(s, (flags & KVQ_FIND_CYCLES) ? 1 : 0) ||
              kvq_scan_set_read_stats(s, ((flags & KVQ_FIND_READ_STATS) ? KVQ_READ_STATS : 0) | ((flags & KVQ_FIND_DUPLICATION) ? KVQ_READ_DUPLICATION : 0)) ||
              kvq_scan_set_overrepresented(s, (flags & KVQ_FIND_OVERREPRESENTED) ? 1 : 0) ||
              kvq_scan_set_adapters(s, probes, probe_lens, (flags & KVQ_FIND_ADAPTERS) ? nprobes : 0) ||
              kvq_scan_set_clip(s, probes, probe_lens, (flags & KVQ_FIND_CLIP) ? nprobes : 0) ||
              kvq_scan_set_adapter_mismatches(s, mismatch_per) ||
              kvq_scan_set_emit(s, (flags & KVQ_FIND_EMIT) ? 1 : 0, emit_min) ||
              ((flags & KVQ_FIND_EMIT) && kvq_scan_set_emit_compress(s, (flags & KVQ_FIND_EMIT_BGZF) ? 1 : 0)))) {
        kvq_scan_destroy(s); kvq_table_destroy(t); s = nullptr; t = nullptr;
    }
    // the one output of KVQ_FIND_EMIT: every file of the call goes to it, in order (a rescan after an arena overflow empties it: pass_clear)
    int emit_fd = -1;
    if (s && emit_path) {
        emit_fd = open(emit_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        if (emit_fd < 0 || kvq_scan_set_emit_fd(s, emit_fd)) {
            if (emit_fd < 0) kvq_set_error(KVQ_ERR_IO, "cannot open '%s' for the emitted reads", emit_path);
            else close(emit_fd);
            emit_fd = -1;
            kvq_scan_destroy(s); kvq_table_destroy(t); s = nullptr; t = nullptr;
        }
    }
    const double tf1 = now_ms();
    // the two pinned host buffers outlive the call: pinning and unpinning 130 MB costs more than
    // streaming a 1 GB file through them (only one findseqs runs at a time, g_running)
    static uint8_t *g_pin = nullptr;
    const int64_t pin_cap = BATCH_BYTES + 2 * KVQ_SCANBUFSIZE;
    // How the text gets to the GPU.  BAM files (by their bytes, whatever the flags say): all of them take the BAM route; BAM
    // beside other files is refused.  (A file that cannot be opened leaves the decision to the other routes, which report it.)
    // A device route of gzip files: asked for, and every file is a ".gz" (the host reader decides by suffix) that is BGZF to
    // its end -- or, with KVQ_FIND_DEVICE_GZIP, any gzip, each file taking its own way; else the host route, unchanged.
    Route route = ROUTE_HOST;
    std::vector<InputFile> in;
    bool failed = false;
    if (s) {
        auto open_all = [&](bool bam) {
            in.resize((size_t)std::max(nfiles, 0));
            for (int32_t i = 0; i < nfiles; i++) {
                if ((!bam && !gz_suffix(files[i])) || input_open(files[i], bam, in[i]) != KVQ_OK) return false;
                if (!bam && !in[i].bgzf && !(flags & KVQ_FIND_DEVICE_GZIP)) return false;          // (no route for it: the files behind it need no walk)
            }
            return nfiles > 0;
        };
        int nbam = 0; bool unreadable = false;
        for (int32_t i = 0; i < nfiles; i++) { const int v = bam_peek(files[i]); unreadable |= v < 0; nbam += v > 0; }
        if (!unreadable && nbam > 0 && nbam < nfiles) { kvq_set_error(KVQ_ERR_IO, "cannot scan BAM and FastQ files in one call"); failed = true; }
        else if (!unreadable && nbam > 0) { route = ROUTE_BAM; failed = !open_all(true); }
        else if (flags & (KVQ_FIND_DEVICE_INFLATE | KVQ_FIND_DEVICE_GZIP)) {
            if (open_all(false)) {
                bool all_bgzf = true;
                for (auto &f : in) all_bgzf &= f.bgzf;
                route = all_bgzf ? ROUTE_BGZF : (flags & KVQ_FIND_DEVICE_GZIP) ? ROUTE_GZIP : ROUTE_HOST;
            } else kvq_clear_error();                                  // (the host route reports what is wrong with a file)
        }
    }
    if (s && !failed && route == ROUTE_HOST && !g_pin && hipHostMalloc((void **)&g_pin, (size_t)pin_cap * 2, hipHostMallocDefault) != hipSuccess) {
        kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for scanning"); g_pin = nullptr;
    }
    uint8_t *const pin = g_pin;
    // KVQ_BATCH_MB=<2..64>: smaller batches (diagnostic: many batches out of a small file); the buffers keep their size
    int64_t use_cap = pin_cap;
    if (const char *mb = getenv("KVQ_BATCH_MB")) {
        const long v = atol(mb);
        if (v >= 2 && (v << 20) < BATCH_BYTES) use_cap = ((int64_t)v << 20) + 2 * KVQ_SCANBUFSIZE;
    }
    const double tf2 = now_ms();
    if (s && !failed && (pin || route != ROUTE_HOST)) {
        for (int attempt = 0; attempt < 4; attempt++) {
            const int rc = findseqs_pass(s, route, files, nfiles, pin, pin ? pin + pin_cap : nullptr, use_cap, in);
            if (rc != KVQ_NEED_RESCAN) break;
            // the hit arena was too small (it has been enlarged): scan again from the start
            if (kvq_scan_reset(s)) break;
            if (attempt == 3) kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results");
        }
    }
    const double tf3 = now_ms();
    if (s && s->stream) (void)hipStreamSynchronize(s->stream);        // nothing may still be reading the host buffers
    if (emit_fd >= 0) {
        // (the scan object may be kept for the next call: it must not hold the descriptor of a file this call closes)
        emit_detach_fd(s);
        if (close(emit_fd) != 0 && !kvq_error_code()) kvq_set_error(KVQ_ERR_IO, "cannot write the emitted reads to '%s'", emit_path);
    }
    if (g_timing) fprintf(stderr, "findseqs: table+scan %.1f  pinned alloc %.1f  passes %.1f  free %.1f ms\n", tf1 - tf0, tf2 - tf1, tf3 - tf2, now_ms() - tf3);
    if (s && (route == ROUTE_BGZF || route == ROUTE_GZIP)) s->path_bits |= 16;      // (kvq_scan_path bit 4: the text was inflated on the device;
                                                                                    // bit 5, set by GzipProducer: a file took the speculative route)
    g_running = 0;
    if (s) s->t = t;          // the scan owns its table: destroyed with it (kvq_findseqs_free)
    else if (t) kvq_table_destroy(t);
    return s;
}

extern "C" kvq_scan *kvq_findseqs(const char *const *files, int32_t nfiles,
                                  const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq)
{
    return findseqs_impl(files, nfiles, seqs, seqlens, nseq, 0);
}

extern "C" kvq_scan *kvq_findseqs_ex(const char *const *files, int32_t nfiles,
                                     const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, uint32_t flags)
{
    kvq_find_opts o; memset(&o, 0, sizeof(o));
    o.size = (uint32_t)sizeof(o); o.flags = flags & ~(KVQ_FIND_PROFILE | KVQ_FIND_CYCLES);       // (the profile has cutoffs: kvq_findseqs_opts)
    // (... but for the per-read statistics, which need none: with them KVQ_FIND_PROFILE is a profile with no cutoffs)
    // (KVQ_FIND_ADAPTERS and KVQ_FIND_CLIP go through as they are: this structure has no room for probes, and the flags without them are "bad size")
    if ((flags & (KVQ_FIND_READ_STATS | KVQ_FIND_DUPLICATION | KVQ_FIND_OVERREPRESENTED | KVQ_FIND_ADAPTERS)) && (flags & KVQ_FIND_PROFILE)) o.flags = flags;
    return kvq_findseqs_opts(files, nfiles, seqs, seqlens, nseq, &o);
}

extern "C" kvq_scan *kvq_findseqs_opts(const char *const *files, int32_t nfiles,
                                       const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, const kvq_find_opts *opts)
{
    if (opts && opts->size < sizeof(kvq_find_opts)) { kvq_clear_error(); kvq_set_error(KVQ_ERR_RUNTIME, "kvq_findseqs_opts: bad size"); return nullptr; }
    return findseqs_impl(files, nfiles, seqs, seqlens, nseq, opts ? opts->flags : 0u, opts);
}

// destroy a scan returned by kvq_findseqs together with the table it created
extern "C" void kvq_findseqs_free(kvq_scan *s)
{
    if (!s) return;
    kvq_table *t = const_cast<kvq_table *>(s->t);
    {
        // kept for the next call with the same sequences and settings (one pair; KVQ_KEEP_SCAN=0: never)
        static const bool keep = !(getenv("KVQ_KEEP_SCAN") && getenv("KVQ_KEEP_SCAN")[0] == '0');
        std::lock_guard<std::mutex> l(g_kept_lock);
        if (keep && t && !g_kept.s && s->finished) { g_kept.t = t; g_kept.s = s; (void)hipGetDevice(&g_kept.dev); return; }
    }
    kvq_scan_destroy(s);
    kvq_table_destroy(t);
}

