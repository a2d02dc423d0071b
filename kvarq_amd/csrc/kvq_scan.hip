// kvarq_amd/csrc/kvq_scan.hip -- the scan object and the life of a batch: create / reset / destroy, the chain of the persistent kernels,
// run_batch (the kernels of one batch, in named steps), the one whole-batch redo, and the ways a batch comes in (device, host, staged)
#include "kvq_host.h"
#include "kvq_lines.h"
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string.h>

// after the kernels of one batch: merge the seed-filter kernel's staged counters and error
// into the scan's, or -- when its speculated record split failed validation -- forget
// everything the batch appended to the hit arena (the host rescans it exhaustively)
extern "C" __global__ void __launch_bounds__(256)
kvq_commit_batch(unsigned long long *stage, unsigned long long *ctr, unsigned long long *err_stage, unsigned long long *err,
                 const unsigned int *fail, unsigned int *arena_n, unsigned int *range)
{
    KVQ_BESIDE_SCAN();
    const bool bad = (*fail & 1u) != 0u;          // (the bits above count skipped tiles: kvq_validate_tiles)
    // (the scan kernel's workgroups add to one of KVQ_STAGE_COPIES copies of the staged counters -- a thousand atomics on
    // one word take 12 us at the end of every launch, an eighth of them a fraction of that: the copies are put together here)
    for (int i = threadIdx.x; i < KVQ_STAGE_SLOTS; i += blockDim.x) {
        unsigned long long v = 0;
        for (int c = 0; c < KVQ_STAGE_COPIES; c++) {
            const unsigned long long w = stage[(size_t)c * KVQ_STAGE_SLOTS + i];
            v = i == KVQ_CTR_LONGEST_ ? (v > w ? v : w) : v + w;
            stage[(size_t)c * KVQ_STAGE_SLOTS + i] = 0;
        }
        if (v && !bad) { if (i == KVQ_CTR_LONGEST_) atomicMax(&ctr[i], v); else atomicAdd(&ctr[i], v); }
    }
    if (threadIdx.x == 0) {
        if (bad) *arena_n = range[0];
        else if (*err_stage != ~0ull) atomicMin(err, *err_stage);
        *err_stage = ~0ull;
        range[1] = *arena_n;                       // the batch's hits end here
    }
}

// the scan's device state back to "nothing scanned" in one launch: the small words (err and the
// staged err to all ones), counters, coverage marks (all 8-byte words)
extern "C" __global__ void __launch_bounds__(256)
kvq_reset_state(unsigned long long *small, size_t small_words, unsigned long long *ctr, size_t ctr_words,
                unsigned long long *cov, size_t cov_words)
{
    KVQ_BESIDE_SCAN();
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < small_words; i += step) small[i] = (i == KvqSmall::ERR_WORD || i == KvqSmall::ERR_STAGE_WORD) ? ~0ull : 0ull;      // err, staged err
    for (size_t i = i0; i < ctr_words; i += step) ctr[i] = 0ull;
    for (size_t i = i0; i < cov_words; i += step) cov[i] = 0ull;
}

// ---- the records of the hits (kernels_records.hip) ------------------------------------------------------------------------
static KvqRecTable rec_table(const kvq_scan *s)
{
    KvqRecTable T;
    T.key = s->d_rkey.as<unsigned long long>(); T.off = s->d_roff.as<unsigned long long>(); T.len = s->d_rlen.as<unsigned int>();
    T.dir = s->d_rdir.as<unsigned int>(); T.ctr = s->d_rsmall.as<unsigned long long>();
    T.store = s->d_rstore.as<uint8_t>(); T.store_cap = s->rstore_cap; T.mask = s->rslots - 1u;
    return T;
}

// the table and the store empty, the table sized for the arena as it is now (it grows only between scans: the arena does)
static int records_prepare(kvq_scan *s)
{
    int rc;
    uint64_t slots = 1024; while (slots < 2ull * s->arena_cap) slots <<= 1;
    if (s->rstore_cap == 0) {
        // KVQ_RECORD_CAP=<bytes>: a smaller first store (the tests force the grow-and-rescan path with it)
        unsigned long long cap = 32ull << 20;
        if (const char *e = getenv("KVQ_RECORD_CAP")) { const long long v = atoll(e); if (v >= 0 && (unsigned long long)v < cap) cap = (unsigned long long)v; }
        if ((rc = s->d_rstore.ensure((size_t)std::max<unsigned long long>(cap, 256) + 64))) return rc;
        s->rstore_cap = cap;
    }
    if ((rc = s->d_rsmall.ensure(256))) return rc;
    if (slots > s->rslots) {
        if ((rc = s->d_rkey.ensure((size_t)slots * 8)) || (rc = s->d_roff.ensure((size_t)slots * 8)) ||
            (rc = s->d_rlen.ensure((size_t)slots * 4)) || (rc = s->d_rdir.ensure((size_t)slots * 4))) return rc;
        KVQ_HIP(hipMemsetAsync(s->d_rkey.p, 0, (size_t)slots * 8, s->stream));
        s->rslots = (uint32_t)slots;
    } else {
        hipLaunchKernelGGL(kvq_records_clear, dim3(256), dim3(256), 0, s->stream, rec_table(s));
    }
    KVQ_HIP(hipMemsetAsync(s->d_rsmall.p, 0, 256, s->stream));
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

static int reset_device_state(kvq_scan *s)
{
    hipLaunchKernelGGL(kvq_reset_state, dim3(256), dim3(256), 0, s->stream, (unsigned long long *)s->d_small.p, KvqSmall::BYTES / 8,
                       s->d_ctr, (size_t)s->t->ctr_len, s->d_covdiff.as<unsigned long long>(), (size_t)s->t->bases + (size_t)s->t->nseq + 1);
    KVQ_HIP(hipGetLastError());
    if (const int rc = passes_clear(s)) return rc;
    if (s->records_on) return records_prepare(s);
    return KVQ_OK;
}

static int ensure_arena(kvq_scan *s, uint64_t hits, uint64_t blob)
{
    if (hits > 0xFFFFFFF0ull) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    if (hits > s->arena_cap) {
        int rc = s->d_arena.ensure((size_t)hits * sizeof(KvqHit)); if (rc) return rc;
        s->arena_cap = (uint32_t)hits;
    }
    if (blob > s->blob_cap) {
        if (blob > 0xFFFFFFF0ull) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
        int rc = s->d_blob.ensure((size_t)blob); if (rc) return rc;
        s->blob_cap = blob;
    }
    return KVQ_OK;
}

static std::atomic<int> g_live_scans{0};
int kvq_live_scans() { return g_live_scans.load(); }

// everything a new scan object owns; on an error the caller destroys what there is
static int scan_init(kvq_scan *s, void *d_counters)
{
    int rc;
    const kvq_table *t = s->t;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { kvq_set_error(KVQ_ERR_DEVICE, "hipStreamCreate failed"); return KVQ_ERR_DEVICE; }
    if (d_counters) s->d_ctr = (unsigned long long *)d_counters;
    else {
        if ((rc = s->d_ctr_own.ensure((size_t)t->ctr_len * 8))) return rc;
        s->d_ctr = s->d_ctr_own.as<unsigned long long>();
    }
    if ((rc = s->d_small.ensure(KvqSmall::BYTES))) return rc;
    if ((rc = s->d_covdiff.ensure(((size_t)t->bases + (size_t)t->nseq + 1) * 8))) return rc;
    const KvqSmall small(s->d_small.p);
    s->d_arena_n = small.arena_n; s->d_blob_n = small.blob_n; s->d_err = small.err; s->d_err_stage = small.err_stage;
    s->d_range = small.range; s->d_fail = small.fail; s->d_stage_ctr = small.stage_ctr;
    {
        // KVQ_ARENA_CAP=<hits>, KVQ_BLOB_CAP=<bytes>: a smaller first arena / blob (the tests reach "exactly full", "one more" and the
        // grow-and-rescan paths at small shapes with them); never larger than the defaults, never below 64 hits / 256 bytes
        unsigned long long hits = 1u << 20, blob = 64ull << 20;
        if (const char *e = getenv("KVQ_ARENA_CAP")) { const long long v = atoll(e); if (v >= 0 && (unsigned long long)v < hits) hits = std::max<unsigned long long>((unsigned long long)v, 64); }
        if (const char *e = getenv("KVQ_BLOB_CAP")) { const long long v = atoll(e); if (v >= 0 && (unsigned long long)v < blob) blob = std::max<unsigned long long>((unsigned long long)v, 256); }
        if ((rc = ensure_arena(s, hits, blob))) return rc;
    }
    if ((rc = s->d_surv.ensure(KvqSurvivors::bytes()))) return rc;
    {
        // header: slots handed out, the list's size (KVQ_SURV_CAP=<slots> shrinks it for the tests: a full list costs speed, never results)
        unsigned int hdr[64] = { 0 };
        hdr[1] = KVQ_SURV_CAP;
        if (const char *e = getenv("KVQ_SURV_CAP")) { const long v = atol(e); if (v >= 0 && v < (long)KVQ_SURV_CAP) hdr[1] = (unsigned int)v; }
        s->surv_cap = hdr[1];
        KVQ_HIP(hipMemcpyAsync(s->d_surv.p, hdr, 256, hipMemcpyHostToDevice, s->stream));
        KVQ_HIP(hipStreamSynchronize(s->stream));
    }
    if ((rc = s->d_redo.ensure(KvqRedo::bytes()))) return rc;
    KVQ_HIP(hipMemsetAsync(s->d_redo.p, 0, 256, s->stream));      // (the block comes from the cache as it was left: the redo's two counts start at zero)
    s->pin_cap = (size_t)t->ctr_len * 8 + (4u << 20);
    {
        size_t c = 0;
        s->pin_small = (uint8_t *)pinned_take(KvqPinSmall::BYTES, &c); s->pin_small_cap = c;
        s->pin = (uint8_t *)pinned_take(s->pin_cap, &c);
        if (s->pin) s->pin_cap = c;
        if (!s->pin_small || !s->pin) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
        memset(s->pin_small, 0, KvqPinSmall::BYTES);
    }
    memset(s->pin, 0, s->pin_cap < (1u << 20) ? s->pin_cap : (1u << 20));
    s->res = kvq_result_layout(0, 0);
    s->pin_res = s->pin + kvq_ctr_bytes(t);
    if ((rc = reset_device_state(s))) return rc;
    s->h_ctr.assign((size_t)t->ctr_len, 0);
    return KVQ_OK;
}

extern "C" kvq_scan *kvq_scan_create(const kvq_table *t, void *d_counters)
{
    kvq_clear_error();
    kvq_scan *s = new kvq_scan();
    g_live_scans++;
    s->t = t;
    if (scan_init(s, d_counters) != KVQ_OK) { kvq_scan_destroy(s); return nullptr; }
    return s;
}

// The scan kernel is persistent and takes every wave slot and all of the LDS of every CU: two of them at once
// (scan objects on different streams, e.g. a caller that enqueues the next job while it collects the last one)
// only get in each other's way.  So the main kernels of a process form a chain: each waits for the one enqueued
// before it, whatever stream that was on.  Everything else of a scan (tables, validation, fold, ordering, copies)
// is left free to run beside the next scan's kernel.
static std::mutex g_chain_lock;
static hipEvent_t g_chain_done = nullptr;         // recorded behind the main kernel enqueued last
static const kvq_scan *g_chain_owner = nullptr;   // (the event is its: forgotten when that scan goes away)

// is a scan kernel of ANOTHER scan object of this process still on the device (enqueued or running)?
bool kvq_chain_busy(const kvq_scan *s)
{
    std::lock_guard<std::mutex> l(g_chain_lock);
    if (!g_chain_done || g_chain_owner == s) return false;
    const bool busy = hipEventQuery(g_chain_done) == hipErrorNotReady;
    (void)hipGetLastError();
    return busy;
}
int kvq_chain_wait(kvq_scan *s, bool *behind_a_running_scan)
{
    std::lock_guard<std::mutex> l(g_chain_lock);
    if (behind_a_running_scan) *behind_a_running_scan = false;
    if (g_chain_done && g_chain_owner != s) {
        // (is the scan in front still on the device?  Then the caller keeps several jobs in flight, and the one after this will
        // be enqueued behind this one in the same way: kvq_seeded_launch lets it start without waiting for this scan's survivors)
        if (behind_a_running_scan) { *behind_a_running_scan = hipEventQuery(g_chain_done) == hipErrorNotReady; (void)hipGetLastError(); }
        KVQ_HIP(hipStreamWaitEvent(s->stream, g_chain_done, 0));
    }
    return KVQ_OK;
}
int kvq_chain_publish(kvq_scan *s)
{
    if (!s->ev_chain) KVQ_HIP(hipEventCreateWithFlags(&s->ev_chain, hipEventDisableTiming));
    KVQ_HIP(hipEventRecord(s->ev_chain, s->stream));
    std::lock_guard<std::mutex> l(g_chain_lock);
    g_chain_done = s->ev_chain; g_chain_owner = s;
    return KVQ_OK;
}
static void chain_forget(const kvq_scan *s)
{
    std::lock_guard<std::mutex> l(g_chain_lock);
    if (g_chain_owner == s) { g_chain_done = nullptr; g_chain_owner = nullptr; }
}

// timing events are kept for the next scan of the same handle (creating a pair costs several microseconds)
static void drop_events(kvq_scan *s, bool destroy = false)
{
    auto keep = [s](std::vector<KvqEventPair> &v) { s->ev_free.insert(s->ev_free.end(), v.begin(), v.end()); v.clear(); };
    keep(s->ev_all); keep(s->ev_main);
    for (KvqPass &p : s->passes) keep(p.ev);
    if (destroy) {
        chain_forget(s);
        for (auto &e : s->ev_free) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
        s->ev_free.clear();
    }
}

extern "C" void kvq_scan_destroy(kvq_scan *s)
{
    if (!s) return;
    g_live_scans--;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    drop_events(s, true);
    s->d_ctr_own.release();
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    if (s->pin) pinned_give(s->pin, s->pin_cap);
    if (s->pin_small) pinned_give(s->pin_small, s->pin_small_cap);
    for (int i = 0; i < 2; i++) if (s->ev_copy[i]) (void)hipEventDestroy(s->ev_copy[i]);
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    if (s->ev_chain) (void)hipEventDestroy(s->ev_chain);
    if (s->pin_rec) pinned_give(s->pin_rec, s->pin_rec_cap);
    for (KvqPass &p : s->passes) { if (p.pin) pinned_give(p.pin, p.pin_cap); p.d.release(); }
    if (s->emit_pin) pinned_give(s->emit_pin, s->emit_pin_cap);
    for (hipEvent_t e : s->emit_ev) if (e) (void)hipEventDestroy(e);
    deflate_off(s);
    DevBuf *bufs[] = { &s->d_emit_rec, &s->d_emit_off, &s->d_emit_bsum, &s->d_emit_store, &s->d_dup, &s->d_rkey, &s->d_roff, &s->d_rlen, &s->d_rdir, &s->d_rstore, &s->d_rsmall, &s->d_rres, &s->d_surv, &s->d_redo, &s->d_ctr_all, &s->d_gather_cnt, &s->d_gather_res, &s->d_sort_tmp, &s->d_sorted, &s->d_result, &s->d_order, &s->d_finish, &s->d_covdiff, &s->d_seg_base, &s->d_seg_cnt, &s->d_chunk_nrec, &s->d_rec_base, &s->d_nl4,
                       &s->d_rec_start, &s->d_read_off, &s->d_read_len, &s->d_arena, &s->d_blob, &s->d_small, &s->d_stage, &s->d_stage_b };
    for (DevBuf *b : bufs) b->release();
    s->pool.release();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

extern "C" int32_t kvq_scan_path(const kvq_scan *s) { return s->path_bits; }
extern "C" void kvq_scan_force_exhaustive(kvq_scan *s, int32_t on) { s->force_exhaustive = on != 0; }

int scan_idle(const kvq_scan *s, const char *who)
{
    if (s->batches.empty() && !s->copied_pending && s->host_pending < 0) return KVQ_OK;
    kvq_set_error(KVQ_ERR_RUNTIME, "%s: only before the first batch or after kvq_scan_reset", who);
    return KVQ_ERR_RUNTIME;
}

extern "C" int32_t kvq_scan_set_records(kvq_scan *s, int32_t on)
{
    kvq_clear_error();
    if (const int rc = scan_idle(s, "kvq_scan_set_records")) return rc;
    if (on && s->comm) {
        kvq_set_error(KVQ_ERR_RUNTIME, "records are not gathered across ranks: a scan with a communicator cannot keep them");
        return KVQ_ERR_RUNTIME;
    }
    const bool was = s->records_on;
    s->records_on = on != 0;
    s->rec_store_bytes = 0;
    return s->records_on && !was ? records_prepare(s) : KVQ_OK;
}
extern "C" int32_t kvq_scan_set_long_reads(kvq_scan *s, int32_t mode)
{
    kvq_clear_error();
    if (const int rc = scan_idle(s, "kvq_scan_set_long_reads")) return rc;
    if (mode < 0 || mode > 2) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_long_reads: mode must be 0 (off), 1 (on) or 2 (auto)"); return KVQ_ERR_RUNTIME; }
    s->long_mode = mode;
    return KVQ_OK;
}
extern "C" int32_t kvq_scan_reset(kvq_scan *s)
{
    kvq_clear_error();
    const double tr0 = now_ms();
    KVQ_HIP(hipStreamSynchronize(s->stream));
    drop_events(s);
    if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
    s->batches.clear(); s->host_batches = false; s->host_pending = -1; s->copied_pending = false; s->parsed = 0; s->total = 0;
    s->ms_all = s->ms_main = 0; for (KvqPass &p : s->passes) p.ms = 0;
    s->main_launches = 0; s->finished = false; s->reduced = false; s->gathered = false; s->path_bits = 0; s->kernel_cell = 0; s->kernel_grid = 0; s->n_hits = 0;
    for (int64_t &w : s->launch_info) w = 0;
    s->tail_pending = false;
    s->kept_tiles.clear(); s->kept_redo.clear();
    s->pool.used = 0;
    const int rr = reset_device_state(s);
    if (g_timing) fprintf(stderr, "reset host %.3f ms\n", now_ms() - tr0);
    return rr;
}

static KvqParams make_params(const kvq_scan *s)
{
    const kvq_table *t = s->t;
    KvqParams P;
    P.maxerrors = t->cfg.maxerrors; P.minoverlap = t->cfg.minoverlap; P.minreadlength = t->cfg.minreadlength;
    P.amin = (int32_t)t->cfg.Amin; P.nseq = t->nseq;
    P.tab = t->d_tab.as<uint8_t>(); P.tab_off = t->d_off.as<int32_t>();
    P.ctr = s->d_ctr; P.covdiff = s->d_covdiff.as<unsigned long long>();
    P.off_nseqhits = t->off_nseqhits; P.off_nseqbasehits = t->off_nseqbasehits; P.off_cov = t->off_cov; P.off_mut = t->off_mut;
    P.arena = s->d_arena.as<KvqHit>(); P.arena_cap = s->arena_cap; P.arena_n = s->d_arena_n;
    P.blob = s->d_blob.as<uint8_t>(); P.blob_cap = s->blob_cap; P.blob_n = s->d_blob_n;
    P.err = s->d_err;
    return P;
}

static int new_event_pair(kvq_scan *s, std::vector<std::pair<hipEvent_t, hipEvent_t>> &v)
{
    if (!s->ev_free.empty()) { v.push_back(s->ev_free.back()); s->ev_free.pop_back(); return KVQ_OK; }
    hipEvent_t a, b;
    KVQ_HIP(hipEventCreate(&a)); KVQ_HIP(hipEventCreate(&b));
    v.emplace_back(a, b);
    return KVQ_OK;
}

// what the steps of run_batch share: the batch, how it is scanned, and its chunk table in the pool (chunk_table)
struct BatchRun {
    const uint8_t *d_data; int64_t nbytes, nchunks, fpos_base; size_t batch_no;
    bool read_list = false;          // the read-list route: the exhaustive pass's index and trim, then kvq_seed_list for the seeded sequences (no tiles, nothing staged)
    bool use_seeded;                 // the seed-filter kernel takes the sequences it serves; the exhaustive kernels the rest (else: all)
    KvqParams P;
    const uint32_t *d_co;            // the chunk offsets in the device half of the pool
    std::vector<uint32_t> sb;        // the first segment (KVQ_SEG_BYTES) of every chunk; sb[nchunks]: segments of the batch
    uint32_t maxseg, maxchunk;       // the most segments / bytes a chunk has
    int64_t nrec = -1;               // records of the batch, once index_records has run for it (exhaustive_pass; the profile)
};

// chunk table: written into the pinned half of the pool, copied to its device half (async)
static int chunk_table(kvq_scan *s, BatchRun &B, const int64_t *chunk_off)
{
    int rc;
    const int64_t nchunks = B.nchunks;
    // (room for everything this batch puts into the pool -- chunk offsets here; first tiles, parameter
    // block, tile table and tile reports in kvq_seeded_launch, whose tiles own at least kvq_min_tile() bytes --
    // is made in one go: the pool must not move between the two)
    const size_t tiles_bound = (size_t)(B.nbytes / kvq_min_tile()) + (size_t)nchunks + 2;
    if ((rc = s->pool.reserve(((size_t)nchunks + 1) * 8 + tiles_bound * 24 + 65536, s->stream))) return rc;
    const size_t co_at = s->pool.take(((size_t)nchunks + 1) * 4);
    s->cur_co_at = co_at;
    uint32_t *co = reinterpret_cast<uint32_t *>(s->pool.h + co_at);
    B.d_co = reinterpret_cast<const uint32_t *>(s->pool.d + co_at);
    B.sb.resize((size_t)nchunks + 1);
    B.maxseg = B.maxchunk = 0; uint64_t segs = 0;
    for (int64_t c = 0; c <= nchunks; c++) co[c] = (uint32_t)chunk_off[c];      // (in range and ascending: check_batch)
    for (int64_t c = 0; c < nchunks; c++) {
        const uint32_t a = co[c], b = co[c + 1];
        const uint32_t n = b > a ? (uint32_t)(((uint64_t)b - (a & ~15u) + KVQ_SEG_BYTES - 1) / KVQ_SEG_BYTES) : 0u;
        B.sb[c] = (uint32_t)segs; segs += n;
        B.maxseg = std::max(B.maxseg, n); B.maxchunk = std::max(B.maxchunk, b - a);
    }
    B.sb[nchunks] = (uint32_t)segs;
    // (the seed-filter launch copies the chunk offsets together with its own tables: one transfer)
    if (!B.use_seeded) KVQ_HIP(hipMemcpyAsync(s->pool.d + co_at, co, ((size_t)nchunks + 1) * 4, hipMemcpyHostToDevice, s->stream));
    return KVQ_OK;
}

// The exact record index of a batch, from its newline counts: nl4 / rec_start of every complete record of every chunk (d_nl4,
// d_rec_start), B.nrec of them.  It needs one host round trip (records per chunk) to size its arrays.  Its users: the
// exhaustive pass and the profile (which takes the exhaustive pass's index where a batch has one).
static int index_records(kvq_scan *s, BatchRun &B)
{
    int rc;
    const uint8_t *d_data = B.d_data; const int64_t nchunks = B.nchunks; const uint32_t *d_co = B.d_co; const uint64_t segs = B.sb[nchunks];
    if ((rc = s->d_seg_base.ensure(B.sb.size() * 4)) || (rc = s->d_seg_cnt.ensure((size_t)(segs + 1) * 4)) ||
        (rc = s->d_chunk_nrec.ensure((size_t)(nchunks + 1) * 4)) || (rc = s->d_rec_base.ensure((size_t)(nchunks + 1) * 4))) return rc;
    KVQ_HIP(hipMemcpyAsync(s->d_seg_base.p, B.sb.data(), B.sb.size() * 4, hipMemcpyHostToDevice, s->stream));
    const uint32_t gx = std::max(1u, std::min(65u, (B.maxseg + 3) / 4));
    for (int64_t c0 = 0; c0 < nchunks; c0 += 32768) {
        const uint32_t ny = (uint32_t)std::min<int64_t>(32768, nchunks - c0);
        hipLaunchKernelGGL(kvq_count_lines, dim3(gx, ny), dim3(256), 0, s->stream, d_data,
                           d_co + c0, s->d_seg_base.as<uint32_t>() + c0, s->d_seg_cnt.as<uint32_t>());
    }
    hipLaunchKernelGGL(kvq_scan_segments, dim3((uint32_t)((nchunks + 3) / 4)), dim3(256), 0, s->stream, (uint32_t)nchunks,
                       s->d_seg_base.as<uint32_t>(), s->d_seg_cnt.as<uint32_t>(), s->d_chunk_nrec.as<uint32_t>());
    std::vector<uint32_t> nrec((size_t)nchunks), rbase((size_t)nchunks + 1);
    KVQ_HIP(hipMemcpyAsync(nrec.data(), s->d_chunk_nrec.p, (size_t)nchunks * 4, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    uint64_t R = 0;
    for (int64_t c = 0; c < nchunks; c++) { rbase[c] = (uint32_t)R; R += nrec[c]; }
    rbase[nchunks] = (uint32_t)R;
    B.nrec = (int64_t)R;
    if (R == 0) return KVQ_OK;
    if ((rc = s->d_nl4.ensure((size_t)R * 16)) || (rc = s->d_rec_start.ensure((size_t)R * 4))) return rc;
    KVQ_HIP(hipMemcpyAsync(s->d_rec_base.p, rbase.data(), rbase.size() * 4, hipMemcpyHostToDevice, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    for (int64_t c0 = 0; c0 < nchunks; c0 += 32768) {
        const uint32_t ny = (uint32_t)std::min<int64_t>(32768, nchunks - c0);
        hipLaunchKernelGGL(kvq_index_records, dim3(gx, ny), dim3(256), 0, s->stream, d_data,
                           d_co + c0, s->d_seg_base.as<uint32_t>() + c0, s->d_seg_cnt.as<uint32_t>(),
                           s->d_chunk_nrec.as<uint32_t>() + c0, s->d_rec_base.as<uint32_t>() + c0,
                           s->d_nl4.as<uint32_t>(), s->d_rec_start.as<uint32_t>());
    }
    return KVQ_OK;
}

// The adapter clip (kvq_scan_set_clip), in front of everything that reads the batch's scores: the exact index --
// which the exhaustive pass and the profile then take as it is --, and kvq_clip_records over it, which WRITES the batch's text
// where it lies.  Every first run of a batch, a replay after an arena overflow among them (the array has been cleared with the
// arena: the records are counted anew, and masking a masked text changes nothing); the exhaustive redo of a failed batch leaves it
// alone -- its text is masked and its records are counted.
static int clip_text(kvq_scan *s, BatchRun &B)
{
    int rc;
    // (a seed-filter batch copies its chunk offsets together with its tables, behind this step: the index wants them now)
    if (B.use_seeded) KVQ_HIP(hipMemcpyAsync(s->pool.d + s->cur_co_at, s->pool.h + s->cur_co_at, ((size_t)B.nchunks + 1) * 4, hipMemcpyHostToDevice, s->stream));
    if ((rc = index_records(s, B))) return rc;
    KvqPass &p = s->passes[KVQ_PASS_CLIP];
    if (B.nrec <= 0) return KVQ_OK;
    if ((rc = new_event_pair(s, p.ev))) return rc;
    KVQ_HIP(hipEventRecord(p.ev.back().first, s->stream));
    if ((rc = clip_enqueue(s, const_cast<uint8_t *>(B.d_data), (uint64_t)B.nrec))) return rc;
    KVQ_HIP(hipEventRecord(p.ev.back().second, s->stream));
    return KVQ_OK;
}

// The exhaustive pass over every record of the batch, for the n_exh sequences of d_exh (none: only the records are counted,
// when no seed-filter launch has done it).
static int exhaustive_pass(kvq_scan *s, BatchRun &B, const int32_t *d_exh, int32_t n_exh, bool hist_done)
{
    int rc;
    const uint8_t *d_data = B.d_data;
    if (n_exh > 0) s->path_bits |= 2;
    if (B.nrec < 0 && (rc = index_records(s, B))) return rc;      // (clip_text has made the index of a batch it masked)
    const uint64_t R = (uint64_t)B.nrec;
    if (R == 0) return KVQ_OK;
    if ((rc = s->d_read_off.ensure((size_t)R * 4)) || (rc = s->d_read_len.ensure((size_t)R * 4))) return rc;
    const uint32_t per_block = 4 * KVQ_TRIM_RPW;
    hipLaunchKernelGGL(kvq_trim_records, dim3((uint32_t)((R + per_block - 1) / per_block)), dim3(256), 0, s->stream, B.P, d_data,
                       B.fpos_base, (uint32_t)R, KvqDevCount{ nullptr, 0, 0, nullptr }, s->d_nl4.as<uint32_t>(), s->d_rec_start.as<uint32_t>(),
                       s->d_read_off.as<uint32_t>(), s->d_read_len.as<int32_t>(), hist_done ? 0 : 1, (uint32_t)KVQ_TRIM_RPW, (unsigned int *)nullptr, 0u);
    if (n_exh > 0) {
        const bool main_here = !B.use_seeded && !B.read_list;     // (the read-list route's main kernel is kvq_seed_list)
        if (main_here) { if ((rc = new_event_pair(s, s->ev_main))) return rc; KVQ_HIP(hipEventRecord(s->ev_main.back().first, s->stream)); }
        hipLaunchKernelGGL(kvq_match_all, dim3((uint32_t)((R + 3) / 4)), dim3(256), 0, s->stream, B.P, d_data, B.fpos_base, (uint32_t)R, KvqDevCount{ nullptr, 0, 0, nullptr },
                           s->d_read_off.as<uint32_t>(), s->d_read_len.as<int32_t>(), d_exh, n_exh);
        if (main_here) { KVQ_HIP(hipEventRecord(s->ev_main.back().second, s->stream)); s->main_launches++; }
    }
    return KVQ_OK;
}

// The records of tiles that the fused scan skipped (a record longer than the tile's look-ahead, more newlines than a
// tile's tables hold) go through the exhaustive kernels for the seeded sequences -- found again from the exact newline
// counts (kvq_collect_skipped walks them from what kvq_validate_tiles wrote for each such tile), trimmed, matched --
// right behind every seed-filter launch, WITHOUT the host looking: the kernels are launched with fixed grids, read
// the number of tiles and of records from device memory and return at once when there are none (the usual case: three
// empty launches).  A batch that failed validation is left alone (it is redone as a whole), and so is one whose
// skipped tiles hold more records than KVQ_REDO_CAP (kvq_dev_count raises its fail bit).  Their hits lie in the
// batch's own range of the arena, closed by close_batch.
static void redo_skipped_tiles(kvq_scan *s, const BatchRun &B)
{
    const uint8_t *d_data = B.d_data; const int64_t fpos_base = B.fpos_base; const KvqParams &P = B.P;
    const KvqRedo Rd(s->d_redo.p);
    unsigned int *const failw = s->d_fail + B.batch_no;
    const KvqSkippedTile *tiles = reinterpret_cast<const KvqSkippedTile *>(s->pool.d + s->cur_skip_at);
    const KvqDevCount ntile{ failw, 8, KVQ_SKIP_CAP, failw }, nrec{ Rd.count, 0, KVQ_REDO_CAP - KVQ_LONG_CAP, failw }, nlong{ Rd.count + 1, 0, 0xFFFFFFFFu, failw };
    hipLaunchKernelGGL(kvq_collect_skipped, dim3(16), dim3(256), 0, s->stream, d_data, tiles, 0u, ntile, Rd.nl4, Rd.rec_start, Rd.count, KVQ_REDO_CAP - KVQ_LONG_CAP);
    // (few records, some of them very long: a wave per record for the trim; the matcher shares a record's sequences and
    // alignments out over many waves)
    hipLaunchKernelGGL(kvq_trim_records, dim3(32), dim3(256), 0, s->stream, P, d_data, fpos_base, 0u, nrec, Rd.nl4, Rd.rec_start, Rd.read_off, Rd.read_len, 1, 1u, Rd.count + 1, KVQ_REDO_CAP - 1u);
    // The matcher, twice: the ordinary reads a wave each (the sequences of a read shared out over a few workgroups), the
    // long ones -- a handful of reads of thousands of bases, which the trim has put on a list of their own -- spread out
    // over sequences and alignments.  Grids of a fixed, modest size (an empty launch of sixteen thousand workgroups costs
    // 50 us, one of a few hundred next to nothing; the kernels stride over what there is): small as long as this scan
    // object has never had a skipped tile.
    static const char *mg = getenv("KVQ_MGRID");           // (experiments: workgroups of the long reads' launch)
    const uint32_t lgrid = mg && atoi(mg) > 0 ? (uint32_t)atoi(mg) : 1536u;
    const dim3 ogrid = s->seen_skips ? dim3(128, (uint32_t)std::min<size_t>(s->t->seeded.size(), 4), 1) : dim3(16, (uint32_t)std::min<size_t>(s->t->seeded.size(), 4), 1);
    if (!s->t->seeded.empty()) {
        hipLaunchKernelGGL(kvq_match_all, ogrid, dim3(256), 0, s->stream, P, d_data, fpos_base, 0u, nrec,
                           Rd.read_off, Rd.read_len, s->t->d_seeded.as<int32_t>(), (int32_t)s->t->seeded.size());
        hipLaunchKernelGGL(kvq_match_long, dim3(s->seen_skips ? lgrid : 256u), dim3(256), 0, s->stream, P, d_data, fpos_base, nlong,
                           Rd.read_off, Rd.read_len, s->t->d_seeded.as<int32_t>(), (int32_t)s->t->seeded.size(), KVQ_REDO_CAP - 1u);
    }
}

// Does the batch take the read-list route (kvq_scan_set_long_reads)?  Only where it was asked for, the table has a seed index with seeded
// sequences and nothing forces the exhaustive kernels; in auto mode only when the batch's head says long reads: the average record among its
// first 128 KiB (kvq_tile_for_text) is at least a KVQ_LONG_READ read's (bases and scores of 1024 and the least the other two lines take) --
// or the head holds too few lines for an average, which only lines of many KiB do.  The head is looked at with variables of its own: the
// scan's tile geometry stays what its first batch made it.  Decided once per batch (a replayed batch goes the way it went).
static int decide_read_list(kvq_scan *s, Batch &b, const uint8_t *d_data, bool exhaustive_only, bool *take)
{
    const kvq_table *t = s->t;
    *take = false;
    if (exhaustive_only || !s->long_mode || !t->index || t->seeded.empty() || s->force_exhaustive) return KVQ_OK;
    if (b.read_list < 0) {
        b.read_list = 1;
        if (s->long_mode == 2) {
            std::vector<uint8_t> head((size_t)std::min<int64_t>(b.nbytes, 128 << 10));
            KVQ_HIP(hipMemcpyAsync(head.data(), d_data, head.size(), hipMemcpyDeviceToHost, s->stream));
            KVQ_HIP(hipStreamSynchronize(s->stream));
            uint32_t rec = 0;
            (void)kvq_tile_for_text(head.data(), head.size(), &rec);
            b.read_list = rec >= 2u * KVQ_MAX_READLENGTH + 25u || (rec == 0 && head.size() == (size_t)(128 << 10)) ? 1 : 0;
        }
    }
    *take = b.read_list == 1;
    return KVQ_OK;
}

// closing the batch: hits of this batch = arena[range[batch_no], range[batch_no + 1]) (kvq_commit_batch closes the range of a
// seed-filter batch and merges or forgets what it staged); then the fold of its hits and, when asked for, their records
static int close_batch(kvq_scan *s, const BatchRun &B)
{
    unsigned int *const range = s->d_range + B.batch_no;
    if (B.use_seeded)
        hipLaunchKernelGGL(kvq_commit_batch, dim3(1), dim3(256), 0, s->stream, s->d_stage_ctr, s->d_ctr, s->d_err_stage, s->d_err,
                           (const unsigned int *)(s->d_fail + B.batch_no), s->d_arena_n, range);
    else
        KVQ_HIP(hipMemcpyAsync(range + 1, s->d_arena_n, 4, hipMemcpyDeviceToDevice, s->stream));
    hipLaunchKernelGGL(kvq_fold_batch, dim3(512), dim3(256), 0, s->stream, B.P, B.d_data, B.fpos_base,
                       (const unsigned int *)range, (const unsigned int *)(range + 1));
    if (s->records_on)
        hipLaunchKernelGGL(kvq_gather_records, dim3(512), dim3(256), 0, s->stream, rec_table(s), (const KvqHit *)B.P.arena, B.P.arena_cap, B.d_data,
                           B.nbytes, B.fpos_base, B.d_co, (uint32_t)B.nchunks, (const unsigned int *)range, (const unsigned int *)(range + 1));
    return KVQ_OK;
}

// Enqueue every kernel of batch `batch_no` of the scan's list, whose text lies at d_data (check_batch has passed it).  exhaustive_only: the
// redo of a batch whose speculated record split failed.  The seed-filter launch is left inline: one call and the bookkeeping around it.
static int run_batch(kvq_scan *s, size_t batch_no, const uint8_t *d_data, bool exhaustive_only)
{
    const kvq_table *t = s->t;
    const double tb0 = now_ms();
    Batch &b = s->batches[batch_no];               // (no step touches the list)
    BatchRun B;
    B.d_data = d_data; B.nbytes = b.nbytes; B.nchunks = (int64_t)b.chunk_off.size() - 1; B.fpos_base = b.fpos_base; B.batch_no = batch_no;
    if (B.nbytes <= 0 || B.nchunks <= 0) return KVQ_OK;
    B.P = make_params(s);
    int rc;
    if ((rc = decide_read_list(s, b, d_data, exhaustive_only, &B.read_list))) return rc;
    B.use_seeded = t->index && !t->seeded.empty() && !s->force_exhaustive && !exhaustive_only && !B.read_list;
    s->cur_chunk_off = b.chunk_off;
    const bool split = B.use_seeded || B.read_list;        // the seeded sequences have a kernel of their own: the exhaustive kernels take the rest
    const int32_t *d_exh = split ? t->d_exh.as<int32_t>() : t->d_all.as<int32_t>();
    const int32_t n_exh = split ? (int32_t)t->exhaustive.size() : t->nseq;

    if ((rc = chunk_table(s, B, b.chunk_off.data()))) return rc;
    if ((rc = new_event_pair(s, s->ev_all))) return rc;
    KVQ_HIP(hipEventRecord(s->ev_all.back().first, s->stream));
    if (s->clip.n && !exhaustive_only && (rc = clip_text(s, B))) return rc;

    if (B.use_seeded) {
        if ((rc = new_event_pair(s, s->ev_main))) return rc;
        KvqParams PS = B.P;                        // counters and error of this batch are staged until it is validated (the pair of events is recorded right around the scan kernel: kvq_seeded_launch)
        PS.ctr = s->d_stage_ctr; PS.err = s->d_err_stage;
        s->cur_fail = s->d_fail + batch_no;
        if ((rc = kvq_seeded_launch(s, PS, d_data, B.nbytes, B.d_co, B.nchunks, B.fpos_base, B.maxchunk))) return rc;
        s->main_launches++; s->path_bits |= 1;
    }
    if ((!B.use_seeded || n_exh > 0) && (rc = exhaustive_pass(s, B, d_exh, n_exh, B.use_seeded))) return rc;
    if (B.read_list) {
        // the reads the exhaustive pass has indexed and trimmed (and counted), through the seed filter for the seeded sequences: counters
        // and err are written directly, as there -- nothing is speculated
        s->path_bits |= 128;
        if (B.nrec > 0) {
            const SeedIndex *ix = t->index;
            const uint32_t R = (uint32_t)B.nrec;
            if ((rc = new_event_pair(s, s->ev_main))) return rc;
            KVQ_HIP(hipEventRecord(s->ev_main.back().first, s->stream));
            hipLaunchKernelGGL(kvq_seed_list, dim3(std::min<uint32_t>((R + 3u) / 4u, KVQ_LIST_GRID_MAX)), dim3(256), 0, s->stream, B.P, d_data, B.fpos_base, R,
                               s->d_read_off.as<uint32_t>(), s->d_read_len.as<int32_t>(), t->d_seeded.as<int32_t>(), (int32_t)t->seeded.size(), ix->dev, (int32_t)ix->k);
            KVQ_HIP(hipEventRecord(s->ev_main.back().second, s->stream));
            s->main_launches++;
        }
    }
    if (B.use_seeded && s->cur_ntiles) redo_skipped_tiles(s, B);      // (a batch of empty chunks has scanned no tile: nothing was skipped, and the redo's counts are the LAST launch's)
    if ((rc = close_batch(s, B))) return rc;
    // the profile: every batch once, by its first pass (the redo of a batch that failed validation leaves it alone, and so does
    // the redo of skipped tiles), from the exact index -- the exhaustive pass's where the batch has one; a seeded batch waits
    // on the host once for its own.  In front of the closing event: what guards the batch's text guards this pass too
    // (the cycles, the per-read statistics, the overrepresented sequences and the adapter content are on only beside the profile: right behind it, from the same index)
    if (s->passes[KVQ_PASS_PROFILE].on && !exhaustive_only) {
        if (B.nrec < 0 && (rc = index_records(s, B))) return rc;
        for (int i = 0; i < KVQ_PASSES && B.nrec > 0; i++) {
            KvqPass &p = s->passes[i];
            if (!p.on || i == KVQ_PASS_CLIP || i == KVQ_PASS_EMIT) continue;     // (the clip has run in front of the scan: clip_text; the emit follows below, profile or not)
            if ((rc = new_event_pair(s, p.ev))) return rc;
            KVQ_HIP(hipEventRecord(p.ev.back().first, s->stream));
            switch (i) {
            case KVQ_PASS_PROFILE: rc = profile_enqueue(s, d_data, (uint64_t)B.nrec); break;
            case KVQ_PASS_CYCLES: rc = cycles_enqueue(s, d_data, (uint64_t)B.nrec); break;
            case KVQ_PASS_READS: rc = reads_enqueue(s, d_data, (uint64_t)B.nrec); break;
            case KVQ_PASS_OVER: rc = over_enqueue(s, d_data, (uint64_t)B.nrec); break;
            case KVQ_PASS_ADAPT: rc = adapt_enqueue(s, d_data, (uint64_t)B.nrec); break;
            }
            if (rc) return rc;
            KVQ_HIP(hipEventRecord(p.ev.back().second, s->stream));
        }
    }
    // the emit (kvq_scan_set_emit): every batch once, by its first pass, like the profile -- behind the scan and
    // behind clip_text, whose mask it reads, from the index the batch has (its own where nobody has made one); it needs no profile
    if (s->passes[KVQ_PASS_EMIT].on && !exhaustive_only) {
        if (B.nrec < 0 && (rc = index_records(s, B))) return rc;
        if (B.nrec > 0 && (rc = emit_enqueue(s, d_data, B.nbytes, (uint64_t)B.nrec))) return rc;
    }
    KVQ_HIP(hipEventRecord(s->ev_all.back().second, s->stream));
    KVQ_HIP(hipGetLastError());
    if (g_timing) fprintf(stderr, "run_batch host %.3f ms\n", now_ms() - tb0);
    return KVQ_OK;
}

// (measurement, kvq_scan_set_keep_skipped) host copies of what the batch's seed-filter launch left for the redo of its skipped tiles, taken
// while the pool still holds them: the descriptors kvq_validate_tiles wrote (fail >> 8 of them) and the entries kvq_collect_skipped
// put on the redo list (those the scan kernel put there itself, KVQ_REDO_TRIMMED, left out).  The batch's kernels are through.
static int keep_skipped_lists(kvq_scan *s, unsigned int fail)
{
    s->kept_tiles.clear(); s->kept_redo.clear();
    const size_t nt = std::min<size_t>(fail >> 8, KVQ_SKIP_CAP);
    if (!nt || !s->cur_ntiles) return KVQ_OK;
    const KvqRedo Rd(s->d_redo.p);
    unsigned int cnt = 0;
    s->kept_tiles.resize(nt * 6);
    KVQ_HIP(hipMemcpyAsync(s->kept_tiles.data(), s->pool.d + s->cur_skip_at, nt * sizeof(KvqSkippedTile), hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipMemcpyAsync(&cnt, Rd.count, 4, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    const size_t n = std::min<size_t>(cnt, KVQ_REDO_CAP - KVQ_LONG_CAP);
    if (!n) return KVQ_OK;
    std::vector<uint32_t> nl4(4 * n), rs(n);
    KVQ_HIP(hipMemcpyAsync(nl4.data(), Rd.nl4, n * 16, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipMemcpyAsync(rs.data(), Rd.rec_start, n * 4, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < n; i++) {
        if (rs[i] == KVQ_REDO_TRIMMED) continue;
        s->kept_redo.push_back(rs[i]);
        s->kept_redo.insert(s->kept_redo.end(), nl4.begin() + 4 * i, nl4.begin() + 4 * i + 4);
    }
    return KVQ_OK;
}
extern "C" int32_t kvq_scan_set_keep_skipped(kvq_scan *s, int32_t on)
{
    kvq_clear_error();
    if (const int rc = scan_idle(s, "kvq_scan_set_keep_skipped")) return rc;
    s->keep_skipped = on != 0;
    s->kept_tiles.clear(); s->kept_redo.clear();
    return KVQ_OK;
}
static int kept_lists_ready(const kvq_scan *s, const char *who)
{
    if (s->keep_skipped && s->finished) return KVQ_OK;
    kvq_set_error(KVQ_ERR_RUNTIME, "%s: only on a finished scan that kvq_scan_set_keep_skipped was turned on for", who);
    return KVQ_ERR_RUNTIME;
}
extern "C" int64_t kvq_scan_skipped_tiles(const kvq_scan *s, uint32_t *out, int64_t cap)
{
    kvq_clear_error();
    if (kept_lists_ready(s, "kvq_scan_skipped_tiles")) return -1;
    const int64_t n = (int64_t)(s->kept_tiles.size() / 6);
    if (out && cap > 0) memcpy(out, s->kept_tiles.data(), (size_t)std::min(n, cap) * 24);
    return n;
}
extern "C" int64_t kvq_scan_redo_list(const kvq_scan *s, uint32_t *nl4_out, uint32_t *rec_start_out, int64_t cap)
{
    kvq_clear_error();
    if (kept_lists_ready(s, "kvq_scan_redo_list")) return -1;
    const int64_t n = (int64_t)(s->kept_redo.size() / 5);
    for (int64_t i = 0; i < std::min(n, cap); i++) {
        if (rec_start_out) rec_start_out[i] = s->kept_redo[5 * (size_t)i];
        if (nl4_out) memcpy(nl4_out + 4 * i, &s->kept_redo[5 * (size_t)i + 1], 16);
    }
    return n;
}

// A batch's fail word, read once its kernels are through (the one place where it is read).  0: nothing.  Bit 0 clear: only some tiles were
// skipped, and their records have been through the exhaustive kernels behind the scan (redo_skipped_tiles).  Bit 0 set: the seed-filter pass
// failed validation (a tile's speculated record split disagreed with the newline count, one read flooded a wave's queues) and was rolled back
// on the device: the batch is scanned again as a whole, exhaustively, from `text`, as a batch of its own at the end of the list (*redone).
static int redo_if_failed(kvq_scan *s, size_t b, unsigned int fail, const uint8_t *text, bool *redone)
{
    *redone = false;
    if (s->keep_skipped) { if (const int rc = keep_skipped_lists(s, fail)) return rc; }
    if (!fail) return KVQ_OK;
    if (!(fail & 1u)) { s->path_bits |= 8 | 2; s->seen_skips = true; return KVQ_OK; }
    // (the redo's place on the list is the one batch number that check_batch has not seen: beyond the last range word there is no room for it)
    if (s->batches.size() >= KVQ_MAX_BATCHES) { kvq_set_error(KVQ_ERR_RUNTIME, "too many batches in one scan"); return KVQ_ERR_RUNTIME; }
    s->batches[b].redone = true;
    s->tile_bytes = kvq_choose_tile(1u << 20, 0); s->rec_bytes = 0;  // (a record may have outgrown the look-ahead: back to the full one)
    Batch again = s->batches[b]; again.is_redo = true;
    s->batches.push_back(again);
    s->path_bits |= 4;
    *redone = true;
    return run_batch(s, s->batches.size() - 1, text, true);
}

// what a batch must satisfy, found out before it is put on the scan's list (a listed batch must close its range
// of hits: one that was refused would leave a hole that the batches behind it fall into).  run_batch relies on it.
static int check_batch(const void *data, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, size_t batch_no, bool device)
{
    if (nbytes > 0xFFF00000ll) { kvq_set_error(KVQ_ERR_RUNTIME, "batch of %lld bytes is too large (< 4 GiB - 1 MiB)", (long long)nbytes); return KVQ_ERR_RUNTIME; }
    if (batch_no >= KVQ_MAX_BATCHES) { kvq_set_error(KVQ_ERR_RUNTIME, "too many batches in one scan"); return KVQ_ERR_RUNTIME; }
    if (device && ((uintptr_t)data & 15u) != 0) { kvq_set_error(KVQ_ERR_RUNTIME, "device buffer must be 16-byte aligned"); return KVQ_ERR_RUNTIME; }
    for (int64_t c = 0; c <= nchunks; c++)
        if (chunk_off[c] < 0 || chunk_off[c] > nbytes || (c && chunk_off[c] < chunk_off[c - 1])) {
            kvq_set_error(KVQ_ERR_RUNTIME, "bad chunk offsets"); return KVQ_ERR_RUNTIME;
        }
    return KVQ_OK;
}

// (measurement) the exact record index of a batch, as run_batch makes it -- check_batch, chunk_table, index_records, on the scan's
// stream -- brought to the host: the records per chunk, and the first `cap` records' nl4 (four words each) and rec_start.  Only on a
// scan that holds no batch; it leaves none behind, and no hit or counter.  Returns the records of the batch, -1 on an error.
extern "C" int64_t kvq_scan_index_device(kvq_scan *s, const void *d_text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                         uint32_t *nl4_out, uint32_t *rec_start_out, int64_t cap, uint32_t *chunk_nrec_out)
{
    kvq_clear_error();
    if (scan_idle(s, "kvq_scan_index_device")) return -1;
    if (nbytes <= 0 || nchunks <= 0) return 0;
    if (check_batch(d_text, nbytes, chunk_off, nchunks, 0, true)) return -1;
    BatchRun B;
    B.d_data = (const uint8_t *)d_text; B.nbytes = nbytes; B.nchunks = nchunks; B.fpos_base = 0; B.batch_no = 0; B.use_seeded = false;
    const size_t pool_used = s->pool.used;
    auto run = [&]() -> int {
        int rc;
        if ((rc = chunk_table(s, B, chunk_off)) || (rc = index_records(s, B))) return rc;
        const size_t n = (size_t)std::min<int64_t>(B.nrec, std::max<int64_t>(cap, 0));
        if (chunk_nrec_out) KVQ_HIP(hipMemcpyAsync(chunk_nrec_out, s->d_chunk_nrec.p, (size_t)nchunks * 4, hipMemcpyDeviceToHost, s->stream));
        if (n && nl4_out) KVQ_HIP(hipMemcpyAsync(nl4_out, s->d_nl4.p, n * 16, hipMemcpyDeviceToHost, s->stream));
        if (n && rec_start_out) KVQ_HIP(hipMemcpyAsync(rec_start_out, s->d_rec_start.p, n * 4, hipMemcpyDeviceToHost, s->stream));
        KVQ_HIP(hipStreamSynchronize(s->stream));
        KVQ_HIP(hipGetLastError());
        return KVQ_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(s->stream);
    s->pool.used = pool_used;                      // (the stream is idle: the chunk table's place in the pool is free again)
    return rc ? -1 : B.nrec;
}

extern "C" int32_t kvq_scan_device(kvq_scan *s, const void *d_data, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base)
{
    kvq_clear_error();
    if (nbytes <= 0 || nchunks <= 0) return KVQ_OK;                  // nothing to scan: not a batch
    int rc = check_batch(d_data, nbytes, chunk_off, nchunks, s->batches.size(), true); if (rc) return rc;
    Batch b; b.d_data = (const uint8_t *)d_data; b.nbytes = nbytes; b.fpos_base = fpos_base;
    b.chunk_off.assign(chunk_off, chunk_off + nchunks + 1);
    s->batches.push_back(b);
    s->parsed += nbytes; s->total += nbytes;
    return run_batch(s, s->batches.size() - 1, (const uint8_t *)d_data, false);
}

// Host batches.  kvq_scan_host_async(k) sends batch k's text across PCIe at once (copy stream, the staging buffer that is
// free) and enqueues the kernels of batch k - 1, whose text has arrived meanwhile, behind the settled batch k - 2: copies
// follow each other without a gap, kernels run beside them, and the host is back reading the next batch while both go on.
// Settling a batch = waiting for its kernels and looking at its fail word: when its seed-filter pass failed validation it is
// scanned again, exhaustively, while its text is still in its staging buffer.
static DevBuf &stage_of(kvq_scan *s, int slot) { return slot == 0 ? s->d_stage : s->d_stage_b; }

static int settle_in_flight(kvq_scan *s)
{
    KVQ_HIP(hipStreamSynchronize(s->stream));
    if (s->host_pending < 0) return KVQ_OK;
    const size_t b = (size_t)s->host_pending;
    s->host_pending = -1;
    if (!(s->path_bits & 1)) return KVQ_OK;
    const unsigned int fail = *KvqPinSmall(s->pin_small).cur_fail;     // copied behind the batch
    const uint8_t *text = s->batches[b].staged ? s->batches[b].staged : stage_of(s, s->run_slot).as<uint8_t>();
    bool redone = false;
    const int rc = redo_if_failed(s, b, fail, text, &redone);
    if (redone && !rc) KVQ_HIP(hipStreamSynchronize(s->stream));          // (the text is given back to its owner when this returns)
    return rc;
}

// enqueue the kernels of a host-side batch whose text lies at `text` and make it the batch in flight (the one before it
// has been settled: the table pool is free)
static int enqueue_host_batch(kvq_scan *s, const Batch &b, const uint8_t *text)
{
    unsigned int *const cur_fail = KvqPinSmall(s->pin_small).cur_fail;
    s->pool.used = 0;
    *cur_fail = 0;                                               // "speculation failed" of the batch about to be enqueued
    s->batches.push_back(b);
    const size_t batch_no = s->batches.size() - 1;
    const int rc = run_batch(s, batch_no, text, false);
    if (rc) return rc;
    if (s->path_bits & 1) KVQ_HIP(hipMemcpyAsync(cur_fail, s->d_fail + batch_no, 4, hipMemcpyDeviceToHost, s->stream));
    s->host_pending = (int64_t)batch_no;
    return KVQ_OK;
}

// the kernels of the batch whose text has been sent (the batch in flight has been settled)
static int launch_copied(kvq_scan *s)
{
    if (!s->copied_pending) return KVQ_OK;
    s->copied_pending = false;
    const int slot = s->copied_slot;
    KVQ_HIP(hipStreamWaitEvent(s->stream, s->ev_copy[slot], 0));
    s->run_slot = slot;
    return enqueue_host_batch(s, s->copied, stage_of(s, slot).as<uint8_t>());
}

// everything handed over so far is scanned and settled
extern "C" int32_t kvq_scan_host_drain(kvq_scan *s)
{
    int rc;
    if ((rc = settle_in_flight(s))) return rc;
    if ((rc = launch_copied(s))) return rc;
    return settle_in_flight(s);
}

// hand over one host batch and return; h_data must stay untouched until kvq_scan_host_copied(s) (or the next
// kvq_scan_host_async / kvq_scan_host_drain / kvq_scan_finish) has returned
extern "C" int32_t kvq_scan_host_async(kvq_scan *s, const void *h_data, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base)
{
    kvq_clear_error();
    if (nbytes <= 0 || nchunks <= 0) return KVQ_OK;
    int rc;
    if ((rc = check_batch(h_data, nbytes, chunk_off, nchunks, s->batches.size() + (s->copied_pending ? 1u : 0u), false))) return rc;
    if ((rc = settle_in_flight(s))) return rc;                     // the batch whose kernels ran while the caller read this one
    if ((rc = launch_copied(s))) return rc;                        // the batch handed over last call: its text has arrived meanwhile
    const int slot = s->run_slot == 0 ? 1 : 0;                     // (the buffer of the batch settled just now, or one never used)
    DevBuf &stage = stage_of(s, slot);
    if ((rc = stage.ensure((size_t)nbytes + 64))) return rc;
    if (!s->copy_stream) KVQ_HIP(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) if (!s->ev_copy[i]) KVQ_HIP(hipEventCreateWithFlags(&s->ev_copy[i], hipEventDisableTiming));
    if (s->tile_bytes == 0)                                      // size the seed-filter tiles from the head of the text
        s->tile_bytes = kvq_tile_for_text((const uint8_t *)h_data, (size_t)std::min<int64_t>(nbytes, 128 << 10), &s->rec_bytes);
    KVQ_HIP(hipMemcpyAsync(stage.p, h_data, (size_t)nbytes, hipMemcpyHostToDevice, s->copy_stream));
    KVQ_HIP(hipEventRecord(s->ev_copy[slot], s->copy_stream));
    s->copied = Batch(); s->copied.d_data = nullptr; s->copied.nbytes = nbytes; s->copied.fpos_base = fpos_base;
    s->copied.chunk_off.assign(chunk_off, chunk_off + nchunks + 1);
    s->copied_pending = true; s->copied_slot = slot;
    s->host_batches = true;
    s->parsed += nbytes; s->total += nbytes;
    // (a caller that alternates two host buffers writes next into the one of the call before: that text has left it)
    if (s->host_pending >= 0) KVQ_HIP(hipEventSynchronize(s->ev_copy[s->run_slot]));
    return KVQ_OK;
}

// a batch already in device memory that the caller reuses once the next batch is handed over (kvq_host.h)
int kvq_scan_staged(kvq_scan *s, const uint8_t *d_text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base)
{
    kvq_clear_error();
    if (nbytes <= 0 || nchunks <= 0) return KVQ_OK;
    int rc;
    if ((rc = check_batch(d_text, nbytes, chunk_off, nchunks, s->batches.size() + (s->copied_pending ? 1u : 0u), true))) return rc;
    if ((rc = settle_in_flight(s))) return rc;                     // (the batch before: its text is still where the caller put it)
    if ((rc = launch_copied(s))) return rc;
    if (s->tile_bytes == 0) {                                      // size the seed-filter tiles from the head of the text
        std::vector<uint8_t> head((size_t)std::min<int64_t>(nbytes, 128 << 10));
        KVQ_HIP(hipMemcpyAsync(head.data(), d_text, head.size(), hipMemcpyDeviceToHost, s->stream));
        KVQ_HIP(hipStreamSynchronize(s->stream));
        s->tile_bytes = kvq_tile_for_text(head.data(), head.size(), &s->rec_bytes);
    }
    Batch b; b.d_data = nullptr; b.staged = d_text; b.nbytes = nbytes; b.fpos_base = fpos_base;
    b.chunk_off.assign(chunk_off, chunk_off + nchunks + 1);
    s->host_batches = true;
    s->parsed += nbytes; s->total += nbytes;
    return enqueue_host_batch(s, b, d_text);
}

// wait until the text of the last kvq_scan_host_async batch has left the host buffer
extern "C" int32_t kvq_scan_host_copied(kvq_scan *s)
{
    if (s->copied_pending && s->ev_copy[s->copied_slot]) KVQ_HIP(hipEventSynchronize(s->ev_copy[s->copied_slot]));
    return KVQ_OK;
}

// the blocking form: h_data may be reused when the call returns
extern "C" int32_t kvq_scan_host(kvq_scan *s, const void *h_data, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base)
{
    const int rc = kvq_scan_host_async(s, h_data, nbytes, chunk_off, nchunks, fpos_base);
    return rc ? rc : kvq_scan_host_copied(s);
}
