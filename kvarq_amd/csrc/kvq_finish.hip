// kvarq_amd/csrc/kvq_finish.hip -- the end of a scan: the tail enqueued behind its kernels, the records of the hits, finish_once and its
// steps (redo of failed device batches, growth and rescan, fetch), the replay of device batches, the finish over ranks, the result accessors
#include "kvq_host.h"
#include <algorithm>
#include <string.h>

static_assert(sizeof(KvqFinishState) <= KvqPinSmall::STATE_BYTES && sizeof(KvqFinishState) % 4 == 0, "pin_small holds a KvqFinishState");

// the scan's eight small words, its per-batch "speculation failed" flags and what kvq_finish_plan and the
// ordering left (hit count, layout, "crowded") -> pinned host memory
extern "C" __global__ void __launch_bounds__(256)
kvq_publish_small(const unsigned int *__restrict__ small, const unsigned int *__restrict__ fail, unsigned int nbatches,
                  const unsigned int *__restrict__ state, unsigned int state_words,
                  unsigned int *host_small, unsigned int *host_fail, unsigned int *host_state)
{
    KVQ_BESIDE_SCAN();
    if (threadIdx.x < KvqSmall::PUBLISHED_WORDS) host_small[threadIdx.x] = small[threadIdx.x];
    for (unsigned int i = threadIdx.x; i < nbatches; i += blockDim.x) host_fail[i] = fail[i];
    for (unsigned int i = threadIdx.x; i < state_words; i += blockDim.x) host_state[i] = state[i];
    __threadfence_system();
}

// The tail of a scan -- coverage marks -> counters, the plan of the ordering, the ordering itself, the gather into the result arrays,
// the words the host needs, the copies -- enqueued behind the scan's kernels: nothing in it needs a number the host would first have
// to fetch.  finish_once waits for it ONCE; kvq_scan_finish_begin enqueues it ahead of time (a job whose batches are all fed), so that
// a caller with several jobs in flight finds it done when it comes to kvq_scan_finish -- otherwise the host sits out the ordering
// kernels of every small job before it enqueues the next one, and those kernels run beside another job's scan at a tenth of their speed.
// the records' part of the tail: the (offset, length) of every hit's record in canonical order, and copies of the record
// words, of as many of those as the last scan of this handle had and of as many store bytes (finish_records fetches the rest)
static int records_tail(kvq_scan *s, const KvqFinishState *d_st)
{
    int rc;
    const size_t hoff = kvq_align256((size_t)s->arena_cap * 8);
    if ((rc = s->d_rres.ensure(hoff + (size_t)s->arena_cap * 4 + 256))) return rc;
    long long *d_off = s->d_rres.as<long long>();
    int32_t *d_len = reinterpret_cast<int32_t *>(s->d_rres.as<uint8_t>() + hoff);
    hipLaunchKernelGGL(kvq_record_lookup, dim3(256), dim3(256), 0, s->stream, rec_table(s), d_st, (const uint8_t *)s->d_result.p, d_off, d_len);
    KVQ_HIP(hipGetLastError());
    s->rec_tail_n = s->rec_tail_b = 0;
    if (!s->pin_rec) return KVQ_OK;                  // (the first finish of this handle: fetched there)
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(s->rec_spec_n, s->rec_hcap), s->arena_cap);
    const uint64_t b = std::min<uint64_t>(std::min<uint64_t>(s->rec_spec_b, s->rec_scap), s->rstore_cap);
    const KvqPinRec H(s->pin_rec, s->rec_hcap);
    if (n) {
        KVQ_HIP(hipMemcpyAsync(H.off, d_off, n * 8, hipMemcpyDeviceToHost, s->stream));
        KVQ_HIP(hipMemcpyAsync(H.len, d_len, n * 4, hipMemcpyDeviceToHost, s->stream));
    }
    if (b) KVQ_HIP(hipMemcpyAsync(H.store, s->d_rstore.p, b, hipMemcpyDeviceToHost, s->stream));
    s->rec_tail_n = n; s->rec_tail_b = b;
    return KVQ_OK;
}

// What a buffer of `cap` bytes, of which an overflowing scan used `used`, is grown to for the rescan.  `used` undercounts
// when the hit arena overflowed too (hits that did not fit were never folded, nor their records gathered): scale it by them.
static uint64_t grown_for_rescan(uint64_t used, uint64_t n_hits, uint32_t arena_cap, uint64_t cap)
{
    uint64_t want = used;
    if (n_hits > arena_cap && arena_cap) want = (uint64_t)((double)used * ((double)n_hits / arena_cap) * 1.25) + (1 << 20);
    return std::max<uint64_t>(want + want / 8, cap);
}

// after the tail has been waited for: did the store hold the scan's records?  A store too small (or a table that went round)
// is grown to what the scan needed and the scan asked to go again, like an overflowing hit blob
static int records_check(kvq_scan *s, uint64_t n_hits, unsigned long long *used, bool *grow)
{
    *grow = false;
    unsigned long long w[4] = { 0, 0, 0, 0 };
    KVQ_HIP(hipMemcpyAsync(w, s->d_rsmall.p, 32, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    *used = w[0];
    if (w[0] <= s->rstore_cap && !w[2]) return KVQ_OK;
    const unsigned long long want = grown_for_rescan(w[0], n_hits, s->arena_cap, s->rstore_cap);
    if (want > 0xFFFFFFF0ull) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    int rc; if ((rc = s->d_rstore.ensure((size_t)want + 64))) return rc;
    s->rstore_cap = want;
    *grow = true;
    return KVQ_OK;
}

// the hits are in their final order: what the tail did not fetch of the record words and the store
static int records_fetch(kvq_scan *s, uint64_t n_hits, unsigned long long used)
{
    const size_t hoff = kvq_align256((size_t)s->arena_cap * 8);
    bool all = false;
    if (!s->pin_rec || n_hits > s->rec_hcap || used > s->rec_scap) {
        const uint64_t hc = std::max<uint64_t>(n_hits + n_hits / 4 + 4096, s->rec_hcap), sc = std::max<uint64_t>(used + used / 4 + (1 << 20), s->rec_scap);
        const size_t want = KvqPinRec::bytes(hc, sc);
        size_t got = 0; uint8_t *np = (uint8_t *)pinned_take(want, &got);
        if (!np) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
        if (s->pin_rec) pinned_give(s->pin_rec, s->pin_rec_cap);
        s->pin_rec = np; s->pin_rec_cap = got; s->rec_hcap = hc; s->rec_scap = sc;
        all = true;
    }
    const KvqPinRec H(s->pin_rec, s->rec_hcap);
    bool copied = false;
    if (n_hits && (all || n_hits > s->rec_tail_n)) {
        KVQ_HIP(hipMemcpyAsync(H.off, s->d_rres.p, n_hits * 8, hipMemcpyDeviceToHost, s->stream));
        KVQ_HIP(hipMemcpyAsync(H.len, s->d_rres.as<uint8_t>() + hoff, n_hits * 4, hipMemcpyDeviceToHost, s->stream));
        copied = true;
    }
    if (used && (all || used > s->rec_tail_b)) {
        KVQ_HIP(hipMemcpyAsync(H.store, s->d_rstore.p, used, hipMemcpyDeviceToHost, s->stream));
        copied = true;
    }
    if (copied) KVQ_HIP(hipStreamSynchronize(s->stream));
    s->rec_store_bytes = (int64_t)used;
    s->rec_spec_n = n_hits + n_hits / 8 + 4096; s->rec_spec_b = used + used / 8 + 65536;
    return KVQ_OK;
}

// KVQ_ORDER=mergesort: the comparison sort for every scan, not only for crowded buckets.  Asked once per tail (enqueue_tail), so
// that a process can switch between the two orderings from one finish to the next; finish_once goes by what its tail was given
static bool order_by_mergesort() { const char *e = getenv("KVQ_ORDER"); return e && !strcmp(e, "mergesort"); }

static int enqueue_tail(kvq_scan *s)
{
    int rc;
    const kvq_table *t = s->t;
    const size_t ctr_b = kvq_ctr_bytes(t);
    const KvqPinSmall H(s->pin_small);
    uint32_t nb_max = 256; while ((uint64_t)nb_max < 4ull * s->arena_cap && nb_max < KVQ_BUCKETS_MAX) nb_max <<= 1;
    const size_t order_b = kvq_order_scratch_zero_bytes(nb_max) + (size_t)s->arena_cap * 4;
    if (order_b > s->d_order.cap || nb_max != s->order_nb_max) {
        if ((rc = s->d_order.ensure(order_b))) return rc;
        KVQ_HIP(hipMemsetAsync(s->d_order.p, 0, kvq_order_scratch_zero_bytes(nb_max), s->stream));    // (kvq_order_clear leaves them zero again)
        s->order_nb_max = nb_max;
    }
    const KvqOrderScratch W = kvq_order_scratch(s->d_order.p, nb_max);
    if ((rc = s->d_finish.ensure(sizeof(KvqFinishState) + 256))) return rc;
    KvqFinishState *d_st = s->d_finish.as<KvqFinishState>();
    const size_t res_cap = kvq_result_layout(s->arena_cap, s->blob_cap).total + 256;
    if ((rc = s->d_result.ensure(res_cap))) return rc;
    // file positions of this scan lie in [lo, hi)
    int64_t lo = 0, hi = 1;
    for (size_t b = 0; b < s->batches.size(); b++) {
        const int64_t a = s->batches[b].fpos_base, e = a + s->batches[b].nbytes;
        if (b == 0 || a < lo) lo = a;
        if (b == 0 || e > hi) hi = e;
    }
    const size_t nb0 = s->batches.size();
    hipLaunchKernelGGL(kvq_finish_plan, dim3(1), dim3(64), 0, s->stream, (const unsigned int *)s->d_arena_n, s->arena_cap,
                       (const unsigned long long *)s->d_blob_n, (unsigned long long)s->blob_cap, (const unsigned long long *)s->d_err,
                       (long long)lo, (long long)hi, nb_max, d_st);
    if (t->nseq > 0)
        hipLaunchKernelGGL(kvq_cov_apply, dim3((uint32_t)((t->nseq + 3) / 4)), dim3(256), 0, s->stream, make_params(s));
    s->tail_mergesort = order_by_mergesort();
    if (!s->tail_mergesort &&
        (rc = kvq_order_by_buckets(s->stream, s->d_arena.as<KvqHit>(), s->d_blob.as<uint8_t>(), s->blob_cap, d_st, W, s->d_result.as<uint8_t>()))) return rc;
    if (s->records_on && (rc = records_tail(s, d_st))) return rc;
    if ((rc = passes_tail(s))) return rc;
    hipLaunchKernelGGL(kvq_publish_small, dim3(1), dim3(256), 0, s->stream, (const unsigned int *)s->d_small.p,
                       (const unsigned int *)s->d_fail, (unsigned int)nb0, (const unsigned int *)d_st, (unsigned int)(sizeof(KvqFinishState) / 4),
                       H.small, H.fail, H.state);
    KVQ_HIP(hipGetLastError());
    // results: as many bytes as the last scan of this handle had (a guess: what is missing is fetched by finish_once)
    size_t spec = std::min(s->spec_bytes, res_cap);
    if (ctr_b + spec > s->pin_cap) spec = s->pin_cap > ctr_b ? s->pin_cap - ctr_b : 0;
    KVQ_HIP(hipMemcpyAsync(s->pin, s->d_ctr, (size_t)t->ctr_len * 8, hipMemcpyDeviceToHost, s->stream));
    if (spec) KVQ_HIP(hipMemcpyAsync(s->pin + ctr_b, s->d_result.p, spec, hipMemcpyDeviceToHost, s->stream));
    s->tail_nb0 = nb0; s->tail_spec = spec; s->tail_pending = true;
    return KVQ_OK;
}

extern "C" int32_t kvq_scan_finish_begin(kvq_scan *s)
{
    kvq_clear_error();
    if (!s || s->finished) return KVQ_OK;
    // (a host batch in flight is settled first -- that waits for it; a scan of device batches is not waited for at all)
    if (s->host_pending >= 0 || s->copied_pending) { const int rc0 = kvq_scan_host_drain(s); if (rc0) return rc0; }
    return enqueue_tail(s);
}

// ---- the steps of finish_once ----
// device batches whose seed-filter pass failed validation: scan those again exhaustively (redo_if_failed; host batches were redone on
// the spot, when they were settled).  *any: the scan has to be finished again.
static int redo_failed_device_batches(kvq_scan *s, size_t nb0, bool *any)
{
    *any = false;
    if (!nb0 || !(s->path_bits & 1)) return KVQ_OK;
    const unsigned int *fail = KvqPinSmall(s->pin_small).fail;
    for (size_t b = 0; b < nb0; b++) {
        if (s->batches[b].redone || s->batches[b].is_redo || !s->batches[b].d_data) continue;
        bool redone = false;
        if (const int rc = redo_if_failed(s, b, fail[b], s->batches[b].d_data, &redone)) return rc;
        *any |= redone;
    }
    return KVQ_OK;
}

// first malformed record in stream order (workhorse.c:1037-1048)
static int format_error(unsigned long long err)
{
    const long fpos = (long)(err >> 16); const int kind = (int)((err >> 8) & 0xFF); const int ch = (int)(err & 0xFF);
    if (kind == 0) kvq_set_error(KVQ_ERR_FORMAT, "record must start with '@' (and not '%c') fpos=%ld", ch, fpos);
    else kvq_set_error(KVQ_ERR_FORMAT, "3rd line of record must start with '+' fpos=%ld", fpos);
    return KVQ_ERR_FORMAT;
}

// did the hit arena, the hit blob and the record store hold the scan?  What did not is grown to what this scan needs, and
// KVQ_NEED_RESCAN asks for the scan again.  *rec_used: bytes of the record store in use.
static int grow_or_go_on(kvq_scan *s, const KvqFinishState &st, unsigned long long *rec_used)
{
    int rc;
    bool rec_grow = false;
    *rec_used = 0;
    if (s->records_on && (rc = records_check(s, st.n_raw, rec_used, &rec_grow))) return rc;
    if (st.n_raw > s->arena_cap || st.blob_n > s->blob_cap) {
        const uint64_t want_hits = std::max<uint64_t>(st.n_raw + st.n_raw / 8 + 1024, s->arena_cap);
        if ((rc = ensure_arena(s, want_hits, grown_for_rescan(st.blob_n, st.n_raw, s->arena_cap, s->blob_cap)))) return rc;
        return KVQ_NEED_RESCAN;
    }
    return rec_grow ? KVQ_NEED_RESCAN : KVQ_OK;
}

// a larger landing buffer for `need` bytes: the counters, already there, move over; what the tail fetched of the results is lost
static int grow_landing(kvq_scan *s, size_t need, size_t ctr_b)
{
    const size_t want = need * 5 / 4 + (1 << 20);
    size_t got = 0; uint8_t *np = (uint8_t *)pinned_take(want, &got);
    if (!np) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    memcpy(np, s->pin, ctr_b);
    pinned_give(s->pin, s->pin_cap);
    s->pin = np; s->pin_cap = got;
    return KVQ_OK;
}

static void sum_timing(kvq_scan *s)
{
    auto sum = [](const std::vector<KvqEventPair> &v) {
        double total = 0;
        for (auto &e : v) { float ms = 0; if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) total += ms; }
        return total;
    };
    s->ms_all = sum(s->ev_all); s->ms_main = sum(s->ev_main);
    for (KvqPass &p : s->passes) p.ms = sum(p.ev);
    (void)hipGetLastError();                 // (a pair that was never recorded is not an error of the scan)
}

// wait for the tail ONCE, then: redo what failed (and go round again), report a format error, grow and ask for a rescan, or fetch what the
// tail did not bring and close the scan (the merge-sort fallback and the fetch stay inline: they share `refetch` and the layout)
static int finish_once(kvq_scan *s)
{
    const double t0 = now_ms();
    { const int rc0 = kvq_scan_host_drain(s); if (rc0) return rc0; }          // settle the host batch in flight
    int rc;
    const kvq_table *t = s->t;
    const size_t ctr_b = kvq_ctr_bytes(t);
    const KvqFinishState *h_st = reinterpret_cast<const KvqFinishState *>(KvqPinSmall(s->pin_small).state);

    for (int round = 0; round < 3; round++) {
        // (the tail may have been enqueued ahead of time, by kvq_scan_finish_begin, for exactly the batches there are)
        if (!(s->tail_pending && s->tail_nb0 == s->batches.size()) && (rc = enqueue_tail(s))) return rc;
        s->tail_pending = false;
        size_t spec = s->tail_spec;
        KvqFinishState *d_st = s->d_finish.as<KvqFinishState>();
        KVQ_HIP(hipStreamSynchronize(s->stream));
        const double t1 = now_ms();

        bool any = false;
        if ((rc = redo_failed_device_batches(s, s->tail_nb0, &any))) return rc;
        if (any) continue;
        const KvqFinishState st = *h_st;
        const uint32_t n_hits = st.n_raw;
        if (st.err != ~0ull) return format_error(st.err);
        unsigned long long rec_used = 0;
        if ((rc = grow_or_go_on(s, st, &rec_used))) return rc;
        const KvqResultLayout L = st.L;
        if (ctr_b + L.total > s->pin_cap) {
            if ((rc = grow_landing(s, ctr_b + L.total, ctr_b))) return rc;
            spec = 0;
        }
        bool refetch = L.total > spec;
        const bool by_mergesort = n_hits && (s->tail_mergesort || st.crowded);
        if (by_mergesort) {
            // crowded buckets (or the comparison sort asked for): order the hits with the merge sort instead
            if ((rc = kvq_order_by_mergesort(s->stream, s->d_arena.as<KvqHit>(), n_hits, s->d_blob.as<uint8_t>(), s->blob_cap, d_st,
                                             s->d_sort_tmp, s->d_sorted, s->d_result.as<uint8_t>()))) return rc;
            refetch = true;
            if (s->records_on && (rc = records_tail(s, d_st))) return rc;      // (the records follow the hits' new order: fetched again below)
            s->rec_tail_n = 0;
        }
        if (n_hits && refetch) {
            KVQ_HIP(hipMemcpyAsync(s->pin + ctr_b, s->d_result.p, L.total, hipMemcpyDeviceToHost, s->stream));
            KVQ_HIP(hipStreamSynchronize(s->stream));
        }
        if (s->records_on && (rc = records_fetch(s, n_hits, rec_used))) return rc;
        memcpy(s->h_ctr.data(), s->pin, (size_t)t->ctr_len * 8);
        if ((rc = passes_landed(s))) return rc;
        s->pin_res = s->pin + ctr_b;
        if (!n_hits) memset(s->pin_res + L.hitseq_off, 0, 8);
        s->res = L; s->n_hits = n_hits;
        { const int64_t info[7] = { (int64_t)st.n, (int64_t)st.nb, (int64_t)st.shift, (int64_t)st.bc, (int64_t)st.lo, (int64_t)st.crowded, by_mergesort ? 1 : 0 };
          memcpy(s->order_info, info, sizeof(info)); }
        s->spec_bytes = L.total + L.total / 8 + 65536;
        sum_timing(s);
        s->finished = true;
        if (g_timing) {
            unsigned int rc2[2] = { 0, 0 };
            if (s->d_redo.p) (void)hipMemcpy(rc2, s->d_redo.p, 8, hipMemcpyDeviceToHost);
            fprintf(stderr, "finish: enqueue + wait %.3f  rest %.3f ms (%u hits; the last launch's skipped tiles left %u records, %u of them long)\n", t1 - t0, now_ms() - t1, n_hits, rc2[0], rc2[1]);
        }
        return KVQ_OK;
    }
    kvq_set_error(KVQ_ERR_RUNTIME, "a redone batch failed validation again");
    return KVQ_ERR_RUNTIME;
}

// returns KVQ_OK, an error code, or KVQ_NEED_RESCAN when host batches must be fed again
int kvq_scan_finish_internal(kvq_scan *s)
{
    for (int attempt = 0; attempt < 4; attempt++) {
        int rc = finish_once(s);
        if (rc != KVQ_NEED_RESCAN) return rc;
        if (s->host_batches) return KVQ_NEED_RESCAN;
        // device batches are still resident: replay them into the larger arena
        std::vector<Batch> again; again.swap(s->batches);
        drop_events(s); s->main_launches = 0; s->path_bits = 0; s->tail_pending = false;
        if ((rc = reset_device_state(s))) return rc;
        s->pool.used = 0;
        for (size_t b = 0; b < again.size(); b++) {
            if (again[b].is_redo) continue;            // the exhaustive redo of a failed batch: its original is replayed and judged afresh
            Batch nb = again[b]; nb.redone = false;
            s->batches.push_back(nb);
            if ((rc = run_batch(s, s->batches.size() - 1, nb.d_data, false))) return rc;
        }
    }
    kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results");
    return KVQ_ERR_MEMORY;
}

// several GPUs (kvq_scan_set_comm): `finish` is collective.  First the ranks agree on how their own scans
// ended -- the maximum of 0 (fine), 1 (this rank has to be fed its host batches again) and 2 (failed): only when
// every rank is fine are the counters of all ranks summed (into an array of their own: the rank's counters stay
// what they are, so that finishing twice does not sum sums); when some rank has to go round again every rank
// returns KVQ_ERR_RESCAN and goes round with it, with no sum taken (the collectives of the ranks stay in step);
// a failure anywhere is an error everywhere.
static int finish_over_ranks(kvq_scan *s, int rc_own)
{
    int rc;
    // (d_finish and d_ctr_all were made by kvq_scan_set_comm: nothing in front of the status exchange can fail on this rank alone)
    if ((rc = s->d_finish.ensure(sizeof(KvqFinishState) + 256))) return rc;
    unsigned long long *scratch = (unsigned long long *)((char *)s->d_finish.p + ((sizeof(KvqFinishState) + 15) & ~(size_t)15));
    unsigned long long worst = 0;
    const unsigned long long mine = rc_own == KVQ_OK ? 0ull : rc_own == KVQ_ERR_RESCAN ? 1ull : 2ull;
    if ((rc = kvq_comm_max_status(s->comm, mine, scratch, s->stream, &worst))) return rc;
    if (worst == 2) {
        if (rc_own != KVQ_OK && rc_own != KVQ_ERR_RESCAN) return rc_own;             // (its own message stands)
        kvq_set_error(KVQ_ERR_RUNTIME, "the scan of another rank has failed");
        return KVQ_ERR_RUNTIME;
    }
    if (worst == 1) {
        if (rc_own != KVQ_ERR_RESCAN) kvq_set_error(KVQ_ERR_RESCAN, "the hit arena of another rank overflowed on host batches: every rank resets its scan and feeds its batches again");
        s->finished = false;
        return KVQ_ERR_RESCAN;
    }
    if ((rc = s->d_ctr_all.ensure((size_t)s->t->ctr_len * 8))) return rc;
    if ((rc = kvq_comm_reduce_counters(s->comm, s->d_ctr, s->d_ctr_all.as<unsigned long long>(), s->t->ctr_len, scratch, s->stream))) return rc;
    KVQ_HIP(hipMemcpyAsync(s->pin, s->d_ctr_all.p, (size_t)s->t->ctr_len * 8, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    memcpy(s->h_ctr.data(), s->pin, (size_t)s->t->ctr_len * 8);
    s->reduced = true;
    return KVQ_OK;
}

extern "C" int32_t kvq_scan_finish(kvq_scan *s)
{
    kvq_clear_error();
    int rc = kvq_scan_finish_internal(s);
    if (rc == KVQ_NEED_RESCAN) { kvq_set_error(KVQ_ERR_RESCAN, "hit arena overflow on host batches: the arena has been enlarged, reset the scan and feed the batches again"); rc = KVQ_ERR_RESCAN; }
    if (s->comm) {
        const int saved = kvq_error_code(); char msg[1024]; kvq_last_error(msg, sizeof(msg));
        const int rc2 = finish_over_ranks(s, rc);
        if (rc && rc2 == rc) kvq_set_error(saved, "%s", msg);
        rc = rc2;
    }
    return rc;
}

extern "C" const uint8_t *kvq_scan_record_blob(const kvq_scan *s)
{
    return s->records_on && s->finished ? KvqPinRec(s->pin_rec, s->rec_hcap).store : nullptr;
}
extern "C" const int64_t *kvq_scan_hit_record_off(const kvq_scan *s) { return s->records_on && s->finished ? KvqPinRec(s->pin_rec, s->rec_hcap).off : nullptr; }
extern "C" const int32_t *kvq_scan_hit_record_len(const kvq_scan *s)
{
    return s->records_on && s->finished ? KvqPinRec(s->pin_rec, s->rec_hcap).len : nullptr;
}
extern "C" int64_t kvq_scan_record_bytes(const kvq_scan *s) { return s->records_on && s->finished ? s->rec_store_bytes : 0; }
extern "C" int64_t kvq_scan_n_hits(const kvq_scan *s) { return (int64_t)s->n_hits; }
extern "C" const int32_t *kvq_scan_hit_seq_nr(const kvq_scan *s) { return reinterpret_cast<const int32_t *>(s->pin_res + s->res.seq_nr); }
extern "C" const int64_t *kvq_scan_hit_file_pos(const kvq_scan *s) { return reinterpret_cast<const int64_t *>(s->pin_res + s->res.file_pos); }
extern "C" const int32_t *kvq_scan_hit_seq_pos(const kvq_scan *s) { return reinterpret_cast<const int32_t *>(s->pin_res + s->res.seq_pos); }
extern "C" const int32_t *kvq_scan_hit_length(const kvq_scan *s) { return reinterpret_cast<const int32_t *>(s->pin_res + s->res.length); }
extern "C" const int32_t *kvq_scan_hit_readlength(const kvq_scan *s) { return reinterpret_cast<const int32_t *>(s->pin_res + s->res.readlength); }
extern "C" const uint8_t *kvq_scan_hitseq_blob(const kvq_scan *s) { return s->pin_res + s->res.blob; }
extern "C" const int64_t *kvq_scan_hitseq_offsets(const kvq_scan *s) { return reinterpret_cast<const int64_t *>(s->pin_res + s->res.hitseq_off); }
extern "C" const int64_t *kvq_scan_counters(const kvq_scan *s) { return s->h_ctr.data(); }
extern "C" void *kvq_scan_device_counters(const kvq_scan *s) { return s->reduced ? s->d_ctr_all.p : (void *)s->d_ctr; }
extern "C" void *kvq_scan_device_counters_own(const kvq_scan *s) { return s->d_ctr; }
extern "C" int64_t kvq_scan_parsed(const kvq_scan *s) { return s->parsed; }
extern "C" int64_t kvq_scan_total(const kvq_scan *s) { return s->total; }
extern "C" double kvq_scan_kernel_ms(const kvq_scan *s) { return s->ms_all; }
extern "C" double kvq_scan_main_kernel_ms(const kvq_scan *s) { return s->ms_main; }
extern "C" double kvq_scan_profile_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_PROFILE].ms; }
extern "C" double kvq_scan_cycles_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_CYCLES].ms; }
extern "C" double kvq_scan_reads_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_READS].ms; }
extern "C" double kvq_scan_over_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_OVER].ms; }
extern "C" double kvq_scan_adapt_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_ADAPT].ms; }
extern "C" double kvq_scan_clip_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_CLIP].ms; }
extern "C" double kvq_scan_emit_kernel_ms(const kvq_scan *s) { return s->passes[KVQ_PASS_EMIT].ms; }
// (measurement) ms from the end of a's last main kernel to the start of b's first one (both finished, neither reset since); < 0: unknown
extern "C" double kvq_scan_gap_ms(const kvq_scan *a, const kvq_scan *b)
{
    if (!a || !b || a->ev_main.empty() || b->ev_main.empty()) return -1.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, a->ev_main.back().second, b->ev_main.front().first) != hipSuccess) { (void)hipGetLastError(); return -1.0; }
    return (double)ms;
}
// (measurement) how the finished scan's hits were put in order: what kvq_finish_plan left, and the capacities as they are now
extern "C" void kvq_scan_order_info(const kvq_scan *s, int64_t out[9])
{
    for (int i = 0; i < 7; i++) out[i] = s->finished ? s->order_info[i] : 0;
    out[7] = (int64_t)s->arena_cap; out[8] = (int64_t)s->blob_cap;
}
// (measurement) the lists the finished scan's last seed-filter launch left behind: the words are read from the device here, when asked
// (kvq_expand_tiles zeroes the three counts in front of every such launch; nothing on the scan's path looks at them for this)
extern "C" int32_t kvq_scan_match_info(const kvq_scan *s, int64_t out[4])
{
    out[0] = out[2] = out[3] = 0; out[1] = (int64_t)s->surv_cap;
    if (!s->finished || !s->kernel_cell) return KVQ_OK;
    unsigned int sv = 0, rd[2] = { 0, 0 };
    if (s->d_surv.p) KVQ_HIP(hipMemcpy(&sv, KvqSurvivors(s->d_surv.p).count, 4, hipMemcpyDeviceToHost));
    if (s->d_redo.p) KVQ_HIP(hipMemcpy(rd, KvqRedo(s->d_redo.p).count, 8, hipMemcpyDeviceToHost));
    out[0] = sv; out[2] = rd[0]; out[3] = rd[1];
    return KVQ_OK;
}
extern "C" int64_t kvq_scan_main_kernel_launches(const kvq_scan *s) { return s->main_launches; }
