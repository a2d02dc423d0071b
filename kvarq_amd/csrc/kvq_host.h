// kvarq_amd/csrc/kvq_host.h -- host-side internals of libkvarq_hip.so
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <unistd.h>
#include <utility>
#include <vector>

#include "../../include/kvarq_hip.h"
#include "kvq_device.h"

// ---- error state (thread local) ----------------------------------------------
void kvq_set_error(int code, const char *fmt, ...);
void kvq_clear_error();
int  kvq_error_code();

#define KVQ_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            kvq_set_error(KVQ_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return KVQ_ERR_DEVICE;                                                            \
        }                                                                                     \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t n);          // KVQ_OK / error code; contents are NOT preserved
    void release();
    template <class T> T *as() const { return (T *)p; }
};

// per-batch tables (chunk offsets, tile maps): pinned host memory mirrored by device
// memory, bump-allocated so that a batch can be enqueued without waiting for the previous one
struct TablePool {
    uint8_t *h = nullptr, *d = nullptr; size_t cap = 0, used = 0, h_cap = 0, d_cap = 0;
    int reserve(size_t bytes, hipStream_t stream);   // makes room (may synchronise the stream when growing)
    size_t take(size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; }
    void release();
};

struct kvq_table {
    kvq_config cfg;
    int32_t nseq = 0;
    int64_t bases = 0;
    std::vector<uint8_t> h_tab;          // concatenated bytes
    std::vector<int32_t> h_off;          // nseq + 1
    std::vector<int32_t> exhaustive;     // sequences the exhaustive kernel serves
    std::vector<int32_t> seeded;         // sequences the seed-filter kernel serves
    std::vector<uint8_t> is_seeded;
    int32_t seed_k = 0;
    int device = 0;                      // the device the table's blocks live on
    DevBuf d_tab, d_off, d_exh, d_all, d_seeded;
    struct SeedIndex *index = nullptr;   // kernels_seeded
    int64_t ctr_len, off_nseqhits, off_nseqbasehits, off_cov, off_mut;
};
static inline size_t kvq_align256(size_t n) { return (n + 255) & ~(size_t)255; }
// the counters' bytes in the landing buffer of finish (kvq_scan::pin): the result arrays start behind them
static inline size_t kvq_ctr_bytes(const kvq_table *t) { return kvq_align256((size_t)t->ctr_len * 8); }

// where each array of a finished scan lives inside the result buffer (device copy and pinned host copy alike)
struct KvqResultLayout {
    size_t file_pos = 0, hitseq_off = 0, seq_nr = 0, seq_pos = 0, length = 0, readlength = 0, blob = 0, total = 0;
};

struct Batch {
    const uint8_t *d_data; int64_t nbytes; int64_t fpos_base;
    std::vector<int64_t> chunk_off;
    bool redone = false;      // its seed-filter pass failed validation; an exhaustive redo batch follows
    int8_t read_list = -1;    // the batch takes the read-list route (run_batch decides once: a replayed batch goes the way it went); -1: not decided
    bool is_redo = false;     // this batch is such a redo (or the redo of another batch's skipped tiles)
    const uint8_t *staged = nullptr;   // device text owned by the caller while the batch is in flight (kvq_scan_staged): a host batch for every other purpose
};

struct kvq_comm;
#define KVQ_REDO_CAP 16384u            // records that the skipped tiles of one launch may leave (beyond: the batch is redone as a whole)
// The scan kernel's survivors (round 4): a work item that passed the 16-base test -- a true hit as a rule, 0.02 per read -- is put on
// this list instead of being verified where it was found; kvq_verify_survivors, right behind the scan kernel, does the byte-exact
// part for all of them at once (a lane each).  Where it was found it cost its wave some twenty dependent trips to memory, and the
// other seven waves of the tile the wait for it: 6 % of the kernel's time for 0.003 hits per read.  A full list costs nothing but
// speed: the items that do not fit are verified in place, as before.
struct KvqSurvivor { uint32_t boff; uint16_t rl, p; uint64_t en; uint32_t kind, pad; };      // batch offset of the trimmed read, its length, read position of the seed, index entry, which index
#define KVQ_SURV_CAP (1u << 22)
#define KVQ_SURV_CHUNK 16u             // a wave takes the list's slots a chunk at a time (one atomic on the list's counter per chunk, not per survivor:
                                       // a word in memory takes ~88 atomics per microsecond, hit-dense input would queue up on it)
struct KvqSurvivors {
    unsigned int *count; KvqSurvivor *item;
    static size_t bytes() { return 256 + (size_t)KVQ_SURV_CAP * sizeof(KvqSurvivor); }
    __host__ __device__ explicit KvqSurvivors(void *p) { count = (unsigned int *)p; item = (KvqSurvivor *)((char *)p + 256); }
};
struct KvqRedo {                      // where the pieces lie inside kvq_scan::d_redo
    unsigned int *count; uint32_t *nl4, *rec_start, *read_off; int32_t *read_len;
    static size_t bytes() { return 256 + (size_t)KVQ_REDO_CAP * (16 + 4 + 4 + 4); }
    __host__ __device__ explicit KvqRedo(void *p) { char *c = (char *)p; count = (unsigned int *)c; nl4 = (uint32_t *)(c + 256); rec_start = nl4 + 4 * (size_t)KVQ_REDO_CAP; read_off = rec_start + KVQ_REDO_CAP; read_len = (int32_t *)(read_off + KVQ_REDO_CAP); }
};

// ---- where the pieces lie inside three small blocks of a scan -----------------
#define KVQ_MAX_BATCHES 65536
// kvq_scan::d_small (device): the eight small words kvq_publish_small hands to the host -- [0] arena_n u32, [8] blob_n, [16] err, [24] err of the batch
// in flight (u64) --, a range word per batch and one more (hits of batch b = arena[range[b], range[b + 1])), a "speculation failed" word per batch,
// the staging counters of the batch in flight (records, longest, read-length histogram)
struct KvqSmall {
    static constexpr size_t BLOB_N = 8, ERR = 16, ERR_STAGE = 24, RANGE = 64, FAIL = RANGE + 4 * (KVQ_MAX_BATCHES + 1),
                            STAGE = (FAIL + 4 * KVQ_MAX_BATCHES + 255) & ~(size_t)255, BYTES = STAGE + 8 * KVQ_STAGE_SLOTS * KVQ_STAGE_COPIES;
    static constexpr unsigned int PUBLISHED_WORDS = 8;
    static constexpr size_t ERR_WORD = ERR / 8, ERR_STAGE_WORD = ERR_STAGE / 8;      // kvq_reset_state writes 8-byte words: zeros, but all ones ("no error") into these two
    static_assert(ERR % 8 == 0 && ERR_STAGE % 8 == 0 && BYTES % 8 == 0 && ERR_STAGE + 8 <= RANGE, "kvq_reset_state writes 8-byte words");
    unsigned int *arena_n, *range, *fail; unsigned long long *blob_n, *err, *err_stage, *stage_ctr;
    explicit KvqSmall(void *p)
    {
        char *c = (char *)p; arena_n = (unsigned int *)c; range = (unsigned int *)(c + RANGE); fail = (unsigned int *)(c + FAIL);
        blob_n = (unsigned long long *)(c + BLOB_N); err = (unsigned long long *)(c + ERR); err_stage = (unsigned long long *)(c + ERR_STAGE); stage_ctr = (unsigned long long *)(c + STAGE);
    }
};
// kvq_scan::pin_small (pinned): the copy of the small words, the fail word of the host batch in flight (copied behind its kernels), and what
// kvq_publish_small leaves at the end of a scan: the fail word of every batch, the KvqFinishState
struct KvqPinSmall {
    static constexpr size_t CUR_FAIL = 40, FAIL = 64, STATE = FAIL + 4 * (size_t)KVQ_MAX_BATCHES, STATE_BYTES = 512, BYTES = STATE + STATE_BYTES;
    static_assert(4 * KvqSmall::PUBLISHED_WORDS <= CUR_FAIL && CUR_FAIL + 4 <= FAIL, "the pieces of pin_small overlap");
    unsigned int *small, *cur_fail, *fail, *state;
    explicit KvqPinSmall(uint8_t *p) { small = (unsigned int *)p; cur_fail = (unsigned int *)(p + CUR_FAIL); fail = (unsigned int *)(p + FAIL); state = (unsigned int *)(p + STATE); }
};
// kvq_scan::pin_rec (pinned), laid out for `hcap` hits: the record words, the offset and the length of every hit's record, the store
struct KvqPinRec {
    int64_t *off; int32_t *len; uint8_t *store;
    static size_t bytes(uint64_t hcap, uint64_t scap) { return 256 + kvq_align256(hcap * 8) + kvq_align256(hcap * 4) + scap; }
    KvqPinRec(uint8_t *p, uint64_t hcap) { off = (int64_t *)(p + 256); len = (int32_t *)(p + 256 + kvq_align256(hcap * 8)); store = (uint8_t *)len + kvq_align256(hcap * 4); }
};
int kvq_live_scans();                 // scan objects alive in this process
// the persistent scan kernels of a process run one behind the other (two at once only get in each other's way): a launch waits for
// the event the last one published, on its own stream, right in front of its scan kernel -- its table upload and kvq_expand_tiles do not wait
int kvq_chain_wait(struct kvq_scan *s, bool *behind_a_running_scan = nullptr);
bool kvq_chain_busy(const struct kvq_scan *s);     // a scan kernel of another scan object of the process is still on the device
int kvq_chain_publish(struct kvq_scan *s);
uint32_t kvq_device_cu_count();       // compute units of the current device
int kvq_comm_reduce_counters(kvq_comm *c, const unsigned long long *d_in, unsigned long long *d_out, int64_t ctr_len, unsigned long long *d_scratch, hipStream_t stream);
int kvq_comm_max_status(kvq_comm *c, unsigned long long mine, unsigned long long *d_scratch, hipStream_t stream, unsigned long long *out);

// An input pass: a kernel that every batch runs once over its exact record index and that adds to one device array, which the
// tail of the scan brings to the host.  The cycles' array has the kernel's own scratch word behind the words that land.
// (the clip is no pass behind the scan: its kernel runs in front of it and needs no profile -- clip_text in kvq_scan.hip; its array shares the lifecycle)
// (the emit is the last pass behind the scan and needs no profile either -- emit_enqueue in kvq_profile.hip; its eight words share the lifecycle)
enum { KVQ_PASS_PROFILE, KVQ_PASS_CYCLES, KVQ_PASS_READS, KVQ_PASS_OVER, KVQ_PASS_ADAPT, KVQ_PASS_CLIP, KVQ_PASS_EMIT, KVQ_PASSES };
typedef std::pair<hipEvent_t, hipEvent_t> KvqEventPair;
struct KvqPass {
    bool on = false;
    DevBuf d; size_t d_bytes = 0;                       // the device array, and what of it is cleared
    int64_t *pin = nullptr; size_t pin_cap = 0;         // its pinned landing buffer
    size_t words = 0;                                   // the words of d that land
    std::vector<int64_t> h;                             // the finished scan's copy
    std::vector<KvqEventPair> ev; double ms = 0;        // around the pass's kernels of every batch; their sum
};

// the device buffers of a deflate (kernels_deflate.hip): the slots of a round's members, their sizes (which become
// their offsets) and lengths, the tokens of the workgroups of the grid, the words
struct KvqDeflateBufs { DevBuf slots, sizes, lens, tokens, words; };
int  kvq_deflate_enqueue(const uint8_t *d_text, uint64_t nbytes, uint8_t *d_out, uint64_t cap, KvqDeflateBufs &B, hipStream_t stream);
void kvq_deflate_release(KvqDeflateBufs &B);

// the probes of an adapter option as the caller gave them: n of them (0: the option is off), their lengths and bytes; what is
// not in use is zero
struct KvqProbeSet {
    int32_t n = 0; uint8_t lens[KVQ_ADAPT_MAX_PROBES] = { 0 }; uint8_t probes[KVQ_ADAPT_MAX_PROBES][KVQ_ADAPT_MAX_PROBE] = { { 0 } };
    void clear() { *this = KvqProbeSet(); }
    void assign(const uint8_t *const *p, const int32_t *l, int32_t count)
    {
        clear();
        n = count;
        for (int32_t k = 0; k < n; k++) { lens[k] = (uint8_t)l[k]; memcpy(probes[k], p[k], (size_t)l[k]); }
    }
};

struct kvq_scan {
    const kvq_table *t = nullptr;
    kvq_comm *comm = nullptr;            // several GPUs: `finish` sums the counters of all ranks over it (kvq_dist.hip)
    hipStream_t stream = nullptr;
    bool force_exhaustive = false;
    int long_mode = 0;                   // the read-list route (kvq_scan_set_long_reads): 0 off, 1 every batch, 2 the batches whose head says long reads
    // counters
    unsigned long long *d_ctr = nullptr; DevBuf d_ctr_own;
    std::vector<int64_t> h_ctr;
    // per-batch scratch
    uint32_t cus = 0;                  // compute units of the scan's device (asked once)
    bool seen_skips = false;           // a tile of this scan object has left records to the redo before (kept across resets: sizes the redo's launches)
    bool tail_pending = false; size_t tail_nb0 = 0, tail_spec = 0;      // the tail of the scan (enqueue_tail) is on the stream for these batches: kvq_scan_finish_begin
    bool tail_mergesort = false;       // ... and was enqueued without the bucket ordering (KVQ_ORDER=mergesort at that moment)
    int64_t order_info[7] = { 0, 0, 0, 0, 0, 0, 0 };                    // kvq_scan_order_info: n, nb, shift, bc, lo, crowded, "the merge sort made the result" of the finished scan
    uint32_t surv_cap = 0;             // slots of d_surv's list (KVQ_SURV_CAP, or what the environment cut it to)
    DevBuf d_surv;                     // what passed the scan kernel's 16-base test, for kvq_verify_survivors (KvqSurvivors)
    DevBuf d_redo;                     // the redo of skipped tiles (KvqRedo: count, newline quadruples, record starts, trimmed reads)
    bool keep_skipped = false;         // (measurement) kvq_scan_set_keep_skipped: redo_if_failed keeps host copies of the two lists below
    std::vector<uint32_t> kept_tiles;  // the skipped-tile descriptors of the batch whose fail word was read last (six words each, as kvq_validate_tiles wrote them)
    std::vector<uint32_t> kept_redo;   // what kvq_collect_skipped put on the redo list for them (five words each: rec_start, nl4)
    DevBuf d_seg_base, d_seg_cnt, d_chunk_nrec, d_rec_base, d_nl4, d_rec_start, d_read_off, d_read_len;
    // hit arena
    DevBuf d_covdiff;                  // coverage marks (KvqParams::covdiff)
    uint32_t tile_bytes = 0;           // bytes a tile of the seed-filter kernel owns (0 = not chosen yet; kvq_choose_tile)
    uint32_t rec_bytes = 0;            // average record among the first bytes of the text (0 = unknown)
    DevBuf d_arena, d_blob, d_small;   // d_small: KvqSmall; the seven pointers below are its pieces
    uint32_t arena_cap = 0; uint64_t blob_cap = 0;
    unsigned int *d_arena_n = nullptr, *d_range = nullptr, *d_fail = nullptr, *cur_fail = nullptr;
    unsigned long long *d_blob_n = nullptr, *d_err = nullptr, *d_err_stage = nullptr, *d_stage_ctr = nullptr;
    int path_bits = 0;
    int32_t kernel_cell = 0;           // the kvq_scan_bp instantiation of the last seed-filter launch (kvq_scan_kernel_pick)
    int32_t kernel_grid = 0;           // ... and its workgroups (kvq_scan_grid)
    int64_t launch_info[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };         // kvq_scan_launch_info: the seed-filter launches since the scan was made or reset (kvq_launch.hip writes, nothing reads)
    std::vector<int64_t> cur_chunk_off;  // chunk offsets of the batch being enqueued
    size_t cur_co_at = 0;                // ... and where run_batch put them in the pool
    size_t cur_skip_at = 0, cur_first_at = 0; uint32_t cur_ntiles = 0;   // the batch's list of skipped tiles, its first-tile table
    TablePool pool;
    // staging for host batches
    // Host batches: two staging buffers.  A batch's text crosses PCIe on copy_stream as soon as it is handed over; its
    // kernels are enqueued one call later, when the batch in front of it has been settled -- the copy engine never waits
    // for kernels, the kernels never wait for the host
    DevBuf d_stage, d_stage_b;
    int run_slot = 1;                    // the buffer of the batch whose kernels are in flight (the next text goes to the other one)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy[2] = { nullptr, nullptr };
    bool copied_pending = false; int copied_slot = 0; Batch copied;   // the batch whose text is on its way (or there), kernels not yet enqueued
    // replay list (device batches) + bookkeeping
    std::vector<Batch> batches;
    bool host_batches = false;
    int64_t host_pending = -1;           // index of the host batch in flight (kvq_scan_host_async), -1: none
    hipEvent_t ev_chain = nullptr;       // what the next scan of the process waits for.  One job at a time: this scan's last seed-filter launch AND its kvq_verify_survivors are through (recorded behind the two, in front of kvq_validate_tiles).  Jobs in flight (the launch went `beside`, kvq_seeded_launch): the scan kernel alone is through -- recorded behind it and IN FRONT of kvq_verify_survivors, which then runs beside the next scan
    int64_t parsed = 0, total = 0;
    // timing
    std::vector<KvqEventPair> ev_all, ev_main, ev_free;     // ev_free: pairs of earlier scans, reused (the passes below have their own)
    double ms_all = 0, ms_main = 0; int64_t main_launches = 0;
    // results: ordered and laid out on the device (kernels_results.hip), one copy into pinned host memory
    DevBuf d_sort_tmp, d_sorted, d_result, d_order, d_finish;   // d_order: bucket arrays of the ordering; d_finish: KvqFinishState
    uint32_t order_nb_max = 0;                    // the bucket arrays in d_order are laid out for this many buckets
    uint8_t *pin_res = nullptr;                   // where the result arrays start inside pin (behind the counters)
    size_t spec_bytes = 1u << 20;                 // result bytes fetched together with the counters, before their number is known (the last scan's)
    uint8_t *pin = nullptr; size_t pin_cap = 0;   // pinned landing buffer of finish: the result arrays, then the counters
    uint8_t *pin_small = nullptr; size_t pin_small_cap = 0;   // pinned landing buffer for the scan's small words and fail flags (KvqPinSmall)
    KvqResultLayout res;                          // where the arrays sit inside pin
    uint64_t n_hits = 0;
    bool finished = false;
    // several ranks (kvq_dist.hip)
    DevBuf d_ctr_all;                             // the counters of all ranks, summed (the rank's own stay in d_ctr: a repeated finish sums them afresh)
    DevBuf d_gather_cnt, d_gather_res;            // kvq_scan_gather_hits: counts of the ranks, the gathered arrays
    bool reduced = false, gathered = false;
    // the records of the hits (kvq_scan_set_records, kernels_records.hip): a table keyed by file_pos, a store of record
    // bytes, and the per-hit (offset, length) the finish looks up; all of it lands in pin_rec
    bool records_on = false;
    DevBuf d_rkey, d_roff, d_rlen, d_rdir, d_rstore, d_rsmall, d_rres;
    uint32_t rslots = 0;                          // slots of the table (a power of two, >= 2 x arena_cap)
    unsigned long long rstore_cap = 0;            // bytes of the store (KVQ_RECORD_CAP caps the first one)
    uint8_t *pin_rec = nullptr; size_t pin_rec_cap = 0;   // pinned (KvqPinRec): the record words, offsets [rec_hcap], lengths [rec_hcap], store bytes [rec_scap]
    uint64_t rec_hcap = 0, rec_scap = 0;
    uint64_t rec_tail_n = 0, rec_tail_b = 0;      // what the tail fetched ahead of time (offsets / lengths of that many hits, that many store bytes)
    uint64_t rec_spec_n = 4096, rec_spec_b = 1u << 20;   // ... guessed from the last scan of this handle
    int64_t rec_store_bytes = 0;                  // store bytes of the finished scan
    // the passes over a batch's exact record index (kvq_profile.hip; DESIGN section 13, "the lifecycle of an input pass"), in the
    // order they run: the profile of the input (kvq_scan_set_profile), the per-cycle counts beside it (kvq_scan_set_cycles) and what
    // the individual reads look like (kvq_scan_set_read_stats), the overrepresented sequences (kvq_scan_set_overrepresented) and the adapter content
    // (kvq_scan_set_adapters).  All but
    // the first keep their buffers only while they are on
    KvqPass passes[KVQ_PASSES];
    int32_t prof_ncut = 0; uint8_t prof_cuts[KVQ_PROFILE_MAX_CUTOFFS] = { 0 };      // the profile's cutoffs
    // the reads pass: bit 0 of its mode the per-read distributions (the pass's array), bit 1 the duplication (d_dup: the state block,
    // two tables of dup_slots slots, the result array kvq_dup_levels writes; KvqDupLayout), which lands behind the distributions
    int32_t reads_mode = 0;
    DevBuf d_dup; uint64_t dup_slots = 0;
    std::vector<int64_t> h_dup;
    // the overrepresented sequences: M, the slots of the table (the pass's array: KvqOverLayout), and the records the pass has seen
    // since it was last cleared -- the first M of them make the candidates
    uint64_t over_M = 0, over_slots = 0, over_seen = 0;
    // the probes of the adapter content (kvq_scan_set_adapters) and of the adapter clip (kvq_scan_set_clip; its
    // array is passes[KVQ_PASS_CLIP]); n == 0: off
    KvqProbeSet adapt, clip;
    // one mismatch per this many bases in the probes of both (kvq_scan_set_adapter_mismatches): 0, the exact rule, or 10 .. 32
    int32_t adapt_per = 0;
    // the emit (kvq_scan_set_emit): its words are passes[KVQ_PASS_EMIT] (the array has the batch's total and the copies of
    // the guards behind the words that land).  Per record what kvq_emit_size says of it and where its output begins, the block sums of
    // the prefix sum, the store of a batch (nbytes + nrec bytes between two guards: KvqEmitLayout), reused batch after batch; a pinned
    // buffer of two halves through which the emitted bytes reach the sink: the host buffer, or the caller's file descriptor
    int32_t emit_min = 0;
    DevBuf d_emit_rec, d_emit_off, d_emit_bsum, d_emit_store;
    uint8_t *emit_pin = nullptr; size_t emit_pin_cap = 0;
    hipEvent_t emit_ev[2] = { nullptr, nullptr };
    std::vector<uint8_t> emit_sink; int emit_fd = -1;
    int64_t emit_guard_bad = 0;
    // the emit's deflate (kvq_scan_set_emit_compress): on, every batch's text goes through kvq_deflate_enqueue into
    // d_deflate_out and that stream takes the text's way through the two halves; the words of the batches so far (summed on the host:
    // every batch lands its own in deflate_pin), whether the sink has its EOF member, the event pairs around the batches' kernels
    bool emit_compress = false, emit_eof_done = false;
    KvqDeflateBufs deflate; DevBuf d_deflate_out;
    int64_t *deflate_pin = nullptr; size_t deflate_pin_cap = 0;
    int64_t deflate_words[KVQ_DEFLATE_WORDS] = { 0 };
    std::vector<KvqEventPair> deflate_ev; size_t deflate_ev_n = 0;
};

// kvq_scan.hip: KVQ_OK while the scan holds no batch -- the one moment at which the setter `who` may change an option -- else its refusal
int scan_idle(const kvq_scan *s, const char *who);

// kernels_seeded.hip
struct SeedIndex;
SeedIndex *kvq_seed_index_build(kvq_table *t);           // nullptr when no sequence qualifies
void       kvq_seed_index_destroy(SeedIndex *ix);
// enqueue the fused seed-filter scan of one batch; returns KVQ_OK or error
int kvq_seeded_launch(kvq_scan *s, const KvqParams &P, const uint8_t *d_data, int64_t nbytes,
                      const uint32_t *d_chunk_off, int64_t nchunks, int64_t fpos_base, uint32_t max_chunk_bytes);

uint32_t kvq_choose_tile(uint32_t maxline, uint32_t rec_bytes);
uint32_t kvq_min_tile();
int32_t  kvq_scan_pick(int k, int stride, bool ix_dense, uint32_t rec_bytes, uint32_t tile_bytes, uint32_t dbg, int lg_env, int dense_env);   // (kvq_launch.hip)

// synth.hip
// (C ABI only)

// kvq_scan.hip: a batch whose text the CALLER has put into device memory and keeps there only until the next batch
// is handed over (the device-inflate route of findseqs): scanned, settled and -- on a hit-arena overflow -- fed again
// like a host batch, never replayed from its buffer
int kvq_scan_staged(kvq_scan *s, const uint8_t *d_text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base);

// kernels_inflate.hip
struct kvq_bgzf_entry_ { int64_t off; uint32_t size, hdr, isize; };     // a BGZF block of a file: offset, bytes, header bytes, inflated bytes
int kvq_inflate_bgzf_launch(const uint8_t *d_in, int64_t in_bytes, const kvq_bgzf_block *d_tab, int64_t nblocks,
                            uint8_t *d_out, int64_t out_bytes, int32_t *d_status, hipStream_t stream);
int kvq_cut_chunks_launch(const uint8_t *d_text, int64_t have, int64_t cs, int64_t fill, int64_t *d_offs, int64_t cap, int64_t *d_res, hipStream_t stream);

// kvq_findseqs.hip: engine.stop() has asked the running findseqs to end (every walk looks at every run)
bool kvq_stop_requested();

// ---- input files (kvq_routes.hip, kvq_reader.hip) ----------------------------
// up to k bytes at offset `at` of an open file: the `read` of kvq_bgzf_peek and kvq_bgzf_walk (an error reads nothing)
struct PreadAt {
    int fdn;
    int64_t operator()(uint8_t *dst, int64_t k, int64_t at) const { const ssize_t got = pread(fdn, dst, (size_t)k, (off_t)at); return got < 0 ? 0 : (int64_t)got; }
};
// gzip or not is decided by the name (workhorse.c:582)
static inline bool gz_suffix(const std::string &name) { return name.size() >= 3 && name.compare(name.size() - 3, 3, ".gz") == 0; }
