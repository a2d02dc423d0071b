// kvarq_amd/csrc/kvq_profile.hip -- the input passes (include/kvarq_hip.h, DESIGN sections 13, 14, 16, 17 and 18), host side: the profile, the
// per-cycle counts, the per-read statistics, the overrepresented sequences, the adapter content and the adapter clip (section 19), with the mismatch rate of their probes (section 20), and the emit of the trimmed reads (section 21), as options of a scan object, the steps of their common lifecycle, the launch of
// each pass behind a batch's kernels and its way to the host in the tail of a scan (their CPU twins: kvq_twins.cpp)
#include "kvq_host.h"
#include "kvq_lines.h"
#include "kvq_deflate.h"
#include <array>
#include <string.h>
#include <sys/stat.h>

// ---- the lifecycle of an input pass: what the three share, written once ----
// make or grow the device array (d_bytes, none: 0) and the landing buffer; `words` of the array land
static int pass_make(KvqPass &p, size_t d_bytes, size_t words, size_t pin_bytes)
{
    int rc;
    if (d_bytes && (rc = p.d.ensure(d_bytes))) return rc;
    if (p.pin_cap < pin_bytes) {
        if (p.pin) pinned_give(p.pin, p.pin_cap);
        p.pin = (int64_t *)pinned_take(pin_bytes, &p.pin_cap);
        if (!p.pin) { p.pin_cap = 0; kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    p.on = true; p.d_bytes = d_bytes; p.words = words;
    p.h.clear();
    return KVQ_OK;
}
// off, the buffers given back (the cycles and the reads; the profile keeps its buffers and is only marked off)
static void pass_off(kvq_scan *s, KvqPass &p)
{
    if (p.d.p) (void)hipStreamSynchronize(s->stream);       // (a reset has enqueued its clearing: the block goes back to a cache other streams take from)
    if (p.pin) pinned_give(p.pin, p.pin_cap);
    p.pin = nullptr; p.pin_cap = 0;
    p.d.release();
    p.h.clear(); p.h.shrink_to_fit();
    p.on = false; p.d_bytes = p.words = 0;
}
static void reads_off(kvq_scan *s)
{
    if (s->d_dup.p) (void)hipStreamSynchronize(s->stream);  // (as pass_off)
    s->d_dup.release();
    s->h_dup.clear(); s->h_dup.shrink_to_fit();
    s->reads_mode = 0; s->dup_slots = 0;
    pass_off(s, s->passes[KVQ_PASS_READS]);
}

// where the pieces lie inside kvq_scan::d_dup: the state block, the result array of kvq_dup_levels, the two tables
struct KvqDupLayout {
    static constexpr size_t STATE = 0, RESULT = 1024, TABLES = 2048;
    static_assert(KvqDupState::WORDS * 8 <= RESULT && RESULT + KVQ_DUP_WORDS * 8 <= TABLES, "the pieces of d_dup overlap");
    static size_t bytes(uint64_t slots) { return TABLES + 2 * (size_t)slots * 16; }
};
static KvqDupTable dup_table(const kvq_scan *s)
{
    KvqDupTable T; T.state = nullptr; T.tab[0] = T.tab[1] = nullptr; T.lg = 0;
    if (!(s->reads_mode & KVQ_READ_DUPLICATION)) return T;
    char *p = (char *)s->d_dup.p;
    T.state = (unsigned long long *)(p + KvqDupLayout::STATE);
    T.tab[0] = (unsigned long long *)(p + KvqDupLayout::TABLES); T.tab[1] = T.tab[0] + 2 * s->dup_slots;
    while ((1ull << T.lg) < s->dup_slots) T.lg++;
    return T;
}

// where the pieces lie inside the array of KVQ_PASS_OVER: the result array of kvq_over_select (the words that land), the state block, the table
struct KvqOverLayout {
    static constexpr size_t RESULT = 0, STATE = (size_t)KVQ_OVER_WORDS * 8, TABLE = STATE + 256;
    static_assert(KvqOverState::WORDS * 8 <= 256 && STATE % 8 == 0, "the pieces of the array overlap");
    static size_t bytes(uint64_t slots) { return TABLE + (size_t)slots * KVQ_OVER_ROW_WORDS * 8; }
};
static KvqOverTable over_table(const kvq_scan *s)
{
    KvqOverTable T; T.lg = 0;
    char *p = (char *)s->passes[KVQ_PASS_OVER].d.p;
    T.state = (unsigned long long *)(p + KvqOverLayout::STATE); T.slots = (unsigned long long *)(p + KvqOverLayout::TABLE);
    while ((1ull << T.lg) < s->over_slots) T.lg++;
    return T;
}
static void over_off(kvq_scan *s)
{
    s->over_M = s->over_slots = s->over_seen = 0;
    pass_off(s, s->passes[KVQ_PASS_OVER]);
}

static void adapt_off(kvq_scan *s)
{
    s->adapt.clear();
    pass_off(s, s->passes[KVQ_PASS_ADAPT]);
}

// the device arrays of the passes that are on (and the duplication's table: a zero state block is level 0 with table 0 active) back to
// zero: wherever the hit arena is cleared (reset_device_state), so that a replay, a rescan round and a file read again count every record once
static int pass_clear(kvq_scan *s, int which)
{
    const KvqPass &p = s->passes[which];
    if (p.d_bytes) KVQ_HIP(hipMemsetAsync(p.d.p, 0, p.d_bytes, s->stream));
    if (which == KVQ_PASS_READS && (s->reads_mode & KVQ_READ_DUPLICATION)) KVQ_HIP(hipMemsetAsync(s->d_dup.p, 0, KvqDupLayout::bytes(s->dup_slots), s->stream));
    if (which == KVQ_PASS_OVER) s->over_seen = 0;            // (the table is the pass's array: empty again, and the next record is number 0)
    if (which == KVQ_PASS_EMIT) {
        // the sink is empty again: a batch that runs again is emitted once (no batch is in flight here: every batch's emit ends with a host wait)
        s->emit_sink.clear(); s->emit_guard_bad = 0;
        // (and with it the deflate's words and its EOF member: a replay still leaves one stream with one end)
        for (int64_t &w : s->deflate_words) w = 0;
        s->emit_eof_done = false; s->deflate_ev_n = 0;
        // (a regular file is truncated and sought to its start; what is no such file -- a pipe, a terminal -- cannot take anything back)
        struct stat st;
        if (s->emit_fd >= 0 && fstat(s->emit_fd, &st) == 0 && S_ISREG(st.st_mode) && (ftruncate(s->emit_fd, 0) != 0 || lseek(s->emit_fd, 0, SEEK_SET) != 0)) {
            kvq_set_error(KVQ_ERR_IO, "cannot empty the file of the emitted reads");
            return KVQ_ERR_IO;
        }
    }
    return KVQ_OK;
}
static int passes_clear(kvq_scan *s)
{
    for (int i = 0; i < KVQ_PASSES; i++) if (s->passes[i].on) { const int rc = pass_clear(s, i); if (rc) return rc; }
    return KVQ_OK;
}

// the tail of a scan: the arrays on their way to the host (finish_once waits for the tail), and what kvq_dup_levels makes of the
// active table behind the distributions; passes_landed: the finished scan's copies
static int passes_tail(kvq_scan *s)
{
    if (s->passes[KVQ_PASS_OVER].on) {
        // (in front of the copies: the result array is the part of the pass's array that lands)
        unsigned long long *res = (unsigned long long *)((char *)s->passes[KVQ_PASS_OVER].d.p + KvqOverLayout::RESULT);
        KVQ_HIP(hipMemsetAsync(res, 0, (size_t)KVQ_OVER_WORDS * 8, s->stream));
        hipLaunchKernelGGL(kvq_over_select, dim3((uint32_t)std::min<uint64_t>(s->over_slots / 256, KVQ_OVER_GRID_MAX)), dim3(256), 0, s->stream,
                           over_table(s), (unsigned long long)s->over_M, res);
        KVQ_HIP(hipGetLastError());
    }
    for (KvqPass &p : s->passes) if (p.on && p.words) KVQ_HIP(hipMemcpyAsync(p.pin, p.d.p, p.words * 8, hipMemcpyDeviceToHost, s->stream));
    if (s->reads_mode & KVQ_READ_DUPLICATION) {
        unsigned long long *res = (unsigned long long *)((char *)s->d_dup.p + KvqDupLayout::RESULT);
        KVQ_HIP(hipMemsetAsync(res, 0, (size_t)KVQ_DUP_WORDS * 8, s->stream));
        hipLaunchKernelGGL(kvq_dup_levels, dim3((uint32_t)std::min<uint64_t>(s->dup_slots / 256, KVQ_DUP_GRID_MAX)), dim3(256), 0, s->stream, dup_table(s), res);
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipMemcpyAsync(s->passes[KVQ_PASS_READS].pin + KVQ_READS_WORDS, res, (size_t)KVQ_DUP_WORDS * 8, hipMemcpyDeviceToHost, s->stream));
    }
    return KVQ_OK;
}
static int emit_append(kvq_scan *s, const uint8_t *p, size_t n);
static int passes_landed(kvq_scan *s)
{
    for (KvqPass &p : s->passes) if (p.on) p.h.assign(p.pin, p.pin + p.words);
    if (s->reads_mode & KVQ_READ_DUPLICATION) {
        const int64_t *dup = s->passes[KVQ_PASS_READS].pin + KVQ_READS_WORDS;
        s->h_dup.assign(dup, dup + KVQ_DUP_WORDS);
    }
    if (s->passes[KVQ_PASS_OVER].on) {
        // the rows landed in the order the slots' workgroups came by: into the canonical one -- count descending, ties by hash ascending as unsigned
        typedef std::array<int64_t, KVQ_OVER_ROW_WORDS> Row;
        std::vector<int64_t> &h = s->passes[KVQ_PASS_OVER].h;
        h[KVQ_OVER_LISTED] = std::min<int64_t>(h[KVQ_OVER_LISTED], KVQ_OVER_MAX_ROWS);
        std::vector<Row> rows((size_t)h[KVQ_OVER_LISTED]);
        if (!rows.empty()) memcpy(rows.data(), h.data() + KVQ_OVER_ROWS, rows.size() * sizeof(Row));
        std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
            return a[KVQ_OVER_ROW_COUNT] != b[KVQ_OVER_ROW_COUNT] ? a[KVQ_OVER_ROW_COUNT] > b[KVQ_OVER_ROW_COUNT]
                                                                  : (uint64_t)a[KVQ_OVER_ROW_HASH] < (uint64_t)b[KVQ_OVER_ROW_HASH];
        });
        if (!rows.empty()) memcpy(h.data() + KVQ_OVER_ROWS, rows.data(), rows.size() * sizeof(Row));
    }
    if (s->passes[KVQ_PASS_ADAPT].on) {
        // the words that are no sums: n and every m_k
        std::vector<int64_t> &h = s->passes[KVQ_PASS_ADAPT].h;
        h[KVQ_ADAPT_N] = s->adapt.n;
        if (s->adapt_per) h[KVQ_ADAPT_PER] = s->adapt_per;
        for (int k = 0; k < s->adapt.n; k++) h[KVQ_ADAPT_BLOCKS + (size_t)k * KVQ_ADAPT_BLOCK_WORDS + KVQ_ADAPT_B_M] = s->adapt.lens[k];
    }
    if (s->passes[KVQ_PASS_CLIP].on) {
        // the words that are no sums: n and per
        s->passes[KVQ_PASS_CLIP].h[KVQ_CLIP_N] = s->clip.n;
        if (s->adapt_per) s->passes[KVQ_PASS_CLIP].h[KVQ_CLIP_PER] = s->adapt_per;
    }
    if (s->passes[KVQ_PASS_EMIT].on) s->passes[KVQ_PASS_EMIT].h[KVQ_EMIT_N] = s->emit_min;      // (the word that is no sum)
    // the scan is over: the compressed sink gets its EOF member, once
    if (s->passes[KVQ_PASS_EMIT].on && s->emit_compress && !s->emit_eof_done) {
        s->emit_eof_done = true;
        return emit_append(s, kvq_bgzf_eof(), KVQ_BGZF_EOF_BYTES);
    }
    return KVQ_OK;
}
// what an accessor hands out: the copy of a pass that is on, of a finished scan
static const int64_t *pass_result(const kvq_scan *s, int which)
{
    const KvqPass &p = s->passes[which];
    return p.on && s->finished && !p.h.empty() ? p.h.data() : nullptr;
}

// ---- the profile ----
extern "C" int64_t kvq_profile_len(int32_t ncut)
{
    return ncut < 0 || ncut > KVQ_PROFILE_MAX_CUTOFFS ? 0 : (int64_t)KVQ_PROF_CUTOFFS + (int64_t)ncut * KVQ_PROF_CUT_WORDS;
}

extern "C" int32_t kvq_scan_set_profile(kvq_scan *s, const uint8_t *cutoffs, int32_t ncut)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_profile"))) return rc;
    if (ncut < 0) { s->passes[KVQ_PASS_PROFILE].on = false; s->prof_ncut = 0; pass_off(s, s->passes[KVQ_PASS_CYCLES]); reads_off(s); over_off(s); adapt_off(s); return KVQ_OK; }
    if (ncut > KVQ_PROFILE_MAX_CUTOFFS || (ncut > 0 && !cutoffs)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_profile: at most %d cutoffs", KVQ_PROFILE_MAX_CUTOFFS);
        return KVQ_ERR_RUNTIME;
    }
    if (s->comm) {
        kvq_set_error(KVQ_ERR_RUNTIME, "the profile is not reduced across ranks: a scan with a communicator cannot keep one");
        return KVQ_ERR_RUNTIME;
    }
    const size_t words = (size_t)kvq_profile_len(ncut);
    if ((rc = pass_make(s->passes[KVQ_PASS_PROFILE], words * 8, words, words * 8))) return rc;
    s->prof_ncut = ncut;
    memset(s->prof_cuts, 0, sizeof(s->prof_cuts));
    if (ncut) memcpy(s->prof_cuts, cutoffs, (size_t)ncut);
    return pass_clear(s, KVQ_PASS_PROFILE);
}

// The two forms of the kernel's byte histograms (kernels_profile.hip: prof_byte; the results are the same).  Copies spread over
// the lanes are the faster form as long as their 16 KiB of LDS leave four workgroups on a CU, which the kernel's registers
// allow: up to four cutoffs.  Beyond, the wave counts its equal bytes first (profiles/profile_rate.txt has both, measured).
// KVQ_PROFILE_HIST=spread / wave: that form whatever the cutoffs (tools/profile_rate.py).
static bool profile_spread(int ncut)
{
    static const char *e = getenv("KVQ_PROFILE_HIST");
    if (e && !strcmp(e, "spread")) return true;
    if (e && !strcmp(e, "wave")) return false;
    return (size_t)KvqProfLds::words(ncut, true) * 4 <= 40960;
}

// the profile pass over the R records of a batch whose index (kvq_index_records: nl4) is on the scan's stream
static int profile_enqueue(kvq_scan *s, const uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    KvqProfileCuts C; C.n = s->prof_ncut; C.packed = 0;
    for (int k = 0; k < s->prof_ncut; k++) C.packed |= (unsigned long long)s->prof_cuts[k] << (8 * k);
    const bool spread = profile_spread(s->prof_ncut);
    const uint32_t per_block = 4 * KVQ_TRIM_RPW;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((R + per_block - 1) / per_block, 2048);      // (the kernel strides over what there is)
    hipLaunchKernelGGL(kvq_profile_records, dim3(grid), dim3(256), (size_t)KvqProfLds::words(C.n, spread) * 4, s->stream, d_data,
                       s->d_nl4.as<uint32_t>(), (uint32_t)R, C, spread ? 1u : 0u, s->passes[KVQ_PASS_PROFILE].d.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

extern "C" const int64_t *kvq_scan_profile(const kvq_scan *s) { return pass_result(s, KVQ_PASS_PROFILE); }
extern "C" int32_t kvq_scan_profile_cutoffs(const kvq_scan *s, uint8_t *cutoffs8)
{
    if (!s->passes[KVQ_PASS_PROFILE].on) return -1;
    if (cutoffs8 && s->prof_ncut) memcpy(cutoffs8, s->prof_cuts, (size_t)s->prof_ncut);
    return s->prof_ncut;
}

// ---- per-cycle counts ----
extern "C" int64_t kvq_cycles_len(void) { return 2 * (int64_t)KVQ_CYCLES * 256; }

extern "C" int32_t kvq_scan_set_cycles(kvq_scan *s, int32_t on)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_cycles"))) return rc;
    KvqPass &p = s->passes[KVQ_PASS_CYCLES];
    if (!on) { pass_off(s, p); return KVQ_OK; }
    if (!s->passes[KVQ_PASS_PROFILE].on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_cycles: the scan keeps no profile (the cycles ride on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    const size_t words = (size_t)kvq_cycles_len();
    if ((rc = pass_make(p, (words + 1) * 8, words, words * 8))) { pass_off(s, p); return rc; }      // (the kernel's scratch word behind the array)
    return pass_clear(s, KVQ_PASS_CYCLES);
}

// The slab width (kernels_profile.hip).  KVQ_CYCLES_SLAB=64 / 128: that width (tools/cycles_rate.py).
static bool cycles_alt_width()
{
    static const char *e = getenv("KVQ_CYCLES_SLAB");
    return e && (uint32_t)atoi(e) == KVQ_CYC_SLAB_ALT;
}

// the cycles pass over the R records of a batch, behind its profile pass: slab 0, which every record reaches and which raises
// the longest line; then the other slabs, which read it (a workgroup of a slab that no line reaches returns at once)
static int cycles_enqueue(kvq_scan *s, const uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    const bool alt = cycles_alt_width();
    const uint32_t W = alt ? KVQ_CYC_SLAB_ALT : KVQ_CYC_SLAB;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((R + 255) / 256, 1024);             // (the kernel strides over what there is)
    auto *kernel = alt ? kvq_profile_cycles_alt : kvq_profile_cycles;
    unsigned long long *d_cyc = s->passes[KVQ_PASS_CYCLES].d.as<unsigned long long>();
    hipLaunchKernelGGL(kernel, dim3(grid, 1), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)R, 0u, d_cyc);
    hipLaunchKernelGGL(kernel, dim3(grid, KVQ_CYCLES / W - 1u), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)R, 1u, d_cyc);
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

extern "C" const int64_t *kvq_scan_cycles(const kvq_scan *s) { return pass_result(s, KVQ_PASS_CYCLES); }

// ---- per-read distributions and duplication ----
extern "C" int64_t kvq_reads_len(void) { return KVQ_READS_WORDS; }
extern "C" int64_t kvq_dup_len(void) { return KVQ_DUP_WORDS; }

extern "C" int32_t kvq_scan_set_read_stats(kvq_scan *s, int32_t mode)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_read_stats"))) return rc;
    if (!mode) { reads_off(s); return KVQ_OK; }
    if (mode & ~(KVQ_READ_STATS | KVQ_READ_DUPLICATION)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_read_stats: mode is bit 0 (the distributions) and bit 1 (the duplication)");
        return KVQ_ERR_RUNTIME;
    }
    if (!s->passes[KVQ_PASS_PROFILE].on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_read_stats: the scan keeps no profile (the per-read statistics ride on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    const char *e = getenv("KVQ_DUP_SLOTS");
    const uint64_t slots = (mode & KVQ_READ_DUPLICATION) ? dup_slots_from(e ? atoll(e) : 0) : 0;
    if (mode != s->reads_mode || slots != s->dup_slots) reads_off(s);        // (a kept scan object asked for the same again keeps its buffers)
    const size_t words = (mode & KVQ_READ_STATS) ? KVQ_READS_WORDS : 0;
    if ((rc = pass_make(s->passes[KVQ_PASS_READS], words * 8, words, (size_t)(KVQ_READS_WORDS + KVQ_DUP_WORDS) * 8)) ||
        ((mode & KVQ_READ_DUPLICATION) && (rc = s->d_dup.ensure(KvqDupLayout::bytes(slots))))) { reads_off(s); return rc; }
    s->reads_mode = mode; s->dup_slots = slots;
    s->h_dup.clear();
    return pass_clear(s, KVQ_PASS_READS);
}

// the pass over the R records of a batch, behind its profile pass.  With the duplication the records go in slices of at most a
// quarter of the table's slots, the settle behind every slice: with at most half the slots taken in front of a slice the table
// is never more than three-quarters full, and no insert is ever refused
static int reads_enqueue(kvq_scan *s, const uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    const bool dup = (s->reads_mode & KVQ_READ_DUPLICATION) != 0;
    const KvqDupTable T = dup_table(s);
    const uint64_t slice = dup ? s->dup_slots / 4 : R;
    const uint32_t settle_grid = (uint32_t)std::min<uint64_t>(s->dup_slots / 256, KVQ_DUP_GRID_MAX);
    for (uint64_t r0 = 0; r0 < R; r0 += slice) {
        const uint64_t r1 = std::min(R, r0 + slice);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((r1 - r0 + 15) / 16, 2048);         // (the kernel strides over what there is)
        hipLaunchKernelGGL(kvq_reads_records, dim3(grid), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)r0, (uint32_t)r1,
                           (uint32_t)s->reads_mode, s->passes[KVQ_PASS_READS].d.as<unsigned long long>(), T);
        if (dup) {
            hipLaunchKernelGGL(kvq_dup_plan, dim3(settle_grid), dim3(256), 0, s->stream, T);
            hipLaunchKernelGGL(kvq_dup_purge, dim3(settle_grid), dim3(256), 0, s->stream, T);
        }
    }
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

extern "C" const int64_t *kvq_scan_reads(const kvq_scan *s) { return pass_result(s, KVQ_PASS_READS); }
extern "C" const int64_t *kvq_scan_dup(const kvq_scan *s) { return (s->reads_mode & KVQ_READ_DUPLICATION) && s->finished && !s->h_dup.empty() ? s->h_dup.data() : nullptr; }

// ---- overrepresented sequences ----
extern "C" int64_t kvq_over_len(void) { return KVQ_OVER_WORDS; }

extern "C" int32_t kvq_scan_set_overrepresented(kvq_scan *s, int32_t on)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_overrepresented"))) return rc;
    if (!on) { over_off(s); return KVQ_OK; }
    if (!s->passes[KVQ_PASS_PROFILE].on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_overrepresented: the scan keeps no profile (the overrepresented sequences ride on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    const char *e = getenv("KVQ_OVER_RECORDS");
    const uint64_t M = over_records_from(e ? atoll(e) : 0), slots = over_slots_from(M);
    if (slots != s->over_slots) over_off(s);                 // (a kept scan object asked for the same again keeps its buffers)
    if ((rc = pass_make(s->passes[KVQ_PASS_OVER], KvqOverLayout::bytes(slots), KVQ_OVER_WORDS, (size_t)KVQ_OVER_WORDS * 8))) { over_off(s); return rc; }
    s->over_M = M; s->over_slots = slots;
    return pass_clear(s, KVQ_PASS_OVER);
}

// the pass over the R records of a batch, behind its other passes: the records with a number below M make candidates (INSERT), the
// rest are looked up -- two launches for the one batch that M cuts, in that order on the scan's stream; one for every other
static int over_enqueue(kvq_scan *s, const uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    const uint64_t n_insert = std::min(R, s->over_seen < s->over_M ? s->over_M - s->over_seen : 0);
    const KvqOverTable T = over_table(s);
    const uint64_t cut[3] = { 0, n_insert, R };
    for (int mode = 0; mode < 2; mode++) {
        const uint64_t r0 = cut[mode], r1 = cut[mode + 1];
        if (r0 == r1) continue;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((r1 - r0 + 63) / 64, 2048);             // (the kernel strides over what there is)
        hipLaunchKernelGGL(kvq_over_records, dim3(grid), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)r0, (uint32_t)r1,
                           mode == 0 ? 1u : 0u, T);
    }
    KVQ_HIP(hipGetLastError());
    s->over_seen += R;
    return KVQ_OK;
}

extern "C" const int64_t *kvq_scan_over(const kvq_scan *s) { return pass_result(s, KVQ_PASS_OVER); }

// ---- adapter content ----
extern "C" int64_t kvq_adapt_len(void) { return KVQ_ADAPT_WORDS; }

extern "C" int32_t kvq_scan_set_adapters(kvq_scan *s, const uint8_t *const *probes, const int32_t *lens, int32_t n)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_adapters"))) return rc;
    if (n == 0) { adapt_off(s); return KVQ_OK; }
    if (!s->passes[KVQ_PASS_PROFILE].on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_adapters: the scan keeps no profile (the adapter content rides on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    if (!adapt_probes_ok("kvq_scan_set_adapters", probes, lens, n)) return KVQ_ERR_RUNTIME;
    if ((rc = pass_make(s->passes[KVQ_PASS_ADAPT], (size_t)KVQ_ADAPT_WORDS * 8, KVQ_ADAPT_WORDS, (size_t)KVQ_ADAPT_WORDS * 8))) { adapt_off(s); return rc; }
    s->adapt.assign(probes, lens, n);
    return pass_clear(s, KVQ_PASS_ADAPT);
}

// a probe set as the exact search takes it, by value: 2-bit codes, masks and lengths
static KvqAdaptProbes adapt_probes(const KvqProbeSet &S)
{
    KvqAdaptProbes P; memset(&P, 0, sizeof(P));
    P.n = (uint32_t)S.n;
    for (int k = 0; k < S.n; k++) {
        const uint32_t m = S.lens[k];
        for (uint32_t i = 0; i < m; i++) P.code[k] |= (unsigned long long)((S.probes[k][i] >> 1) & 3u) << (2u * i);
        P.mask[k] = m >= 32u ? ~0ull : (1ull << (2u * m)) - 1ull;               // (no shift by 64)
        P.m[k] = m;
    }
    return P;
}

// ---- probes that tolerate mismatches ----
extern "C" int32_t kvq_scan_set_adapter_mismatches(kvq_scan *s, int32_t per)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_adapter_mismatches"))) return rc;
    if (!adapt_per_ok("kvq_scan_set_adapter_mismatches", per)) return KVQ_ERR_RUNTIME;
    s->adapt_per = per;
    return KVQ_OK;
}
extern "C" int32_t kvq_scan_adapter_mismatches(const kvq_scan *s) { return s->adapt_per; }

// a probe set as the tolerant search takes it, by value: two planes of one bit a base, masks, lengths and budgets
static KvqAdaptProbesMm adapt_probes_mm(const KvqProbeSet &S, int32_t per)
{
    KvqAdaptProbesMm P; memset(&P, 0, sizeof(P));
    P.n = (uint32_t)S.n; P.per = (uint32_t)per;
    for (int k = 0; k < S.n; k++) {
        const uint32_t m = S.lens[k];
        for (uint32_t i = 0; i < m; i++) { P.lo[k] |= (uint32_t)((S.probes[k][i] >> 1) & 1u) << i; P.hi[k] |= (uint32_t)((S.probes[k][i] >> 2) & 1u) << i; }
        P.mask[k] = m >= 32u ? ~0u : (1u << m) - 1u;                            // (no shift by 32)
        P.m[k] = m; P.e[k] = m / (uint32_t)per;
    }
    return P;
}

// the pass over the R records of a batch, behind its other passes: the probes go along by value; with a mismatch rate, the
// instantiation for the tolerant probes in place of the one for the exact ones
template <class Probes> static int adapt_launch(kvq_scan *s, const uint8_t *d_data, uint64_t R, const Probes &P)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>((R + 15) / 16, 2048);               // (the kernel strides over what there is)
    hipLaunchKernelGGL(kvq_probe_kernels<Probes>(P.n).adapt, dim3(grid), dim3(256), (size_t)KvqAdaptLds::words(P.n) * 4, s->stream, d_data, s->d_nl4.as<uint32_t>(),
                       (uint32_t)R, P, s->passes[KVQ_PASS_ADAPT].d.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}
static int adapt_enqueue(kvq_scan *s, const uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    return s->adapt_per > 0 ? adapt_launch(s, d_data, R, adapt_probes_mm(s->adapt, s->adapt_per)) : adapt_launch(s, d_data, R, adapt_probes(s->adapt));
}

extern "C" const int64_t *kvq_scan_adapters(const kvq_scan *s) { return pass_result(s, KVQ_PASS_ADAPT); }

// ---- adapter clipping ----
// Its array goes through the lifecycle above (made, cleared, landed and given back as the others'), but the clip is no pass behind
// a batch's scan: its kernel runs in front of it (clip_text in kvq_scan.hip), and it needs no profile.
extern "C" int64_t kvq_clip_len(void) { return KVQ_CLIP_WORDS; }

static void clip_off(kvq_scan *s)
{
    s->clip.clear();
    pass_off(s, s->passes[KVQ_PASS_CLIP]);
}

extern "C" int32_t kvq_scan_set_clip(kvq_scan *s, const uint8_t *const *probes, const int32_t *lens, int32_t n)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_clip"))) return rc;
    if (n == 0) { clip_off(s); return KVQ_OK; }
    if (!adapt_probes_ok("kvq_scan_set_clip", probes, lens, n)) return KVQ_ERR_RUNTIME;
    if ((int)(int8_t)s->t->cfg.Amin <= (int)'!') {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_clip: Amin %d is not above '!' (33): a masked score would end no run, and the mask could not clip", (int)(int8_t)s->t->cfg.Amin);
        return KVQ_ERR_RUNTIME;
    }
    if ((rc = pass_make(s->passes[KVQ_PASS_CLIP], (size_t)KVQ_CLIP_WORDS * 8, KVQ_CLIP_WORDS, (size_t)KVQ_CLIP_WORDS * 8))) { clip_off(s); return rc; }
    s->clip.assign(probes, lens, n);
    return pass_clear(s, KVQ_PASS_CLIP);
}

// the clip over the R records of a batch whose index is on the scan's stream, in front of its scan: the text at d_data is written
template <class Probes> static int clip_launch(kvq_scan *s, uint8_t *d_data, uint64_t R, const Probes &P)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>((R + 15) / 16, 2048);               // (the kernel strides over what there is)
    hipLaunchKernelGGL(kvq_probe_kernels<Probes>(P.n).clip, dim3(grid), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)R, P,
                       s->passes[KVQ_PASS_CLIP].d.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}
static int clip_enqueue(kvq_scan *s, uint8_t *d_data, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    return s->adapt_per > 0 ? clip_launch(s, d_data, R, adapt_probes_mm(s->clip, s->adapt_per)) : clip_launch(s, d_data, R, adapt_probes(s->clip));
}

extern "C" const int64_t *kvq_scan_clip(const kvq_scan *s) { return pass_result(s, KVQ_PASS_CLIP); }

// ---- the reads the scan saw, as FastQ text ----
// Its eight words go through the lifecycle above; behind them in the pass's array lies the byte count of the batch in flight.
// Everything else is the emit's own: what kvq_emit_size says per record, the prefix sum's block sums, the offsets, the store.
extern "C" int64_t kvq_emit_len(void) { return KVQ_EMIT_WORDS; }

// where the pieces lie: the pass's device array (the words that land, the batch's total), its pinned buffer (the landing words,
// the total, the copies of the two guards), the store (a guard, the batch's bytes, a guard right behind the last of them)
struct KvqEmitLayout {
    static constexpr size_t D_TOTAL = KVQ_EMIT_WORDS, D_WORDS = 16, PIN_TOTAL = KVQ_EMIT_WORDS, PIN_GUARDS = 16, PIN_WORDS = 32;
    static constexpr size_t GUARD = 64, HALF = 8u << 20;
    static constexpr int GUARD_BYTE = 0xA5;
    static size_t store_bytes(size_t cap) { return GUARD + cap + GUARD + 16; }
};
static_assert(KvqEmitLayout::PIN_GUARDS * 8 + 2 * KvqEmitLayout::GUARD <= KvqEmitLayout::PIN_WORDS * 8, "the pieces of the emit's pinned buffer overlap");

// the deflate off: its buffers given back (the stream has been waited for)
static void deflate_off(kvq_scan *s)
{
    kvq_deflate_release(s->deflate); s->d_deflate_out.release();
    if (s->deflate_pin) pinned_give(s->deflate_pin, s->deflate_pin_cap);
    s->deflate_pin = nullptr; s->deflate_pin_cap = 0;
    for (auto &e : s->deflate_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    s->deflate_ev.clear(); s->deflate_ev_n = 0;
    for (int64_t &w : s->deflate_words) w = 0;
    s->emit_compress = false; s->emit_eof_done = false;
}

static void emit_off(kvq_scan *s)
{
    pass_off(s, s->passes[KVQ_PASS_EMIT]);               // (waits for the stream where there is anything to wait for)
    for (DevBuf *b : { &s->d_emit_rec, &s->d_emit_off, &s->d_emit_bsum, &s->d_emit_store }) b->release();
    if (s->emit_pin) pinned_give(s->emit_pin, s->emit_pin_cap);
    s->emit_pin = nullptr; s->emit_pin_cap = 0;
    for (hipEvent_t &e : s->emit_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    s->emit_sink.clear(); s->emit_sink.shrink_to_fit();
    s->emit_fd = -1; s->emit_min = 0; s->emit_guard_bad = 0;
    deflate_off(s);
}

extern "C" int32_t kvq_scan_set_emit(kvq_scan *s, int32_t on, int32_t min_length)
{
    int rc;
    kvq_clear_error();
    if ((rc = scan_idle(s, "kvq_scan_set_emit"))) return rc;
    if (!on) { emit_off(s); return KVQ_OK; }
    if (s->comm) {
        kvq_set_error(KVQ_ERR_RUNTIME, "the emitted reads are not gathered across ranks: a scan with a communicator cannot emit them");
        return KVQ_ERR_RUNTIME;
    }
    if ((rc = pass_make(s->passes[KVQ_PASS_EMIT], KvqEmitLayout::D_WORDS * 8, KVQ_EMIT_WORDS, KvqEmitLayout::PIN_WORDS * 8))) { emit_off(s); return rc; }
    if (!s->emit_pin) {
        s->emit_pin = (uint8_t *)pinned_take(2 * KvqEmitLayout::HALF, &s->emit_pin_cap);
        if (!s->emit_pin) { emit_off(s); kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    for (hipEvent_t &e : s->emit_ev)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; emit_off(s); kvq_set_error(KVQ_ERR_DEVICE, "hipEventCreate failed"); return KVQ_ERR_DEVICE; }
    s->emit_min = min_length < 0 ? std::max<int32_t>(s->t->cfg.minreadlength, 0) : min_length;
    return pass_clear(s, KVQ_PASS_EMIT);
}

extern "C" int32_t kvq_scan_set_emit_fd(kvq_scan *s, int32_t fd)
{
    kvq_clear_error();
    if (const int rc = scan_idle(s, "kvq_scan_set_emit_fd")) return rc;
    if (!s->passes[KVQ_PASS_EMIT].on) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_emit_fd: the scan emits nothing (kvq_scan_set_emit first)"); return KVQ_ERR_RUNTIME; }
    s->emit_fd = fd < 0 ? -1 : fd;
    return KVQ_OK;
}
extern "C" int32_t kvq_scan_set_emit_compress(kvq_scan *s, int32_t on)
{
    kvq_clear_error();
    if (const int rc = scan_idle(s, "kvq_scan_set_emit_compress")) return rc;
    if (!s->passes[KVQ_PASS_EMIT].on) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_emit_compress: the scan emits nothing (kvq_scan_set_emit first)"); return KVQ_ERR_RUNTIME; }
    if (!on) { (void)hipStreamSynchronize(s->stream); deflate_off(s); return KVQ_OK; }
    if (!s->deflate_pin) {
        s->deflate_pin = (int64_t *)pinned_take(16 * 8, &s->deflate_pin_cap);
        if (!s->deflate_pin) { kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    s->emit_compress = true; s->emit_eof_done = false;
    for (int64_t &w : s->deflate_words) w = 0;
    return KVQ_OK;
}
// the file descriptor is about to be closed by its owner (kvq_findseqs): the sink is the host buffer again, whatever the scan holds
static void emit_detach_fd(kvq_scan *s) { s->emit_fd = -1; }

// n bytes of emitted text to the sink
static int emit_append(kvq_scan *s, const uint8_t *p, size_t n)
{
    if (s->emit_fd < 0) { s->emit_sink.insert(s->emit_sink.end(), p, p + n); return KVQ_OK; }
    while (n) {
        const ssize_t w = write(s->emit_fd, p, n);
        if (w <= 0) { kvq_set_error(KVQ_ERR_IO, "cannot write the emitted reads"); return KVQ_ERR_IO; }
        p += w; n -= (size_t)w;
    }
    return KVQ_OK;
}

static int new_event_pair(kvq_scan *s, std::vector<KvqEventPair> &v);     // (kvq_scan.hip)

// BGZF(store[0, total)) of a batch into d_deflate_out, behind the emit's kernels on the scan's stream: ONE HOST
// WAIT for the compressed byte count and the batch's words, which join the scan's.  *src, *n: the stream that takes the text's
// place on the way to the sink.
static int emit_deflate(kvq_scan *s, const uint8_t *store, uint64_t total, const uint8_t **src, uint64_t *n)
{
    int rc;
    const uint64_t cap = kvq_deflate_bound_bytes(total);
    if ((rc = s->d_deflate_out.ensure((size_t)cap + 16))) return rc;
    if (s->deflate_ev_n == s->deflate_ev.size()) {
        KvqEventPair e(nullptr, nullptr);
        if (hipEventCreate(&e.first) != hipSuccess || hipEventCreate(&e.second) != hipSuccess) {
            if (e.first) (void)hipEventDestroy(e.first);
            kvq_set_error(KVQ_ERR_DEVICE, "hipEventCreate failed"); return KVQ_ERR_DEVICE;
        }
        s->deflate_ev.push_back(e);
    }
    const KvqEventPair &ev = s->deflate_ev[s->deflate_ev_n++];
    KVQ_HIP(hipEventRecord(ev.first, s->stream));
    if ((rc = kvq_deflate_enqueue(store, total, s->d_deflate_out.as<uint8_t>(), cap, s->deflate, s->stream))) return rc;
    KVQ_HIP(hipEventRecord(ev.second, s->stream));
    KVQ_HIP(hipMemcpyAsync(s->deflate_pin, s->deflate.words.p, 16 * 8, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    const int64_t *w = s->deflate_pin;
    const uint64_t out = (uint64_t)w[8];
    if (out > cap || out != (uint64_t)w[KVQ_DEFLATE_BYTES_OUT] || (uint64_t)w[KVQ_DEFLATE_BYTES_IN] != total) {
        kvq_set_error(KVQ_ERR_RUNTIME, "the deflate of %llu emitted bytes took %lld of them and made %llu bytes", (unsigned long long)total, (long long)w[KVQ_DEFLATE_BYTES_IN], (unsigned long long)out);
        return KVQ_ERR_RUNTIME;
    }
    for (int i = 0; i < KVQ_DEFLATE_WORDS; i++)
        s->deflate_words[i] = i == KVQ_DEFLATE_MAX_DISTANCE || i == KVQ_DEFLATE_MAX_LENGTH ? std::max(s->deflate_words[i], w[i]) : s->deflate_words[i] + w[i];
    *src = s->d_deflate_out.as<uint8_t>(); *n = out;
    return KVQ_OK;
}

// The emit of the R records of a batch of nbytes bytes whose index (nl4, rec_start) is on the scan's stream, behind its scan: the
// sizes, their prefix sum, ONE HOST WAIT for the batch's byte count, the copy into the store, and the store's bytes through the two
// halves of the pinned buffer to the sink -- the copy of a half runs while the half before it is appended.  The batch's emit is
// over when this returns: the store and the index are free for the next batch.
static int emit_enqueue(kvq_scan *s, const uint8_t *d_data, int64_t nbytes, uint64_t R)
{
    if (R == 0) return KVQ_OK;
    int rc;
    KvqPass &p = s->passes[KVQ_PASS_EMIT];
    const uint32_t nblocks = (uint32_t)((R + KVQ_EMIT_SCAN_BLOCK - 1) / KVQ_EMIT_SCAN_BLOCK);
    const size_t cap = (size_t)nbytes + (size_t)R;           // an emitted record is at most its input record plus one byte
    if ((rc = s->d_emit_rec.ensure((size_t)R * sizeof(KvqEmitRec))) || (rc = s->d_emit_off.ensure((size_t)R * 8)) ||
        (rc = s->d_emit_bsum.ensure((size_t)nblocks * 8)) || (rc = s->d_emit_store.ensure(KvqEmitLayout::store_bytes(cap)))) return rc;
    unsigned long long *const d_words = p.d.as<unsigned long long>(), *const d_total = d_words + KvqEmitLayout::D_TOTAL;
    KvqEmitRec *const d_rec = s->d_emit_rec.as<KvqEmitRec>();
    uint8_t *const store = s->d_emit_store.as<uint8_t>() + KvqEmitLayout::GUARD;
    const uint32_t sgrid = (uint32_t)std::min<uint64_t>(nblocks, 2048);                    // (the kernels stride over what there is)
    if ((rc = new_event_pair(s, p.ev))) return rc;
    KVQ_HIP(hipEventRecord(p.ev.back().first, s->stream));
    hipLaunchKernelGGL(kvq_emit_size, dim3((uint32_t)std::min<uint64_t>((R + 4 * KVQ_TRIM_RPW - 1) / (4 * KVQ_TRIM_RPW), 2048)), dim3(256), 0, s->stream, d_data,
                       s->d_nl4.as<uint32_t>(), s->d_rec_start.as<uint32_t>(), (uint32_t)R, (int32_t)s->t->cfg.Amin, (uint32_t)s->emit_min, d_rec, d_words);
    hipLaunchKernelGGL(kvq_emit_block_sums, dim3(sgrid), dim3(256), 0, s->stream, (const KvqEmitRec *)d_rec, (uint32_t)R, s->d_emit_bsum.as<unsigned long long>());
    hipLaunchKernelGGL(kvq_emit_scan_blocks, dim3(1), dim3(256), 0, s->stream, s->d_emit_bsum.as<unsigned long long>(), nblocks, d_total);
    hipLaunchKernelGGL(kvq_emit_offsets, dim3(sgrid), dim3(256), 0, s->stream, (const KvqEmitRec *)d_rec, (uint32_t)R,
                       (const unsigned long long *)s->d_emit_bsum.as<unsigned long long>(), s->d_emit_off.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    KVQ_HIP(hipEventRecord(p.ev.back().second, s->stream));
    KVQ_HIP(hipMemcpyAsync(p.pin + KvqEmitLayout::PIN_TOTAL, d_total, 8, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipStreamSynchronize(s->stream));
    const uint64_t total = (uint64_t)p.pin[KvqEmitLayout::PIN_TOTAL];
    if (total > cap) { kvq_set_error(KVQ_ERR_RUNTIME, "the emit of a batch of %lld bytes and %llu records sized itself at %llu bytes", (long long)nbytes, (unsigned long long)R, (unsigned long long)total); return KVQ_ERR_RUNTIME; }
    KVQ_HIP(hipMemsetAsync(store - KvqEmitLayout::GUARD, KvqEmitLayout::GUARD_BYTE, KvqEmitLayout::GUARD, s->stream));
    KVQ_HIP(hipMemsetAsync(store + total, KvqEmitLayout::GUARD_BYTE, KvqEmitLayout::GUARD, s->stream));
    if (total) {
        if ((rc = new_event_pair(s, p.ev))) return rc;
        KVQ_HIP(hipEventRecord(p.ev.back().first, s->stream));
        hipLaunchKernelGGL(kvq_emit_copy, dim3((uint32_t)std::min<uint64_t>((R + 15) / 16, 2048)), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(),
                           s->d_rec_start.as<uint32_t>(), (uint32_t)R, (const KvqEmitRec *)d_rec, (const unsigned long long *)s->d_emit_off.as<unsigned long long>(), store);
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipEventRecord(p.ev.back().second, s->stream));
    }
    uint8_t *const guards = (uint8_t *)(p.pin + KvqEmitLayout::PIN_GUARDS);
    KVQ_HIP(hipMemcpyAsync(guards, store - KvqEmitLayout::GUARD, KvqEmitLayout::GUARD, hipMemcpyDeviceToHost, s->stream));
    KVQ_HIP(hipMemcpyAsync(guards + KvqEmitLayout::GUARD, store + total, KvqEmitLayout::GUARD, hipMemcpyDeviceToHost, s->stream));
    const size_t H = KvqEmitLayout::HALF;
    size_t prev_n = 0;
    // (with kvq_scan_set_emit_compress the batch's BGZF stream takes the text's place from here on: the text stays on the device)
    const uint8_t *store_out = store; uint64_t total_out = total;
    if (s->emit_compress && total && (rc = emit_deflate(s, store, total, &store_out, &total_out))) return rc;
    for (uint64_t at = 0, i = 0; at < total_out; at += H, i++) {
        const size_t n = (size_t)std::min<uint64_t>(H, total_out - at);
        KVQ_HIP(hipMemcpyAsync(s->emit_pin + (i & 1) * H, store_out + at, n, hipMemcpyDeviceToHost, s->stream));
        KVQ_HIP(hipEventRecord(s->emit_ev[i & 1], s->stream));
        if (i) {
            KVQ_HIP(hipEventSynchronize(s->emit_ev[(i - 1) & 1]));
            if ((rc = emit_append(s, s->emit_pin + ((i - 1) & 1) * H, prev_n))) { (void)hipStreamSynchronize(s->stream); return rc; }
        }
        prev_n = n;
    }
    KVQ_HIP(hipStreamSynchronize(s->stream));
    if (total_out && (rc = emit_append(s, s->emit_pin + (((total_out - 1) / H) & 1) * H, prev_n))) return rc;
    for (size_t i = 0; i < 2 * KvqEmitLayout::GUARD; i++) s->emit_guard_bad += guards[i] != (uint8_t)KvqEmitLayout::GUARD_BYTE;
    return KVQ_OK;
}

extern "C" const int64_t *kvq_scan_emit(const kvq_scan *s) { return pass_result(s, KVQ_PASS_EMIT); }
extern "C" int64_t kvq_scan_emit_guard(const kvq_scan *s) { return s->passes[KVQ_PASS_EMIT].on ? s->emit_guard_bad : -1; }
extern "C" int32_t kvq_scan_emitted(const kvq_scan *s, const uint8_t **text, int64_t *nbytes)
{
    kvq_clear_error();
    if (text) *text = nullptr;
    if (nbytes) *nbytes = 0;
    if (!s->passes[KVQ_PASS_EMIT].on || !s->finished) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_emitted: only on a finished scan that kvq_scan_set_emit was turned on for");
        return KVQ_ERR_RUNTIME;
    }
    if (text && !s->emit_sink.empty()) *text = s->emit_sink.data();
    if (nbytes) *nbytes = (int64_t)s->emit_sink.size();
    return KVQ_OK;
}

// ---- the emit's deflate ----
extern "C" const int64_t *kvq_scan_emit_compress(const kvq_scan *s)
{
    return s->passes[KVQ_PASS_EMIT].on && s->emit_compress && s->finished ? s->deflate_words : nullptr;
}
extern "C" double kvq_scan_emit_deflate_kernel_ms(const kvq_scan *s)
{
    double total = 0;
    if (!s->emit_compress || !s->finished) return 0;
    for (size_t i = 0; i < s->deflate_ev_n; i++) { float ms = 0; if (hipEventElapsedTime(&ms, s->deflate_ev[i].first, s->deflate_ev[i].second) == hipSuccess) total += ms; }
    (void)hipGetLastError();
    return total;
}
