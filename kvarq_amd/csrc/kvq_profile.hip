// kvarq_amd/csrc/kvq_profile.hip -- the profile of the input (include/kvarq_hip.h), host side: the option of a
// scan object, the launch of kvq_profile_records behind a batch's kernels, its way to the host in the tail of a scan, and the
// CPU twin of the kernel (the definition in plain C++: test infrastructure, never a fallback)
#include "kvq_host.h"
#include <string.h>
#include <unordered_map>

extern "C" int64_t kvq_profile_len(int32_t ncut)
{
    return ncut < 0 || ncut > KVQ_PROFILE_MAX_CUTOFFS ? 0 : (int64_t)KVQ_PROF_CUTOFFS + (int64_t)ncut * KVQ_PROF_CUT_WORDS;
}

static void cycles_off(kvq_scan *s);
static void reads_off(kvq_scan *s);

extern "C" int32_t kvq_scan_set_profile(kvq_scan *s, const uint8_t *cutoffs, int32_t ncut)
{
    kvq_clear_error();
    if (!s->batches.empty() || s->copied_pending || s->host_pending >= 0) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_profile: only before the first batch or after kvq_scan_reset");
        return KVQ_ERR_RUNTIME;
    }
    if (ncut < 0) { s->profile_on = false; s->prof_ncut = 0; cycles_off(s); reads_off(s); return KVQ_OK; }
    if (ncut > KVQ_PROFILE_MAX_CUTOFFS || (ncut > 0 && !cutoffs)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_profile: at most %d cutoffs", KVQ_PROFILE_MAX_CUTOFFS);
        return KVQ_ERR_RUNTIME;
    }
    if (s->comm) {
        kvq_set_error(KVQ_ERR_RUNTIME, "the profile is not reduced across ranks: a scan with a communicator cannot keep one");
        return KVQ_ERR_RUNTIME;
    }
    int rc;
    const size_t bytes = (size_t)kvq_profile_len(ncut) * 8;
    if ((rc = s->d_prof.ensure(bytes))) return rc;
    if (s->pin_prof_cap < bytes) {
        if (s->pin_prof) pinned_give(s->pin_prof, s->pin_prof_cap);
        s->pin_prof = (int64_t *)pinned_take(bytes, &s->pin_prof_cap);
        if (!s->pin_prof) { s->pin_prof_cap = 0; kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    s->profile_on = true; s->prof_ncut = ncut;
    memset(s->prof_cuts, 0, sizeof(s->prof_cuts));
    if (ncut) memcpy(s->prof_cuts, cutoffs, (size_t)ncut);
    s->h_prof.clear();
    KVQ_HIP(hipMemsetAsync(s->d_prof.p, 0, bytes, s->stream));
    return KVQ_OK;
}

// the device array back to zero: wherever the hit arena is cleared (reset_device_state), so that a replay, a rescan round and
// a file read again count every record once
static int profile_clear(kvq_scan *s)
{
    KVQ_HIP(hipMemsetAsync(s->d_prof.p, 0, (size_t)kvq_profile_len(s->prof_ncut) * 8, s->stream));
    return KVQ_OK;
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
                       s->d_nl4.as<uint32_t>(), (uint32_t)R, C, spread ? 1u : 0u, s->d_prof.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

// the tail of a scan: the array on its way to the host (finish_once waits for the tail)
static int profile_tail(kvq_scan *s)
{
    KVQ_HIP(hipMemcpyAsync(s->pin_prof, s->d_prof.p, (size_t)kvq_profile_len(s->prof_ncut) * 8, hipMemcpyDeviceToHost, s->stream));
    return KVQ_OK;
}
static void profile_landed(kvq_scan *s) { s->h_prof.assign(s->pin_prof, s->pin_prof + kvq_profile_len(s->prof_ncut)); }

extern "C" const int64_t *kvq_scan_profile(const kvq_scan *s) { return s->profile_on && s->finished && !s->h_prof.empty() ? s->h_prof.data() : nullptr; }
extern "C" int32_t kvq_scan_profile_cutoffs(const kvq_scan *s, uint8_t *cutoffs8)
{
    if (!s->profile_on) return -1;
    if (cutoffs8 && s->prof_ncut) memcpy(cutoffs8, s->prof_cuts, (size_t)s->prof_ncut);
    return s->prof_ncut;
}

// ---- per-cycle counts (include/kvarq_hip.h): the same four steps beside the profile's ----
extern "C" int64_t kvq_cycles_len(void) { return 2 * (int64_t)KVQ_CYCLES * 256; }
static size_t cycles_device_bytes() { return ((size_t)kvq_cycles_len() + 1) * 8; }       // (the kernel's scratch word behind the array)

static void cycles_off(kvq_scan *s)
{
    if (s->d_cyc.p) (void)hipStreamSynchronize(s->stream);       // (a reset has enqueued its clearing: the block goes back to a cache other streams take from)
    if (s->pin_cyc) pinned_give(s->pin_cyc, s->pin_cyc_cap);
    s->pin_cyc = nullptr; s->pin_cyc_cap = 0;
    s->d_cyc.release();
    s->h_cyc.clear(); s->h_cyc.shrink_to_fit();
    s->cycles_on = false;
}

static int cycles_clear(kvq_scan *s)
{
    KVQ_HIP(hipMemsetAsync(s->d_cyc.p, 0, cycles_device_bytes(), s->stream));
    return KVQ_OK;
}

extern "C" int32_t kvq_scan_set_cycles(kvq_scan *s, int32_t on)
{
    kvq_clear_error();
    if (!s->batches.empty() || s->copied_pending || s->host_pending >= 0) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_cycles: only before the first batch or after kvq_scan_reset");
        return KVQ_ERR_RUNTIME;
    }
    if (!on) { cycles_off(s); return KVQ_OK; }
    if (!s->profile_on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_cycles: the scan keeps no profile (the cycles ride on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    int rc;
    if ((rc = s->d_cyc.ensure(cycles_device_bytes()))) return rc;
    const size_t bytes = (size_t)kvq_cycles_len() * 8;
    if (s->pin_cyc_cap < bytes) {
        if (s->pin_cyc) pinned_give(s->pin_cyc, s->pin_cyc_cap);
        s->pin_cyc = (int64_t *)pinned_take(bytes, &s->pin_cyc_cap);
        if (!s->pin_cyc) { s->pin_cyc_cap = 0; s->d_cyc.release(); kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    s->cycles_on = true;
    s->h_cyc.clear();
    return cycles_clear(s);
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
    hipLaunchKernelGGL(kernel, dim3(grid, 1), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)R, 0u, s->d_cyc.as<unsigned long long>());
    hipLaunchKernelGGL(kernel, dim3(grid, KVQ_CYCLES / W - 1u), dim3(256), 0, s->stream, d_data, s->d_nl4.as<uint32_t>(), (uint32_t)R, 1u, s->d_cyc.as<unsigned long long>());
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

static int cycles_tail(kvq_scan *s)
{
    KVQ_HIP(hipMemcpyAsync(s->pin_cyc, s->d_cyc.p, (size_t)kvq_cycles_len() * 8, hipMemcpyDeviceToHost, s->stream));
    return KVQ_OK;
}
static void cycles_landed(kvq_scan *s) { s->h_cyc.assign(s->pin_cyc, s->pin_cyc + kvq_cycles_len()); }

extern "C" const int64_t *kvq_scan_cycles(const kvq_scan *s) { return s->cycles_on && s->finished && !s->h_cyc.empty() ? s->h_cyc.data() : nullptr; }

// ---- per-read distributions and duplication (include/kvarq_hip.h): the same steps once more ----
extern "C" int64_t kvq_reads_len(void) { return KVQ_READS_WORDS; }
extern "C" int64_t kvq_dup_len(void) { return KVQ_DUP_WORDS; }

// C from a wish: the default, or what the wish shrinks it to -- no less than KVQ_DUP_MIN_SLOTS, rounded down to a power of two
static uint64_t dup_slots_from(long long wish)
{
    if (wish <= 0 || wish >= KVQ_DUP_DEFAULT_SLOTS) return KVQ_DUP_DEFAULT_SLOTS;
    uint64_t c = KVQ_DUP_MIN_SLOTS;
    while (2 * c <= (uint64_t)wish) c *= 2;
    return c;
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

static void reads_off(kvq_scan *s)
{
    if (s->d_reads.p || s->d_dup.p) (void)hipStreamSynchronize(s->stream);       // (as cycles_off: a reset has enqueued their clearing)
    if (s->pin_reads) pinned_give(s->pin_reads, s->pin_reads_cap);
    s->pin_reads = nullptr; s->pin_reads_cap = 0;
    s->d_reads.release(); s->d_dup.release();
    s->h_reads.clear(); s->h_reads.shrink_to_fit(); s->h_dup.clear(); s->h_dup.shrink_to_fit();
    s->reads_mode = 0; s->dup_slots = 0;
}

// the array AND the table back to zero: wherever the profile is cleared, so that a replay, a rescan round and a file read again
// count every record once (a zero state block is level 0 with table 0 active)
static int reads_clear(kvq_scan *s)
{
    if (s->reads_mode & KVQ_READ_STATS) KVQ_HIP(hipMemsetAsync(s->d_reads.p, 0, (size_t)KVQ_READS_WORDS * 8, s->stream));
    if (s->reads_mode & KVQ_READ_DUPLICATION) KVQ_HIP(hipMemsetAsync(s->d_dup.p, 0, KvqDupLayout::bytes(s->dup_slots), s->stream));
    return KVQ_OK;
}

extern "C" int32_t kvq_scan_set_read_stats(kvq_scan *s, int32_t mode)
{
    kvq_clear_error();
    if (!s->batches.empty() || s->copied_pending || s->host_pending >= 0) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_read_stats: only before the first batch or after kvq_scan_reset");
        return KVQ_ERR_RUNTIME;
    }
    if (!mode) { reads_off(s); return KVQ_OK; }
    if (mode & ~(KVQ_READ_STATS | KVQ_READ_DUPLICATION)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_read_stats: mode is bit 0 (the distributions) and bit 1 (the duplication)");
        return KVQ_ERR_RUNTIME;
    }
    if (!s->profile_on) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_read_stats: the scan keeps no profile (the per-read statistics ride on its record set and index: kvq_scan_set_profile first)");
        return KVQ_ERR_RUNTIME;
    }
    const char *e = getenv("KVQ_DUP_SLOTS");
    const uint64_t slots = (mode & KVQ_READ_DUPLICATION) ? dup_slots_from(e ? atoll(e) : 0) : 0;
    if (mode != s->reads_mode || slots != s->dup_slots) reads_off(s);        // (a kept scan object asked for the same again keeps its buffers)
    int rc;
    if ((mode & KVQ_READ_STATS) && (rc = s->d_reads.ensure((size_t)KVQ_READS_WORDS * 8))) return rc;
    if ((mode & KVQ_READ_DUPLICATION) && (rc = s->d_dup.ensure(KvqDupLayout::bytes(slots)))) { reads_off(s); return rc; }
    const size_t bytes = (size_t)(KVQ_READS_WORDS + KVQ_DUP_WORDS) * 8;
    if (s->pin_reads_cap < bytes) {
        if (s->pin_reads) pinned_give(s->pin_reads, s->pin_reads_cap);
        s->pin_reads = (int64_t *)pinned_take(bytes, &s->pin_reads_cap);
        if (!s->pin_reads) { s->pin_reads_cap = 0; reads_off(s); kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for results"); return KVQ_ERR_MEMORY; }
    }
    s->reads_mode = mode; s->dup_slots = slots;
    s->h_reads.clear(); s->h_dup.clear();
    return reads_clear(s);
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
                           (uint32_t)s->reads_mode, s->d_reads.as<unsigned long long>(), T);
        if (dup) {
            hipLaunchKernelGGL(kvq_dup_plan, dim3(settle_grid), dim3(256), 0, s->stream, T);
            hipLaunchKernelGGL(kvq_dup_purge, dim3(settle_grid), dim3(256), 0, s->stream, T);
        }
    }
    KVQ_HIP(hipGetLastError());
    return KVQ_OK;
}

// the tail of a scan: the array, and what kvq_dup_levels makes of the active table, on their way to the host
static int reads_tail(kvq_scan *s)
{
    if (s->reads_mode & KVQ_READ_STATS)
        KVQ_HIP(hipMemcpyAsync(s->pin_reads, s->d_reads.p, (size_t)KVQ_READS_WORDS * 8, hipMemcpyDeviceToHost, s->stream));
    if (s->reads_mode & KVQ_READ_DUPLICATION) {
        unsigned long long *res = (unsigned long long *)((char *)s->d_dup.p + KvqDupLayout::RESULT);
        KVQ_HIP(hipMemsetAsync(res, 0, (size_t)KVQ_DUP_WORDS * 8, s->stream));
        hipLaunchKernelGGL(kvq_dup_levels, dim3((uint32_t)std::min<uint64_t>(s->dup_slots / 256, KVQ_DUP_GRID_MAX)), dim3(256), 0, s->stream, dup_table(s), res);
        KVQ_HIP(hipGetLastError());
        KVQ_HIP(hipMemcpyAsync(s->pin_reads + KVQ_READS_WORDS, res, (size_t)KVQ_DUP_WORDS * 8, hipMemcpyDeviceToHost, s->stream));
    }
    return KVQ_OK;
}
static void reads_landed(kvq_scan *s)
{
    if (s->reads_mode & KVQ_READ_STATS) s->h_reads.assign(s->pin_reads, s->pin_reads + KVQ_READS_WORDS);
    if (s->reads_mode & KVQ_READ_DUPLICATION) s->h_dup.assign(s->pin_reads + KVQ_READS_WORDS, s->pin_reads + KVQ_READS_WORDS + KVQ_DUP_WORDS);
}

extern "C" const int64_t *kvq_scan_reads(const kvq_scan *s) { return (s->reads_mode & KVQ_READ_STATS) && s->finished && !s->h_reads.empty() ? s->h_reads.data() : nullptr; }
extern "C" const int64_t *kvq_scan_dup(const kvq_scan *s) { return (s->reads_mode & KVQ_READ_DUPLICATION) && s->finished && !s->h_dup.empty() ? s->h_dup.data() : nullptr; }

// ---- the twins ----
extern "C" uint64_t kvq_dup_hash_host(const uint8_t *line, int64_t L) { return line && L > 0 ? kvq_dup_hash(line, (uint64_t)L) : 0; }

extern "C" int32_t kvq_reads_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t slots,
                                  int64_t *reads_out, int64_t *dup_out)
{
    kvq_clear_error();
    bool ok = nbytes >= 0 && nchunks >= 0 && (nchunks == 0 || chunk_off);
    for (int64_t c = 0; ok && c <= nchunks && nchunks > 0; c++) ok = chunk_off[c] >= 0 && chunk_off[c] <= nbytes && (!c || chunk_off[c] >= chunk_off[c - 1]);
    if (!ok) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_reads_host: bad arguments"); return KVQ_ERR_RUNTIME; }
    std::unordered_map<uint64_t, int64_t> keys;                                // every key of the input with its count
    int64_t keyed = 0, unkeyed = 0;
    for (int64_t c = 0; c < nchunks; c++) {
        int64_t nl[4]; int have = 0;
        for (int64_t i = chunk_off[c]; i < chunk_off[c + 1]; i++) {
            if (text[i] != '\n') continue;
            nl[have++] = i;
            if (have < 4) continue;                                            // a complete record of the chunk
            have = 0;
            const uint8_t *bases = text + nl[0] + 1, *scores = text + nl[2] + 1;
            int64_t L = nl[1] - nl[0] - 1, Q = nl[3] - nl[2] - 1;
            if (L > 0 && bases[L - 1] == '\r') L--;                            // a trailing '\r' is not part of its line
            if (Q > 0 && scores[Q - 1] == '\r') Q--;
            if (reads_out) {
                int64_t a = 0, g = 0, n = 0, S = 0;
                for (int64_t j = 0; j < L; j++) {
                    const uint8_t b = bases[j];
                    a += b == 'A' || b == 'C' || b == 'G' || b == 'T'; g += b == 'G' || b == 'C'; n += b == 'N';
                }
                for (int64_t j = 0; j < Q; j++) S += scores[j];
                reads_out[KVQ_READS_RECORDS]++;
                if (a > 0) reads_out[KVQ_READS_GC + (200 * g + a) / (2 * a)]++; else reads_out[KVQ_READS_GC_NONE]++;
                if (Q > 0) reads_out[KVQ_READS_MEANQ + (2 * S + Q) / (2 * Q)]++; else reads_out[KVQ_READS_MEANQ_NONE]++;
                reads_out[KVQ_READS_NCOUNT + std::min<int64_t>(n, 255)]++;
            }
            if (dup_out) {
                if (L == 0) unkeyed++;
                else { keyed++; keys[kvq_dup_hash(bases, (uint64_t)L)]++; }
            }
        }
    }
    if (!dup_out) return KVQ_OK;
    const uint64_t C = dup_slots_from(slots);
    uint32_t level = 0;
    for (;; level++) {                                                          // the smallest level with at most C / 2 distinct tracked keys
        uint64_t tracked = 0;
        for (const auto &k : keys) tracked += kvq_dup_tracked(k.first, level);
        if (tracked <= C / 2) break;
    }
    memset(dup_out, 0, (size_t)KVQ_DUP_WORDS * 8);
    dup_out[KVQ_DUP_LEVEL] = level; dup_out[KVQ_DUP_SLOTS] = (int64_t)C; dup_out[KVQ_DUP_KEYED] = keyed; dup_out[KVQ_DUP_UNKEYED] = unkeyed;
    for (const auto &k : keys) {
        if (!kvq_dup_tracked(k.first, level)) continue;
        const uint32_t b = kvq_dup_bin((uint64_t)k.second);
        dup_out[KVQ_DUP_DISTINCT + b]++; dup_out[KVQ_DUP_RECORDS + b] += k.second;
        dup_out[KVQ_DUP_TRACKED_KEYS]++; dup_out[KVQ_DUP_TRACKED_RECORDS] += k.second;
    }
    return KVQ_OK;
}

extern "C" int32_t kvq_cycles_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t *out)
{
    kvq_clear_error();
    bool ok = out && nbytes >= 0 && nchunks >= 0 && (nchunks == 0 || chunk_off);
    for (int64_t c = 0; ok && c <= nchunks && nchunks > 0; c++) ok = chunk_off[c] >= 0 && chunk_off[c] <= nbytes && (!c || chunk_off[c] >= chunk_off[c - 1]);
    if (!ok) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_cycles_host: bad arguments"); return KVQ_ERR_RUNTIME; }
    int64_t *const score = out, *const base = out + (int64_t)KVQ_CYCLES * 256;
    for (int64_t c = 0; c < nchunks; c++) {
        int64_t nl[4]; int have = 0;
        for (int64_t i = chunk_off[c]; i < chunk_off[c + 1]; i++) {
            if (text[i] != '\n') continue;
            nl[have++] = i;
            if (have < 4) continue;                                            // a complete record of the chunk
            have = 0;
            for (int64_t p = 0; p < KVQ_CYCLES && nl[0] + 1 + p < nl[1]; p++) base[p * 256 + text[nl[0] + 1 + p]]++;
            for (int64_t p = 0; p < KVQ_CYCLES && nl[2] + 1 + p < nl[3]; p++) score[p * 256 + text[nl[2] + 1 + p]]++;
        }
    }
    return KVQ_OK;
}

extern "C" int32_t kvq_profile_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                    const uint8_t *cutoffs, int32_t ncut, int64_t *out)
{
    kvq_clear_error();
    bool ok = out && nbytes >= 0 && nchunks >= 0 && ncut >= 0 && ncut <= KVQ_PROFILE_MAX_CUTOFFS && (ncut == 0 || cutoffs) && (nchunks == 0 || chunk_off);
    for (int64_t c = 0; ok && c <= nchunks && nchunks > 0; c++) ok = chunk_off[c] >= 0 && chunk_off[c] <= nbytes && (!c || chunk_off[c] >= chunk_off[c - 1]);
    if (!ok) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_profile_host: bad arguments"); return KVQ_ERR_RUNTIME; }
    auto raise = [&](int at, int64_t v) { if (v > out[at]) out[at] = v; };
    std::vector<int64_t> nl;
    for (int64_t c = 0; c < nchunks; c++) {
        nl.clear();
        for (int64_t i = chunk_off[c]; i < chunk_off[c + 1]; i++) if (text[i] == '\n') nl.push_back(i);
        for (size_t r = 0; r + 4 <= nl.size(); r += 4) {                       // the complete records of the chunk
            const int64_t n0 = nl[r], n1 = nl[r + 1], n2 = nl[r + 2], n3 = nl[r + 3];
            const int64_t L = n1 - n0 - 1, Q = n3 - n2 - 1;
            out[KVQ_PROF_RECORDS]++; out[KVQ_PROF_BASE_LINE_BYTES] += L; out[KVQ_PROF_SCORE_LINE_BYTES] += Q; out[KVQ_PROF_MISMATCHED] += L != Q;
            raise(KVQ_PROF_LONGEST, L + 1);
            out[KVQ_PROF_RAW_LENGTHS + std::min<int64_t>(L, KVQ_PROF_RAW_BINS - 1)]++;
            for (int64_t i = n0 + 1; i < n1; i++) out[KVQ_PROF_BASE_BYTES + text[i]]++;
            for (int64_t i = n2 + 1; i < n3; i++) out[KVQ_PROF_SCORE_BYTES + text[i]]++;
            for (int k = 0; k < ncut; k++) {
                // workhorse.c:1055-1068 over the score line and its newline
                const int amin = (int8_t)cutoffs[k];
                int64_t run = n2 + 1, best = 0;
                for (int64_t i = n2 + 1; i <= n3; i++) {
                    if ((int)(int8_t)text[i] >= amin) { if (run < 0) run = i; }
                    else { if (run >= 0 && i - run > best) best = i - run; run = -1; }
                }
                int64_t *const cut = out + KVQ_PROF_CUTOFFS + (int64_t)k * KVQ_PROF_CUT_WORDS;
                if (best < KVQ_MAX_READLENGTH) cut[1 + best]++;                 // add_rl, workhorse.c:394-402
                if (best + 1 > cut[0]) cut[0] = best + 1;
            }
        }
    }
    return KVQ_OK;
}
