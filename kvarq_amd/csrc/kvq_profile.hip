// kvarq_amd/csrc/kvq_profile.hip -- the profile of the input (include/kvarq_hip.h), host side: the option of a
// scan object, the launch of kvq_profile_records behind a batch's kernels, its way to the host in the tail of a scan, and the
// CPU twin of the kernel (the definition in plain C++: test infrastructure, never a fallback)
#include "kvq_host.h"
#include <string.h>

extern "C" int64_t kvq_profile_len(int32_t ncut)
{
    return ncut < 0 || ncut > KVQ_PROFILE_MAX_CUTOFFS ? 0 : (int64_t)KVQ_PROF_CUTOFFS + (int64_t)ncut * KVQ_PROF_CUT_WORDS;
}

static void cycles_off(kvq_scan *s);

extern "C" int32_t kvq_scan_set_profile(kvq_scan *s, const uint8_t *cutoffs, int32_t ncut)
{
    kvq_clear_error();
    if (!s->batches.empty() || s->copied_pending || s->host_pending >= 0) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_scan_set_profile: only before the first batch or after kvq_scan_reset");
        return KVQ_ERR_RUNTIME;
    }
    if (ncut < 0) { s->profile_on = false; s->prof_ncut = 0; cycles_off(s); return KVQ_OK; }
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

// ---- the twins ----
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
