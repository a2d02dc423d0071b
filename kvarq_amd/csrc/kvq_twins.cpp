// kvarq_amd/csrc/kvq_twins.cpp -- the CPU twins of the input passes, of the adapter clip and of the emit (include/kvarq_hip.h, DESIGN
// sections 13, 14, 16, 17, 18, 19, 20 and 21): the definitions of kvq_profile_records, kvq_profile_cycles, kvq_reads_records,
// kvq_over_records, kvq_adapt_records, kvq_clip_records, kvq_adapt_records_mm, kvq_clip_records_mm and of the kernels of
// kernels_emit.hip in plain C++ (test infrastructure, never a fallback).  Nothing of HIP: the file also compiles on its own.  One
// argument check serves all nine and one record walk the first eight (the emit walks with the record's first byte beside its newlines).
#include "../../include/kvarq_hip.h"
#include "kvq_dup_hash.h"
#include "kvq_deflate.h"
#include <algorithm>
#include <string.h>
#include <unordered_map>
#include <utility>
#include <vector>

void kvq_set_error(int code, const char *fmt, ...);      // (kvq_runtime.hip)
void kvq_clear_error();

// C from a wish: the default, or what the wish shrinks it to -- no less than KVQ_DUP_MIN_SLOTS, rounded down to a power of two
// (kvq_scan_set_read_stats sizes the device's tables with it)
static uint64_t dup_slots_from(long long wish)
{
    if (wish <= 0 || wish >= KVQ_DUP_DEFAULT_SLOTS) return KVQ_DUP_DEFAULT_SLOTS;
    uint64_t c = KVQ_DUP_MIN_SLOTS;
    while (2 * c <= (uint64_t)wish) c *= 2;
    return c;
}

// M of the overrepresented sequences from a wish: the default, or the wish clamped (kvq_scan_set_overrepresented reads it from
// KVQ_OVER_RECORDS); the slots of a table for M candidates: four times M rounded up to a power of two, at least 1024
static uint64_t over_records_from(long long wish)
{
    if (wish <= 0) return KVQ_OVER_DEFAULT_RECORDS;
    return (uint64_t)std::min<long long>(std::max<long long>(wish, KVQ_OVER_MIN_RECORDS), KVQ_OVER_MAX_RECORDS);
}
static uint64_t over_slots_from(uint64_t M)
{
    uint64_t c = 256;
    while (c < M) c *= 2;
    return 4 * c;
}

// what every twin asks of its text and chunk table (`ok`: what it asks beyond that)
static bool twin_args(const char *who, bool ok, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks)
{
    kvq_clear_error();
    ok = ok && nbytes >= 0 && nchunks >= 0 && (nchunks == 0 || chunk_off);
    for (int64_t c = 0; ok && c <= nchunks && nchunks > 0; c++) ok = chunk_off[c] >= 0 && chunk_off[c] <= nbytes && (!c || chunk_off[c] >= chunk_off[c - 1]);
    if (!ok) kvq_set_error(KVQ_ERR_RUNTIME, "%s: bad arguments", who);
    return ok;
}

// every four newlines of a chunk are a record: fn(n0, n1, n2, n3), their offsets (an incomplete tail of a chunk is no record)
template <class F> static void for_each_record(const uint8_t *text, const int64_t *chunk_off, int64_t nchunks, F fn)
{
    for (int64_t c = 0; c < nchunks; c++) {
        int64_t nl[4]; int have = 0;
        for (int64_t i = chunk_off[c]; i < chunk_off[c + 1]; i++) {
            if (text[i] != '\n') continue;
            nl[have++] = i;
            if (have == 4) { have = 0; fn(nl[0], nl[1], nl[2], nl[3]); }
        }
    }
}

extern "C" uint64_t kvq_dup_hash_host(const uint8_t *line, int64_t L) { return line && L > 0 ? kvq_dup_hash(line, (uint64_t)L) : 0; }

extern "C" int32_t kvq_reads_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t slots,
                                  int64_t *reads_out, int64_t *dup_out)
{
    if (!twin_args("kvq_reads_host", true, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    std::unordered_map<uint64_t, int64_t> keys;                                // every key of the input with its count
    int64_t keyed = 0, unkeyed = 0;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t n2, int64_t n3) {
        const uint8_t *bases = text + n0 + 1, *scores = text + n2 + 1;
        int64_t L = n1 - n0 - 1, Q = n3 - n2 - 1;
        if (L > 0 && bases[L - 1] == '\r') L--;                                // a trailing '\r' is not part of its line
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
    });
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

extern "C" int32_t kvq_over_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t records_limit,
                                 int64_t *out)
{
    if (!twin_args("kvq_over_host", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    struct Cand { int64_t count = 0, n = 0; uint8_t key[KVQ_DUP_KEY_BYTES] = { 0 }; };
    const uint64_t M = over_records_from(records_limit);
    std::unordered_map<uint64_t, Cand> cands;                                  // the keys of the first M records, by their hash
    int64_t keyed = 0, unkeyed = 0;
    uint64_t number = 0;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t, int64_t) {
        const uint8_t *bases = text + n0 + 1;
        int64_t L = n1 - n0 - 1;
        if (L > 0 && bases[L - 1] == '\r') L--;                                // a trailing '\r' is not part of its line
        const uint64_t mine = number++;
        if (L == 0) { unkeyed++; return; }
        keyed++;
        const uint64_t h = kvq_dup_hash(bases, (uint64_t)L);
        auto at = cands.find(h);
        if (at == cands.end()) {
            if (mine >= M) return;                                              // no candidate: counted nowhere but in `keyed`
            at = cands.emplace(h, Cand()).first;                                // (the bytes of whichever key came first to the hash)
            at->second.n = std::min<int64_t>(L, KVQ_DUP_KEY_BYTES);
            memcpy(at->second.key, bases, (size_t)at->second.n);
        }
        at->second.count++;
    });
    memset(out, 0, (size_t)KVQ_OVER_WORDS * 8);
    out[KVQ_OVER_M] = (int64_t)M; out[KVQ_OVER_SLOTS] = (int64_t)over_slots_from(M); out[KVQ_OVER_KEYED] = keyed; out[KVQ_OVER_UNKEYED] = unkeyed;
    std::vector<std::pair<uint64_t, const Cand *>> listed;
    for (const auto &c : cands) {
        out[KVQ_OVER_CANDIDATES]++; out[KVQ_OVER_COUNTED] += c.second.count;
        if (c.second.count >= 2 && 1000 * c.second.count >= keyed) listed.emplace_back(c.first, &c.second);
    }
    std::sort(listed.begin(), listed.end(), [](const std::pair<uint64_t, const Cand *> &a, const std::pair<uint64_t, const Cand *> &b) {
        return a.second->count != b.second->count ? a.second->count > b.second->count : a.first < b.first;
    });
    out[KVQ_OVER_LISTED] = (int64_t)listed.size();                              // (at most KVQ_OVER_MAX_ROWS: the counts sum to at most `keyed`)
    for (size_t r = 0; r < listed.size(); r++) {
        int64_t *row = out + KVQ_OVER_ROWS + (int64_t)r * KVQ_OVER_ROW_WORDS;
        row[KVQ_OVER_ROW_HASH] = (int64_t)listed[r].first; row[KVQ_OVER_ROW_COUNT] = listed[r].second->count; row[KVQ_OVER_ROW_N] = listed[r].second->n;
        for (int i = 0; i < 8; i++) {
            uint64_t w = 0;
            for (int j = 0; j < 8; j++) w |= (uint64_t)listed[r].second->key[8 * i + j] << (8 * j);
            row[KVQ_OVER_ROW_KEY + i] = (int64_t)w;
        }
    }
    return KVQ_OK;
}

// what kvq_scan_set_adapters and kvq_adapt_host ask of their probes: 1 .. KVQ_ADAPT_MAX_PROBES of them, KVQ_ADAPT_MIN_PROBE ..
// KVQ_ADAPT_MAX_PROBE bytes each, every byte an upper-case A C G T
static bool adapt_probes_ok(const char *who, const uint8_t *const *probes, const int32_t *lens, int32_t n)
{
    bool ok = n >= 1 && n <= KVQ_ADAPT_MAX_PROBES && probes && lens;
    for (int32_t k = 0; ok && k < n; k++) {
        ok = probes[k] && lens[k] >= KVQ_ADAPT_MIN_PROBE && lens[k] <= KVQ_ADAPT_MAX_PROBE;
        for (int32_t i = 0; ok && i < lens[k]; i++) ok = probes[k][i] == 'A' || probes[k][i] == 'C' || probes[k][i] == 'G' || probes[k][i] == 'T';
    }
    if (!ok) kvq_set_error(KVQ_ERR_RUNTIME, "%s: 1 to %d probes of %d to %d bytes, every byte one of upper-case A C G T", who,
                           KVQ_ADAPT_MAX_PROBES, KVQ_ADAPT_MIN_PROBE, KVQ_ADAPT_MAX_PROBE);
    return ok;
}

extern "C" int32_t kvq_adapt_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                  const uint8_t *const *probes, const int32_t *lens, int32_t n, int64_t *out)
{
    if (!twin_args("kvq_adapt_host", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    if (!adapt_probes_ok("kvq_adapt_host", probes, lens, n)) return KVQ_ERR_RUNTIME;
    out[KVQ_ADAPT_N] = n;
    for (int32_t k = 0; k < n; k++) out[KVQ_ADAPT_BLOCKS + (int64_t)k * KVQ_ADAPT_BLOCK_WORDS + KVQ_ADAPT_B_M] = lens[k];
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t, int64_t) {
        const uint8_t *line = text + n0 + 1;
        int64_t L = n1 - n0 - 1;
        if (L > 0 && line[L - 1] == '\r') L--;                                 // a trailing '\r' is not part of its line
        int64_t clip = L;
        bool full = false, tailed = false;
        for (int32_t k = 0; k < n; k++) {
            int64_t *const blk = out + KVQ_ADAPT_BLOCKS + (int64_t)k * KVQ_ADAPT_BLOCK_WORDS;
            const int64_t m = lens[k];
            int64_t first = -1, tail = -1;
            for (int64_t p = 0; first < 0 && p + m <= L; p++) if (!memcmp(line + p, probes[k], (size_t)m)) first = p;
            for (int64_t t = std::min(m - 1, L); first < 0 && tail < 0 && t >= KVQ_ADAPT_MIN_TAIL; t--)
                if (!memcmp(line + L - t, probes[k], (size_t)t)) tail = t;
            if (first >= 0) {
                full = true; clip = std::min(clip, first);
                blk[KVQ_ADAPT_B_FIRST]++;
                blk[first < KVQ_ADAPT_POSITIONS ? KVQ_ADAPT_B_FIRST_BINS + first : (int64_t)KVQ_ADAPT_B_BEYOND]++;
            } else if (tail >= 0) {
                tailed = true; clip = std::min(clip, L - tail);
                blk[KVQ_ADAPT_B_TAIL]++; blk[KVQ_ADAPT_B_TAIL_BINS + tail]++;
            }
        }
        out[KVQ_ADAPT_RECORDS]++;
        out[full ? KVQ_ADAPT_WITH_FULL : KVQ_ADAPT_TAIL_ONLY] += full || tailed;
        out[KVQ_ADAPT_CLIP + std::min<int64_t>(clip, KVQ_ADAPT_CLIP_BINS - 1)]++;
    });
    return KVQ_OK;
}

extern "C" int32_t kvq_clip_host(uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                 const uint8_t *const *probes, const int32_t *lens, int32_t n, int64_t *out)
{
    if (!twin_args("kvq_clip_host", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    if (!adapt_probes_ok("kvq_clip_host", probes, lens, n)) return KVQ_ERR_RUNTIME;
    out[KVQ_CLIP_N] = n;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t n2, int64_t n3) {
        const uint8_t *line = text + n0 + 1;
        int64_t L = n1 - n0 - 1, S = n3 - n2 - 1;
        if (L > 0 && line[L - 1] == '\r') L--;                                 // a trailing '\r' is not part of its line
        if (S > 0 && text[n2 + S] == '\r') S--;
        int64_t clip = L;
        for (int32_t k = 0; k < n; k++) {
            const int64_t m = lens[k];
            int64_t first = -1, tail = -1;
            for (int64_t p = 0; first < 0 && p + m <= L; p++) if (!memcmp(line + p, probes[k], (size_t)m)) first = p;
            for (int64_t t = std::min(m - 1, L); first < 0 && tail < 0 && t >= KVQ_ADAPT_MIN_TAIL; t--)
                if (!memcmp(line + L - t, probes[k], (size_t)t)) tail = t;
            if (first >= 0) clip = std::min(clip, first);
            else if (tail >= 0) clip = std::min(clip, L - tail);
        }
        out[KVQ_CLIP_RECORDS]++;
        if (clip >= L) return;
        out[KVQ_CLIP_CLIPPED]++; out[KVQ_CLIP_MASKED] += std::max<int64_t>(0, S - clip); out[KVQ_CLIP_BASES_CUT] += L - clip;
        for (int64_t p = clip; p < S; p++) text[n2 + 1 + p] = '!';
    });
    return KVQ_OK;
}

// ---- probes that tolerate mismatches ----
static bool adapt_per_ok(const char *who, int32_t per)
{
    const bool ok = per == 0 || (per >= KVQ_ADAPT_MIN_PER && per <= KVQ_ADAPT_MAX_PER);
    if (!ok) kvq_set_error(KVQ_ERR_RUNTIME, "%s: the mismatch rate is 0 (exact) or one mismatch per %d to %d bases", who, KVQ_ADAPT_MIN_PER, KVQ_ADAPT_MAX_PER);
    return ok;
}
// the positions at which a[0, n) and b[0, n) differ, as bytes
static int64_t adapt_ham(const uint8_t *a, const uint8_t *b, int64_t n)
{
    int64_t d = 0;
    for (int64_t i = 0; i < n; i++) d += a[i] != b[i];
    return d;
}
// FIRST, DIST and TAIL of one probe of m bytes on a line of L bytes (-1: none); E(len) = len / per, 0 when per is 0
static void adapt_search_mm(const uint8_t *line, int64_t L, const uint8_t *probe, int64_t m, int32_t per, int64_t &first, int64_t &dist, int64_t &tail)
{
    first = dist = tail = -1;
    const int64_t Em = per ? m / per : 0;
    for (int64_t p = 0; first < 0 && p + m <= L; p++) {                       // the smallest p, whatever a later window's distance
        const int64_t d = adapt_ham(line + p, probe, m);
        if (d <= Em) { first = p; dist = d; }
    }
    for (int64_t t = std::min(m - 1, L); first < 0 && tail < 0 && t >= KVQ_ADAPT_MIN_TAIL; t--)     // the largest t, E of t
        if (adapt_ham(line + L - t, probe, t) <= (per ? t / per : 0)) tail = t;
}

extern "C" int32_t kvq_adapt_host_mm(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                     const uint8_t *const *probes, const int32_t *lens, int32_t n, int32_t per, int64_t *out)
{
    if (!twin_args("kvq_adapt_host_mm", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    if (!adapt_probes_ok("kvq_adapt_host_mm", probes, lens, n) || !adapt_per_ok("kvq_adapt_host_mm", per)) return KVQ_ERR_RUNTIME;
    out[KVQ_ADAPT_N] = n;
    if (per) out[KVQ_ADAPT_PER] = per;
    for (int32_t k = 0; k < n; k++) out[KVQ_ADAPT_BLOCKS + (int64_t)k * KVQ_ADAPT_BLOCK_WORDS + KVQ_ADAPT_B_M] = lens[k];
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t, int64_t) {
        const uint8_t *line = text + n0 + 1;
        int64_t L = n1 - n0 - 1;
        if (L > 0 && line[L - 1] == '\r') L--;                                 // a trailing '\r' is not part of its line
        int64_t clip = L;
        bool full = false, tailed = false;
        for (int32_t k = 0; k < n; k++) {
            int64_t *const blk = out + KVQ_ADAPT_BLOCKS + (int64_t)k * KVQ_ADAPT_BLOCK_WORDS;
            int64_t first, dist, tail;
            adapt_search_mm(line, L, probes[k], lens[k], per, first, dist, tail);
            if (first >= 0) {
                full = true; clip = std::min(clip, first);
                blk[KVQ_ADAPT_B_FIRST]++;
                blk[first < KVQ_ADAPT_POSITIONS ? KVQ_ADAPT_B_FIRST_BINS + first : (int64_t)KVQ_ADAPT_B_BEYOND]++;
                if (per) blk[KVQ_ADAPT_B_DIST + dist]++;
            } else if (tail >= 0) {
                tailed = true; clip = std::min(clip, L - tail);
                blk[KVQ_ADAPT_B_TAIL]++; blk[KVQ_ADAPT_B_TAIL_BINS + tail]++;
            }
        }
        out[KVQ_ADAPT_RECORDS]++;
        out[full ? KVQ_ADAPT_WITH_FULL : KVQ_ADAPT_TAIL_ONLY] += full || tailed;
        out[KVQ_ADAPT_CLIP + std::min<int64_t>(clip, KVQ_ADAPT_CLIP_BINS - 1)]++;
    });
    return KVQ_OK;
}

extern "C" int32_t kvq_clip_host_mm(uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                    const uint8_t *const *probes, const int32_t *lens, int32_t n, int32_t per, int64_t *out)
{
    if (!twin_args("kvq_clip_host_mm", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    if (!adapt_probes_ok("kvq_clip_host_mm", probes, lens, n) || !adapt_per_ok("kvq_clip_host_mm", per)) return KVQ_ERR_RUNTIME;
    out[KVQ_CLIP_N] = n;
    if (per) out[KVQ_CLIP_PER] = per;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t n2, int64_t n3) {
        const uint8_t *line = text + n0 + 1;
        int64_t L = n1 - n0 - 1, S = n3 - n2 - 1;
        if (L > 0 && line[L - 1] == '\r') L--;                                 // a trailing '\r' is not part of its line
        if (S > 0 && text[n2 + S] == '\r') S--;
        int64_t clip = L;
        for (int32_t k = 0; k < n; k++) {
            int64_t first, dist, tail;
            adapt_search_mm(line, L, probes[k], lens[k], per, first, dist, tail);
            if (first >= 0) clip = std::min(clip, first);
            else if (tail >= 0) clip = std::min(clip, L - tail);
        }
        out[KVQ_CLIP_RECORDS]++;
        if (clip >= L) return;
        out[KVQ_CLIP_CLIPPED]++; out[KVQ_CLIP_MASKED] += std::max<int64_t>(0, S - clip); out[KVQ_CLIP_BASES_CUT] += L - clip;
        for (int64_t p = clip; p < S; p++) text[n2 + 1 + p] = '!';
    });
    return KVQ_OK;
}

extern "C" int32_t kvq_cycles_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t *out)
{
    if (!twin_args("kvq_cycles_host", out != nullptr, nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    int64_t *const score = out, *const base = out + (int64_t)KVQ_CYCLES * 256;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t n2, int64_t n3) {
        for (int64_t p = 0; p < KVQ_CYCLES && n0 + 1 + p < n1; p++) base[p * 256 + text[n0 + 1 + p]]++;
        for (int64_t p = 0; p < KVQ_CYCLES && n2 + 1 + p < n3; p++) score[p * 256 + text[n2 + 1 + p]]++;
    });
    return KVQ_OK;
}

extern "C" int32_t kvq_profile_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                    const uint8_t *cutoffs, int32_t ncut, int64_t *out)
{
    if (!twin_args("kvq_profile_host", out && ncut >= 0 && ncut <= KVQ_PROFILE_MAX_CUTOFFS && (ncut == 0 || cutoffs), nbytes, chunk_off, nchunks)) return KVQ_ERR_RUNTIME;
    for_each_record(text, chunk_off, nchunks, [&](int64_t n0, int64_t n1, int64_t n2, int64_t n3) {
        const int64_t L = n1 - n0 - 1, Q = n3 - n2 - 1;
        out[KVQ_PROF_RECORDS]++; out[KVQ_PROF_BASE_LINE_BYTES] += L; out[KVQ_PROF_SCORE_LINE_BYTES] += Q; out[KVQ_PROF_MISMATCHED] += L != Q;
        out[KVQ_PROF_LONGEST] = std::max(out[KVQ_PROF_LONGEST], L + 1);
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
    });
    return KVQ_OK;
}

// ---- the emitted reads ----
extern "C" int64_t kvq_emit_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int32_t amin_, int32_t min_length,
                                 uint8_t *out_text, int64_t out_cap, int64_t *out_words)
{
    if (!twin_args("kvq_emit_host", out_words && min_length >= 0 && out_cap >= 0 && (out_cap == 0 || out_text), nbytes, chunk_off, nchunks)) return -1;
    const int amin = (int8_t)amin_;
    int64_t at = 0; bool full = false;
    out_words[KVQ_EMIT_N] = min_length;
    for (int64_t c = 0; c < nchunks; c++) {
        // for_each_record's walk, with the record's first byte beside its newlines
        int64_t nl[4], r0 = chunk_off[c]; int have = 0;
        for (int64_t i = chunk_off[c]; i < chunk_off[c + 1]; i++) {
            if (text[i] != '\n') continue;
            nl[have++] = i;
            if (have < 4) continue;
            have = 0;
            const int64_t n0 = nl[0], n1 = nl[1], n2 = nl[2], n3 = nl[3], start0 = r0;
            r0 = n3 + 1;
            const int64_t L = n1 - n0 - 1, Q = n3 - n2 - 1;
            out_words[KVQ_EMIT_RECORDS]++; out_words[KVQ_EMIT_BASES_IN] += L;
            if (L != Q) { out_words[KVQ_EMIT_MISMATCHED]++; continue; }
            // workhorse.c:1055-1068 over the score line and its newline: the first of the longest runs that a low byte closes
            int64_t run = n2 + 1, best = 0, bstart = n2 + 1;
            for (int64_t j = n2 + 1; j <= n3; j++) {
                if ((int)(int8_t)text[j] >= amin) { if (run < 0) run = j; }
                else { if (run >= 0 && j - run > best) { best = j - run; bstart = run; } run = -1; }
            }
            if (best < min_length) { out_words[KVQ_EMIT_SHORT]++; continue; }
            const int64_t start = bstart - (n2 + 1);
            const int64_t name = n0 - start0 - (n0 > start0 && text[n0 - 1] == '\r' ? 1 : 0);
            const int64_t bytes = name + 2 * best + 5;
            out_words[KVQ_EMIT_EMITTED]++; out_words[KVQ_EMIT_BASES_OUT] += best; out_words[KVQ_EMIT_BYTES_OUT] += bytes;
            if (at + bytes > out_cap) { full = true; at += bytes; continue; }
            uint8_t *o = out_text + at;
            if (name) memcpy(o, text + start0, (size_t)name);
            o += name; *o++ = '\n';
            if (best) memcpy(o, text + n0 + 1 + start, (size_t)best);
            o += best; *o++ = '\n'; *o++ = '+'; *o++ = '\n';
            if (best) memcpy(o, text + n2 + 1 + start, (size_t)best);
            o += best; *o++ = '\n';
            at += bytes;
        }
    }
    if (full) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_emit_host: the text emits %lld bytes, out_cap is %lld", (long long)at, (long long)out_cap); return -1; }
    return at;
}

// ---- the emitted reads, deflated to BGZF ----
// The definition of kvq_deflate_blocks (kernels_deflate.hip) in plain C++, over the same kvq_deflate.h: block after block, segment
// after segment, where the kernel has a workgroup a block and a lane a segment.  (A little-endian host: the words of the bit
// buffer are the stream's bytes.)
struct DeflateTwinSink {
    KvqDeflatePlan *P; uint32_t *tok; uint32_t ntok; int64_t *words;
    void literal(uint8_t b) { tok[ntok++] = b; P->ll_freq[b]++; words[KVQ_DEFLATE_LITERALS]++; }
    void match(uint32_t len, uint32_t dist)
    {
        uint32_t s, n, e;
        tok[ntok++] = KVQ_DEFLATE_TOKEN_MATCH | (len << 16) | dist;
        kvq_deflate_len_sym(len, s, n, e); P->ll_freq[s]++;
        kvq_deflate_dist_sym(dist, s, n, e); P->d_freq[s]++;
        words[KVQ_DEFLATE_MATCHES]++;
        words[KVQ_DEFLATE_MAX_DISTANCE] = std::max<int64_t>(words[KVQ_DEFLATE_MAX_DISTANCE], dist);
        words[KVQ_DEFLATE_MAX_LENGTH] = std::max<int64_t>(words[KVQ_DEFLATE_MAX_LENGTH], len);
    }
};

extern "C" int64_t kvq_deflate_len(void) { return KVQ_DEFLATE_WORDS; }
extern "C" int64_t kvq_deflate_bound(int64_t nbytes) { return nbytes < 0 ? -1 : (int64_t)kvq_deflate_bound_bytes((uint64_t)nbytes); }
extern "C" const uint8_t *kvq_bgzf_eof(void)
{
    static const uint8_t eof[KVQ_BGZF_EOF_BYTES] = { 0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 'B', 'C', 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    return eof;
}

extern "C" int32_t kvq_deflate_lengths_host(const uint32_t *freq, int32_t nsym, int32_t limit, uint8_t *lens)
{
    kvq_clear_error();
    int64_t used = 0; uint64_t sum = 0;
    for (int32_t s = 0; freq && s < nsym && s < 288; s++) { used += freq[s] != 0; sum += freq[s]; }
    if (!freq || !lens || nsym < 0 || nsym > 288 || limit < 1 || limit > 15 || used > (1ll << limit) || sum > 0xFFFFFFFFull) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_deflate_lengths_host: bad arguments");
        return KVQ_ERR_RUNTIME;
    }
    KvqDeflateWork w;
    kvq_deflate_lengths(freq, nsym, limit, lens, &w);
    return KVQ_OK;
}

extern "C" int64_t kvq_deflate_bgzf_host(const uint8_t *text, int64_t nbytes, uint8_t *out, int64_t out_cap, int64_t *out_words)
{
    kvq_clear_error();
    if (nbytes < 0 || out_cap < 0 || !out_words || (nbytes > 0 && !text) || (out_cap > 0 && !out)) {
        kvq_set_error(KVQ_ERR_RUNTIME, "kvq_deflate_bgzf_host: bad arguments");
        return -1;
    }
    for (int i = 0; i < KVQ_DEFLATE_WORDS; i++) out_words[i] = 0;
    uint32_t table[256];
    for (uint32_t i = 0; i < 256u; i++) table[i] = kvq_crc_entry(i);
    std::vector<uint8_t> own(KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS), fin(KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS);
    std::vector<uint32_t> tok(KVQ_DEFLATE_BLOCK), bits(KVQ_DEFLATE_MEMBER_MAX / 4);
    std::vector<KvqDeflatePlan> plan(1);
    KvqDeflatePlan *const P = plan.data();
    int64_t at = 0; bool full = false;
    for (int64_t b0 = 0; b0 < nbytes; b0 += KVQ_DEFLATE_BLOCK) {
        const uint8_t *blk = text + b0;
        const uint32_t n = (uint32_t)std::min<int64_t>(KVQ_DEFLATE_BLOCK, nbytes - b0);
        memset(P->ll_freq, 0, sizeof P->ll_freq); memset(P->d_freq, 0, sizeof P->d_freq);
        int64_t parse[KVQ_DEFLATE_WORDS] = { 0 };               // (the parse's words count where its tokens are the stream)
        DeflateTwinSink sink = { P, tok.data(), 0, parse };
        uint32_t crc = 0;
        for (uint32_t seg = 0; seg < KVQ_DEFLATE_SEGS; seg++) kvq_deflate_final_table(blk, n, seg, fin.data());
        for (uint32_t seg = 0; seg < KVQ_DEFLATE_SEGS; seg++) {
            kvq_deflate_parse(blk, n, seg, own.data(), fin.data(), sink);
            // the segment's own CRC, moved to the front by the bytes behind the segment
            const uint32_t sb = kvq_deflate_seg_begin(seg, n), se = kvq_deflate_seg_begin(seg + 1u, n);
            crc ^= kvq_crc_mul(kvq_crc_shift(n - se), kvq_crc_bytes(table, 0u, blk + sb, se - sb));
        }
        P->ll_freq[256] = 1;
        kvq_deflate_plan(P, n);
        const uint32_t stream = kvq_deflate_stream_bytes(P, n), member = KVQ_BGZF_HEADER + stream + KVQ_BGZF_TRAILER;
        out_words[KVQ_DEFLATE_MEMBERS]++; out_words[KVQ_DEFLATE_BYTES_IN] += n; out_words[KVQ_DEFLATE_BYTES_OUT] += member; out_words[KVQ_DEFLATE_STORED] += P->stored;
        if (!P->stored) {
            out_words[KVQ_DEFLATE_MATCHES] += parse[KVQ_DEFLATE_MATCHES]; out_words[KVQ_DEFLATE_LITERALS] += parse[KVQ_DEFLATE_LITERALS];
            out_words[KVQ_DEFLATE_MAX_DISTANCE] = std::max(out_words[KVQ_DEFLATE_MAX_DISTANCE], parse[KVQ_DEFLATE_MAX_DISTANCE]);
            out_words[KVQ_DEFLATE_MAX_LENGTH] = std::max(out_words[KVQ_DEFLATE_MAX_LENGTH], parse[KVQ_DEFLATE_MAX_LENGTH]);
        }
        if (at + (int64_t)member > out_cap) { full = true; at += member; continue; }
        uint8_t *o = out + at;
        for (uint32_t i = 0; i < KVQ_BGZF_HEADER; i++) *o++ = kvq_bgzf_header_byte(i, member);
        if (P->stored) {
            for (uint32_t i = 0; i < 5u; i++) *o++ = kvq_deflate_stored_byte(i, n);
            memcpy(o, blk, n);
        } else {
            std::fill(bits.begin(), bits.end(), 0u);
            KvqBitsOut<KvqPlainOr> w;
            w.open(bits.data(), 0u);
            kvq_deflate_put_header(P, w);
            for (uint32_t i = 0; i < sink.ntok; i++) kvq_deflate_put_token(P, tok[i], w);
            w.put(P->ll_code[256], P->ll_len[256]);
            w.close();
            memcpy(o, bits.data(), stream);
        }
        o += stream - (P->stored ? 5u : 0u);
        for (uint32_t i = 0; i < 4u; i++) *o++ = (uint8_t)(crc >> (8u * i));
        for (uint32_t i = 0; i < 4u; i++) *o++ = (uint8_t)(n >> (8u * i));
        at += member;
    }
    if (full) { kvq_set_error(KVQ_ERR_RUNTIME, "kvq_deflate_bgzf_host: the text takes %lld bytes, out_cap is %lld", (long long)at, (long long)out_cap); return -1; }
    return at;
}
