// kvarq_amd/csrc/kvq_runtime.hip -- what every other host file of libkvarq_hip.so stands on: error state and config,
// the block cache and the memory helpers, device plumbing, the target table.  The scan object and the life of a batch
// (batches -> kernels -> hits) are in kvq_scan.hip, the end of a scan and its results in kvq_finish.hip; the
// engine.findseqs driver lives in kvq_findseqs.hip, its host reader in kvq_reader.hip, its device routes in kvq_routes.hip.
#include "kvq_host.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <stdarg.h>
#include <string.h>
#include <chrono>

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static const bool g_timing = getenv("KVQ_TIMING") != nullptr;

// internal: arena too small or speculation failed; the caller must rescan
#define KVQ_NEED_RESCAN (-2)

// ---------------------------------------------------------------------------
// error state and config
// ---------------------------------------------------------------------------

static thread_local int  tl_err_code = 0;
static thread_local char tl_err_msg[1024] = "";

void kvq_set_error(int code, const char *fmt, ...)
{
    tl_err_code = code;
    va_list ap; va_start(ap, fmt);
    vsnprintf(tl_err_msg, sizeof(tl_err_msg), fmt, ap);
    va_end(ap);
}
void kvq_clear_error() { tl_err_code = 0; tl_err_msg[0] = 0; }
int  kvq_error_code() { return tl_err_code; }

extern "C" int32_t kvq_last_error(char *msg, size_t cap)
{
    if (msg && cap) { strncpy(msg, tl_err_msg, cap - 1); msg[cap - 1] = 0; }
    return tl_err_code;
}

static std::mutex g_cfg_lock;
static kvq_config g_cfg = { 0, 20, 10, 1, '!', '!' };      // workhorse.c:71-75

extern "C" void kvq_config_set(const kvq_config *cfg) { std::lock_guard<std::mutex> l(g_cfg_lock); g_cfg = *cfg; }
extern "C" void kvq_config_get(kvq_config *cfg) { std::lock_guard<std::mutex> l(g_cfg_lock); *cfg = g_cfg; }
extern "C" const char *kvq_version(void) { return "kvarq_hip 0.1 (gfx950)"; }

// ---------------------------------------------------------------------------
// device plumbing
// ---------------------------------------------------------------------------

// Blocks a destroyed scan or table gives back are kept for the next one (per device, up to a bound): a scan's dozen
// hipMalloc / hipFree calls and its pinned buffers cost about 15 ms a scan, more than the kernels of a 3 GB file.
// A block in the cache is idle: whoever releases one has waited for the work that used it (kvq_scan_destroy,
// kvq_table_destroy); a buffer that grows while its scan is running goes back to the driver instead (hipFree waits).
namespace {
struct BlockCache {
    struct E { void *p; size_t cap; int dev; };
    std::mutex m; std::vector<E> v; size_t bytes = 0; const size_t max_bytes; const bool host;
    BlockCache(size_t mb, bool h) : max_bytes(mb), host(h) {}
    void *take(size_t n, size_t *cap)
    {
        int dev = 0; (void)hipGetDevice(&dev);
        std::lock_guard<std::mutex> l(m);
        size_t best = v.size();
        for (size_t i = 0; i < v.size(); i++)
            if (v[i].dev == dev && v[i].cap >= n && v[i].cap <= 2 * n + (1u << 20) && (best == v.size() || v[i].cap < v[best].cap)) best = i;
        if (best == v.size()) return nullptr;
        void *p = v[best].p; *cap = v[best].cap; bytes -= v[best].cap;
        v.erase(v.begin() + (long)best);
        return p;
    }
    bool put(void *p, size_t cap)
    {
        // the device that OWNS the block, not the one that is current in the calling thread: a scan may be destroyed from
        // another thread than the one that made it (Python's garbage collector; ranks as threads closed by their parent),
        // and a block filed under the wrong device would later be handed to a scan there
        int dev = 0; (void)hipGetDevice(&dev);
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) == hipSuccess) dev = at.device; else (void)hipGetLastError();
        std::lock_guard<std::mutex> l(m);
        if (cap > max_bytes / 2 || v.size() >= 256) return false;
        while (bytes + cap > max_bytes && !v.empty()) {          // the oldest blocks make room
            if (host) (void)hipHostFree(v[0].p); else (void)hipFree(v[0].p);
            bytes -= v[0].cap; v.erase(v.begin());
        }
        v.push_back({ p, cap, dev }); bytes += cap;
        return true;
    }
    size_t held() { std::lock_guard<std::mutex> l(m); return bytes; }
    void drop()
    {
        std::lock_guard<std::mutex> l(m);
        for (auto &e : v) { if (host) (void)hipHostFree(e.p); else (void)hipFree(e.p); }
        v.clear(); bytes = 0;
    }
};
static bool cache_on() { static const bool on = !(getenv("KVQ_BLOCK_CACHE") && getenv("KVQ_BLOCK_CACHE")[0] == '0'); return on; }
static BlockCache g_dev_blocks((size_t)2 << 30, false), g_pin_blocks((size_t)512 << 20, true);
}

// give the cached blocks back to the driver (a host that wants the memory; nothing needs calling this)
void kvq_drop_kept_scan();      // kvq_findseqs.hip
extern "C" void kvq_release_cached(void) { kvq_drop_kept_scan(); g_dev_blocks.drop(); g_pin_blocks.drop(); }

int DevBuf::ensure(size_t n)
{
    if (n <= cap && p) return KVQ_OK;
    size_t want = n + n / 4 + 256;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    if (cache_on()) { size_t c = 0; if (void *q = g_dev_blocks.take(n + 256, &c)) { p = q; cap = c; return KVQ_OK; } }
    hipError_t e = hipMalloc(&p, want);
    if (e == hipErrorOutOfMemory && g_dev_blocks.held()) { g_dev_blocks.drop(); e = hipMalloc(&p, want); }
    if (e != hipSuccess) {
        p = nullptr;
        kvq_set_error(e == hipErrorOutOfMemory ? KVQ_ERR_MEMORY : KVQ_ERR_DEVICE, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return tl_err_code;
    }
    cap = want;
    return KVQ_OK;
}
void DevBuf::release() { if (p && !(cache_on() && g_dev_blocks.put(p, cap))) (void)hipFree(p); p = nullptr; cap = 0; }

// pinned host memory through the same kind of cache (*cap: what the block holds, at least n)
static void *pinned_take(size_t n, size_t *cap)
{
    if (cache_on()) if (void *q = g_pin_blocks.take(n, cap)) return q;
    void *p = nullptr;
    if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) return nullptr;
    *cap = n;
    return p;
}
static void pinned_give(void *p, size_t cap) { if (p && !(cache_on() && g_pin_blocks.put(p, cap))) (void)hipHostFree(p); }
// a grow-only pinned buffer kept from call to call (the device routes' and the BAM runs'): contents are NOT preserved
static int pinned_grow(void **p, size_t *cap, size_t need)
{
    if (*cap >= need) return KVQ_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 4;
    if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) { *p = nullptr; kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate memory for scanning"); return KVQ_ERR_MEMORY; }
    *cap = want;
    return KVQ_OK;
}

int TablePool::reserve(size_t bytes, hipStream_t stream)
{
    bytes = (bytes + 4095) & ~(size_t)4095;
    if (used + bytes <= cap) return KVQ_OK;
    // grow: earlier batches may still read the old blocks, so wait for them first; what they have left there
    // (tile reports, lists of skipped tiles: found again by their offsets) moves over
    if (stream) KVQ_HIP(hipStreamSynchronize(stream));
    const size_t want = std::max<size_t>(2 * cap, std::max<size_t>(used + bytes, (size_t)8 << 20));
    size_t hcap = 0; uint8_t *nh = (uint8_t *)pinned_take(want, &hcap);
    DevBuf nd;
    if (!nh || nd.ensure(want) != KVQ_OK) {
        if (nh) pinned_give(nh, hcap);
        kvq_set_error(KVQ_ERR_MEMORY, "cannot allocate %zu bytes of batch tables", want);
        return KVQ_ERR_MEMORY;
    }
    if (used) { memcpy(nh, h, used); KVQ_HIP(hipMemcpy(nd.p, d, used, hipMemcpyDeviceToDevice)); }
    const size_t keep = used;
    release();
    h = nh; h_cap = hcap; d = (uint8_t *)nd.p; d_cap = nd.cap; cap = want; used = keep;
    return KVQ_OK;
}
void TablePool::release()
{
    if (h) pinned_give(h, h_cap);
    if (d) { DevBuf b; b.p = d; b.cap = d_cap; b.release(); }
    h = d = nullptr; cap = used = 0; h_cap = d_cap = 0;
}

extern "C" int32_t kvq_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
uint32_t kvq_device_cu_count()
{
    int dev = 0; hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount <= 0) return 256u;
    return (uint32_t)pr.multiProcessorCount;
}
extern "C" int32_t kvq_set_device(int32_t o) { KVQ_HIP(hipSetDevice(o)); return KVQ_OK; }
extern "C" void *kvq_device_alloc(int64_t n)
{
    void *p = nullptr;
    if (hipMalloc(&p, (size_t)n + 256) != hipSuccess) { kvq_set_error(KVQ_ERR_MEMORY, "hipMalloc(%lld) failed", (long long)n); return nullptr; }
    return p;
}
extern "C" void kvq_device_free(void *p) { if (p) (void)hipFree(p); }
extern "C" int32_t kvq_memcpy_h2d(void *d, const void *h, int64_t n) { KVQ_HIP(hipMemcpy(d, h, (size_t)n, hipMemcpyHostToDevice)); return KVQ_OK; }
extern "C" int32_t kvq_memcpy_d2h(void *h, const void *d, int64_t n) { KVQ_HIP(hipMemcpy(h, d, (size_t)n, hipMemcpyDeviceToHost)); return KVQ_OK; }
extern "C" int32_t kvq_memset_d(void *d, int32_t v, int64_t n) { KVQ_HIP(hipMemset(d, v, (size_t)n)); return KVQ_OK; }
extern "C" int32_t kvq_device_synchronize(void) { KVQ_HIP(hipDeviceSynchronize()); return KVQ_OK; }

// ---------------------------------------------------------------------------
// table
// ---------------------------------------------------------------------------

extern "C" kvq_table *kvq_table_create(const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, const kvq_config *cfg)
{
    kvq_clear_error();
    if (kvq_device_count() <= 0) { kvq_set_error(KVQ_ERR_DEVICE, "no HIP device available: libkvarq_hip has no CPU path"); return nullptr; }
    kvq_table *t = new kvq_table();
    if (cfg) t->cfg = *cfg; else kvq_config_get(&t->cfg);
    t->nseq = nseq;
    t->h_off.resize((size_t)nseq + 1);
    int64_t tot = 0;
    for (int i = 0; i < nseq; i++) {
        if (seqlens[i] < 0) { kvq_set_error(KVQ_ERR_TYPE, "seqlist must be list of strings"); delete t; return nullptr; }
        t->h_off[i] = (int32_t)tot; tot += seqlens[i];
        if (tot > 0x7FFFFFFF) { kvq_set_error(KVQ_ERR_MEMORY, "sequence table too large"); delete t; return nullptr; }
    }
    t->h_off[nseq] = (int32_t)tot;
    t->bases = tot;
    t->h_tab.resize((size_t)tot + 64, 0);
    for (int i = 0; i < nseq; i++) if (seqlens[i]) memcpy(&t->h_tab[t->h_off[i]], seqs[i], (size_t)seqlens[i]);
    // counters layout (include/kvarq_hip.h)
    t->off_nseqhits = KVQ_CTR_RL_ + KVQ_RL_BINS;
    t->off_nseqbasehits = t->off_nseqhits + nseq;
    t->off_cov = t->off_nseqbasehits + nseq;
    t->off_mut = t->off_cov + tot;
    t->ctr_len = t->off_mut + 6 * tot;

    (void)hipGetDevice(&t->device);
    t->is_seeded.assign((size_t)nseq, 0);
    t->index = kvq_seed_index_build(t);      // fills seeded / is_seeded / seed_k
    if (kvq_error_code()) { kvq_table_destroy(t); return nullptr; }
    for (int i = 0; i < nseq; i++) if (!t->is_seeded[i]) t->exhaustive.push_back(i);

    std::vector<int32_t> all((size_t)nseq);
    for (int i = 0; i < nseq; i++) all[i] = i;
    bool ok = t->d_tab.ensure(t->h_tab.size()) == KVQ_OK && t->d_off.ensure((size_t)(nseq + 1) * 4) == KVQ_OK &&
              t->d_exh.ensure((size_t)(nseq + 1) * 4) == KVQ_OK && t->d_all.ensure((size_t)(nseq + 1) * 4) == KVQ_OK &&
              t->d_seeded.ensure((size_t)(nseq + 1) * 4) == KVQ_OK;
    if (ok) {
        ok = hipMemcpy(t->d_tab.p, t->h_tab.data(), t->h_tab.size(), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(t->d_off.p, t->h_off.data(), (size_t)(nseq + 1) * 4, hipMemcpyHostToDevice) == hipSuccess &&
             (t->exhaustive.empty() || hipMemcpy(t->d_exh.p, t->exhaustive.data(), t->exhaustive.size() * 4, hipMemcpyHostToDevice) == hipSuccess) &&
             (t->seeded.empty() || hipMemcpy(t->d_seeded.p, t->seeded.data(), t->seeded.size() * 4, hipMemcpyHostToDevice) == hipSuccess) &&
             (nseq == 0 || hipMemcpy(t->d_all.p, all.data(), (size_t)nseq * 4, hipMemcpyHostToDevice) == hipSuccess);
        if (!ok) kvq_set_error(KVQ_ERR_DEVICE, "uploading the sequence table failed");
    }
    if (!ok) { kvq_table_destroy(t); return nullptr; }
    return t;
}

extern "C" void kvq_table_destroy(kvq_table *t)
{
    if (!t) return;
    {
        // (its blocks go to the cache, not through hipFree: nothing may still be reading them -- on the device the table lives on,
        // which need not be the calling thread's current one)
        int cur = 0; (void)hipGetDevice(&cur);
        if (t->device != cur) (void)hipSetDevice(t->device);
        (void)hipDeviceSynchronize();
        if (t->device != cur) (void)hipSetDevice(cur);
    }
    if (t->index) kvq_seed_index_destroy(t->index);
    t->d_tab.release(); t->d_off.release(); t->d_exh.release(); t->d_all.release(); t->d_seeded.release();
    delete t;
}
extern "C" int32_t kvq_table_nseq(const kvq_table *t) { return t->nseq; }
extern "C" int64_t kvq_table_bases(const kvq_table *t) { return t->bases; }
extern "C" int32_t kvq_table_seq_is_seeded(const kvq_table *t, int32_t s) { return (s >= 0 && s < t->nseq) ? t->is_seeded[s] : 0; }
extern "C" int32_t kvq_table_seed_k(const kvq_table *t) { return t->seed_k; }
extern "C" int64_t kvq_counters_len(const kvq_table *t) { return t->ctr_len; }
extern "C" int64_t kvq_counters_off_nseqhits(const kvq_table *t) { return t->off_nseqhits; }
extern "C" int64_t kvq_counters_off_nseqbasehits(const kvq_table *t) { return t->off_nseqbasehits; }
extern "C" int64_t kvq_counters_off_coverage(const kvq_table *t) { return t->off_cov; }
extern "C" int64_t kvq_counters_off_mutations(const kvq_table *t) { return t->off_mut; }
extern "C" int64_t kvq_table_seq_offset(const kvq_table *t, int32_t s) { return (s >= 0 && s <= t->nseq) ? t->h_off[s] : -1; }
