// kvarq_amd/csrc/kernels_list.hip -- the seed filter over a LIST of reads: the matcher of the opt-in
// read-list route (kvq_scan_set_long_reads), for texts whose records no tile of kvq_scan_bp can hold.  It takes the reads as
// kvq_trim_records leaves them (read_off / read_len), looks their K-mers up in the seed index of kernels_seeded.hip and
// verifies what the index names byte by byte; the hits are the ones kvq_match_all gives for the seeded sequences.
//
// Which lookup finds which job (kvq_jobs_of / kvq_job), for a read of rl bases, a sequence of sl, e = maxerrors:
//   family S  the read's positions p = 0 (mod stride), in the anchors' index: an entry (s, pos) is job C_i, i = p - pos, of a
//             sequence inside the read (rl > sl); the block is number pos / pitch of the sequence's copy pos % pitch
//   family H  the read's blocks at K t, t = 0 .. e, in the index of all positions: an entry (s, pos) is si = pos - K t: job
//             B_si where that lies in B's range, job C_si where rl <= sl and 0 <= si <= sl - rl (both at si = sl - rl >= 1:
//             the reference's duplicate hit)
//   family T  the read's blocks at rl - K (t + 1) in the index of all positions: job A_i, i = rl - K (t + 1) - pos
// Every job's e + 1 blocks lie inside its overlap ((e + 1) K <= min(minoverlap, minreadlength), kvq_seed_k; a seeded sequence
// holds its anchor copies, kvq_seed_index_build), so one of them is free of errors when the job is within budget.
//
// A work item (job, block t) emits if and only if the job is within budget, byte-exact, its own block is byte-equal to the
// sequence (a lookup only says that the CODES are equal: 'N' has the code of 'G', 'a' that of 'A'), and no block t' < t of
// the same job and family is: equal bytes have equal codes, so every error-free block of a job is looked up and found, and
// exactly the first of them emits.  No second pass sorts duplicates out.
#include "kvq_device.h"

#define KVQ_LIST_Q 256u            // candidates (read position, code, family, block) a wave's queue holds
#define KVQ_LIST_GRID_MAX 4096u    // workgroups of a launch at the most (the waves stride over the list)

__device__ __forceinline__ bool kvq_list_block_eq(const uint8_t *x, const uint8_t *y, int K)
{
    bool eq = true;
    for (int i = 0; i < K; i++) eq &= x[i] == y[i];
    return eq;
}

// sixteen bytes of text as sixteen 2-bit codes, base i in bits 2i, 2i + 1 (the arithmetic of kvq_scan_bp's pass 0)
__device__ __forceinline__ uint32_t kvq_list_pack16(const uint4 v)
{
    const uint32_t d0 = __builtin_amdgcn_udot4((v.x >> 1) & 0x03030303u, 0x40100401u, 0u, false);
    const uint32_t d1 = __builtin_amdgcn_udot4((v.y >> 1) & 0x03030303u, 0x40100401u, 0u, false);
    const uint32_t d2 = __builtin_amdgcn_udot4((v.z >> 1) & 0x03030303u, 0x40100401u, 0u, false);
    const uint32_t d3 = __builtin_amdgcn_udot4((v.w >> 1) & 0x03030303u, 0x40100401u, 0u, false);
    return d0 | (d1 << 8) | (d2 << 16) | (d3 << 24);
}

// what a wave's lanes wrote to its part of the LDS is there for its other lanes
__device__ __forceinline__ void kvq_list_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave per read, four reads per workgroup, the waves stride over the list
extern "C" __global__ void __launch_bounds__(256)
kvq_seed_list(KvqParams P, const uint8_t *__restrict__ data, int64_t fpos_base, uint32_t nrec,
              const uint32_t *__restrict__ read_off, const int32_t *__restrict__ read_len,
              const int32_t *__restrict__ seq_list, int32_t nlist, SeedTables T, int32_t K)
{
    __shared__ uint32_t bm[(1u << (2 * KVQ_K_MAX)) / 32u];          // the anchors' bitmap
    __shared__ uint32_t q_p[4][KVQ_LIST_Q], q_m[4][KVQ_LIST_Q];     // the waves' queues: read position; code | family << 16 | block << 18
    __shared__ uint32_t w_pre[4][64], w_st[4][64];                  // a round of the drain: work items in front of a candidate, its CSR start
    __shared__ int min_sl;                                          // the shortest listed sequence
    const uint32_t NC = 1u << (2 * K), kmask = NC - 1u;
    const int lane = kvq_lane(), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) min_sl = 0x7FFFFFFF;
    for (uint32_t i = threadIdx.x; i < (NC >= 32u ? NC / 32u : 1u); i += blockDim.x) bm[i] = T.bm1[i];
    __syncthreads();
    {
        int m = 0x7FFFFFFF;
        for (int q = (int)threadIdx.x; q < nlist; q += (int)blockDim.x) { const int s = seq_list[q]; const int sl = P.tab_off[s + 1] - P.tab_off[s]; m = sl < m ? sl : m; }
        if (m != 0x7FFFFFFF) atomicMin(&min_sl, m);
    }
    __syncthreads();
    const int e = P.maxerrors, mo = P.minoverlap, stride = T.stride, pitch = T.pitch;
    uint32_t *const qp = q_p[wave], *const qm = q_m[wave], *const pre = w_pre[wave], *const cst = w_st[wave];

    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wave; g < nrec; g += gridDim.x * 4u) {
        const int rl = read_len[g];
        if (rl < K * (e + 1)) continue;                 // (failed the length gate: -1; no read that passed it is shorter than e + 1 blocks)
        const uint32_t ro = read_off[g];
        const uint8_t *read = data + ro;
        const int64_t fpos = fpos_base + ro;
        uint32_t qn = 0;                                // candidates in the queue (the same in every lane)

        // every candidate of the queue against every index entry of its code, a lane per work item
        auto drain = [&]() {
            kvq_list_wave_sync();
            for (uint32_t b = 0; b < qn; b += 64u) {
                const uint32_t ci = b + (uint32_t)lane;
                uint32_t st = 0, n = 0;
                if (ci < qn) {
                    const uint32_t meta = qm[ci];
                    const uint32_t key = (meta & 0xFFFFu) + (((meta >> 16) & 3u) ? NC : 0u);
                    st = T.start[key]; n = T.start[key + 1] - st;
                }
                const uint32_t incl = kvq_wave_incl_scan(n);
                const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                pre[lane] = incl - n; cst[lane] = st;
                kvq_list_wave_sync();
                for (uint32_t it0 = 0; it0 < tot; it0 += 64u) {
                    const uint32_t it = it0 + (uint32_t)lane;
                    bool hit1 = false, hit2 = false;
                    int s = 0, spos1 = 0, len1 = 0, spos2 = 0, len2 = 0; uint32_t key1 = 0, key2 = 0;
                    if (it < tot) {
                        int c = 0;                       // the last candidate with no more than `it` items in front of it
#pragma unroll
                        for (int step = 32; step; step >>= 1) if (pre[c + step] <= it) c += step;
                        const uint32_t meta = qm[b + (uint32_t)c];
                        const int p = (int)qp[b + (uint32_t)c], fam = (int)((meta >> 16) & 3u), t = (int)(meta >> 18);
                        const uint64_t en = T.ent[cst[c] + (it - pre[c])].en;
                        const int pos = (int)(en & 0xFFFu), sl = (int)(en >> 52);
                        s = (int)((en >> 12) & 0xFFFFFu);
                        const uint8_t *seq = P.tab + (uint32_t)((en >> 32) & 0xFFFFFu);
                        const KvqJobs J = kvq_jobs_of(rl, sl, mo);
                        int ri, si, j1 = -1, j2 = -1;
                        bool first = kvq_list_block_eq(read + p, seq + pos, K);      // (equal codes, not yet equal bytes: 'N' and 'G', 'a' and 'A')
                        if (fam == 0) {
                            const int i = p - pos;
                            if (rl > sl && i >= 0 && i <= rl - sl) {
                                j1 = J.nA + J.nB + i;
                                const int tb = pos / pitch, sft = pos - tb * pitch;
                                for (int u = 0; u < tb; u++) first &= !kvq_list_block_eq(read + i + u * pitch + sft, seq + u * pitch + sft, K);
                            }
                        } else if (fam == 1) {
                            const int d = pos - K * t;
                            if (d >= 0) {
                                if (J.nB > 0 && d <= J.iB_hi && d > J.iB_hi - J.nB) j1 = J.nA + (J.iB_hi - d);
                                if (rl <= sl && d <= sl - rl) j2 = J.nA + J.nB + d;
                                if (j1 >= 0 || j2 >= 0)
                                    for (int u = 0; u < t; u++) first &= !kvq_list_block_eq(read + K * u, seq + d + K * u, K);
                            }
                        } else {
                            const int i = p - pos;
                            if (J.nA > 0 && i <= J.iA_hi && i > J.iA_hi - J.nA) {
                                j1 = J.iA_hi - i;
                                for (int u = 0; u < t; u++) first &= !kvq_list_block_eq(read + rl - K * (u + 1), seq + rl - K * (u + 1) - i, K);
                            }
                        }
                        if (first && j1 >= 0) { kvq_job(J, j1, rl, sl, ri, si, len1, spos1, key1); hit1 = within_budget(read + ri, seq + si, len1, e); }
                        if (first && j2 >= 0) { kvq_job(J, j2, rl, sl, ri, si, len2, spos2, key2); hit2 = within_budget(read + ri, seq + si, len2, e); }
                    }
                    kvq_emit(P, hit1, fpos, s, spos1, len1, rl, key1);
                    kvq_emit(P, hit2, fpos, s, spos2, len2, rl, key2);
                }
                kvq_list_wave_sync();                   // (the next round writes pre / cst again)
            }
            qn = 0;
        };
        // the flagged lanes' candidates onto the queue, in lane order; a queue that cannot take them is drained first
        auto push = [&](bool c, uint32_t p, uint32_t meta) {
            const uint64_t m = __ballot(c);
            if (m == 0) return;
            const uint32_t n = (uint32_t)__popcll(m);
            if (qn + n > KVQ_LIST_Q) drain();
            if (c) { const uint32_t i = qn + (uint32_t)__popcll(m & kvq_lanemask_lt()); qp[i] = p; qm[i] = meta; }
            qn += n;
        };

        {   // families H (lanes 0 .. e) and T (lanes 32 .. 32 + e): the read's fixed blocks in the index of all positions
            const int t = lane & 31, fam = lane < 32 ? 1 : 2;
            bool c = false; uint32_t p = 0, meta = 0;
            if (t <= e) {
                p = (uint32_t)(fam == 1 ? K * t : rl - K * (t + 1));
                uint32_t code = 0;
                for (int i = 0; i < K; i++) code |= (((uint32_t)read[p + (uint32_t)i] >> 1) & 3u) << (2 * i);
                const uint32_t key = NC + code;
                c = ((T.bm1[key >> 5] >> (key & 31u)) & 1u) != 0u;
                meta = code | ((uint32_t)fam << 16) | ((uint32_t)t << 18);
            }
            push(c, p, meta);
        }
        if (rl > min_sl) {
            // family S: the read 1 KiB at a time, sixteen bases a lane (loaded from the 16-byte boundary in front of the read; the
            // text is readable to the boundary behind its end), the next KiB on its way while this one is looked up
            const uint32_t sh = ro & 15u, a0 = ro - sh, end = ro + (uint32_t)rl;
            const uint32_t last_v = (end - 1u) & ~15u;
            const uint32_t nch = (sh + (uint32_t)rl + 1023u) / 1024u;
            const uint32_t j0 = sh & (uint32_t)(stride - 1);      // (the stride divides 16: the lane's bases j = sh (mod stride) are read positions 0 (mod stride))
            auto packload = [&](uint32_t c) -> uint32_t {
                const uint32_t q = a0 + 1024u * c + 16u * (uint32_t)lane;
                const uint4 v = *reinterpret_cast<const uint4 *>(data + (q < end ? q : last_v));
                return q < end ? kvq_list_pack16(v) : 0u;
            };
            uint32_t cur = packload(0u);
            for (uint32_t c = 0; c < nch; c++) {
                const uint32_t nx = c + 1u < nch ? packload(c + 1u) : 0u;
                // the sixteen bases behind the lane's own: the next lane's (lane 63: the next KiB's first)
                uint32_t hi = (uint32_t)__shfl_down((int)cur, 1, 64);
                const uint32_t nx0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nx);
                if (lane == 63) hi = nx0;
                const uint64_t W = (uint64_t)cur | ((uint64_t)hi << 32);
                const int p0 = (int)(1024u * c + 16u * (uint32_t)lane) - (int)sh;
                for (uint32_t j = j0; j < 16u; j += (uint32_t)stride) {
                    const int p = p0 + (int)j;
                    const uint32_t code = (uint32_t)(W >> (2u * j)) & kmask;
                    const bool cand = p >= 0 && p + K <= rl && ((bm[code >> 5] >> (code & 31u)) & 1u) != 0u;
                    push(cand, (uint32_t)p, code);
                }
                cur = nx;
            }
        }
        if (qn) drain();
    }
}
