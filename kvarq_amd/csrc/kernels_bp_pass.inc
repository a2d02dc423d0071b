// kernels_bp_pass.inc -- one pass of kvq_scan_bp over a tile's records: trim, seed filter, P4 (textually included twice by the kernel).
// BP_STRAIGHT 1: the tile's only pass, the wave's only stretch, one window of work items -- no loops; sets `bail` and stops where that
//                does not hold (a queue that overflows, more than BP_Q2W work items), before anything has been emitted
// BP_STRAIGHT 0: the loops -- passes of RP records, stretches halved when a queue overflows, windows of BP_Q2W work items
// in: nrec, jn, Ja, g0, text, lg, G, RP, gl, gr, recount (the reads of the pass are in the histogram already), wave, lane, tid, dbg, S, A_
#if BP_STRAIGHT
        {
            const uint32_t pass0 = 0;
#else
        for (uint32_t pass0 = 0; pass0 < nrec; pass0 += RP) {
#endif
            const uint32_t k = pass0 + gr;
            const bool have = k < nrec;
            uint32_t roff = 0; int rl = 0;
            // (the loops beside a straight body, which run once in a blue moon, fetch the two bytes where they are looked at: held across the loops
            // they are two vector registers more than the kernel has)
            constexpr bool late_probes = !BP_STRAIGHT && LG >= 0 && !DENSE;
            uint32_t c0, cp;                                        // the record's '@' and '+' (1037-1048): fetched here by the group's first lane, looked at behind the pass
            if (have) {
                const uint32_t m = jn + 4u * k;
                const uint32_t rstart = m == 0 ? ST_PRE + (Ja & 15u) : (uint32_t)S.nl[m - 1] + 1u;
                const uint32_t n0 = S.nl[m], n1 = S.nl[m + 1], n2 = S.nl[m + 2], n3 = S.nl[m + 3];
                const uint32_t sread = n0 + 1u, plus = n1 + 1u, sscore = n2 + 1u;
        KVQ_MARK("trim" BP_SFX);
                if (gl == 0 && !late_probes) { if (dbg & 8u) { c0 = '@'; cp = '+'; } else { c0 = text[rstart]; cp = text[plus]; } }   // (diagnostic 8: no '@' / '+' probes -- ablation only)
                // quality trim (1055-1068): this lane's slice of the score line is a bit range of the good plane
                const int Q = (int)(n3 - sscore);                   // the closing '\n' is implied
                const int per = (Q + (int)G - 1) >> lg;
                Seg sg; sg.beg = (int)mul_u24(gl, (uint32_t)per); if (sg.beg > Q) sg.beg = Q;
                int s1 = sg.beg + per; if (s1 > Q) s1 = Q;
                sg.len = 0; sg.pre = 0; sg.suf = 0; sg.best = 0; sg.bstart = sg.beg;
                {
                    // one round of at most 64 score bits
                    auto round = [&](int c0_) -> Seg {
                        const int n = s1 - c0_ < 64 ? s1 - c0_ : 64;
                        const uint32_t bit = sscore + (uint32_t)c0_;
                        const uint32_t a = BP_LDS_GDP + ((bit >> 5) << 2), sh = bit & 31u;
                        const uint32_t d0 = lds_u32_at(a), d1 = lds_u32_at(a + 4u), d2 = lds_u32_at(a + 8u);
                        const uint64_t nmask = n < 64 ? (1ull << n) - 1ull : ~0ull;
                        const uint64_t mm = (((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32) | (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh)) & nmask;
                        Seg sub; sub.beg = c0_; sub.len = n;
                        int bs;
                        bp_runs64(mm, n, dbg, sub.pre, sub.suf, sub.best, bs);
                        sub.bstart = c0_ + bs;
                        return sub;
                    };
                    if (!__any(per > 64)) sg = round(sg.beg);
                    else {
                        for (int cc = sg.beg; cc < s1; cc += 64) {
                            const Seg sub = round(cc);
                            sg = (cc == sg.beg) ? sub : seg_merge(sg, sub);
                        }
                    }
                }
                // ordered tree merge over the G lanes of the read
                if (G == 4u) {
#define KVQ_QUAD(v, ctl) __builtin_amdgcn_update_dpp(0, (v), (ctl), 0xf, 0xf, true)
                    {
                        Seg B;                                                       // lane ^ 1: quad_perm [1,0,3,2]
                        B.len = KVQ_QUAD(sg.len, 0xB1); B.pre = KVQ_QUAD(sg.pre, 0xB1); B.suf = KVQ_QUAD(sg.suf, 0xB1);
                        B.best = KVQ_QUAD(sg.best, 0xB1); B.bstart = KVQ_QUAD(sg.bstart, 0xB1); B.beg = 0;
                        sg = seg_merge(sg, B);
                    }
                    {
                        Seg B;                                                       // lane ^ 2: quad_perm [2,3,0,1]
                        B.len = KVQ_QUAD(sg.len, 0x4E); B.pre = KVQ_QUAD(sg.pre, 0x4E); B.suf = KVQ_QUAD(sg.suf, 0x4E);
                        B.best = KVQ_QUAD(sg.best, 0x4E); B.bstart = KVQ_QUAD(sg.bstart, 0x4E); B.beg = 0;
                        sg = seg_merge(sg, B);
                    }
                    rl = KVQ_QUAD(sg.best, 0x00);
                    roff = sread + (uint32_t)KVQ_QUAD(sg.bstart, 0x00);              // 1070
#undef KVQ_QUAD
                } else {
                    for (uint32_t d = 1; d < G; d <<= 1) {
                        Seg B;
                        B.len = __shfl_xor(sg.len, (int)d, 64); B.pre = __shfl_xor(sg.pre, (int)d, 64); B.suf = __shfl_xor(sg.suf, (int)d, 64);
                        B.best = __shfl_xor(sg.best, (int)d, 64); B.bstart = __shfl_xor(sg.bstart, (int)d, 64); B.beg = 0;
                        if ((gl & d) == 0) sg = seg_merge(sg, B);
                    }
                    rl = __shfl(sg.best, lane & ~(int)(G - 1u), 64);
                    roff = sread + (uint32_t)__shfl(sg.bstart, lane & ~(int)(G - 1u), 64);             // 1070
                }
                // (the longest read: a running maximum per lane, put together once at the end of the kernel -- an
                // atomic maximum in LDS per read is turned into a scalar loop over the wave's lanes by the compiler)
                my_longest = my_longest > (uint32_t)(rl + 1) ? my_longest : (uint32_t)(rl + 1);
                if (gl == 0) {
                    if (rl < KVQ_RL_BINS && !recount) atomicAdd(&S.hist[rl >> 1], 1u << (16 * (rl & 1)));          // 394-402
                    S.rinfo[k] = roff | ((uint32_t)rl << 16);
                }
            }
        KVQ_MARK("trim end / filter" BP_SFX);
            BSTAMP(4);
            KVQ_SETPRIO(2);
            // filter + verify, wave by wave (the wave's reads, candidates and work items are its own)
            const uint32_t rpw = 64u >> lg, grw = (uint32_t)lane >> lg;
            const uint32_t wfirst = pass0 + wave * rpw;
            const uint32_t npass = wfirst < nrec ? (nrec - wfirst < rpw ? nrec - wfirst : rpw) : 0u;
            uint32_t *const q1 = S.q1 + wave * BP_QW; uint32_t *const q2 = S.q2 + wave * BP_Q2W;
            uint32_t sub = (dbg & 128u) ? npass : 0u, step = rpw;             // (diagnostic 128: trim only)
#if BP_STRAIGHT
            if (sub < npass) {
#else
            while (sub < npass) {
#endif
                BTALLY(6, lane == 0);
                // (a stretch is one turn of this loop unless a queue overflows; what depends on the read only is worked out here, where it is
                // wanted, not hoisted in front of the loop into a dozen registers and spilled wave masks: the compiler cannot know the trip count)
                asm volatile("" : "+v"(rl), "+v"(roff));
                int minrl, me_; const __attribute__((address_space(1))) uint8_t *bmL;
                {
                    const BpArgsPtr A = bp_args(A_);
                    minrl = A->P.minreadlength; me_ = A->P.maxerrors;
                    bmL = (const __attribute__((address_space(1))) uint8_t *)A->X.bm1 + (1 << (2 * KK)) / 8;
                }
                const bool mine = have && rl >= minrl && !(dbg & 2u) && grw >= sub && grw - sub < step;       // 1100
                uint32_t qn = 0;
                int e0 = 0, e1 = 0;
                if (mine) {
                    const int NPe = (rl - KK) / SS + 1;
                    const int per = (NPe + (int)G - 1) >> lg;
                    e0 = (int)mul_u24(gl, (uint32_t)per); if (e0 > NPe) e0 = NPe;
                    e1 = e0 + per; if (e1 > NPe) e1 = NPe;
                }
                // is the 8-mer at read position pp anywhere in a sequence?  (bitmap of all sequence 8-mers: global memory)
                // (the load is issued whether the block is wanted or not -- any code has its byte in the bitmap --
                // so that the two lookups of a lane travel together instead of each behind a branch of its own)
                auto fixed_block = [&](int pp, bool ok) -> bool {
                    const uint32_t code = cdp_code<KK>(roff + (uint32_t)(ok ? pp : 0));
                    const uint32_t bits = bmL[code >> 3];
                    return ok & (bool)((bits >> (code & 7u)) & 1u);
                };
                auto head_ok = [&](int jj) { return mine && jj <= me_ && (jj + 1) * KK <= rl; };
                auto tail_ok = [&](int jj) { const int pp = rl - (jj + 1) * KK; return mine && jj <= me_ && pp >= 0 && !((pp % KK) == 0 && pp <= me_ * KK); };
                const bool hhit = fixed_block((int)gl * KK, head_ok((int)gl));
                const bool thit = fixed_block(rl - ((int)gl + 1) * KK, tail_ok((int)gl));
                constexpr int NR = SS == 8 ? 6 : SS == 4 ? 12 : (LG == 3 || LG == 1) ? 24 : 18;  // lookups per lane and round (18: a 150-base read's 72 even positions over four lanes; 24: a 300-base read's 147 over eight -- 19 a lane -- or a 100-base read's 47 over two, one round instead of two)
                bool first = true;
                if constexpr (!DENSE) {
                for (int ee = e0; __any(ee < e1); ee += NR, first = false) {
                    const bool act = ee < e1;
#include "kernels_bp_lookup.inc"
                    const int nv = act ? (e1 - ee < NR ? e1 - ee : NR) : 0;
                    hA &= (1u << nv) - 1u;                                      // nv <= 24
                    const bool hh = first && hhit, th = first && thit;
                    const uint32_t c = (uint32_t)__popc(hA) + (hh ? 1u : 0u) + (th ? 1u : 0u);
                    const uint32_t inc = kvq_wave_incl_scan(c);
                    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                    if (tot) {
                        uint32_t idx = qn + inc - c;
                        while (hA) {
                            const int j = __ffs((int)hA) - 1; hA &= hA - 1u;
                            if (idx < BP_QW) q1[idx] = k | ((uint32_t)(SS * (ee + j)) << 9);        // beyond the cap: dropped, the stretch is redone in halves
                            idx++;
                        }
                        if (hh) { if (idx < BP_QW) q1[idx] = k | ((gl * KK) << 9) | (1u << BP_Q1_KIND); idx++; }
                        if (th && idx < BP_QW) { const uint32_t pt = (uint32_t)(rl - ((int)gl + 1) * KK); q1[idx] = k | (pt << 9) | (1u << BP_Q1_KIND); }
                        qn += tot;
                    }
                }
                // groups narrower than e+1 lanes: the remaining head and tail blocks, one push round each
                for (int t = (int)G; t <= me_; t += (int)G) {
                    const int jj = t + (int)gl;
#pragma unroll
                    for (int side = 0; side < 2; side++) {
                        const int pp = side ? rl - (jj + 1) * KK : jj * KK;
                        const bool hit = fixed_block(pp, side ? tail_ok(jj) : head_ok(jj));
                        const uint64_t mm = __ballot(hit);
                        if (mm) {
                            const uint32_t idx = qn + (uint32_t)__popcll(mm & kvq_lanemask_lt());
                            if (hit && idx < BP_QW) q1[idx] = k | ((uint32_t)pp << 9) | (1u << BP_Q1_KIND);
                            qn += (uint32_t)__popcll(mm);
                        }
                    }
                }
                }   // !DENSE
        KVQ_MARK("filter end / P4a" BP_SFX);
                BSTAMP(5);
                KVQ_SETPRIO(3);

                // ---- P4: candidates -> (candidate, index entry) work items, one per lane -> a window of sixteen bases of the diagonal
                // as 2-bit codes against the entry's own copy of the sequence around the seed (SeedEntry::ctx; equal bytes have equal
                // codes, so this only ever rejects, and nearly every false candidate ends here: TWO dependent loads, code -> range of
                // entries -> entry; round 3 went on to the 2-bit table for the bases) -> what is left goes through bp_verify_rest ----
                if constexpr (!DENSE) {
                const bool over = qn > BP_QW;                             // candidates were dropped
                const uint32_t qn_ok = (over || (dbg & 1u)) ? 0u : qn;
#if BP_STRAIGHT
                if (over) bail = true;
                else {
#else
                if (over && step > 1u) { step >>= 1; continue; }
                if (over) {
                    // ONE read has more candidates than the queue holds (step == 1): it alone goes to the exhaustive matcher behind the scan (the redo's
                    // list: trimmed and counted here, KVQ_REDO_TRIMMED), its tile carries on; a full list fails the batch
                    if (mine && gl == 0) {
                        const BpArgsPtr A = bp_args(A_);
                        const KvqRedo Rd(A->redo);
                        const uint32_t boff = g0 - ST_PRE + roff;
                        bool put = false;
                        if (A->redo) {
                            if (rl >= KVQ_LONG_READ) {
                                const unsigned int i = atomicAdd(Rd.count + 1, 1u);
                                if (i < KVQ_LONG_CAP) { Rd.read_off[KVQ_REDO_CAP - 1u - i] = boff; Rd.read_len[KVQ_REDO_CAP - 1u - i] = rl; put = true; }
                            }
                            if (!put) {
                                const unsigned int i = atomicAdd(Rd.count, 1u);
                                if (i < A->redo_cap) { Rd.rec_start[i] = KVQ_REDO_TRIMMED; Rd.read_off[i] = boff; Rd.read_len[i] = rl; }
                                put = true;                                  // (beyond the cap: kvq_dev_count fails the batch)
                            }
                        }
                        if (!put) S.fallback = 1u;
                        else atomicOr(A->fail, 2u);                      // (reported as records that went through the exhaustive kernels; the next launches of this scan object use the wide grids)
                    }
                }
#endif
#include "kernels_bp_p4.inc"
#if BP_STRAIGHT
                }
#endif
                } else {
                    // ---- dense tables, short seeds: candidates by the dozen per read (round 4).  Nothing is dropped and nothing filtered twice:
                    // the lanes push what a round of lookups found as far as the queue has room, the queue is drained (the work items of its
                    // candidates verified), and the pushing goes on where it stopped; the sparse kernel halves the stretch and filters it again
                    // when a queue overflows -- up to six times per stretch with the MTBC table x 8 ----
                    uint32_t hA = 0, hpos = 0, tpos = 0; bool hh = false, th = false;
                    int ee = e0, xt = (int)G;
                    int ee_of_hA = e0;                                          // the round the pending anchor bits belong to
                    bool done = false;
                    while (!done) {
                        bool full = false;
                        while (!full) {
                            if (!__any(hA != 0u || hh || th)) {
                                // nothing pending: the next round of lookups (spelled out here, not a lambda: what a lambda captures by reference lives in scratch memory)
                                ee_of_hA = ee;
                                if (__any(ee < e1)) {
                                    const bool act = ee < e1;
                                    uint32_t hA_;
                                    {
#include "kernels_bp_lookup.inc"
                                        hA_ = hA;
                                    }
                                    const int nv = act ? (e1 - ee < NR ? e1 - ee : NR) : 0;
                                    hA = hA_ & ((1u << nv) - 1u);
                                    if (first) { hh = hhit; th = thit; hpos = gl * KK; tpos = (uint32_t)(rl - ((int)gl + 1) * KK); first = false; }
                                    ee += NR;
                                } else if (xt <= me_) {                             // groups narrower than e + 1 lanes: the remaining head and tail blocks
                                    const int jj = xt + (int)gl;
                                    hpos = (uint32_t)(jj * KK); tpos = (uint32_t)(rl - (jj + 1) * KK);
                                    hh = fixed_block((int)hpos, head_ok(jj)); th = fixed_block((int)tpos, tail_ok(jj));
                                    xt += (int)G;
                                } else { done = true; break; }
                                continue;
                            }
                            const uint32_t c = (uint32_t)__popc(hA) + (hh ? 1u : 0u) + (th ? 1u : 0u);
                            const uint32_t inc = kvq_wave_incl_scan(c);
                            const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                            uint32_t idx = qn + inc - c;
                            while (hA && idx < BP_QW) {
                                const int j = __ffs((int)hA) - 1; hA &= hA - 1u;
                                q1[idx++] = k | ((uint32_t)(SS * (ee_of_hA + j)) << 9);
                            }
                            if (hh && idx < BP_QW) { q1[idx++] = k | (hpos << 9) | (1u << BP_Q1_KIND); hh = false; }
                            if (th && idx < BP_QW) { q1[idx++] = k | (tpos << 9) | (1u << BP_Q1_KIND); th = false; }
                            full = qn + tot >= BP_QW;
                            qn = qn + tot < BP_QW ? qn + tot : BP_QW;
                        }
                        {
                            const uint32_t qn_ok = (dbg & 1u) ? 0u : qn;
#include "kernels_bp_p4.inc"
                        }
                        qn = 0;
                    }
                }
                KVQ_SETPRIO(2);
                sub += step;
            }
            KVQ_SETPRIO(0);
            // the '@' / '+' checks of the pass's records (the bytes have come back long ago)
            if (have && gl == 0) {                                      // (lanes that fetched nothing never look)
                const uint32_t m = jn + 4u * k;
                if constexpr (late_probes) {
                    if (!(dbg & 8u)) {
                        c0 = text[m == 0 ? ST_PRE + (Ja & 15u) : (uint32_t)S.nl[m - 1] + 1u];
                        cp = c0 == '@' ? (uint32_t)text[(uint32_t)S.nl[m + 1] + 1u] : (uint32_t)'+';
                    } else { c0 = '@'; cp = '+'; }
                }
                if (!bail && (c0 != '@' || cp != '+')) {
                    const BpArgsPtr A = bp_args(A_);
                    const uint32_t rstart = m == 0 ? ST_PRE + (Ja & 15u) : (uint32_t)S.nl[m - 1] + 1u, plus = (uint32_t)S.nl[m + 1] + 1u;
                    const int64_t tf = A->fpos_base + (int64_t)g0;
                    if (c0 != '@') atomicMin(A->P.err, ((unsigned long long)(tf + rstart - ST_PRE) << 16) | (0ull << 8) | c0);
                    else atomicMin(A->P.err, ((unsigned long long)(tf + plus - ST_PRE) << 16) | (1ull << 8) | cp);
                }
            }
        KVQ_MARK("P4 end" BP_SFX);
            BSTAMP(6);
        }
