// kernels_bp_p4.inc -- P4 of kvq_scan_bp: the wave's qn_ok queued candidates -> work items -> 16-base window test -> bp_verify_rest
// (textually included by kernels_bp_pass.inc: the halving kernels run it once per stretch, the draining ones whenever their queue is full).
// BP_STRAIGHT 1: one window of work items and no loop round it; more than BP_Q2W of them set `bail` and nothing is tested
// in: qn_ok, q1, q2, me_, lane, text, g0, S, A_, bail
                if (qn_ok) {
                    typedef const __attribute__((address_space(1))) u32x4_t *GlbEntries;
                    typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
                    typedef const __attribute__((address_space(1))) u32x2_t __attribute__((aligned(4))) *GlbPairs;
                    GlbWords start; GlbEntries ent; int need;
                    {
                        const BpArgsPtr A = bp_args(A_);
                        start = (GlbWords)A->X.start; ent = (GlbEntries)A->X.ent;
                        need = (me_ + 1) * KK;                            // no alignment is shorter (kvq_seed_index_build)
                    }
                    // (the items are numbered in candidate order; the queue takes BP_Q2W of them a round -- one round, unless a read matches
                    // dozens of sequences of a dense table: then the candidates, a hundred at most, are simply walked again for the next window)
                    BTALLY(5, lane == 0);
#if BP_STRAIGHT
                    {
                        const uint32_t w0 = 0;
#else
                    for (uint32_t w0 = 0; ; w0 += BP_Q2W) {
#endif
                        uint32_t run = 0;
                        for (uint32_t q0 = 0; q0 < qn_ok; q0 += 64u) {
                            const uint32_t qi = q0 + lane;
                            uint32_t en0 = 0, ne = 0;
                            if (qi < qn_ok) {
                                const uint32_t cd = q1[qi];
                                BTALLY(0, w0 == 0u && (cd >> BP_Q1_KIND) == 0u); BTALLY(1, w0 == 0u && (cd >> BP_Q1_KIND) != 0u);
                                const uint32_t code = cdp_code<KK>((S.rinfo[cd & 511u] & 0xFFFFu) + ((cd >> 9) & 0xFFFFu));
                                const u32x2_t st = *(GlbPairs)(start + (code | ((cd >> BP_Q1_KIND) << (2 * KK))));      // (the ALL index's codes follow the anchors')
                                en0 = st.x; ne = st.y - st.x;
                            }
                            const uint32_t inc = kvq_wave_incl_scan(ne);
                            const uint32_t base = run + inc - ne - w0;                          // (unsigned: items in front of w0 wrap beyond the queue)
                            for (uint32_t j = 0; j < ne; j++)
                                if (base + j < BP_Q2W) q2[base + j] = (qi << 22) | (en0 + j);
                            run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
                        }
        KVQ_MARK("P4b" BP_SFX);
#if BP_STRAIGHT
                        if (run > BP_Q2W) bail = true;                          // (more work items than one window: the loops walk them)
                        const uint32_t n_items = bail ? 0u : run;
#else
                        const uint32_t n_items = run - w0 < BP_Q2W ? run - w0 : BP_Q2W;
#endif
                        for (uint32_t i0 = 0; i0 < n_items; i0 += 64u) {
                            BTALLY(4, lane == 0);
                            const uint32_t ii = i0 + lane;
                            bool alive = false;
                            uint32_t kind = 0, croff = 0, en_lo = 0, en_hi = 0; int p = 0, crl = 0;
                            BTALLY(2, ii < n_items);
                            if (ii < n_items) {
                                const uint32_t it = q2[ii];
                                const u32x4_t E = ent[it & 0x3FFFFFu];
                                const uint32_t cd = q1[it >> 22];
                                p = (int)((cd >> 9) & 0xFFFFu); kind = cd >> BP_Q1_KIND;
                                const uint32_t ri = S.rinfo[cd & 511u];
                                croff = ri & 0xFFFFu; crl = (int)(ri >> 16);
                                en_lo = E.x; en_hi = E.y;
                                const int q = (int)(E.x & 4095u), seql = (int)(E.y >> 20);
                                const int d = q - p;                     // sequence index = read index + d
                                const int a = d < 0 ? -d : 0;
                                const int L = (crl < seql - d ? crl : seql - d) - a;
                                if (L >= need) {
                                    // a window of min(L, 16) bases of the diagonal that lies inside the entry's 32: at the seed, or flush with the end of the overlap
                                    const int wn = L < 16 ? L : 16;
                                    const int w = p < a + L - wn ? p : a + L - wn;
                                    const uint32_t sh = 2u * (uint32_t)(w - p + 16);          // 0 .. 32
                                    const uint32_t seqw = (uint32_t)((((uint64_t)E.w << 32) | E.z) >> sh);
                                    const uint32_t v = cdp32(croff + (uint32_t)w) ^ seqw;
                                    uint32_t dm = (v | (v >> 1)) & 0x55555555u;
                                    if (wn < 16) dm &= (1u << (2 * wn)) - 1u;
                                    alive = __popc(dm) <= me_;
                                }
                            }
                            const bool any_alive = __any(alive);
                            BTALLY(3, alive); BTALLY(7, lane == 0 && any_alive);
                            if (any_alive) {
                                // onto the survivors' list (one atomic per wave), verified behind the kernel; what the list has no room for, here
                                const KvqSurvivors Sv(bp_args(A_)->surv);
                                if (Sv.count) {
                                    const uint64_t am = __ballot(alive);
                                    const uint32_t na = (uint32_t)__popcll(am);
                                    uint32_t at = rfl(S.sv_at[wave]), end = rfl(S.sv_end[wave]);
                                    if (at + na > end) {
                                        // the wave's chunk is used up: what is left of it is marked dead (read length 0), a new one is taken
                                        // (sixteen slots, or as many as this batch of work items needs)
                                        if (at + lane < end) Sv.item[at + lane].rl = 0;
                                        const uint32_t want = na > KVQ_SURV_CHUNK ? na : KVQ_SURV_CHUNK;
                                        uint32_t base = 0;
                                        if (lane == 0) base = atomicAdd(Sv.count, want);
                                        base = rfl(base);
                                        const uint32_t cap = bp_args(A_)->surv_cap;
                                        if (base + want <= cap) { at = base; end = base + want; }
                                        else {
                                            // (the list is full; slots of this chunk that lie inside it are nobody's: dead)
                                            if (lane < want && base + lane < cap) Sv.item[base + lane].rl = 0;
                                            at = end = 0;
                                        }
                                    }
                                    if (at + na <= end && end != 0u) {
                                        if (alive) {
                                            KvqSurvivor v;
                                            v.boff = g0 - ST_PRE + croff; v.rl = (uint16_t)crl; v.p = (uint16_t)p; v.en = ((uint64_t)en_hi << 32) | en_lo; v.kind = kind; v.pad = 0;
                                            Sv.item[at + (uint32_t)__popcll(am & kvq_lanemask_lt())] = v;
                                            alive = false;
                                        }
                                        at += na;
                                    }
                                    if (lane == 0) { S.sv_at[wave] = at; S.sv_end[wave] = end; }
                                }
                                if (__any(alive)) {
                                    // (what the byte-exact part needs of the parameters is fetched here, where it is wanted once in a blue moon: held
                                    // across the work-item loops it cost the hot path a dozen scalar registers)
                                    BpHot H; int64_t tile_fpos;
                                    {
                                        const BpArgsPtr A = bp_args(A_);
                                        H.cold = &A_->P; H.tab = (GlbBytes)A->P.tab; H.tab2 = (GlbWords)A->X.tab2; H.maxerrors = me_; H.minoverlap = A->P.minoverlap; H.pitch = A->X.pitch;
                                        tile_fpos = A->fpos_base + (int64_t)g0;
                                    }
                                    bp_verify_rest<KK>(H, text, alive, croff, crl, p, kind, en_lo, en_hi, tile_fpos, SS);
                                }
                            }
                        }
#if !BP_STRAIGHT
                        if (run <= w0 + BP_Q2W) break;
#endif
                    }
                }
