// kvarq_amd/csrc/kvq_deflate.h -- raw DEFLATE (RFC 1951) of ONE BGZF member, host and device alike (include/kvarq_hip.h, DESIGN
// section 23): what the twin (kvq_deflate_bgzf_host, kvq_twins.cpp) and the kernel (kernels_deflate.hip) must not state twice --
// the symbol tables, the hash, the parse of a segment, the length-limited code builder, the header's run-length coding, the token
// costs, the bit writer and the CRC operators.  No heap, nothing of HIP beyond the function attributes.
//
// The output is a function of the block's bytes alone.  A block of n <= 65 280 bytes is cut into segments of 255 bytes; segment s
// is parsed greedily and serially from its first byte, and sees nothing of the parse of any other segment:
//   - a table of KVQ_DEFLATE_SLOTS slots per segment maps the hash of three bytes to the LAST position of the segment that has it
//     (positions p with p + 3 <= n; every position is entered, those inside a match too).  The parse of segment s keeps its own
//     table as it goes (the positions in front of the current one), and looks into the FINAL tables of segments s - 1 and s - 2,
//     which are functions of the text: the farthest byte a match can point at is the first of segment s - 2.
//   - at position p with p + 3 <= end of the segment the candidates are, in this order, the own table's, segment s - 1's and
//     segment s - 2's; a candidate's match is the common prefix of the RAW block at both positions, cut at the segment's end; the
//     longest wins, the first among equals.  Three bytes or more are a match (length 3 .. 255, distance 1 .. 762: a match begins three bytes in front of its segment's end at the latest), else block[p]
//     is a literal.
// The tokens of the segments in order, then end-of-block, are coded with one dynamic Huffman code (kvq_deflate_plan) unless the
// stored block is no longer.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define KVQ_DHD __host__ __device__ __forceinline__
#else
#define KVQ_DHD inline
#endif

#define KVQ_DEFLATE_BLOCK   65280u      // bytes of text a member takes (bgzip's 0xff00)
#define KVQ_DEFLATE_SEG     255u        // bytes a segment (a lane of the kernel) parses
#define KVQ_DEFLATE_SEGS    256u
#define KVQ_DEFLATE_SLOTS   128u        // slots of a segment's hash table
#define KVQ_DEFLATE_EMPTY   0xFFu       // (a position inside a segment is 0 .. 254)
#define KVQ_DEFLATE_MIN     3u
#define KVQ_DEFLATE_REACH   2u          // segments in front of its own a parse looks into
#define KVQ_BGZF_HEADER     18u
#define KVQ_BGZF_TRAILER    8u
#define KVQ_BGZF_EOF_BYTES  28u
#define KVQ_DEFLATE_MEMBER_MAX 65536u
#define KVQ_DEFLATE_LL      286
#define KVQ_DEFLATE_D       30
#define KVQ_DEFLATE_CL      19
#define KVQ_DEFLATE_TOKEN_MATCH 0x80000000u      // a token: a literal's byte, or this bit | length << 16 | distance

// ---- the symbol tables ----
KVQ_DHD uint32_t kvq_deflate_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }
// length 3 .. 258 -> its symbol 257 .. 285, the number of its extra bits and their value
KVQ_DHD void kvq_deflate_len_sym(uint32_t len, uint32_t &sym, uint32_t &nextra, uint32_t &extra)
{
    const uint32_t l = len - 3u;
    if (len == 258u) { sym = 285u; nextra = 0u; extra = 0u; }
    else if (l < 8u) { sym = 257u + l; nextra = 0u; extra = 0u; }
    else {
        nextra = kvq_deflate_log2(l) - 2u;
        sym = 257u + 4u * (nextra + 1u) + ((l >> nextra) & 3u);
        extra = l & ((1u << nextra) - 1u);
    }
}
// distance 1 .. 32 768 -> its symbol 0 .. 29, the number of its extra bits and their value
KVQ_DHD void kvq_deflate_dist_sym(uint32_t dist, uint32_t &sym, uint32_t &nextra, uint32_t &extra)
{
    const uint32_t d = dist - 1u;
    if (d < 4u) { sym = d; nextra = 0u; extra = 0u; }
    else {
        nextra = kvq_deflate_log2(d) - 1u;
        sym = 2u * (nextra + 1u) + ((d >> nextra) & 1u);
        extra = d & ((1u << nextra) - 1u);
    }
}
KVQ_DHD uint32_t kvq_deflate_ll_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
KVQ_DHD uint32_t kvq_deflate_d_extra(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }
KVQ_DHD uint32_t kvq_deflate_cl_extra(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }
// the order in which the header states the lengths of the code-length code
KVQ_DHD uint32_t kvq_deflate_cl_order(uint32_t i)
{
    const uint8_t order[KVQ_DEFLATE_CL] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    return order[i];
}

// ---- the hash and the tables ----
KVQ_DHD uint32_t kvq_deflate_hash(const uint8_t *p)
{
    return (((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) * 0x9E3779B1u) >> 25;
}
static_assert(KVQ_DEFLATE_SLOTS == 1u << (32 - 25), "the hash has as many values as a table has slots");
// slot `slot` of segment `seg` in a table block of KVQ_DEFLATE_SLOTS * KVQ_DEFLATE_SEGS bytes (the lanes of a wave lie side by side)
KVQ_DHD uint32_t kvq_deflate_slot(uint32_t seg, uint32_t slot) { return slot * KVQ_DEFLATE_SEGS + seg; }
KVQ_DHD uint32_t kvq_deflate_seg_begin(uint32_t seg, uint32_t n) { const uint32_t b = seg * KVQ_DEFLATE_SEG; return b < n ? b : n; }

// the final table of segment seg (every slot is written)
KVQ_DHD void kvq_deflate_final_table(const uint8_t *blk, uint32_t n, uint32_t seg, uint8_t *fin)
{
    for (uint32_t h = 0; h < KVQ_DEFLATE_SLOTS; h++) fin[kvq_deflate_slot(seg, h)] = KVQ_DEFLATE_EMPTY;
    const uint32_t b = kvq_deflate_seg_begin(seg, n), e = kvq_deflate_seg_begin(seg + 1u, n);
    for (uint32_t p = b; p < e && p + 3u <= n; p++) fin[kvq_deflate_slot(seg, kvq_deflate_hash(blk + p))] = (uint8_t)(p - b);
}

// the common prefix of blk[q ..] and blk[p ..], q < p, at most `most` bytes
KVQ_DHD uint32_t kvq_deflate_common(const uint8_t *blk, uint32_t q, uint32_t p, uint32_t most)
{
    uint32_t k = 0;
    while (k < most && blk[q + k] == blk[p + k]) k++;
    return k;
}

// The parse of segment seg: sink.literal(byte) and sink.match(length, distance) in the order of the text.  own: a table block whose
// slots of this segment the parse uses up (it ends as the segment's final table); fin: the block of the final tables.
template <class Sink>
KVQ_DHD void kvq_deflate_parse(const uint8_t *blk, uint32_t n, uint32_t seg, uint8_t *own, const uint8_t *fin, Sink &sink)
{
    const uint32_t b = kvq_deflate_seg_begin(seg, n), e = kvq_deflate_seg_begin(seg + 1u, n);
    for (uint32_t h = 0; h < KVQ_DEFLATE_SLOTS; h++) own[kvq_deflate_slot(seg, h)] = KVQ_DEFLATE_EMPTY;
    uint32_t p = b;
    while (p < e) {
        uint32_t best = 0, best_q = 0;
        if (p + KVQ_DEFLATE_MIN <= e) {
            const uint32_t h = kvq_deflate_hash(blk + p), most = e - p;
            for (uint32_t back = 0; back <= KVQ_DEFLATE_REACH && back <= seg; back++) {
                const uint32_t at = back ? fin[kvq_deflate_slot(seg - back, h)] : own[kvq_deflate_slot(seg, h)];
                if (at == KVQ_DEFLATE_EMPTY) continue;
                const uint32_t q = (seg - back) * KVQ_DEFLATE_SEG + at;
                const uint32_t k = kvq_deflate_common(blk, q, p, most);
                if (k > best) { best = k; best_q = q; }
            }
        }
        uint32_t step = 1u;
        if (best >= KVQ_DEFLATE_MIN) { sink.match(best, p - best_q); step = best; }
        else sink.literal(blk[p]);
        for (uint32_t i = p; i < p + step && i + 3u <= n; i++) own[kvq_deflate_slot(seg, kvq_deflate_hash(blk + i))] = (uint8_t)(i - b);
        p += step;
    }
}

// ---- the length-limited code builder ----
// Lengths of a prefix code for freq[0, nsym), none above `limit`: the Huffman tree of the used symbols, sorted by (count, symbol)
// ascending and merged through two queues (of two equal weights the leaf goes first); depths above the limit are cut to it and the
// Kraft sum is brought back to one by moving a code from the longest length that has one below the limit down a bit (as miniz
// does); the lengths then go to the symbols in sorted order, the longest to the rarest.  An unused symbol gets 0, a single used
// one 1 (DEFLATE's one-code case), no used one nothing.
struct KvqDeflateWork {
    uint16_t order[288];
    uint16_t parent[576];
    uint32_t weight[576];
};
KVQ_DHD void kvq_deflate_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *lens, KvqDeflateWork *w)
{
    int n = 0;
    for (int s = 0; s < nsym; s++) { lens[s] = 0; if (freq[s]) w->order[n++] = (uint16_t)s; }
    if (n == 0) return;
    if (n == 1) { lens[w->order[0]] = 1; return; }
    // (the keys are all different: any sort gives the one order)
    const int gaps[6] = { 132, 57, 23, 10, 4, 1 };
    for (int gi = 0; gi < 6; gi++) {
        const int gap = gaps[gi];
        for (int i = gap; i < n; i++) {
            const uint16_t s = w->order[i];
            const uint32_t f = freq[s];
            int j = i;
            for (; j >= gap; j -= gap) {
                const uint16_t t = w->order[j - gap];
                if (freq[t] < f || (freq[t] == f && t < s)) break;
                w->order[j] = t;
            }
            w->order[j] = s;
        }
    }
    for (int i = 0; i < n; i++) w->weight[i] = freq[w->order[i]];
    int leaf = 0, inner = n;
    for (int k = n; k < 2 * n - 1; k++) {
        uint32_t sum = 0;
        for (int two = 0; two < 2; two++) {
            int pick;
            if (leaf < n && (inner >= k || w->weight[leaf] <= w->weight[inner])) pick = leaf++;
            else pick = inner++;
            sum += w->weight[pick];
            w->parent[pick] = (uint16_t)k;
        }
        w->weight[k] = sum;
    }
    // (a node's parent has a higher index: the depths from the root down, in place of the weights)
    w->weight[2 * n - 2] = 0;
    for (int i = 2 * n - 3; i >= 0; i--) w->weight[i] = w->weight[w->parent[i]] + 1u;
    uint32_t count[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int i = 0; i < n; i++) count[w->weight[i] < (uint32_t)limit ? w->weight[i] : (uint32_t)limit]++;
    uint32_t total = 0;
    for (int l = limit; l > 0; l--) total += count[l] << (limit - l);
    while (total > (1u << limit)) {
        count[limit]--;
        for (int l = limit - 1; l > 0; l--) if (count[l]) { count[l]--; count[l + 1] += 2; break; }
        total--;
    }
    int at = 0;
    for (int l = limit; l > 0; l--) for (uint32_t c = 0; c < count[l]; c++) lens[w->order[at++]] = (uint8_t)l;
}

// the canonical codes of lens[0, nsym), each with its bits reversed: as it goes into the stream, first bit lowest
KVQ_DHD void kvq_deflate_codes(const uint8_t *lens, int nsym, uint16_t *codes)
{
    uint32_t count[16], next[16];
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < nsym; s++) count[lens[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l < 16; l++) { code = (code + count[l - 1]) << 1; next[l] = code; }
    for (int s = 0; s < nsym; s++) {
        const uint32_t l = lens[s];
        uint32_t c = l ? next[l]++ : 0u, r = 0;
        for (uint32_t i = 0; i < l; i++) { r = (r << 1) | (c & 1u); c >>= 1; }
        codes[s] = (uint16_t)r;
    }
}

// ---- the plan of a block: everything between its histograms and its bits ----
struct KvqDeflatePlan {
    uint32_t ll_freq[288], d_freq[32], cl_freq[20];      // in: the first two, end-of-block counted once
    uint8_t ll_len[288], d_len[32], cl_len[20];
    uint16_t ll_code[288], d_code[32], cl_code[20];
    uint8_t rle_sym[320], rle_extra[320];                // the header's run-length coding of ll_len[0, hlit) and d_len[0, hdist)
    uint32_t nrle, hlit, hdist, hclen;
    uint32_t header_bits, total_bits;                    // of the dynamic block: up to the first token, up to its end
    uint32_t stored;                                     // the stored block is no longer: it is the stream
    KvqDeflateWork work;
};

// The header's run-length coding of lens[0, n): a run of zeros takes 18 (11 .. 138 of them) while eleven or more are left, then 17
// (3 .. 10), then single zeros; a run of another length states it once, then takes 16 (3 .. 6 repeats) while three or more are
// left, then states it again.  Runs do not reach over a change of value, but do reach from the literal lengths into the distances.
KVQ_DHD uint32_t kvq_deflate_rle(const uint8_t *lens, uint32_t n, uint8_t *sym, uint8_t *extra)
{
    uint32_t out = 0;
    for (uint32_t i = 0; i < n; ) {
        const uint8_t v = lens[i];
        uint32_t run = 1;
        while (i + run < n && lens[i + run] == v) run++;
        i += run;
        if (v) { sym[out] = v; extra[out++] = 0; run--; }
        while (run) {
            uint32_t t = 1;
            if (!v && run >= 11u) { t = run < 138u ? run : 138u; sym[out] = 18; extra[out++] = (uint8_t)(t - 11u); }
            else if (!v && run >= 3u) { t = run; sym[out] = 17; extra[out++] = (uint8_t)(t - 3u); }
            else if (v && run >= 3u) { t = run < 6u ? run : 6u; sym[out] = 16; extra[out++] = (uint8_t)(t - 3u); }
            else { sym[out] = v; extra[out++] = 0; }
            run -= t;
        }
    }
    return out;
}

// From ll_freq and d_freq to the codes, the header and the choice.  n: the block's bytes.  Serial.
KVQ_DHD void kvq_deflate_plan(KvqDeflatePlan *P, uint32_t n)
{
    kvq_deflate_lengths(P->ll_freq, KVQ_DEFLATE_LL, 15, P->ll_len, &P->work);
    kvq_deflate_lengths(P->d_freq, KVQ_DEFLATE_D, 15, P->d_len, &P->work);
    // (a block without a match still states one distance code: of one bit, which every decoder takes)
    bool any = false;
    for (int s = 0; s < KVQ_DEFLATE_D; s++) any = any || P->d_len[s];
    if (!any) P->d_len[0] = 1;
    P->hlit = 257; P->hdist = 1;
    for (uint32_t s = 257; s < (uint32_t)KVQ_DEFLATE_LL; s++) if (P->ll_len[s]) P->hlit = s + 1u;
    for (uint32_t s = 1; s < (uint32_t)KVQ_DEFLATE_D; s++) if (P->d_len[s]) P->hdist = s + 1u;
    // (the two runs of lengths lie one behind the other for the run-length coding: in the work's order array, free again)
    uint8_t *all = (uint8_t *)P->work.order;
    for (uint32_t s = 0; s < P->hlit; s++) all[s] = P->ll_len[s];
    for (uint32_t s = 0; s < P->hdist; s++) all[P->hlit + s] = P->d_len[s];
    P->nrle = kvq_deflate_rle(all, P->hlit + P->hdist, P->rle_sym, P->rle_extra);
    for (int s = 0; s < 20; s++) P->cl_freq[s] = 0;
    for (uint32_t i = 0; i < P->nrle; i++) P->cl_freq[P->rle_sym[i]]++;
    kvq_deflate_lengths(P->cl_freq, KVQ_DEFLATE_CL, 7, P->cl_len, &P->work);
    // (a code-length code of one symbol is incomplete, which no decoder takes: a second, unused symbol shares the bit)
    int used = 0, one = 0;
    for (int s = 0; s < KVQ_DEFLATE_CL; s++) if (P->cl_len[s]) { used++; one = s; }
    if (used == 1) P->cl_len[one ? 0 : 1] = 1;
    P->hclen = 4;
    for (uint32_t i = 4; i < (uint32_t)KVQ_DEFLATE_CL; i++) if (P->cl_len[kvq_deflate_cl_order(i)]) P->hclen = i + 1u;
    kvq_deflate_codes(P->ll_len, KVQ_DEFLATE_LL, P->ll_code);
    kvq_deflate_codes(P->d_len, KVQ_DEFLATE_D, P->d_code);
    kvq_deflate_codes(P->cl_len, KVQ_DEFLATE_CL, P->cl_code);
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * P->hclen;
    for (uint32_t i = 0; i < P->nrle; i++) bits += P->cl_len[P->rle_sym[i]] + kvq_deflate_cl_extra(P->rle_sym[i]);
    P->header_bits = bits;
    for (uint32_t s = 0; s < (uint32_t)KVQ_DEFLATE_LL; s++) bits += P->ll_freq[s] * (P->ll_len[s] + kvq_deflate_ll_extra(s));
    for (uint32_t s = 0; s < (uint32_t)KVQ_DEFLATE_D; s++) bits += P->d_freq[s] * (P->d_len[s] + kvq_deflate_d_extra(s));
    P->total_bits = bits;
    P->stored = (bits + 7u) / 8u >= n + 5u ? 1u : 0u;
}
// the bytes of the member's DEFLATE stream
KVQ_DHD uint32_t kvq_deflate_stream_bytes(const KvqDeflatePlan *P, uint32_t n) { return P->stored ? n + 5u : (P->total_bits + 7u) / 8u; }

// ---- the bits ----
// Bits from position `bit` of a zeroed buffer of 32-bit words on, OR-ed in (M::orw(word, value): two writers meet in the word at
// their seam and nowhere else).  put() takes at most 32 bits a call, first bit lowest; close() the rest.
struct KvqPlainOr { static KVQ_DHD void orw(uint32_t *w, uint32_t v) { *w |= v; } };
template <class M>
struct KvqBitsOut {
    uint32_t *buf; uint64_t acc; uint32_t nacc, word;
    KVQ_DHD void open(uint32_t *b, uint32_t bit) { buf = b; acc = 0; nacc = bit & 31u; word = bit >> 5; }
    KVQ_DHD void put(uint32_t v, uint32_t nbits)
    {
        acc |= (uint64_t)v << nacc; nacc += nbits;
        if (nacc >= 32u) { M::orw(buf + word++, (uint32_t)acc); acc >>= 32; nacc -= 32u; }
    }
    KVQ_DHD void close() { if (nacc && (uint32_t)acc) M::orw(buf + word, (uint32_t)acc); nacc = 0; acc = 0; }
};

// ---- the token costs ----
KVQ_DHD uint32_t kvq_deflate_token_bits(const KvqDeflatePlan *P, uint32_t tok)
{
    if (!(tok & KVQ_DEFLATE_TOKEN_MATCH)) return P->ll_len[tok];
    uint32_t ls, ln, le, ds, dn, de;
    kvq_deflate_len_sym((tok >> 16) & 0x7FFFu, ls, ln, le);
    kvq_deflate_dist_sym(tok & 0xFFFFu, ds, dn, de);
    return P->ll_len[ls] + ln + P->d_len[ds] + dn;
}
template <class M>
KVQ_DHD void kvq_deflate_put_token(const KvqDeflatePlan *P, uint32_t tok, KvqBitsOut<M> &o)
{
    if (!(tok & KVQ_DEFLATE_TOKEN_MATCH)) { o.put(P->ll_code[tok], P->ll_len[tok]); return; }
    uint32_t ls, ln, le, ds, dn, de;
    kvq_deflate_len_sym((tok >> 16) & 0x7FFFu, ls, ln, le);
    kvq_deflate_dist_sym(tok & 0xFFFFu, ds, dn, de);
    o.put((uint32_t)P->ll_code[ls] | (le << P->ll_len[ls]), P->ll_len[ls] + ln);
    o.put((uint32_t)P->d_code[ds] | (de << P->d_len[ds]), P->d_len[ds] + dn);
}
// the dynamic block's header (BFINAL and BTYPE with it), from bit 0 on; serial
template <class M>
KVQ_DHD void kvq_deflate_put_header(const KvqDeflatePlan *P, KvqBitsOut<M> &o)
{
    o.put(1u | (2u << 1), 3);
    o.put(P->hlit - 257u, 5); o.put(P->hdist - 1u, 5); o.put(P->hclen - 4u, 4);
    for (uint32_t i = 0; i < P->hclen; i++) o.put(P->cl_len[kvq_deflate_cl_order(i)], 3);
    for (uint32_t i = 0; i < P->nrle; i++) {
        const uint32_t s = P->rle_sym[i];
        o.put((uint32_t)P->cl_code[s] | ((uint32_t)P->rle_extra[i] << P->cl_len[s]), P->cl_len[s] + kvq_deflate_cl_extra(s));
    }
}

// ---- the member's fixed bytes ----
// the 18 bytes in front of a member of `member_bytes` bytes in all
KVQ_DHD uint8_t kvq_bgzf_header_byte(uint32_t i, uint32_t member_bytes)
{
    const uint8_t h[16] = { 0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 'B', 'C', 2, 0 };
    return i < 16u ? h[i] : (uint8_t)((member_bytes - 1u) >> (8u * (i - 16u)));
}
// the empty member that ends a BGZF file
KVQ_DHD uint8_t kvq_bgzf_eof_byte(uint32_t i) { return i < 18u ? kvq_bgzf_header_byte(i, KVQ_BGZF_EOF_BYTES) : i == 18u ? 3 : 0; }
// the five bytes in front of a stored block of n bytes (final)
KVQ_DHD uint8_t kvq_deflate_stored_byte(uint32_t i, uint32_t n)
{
    return i == 0u ? 1 : i == 1u ? (uint8_t)n : i == 2u ? (uint8_t)(n >> 8) : i == 3u ? (uint8_t)~n : (uint8_t)(~n >> 8);
}
// the most bytes the members of a text of n bytes take
KVQ_DHD uint64_t kvq_deflate_members(uint64_t n) { return (n + KVQ_DEFLATE_BLOCK - 1u) / KVQ_DEFLATE_BLOCK; }
KVQ_DHD uint64_t kvq_deflate_bound_bytes(uint64_t n) { return n + kvq_deflate_members(n) * (KVQ_BGZF_HEADER + 5u + KVQ_BGZF_TRAILER); }

// ---- the CRC operators (CRC-32 of gzip, reflected: bit 31 of a word is x^0) ----
#define KVQ_CRC_POLY 0xEDB88320u
KVQ_DHD uint32_t kvq_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1u) ? KVQ_CRC_POLY : 0u);
    return i;
}
// the CRC-32 of p[0, n) behind a text whose CRC-32 is crc (0: none); table: kvq_crc_entry(0 .. 255)
KVQ_DHD uint32_t kvq_crc_bytes(const uint32_t *table, uint32_t crc, const uint8_t *p, uint32_t n)
{
    crc = ~crc;
    for (uint32_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return ~crc;
}
// a times b modulo the polynomial
KVQ_DHD uint32_t kvq_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? KVQ_CRC_POLY : 0u);
    }
    return p;
}
// x^(8 n) modulo the polynomial: the operator that moves a CRC n bytes to the front.  crc(A B) = kvq_crc_mul(kvq_crc_shift(|B|), crc(A)) ^ crc(B)
KVQ_DHD uint32_t kvq_crc_shift(uint32_t nbytes)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1u) p = kvq_crc_mul(p, sq);
        sq = kvq_crc_mul(sq, sq);
    }
    return p;
}
