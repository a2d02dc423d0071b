// kvarq_amd/csrc/kvq_inflate.h -- raw DEFLATE (RFC 1951) for ONE BGZF member, host and device alike.
//
// No zlib, no heap: the caller hands in the compressed payload (n bytes), an output slot of exactly
// isize (<= 64 KiB) bytes and a workspace (the Huffman tables, ~5.5 KB: on the stack on the host, in LDS on
// the device).  The decoder never reads in[] at or past n and never writes output at or past isize: every
// length is checked before it is used.  It rejects what zlib's inflate rejects (over-subscribed or incomplete
// code sets with zlib's exception for a single code of one bit, literal/length symbols 286/287, distance
// codes 30/31, stored LEN/NLEN mismatch, a distance beyond the bytes written so far, ...).
//
// Success: the final block was reached AND exactly isize bytes were produced (the host reader's rule,
// st == Z_STREAM_END && avail_out == 0).  Bytes behind the final block are ignored.  CRC32 is not checked.
// Status: 0, or zlib's codes -3 (Z_DATA_ERROR: the bits are no valid DEFLATE stream) and -5 (Z_BUF_ERROR: the
// payload ends early, or the output would not be exactly isize bytes), -2 for bad arguments.
//
// A group of G::width lanes runs the decoder together: every lane holds the same bit-reader state (all read
// the same bytes), lane 0 makes the serial writes (literals, table bookkeeping), the group fills the fast
// tables and copies back-references and stored blocks together, G::sync() orders the two.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define KVQ_HD __host__ __device__ __forceinline__
#else
#define KVQ_HD inline
#endif

#define KVQ_INF_OK           0
#define KVQ_INF_STREAM_ERROR (-2)
#define KVQ_INF_DATA_ERROR   (-3)
#define KVQ_INF_BUF_ERROR    (-5)
#define KVQ_INF_MAX_ISIZE    65536
#define KVQ_INF_FAST         10          // bits resolved by one lookup; longer codes take the canonical walk

struct KvqHuff {
    uint16_t count[16];                  // codes per length
    uint16_t offs[16];                   // (scratch of the build)
    uint16_t symbol[288];                // symbols in canonical order
    uint16_t fast[1 << KVQ_INF_FAST];    // low KVQ_INF_FAST stream bits -> length << 9 | symbol; 0 = longer code or none
};

struct KvqInflateWork {
    KvqHuff lit, dist;
    uint8_t lens[288 + 32];
    int32_t flag;
};

// where the decoder's bytes go.  KvqFlatOut: straight into the isize-byte slot (the host).  The core has checked every
// position and length against isize before it calls one of these; a copy's bytes all lie behind o already.
struct KvqFlatOut {
    uint8_t *out;
    template <class G> KVQ_HD void lit(const G &g, uint32_t o, uint8_t v) { if (g.lane() == 0) out[o] = v; }
    template <class G> KVQ_HD void stored(const G &g, uint32_t o, const uint8_t *src, uint32_t len)
    {
        for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) out[o + i] = src[i];
    }
    template <class G> KVQ_HD void copy(const G &g, uint32_t o, uint32_t dist, uint32_t len)
    {
        g.sync();
        const uint8_t *src = out + (o - dist);
        if (dist >= len) for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) out[o + i] = src[i];
        else for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) out[o + i] = src[i % dist];
    }
    template <class G> KVQ_HD void finish(const G &g, uint32_t) { g.sync(); }
};

// one thread alone (the host)
struct KvqSerialGroup {
    static constexpr int width = 1;
    KVQ_HD int lane() const { return 0; }
    KVQ_HD void sync() const {}
};

// LSB-first bit reader over in[0, n).  Past the end it shifts in zeros; over() says whether more bits have been
// consumed than there are (checked after every step that consumes: a symbol decided by padding is an error).
struct KvqBits {
    const uint8_t *in; int64_t n, pos; uint64_t buf; int cnt;
    // to 57..64 bits: the bytes are loaded independently of each other (one wait for all of them on the device)
    KVQ_HD void fill()
    {
        if (cnt > 56) return;
        const int k = (64 - cnt) >> 3;
        uint64_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 8; j++)
            if (j < k && pos + j < n) w |= (uint64_t)in[pos + j] << (8 * j);
        buf |= w << cnt; pos += k; cnt += 8 * k;
    }
    KVQ_HD bool over() const { return pos * 8 - cnt > n * 8; }
    KVQ_HD void drop(int k) { buf >>= k; cnt -= k; }
    KVQ_HD uint32_t get(int k) { fill(); const uint32_t v = (uint32_t)(buf & ((1ull << k) - 1ull)); drop(k); return v; }
};

// canonical decode of the low bits of b, at most maxlen of them (puff.c's walk); *len = code length, -1 = none
KVQ_HD int kvq_huff_walk(const KvqHuff *h, uint64_t b, int maxlen, int *len)
{
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxlen; l++) {
        code |= (int)(b & 1u); b >>= 1;
        const int count = h->count[l];
        if (code - count < first) { *len = l; return h->symbol[index + (code - first)]; }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}

KVQ_HD int kvq_huff_decode(KvqBits &br, const KvqHuff *h)
{
    br.fill();
    const uint32_t e = h->fast[br.buf & ((1u << KVQ_INF_FAST) - 1u)];
    if (e) { br.drop((int)(e >> 9)); return (int)(e & 511u); }
    int len = 0;
    const int sym = kvq_huff_walk(h, br.buf, 15, &len);
    if (sym >= 0) br.drop(len);
    return sym;
}

// zlib's inflate_table rules on the number of codes of each length (count[1..15]), see kvq_huff_build.  1 = usable.
template <class C>
KVQ_HD int kvq_code_ok(const C *count, int kind)
{
    int max = 15;
    while (max >= 1 && count[max] == 0) max--;
    if (max == 0) return kind != 0;
    int left = 1;
    for (int l = 1; l <= 15; l++) { left <<= 1; left -= count[l]; if (left < 0) return 0; }
    return !(left > 0 && (kind == 0 || max != 1));
}

// zlib's inflate_table rules.  kind 0: the code-length code (must be complete; no codes at all is refused too,
// where zlib would go on to fail on a missing end-of-block code); kind 1: literal/length and distance codes
// (incomplete only as one code of one bit; no codes at all is accepted, any use of them then fails).
// Returns 1 when the set is usable.
template <class G>
KVQ_HD int kvq_huff_build(const G &g, KvqInflateWork *ws, KvqHuff *h, const uint8_t *len, int n, int kind)
{
    if (g.lane() == 0) {
        for (int l = 0; l < 16; l++) h->count[l] = 0;
        for (int s = 0; s < n; s++) h->count[len[s]]++;
        const int ok = kvq_code_ok(h->count, kind);
        if (ok) {
            h->offs[1] = 0;
            for (int l = 1; l < 15; l++) h->offs[l + 1] = (uint16_t)(h->offs[l] + h->count[l]);
            for (int s = 0; s < n; s++) if (len[s]) h->symbol[h->offs[len[s]]++] = (uint16_t)s;
        }
        ws->flag = ok;
    }
    g.sync();
    const int ok = ws->flag;
    if (ok)
        for (int i = g.lane(); i < (1 << KVQ_INF_FAST); i += G::width) {
            int l = 0;
            const int sym = kvq_huff_walk(h, (uint64_t)i, KVQ_INF_FAST, &l);
            h->fast[i] = (uint16_t)(sym >= 0 ? (l << 9 | sym) : 0);
        }
    g.sync();
    return ok;
}

// RFC 1951 3.2.5
KVQ_HD uint32_t kvq_len_base(int s)
{
    const uint16_t b[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
    return b[s];
}
KVQ_HD int kvq_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
KVQ_HD uint32_t kvq_dist_base(int s)
{
    const uint16_t b[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                             4097, 6145, 8193, 12289, 16385, 24577 };
    return b[s];
}
KVQ_HD int kvq_dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }

template <class G, class Out>
KVQ_HD int kvq_inflate_core(const G &g, KvqInflateWork *ws, const uint8_t *in, int64_t n, Out &out, uint32_t isize)
{
    if (n < 0 || isize > KVQ_INF_MAX_ISIZE) return KVQ_INF_STREAM_ERROR;
    KvqBits br; br.in = in; br.n = n; br.pos = 0; br.buf = 0; br.cnt = 0;
    uint32_t o = 0;                                   // bytes written
    int last = 0;
    do {
        last = (int)br.get(1);
        const int type = (int)br.get(2);
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (type == 3) return KVQ_INF_DATA_ERROR;
        if (type == 0) {
            // stored: to the byte boundary, LEN, NLEN, LEN bytes
            br.drop(br.cnt & 7);
            const uint32_t len = br.get(16), nlen = br.get(16);
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (len != (~nlen & 0xFFFFu)) return KVQ_INF_DATA_ERROR;
            const int64_t p = br.pos - br.cnt / 8;    // next unread byte (cnt is a multiple of 8 here)
            if (p + (int64_t)len > n || o + len > isize) return KVQ_INF_BUF_ERROR;
            out.stored(g, o, in + p, len);
            o += len;
            br.pos = p + len; br.buf = 0; br.cnt = 0;
            continue;
        }
        if (type == 1) {
            if (g.lane() == 0) {
                for (int s = 0; s < 288; s++) ws->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                for (int s = 0; s < 32; s++) ws->lens[288 + s] = 5;      // 30 and 31 complete the code; decoding one is an error
            }
            g.sync();
            kvq_huff_build(g, ws, &ws->lit, ws->lens, 288, 1);
            kvq_huff_build(g, ws, &ws->dist, ws->lens + 288, 32, 1);
        } else {
            const int nlen = (int)br.get(5) + 257, ndist = (int)br.get(5) + 1, ncode = (int)br.get(4) + 4;
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (nlen > 286 || ndist > 30) return KVQ_INF_DATA_ERROR;
            const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
            uint32_t cl[19];
            for (int i = 0; i < 19; i++) cl[i] = 0;
            for (int i = 0; i < ncode; i++) cl[i] = br.get(3);
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (g.lane() == 0) for (int i = 0; i < 19; i++) ws->lens[order[i]] = (uint8_t)cl[i];
            g.sync();
            if (!kvq_huff_build(g, ws, &ws->lit, ws->lens, 19, 0)) return KVQ_INF_DATA_ERROR;
            // the code lengths of both codes (lane 0 writes them; every lane keeps the last one for repeats)
            int idx = 0, prev = -1, has256 = 0;
            while (idx < nlen + ndist) {
                const int sym = kvq_huff_decode(br, &ws->lit);
                if (br.over()) return KVQ_INF_BUF_ERROR;
                if (sym < 0) return KVQ_INF_DATA_ERROR;
                int rep = 1, v = sym;
                if (sym >= 16) {
                    if (sym == 16) { if (prev < 0) return KVQ_INF_DATA_ERROR; v = prev; rep = 3 + (int)br.get(2); }
                    else if (sym == 17) { v = 0; rep = 3 + (int)br.get(3); }
                    else { v = 0; rep = 11 + (int)br.get(7); }
                    if (br.over()) return KVQ_INF_BUF_ERROR;
                    if (idx + rep > nlen + ndist) return KVQ_INF_DATA_ERROR;
                }
                if (idx <= 256 && 256 < idx + rep) has256 = v != 0;
                if (g.lane() == 0) for (int r = 0; r < rep; r++) ws->lens[idx + r] = (uint8_t)v;
                idx += rep; prev = v;
            }
            if (!has256) return KVQ_INF_DATA_ERROR;                       // no end-of-block code
            g.sync();
            if (!kvq_huff_build(g, ws, &ws->lit, ws->lens, nlen, 1)) return KVQ_INF_DATA_ERROR;
            if (!kvq_huff_build(g, ws, &ws->dist, ws->lens + nlen, ndist, 1)) return KVQ_INF_DATA_ERROR;
        }
        // the symbols of a Huffman block
        for (;;) {
            int sym = kvq_huff_decode(br, &ws->lit);
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (sym < 0) return KVQ_INF_DATA_ERROR;
            if (sym < 256) {
                if (o >= isize) return KVQ_INF_BUF_ERROR;
                out.lit(g, o, (uint8_t)sym);
                o++;
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return KVQ_INF_DATA_ERROR;                     // 286, 287
            const uint32_t len = kvq_len_base(sym) + br.get(kvq_len_extra(sym));
            const int ds = kvq_huff_decode(br, &ws->dist);
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (ds < 0 || ds >= 30) return KVQ_INF_DATA_ERROR;
            const uint32_t dist = kvq_dist_base(ds) + br.get(kvq_dist_extra(ds));
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (dist > o) return KVQ_INF_DATA_ERROR;                      // too far back
            if (o + len > isize) return KVQ_INF_BUF_ERROR;
            // every byte of the copy comes from the dist bytes in front of it, written already: no order among the lanes
            out.copy(g, o, dist, len);
            o += len;
        }
    } while (!last);
    if (o != isize) return KVQ_INF_BUF_ERROR;
    out.finish(g, o);
    return KVQ_INF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Plain gzip by chunks: one decoder starts at a bit offset of a whole gzip file's bytes, with the 32 KiB
// in front of it unknown, and writes 16-bit symbols -- 0..255 a byte, KVQ_INF_MARKER + k byte k of that unknown window (a
// back-reference copies symbols as they are, markers included).  It stops at the first block boundary at or past a bound,
// or where the host reader's text ends, and crosses gzip members by the host reader's rules (GzSerial in kvq_reader.hip).
// ---------------------------------------------------------------------------------------------------------------------

#define KVQ_INF_SLOT_FULL   (-7)         // the output would not fit the chunk's slot: nothing written past it
#define KVQ_INF_NEED_INPUT  (-8)         // in[] ends before the file does: the decode needs more of it
#define KVQ_INF_WINDOW      32768
#define KVQ_INF_MARKER      32768u       // symbol of byte k of the unknown window: KVQ_INF_MARKER + k

// GzSerial::skip_gz_header (workhorse.c:482-541) at byte p of a file whose bytes in[0, n) are at hand and which ends at
// file_end (>= n): the magic within `dist` other bytes, method 8, no FHCRC/encrypted/reserved flags, the optional fields.
// Reading past file_end is the host's EOF.  Returns the byte behind the header, -1 when there is none (*why: 1 magic bytes,
// 2 method, 3 flags; *stopped: the byte behind the last one read), -2 when the header reaches past n before file_end.
KVQ_HD int64_t kvq_gz_header(const uint8_t *in, int64_t n, int64_t file_end, int64_t p, int dist, int *why, int64_t *stopped = nullptr)
{
    bool need = false;
    auto getc = [&]() -> int { if (p >= file_end) return -1; if (p >= n) { need = true; return -1; } return in[p++]; };
    int state = 0, y = 0, c;
    for (c = getc(); state != 2 && y <= dist && c != -1; c = getc()) {
        if (c == 0x1F && state == 0) state = 1;
        else if (c == 0x8B && state == 1) state = 2;
        else { state = 0; y++; }
    }
    if (need) return -2;
    if (stopped) *stopped = p;
    if (state != 2) { *why = 1; return -1; }
    if (c != 8) { *why = 2; return -1; }
    const int flags = getc();
    if (need) return -2;
    if (stopped) *stopped = p;
    if (flags & (0x02 | 0x20 | 0xC0)) { *why = 3; return -1; }
    for (int i = 0; i < 6; i++) (void)getc();
    if (flags & 0x04) { int k = getc(); const int hi = getc(); k |= (int)((unsigned)hi << 8); while (k-- > 0) (void)getc(); }
    if (flags & 0x08) { do c = getc(); while (c > 0); }
    if (flags & 0x10) { do c = getc(); while (c > 0); }
    if (need) return -2;
    return p;
}

// The header of a dynamic block behind its BTYPE bits: HLIT, HDIST, HCLEN, the code-length code, the code lengths of both
// codes, with zlib's rules (the code-length code complete, both codes as kvq_huff_build accepts them, an end-of-block code).
// The block finder tests candidates with it and the chunk decoder reads every dynamic header with it, so that the two
// never disagree on a header.  lens (nullptr: not kept) gets the nlen + ndist lengths, written by lane 0.  Returns 0, or
// KVQ_INF_BUF_ERROR (the bits ran out) / KVQ_INF_DATA_ERROR.
template <class G>
KVQ_HD int kvq_dyn_header(const G &g, KvqBits &br, uint8_t *lens, int *pnlen, int *pndist)
{
    const int nlen = (int)br.get(5) + 257, ndist = (int)br.get(5) + 1, ncode = (int)br.get(4) + 4;
    if (br.over()) return KVQ_INF_BUF_ERROR;
    if (nlen > 286 || ndist > 30) return KVQ_INF_DATA_ERROR;
    const uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    uint8_t cl[19];
    for (int i = 0; i < 19; i++) cl[i] = 0;
    for (int i = 0; i < ncode; i++) cl[order[i]] = (uint8_t)br.get(3);
    if (br.over()) return KVQ_INF_BUF_ERROR;
    uint8_t cnt[8], sym[19], offs[8];
    for (int l = 0; l < 8; l++) cnt[l] = 0;
    for (int s = 0; s < 19; s++) cnt[cl[s]]++;
    if (cnt[0] == 19) {
        // zlib takes a code-length code without codes, reads every length as one bit and then misses the end-of-block code:
        // a file cut short within those bits ends its text there
        for (int i = 0; i < nlen + ndist; i += 32) (void)br.get(nlen + ndist - i < 32 ? nlen + ndist - i : 32);
        return br.over() ? KVQ_INF_BUF_ERROR : KVQ_INF_DATA_ERROR;
    }
    {
        uint8_t c16[16];
        for (int l = 0; l < 16; l++) c16[l] = l < 8 ? cnt[l] : 0;
        if (!kvq_code_ok(c16, 0)) return KVQ_INF_DATA_ERROR;
    }
    offs[1] = 0;
    for (int l = 1; l < 7; l++) offs[l + 1] = (uint8_t)(offs[l] + cnt[l]);
    for (int s = 0; s < 19; s++) if (cl[s]) sym[offs[cl[s]]++] = (uint8_t)s;
    uint16_t lc[16], dc[16];
    for (int l = 0; l < 16; l++) { lc[l] = 0; dc[l] = 0; }
    int idx = 0, prev = -1, has256 = 0;
    while (idx < nlen + ndist) {
        br.fill();
        // canonical walk of the (complete) code-length code: always a symbol within 7 bits
        uint64_t b = br.buf;
        int code = 0, first = 0, index = 0, s = -1;
        for (int l = 1; l <= 7; l++) {
            code |= (int)(b & 1u); b >>= 1;
            if (code - cnt[l] < first) { s = sym[index + (code - first)]; br.drop(l); break; }
            index += cnt[l]; first += cnt[l]; first <<= 1; code <<= 1;
        }
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (s < 0) return KVQ_INF_DATA_ERROR;
        int rep = 1, v = s;
        if (s >= 16) {
            if (s == 16) { if (prev < 0) return KVQ_INF_DATA_ERROR; v = prev; rep = 3 + (int)br.get(2); }
            else if (s == 17) { v = 0; rep = 3 + (int)br.get(3); }
            else { v = 0; rep = 11 + (int)br.get(7); }
            if (br.over()) return KVQ_INF_BUF_ERROR;
            if (idx + rep > nlen + ndist) return KVQ_INF_DATA_ERROR;
        }
        if (idx <= 256 && 256 < idx + rep) has256 = v != 0;
        for (int r = 0; r < rep; r++) {
            if (lens && g.lane() == 0) lens[idx + r] = (uint8_t)v;
            if (idx + r < nlen) lc[v]++; else dc[v]++;
        }
        idx += rep; prev = v;
    }
    if (!has256) return KVQ_INF_DATA_ERROR;                       // no end-of-block code
    if (!kvq_code_ok(lc, 1) || !kvq_code_ok(dc, 1)) return KVQ_INF_DATA_ERROR;
    *pnlen = nlen; *pndist = ndist;
    return 0;
}

// is there a block start at bit `bit` of in[0, n) that chunk decoding may start at: BFINAL 0, BTYPE 2 and a header that
// kvq_dyn_header accepts?
KVQ_HD bool kvq_gz_candidate(const uint8_t *in, int64_t n, int64_t bit)
{
    KvqBits br; br.in = in; br.n = n; br.pos = bit >> 3; br.buf = 0; br.cnt = 0;
    br.fill(); br.drop((int)(bit & 7));
    if (br.get(3) != 4u) return false;                            // BFINAL 0, BTYPE 2 (LSB first: 0b100)
    int nlen, ndist;
    return kvq_dyn_header(KvqSerialGroup(), br, nullptr, &nlen, &ndist) == 0;
}

// what one chunk decode found
struct KvqChunkRes {
    int64_t end_bit;        // end == 1: the block boundary it stopped at
    int64_t nsym;           // symbols written
    int64_t mstart;         // output offset of the last gzip member that started inside the chunk, -1 none
    int64_t lowest;         // lowest output position a back-reference reached (negative: into the unknown window), 0 none
    int64_t err_o;          // status != 0: output offset at which the failing block's output starts
    int64_t end_byte;       // end == 2: the byte the host reader has read up to when the text ends (see end_how)
    int64_t mbyte;          // the first byte of the DEFLATE data of the last member that started inside the chunk, -1 none
    int32_t status;         // 0, KVQ_INF_DATA_ERROR, KVQ_INF_SLOT_FULL or KVQ_INF_NEED_INPUT
    int32_t end;            // 1: stopped at a boundary at or past the bound; 2: the text ends
    int32_t end_how;        // end == 2: 1 at most 10 bytes behind a final block (end_byte: the byte behind it), 2 no member header
                            // behind it (end_byte: behind the bytes the header search read), 3 the file is cut short (file_end)
    int32_t pad_;
};

// symbol of output position p (< o) for a policy that keeps symbols at slot[p]: a marker in front of the chunk
#define KVQ_SYM_AT(slot, p) ((p) < 0 ? (uint16_t)(2 * KVQ_INF_MARKER + (p)) : (slot)[p])

// where the chunk decoder's symbols go on the host: straight into the slot
struct KvqMarkOut {
    uint16_t *slot;
    template <class G> KVQ_HD void lit(const G &g, int64_t o, uint8_t v) { if (g.lane() == 0) slot[o] = v; }
    template <class G> KVQ_HD void stored(const G &g, int64_t o, const uint8_t *src, uint32_t len)
    {
        for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) slot[o + i] = src[i];
    }
    template <class G> KVQ_HD void copy(const G &g, int64_t o, uint32_t dist, uint32_t len)
    {
        g.sync();
        const int64_t s0 = o - (int64_t)dist;
        if (dist >= len) for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) slot[o + i] = KVQ_SYM_AT(slot, s0 + i);
        else for (uint32_t i = (uint32_t)g.lane(); i < len; i += G::width) slot[o + i] = KVQ_SYM_AT(slot, s0 + i % dist);
    }
    template <class G> KVQ_HD void finish(const G &g, int64_t) { g.sync(); }
};

// the symbols of one stored or Huffman block (its 3 header bits read) at output offset o; 0 at its end, or a status
template <class G, class Out>
KVQ_HD int kvq_chunk_block(const G &g, KvqInflateWork *ws, KvqBits &br, int type, bool whole, Out &out, int64_t &o, int64_t cap,
                           int64_t wlo, int64_t &lowest)
{
    if (type == 3) return KVQ_INF_DATA_ERROR;
    if (type == 0) {
        br.drop(br.cnt & 7);
        const uint32_t len = br.get(16), nlen = br.get(16);
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (len != (~nlen & 0xFFFFu)) return KVQ_INF_DATA_ERROR;
        const int64_t p = br.pos - br.cnt / 8;
        const int64_t avail = br.n - p;
        // a file cut short inside a stored block: the host reader hands out what is there
        const uint32_t take = (int64_t)len <= avail ? len : (whole ? (uint32_t)(avail > 0 ? avail : 0) : 0u);
        if (take < len && !whole) return KVQ_INF_BUF_ERROR;
        if (o + take > cap) return KVQ_INF_SLOT_FULL;
        out.stored(g, o, br.in + p, take);
        o += take;
        if (take < len) return KVQ_INF_BUF_ERROR;
        br.pos = p + len; br.buf = 0; br.cnt = 0;
        return 0;
    }
    if (type == 1) {
        if (g.lane() == 0) {
            for (int s = 0; s < 288; s++) ws->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (int s = 0; s < 32; s++) ws->lens[288 + s] = 5;
        }
        g.sync();
        kvq_huff_build(g, ws, &ws->lit, ws->lens, 288, 1);
        kvq_huff_build(g, ws, &ws->dist, ws->lens + 288, 32, 1);
    } else {
        int nlen = 0, ndist = 0;
        const int st = kvq_dyn_header(g, br, ws->lens, &nlen, &ndist);
        if (st) return st;
        g.sync();
        if (!kvq_huff_build(g, ws, &ws->lit, ws->lens, nlen, 1)) return KVQ_INF_DATA_ERROR;
        if (!kvq_huff_build(g, ws, &ws->dist, ws->lens + nlen, ndist, 1)) return KVQ_INF_DATA_ERROR;
    }
    for (;;) {
        int sym = kvq_huff_decode(br, &ws->lit);
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (sym < 0) return KVQ_INF_DATA_ERROR;
        if (sym < 256) {
            if (o >= cap) return KVQ_INF_SLOT_FULL;
            out.lit(g, o, (uint8_t)sym);
            o++;
            continue;
        }
        if (sym == 256) return 0;
        sym -= 257;
        if (sym >= 29) return KVQ_INF_DATA_ERROR;
        const uint32_t len = kvq_len_base(sym) + br.get(kvq_len_extra(sym));
        const int ds = kvq_huff_decode(br, &ws->dist);
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (ds < 0 || ds >= 30) return KVQ_INF_DATA_ERROR;
        const uint32_t dist = kvq_dist_base(ds) + br.get(kvq_dist_extra(ds));
        if (br.over()) return KVQ_INF_BUF_ERROR;
        if (o - (int64_t)dist < wlo) return KVQ_INF_DATA_ERROR;   // too far back: before the member, or before a window of wlen bytes
        if (o + len > cap) return KVQ_INF_SLOT_FULL;
        if (o - (int64_t)dist < lowest) lowest = o - (int64_t)dist;
        out.copy(g, o, dist, len);
        o += len;
    }
}

// Decode the whole file's bytes in[0, n) (the file ends at file_end >= n) from bit start_bit, a block start, up to the first
// block boundary at or past stop_bit, into at most cap symbols.  wlen: bytes of the window in front of start_bit that may be
// referred to (32768: unknown, markers; 0 at a member's start; in between where the window is known to be short).
template <class G, class Out>
KVQ_HD void kvq_inflate_chunk(const G &g, KvqInflateWork *ws, const uint8_t *in, int64_t n, int64_t file_end, int64_t start_bit,
                              int64_t stop_bit, int32_t wlen, Out &out, int64_t cap, KvqChunkRes *r)
{
    KvqBits br; br.in = in; br.n = n; br.pos = start_bit >> 3; br.buf = 0; br.cnt = 0;
    br.fill(); br.drop((int)(start_bit & 7));
    const bool whole = n >= file_end;
    int64_t o = 0, wlo = -(int64_t)wlen, mstart = -1, lowest = 0, blk_o = 0, at = start_bit, end_byte = 0, mbyte = -1;
    int st = 0, end = 0, how = 0;
    for (;;) {
        at = br.pos * 8 - br.cnt;
        if (at >= stop_bit) { end = 1; break; }
        blk_o = o;
        const int last = (int)br.get(1), type = (int)br.get(2);
        st = br.over() ? KVQ_INF_BUF_ERROR : kvq_chunk_block(g, ws, br, type, whole, out, o, cap, wlo, lowest);
        if (st == KVQ_INF_BUF_ERROR) {                            // the bits ran out: the text ends where the file is cut short
            if (whole) { st = 0; end = 2; how = 3; end_byte = file_end; } else st = KVQ_INF_NEED_INPUT;
            break;
        }
        if (st) break;
        if (!last) continue;
        // behind a final block another member follows when more than 10 bytes are left, its header within 10 bytes (842-866)
        const int64_t e = (br.pos * 8 - br.cnt + 7) >> 3;
        if (file_end - e <= 10) { end = 2; how = 1; end_byte = e; break; }
        int why = 0;
        const int64_t h = kvq_gz_header(in, n, file_end, e, 10, &why, &end_byte);
        if (h == -2) { st = KVQ_INF_NEED_INPUT; break; }
        if (h < 0) { end = 2; how = 2; break; }
        br.pos = h; br.buf = 0; br.cnt = 0;
        wlo = o; mstart = o; mbyte = h;                           // a new member: an empty window
    }
    out.finish(g, o);
    if (g.lane() == 0) {
        r->end_bit = at; r->nsym = o; r->mstart = mstart; r->lowest = lowest; r->err_o = blk_o;
        r->status = st; r->end = end; r->end_how = how; r->end_byte = end_byte; r->mbyte = mbyte; r->pad_ = 0;
    }
}
