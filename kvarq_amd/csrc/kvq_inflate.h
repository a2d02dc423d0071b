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

// zlib's inflate_table rules.  kind 0: the code-length code (must be complete; no codes at all is refused too,
// where zlib would go on to fail on a missing end-of-block code); kind 1: literal/length and distance codes
// (incomplete only as one code of one bit; no codes at all is accepted, any use of them then fails).
// Returns 1 when the set is usable.
template <class G>
KVQ_HD int kvq_huff_build(const G &g, KvqInflateWork *ws, KvqHuff *h, const uint8_t *len, int n, int kind)
{
    if (g.lane() == 0) {
        int ok = 1;
        for (int l = 0; l < 16; l++) h->count[l] = 0;
        for (int s = 0; s < n; s++) h->count[len[s]]++;
        int max = 15;
        while (max >= 1 && h->count[max] == 0) max--;
        if (max == 0) ok = kind != 0;
        else {
            int left = 1;
            for (int l = 1; l <= 15 && ok; l++) { left <<= 1; left -= h->count[l]; if (left < 0) ok = 0; }
            if (ok && left > 0 && (kind == 0 || max != 1)) ok = 0;
        }
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
