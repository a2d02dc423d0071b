// kvarq_amd/csrc/kvq_bam.h -- BAM records (SAM/BAM specification v1, section 4.2) as FastQ text, host and device alike
// (DESIGN section 12).  One source for the rules a record must keep (the block finder's candidate test, the device walk,
// the host twin and the error path all call kvq_bam_check) and for the text a record writes (kvq_bam_out_len,
// kvq_bam_char): the host twin kvq_bam_to_fastq_host and the GPU route cannot drift apart.
//
// Offsets are relative to a buffer p[0, n) that holds the record bytes read so far; `limit` (>= n) is where the file's
// inflated stream ends, relative to the same p.  Every read is checked against n.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define KVQ_BHD __host__ __device__ __forceinline__
#else
#define KVQ_BHD inline
#endif

#define KVQ_BAM_OK    0            // a well-formed record, wholly inside p[0, n)
#define KVQ_BAM_SHORT 1            // nothing checked so far breaks a rule, but the record ends behind n (more bytes come)
#define KVQ_BAM_BAD   2            // the record breaks a rule
#define KVQ_BAM_FIXED 36           // block_size and the 32 fixed bytes behind it
#define KVQ_BAM_MIN_RECORD 38      // the smallest well-formed record: the fixed bytes and a name of one character

// what the FastQ writer needs of a record (offsets relative to p)
struct KvqBamRec {
    int64_t next;                  // offset of the record behind this one
    int64_t name, seq, qual;       // where the read name, the 4-bit bases and the qualities start
    int32_t l_seq;
    uint32_t l_read_name, flag;
};

KVQ_BHD uint32_t kvq_bam_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
KVQ_BHD int32_t kvq_bam_i32(const uint8_t *p) { return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }

// the rules of a well-formed record at offset o: l_read_name >= 2, the name printable and NUL-terminated,
// refID and next_refID in [-1, n_ref), pos and next_pos >= -1, l_seq >= 0, the variable parts inside block_size, the record
// inside the file's stream.  What can be checked with the bytes there are is checked, so that a verdict of BAD never waits
// for bytes behind n, and a record that is BAD once all its bytes are there is BAD as soon as any of its broken rules shows.
KVQ_BHD int kvq_bam_check(const uint8_t *p, int64_t n, int64_t limit, int32_t n_ref, int64_t o, KvqBamRec *r)
{
    if (o + 4 > n) return n >= limit ? KVQ_BAM_BAD : KVQ_BAM_SHORT;
    const int64_t bs = kvq_bam_i32(p + o);
    if (bs < KVQ_BAM_MIN_RECORD - 4 || o + 4 + bs > limit) return KVQ_BAM_BAD;          // (the sizes rule below needs bs >= 34)
    if (o + KVQ_BAM_FIXED > n) return KVQ_BAM_SHORT;      // (so n < limit whenever a verdict is SHORT)
    const uint8_t *h = p + o + 4;
    const int32_t ref = kvq_bam_i32(h), pos = kvq_bam_i32(h + 4), nref = kvq_bam_i32(h + 20), npos = kvq_bam_i32(h + 24);
    const uint32_t lrn = h[8], ncig = kvq_bam_u16(h + 12), flag = kvq_bam_u16(h + 14);
    const int32_t lseq = kvq_bam_i32(h + 16);
    if (lrn < 2 || ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref || pos < -1 || npos < -1 || lseq < 0) return KVQ_BAM_BAD;
    if (32 + (int64_t)lrn + 4 * (int64_t)ncig + ((int64_t)lseq + 1) / 2 + (int64_t)lseq > bs) return KVQ_BAM_BAD;
    const int64_t nm = o + KVQ_BAM_FIXED;
    if (nm + lrn > n) return KVQ_BAM_SHORT;
    uint32_t bad = p[nm + lrn - 1];                       // the NUL
    for (uint32_t i = 0; i + 1 < lrn; i++) { const uint8_t c = p[nm + i]; bad |= (uint32_t)(c < '!' || c > '~'); }
    if (bad) return KVQ_BAM_BAD;
    if (o + 4 + bs > n) return KVQ_BAM_SHORT;
    r->next = o + 4 + bs; r->name = nm; r->seq = nm + lrn + 4 * (int64_t)ncig; r->qual = r->seq + ((int64_t)lseq + 1) / 2;
    r->l_seq = lseq; r->l_read_name = lrn; r->flag = flag;
    return KVQ_BAM_OK;
}

// the fields of a record kvq_bam_check has passed
KVQ_BHD KvqBamRec kvq_bam_parse(const uint8_t *p, int64_t o)
{
    const uint8_t *h = p + o + 4;
    KvqBamRec r;
    r.l_read_name = h[8]; r.flag = kvq_bam_u16(h + 14); r.l_seq = kvq_bam_i32(h + 16);
    r.next = o + 4 + (int64_t)kvq_bam_i32(p + o); r.name = o + KVQ_BAM_FIXED;
    r.seq = r.name + r.l_read_name + 4 * (int64_t)kvq_bam_u16(h + 12); r.qual = r.seq + ((int64_t)r.l_seq + 1) / 2;
    return r;
}

// the block finder's test of a candidate offset: 4 chained records are well-formed, or the chain reaches the end of p[0, n)
KVQ_BHD bool kvq_bam_candidate(const uint8_t *p, int64_t n, int64_t limit, int32_t n_ref, int64_t o)
{
    for (int k = 0; k < 4 && o < n; k++) {
        KvqBamRec r;
        const int v = kvq_bam_check(p, n, limit, n_ref, o, &r);
        if (v != KVQ_BAM_OK) return v == KVQ_BAM_SHORT;
        o = r.next;
    }
    return true;
}

// a record writes nothing when it is secondary or supplementary or holds no bases
KVQ_BHD bool kvq_bam_writes(const KvqBamRec &r) { return (r.flag & 0x900u) == 0 && r.l_seq > 0; }
KVQ_BHD uint32_t kvq_bam_suffix(const KvqBamRec &r) { const uint32_t m = r.flag & 0xC0u; return m == 0x40u || m == 0x80u ? 2u : 0u; }
// '@' name [/1|/2] '\n' bases '\n' '+' '\n' quals '\n'
KVQ_BHD int64_t kvq_bam_out_len(const KvqBamRec &r) { return kvq_bam_writes(r) ? (int64_t)r.l_read_name + kvq_bam_suffix(r) + 2 * (int64_t)r.l_seq + 5 : 0; }
KVQ_BHD bool kvq_bam_noqual(const uint8_t *p, const KvqBamRec &r) { return p[r.qual] == 0xFF; }

// byte j of the record's FastQ text (0 <= j < kvq_bam_out_len): every byte on its own, so that any lane can write any byte
KVQ_BHD uint8_t kvq_bam_char(const uint8_t *p, const KvqBamRec &r, int64_t j)
{
    const int64_t nl = (int64_t)r.l_read_name - 1, sl = kvq_bam_suffix(r), ls = r.l_seq, h = 1 + nl + sl;
    const bool rev = (r.flag & 0x10u) != 0;
    if (j == 0) return '@';
    if (j < 1 + nl) return p[r.name + j - 1];
    if (j < h) return j == 1 + nl ? '/' : ((r.flag & 0xC0u) == 0x40u ? '1' : '2');
    if (j == h) return '\n';
    if (j < h + 1 + ls) {
        const int64_t i = rev ? ls - 1 - (j - h - 1) : j - h - 1;
        const uint8_t b = p[r.seq + (i >> 1)];
        const uint32_t c = (i & 1) ? (b & 15u) : (b >> 4);
        // "=ACMGRSVTWYHKDBN"; the complement of code c is the code of the complementary base: bits reversed (A 1 <-> T 8, C 2 <-> G 4)
        const uint32_t k = rev ? (((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3)) : c;
        return (uint8_t)"=ACMGRSVTWYHKDBN"[k];
    }
    if (j == h + 1 + ls) return '\n';
    if (j == h + 2 + ls) return '+';
    if (j == h + 3 + ls) return '\n';
    if (j < h + 4 + 2 * ls) {
        if (p[r.qual] == 0xFF) return '"';
        const int64_t i = rev ? ls - 1 - (j - h - 4 - ls) : j - h - 4 - ls;
        return (uint8_t)(p[r.qual + i] + 33u);
    }
    return '\n';
}

// the header in front of the first record: magic, l_text, text, n_ref and n_ref reference entries.  Returns the first record's
// offset, -1 when the header is malformed, -2 when p[0, n) ends inside it
KVQ_BHD int64_t kvq_bam_header(const uint8_t *p, int64_t n, int32_t *n_ref)
{
    if (n < 4) return -2;
    if (p[0] != 'B' || p[1] != 'A' || p[2] != 'M' || p[3] != 1) return -1;
    if (n < 8) return -2;
    const int32_t l_text = kvq_bam_i32(p + 4);
    if (l_text < 0) return -1;
    int64_t o = 8 + (int64_t)l_text;
    if (o + 4 > n) return -2;
    const int32_t nr = kvq_bam_i32(p + o);
    if (nr < 0) return -1;
    o += 4;
    for (int32_t i = 0; i < nr; i++) {
        if (o + 4 > n) return -2;
        const int32_t l_name = kvq_bam_i32(p + o);
        if (l_name < 1) return -1;
        o += 4 + (int64_t)l_name + 4;
        if (o > n) return -2;
    }
    *n_ref = nr;
    return o;
}
