/*
 * include/kvarq_hip.h -- C ABI of libkvarq_hip.so, the MI355X-native engine
 * behind KvarQ's `kvarq.engine` module.
 *
 * Plain pointers and sizes only (no torch / HIP types in the signatures);
 * "device pointer" arguments are ordinary HIP device addresses passed as
 * void*.  Every entry point names the reference interface it replaces
 * (/root/reference/csrc/workhorse.c unless said otherwise).  The Python side
 * (kvarq_amd/engine.py) binds these with ctypes; INTEGRATION.md shows the stub
 * a reference maintainer would add.
 *
 * Threading contract (same as the reference): one scan at a time
 * per process for kvq_findseqs (a second concurrent call fails with
 * KVQ_ERR_RUNTIME "findseqs() already running!"); kvq_poll_stats and
 * kvq_request_stop may be called from any thread while a scan runs.
 */
#ifndef KVARQ_HIP_H
#define KVARQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVQ_MAX_READLENGTH 1024          /* MAX_READLENGTH, workhorse.c:105 */
#define KVQ_SCANBUFSIZE    (1024*1024)   /* SCANBUFSIZE,    workhorse.c:15  */
#define KVQ_MUT_CLASSES    6             /* A C G T N other                 */

/* error classes; kvarq_amd/engine.py maps them to the exceptions the
 * reference raises (workhorse.c:577-605, 794-829, 1038-1047, 1260, 1295) */
enum {
    KVQ_OK          = 0,
    KVQ_ERR_FORMAT  = 1,   /* kvarq.fastq.FastqFileFormatException */
    KVQ_ERR_IO      = 2,   /* IOError      */
    KVQ_ERR_MEMORY  = 3,   /* MemoryError  */
    KVQ_ERR_RUNTIME = 4,   /* RuntimeError */
    KVQ_ERR_TYPE    = 5,   /* TypeError    */
    KVQ_ERR_DEVICE  = 6,   /* no usable GPU / HIP failure: RuntimeError, never a CPU fallback */
    KVQ_ERR_RESCAN  = 7    /* kvq_scan_finish after host batches: the hit arena was too small and has been enlarged;
                            * kvq_scan_reset and feed the same batches again (kvq_findseqs does so itself;
                            * device batches are replayed by the library).  kvarq_amd.scan.Scanner replays them. */
};

/* ---- engine.config / engine.get_config (workhorse.c:1484-1507) -------------
 * process-global, persists across calls; defaults maxerrors 0, minoverlap 20,
 * minreadlength 10, nthreads 1, Amin '!', Azero '!' (workhorse.c:71-75).
 * nthreads = number of host reader/inflate threads; it never changes results. */
typedef struct kvq_config {
    int32_t maxerrors;
    int32_t minoverlap;
    int32_t minreadlength;
    int32_t nthreads;
    int8_t  Amin;
    int8_t  Azero;
} kvq_config;

void kvq_config_set(const kvq_config *cfg);
void kvq_config_get(kvq_config *cfg);

/* ---- error state -----------------------------------------------------------
 * code + message of the last failed call on this thread's most recent scan
 * (the reference's `exception`/`errstr` globals, workhorse.c:95-97,1454-1458) */
int32_t kvq_last_error(char *msg, size_t cap);

/* ---- target-sequence table (the `sequences` argument of findseqs,
 *      workhorse.c:1300-1338; built by kvarq/analyse.py:352-354) -------------- */
typedef struct kvq_table kvq_table;

/* uploads the sequences (arbitrary bytes, any length >= 0) and builds the
 * device-side seed index for the given config (NULL = current global config).
 * Returns NULL on error (kvq_last_error). */
kvq_table *kvq_table_create(const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq,
                            const kvq_config *cfg);
void    kvq_table_destroy(kvq_table *t);
int32_t kvq_table_nseq(const kvq_table *t);
int64_t kvq_table_bases(const kvq_table *t);       /* sum of sequence lengths */
/* 1 if the seed-filter kernel serves sequence s, 0 if the exhaustive kernel does */
int32_t kvq_table_seq_is_seeded(const kvq_table *t, int32_t s);
int32_t kvq_table_seed_k(const kvq_table *t);

/* ---- counters ----------------------------------------------------------------
 * One flat int64 array in device memory, summable across GPUs with a single
 * all-reduce; slot KVQ_CTR_LONGEST is max-reduced instead.
 *   [0] records_parsed   (add_records_parsed, workhorse.c:387-392)
 *   [1] longest read + 1 (rls_longest + 1, workhorse.c:399-400; 0 = none)
 *   [2] hits             (length of the hit list)
 *   [3] reserved
 *   [4 .. 4+1024)                 readlengths      (rls_buf, workhorse.c:394-402)
 *   [.. +S)                       nseqhits         (seqhits, workhorse.c:435)
 *   [.. +S)                       nseqbasehits     (seqbasehits, workhorse.c:434)
 *   [.. +B)                       coverage         (Coverage.coverage per sequence, kvarq/analyse.py:76)
 *   [.. +6B)                      mutations        (Coverage.mutations as A,C,G,T,N,other counts, analyse.py:77-78)
 * with S = number of sequences, B = kvq_table_bases(). */
enum { KVQ_CTR_RECORDS = 0, KVQ_CTR_LONGEST = 1, KVQ_CTR_HITS = 2, KVQ_CTR_READLENGTHS = 4 };
int64_t kvq_counters_len(const kvq_table *t);
int64_t kvq_counters_off_nseqhits(const kvq_table *t);
int64_t kvq_counters_off_nseqbasehits(const kvq_table *t);
int64_t kvq_counters_off_coverage(const kvq_table *t);
int64_t kvq_counters_off_mutations(const kvq_table *t);
/* start of sequence s inside the coverage block (prefix sum of lengths) */
int64_t kvq_table_seq_offset(const kvq_table *t, int32_t s);

/* ---- scan object: scan_filepart (workhorse.c:976-1197) on the GPU ----------- */
typedef struct kvq_scan kvq_scan;

/* d_counters: device buffer of kvq_counters_len() int64 owned by the caller
 * (e.g. a torch tensor that is all-reduced afterwards), zeroed by the caller;
 * NULL = the scan allocates and zeroes its own.
 *
 * Several scan objects may be alive at once (each has its own stream): a caller may enqueue the next job
 * (kvq_scan_reset + kvq_scan_device) on one object before it waits for kvq_scan_finish of another -- the
 * reference's counterpart is a caller that starts the next file while it post-processes the last result.
 * The persistent scan kernels of a process are chained (one at a time, in the order they were enqueued);
 * the small kernels of a finish run beside the next scan. */
kvq_scan *kvq_scan_create(const kvq_table *t, void *d_counters);
void      kvq_scan_destroy(kvq_scan *s);

/* chunk boundaries fastq_read/fastq_rewind (workhorse.c:696-718, 737-956) put
 * on an in-memory stream: writes nchunks+1 offsets (cap >= nbytes/512Ki + 4);
 * returns nchunks, or -1 when a chunk holds no record start. Host only. */
int64_t kvq_chunk_offsets(const uint8_t *data, int64_t nbytes, int64_t *offsets, int64_t cap);

/* Scan nbytes of FastQ text resident in device memory (16-byte aligned,
 * readable up to the next 16-byte boundary).  chunk_off[0..nchunks] are host
 * offsets into d_data; every chunk starts a fresh record count like one
 * fastq_read buffer.  fpos_base = offset of d_data[0] in the concatenated
 * inflated stream (file_pos of a Hit is global, workhorse.c:777).  nbytes must
 * be at most 4 GiB - 1 MiB (offsets inside a batch are 32-bit).  Launches are asynchronous; d_data must stay valid until
 * kvq_scan_finish.  Returns KVQ_OK or an error code. */
int32_t kvq_scan_device(kvq_scan *s, const void *d_data, int64_t nbytes,
                        const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base);

/* same for host memory: copies to a device staging buffer first (the buffer
 * the reference fills with fread/inflate, workhorse.c:986,998) */
int32_t kvq_scan_host(kvq_scan *s, const void *h_data, int64_t nbytes,
                      const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base);

/* the same without waiting for the copy: one host batch is in flight at a time, so that the
 * caller can fill its next buffer (fread / inflate) while this one is copied and scanned.
 * h_data must stay untouched until kvq_scan_host_copied(s) has returned (or the next
 * kvq_scan_host_async / kvq_scan_host_drain / kvq_scan_finish).  kvq_scan_host_drain waits for the
 * batch in flight and settles it (a batch whose record-split speculation failed validation is
 * scanned again with the exhaustive kernels while its text is still staged). */
int32_t kvq_scan_host_async(kvq_scan *s, const void *h_data, int64_t nbytes,
                            const int64_t *chunk_off, int64_t nchunks, int64_t fpos_base);
int32_t kvq_scan_host_copied(kvq_scan *s);
int32_t kvq_scan_host_drain(kvq_scan *s);

/* wait for the device, fold hits into the counters, bring hits (canonical
 * order), hit bytes and counters to the host.  On a malformed
 * record returns KVQ_ERR_FORMAT with the reference's message
 * (workhorse.c:1037-1048) for the first bad record in stream order. */
int32_t kvq_scan_finish(kvq_scan *s);
/* optional, for a caller that keeps several scan objects in flight: every batch of this scan has been fed -- enqueue what
 * kvq_scan_finish would enqueue (the ordering of the hits, the gather, the copies to the host) behind the scan's kernels
 * now and return at once; kvq_scan_finish later only waits for it.  Without it the host sits out those kernels inside
 * kvq_scan_finish before it can enqueue its next job (they run beside another job's scan, slowly).  Feeding another batch
 * afterwards is allowed (kvq_scan_finish enqueues again).  Not part of the reference's interface: engine.findseqs is one call. */
int32_t kvq_scan_finish_begin(kvq_scan *s);

/* results, valid after kvq_scan_finish until kvq_scan_destroy; arrays are
 * owned by the scan object (engine.Hit fields, workhorse.c:1579-1586) */
int64_t        kvq_scan_n_hits(const kvq_scan *s);
const int32_t *kvq_scan_hit_seq_nr(const kvq_scan *s);
const int64_t *kvq_scan_hit_file_pos(const kvq_scan *s);
const int32_t *kvq_scan_hit_seq_pos(const kvq_scan *s);
const int32_t *kvq_scan_hit_length(const kvq_scan *s);
const int32_t *kvq_scan_hit_readlength(const kvq_scan *s);
const uint8_t *kvq_scan_hitseq_blob(const kvq_scan *s);       /* workhorse.c:437-439 */
const int64_t *kvq_scan_hitseq_offsets(const kvq_scan *s);    /* n_hits + 1 */
const int64_t *kvq_scan_counters(const kvq_scan *s);          /* host copy, kvq_counters_len() */
void          *kvq_scan_device_counters(const kvq_scan *s);   /* the device array (several ranks: the sum over all of them once finish has taken it) */
void          *kvq_scan_device_counters_own(const kvq_scan *s);   /* ... this rank's own counters, whatever finish has summed */
int64_t        kvq_scan_parsed(const kvq_scan *s);            /* fastq_parsed          */
int64_t        kvq_scan_total(const kvq_scan *s);             /* fastq_size_estimated  */

/* ---- the records of the hits (the reference's Analyser.extract_hits, kvarq/analyse.py:536-540) ----
 * A hit's RECORD is the bytes of the FastQ record whose bases line holds the hit's file_pos (file_pos is the first base of
 * the trimmed read, so all hits of one read share it): from the first byte of its identifier line to the end of its quality
 * line, that line's '\n' included; when the stream ends without a final newline, to the end of the stream.  The bytes are
 * raw (a '\r' stays).  They are gathered on the GPU while the batch's text is in device memory, each read's record stored
 * once, whatever number of hits it has.
 * kvq_scan_set_records: on or off, before the first batch or after kvq_scan_reset (KVQ_ERR_RUNTIME otherwise), and not with
 * a communicator (records are not gathered across ranks: KVQ_ERR_RUNTIME, from this call or from kvq_scan_set_comm).  A
 * store too small for the records of a scan works like an overflowing hit arena: grown, and KVQ_ERR_RESCAN for host batches.
 * After kvq_scan_finish: hit i's record is blob[off[i], off[i] + len[i]), hits in canonical order; kvq_scan_record_bytes:
 * bytes of the distinct records held.  NULL / 0 when records are off. */
int32_t        kvq_scan_set_records(kvq_scan *s, int32_t on);
const uint8_t *kvq_scan_record_blob(const kvq_scan *s);
/* ---- long reads: the read-list route ----
 * A text of reads of thousands of bases (PacBio HiFi, nanopore) fits no tile of the seed-filter scan kernel and ends in the
 * exhaustive kernels by default, which try every alignment.  kvq_scan_set_long_reads: mode 0 = off (the default), 1 = every
 * batch takes the read-list route, 2 = auto: a batch takes it when the average record among its first 128 KiB
 * (kvq_tile_for_text) is at least 2 * KVQ_MAX_READLENGTH + 25 bytes -- a read of 1024 bases -- or those hold too few lines
 * for an average.  On the route a batch's records are indexed and trimmed as the exhaustive pass does it, the sequences
 * without seeds go through the exhaustive matcher, and the seeded ones through the seed filter over the list of reads
 * (kvq_seed_list): the same hits, counters and records, found by K-mer lookups instead of alignments.  Where the table has no
 * seed index, or kvq_scan_force_exhaustive is on, a batch takes the ordinary path silently.  Before the first batch or after
 * kvq_scan_reset (KVQ_ERR_RUNTIME otherwise); kept across kvq_scan_reset; allowed with a communicator. */
int32_t        kvq_scan_set_long_reads(kvq_scan *s, int32_t mode);
const int64_t *kvq_scan_hit_record_off(const kvq_scan *s);
const int32_t *kvq_scan_hit_record_len(const kvq_scan *s);
int64_t        kvq_scan_record_bytes(const kvq_scan *s);

/* ---- the profile of the input (the reference's `kvarq show -Q q -i`, kvarq/cli.py:201-221, and the guesses of Fastq.__init__ --
 * there from samples of the file, here exact, from every record while its text is in device memory) ----
 * The profile covers exactly the records the scan counts in records_parsed: the complete four-newline records of every chunk
 * (a partial tail of a chunk is dropped, as the scan drops it).  For a record with newlines n0..n3 its BASES LINE is the
 * bytes strictly between n0 and n1, its SCORE LINE the bytes strictly between n2 and n3; bytes are raw (a '\r' is a byte
 * of its line).  One flat int64 array of kvq_profile_len(ncut) = 8 + 256 + 256 + 1025 + ncut * 1025 words:
 *   [0] records                      [1] bytes on bases lines          [2] bytes on score lines
 *   [3] records whose score line and bases line differ in length
 *   [4] longest bases line + 1 (0 = none; a maximum, not a sum)        [5..7] reserved, 0
 *   [8 .. +256)     score_bytes[b]: occurrences of byte value b on score lines
 *   [264 .. +256)   base_bytes[b]: the same for bases lines
 *   [520 .. +1025)  raw_lengths[min(L, 1024)] over the bases-line lengths L
 *   [1545 + 1025 k .. +1025), one block per cutoff k: longest_k + 1 (a maximum), then trimmed_k[0 .. 1023]
 * trimmed_k / longest_k: the engine's own quality trim at Amin = cutoffs[k] (workhorse.c:1055-1068, as kvq_trim_records
 * applies it: the longest run of score bytes >= Amin compared as signed char, the line's closing newline a byte like
 * the others -- it ends the last run when it is below Amin --, the first of equally long runs), counted like add_rl
 * (workhorse.c:394-402): before the length gate, lengths of 1024 and more in no bin but in longest_k.  So trimmed_k is, word
 * for word, the readlengths / KVQ_CTR_LONGEST part of the counters of a scan configured with Amin = cutoffs[k], whatever its
 * other settings.  (Not Fastq.cutoff, whose run at the end of a line does not count: the profile tells what the SCAN will do.)
 * 0 <= ncut <= KVQ_PROFILE_MAX_CUTOFFS; any byte value, duplicates included.
 *   [0] == sum(raw_lengths) == sum(trimmed_k) + (reads of 1024 and more at k) == counters[KVQ_CTR_RECORDS],
 *   sum(score_bytes) == [2], sum(base_bytes) == [1].
 * kvq_scan_set_profile: ncut >= 0 turns the profile on with these cutoffs, ncut < 0 off; before the first batch or after
 * kvq_scan_reset (KVQ_ERR_RUNTIME otherwise), and not with a communicator (the maxima would need a reduction of their own:
 * KVQ_ERR_RUNTIME, from this call or from kvq_scan_set_comm).  Every batch is then profiled once, whatever route brought it and
 * whatever the scan had to redo; kvq_scan_finish brings the array to the host.  kvq_scan_profile: the array (valid after
 * kvq_scan_finish until the next reset), NULL when the profile is off; kvq_scan_profile_cutoffs: writes the cutoffs (up to 8
 * bytes) and returns their number, -1 when off.  With the profile off nothing is enqueued or allocated for it. */
#define KVQ_PROFILE_MAX_CUTOFFS 8
enum { KVQ_PROF_RECORDS = 0, KVQ_PROF_BASE_LINE_BYTES = 1, KVQ_PROF_SCORE_LINE_BYTES = 2, KVQ_PROF_MISMATCHED = 3, KVQ_PROF_LONGEST = 4,
       KVQ_PROF_SCORE_BYTES = 8, KVQ_PROF_BASE_BYTES = 264, KVQ_PROF_RAW_LENGTHS = 520, KVQ_PROF_RAW_BINS = 1025,
       KVQ_PROF_CUTOFFS = 1545, KVQ_PROF_CUT_WORDS = 1025 };
int64_t        kvq_profile_len(int32_t ncut);
int32_t        kvq_scan_set_profile(kvq_scan *s, const uint8_t *cutoffs, int32_t ncut);
const int64_t *kvq_scan_profile(const kvq_scan *s);
int32_t        kvq_scan_profile_cutoffs(const kvq_scan *s, uint8_t *cutoffs8);
/* host only, plain C++: the CPU twin of the profile kernel over the same definition -- test infrastructure and the
 * definition in running code, not a fallback.  text[0, nbytes) with chunk_off[0..nchunks] as for kvq_scan_host; ADDS into
 * out[0, kvq_profile_len(ncut)) (the maxima as maxima).  KVQ_OK, or KVQ_ERR_RUNTIME for bad arguments. */
int32_t        kvq_profile_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                const uint8_t *cutoffs, int32_t ncut, int64_t *out);

/* ---- per-cycle quality and base composition: WHERE IN THE READ the profile's bytes stand ----
 * The per-cycle counts cover exactly the records the profile covers; bases line and score line are as defined there, bytes are
 * raw (a '\r' is a byte of its line).  CYCLE p of a record is byte p (0-based) of its bases line and, independently, byte p of
 * its score line: each line has its own length (a record whose two lines differ in length is legal; the profile counts it in
 * [3]).  Cycles 0 .. KVQ_CYCLES - 1 are counted (KVQ_CYCLES is the engine's KVQ_MAX_READLENGTH); bytes at positions of 1024 and
 * beyond are counted nowhere in this array.  One flat int64 array of kvq_cycles_len() = 2 * 1024 * 256 words:
 *   score[p][b]  at  p * 256 + b                 records whose score line has byte b at position p
 *   base[p][b]   at  1024 * 256 + p * 256 + b    the same for the bases line
 * Every word is a sum (no maxima).  With the profile of the same scan:
 *   for every p < 1024:  sum_b base[p][b] == sum(raw_lengths[L] for L > p);
 *   for every b:  sum_p score[p][b] <= score_bytes[b]  and  sum_p base[p][b] <= base_bytes[b], equalities when no line of that
 *   kind has more than 1024 bytes (what lies beyond cycle 1023 is the difference);
 *   sum_b score[0][b] is the number of records with a non-empty score line.
 * kvq_scan_set_cycles: on != 0 turns the counts on, 0 off; before the first batch or after kvq_scan_reset (KVQ_ERR_RUNTIME
 * otherwise).  They ride on the profile's record set and index: KVQ_ERR_RUNTIME when the scan keeps no profile, and
 * kvq_scan_set_profile(..., ncut < 0) turns them off with it (so a scan with a communicator keeps none either).  Every batch
 * is then counted once, right behind its profile pass; kvq_scan_finish brings the array to the host.  kvq_scan_cycles: the
 * array (valid after kvq_scan_finish until the next reset), NULL when off.  The device array and its pinned landing buffer
 * (4 MiB each) exist only while the option is on; with it off nothing is enqueued or allocated. */
#define KVQ_CYCLES 1024
int64_t        kvq_cycles_len(void);
int32_t        kvq_scan_set_cycles(kvq_scan *s, int32_t on);
const int64_t *kvq_scan_cycles(const kvq_scan *s);
/* host only, plain C++: the CPU twin of kvq_profile_cycles over the same definition -- test infrastructure and the definition
 * in running code, not a fallback.  Arguments as for kvq_profile_host; ADDS into out[0, kvq_cycles_len()). */
int32_t        kvq_cycles_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t *out);

/* ---- per-read GC, mean quality, N counts and duplication: WHAT THE INDIVIDUAL READS LOOK LIKE ----
 * Record set, bases line and score line are the profile's, with one difference: for everything below A TRAILING '\r' IS NOT
 * PART OF ITS LINE (a mean or a key with a '\r' in it is of no use).
 * The per-read distributions: one flat int64 array of kvq_reads_len() = 8 + 101 + 256 + 256 words, every word a sum:
 *   [0] records counted      [1] gc_none: records whose bases line holds no A C G T      [2] meanq_none: records with an
 *   empty score line         [3..7] 0
 *   [8 .. +101)    gc[k]: with a the bytes of the bases line in {A,C,G,T} and g those in {G,C} (upper case only), a record with
 *                  a > 0 counts in bin k = (200 g + a) / (2 a) -- integer division: the GC share in per cent, round half up
 *   [109 .. +256)  meanq[b]: with n the bytes of the score line and S their sum as unsigned bytes, a record with n > 0 counts in
 *                  bin b = (2 S + n) / (2 n): the mean score byte, round half up
 *   [365 .. +256)  ncount[min(c, 255)], c the 'N' bytes of the bases line
 * Lines may be of any length.  [0] == [1] + sum(gc) == [2] + sum(meanq) == sum(ncount) == the profile's records.
 * The duplication: a record's KEY is the first n = min(L, 64) bytes of its bases line of L bytes; a record with L == 0 has none
 * ("unkeyed").  Two records are duplicates when the 64-bit hashes of their keys are equal:
 *   key zero-padded to 64 bytes, as eight little-endian 64-bit words w0..w7;  G = 0x9E3779B97F4A7C15
 *   m(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *   h = m(n + G);  for i in 0..7: h ^= m(w_i + (i + 1) * G);  h = m(h);  if (h == 0) h = 1
 * (kvq_dup_hash in kvarq_amd/csrc/kvq_dup_hash.h: one __host__ __device__ function for the kernel and the CPU twin.)
 * The keys are counted in a hash table of C slots {hash, count}, C a power of two, the slot from the HIGH bits of h.  Key h is
 * TRACKED AT LEVEL s when its s LOW bits are zero.  The result is defined without reference to batches or launches: the LEVEL
 * is the smallest s for which the whole input holds at most C / 2 distinct tracked keys, and the table then holds exactly those
 * keys, each with its full count.  At level 0 that is the exact duplication of the input; above, the exact duplication of a
 * deterministic 1 / 2^s sample of the DISTINCT SEQUENCES, unbiased for the level histogram (FastQC's "first 100 000 sequences"
 * is neither, and a GPU cannot reproduce it run to run).  The result array, kvq_dup_len() = 8 + 16 + 16 words:
 *   [0] level     [1] C     [2] keyed records     [3] unkeyed records     [4] tracked records (the sum of the counts)
 *   [5] tracked distinct keys     [6..7] 0
 *   [8 .. +16) distinct[], [24 .. +16) records[]: the tracked keys, and their records, by the key's count, in bins with the
 *   lower bounds 1 2 3 4 5 6 7 8 9 10 50 100 500 1000 5000 10000
 *   [2] + [3] == the profile's records, sum(records[]) == [4], sum(distinct[]) == [5], at level 0 [4] == [2].
 * C is 2^24 (two tables: 512 MB of device memory, there only while the option is on): a choice, not a measurement.
 * KVQ_DUP_SLOTS=<n> in the environment, read when the option is turned on, shrinks it, to no less than 1024, rounded down to a
 * power of two (the tests reach levels above 0 with a few thousand records that way).
 * kvq_scan_set_read_stats: mode bit 0 the distributions, bit 1 the duplication, 0 both off; before the first batch or after
 * kvq_scan_reset (KVQ_ERR_RUNTIME otherwise).  They ride on the profile's record set and index as the cycles do: KVQ_ERR_RUNTIME
 * when the scan keeps no profile, off together with it, none with a communicator.  Every batch is then counted once, behind its
 * profile (and cycles) pass; wherever the profile is cleared the arrays AND THE TABLE are.  kvq_scan_reads / kvq_scan_dup: the
 * arrays (valid after kvq_scan_finish until the next reset), NULL when that option is off.  Device memory and landing buffers
 * exist only while an option is on; with both off nothing is enqueued or allocated. */
enum { KVQ_READS_RECORDS = 0, KVQ_READS_GC_NONE = 1, KVQ_READS_MEANQ_NONE = 2, KVQ_READS_GC = 8, KVQ_READS_GC_BINS = 101,
       KVQ_READS_MEANQ = 109, KVQ_READS_NCOUNT = 365, KVQ_READS_WORDS = 621 };
enum { KVQ_DUP_LEVEL = 0, KVQ_DUP_SLOTS = 1, KVQ_DUP_KEYED = 2, KVQ_DUP_UNKEYED = 3, KVQ_DUP_TRACKED_RECORDS = 4, KVQ_DUP_TRACKED_KEYS = 5,
       KVQ_DUP_DISTINCT = 8, KVQ_DUP_RECORDS = 24, KVQ_DUP_BINS = 16, KVQ_DUP_WORDS = 40 };
#define KVQ_READ_STATS 1
#define KVQ_READ_DUPLICATION 2
#define KVQ_DUP_DEFAULT_SLOTS (1 << 24)
#define KVQ_DUP_MIN_SLOTS 1024
int64_t        kvq_reads_len(void);
int64_t        kvq_dup_len(void);
int32_t        kvq_scan_set_read_stats(kvq_scan *s, int32_t mode);
const int64_t *kvq_scan_reads(const kvq_scan *s);
const int64_t *kvq_scan_dup(const kvq_scan *s);
/* host only, plain C++: the CPU twin of kvq_reads_records and the table over the same definition -- test infrastructure and
 * the definition in running code, not a fallback.  Arguments as for kvq_profile_host; slots: C (<= 0: the default; otherwise
 * clamped and rounded as KVQ_DUP_SLOTS is).  reads_out (or NULL): ADDS into [0, kvq_reads_len()).  dup_out (or NULL): WRITES
 * [0, kvq_dup_len()) -- the level is found from the final key set, as it is defined.  kvq_dup_hash_host: the hash of the key of
 * a bases line of L >= 1 bytes (kvq_dup_hash), for the tests. */
int32_t        kvq_reads_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t slots,
                              int64_t *reads_out, int64_t *dup_out);
uint64_t       kvq_dup_hash_host(const uint8_t *line, int64_t L);

/* ---- overrepresented sequences: WHICH SEQUENCES THE DUPLICATES ARE ----
 * Records, lines, key and hash are those of the duplication above: the profile's record set, a trailing '\r' is not part of its
 * line, the KEY is the first n = min(L, 64) bytes of the bases line, a record with L == 0 is "unkeyed", the hash is kvq_dup_hash.
 * Two keys with equal hashes are one key (the bytes kept are then those of whichever came first to its slot of the table: a
 * 2^-64 event per pair of keys).
 * The scan's records are numbered from 0 in the order its batches are fed, and within a batch in text order.  The CANDIDATES
 * are the distinct keys of the keyed records with a number < M, M = KVQ_OVER_DEFAULT_RECORDS = 2^18 (KVQ_OVER_RECORDS=<n> in the
 * environment, read when the option is turned on and clamped to KVQ_OVER_MIN_RECORDS .. KVQ_OVER_MAX_RECORDS: the tests' hook).
 * Every candidate's COUNT is the number of records OF THE WHOLE INPUT with its key; records whose key is no candidate count
 * nowhere but in `keyed`.  The result does not depend on batch cuts, slices, launches or rescans.  A candidate is LISTED when
 * count >= 2 and 1000 * count >= keyed (in integers; keyed: of the whole input): a share of 0.1 % and more.  Counts sum to at
 * most keyed, so at most KVQ_OVER_MAX_ROWS = 1000 candidates are listed -- a consequence, not a cut-off.
 * THE LIMIT: a sequence that is not among the first M records is not found, whatever its share.  In a file that is not sorted a
 * sequence with a share of 0.1 % is missing from the first 2^18 records with probability (1 - 0.001)^(2^18) = e^-262; a file
 * sorted by sequence or by position can hide one.
 * The result: one flat int64 array of kvq_over_len() = 8 + 1000 * 11 words:
 *   [0] M     [1] slots of the table: 4 * (M rounded up to a power of two), at least 1024     [2] keyed records
 *   [3] unkeyed records     [4] candidates     [5] records counted on candidates (the sum of the counts)     [6] listed rows
 *   [7] 0
 *   [8 + 11 r .. +11), r < [6]: row r = {hash, count, n, w0 .. w7}, the key zero-padded to 64 bytes as eight little-endian words;
 *   zeros behind the last row.  The rows are in canonical order: count descending, ties by hash ascending AS UNSIGNED.
 *   [2] + [3] == the profile's records, [5] <= [2], [5] == [2] when the input has at most M records.
 * kvq_scan_set_overrepresented: on != 0 turns the pass on, 0 off; rules as for kvq_scan_set_cycles: before the first batch or after
 * kvq_scan_reset, KVQ_ERR_RUNTIME when the scan keeps no profile, off together with it, none with a communicator.  Every batch is
 * then counted once, behind its other passes; wherever the profile is cleared the table is, and the numbering starts at 0 again.
 * kvq_scan_over: the array (valid after kvq_scan_finish until the next reset), NULL when the option is off.  The table (88 bytes a
 * slot: 92 MB at the default M) and the landing buffer exist only while the option is on; off, nothing is enqueued or allocated. */
enum { KVQ_OVER_M = 0, KVQ_OVER_SLOTS = 1, KVQ_OVER_KEYED = 2, KVQ_OVER_UNKEYED = 3, KVQ_OVER_CANDIDATES = 4, KVQ_OVER_COUNTED = 5,
       KVQ_OVER_LISTED = 6, KVQ_OVER_ROWS = 8, KVQ_OVER_ROW_WORDS = 11, KVQ_OVER_ROW_HASH = 0, KVQ_OVER_ROW_COUNT = 1, KVQ_OVER_ROW_N = 2,
       KVQ_OVER_ROW_KEY = 3, KVQ_OVER_MAX_ROWS = 1000, KVQ_OVER_WORDS = 8 + 1000 * 11 };
#define KVQ_OVER_DEFAULT_RECORDS (1 << 18)
#define KVQ_OVER_MIN_RECORDS 16
#define KVQ_OVER_MAX_RECORDS (1 << 22)
int64_t        kvq_over_len(void);
int32_t        kvq_scan_set_overrepresented(kvq_scan *s, int32_t on);
const int64_t *kvq_scan_over(const kvq_scan *s);
/* host only, plain C++: the CPU twin of kvq_over_records and kvq_over_select over the same definition -- test infrastructure and
 * the definition in running code, not a fallback.  Arguments as for kvq_profile_host (the text is ONE scan's input, its records
 * numbered in text order); records_limit: M (<= 0: the default; otherwise clamped as KVQ_OVER_RECORDS is).  WRITES
 * out[0, kvq_over_len()). */
int32_t        kvq_over_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int64_t records_limit,
                             int64_t *out);

/* ---- adapter content: WHERE ADAPTERS BEGIN, PER READ ----
 * Record set, bases line, '\r': the record set and the bases line are the profile's; as for the duplication a trailing '\r' is not
 * part of the line.  L is the line's length after that.
 * PROBES: n probes, 1 <= n <= 8 (KVQ_ADAPT_MAX_PROBES), each m_k bytes long, 8 <= m_k <= 32 (KVQ_ADAPT_MIN_PROBE ..
 * KVQ_ADAPT_MAX_PROBE), every byte one of upper-case A C G T; anything else is refused with KVQ_ERR_RUNTIME.  Matching is on BYTES:
 * 'a' does not match 'A', 'N' matches nothing.  (A kernel that compares the 2-bit codes (byte >> 1) & 3 must also know that the
 * bytes are upper-case A C G T: 'G' and 'N' share a code, and so do a base and its lower-case letter.)
 * PER RECORD AND PROBE k: FIRST_k is the smallest p with p + m_k <= L and line[p, p + m_k) == probe_k, "none" when there is no such
 * p.  TAIL_k is considered only when FIRST_k is none: the largest t with T <= t <= min(m_k - 1, L) and line[L - t, L) ==
 * probe_k[0, t), otherwise "none".  T = 6 (KVQ_ADAPT_MIN_TAIL): a choice, not a measurement -- a random tail matches a probe with
 * probability about 4/3 * 4^-6 = 0.03 %.
 * CLIP of the record is the minimum of FIRST_k over all probes k that have one, of L - TAIL_k over all probes k that have a tail
 * match, and of L: the length an adapter clip would leave.
 * THE RESULT: one flat int64 array of kvq_adapt_len() = 8 + 8 * 1064 + 1025 = 9545 words.  Every word is a sum; the result is
 * independent of batch cuts, launches, routes and rescans.
 *   [0] n     [1] records     [2] records with a full occurrence of any probe
 *   [3] records with no full occurrence of any probe but a tail match of one     [4..7] 0
 *   [8 + 1064 k .. +1064): the block of probe k (blocks of k >= n are zero):
 *       +0 m_k     +1 records with FIRST_k     +2 of those, the records with FIRST_k >= 1024     +3 records with TAIL_k     +4..7 0
 *       +8 .. +1032: first_k[p] for p < 1024     +1032 .. +1064: tail_k[t] (words with t < T or t >= m_k stay 0)
 *   [8520 .. +1025): clip[min(CLIP, 1024)]
 *   sum(first_k) + block[2] == block[1], sum(tail_k) == block[3], sum(clip) == [1] == the profile's records, [2] + [3] <= [1];
 *   clip == the profile's raw_lengths word for word on an input without any match and without '\r'.
 * kvq_scan_set_adapters: n probes of lens[k] bytes turn the pass on, n == 0 turns it off; rules as for kvq_scan_set_cycles: before
 * the first batch or after kvq_scan_reset, KVQ_ERR_RUNTIME when the scan keeps no profile (and therefore with a communicator), off
 * together with the profile.  Every batch is then counted once, behind its other passes; wherever the profile is cleared the array
 * is.  kvq_scan_adapters: the array (valid after kvq_scan_finish until the next reset), NULL when the option is off.  The device
 * array and the landing buffer exist only while the option is on; off, nothing is enqueued or allocated. */
enum { KVQ_ADAPT_N = 0, KVQ_ADAPT_RECORDS = 1, KVQ_ADAPT_WITH_FULL = 2, KVQ_ADAPT_TAIL_ONLY = 3, KVQ_ADAPT_BLOCKS = 8,
       KVQ_ADAPT_BLOCK_WORDS = 1064, KVQ_ADAPT_B_M = 0, KVQ_ADAPT_B_FIRST = 1, KVQ_ADAPT_B_BEYOND = 2, KVQ_ADAPT_B_TAIL = 3,
       KVQ_ADAPT_B_FIRST_BINS = 8, KVQ_ADAPT_POSITIONS = 1024, KVQ_ADAPT_B_TAIL_BINS = 1032, KVQ_ADAPT_MAX_PROBES = 8,
       KVQ_ADAPT_MIN_PROBE = 8, KVQ_ADAPT_MAX_PROBE = 32, KVQ_ADAPT_MIN_TAIL = 6, KVQ_ADAPT_CLIP = 8 + 8 * 1064,
       KVQ_ADAPT_CLIP_BINS = 1025, KVQ_ADAPT_WORDS = 8 + 8 * 1064 + 1025 };
int64_t        kvq_adapt_len(void);
int32_t        kvq_scan_set_adapters(kvq_scan *s, const uint8_t *const *probes, const int32_t *lens, int32_t n);
const int64_t *kvq_scan_adapters(const kvq_scan *s);
/* host only, plain C++: the CPU twin of kvq_adapt_records over the same definition -- test infrastructure and the definition in
 * running code, not a fallback.  Arguments as for kvq_profile_host; probes as for kvq_scan_set_adapters (n == 0 is refused here).
 * ADDS into out[0, kvq_adapt_len()), but for [0] and the blocks' +0, which it sets. */
int32_t        kvq_adapt_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                              const uint8_t *const *probes, const int32_t *lens, int32_t n, int64_t *out);

/* ---- adapter clipping: THE SCORES OF AN ADAPTER BECOME PHRED 0 AHEAD OF THE TRIM ----
 * The trim takes the longest run of score bytes >= Amin, compared as signed chars (workhorse.c:1055-1068).  With the score bytes
 * from the adapter's first base on set to '!' before the scan, no trimmed read reaches into the adapter, whichever kernel trims it.
 * MASK(text, chunk_off, probes): the record set is the profile's (every complete four-newline record of every chunk, newlines at
 * n0 < n1 < n2 < n3).  Per record: L and CLIP are those of the adapter content above, word for word (the bases line without a
 * trailing '\r'; FIRST_k, TAIL_k with T = 6; CLIP the minimum of those and L).  S is the length of the score line -- the bytes
 * strictly between n2 and n3 -- less a trailing '\r'.  A record is CLIPPED when CLIP < L; then every byte text[n2 + 1 + p] with
 * CLIP <= p < S becomes '!' (0x21).  Nothing else changes: not a '\r', a newline, the bases line, an unclipped record or a score
 * line no longer than CLIP.  MASK is idempotent: the bases decide, and the bases do not change.
 * THE RESULT: one flat int64 array of kvq_clip_len() = 8 words, every word but [0] a sum over the records:
 *   [0] n     [1] records     [2] clipped records     [3] sum of max(0, S - CLIP) over the clipped records (positions, not
 *   changes: the same on a text that is already masked)     [4] sum of L - CLIP     [5..7] 0
 * THE CONTRACT: for every route and option the scan of `text` with the clip on returns what the same scan without it returns on
 * MASK(text): hits, hit bytes, stats, counters, coverage, mutations, the records of the hits (their score lines carry the '!')
 * and every word of the profile; the adapter content is that of the unmasked text, the bases being the same.
 * THE MASK IS WRITTEN INTO THE BATCH WHERE IT LIES: the library's staging buffer of a host batch, its own buffer on the
 * device-inflate, gzip and BAM routes, and THE CALLER'S BUFFER for kvq_scan_device -- with the clip on, that buffer is written.
 * A batch that runs again (the redo of a batch whose speculation failed, a rescan after an arena overflow, a device batch named
 * again) is masked again, which changes nothing; the eight words are cleared wherever the hit arena is and counted anew.
 * kvq_scan_set_clip: n probes (rules as for kvq_scan_set_adapters) turn the clip on, n == 0 turns it off; before the first batch
 * or after kvq_scan_reset, as kvq_scan_set_cycles.  It needs no profile and is allowed with a communicator (the words are then
 * the rank's own).  KVQ_ERR_RUNTIME for probes outside the rules and for a table whose Amin, as a signed char, is <= '!': there
 * '!' ends no run and a mask cannot clip.  kvq_scan_clip: the array (valid after kvq_scan_finish until the next reset), NULL
 * when the option is off.  Off, nothing is enqueued or allocated. */
enum { KVQ_CLIP_N = 0, KVQ_CLIP_RECORDS = 1, KVQ_CLIP_CLIPPED = 2, KVQ_CLIP_MASKED = 3, KVQ_CLIP_BASES_CUT = 4, KVQ_CLIP_WORDS = 8 };
int64_t        kvq_clip_len(void);
int32_t        kvq_scan_set_clip(kvq_scan *s, const uint8_t *const *probes, const int32_t *lens, int32_t n);
const int64_t *kvq_scan_clip(const kvq_scan *s);
/* host only, plain C++: the CPU twin of kvq_clip_records over the same definition -- test infrastructure and the definition in
 * running code, not a fallback.  Arguments as for kvq_adapt_host, but the text is WRITTEN: masked in place.  ADDS into
 * out[0, kvq_clip_len()), but for [0], which it sets. */
int32_t        kvq_clip_host(uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                             const uint8_t *const *probes, const int32_t *lens, int32_t n, int64_t *out);

/* ---- adapter probes that tolerate mismatches: ONE INTEGER, per, FOR THE CONTENT PASS AND THE CLIP ----
 * per == 0 is the rule of the two sections above, word for word.  Otherwise 10 <= per <= 32 (KVQ_ADAPT_MIN_PER ..
 * KVQ_ADAPT_MAX_PER), and a comparison over `len` bases may differ from the probe in at most E(len) = len / per positions
 * (integer division).  per = 10 is cutadapt's default rate; the lower bound keeps E <= 3 and every tail shorter than 10 bases
 * exact.
 * WHAT COUNTS AS A MISMATCH: a position differs when the line's byte is not the probe's byte.  'N', a lower-case letter, '.' and
 * a byte with the high bit set are each one mismatch; they are no match merely because they share a 2-bit code with a base.
 * ham(a, b): the number of positions at which two byte strings of the same length differ.
 * Everything else is the adapter content's: the record set, and L as the bases line without a trailing '\r'.
 * FIRST_k: the smallest p with p + m_k <= L and ham(line[p, p + m_k), probe_k) <= E(m_k) -- the smallest p, not the p with the
 * fewest mismatches.  The window lies inside the line: the bytes behind L (the '\r', the newline, whatever a kernel loads behind
 * them) are mismatches like any other, and without the bound p + m_k <= L a window that hangs over the end by E bases would be
 * accepted.  DIST_k: the number of differing positions of that window, 0 .. 3.
 * TAIL_k: considered only when there is no FIRST_k under this same rule: the largest t with T <= t <= min(m_k - 1, L) and
 * ham(line[L - t, L), probe_k[0, t)) <= E(t) -- E of t, not of m_k; the largest t wins even where a smaller t matches exactly.
 * CLIP, MASK and the words of both arrays are as they are, with these additions, written only when per > 0 (with per == 0 they
 * stay 0 and both arrays are the exact rule's, bit for bit):
 *   adapters array [4] = per;   its blocks' words +4 .. +7 = the records with FIRST_k whose DIST_k is 0, 1, 2, 3 (they sum to +1);
 *   clip array [5] = per.
 * WHAT A LOOSER RULE COSTS: on uniformly random bases one 12-base probe matches a 150-base read somewhere with probability about
 * 6.7e-4 at per = 10 against 3.3e-4 exact (the tails of 6 .. 9 bases, which stay exact, are half of it).  Measured on the CPU,
 * 20 000 random reads against four 12-base probes: a clipped share of 0.14 % exact and 0.32 % at per = 10 (beside T's 0.03 % a
 * probe above).
 * kvq_scan_set_adapter_mismatches: one value per scan, for the adapter content and the clip alike; before the first batch or
 * after kvq_scan_reset, as kvq_scan_set_cycles; in any order against kvq_scan_set_adapters and kvq_scan_set_clip (it needs
 * neither, and stays while they go on and off); KVQ_ERR_RUNTIME outside {0} and [10, 32].  kvq_scan_adapter_mismatches: the
 * value.  With per > 0 the passes launch kvq_adapt_records_mm / kvq_clip_records_mm (the tolerant instantiations) in place of the exact
 * kernels, and kvq_scan_adapt_kernel_ms / kvq_scan_clip_kernel_ms report whichever ran. */
enum { KVQ_ADAPT_PER = 4, KVQ_ADAPT_B_DIST = 4, KVQ_ADAPT_DISTS = 4, KVQ_CLIP_PER = 5, KVQ_ADAPT_MIN_PER = 10, KVQ_ADAPT_MAX_PER = 32 };
int32_t        kvq_scan_set_adapter_mismatches(kvq_scan *s, int32_t per);
int32_t        kvq_scan_adapter_mismatches(const kvq_scan *s);
/* host only, plain C++: the CPU twins of kvq_adapt_records_mm and kvq_clip_records_mm -- the argument lists of kvq_adapt_host and
 * kvq_clip_host plus per (outside {0} and [10, 32]: KVQ_ERR_RUNTIME).  With per == 0 they give the results of those two. */
int32_t        kvq_adapt_host_mm(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                 const uint8_t *const *probes, const int32_t *lens, int32_t n, int32_t per, int64_t *out);
int32_t        kvq_clip_host_mm(uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                                const uint8_t *const *probes, const int32_t *lens, int32_t n, int32_t per, int64_t *out);

/* ---- the reads the scan saw, as FastQ text: EVERY RECORD CUT TO WHAT THE TRIM LEAVES OF IT ----
 * EMIT(text, chunk_off, amin, min_length): the record set is the profile's (every complete four-newline record of every chunk,
 * newlines at n0 < n1 < n2 < n3); r0 is the record's first byte: the byte behind the n3 of the record in front of it, or the
 * chunk's first byte.  Per record, in stream order:
 *   name = text[r0, n0) less one trailing '\r';  bases = text[n0 + 1, n1);  scores = text[n2 + 1, n3) -- both raw.
 *   len(bases) != len(scores): the record is MISMATCHED, dropped and counted.
 *   else (start, length) is the scan's trim of the score line (workhorse.c:1055-1068: the longest run of bytes >= amin compared as
 *   signed chars, the line's newline fed too, the first of equal runs), over the whole line, however long.
 *   length < min_length: the record is SHORT, dropped and counted.
 *   else it is EMITTED as  name '\n' bases[start, start + length) "\n+\n" scores[start, start + length) '\n'  -- the third line is
 *   always a bare '+'.  min_length == 0 keeps every well-formed record (with empty lines where nothing survives): the files of
 *   two mates stay in step record for record.
 * An emitted record is at most its input record plus one byte: a batch of nbytes bytes and nrec records emits at most
 * nbytes + nrec bytes, and there is no overflow.
 * THE RESULT: the emitted text, and one flat int64 array of kvq_emit_len() = 8 words, every word but [0] a sum over the records:
 *   [0] n = the min_length in effect    [1] records    [2] emitted    [3] short    [4] mismatched
 *   [5] sum of len(bases) over all records    [6] sum of length over the emitted records    [7] bytes of emitted text
 *   [1] == [2] + [3] + [4];  [7] == the length of the text;  [1] == the profile's records when a profile is on.
 * THE CONTRACT WITH THE CLIP: the emit of `text` with the clip on is the emit of MASK(text) without it (the emit runs behind the
 * clip and behind the scan, on the batch's first pass only); the emitted scores never hold a byte of the mask: they are a run of
 * bytes >= Amin, and the clip refuses an Amin that is not above '!'.
 * The emit does not repeat the scan's '@' / '+' checks: a call that ends in KVQ_ERR_FORMAT ends so as before, and what it has
 * emitted until then is unspecified.
 * kvq_scan_set_emit: on != 0 turns the emit on with min_length (< 0: the table's minreadlength), on == 0 turns it off; before
 * the first batch or after kvq_scan_reset, as kvq_scan_set_cycles.  It needs no profile and is allowed beside every other option;
 * with a communicator it is KVQ_ERR_RUNTIME, as the records are.  amin is the table's Amin.  Off, nothing is enqueued or allocated.
 * THE SINK: a host buffer that grows -- kvq_scan_emitted hands out its bytes (valid after kvq_scan_finish until the next reset;
 * KVQ_ERR_RUNTIME before) -- or, after kvq_scan_set_emit_fd(s, fd) with fd >= 0, that file descriptor, which stays the caller's
 * (fd < 0: the host buffer again; the call needs the emit on).  The sink and the words are cleared wherever the hit arena is --
 * a regular file is truncated to zero and sought to its start; a pipe cannot take anything back --, so a batch that runs again after an arena overflow (a device batch
 * replayed inside kvq_scan_finish, host batches fed again, kvq_findseqs reading its files again) is emitted once.  A batch
 * whose speculation failed is emitted by its first pass alone.  Every batch waits on the host once for its byte count.
 * kvq_scan_emit: the words (valid after kvq_scan_finish until the next reset), NULL when the option is off.
 * kvq_scan_emit_guard (measurement): the store of every batch lies between two blocks of 64 guard bytes, the one behind it
 * right behind the batch's last emitted byte; the number of guard bytes found changed since the last reset (-1: the emit is off). */
enum { KVQ_EMIT_N = 0, KVQ_EMIT_RECORDS = 1, KVQ_EMIT_EMITTED = 2, KVQ_EMIT_SHORT = 3, KVQ_EMIT_MISMATCHED = 4, KVQ_EMIT_BASES_IN = 5,
       KVQ_EMIT_BASES_OUT = 6, KVQ_EMIT_BYTES_OUT = 7, KVQ_EMIT_WORDS = 8 };
int64_t        kvq_emit_len(void);
int32_t        kvq_scan_set_emit(kvq_scan *s, int32_t on, int32_t min_length);
int32_t        kvq_scan_set_emit_fd(kvq_scan *s, int32_t fd);
int32_t        kvq_scan_emitted(const kvq_scan *s, const uint8_t **text, int64_t *nbytes);
const int64_t *kvq_scan_emit(const kvq_scan *s);
int64_t        kvq_scan_emit_guard(const kvq_scan *s);
double         kvq_scan_emit_kernel_ms(const kvq_scan *s);   /* GPU time of kvq_emit_size, the prefix sum and kvq_emit_copy (0 when the emit is off) */
/* host only, plain C++: the CPU twin of the emit over the same definition -- test infrastructure and the definition in running
 * code, not a fallback.  Arguments as for kvq_profile_host; amin a byte compared as a signed char, min_length >= 0.  Writes the
 * emitted text to out_text[0, out_cap) and returns its length, or -1 (bad arguments; out_cap too small for what the text emits:
 * nbytes + the number of records always holds it).  ADDS into out_words[0, kvq_emit_len()), but for [0], which it sets. */
int64_t        kvq_emit_host(const uint8_t *text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks, int32_t amin, int32_t min_length,
                             uint8_t *out_text, int64_t out_cap, int64_t *out_words);

/* ---- the emitted reads, deflated to BGZF on the device: THE OUTPUT IS A FUNCTION OF THE TEXT ALONE ----
 * BGZF(text), for the emitted text of one batch: the text is cut into blocks of 65 280 bytes (bgzip's 0xff00), the last one
 * shorter; an empty text gives no member.  Each block is one BGZF member: the 18-byte header with the 'BC' subfield and BSIZE,
 * one raw DEFLATE stream of one final block, the CRC-32 of the block's bytes, ISIZE.  The stream is a dynamic-Huffman block
 * (BTYPE 2) over the LZ77 parse below, or, where that is no shorter, a stored block (BTYPE 0: 65 280 + 5 + 26 bytes at most,
 * inside the 65 536 a member may have).  There is no fixed-Huffman block.
 * THE PARSE (kvq_deflate.h states it in running code, for the twin and the kernel alike): a block is cut into 256 segments of 255
 * bytes.  A segment is parsed greedily from its first byte and needs nothing of the parse of another.  Every segment has a table
 * of 128 slots that maps the hash of three bytes to the last position of the segment that has it, every position entered; the
 * parse of segment s keeps its own table for the positions in front of the current one and looks into the FINAL tables of
 * segments s - 1 and s - 2.  A candidate's match is the common prefix of the raw block at both places, cut at the segment's end:
 * length 3 .. 255, distance 1 .. 762 (a match begins at 252 of its segment at the latest, against the first byte of segment s - 2); the longest wins, the nearest table among equals; below three bytes the byte is a literal.
 * THE CODES: Huffman lengths limited to 15 (7 for the code-length code) by kvq_deflate_lengths, canonical codes, the header's
 * lengths run-length coded by one greedy rule; a block without a match states one distance code of one bit.
 * Launch geometry, timing and the order of atomics change nothing: the GPU's bytes are the twin's bytes.
 * THE WORDS, kvq_deflate_len() = 8 of them, all sums over the members but the two maxima:
 *   [0] members   [1] bytes in   [2] bytes out (without the EOF member)   [3] members that fell back to stored
 *   [4] match tokens   [5] literal tokens   [6] the longest distance   [7] the longest match -- of the members that are not stored
 * kvq_scan_set_emit_compress(s, on): the emitted text of every batch reaches the sink as BGZF(text); it needs the emit on and
 * the scan idle, and takes the refusals kvq_scan_set_emit_fd takes.  When the scan finishes the sink gets the 28-byte EOF member
 * (kvq_bgzf_eof), once: a scan that emitted nothing yields the EOF member alone, a valid empty gzip.  The words and the EOF
 * flag are cleared where the sink is, so a replay after an arena overflow still leaves one stream with one EOF member.  The
 * uncompressed text never leaves the device; the eight emit words, the guards and every result are what they are without it;
 * [1] equals the emit's word [7].  Every batch waits on the host once more, for its compressed byte count.  Off (the default),
 * nothing is enqueued, allocated or changed.  kvq_scan_emitted then hands out the compressed bytes.
 * kvq_scan_emit_compress: the words (valid after kvq_scan_finish until the next reset), NULL when the option is off.
 * kvq_deflate_bgzf_device: BGZF(d_text[0, nbytes)) into d_out[0, out_cap), both device memory; returns its length or -1 (bad
 * arguments, a device error, out_cap below the length: no byte at or behind out_cap is then written); kvq_deflate_bound(nbytes)
 * always holds it.  No byte behind the length is written.  Sets out_words.  Blocking.
 * kvq_deflate_bgzf_host: the CPU twin over the same definition, test infrastructure and not a fallback; same arguments in host memory.
 * kvq_deflate_lengths_host: the length-limited code builder on its own: lens[0, nsym) for freq[0, nsym), nsym <= 288, limit 1 .. 15;
 * more used symbols than 2^limit, counts that sum to 2^32 or more (the tree's weights are 32-bit), and anything else out of range:
 * KVQ_ERR_RUNTIME.
 * Environment, read at every deflate (for tests): KVQ_DEFLATE_ROUND=<members> lets fewer than 2048 members go through their
 * slots at a time, so that a small text takes several rounds; the output does not depend on it. */
enum { KVQ_DEFLATE_MEMBERS = 0, KVQ_DEFLATE_BYTES_IN = 1, KVQ_DEFLATE_BYTES_OUT = 2, KVQ_DEFLATE_STORED = 3, KVQ_DEFLATE_MATCHES = 4,
       KVQ_DEFLATE_LITERALS = 5, KVQ_DEFLATE_MAX_DISTANCE = 6, KVQ_DEFLATE_MAX_LENGTH = 7, KVQ_DEFLATE_WORDS = 8 };
int64_t        kvq_deflate_len(void);
int64_t        kvq_deflate_bound(int64_t nbytes);
const uint8_t *kvq_bgzf_eof(void);                           /* the 28 bytes */
int32_t        kvq_scan_set_emit_compress(kvq_scan *s, int32_t on);
const int64_t *kvq_scan_emit_compress(const kvq_scan *s);
double         kvq_scan_emit_deflate_kernel_ms(const kvq_scan *s);   /* GPU time of the deflate's kernels (0 when the option is off) */
int64_t        kvq_deflate_bgzf_device(const void *d_text, int64_t nbytes, void *d_out, int64_t out_cap, int64_t *out_words);
int64_t        kvq_deflate_bgzf_host(const uint8_t *text, int64_t nbytes, uint8_t *out, int64_t out_cap, int64_t *out_words);
int32_t        kvq_deflate_lengths_host(const uint32_t *freq, int32_t nsym, int32_t limit, uint8_t *lens);

/* GPU time of all scan kernels enqueued so far on this scan's stream, from HIP
 * events around the launches (valid after kvq_scan_finish); and the same for
 * the dominant (read-scanning) kernel alone plus its launch count */
double  kvq_scan_kernel_ms(const kvq_scan *s);
double  kvq_scan_main_kernel_ms(const kvq_scan *s);
double  kvq_scan_profile_kernel_ms(const kvq_scan *s);   /* ... and for kvq_profile_records alone (0 when the profile is off) */
double  kvq_scan_cycles_kernel_ms(const kvq_scan *s);    /* ... and for kvq_profile_cycles alone (0 when the cycles are off) */
double  kvq_scan_reads_kernel_ms(const kvq_scan *s);     /* ... and for kvq_reads_records and the table's settle kernels (0 when both are off) */
double  kvq_scan_over_kernel_ms(const kvq_scan *s);      /* ... and for kvq_over_records alone (0 when the overrepresented sequences are off) */
double  kvq_scan_adapt_kernel_ms(const kvq_scan *s);     /* ... and for kvq_adapt_records or kvq_adapt_records_mm alone, whichever ran (0 when the adapters are off) */
double  kvq_scan_clip_kernel_ms(const kvq_scan *s);      /* ... and for kvq_clip_records or kvq_clip_records_mm alone (0 when the clip is off) */
/* (measurement) ms between the end of a's last main kernel and the start of b's first one; both finished, not reset since */
double  kvq_scan_gap_ms(const kvq_scan *a, const kvq_scan *b);
/* (measurement) how kvq_scan_finish put the hits of the finished scan in order:
 *   out[0] n       hits put in order            out[5] crowded  a bucket held more than 64 hits
 *   out[1] nb      buckets of the ordering      out[6] 1 when the merge sort produced the result (a crowded
 *   out[2] shift   bucket = (file_pos - lo) >> shift            bucket, or KVQ_ORDER=mergesort), 0: the bucket ordering
 *   out[3] bc      buckets per ordering workgroup (512 contiguous shares)
 *   out[4] lo      smallest fpos_base of the scan's batches
 *   out[7], out[8] hits the arena and bytes the hit blob hold NOW (grown by an overflow; valid at any time).
 * out[0..6] are zero until the scan is finished.  The tests assert with it that an input reached the seam it was built for.
 * Environment, read when a scan object is created: KVQ_ARENA_CAP=<hits> and KVQ_BLOB_CAP=<bytes> shrink the first
 * arena (2^20 hits) and hit blob (64 MiB), to no less than 64 hits / 256 bytes; growth after an overflow is unchanged.
 * Read at every finish: KVQ_ORDER=mergesort orders every scan with the comparison sort. */
void    kvq_scan_order_info(const kvq_scan *s, int64_t out[9]);
/* (measurement) which matchers the last seed-filter launch of the finished scan handed its work to:
 *   out[0] slots of the survivors' list handed out (kvq_verify_survivors counts their bytes; the slots come sixteen at a
 *          time, so this is no count of work items, and it passes out[1] when the list ran full)
 *   out[1] slots the list has (2^22, or what KVQ_SURV_CAP=<slots>, read when the scan object is created, cut it to;
 *          0: every work item is verified where it was found, bp_verify_rest); valid at any time
 *   out[2] records the launch's skipped tiles left on the redo's list (kvq_match_all)
 *   out[3] the reads of 1024 bases and more among them, on a list of their own (kvq_match_long)
 * out[0], out[2], out[3] are zero until the scan is finished and when it had no seed-filter launch.  The words are read
 * from the device when this is called; a scan that does not call it does nothing for it.  Returns 0 or an error code. */
int32_t kvq_scan_match_info(const kvq_scan *s, int64_t out[4]);
/* (measurement) what the host decided for the seed-filter launches of this scan object since kvq_scan_create / kvq_scan_reset
 * (a replay of device batches after a hit-arena overflow launches again and is counted again):
 *   out[0] launches   seed-filter launches (a batch without a tile launches nothing and is not counted)
 *   out[1] pipelined  ... that found the scan kernel in front of them, another scan object's, still on the device
 *   out[2] beside     ... that published the chain AHEAD of their kvq_verify_survivors: the next scan of the process runs
 *                     beside this one's survivors, validation, redo, fold, record gathering, input passes and finish tail.
 *                     Equal to out[1] unless KVQ_SV_MODE is set (read once per process: 0 never beside, 1 always)
 * and of the last of them:
 *   out[3], out[4]    workgroups and threads of its kvq_verify_survivors: 256 x 1024 behind the scan, KVQ_SV_GRID (read once
 *                     per process; 64) x 256 beside the next; a round of that kernel covers out[3] * out[4] slots of the list
 *                     (both 0: the scan object has no list)
 *   out[5] grid cap   the most workgroups its scan kernel might take (kvq_scan_grid: what it took)
 *   out[6] ... and which: 1 every slot (four a CU), 2 one slot in four CUs left free (another scan object's kernel was on the
 *                     device), 3 KVQ_GRID
 *   out[7] CUs of the device      out[8] scan objects alive in the process at that moment
 *   out[9] 1 when the last launch went beside
 * All zero while there was no such launch.  Host-side facts only: it does no device work, and it steers nothing.  The tests
 * assert with it that a scan took the order and the grid it was built for before they compare its result. */
void    kvq_scan_launch_info(const kvq_scan *s, int64_t out[10]);
/* (measurement) the exact record index of one batch in device memory, as every scan makes it for the exhaustive kernels, the
 * read-list route, the clip and the input passes -- the same checks, chunk table and kernels, on the scan's stream --, brought to
 * the host: chunk_nrec_out[c] the complete records of chunk c (nchunks words), and of the first min(R, cap) records
 * nl4_out[4 g + k] the batch offset of record g's k-th newline and rec_start_out[g] that of its first byte (the chunk's begin
 * for a chunk's first record, else one behind the newline that ends the record in front).  The bytes are arbitrary: a record
 * is four newlines.  d_text as for kvq_scan_device (16-byte aligned, readable up to the next multiple of 16 behind nbytes).
 * Allowed only on a scan that holds no batch (before the first, or after kvq_scan_reset); it leaves no batch, hit or counter
 * behind.  Returns R, the records of the batch, or -1 on an error (kvq_last_error).  The tests pin the index with it. */
int64_t kvq_scan_index_device(kvq_scan *s, const void *d_text, int64_t nbytes, const int64_t *chunk_off, int64_t nchunks,
                              uint32_t *nl4_out, uint32_t *rec_start_out, int64_t cap, uint32_t *chunk_nrec_out);
/* (measurement) what the last seed-filter launch of a finished scan of ONE batch left to the redo of its skipped tiles.
 * kvq_scan_set_keep_skipped(s, 1), before the first batch or after kvq_scan_reset, makes the scan keep host copies of both lists
 * at the one place where it reads a batch's fail word; off (the default), nothing is copied and both calls below are errors.
 * kvq_scan_skipped_tiles: the descriptors in the order kvq_validate_tiles wrote them, six words each -- a, b (the chunk, or from
 * z - 1 on when the tile scanned the records in front of a record at z - 1), own_begin, own_end (the bytes whose newlines the tile
 * owns), seen (newlines of [a, own_begin)), first (the record at `a` is the tile's too).  kvq_scan_redo_list: the entries
 * kvq_collect_skipped put on the redo's list for them, nl4 and rec_start as in kvq_scan_index_device, in the order the atomics
 * gave; the reads the scan kernel put there itself, already trimmed, are left out.  Both copy min(n, cap) entries and return n,
 * or -1 on an error. */
int32_t kvq_scan_set_keep_skipped(kvq_scan *s, int32_t on);
int64_t kvq_scan_skipped_tiles(const kvq_scan *s, uint32_t *out, int64_t cap);
int64_t kvq_scan_redo_list(const kvq_scan *s, uint32_t *nl4_out, uint32_t *rec_start_out, int64_t cap);
int64_t kvq_scan_main_kernel_launches(const kvq_scan *s);
/* forget accumulated hits/counters/timers but keep buffers (bench steps) */
int32_t kvq_scan_reset(kvq_scan *s);
/* which kernels produced the result: bit 0 = the seed-filter kernel ran, bit 1 = the
 * exhaustive kernels ran, bit 2 = the seed-filter pass of a batch was discarded (its speculated
 * record split failed validation, one read flooded a wave's queues) and the batch rescanned,
 * bit 3 = tiles of the seed-filter pass left their records alone (a record longer than a tile's
 * look-ahead, more newlines than its tables hold) and those records were scanned again, bit 4 = the text was inflated
 * on the device (kvq_findseqs_ex, KVQ_FIND_DEVICE_INFLATE or KVQ_FIND_DEVICE_GZIP), bit 5 = a file of it took the speculative
 * route of KVQ_FIND_DEVICE_GZIP, bit 6 = the text was decoded from BAM on the device (kvq_findseqs on BAM files),
 * bit 7 = a batch took the read-list route (kvq_scan_set_long_reads): it sets bit 1 only when the exhaustive matcher ran for sequences
 * without seeds, and never bit 0 */
int32_t kvq_scan_path(const kvq_scan *s);
/* 0 = let the table decide, 1 = force the exhaustive kernel for every sequence */
void    kvq_scan_force_exhaustive(kvq_scan *s, int32_t on);

/* which instantiation of the seed-filter scan kernel served a batch (a "cell"): bits 0-3 the seed length K (5..8),
 * bits 4-7 the stride of the seed index (2, 4, 8), bits 8-11 the lane group + 1 (0: worked out per tile, else 2, 3,
 * 4 for lane groups 1, 2, 3 -- two, four, eight lanes a read), then the flags below.  kvq_scan_kernel_pick is the
 * launcher's own choice, a host function of its inputs: the table's seed length, stride and density (its seed index
 * expects more candidates per read than a wave's queue holds), the average record and the tile the head of the text
 * gave (kvq_tile_for_text), and the KVQ_DBG bits; -1 when no kernel exists for them.  kvq_scan_kernel: the cell of
 * the scan's last seed-filter launch since kvq_scan_create / kvq_scan_reset, 0 = none.  kvq_scan_grid: the workgroups
 * of that launch (the tiles of the batch, at most what the device holds at once or what the KVQ_GRID switch allows), 0 = none. */
#define KVQ_CELL_DENSE  0x1000           /* the draining kernels (always for K < 8) */
#define KVQ_CELL_DIAG   0x2000           /* the instantiations that honour the KVQ_DBG switches (K < 8 and draining kernels too) */
#define KVQ_CELL_STAMPS 0x4000           /* the instrumented build (KVQ_DBG bit 16) */
int32_t kvq_scan_kernel_pick(int32_t k, int32_t stride, int32_t dense, uint32_t rec_bytes, uint32_t tile_bytes, uint32_t dbg);
int32_t kvq_scan_kernel(const kvq_scan *s);
int32_t kvq_scan_grid(const kvq_scan *s);
/* host only: the tile (bytes a workgroup owns) of the seed-filter scan for a text whose first n bytes are given (the
 * library looks at the first 128 KiB of a scan's first batch); *rec_bytes_out, where not NULL, gets the average
 * record among them (0 = fewer than 16 lines) */
uint32_t kvq_tile_for_text(const uint8_t *text, size_t n, uint32_t *rec_bytes_out);

/* ---- several GPUs, one process each ----------------------------------------------------------
 * The reference starts nthreads workers on one file and joins them into one result
 * (workhorse.c:1375-1447: pthread_create / pthread_join, counters under mutexes, one hit list).
 * Here every process scans its own stretch of the reads on its own GPU -- no exchange on the data
 * path -- and the join is a collective over RCCL (librccl.so, loaded on first use):
 *   kvq_comm_unique_id   rank 0 makes the 128-byte id of a communicator, the caller hands it to the
 *                        other ranks (any way it likes: a file, MPI, torch.distributed ...)
 *   kvq_comm_create      every rank, collectively, with its number and the id; after kvq_set_device
 *   kvq_scan_set_comm    kvq_scan_finish then is collective.  Behind the rank's own finish the ranks
 *                        agree on how they ended (a maximum over one status word); when all are fine the
 *                        counter arrays of all ranks are summed (one all-reduce on the scan's stream; the
 *                        slot of the longest read takes the maximum) into kvq_scan_counters and
 *                        kvq_scan_device_counters -- the rank's own counters are kept, a second finish
 *                        sums them afresh.  When ANY rank returns KVQ_ERR_RESCAN (hit arena overflow on
 *                        host batches) EVERY rank does, with no sum taken: all ranks reset, feed their
 *                        batches again and finish again, so their collectives stay in step.  Any other
 *                        failure of one rank is an error on all of them.
 *   kvq_comm_create_local  instead of kvq_comm_create: the ranks are threads of ONE process (each with a
 *                        scan of its own, on whatever device it has set) that exchange through host
 *                        memory -- no RCCL; `world_key` is any number the ranks of one communicator
 *                        share.  For hosts without RCCL and for testing the join on a single GPU.
 *   kvq_scan_gather_hits after kvq_scan_finish, collective: the hits of all ranks, in rank order --
 *                        ranks scan consecutive stretches of the stream, so that is the reference's
 *                        order -- replace the rank's own behind kvq_scan_n_hits / kvq_scan_hit_* /
 *                        kvq_scan_hitseq_*: a count exchange (all-gather), then one broadcast per
 *                        rank and array into its place
 *   kvq_comm_allreduce_counters  the same sum for a counter array the caller keeps itself
 *                        (d_scratch16: 16 bytes of device memory) */
typedef struct kvq_comm kvq_comm;
int32_t   kvq_comm_unique_id(void *id128);
kvq_comm *kvq_comm_create(int32_t nranks, int32_t rank, const void *id128);
void      kvq_comm_destroy(kvq_comm *c);
int32_t   kvq_comm_nranks(const kvq_comm *c);
int32_t   kvq_comm_rank(const kvq_comm *c);
int32_t   kvq_scan_set_comm(kvq_scan *s, kvq_comm *c);
int32_t   kvq_scan_gather_hits(kvq_scan *s, kvq_comm *c);
int32_t   kvq_comm_allreduce_counters(kvq_comm *c, void *d_counters, int64_t ctr_len, void *d_scratch16);
kvq_comm *kvq_comm_create_local(int32_t nranks, int32_t rank, uint64_t world_key);
/* where kvq_scan_gather_hits puts the ranks' arrays -- a host function of the counts alone (counts[2r] hits,
 * counts[2r+1] hit bytes of rank r).  parts: 7 x {offset in the rank's own result buffer, offset in the gathered
 * one, bytes} per rank, in the order file_pos, hitseq offsets, seq_nr, seq_pos, length, readlength, hit bytes;
 * blob_base[r]: added to rank r's hitseq offsets; totals: {hits, hit bytes, bytes of the gathered buffer, offset
 * of its hitseq-offset array}.  kvq_gather_host carries the plan out in host memory; kvq_result_layout_words:
 * the offsets of those seven arrays in a result buffer of n hits and blob_bytes hit bytes, then its size. */
int32_t   kvq_gather_plan(int32_t nranks, const uint64_t *counts, uint64_t *parts, uint64_t *blob_base, uint64_t *totals);
int32_t   kvq_gather_host(int32_t nranks, const uint64_t *counts, const uint8_t *const *rank_bufs, uint8_t *out);
void      kvq_result_layout_words(uint64_t n, uint64_t blob_bytes, uint64_t *out8);

/* ---- engine.findseqs (workhorse.c:1249-1464) -------------------------------
 * files: plain or ".gz" (by suffix, workhorse.c:582), scanned as one stream
 * with cumulative file_pos.  Blocking; uses the global config.  Returns a scan
 * object holding the results (never NULL unless out of memory); check
 * kvq_last_error() -- on error the scan object still has to be destroyed. */
kvq_scan *kvq_findseqs(const char *const *files, int32_t nfiles,
                       const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq);

/* the same with options.  KVQ_FIND_DEVICE_INFLATE: when EVERY file is BGZF (bgzip) to its end (at most 10 trailing
 * bytes), the compressed blocks are copied to the GPU, inflated there (kvq_inflate_bgzf_device), cut into the
 * reference's chunks there and scanned where they lie; otherwise the call is kvq_findseqs.  Results, stats() and
 * messages are kvq_findseqs's, but for one: a block that does not inflate fails with KVQ_ERR_IO "error while
 * inflating compressed data : status=<zlib status> fpos=<stream offset of that BLOCK's first inflated byte>".
 * kvq_scan_path bit 4 tells that the text was inflated on the device. */
#define KVQ_FIND_DEVICE_INFLATE 1u
/* KVQ_FIND_DEVICE_GZIP: when EVERY file is a ".gz", each is inflated on the GPU: a BGZF file as above, any other gzip by
 * speculative chunk decoding (kvq_inflate_gzip_device); otherwise the call is kvq_findseqs.  Results,
 * stats() after the call and messages are kvq_findseqs's, but for the fpos of "error while inflating compressed data":
 * for a plain gzip file the stream offset at which the failing DEFLATE block's output starts.  kvq_scan_path bit 5 tells
 * that a file took the speculative route; kvq_gzip_last_report what it did. */
#define KVQ_FIND_DEVICE_GZIP 2u
/* KVQ_FIND_RECORDS: the scan keeps the record of every hit (kvq_scan_set_records; the accessors below).  It ORs with the two
 * inflate flags; alone it is the host route with records. */
#define KVQ_FIND_RECORDS 4u
kvq_scan *kvq_findseqs_ex(const char *const *files, int32_t nfiles,
                          const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, uint32_t flags);

/* the same with the options as a structure (size: sizeof(kvq_find_opts), for later growth; flags: the KVQ_FIND_* above).
 * KVQ_FIND_PROFILE: the scan profiles its input at cutoffs[0, n_cutoffs) (kvq_scan_set_profile; kvq_scan_profile after the
 * call).  An empty sequence list is legal and gives a profile-only call.  opts == NULL: kvq_findseqs.
 * KVQ_FIND_CYCLES: the per-cycle counts too (kvq_scan_set_cycles; kvq_scan_cycles after the call); without KVQ_FIND_PROFILE it is
 * KVQ_ERR_RUNTIME. */
#define KVQ_FIND_PROFILE 8u
#define KVQ_FIND_CYCLES 16u
/* KVQ_FIND_LONG_READS / KVQ_FIND_LONG_READS_AUTO: kvq_scan_set_long_reads mode 1 / 2 for the call, whatever way the text
 * takes to the GPU (host reader, device inflate, BAM). */
#define KVQ_FIND_LONG_READS 32u
#define KVQ_FIND_LONG_READS_AUTO 64u
/* KVQ_FIND_READ_STATS / KVQ_FIND_DUPLICATION: kvq_scan_set_read_stats bit 0 / bit 1 for the call (kvq_scan_reads / kvq_scan_dup
 * after it); without KVQ_FIND_PROFILE they are KVQ_ERR_RUNTIME. */
#define KVQ_FIND_READ_STATS 128u
#define KVQ_FIND_DUPLICATION 256u
/* KVQ_FIND_OVERREPRESENTED: kvq_scan_set_overrepresented for the call (kvq_scan_over after it); without KVQ_FIND_PROFILE it is
 * KVQ_ERR_RUNTIME. */
#define KVQ_FIND_OVERREPRESENTED 512u
typedef struct kvq_find_opts {
    uint32_t size, flags;
    int32_t  n_cutoffs;
    uint8_t  cutoffs[8];
} kvq_find_opts;
/* KVQ_FIND_ADAPTERS: kvq_scan_set_adapters for the call (kvq_scan_adapters after it); without KVQ_FIND_PROFILE it is
 * KVQ_ERR_RUNTIME.  kvq_find_opts keeps its 20 bytes: the probes ride in a longer structure that begins with it, which the
 * library reads only when the flag is set and base.size covers it -- anything else is "bad size". */
#define KVQ_FIND_ADAPTERS 1024u
typedef struct kvq_find_opts_adapters {
    kvq_find_opts base;                  /* base.size: sizeof(kvq_find_opts_adapters) */
    int32_t  n_probes;
    uint8_t  lens[8];
    uint8_t  probes[8][32];
} kvq_find_opts_adapters;
/* KVQ_FIND_CLIP: kvq_scan_set_clip for the call (kvq_scan_clip after it), with the probes of kvq_find_opts_adapters -- the one
 * probe block there is: with KVQ_FIND_ADAPTERS too, both take the same probes.  Refused ("bad size") when base.size does not
 * cover that structure.  It is not tied to KVQ_FIND_PROFILE. */
#define KVQ_FIND_CLIP 2048u
/* KVQ_FIND_ADAPTER_MISMATCHES: kvq_scan_set_adapter_mismatches(mismatch_per) for the call.  The value rides behind the probes in
 * a structure that begins with kvq_find_opts_adapters, read only with the flag and only when base.size covers it -- otherwise
 * "bad size"; the 20-byte and the 288-byte structures keep their meaning.  The flag without KVQ_FIND_ADAPTERS or KVQ_FIND_CLIP is
 * KVQ_ERR_RUNTIME. */
#define KVQ_FIND_ADAPTER_MISMATCHES 4096u
typedef struct kvq_find_opts_adapters_mm {
    kvq_find_opts_adapters a;            /* a.base.size: sizeof(kvq_find_opts_adapters_mm) */
    int32_t  mismatch_per;
} kvq_find_opts_adapters_mm;
/* KVQ_FIND_EMIT: kvq_scan_set_emit(1, min_length) for the call, the sink the file `path`, which the call creates or truncates:
 * every file of the call goes to the one output, in order (kvq_scan_emit after the call).  min_length and path ride behind the
 * mismatch rate in a structure that begins with kvq_find_opts_adapters_mm, read only with the flag and only when base.size covers
 * it -- otherwise "bad size"; the bytes in front stay what they are, and the blocks in front are read only under their own flags
 * (a caller without probes leaves them zero).  min_length < 0: the configured minreadlength.  It is tied to no other flag. */
#define KVQ_FIND_EMIT 8192u
typedef struct kvq_find_opts_emit {
    kvq_find_opts_adapters_mm m;         /* m.a.base.size: sizeof(kvq_find_opts_emit) */
    int32_t  min_length;
    const char *path;
} kvq_find_opts_emit;
/* KVQ_FIND_EMIT_BGZF: kvq_scan_set_emit_compress(1) for the call: the file is BGZF, its EOF member written
 * before the descriptor is closed.  It is read only with KVQ_FIND_EMIT, and without it the call is KVQ_ERR_RUNTIME.  It needs
 * no structure of its own. */
#define KVQ_FIND_EMIT_BGZF 16384u
kvq_scan *kvq_findseqs_opts(const char *const *files, int32_t nfiles,
                            const uint8_t *const *seqs, const int32_t *seqlens, int32_t nseq, const kvq_find_opts *opts);

/* destroys a scan returned by kvq_findseqs together with the table it built */
void kvq_findseqs_free(kvq_scan *s);

/* host-only (no GPU): the chunks the reader cuts from the files, exactly the
 * buffers fastq_read (workhorse.c:737-956) would hand to the scanning threads,
 * as (offset in the inflated stream, length) pairs; returns the number of
 * chunks or -1 (kvq_last_error).  batch_bytes <= 0 selects the default. */
int64_t kvq_host_chunk_plan(const char *const *files, int32_t nfiles, int64_t *chunk_fpos, int64_t *chunk_len,
                            int64_t cap, int64_t *parsed, int64_t *total, int64_t batch_bytes);

/* ---- engine.stats / engine.stop (workhorse.c:1205-1244, 1469-1479) ---------- */
typedef struct kvq_live_stats {
    int64_t records_parsed;
    int64_t parsed;            /* fastq_parsed         */
    int64_t total;             /* fastq_size_estimated */
    int64_t rls_longest;       /* -1 if none */
    int32_t nseq;
    int32_t running;
    int32_t sigints;
    int32_t stop_requested;
} kvq_live_stats;

/* snapshot of the running (or last) findseqs; readlengths/nseqhits/nseqbasehits
 * may be NULL; nseq_cap bounds the two per-sequence arrays */
void kvq_poll_stats(kvq_live_stats *out, int64_t *readlengths /*[1024]*/,
                    int64_t *nseqhits, int64_t *nseqbasehits, int32_t nseq_cap);
void kvq_request_stop(void);
void kvq_count_sigint(void);    /* sigint_cb, workhorse.c:133-136 */
/* signal(SIGINT, sigint_cb) of the module init (workhorse.c:1632) as an explicit, reversible call: a C handler
 * that only counts, so that SIGINTs are counted while the calling thread is inside kvq_findseqs */
int  kvq_sigint_counter_install(void);
void kvq_sigint_counter_remove(void);

/* ---- device + synthetic workload (bench / tests plumbing) -------------------- */
int32_t kvq_device_count(void);
int32_t kvq_set_device(int32_t ordinal);
void   *kvq_device_alloc(int64_t nbytes);               /* 256-byte aligned, NULL on failure */
void    kvq_device_free(void *p);
int32_t kvq_memcpy_h2d(void *d, const void *h, int64_t nbytes);
int32_t kvq_memcpy_d2h(void *h, const void *d, int64_t nbytes);
int32_t kvq_memset_d(void *d, int32_t value, int64_t nbytes);
int32_t kvq_device_synchronize(void);
/* Device and pinned blocks of destroyed scans and tables are kept for the next ones (at most 2 GiB + 512 MiB;
 * KVQ_BLOCK_CACHE=0 turns that off): this hands them back to the driver.  Nothing needs calling it. */
void    kvq_release_cached(void);

/* records first..first+n-1 of the synthetic FastQ stream of SURVEY 8(d)
 * (kvarq_amd/synth.py is the byte-identical numpy statement) written to
 * d_out (n * (2L+25) bytes); d_genome = the synthetic genome in device memory */
int32_t kvq_synth_reads_device(void *d_out, int64_t first, int64_t n, int32_t L,
                               uint64_t seed, const void *d_genome, int64_t genome_size);
/* the same on the host (single thread) */
void    kvq_synth_reads_host(uint8_t *out, int64_t first, int64_t n, int32_t L,
                             uint64_t seed, const uint8_t *genome, int64_t genome_size);
/* i.i.d. genome bases before planting (synth.genome does the planting) */
void    kvq_synth_genome_host(uint8_t *out, int64_t size, uint64_t seed);

/* ---- BGZF (bgzip) members: raw DEFLATE, on the host and on the device -------------------------------------
 * The reference inflates with miniz (workhorse.c:790-884); this is the library's own decoder (no zlib), the same
 * code on both sides.  One member's payload (the bytes between its header and its CRC32/ISIZE trailer) inflates
 * to exactly ISIZE (<= 65536) bytes or fails: status 0, -3 (Z_DATA_ERROR, not a valid DEFLATE stream) or -5
 * (Z_BUF_ERROR, the payload ends early or the output is not exactly ISIZE bytes), -2 for bad arguments.  Bytes
 * behind the final block are ignored; CRC32 is not checked (neither does the reference).  Reads in[0, n) and
 * writes out[0, isize) only. */
int32_t kvq_inflate_raw_host(const uint8_t *in, int64_t n, uint8_t *out, int64_t isize);

/* host only: the blocks of the bytes of a BGZF file -- file offset, block bytes (BSIZE + 1), ISIZE -- up to cap of
 * them; returns their number, or -1 when the bytes are not BGZF to the end (a member without the 'BC' subfield,
 * ISIZE > 65536, more than 10 bytes behind the last block).  A member's payload is
 * [block_off + 12 + XLEN, block_off + csize - 8). */
int64_t kvq_bgzf_index(const uint8_t *file_bytes, int64_t n, int64_t *block_off, uint32_t *csize, uint32_t *isize, int64_t cap);

/* one entry per member, in device memory: its payload at d_in + in_off (in_len bytes), its ISIZE, where its bytes go */
typedef struct kvq_bgzf_block {
    int64_t  in_off;
    int64_t  out_off;
    uint32_t in_len;
    uint32_t isize;
} kvq_bgzf_block;

/* inflate nblocks members on the GPU (one wavefront each) into d_out; d_status[b] (device int32) gets member b's
 * status as above.  An entry outside d_in[0, in_bytes) or d_out[0, out_bytes) gets -2 and touches nothing; a
 * member that fails may have written part of its own output bytes, never any outside them.  Blocking; KVQ_OK or
 * KVQ_ERR_DEVICE. */
int32_t kvq_inflate_bgzf_device(const void *d_in, int64_t in_bytes, const kvq_bgzf_block *d_blocks, int64_t nblocks,
                                void *d_out, int64_t out_bytes, int32_t *d_status);

/* kvq_chunk_offsets for text in device memory (nbytes of it at d_data), cut on the GPU (the cuts of the device-inflate
 * route of kvq_findseqs_ex): writes nchunks+1 offsets, so offsets holds cap + 1 entries (cap >= nbytes/512Ki + 4);
 * returns nchunks, or -1 when a chunk holds no record start (kvq_last_error: the host route's message, offsets
 * relative to d_data) or on a device failure */
int64_t kvq_chunk_offsets_device(const void *d_data, int64_t nbytes, int64_t *offsets, int64_t cap);

/* ---- plain gzip by speculative chunk decoding ----------------------------------------------------
 * A whole gzip file's bytes are cut into chunks of chunk_bytes (>= 64) compressed bytes; each chunk is decoded from the first
 * dynamic-Huffman block header behind its start with its 32 KiB window unknown, the chain of chunks is checked (a chunk whose
 * predecessor did not end exactly at its start is decoded again from where it did end), the windows are resolved in order and
 * the markers replaced.  The text is the host reader's (GzSerial, kvq_reader.hip): members crossed by its rules, a file cut
 * short ends the text, no CRC32 check.  Returns the text's length -- written to out only when it fits out_cap --, or -1 when
 * the DEFLATE data fail (*status: zlib's status, -3; *err_fpos: the text offset at which the failing block's output starts;
 * kvq_last_error: the host route's message), -2 on other errors (no gzip header at byte 0: the host route's message). */
typedef struct kvq_gzip_report {
    int64_t runs;               /* runs of compressed bytes (one per call here; kvq_findseqs_ex: per batch) */
    int64_t chunks;             /* chunks the runs were cut into (after merging those without a candidate) */
    int64_t candidates_tested;  /* bit offsets the block finder examined, up to and including each chunk's candidate */
    int64_t refuted;            /* chunks whose start the chain check moved (a false candidate, or one behind a false one) */
    int64_t redecodes;          /* chunk decodes after the first one of each chunk */
    int64_t slot_overflows;     /* decodes that ran out of slot and were repeated in a larger one */
    int64_t marker_symbols;     /* text bytes that were decoded as markers of an unknown window and replaced */
    int64_t input_retries;      /* runs whose last chunk read past the margin behind them (a block or member header longer than
                                   it) and that were done again with a margin 4x larger; such a run counts once in runs, chunks,
                                   candidates_tested, refuted, slot_overflows and marker_symbols, as its last attempt does, and
                                   the decodes of the attempts before it count in redecodes */
    double  ms_find, ms_decode, ms_resolve, ms_replace;     /* wall time of the phases, every attempt included (each phase ends
                                                               in a wait for its kernels) */
} kvq_gzip_report;

/* on the CPU: the same decoder source and chunked algorithm as on the GPU */
int64_t kvq_inflate_gzip_host(const uint8_t *file, int64_t n, int64_t chunk_bytes, uint8_t *out, int64_t out_cap,
                              int32_t *status, int64_t *err_fpos, kvq_gzip_report *rep);
/* on the GPU: d_file and d_out in device memory; writes d_out[0, text length) only, and only when it fits out_cap.  Blocking */
int64_t kvq_inflate_gzip_device(const void *d_file, int64_t n, int64_t chunk_bytes, void *d_out, int64_t out_cap,
                                int32_t *status, int64_t *err_fpos, kvq_gzip_report *rep);
/* the report of the last kvq_inflate_gzip_* or kvq_findseqs_ex call that took the speculative route */
void    kvq_gzip_last_report(kvq_gzip_report *rep);
/* test hook, for the last kvq_inflate_gzip_* call: the block finder's candidate per nominal chunk start (-1: none; *ncand of
 * them, up to ncand_cap written) and per chunk that held its start bit, the bit it ended at (-1: the text ended in it) and its
 * symbols (up to cap written); returns the number of chunks that held */
/* test hook: from now on every chunk slot of the speculative route (host and device alike) lies between pad_symbols (0..65536;
 * 0: none) canary symbols on each side, checked after each decode; returns how many canary symbols were found overwritten since
 * the call before, and starts counting again */
int64_t kvq_gzip_slot_canaries(int32_t pad_symbols);
int64_t kvq_gzip_last_chunks(int64_t *cand, int64_t ncand_cap, int64_t *start_bit, int64_t *end_bit, int64_t *nsym, int64_t cap,
                             int64_t *ncand);

/* ---- BAM records as FastQ text -------------------------------------------------------------------
 * kvq_findseqs and kvq_findseqs_ex scan a BAM file (its first BGZF block inflates to "BAM\1"; the name does not matter) as
 * its *virtual FastQ text*: every primary record with bases, in file order, as
 *   '@' name ["/1" | "/2" by flag & 0xC0] '\n' bases '\n' '+' '\n' qualities '\n'
 * bases "=ACMGRSVTWYHKDBN"[code], qualities q + 33 ('"' for every base when qualities are absent), both reversed and the
 * bases complemented for flag 0x10; records with flag & 0x900 or l_seq == 0 write nothing.  Hits, counters, stats (but
 * total), records: those of a scan of that text; file_pos counts its bytes.  The text is made on the GPU only: a call whose
 * files are all BAM takes that route whatever the flags say (kvq_scan_path bit 6), one that mixes BAM and other files fails
 * with KVQ_ERR_IO.  A record is well-formed when l_read_name >= 2, its name is printable and NUL-terminated, refID and
 * next_refID lie in [-1, n_ref), pos and next_pos >= -1, l_seq >= 0, 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 +
 * l_seq <= block_size and the record ends inside the file's inflated stream; the first that is not gives KVQ_ERR_IO
 * "malformed BAM record : offset=<its offset in the file's inflated stream>". */
typedef struct kvq_bam_report {
    int64_t runs;               /* runs of whole BGZF blocks (one per call of kvq_bam_to_fastq_device) */
    int64_t segments;           /* segments the runs were cut into (KVQ_BAM_SEGMENT_KB) */
    int64_t refuted;            /* segments the chain check walked again (a false start, or one behind a false one) */
    int64_t check_passes;       /* passes of the chain check, the first one of each run included */
    int64_t records_seen;       /* records on the chain */
    int64_t records_written;    /* ... that wrote text */
    int64_t records_skipped;    /* ... that did not (flag & 0x900, l_seq == 0) */
    int64_t records_noqual;     /* written records without qualities (qual[0] == 0xFF) */
    int64_t bam_bytes;          /* inflated BAM bytes, headers included */
    int64_t text_bytes;         /* FastQ bytes written */
    double  ms_inflate, ms_find, ms_emit;   /* wall time of the phases (each ends in a wait for its kernels; find includes the
                                               chain check's passes) */
} kvq_bam_report;
/* the report of the last kvq_bam_to_fastq_* call or kvq_findseqs call that scanned BAM */
void    kvq_bam_last_report(kvq_bam_report *rep);
/* host only: the header at the front of a file's inflated bytes; returns the first record's offset and *n_ref, -1 when the
 * header is malformed, -2 when the n bytes end inside it */
int64_t kvq_bam_header_host(const uint8_t *inflated, int64_t n, int32_t *n_ref);
/* on the CPU (the twin of the GPU route, over the same source): the virtual FastQ text of the records in inflated[first_record, n),
 * n being the end of the file's inflated stream.  Returns the text's length -- written to out only when it fits cap --, or -1
 * at the first malformed record (*consumed: its offset; kvq_last_error: the route's message), -2 on bad arguments.  *consumed
 * (may be NULL): where the walk stopped */
int64_t kvq_bam_to_fastq_host(const uint8_t *inflated, int64_t n, int32_t n_ref, int64_t first_record, uint8_t *out, int64_t cap,
                              int64_t *consumed);
/* on the GPU, the route's kernels alone: d_in[0, n) and d_out in device memory, segment_bytes (0: KVQ_BAM_SEGMENT_KB, else
 * 1 .. 64 MiB).  Returns the text's length -- written to d_out only when it fits cap --, -1 at the first malformed record
 * (kvq_last_error as above), -2 on other errors.  Blocking; *report (may be NULL) as kvq_bam_last_report */
int64_t kvq_bam_to_fastq_device(const void *d_in, int64_t n, int32_t n_ref, int64_t first_record, void *d_out, int64_t cap,
                                int64_t segment_bytes, kvq_bam_report *report);
/* One run, as the route takes a file: p[0, n) is a prefix of a stream that ends at limit >= n (both relative to p).  Returns
 * the text bytes of the records that lie wholly inside the prefix; *end (may be NULL): where the chain left the prefix, n or
 * the offset of the record the prefix ends inside (what the route carries to the next run).  -1 at a malformed record (*end:
 * its offset; kvq_last_error as above; a rule that shows in the bytes there are is not waited for), -2 on bad arguments or
 * other errors.  kvq_bam_to_fastq_host / _device are these with limit = n (and out_off = 0).  The device run writes its text
 * to d_out + out_off, d_out holding cap bytes, when out_off + text <= cap, and no other byte of d_out; it reads no byte of
 * d_p behind n. */
int64_t kvq_bam_run_host(const uint8_t *p, int64_t n, int64_t limit, int32_t n_ref, int64_t first_record, uint8_t *out, int64_t cap,
                         int64_t *end);
int64_t kvq_bam_run_device(const void *d_p, int64_t n, int64_t limit, int32_t n_ref, int64_t first_record, void *d_out, int64_t out_off,
                           int64_t cap, int64_t segment_bytes, int64_t *end, kvq_bam_report *report);

const char *kvq_version(void);

#ifdef __cplusplus
}
#endif
#endif
