"""
Inputs built for the seams of the finish tail (kvq_fold_batch and kvq_cov_apply in kernels_general.hip, the ordering
and gather kernels of kernels_results.hip, the grow-and-rescan logic of kvq_finish.hip), and the helpers
with which a test shows that its input reached the seam it names.  No GPU here: tests/test_results_host.py checks the
generators against the oracle alone, tests/test_gpu_results.py runs them through the library.

The reference of every text is the oracle (``O.scan_memory(..., fold=True)``): hits in reference order, hit bytes,
coverage and mutations.  Nothing is derived from the library under test; where a generator has to know how many hits
a read yields it asks the oracle.  Texts and references are built once per process and shared (never change them).
"""
import bisect
import functools
import random

import numpy as np

import cases
from oracle import oracle as O

ORDER_BLOCKS = 512          # workgroups of the ordering kernels: contiguous shares of the buckets
BUCKET_MAX = 64             # more hits in one bucket: "crowded", the merge sort orders the scan
GATHER_CHUNK = 256          # hits kvq_gather_shares takes of its share at a time

CFG = dict(cases.DEFAULTS, minreadlength=10)                                                    # maxerrors 0, minoverlap 20
FOLD_CFG = dict(cases.DEFAULTS, maxerrors=2, minoverlap=25, minreadlength=25)


# ---- the reference ------------------------------------------------------------------------------------------------

class Ref(object):
    """the oracle's result of one text (or of several pieces of a stream, added up) as arrays"""

    def __init__(self, seqs, outs):
        self.seqs = list(seqs)
        hits = [h for o in outs for h in o['hits']]
        self.hitseqs = [hs for o in outs for hs in o['hitseqs']]
        self.n = len(hits)
        self.seq_nr = np.array([h.seq_nr for h in hits], dtype=np.int32)
        self.file_pos = np.array([h.file_pos for h in hits], dtype=np.int64)
        self.seq_pos = np.array([h.seq_pos for h in hits], dtype=np.int32)
        self.length = np.array([h.length for h in hits], dtype=np.int32)
        self.readlength = np.array([h.readlength for h in hits], dtype=np.int32)
        self.offsets = np.concatenate([[0], np.cumsum([len(hs) for hs in self.hitseqs])]).astype(np.int64)
        self.blob = b''.join(self.hitseqs)
        self.nseqhits = np.sum([o['stats']['nseqhits'] for o in outs], axis=0).astype(np.int64)
        self.nseqbasehits = np.sum([o['stats']['nseqbasehits'] for o in outs], axis=0).astype(np.int64)
        self.coverage = np.sum([o['coverage'] for o in outs], axis=0).astype(np.int64)
        self.mutations = np.sum([o['mutations'] for o in outs], axis=0).astype(np.int64)
        self.records_parsed = sum(o['stats']['records_parsed'] for o in outs)


def oracle(text, seqs, cfg=CFG, fpos_base=0):
    return O.scan_memory(np.frombuffer(text, dtype=np.uint8), seqs, fpos_base=fpos_base, fold=True, **cfg)


def reference(text, seqs, cfg=CFG):
    return Ref(seqs, [oracle(text, seqs, cfg)])


# ---- helpers ------------------------------------------------------------------------------------------------------

def hits_per_read(file_pos):
    """(file_pos of the read, hits) per read that has hits, in stream order: the hits of one read share its file_pos"""
    fp, cnt = np.unique(np.asarray(file_pos, dtype=np.int64), return_counts=True)
    return list(zip(fp.tolist(), cnt.tolist()))


def occupancy(file_pos, lo, shift, bc, nb):
    """hits per bucket [nb] and per share [ORDER_BLOCKS] of the ordering for the geometry kvq_scan_order_info reports
    (bucket = (file_pos - lo) >> shift, share = bucket // bc), counted from the ORACLE's file_pos column"""
    b = (np.asarray(file_pos, dtype=np.int64) - lo) >> shift
    assert len(b) == 0 or (int(b.min()) >= 0 and int(b.max()) < nb), 'a hit outside the buckets'
    return np.bincount(b, minlength=nb), np.bincount(b // bc, minlength=ORDER_BLOCKS)


def plan_geometry(lo, hi, n, arena_cap=1 << 20):
    """(shift, nb, bc) of the ordering as DESIGN 4.4 states it: `want` = the power of two >= max(256, 4 n), at most the
    same of the arena's capacity and at most 2^22; the smallest shift with span >> shift < want; nb buckets in
    ORDER_BLOCKS shares of bc"""
    nb_max = 256
    while nb_max < 4 * arena_cap and nb_max < (1 << 22):
        nb_max <<= 1
    want = 256
    while want < 4 * n and want < nb_max:
        want <<= 1
    span = max(hi - lo, 1)
    shift = 0
    while (span >> shift) >= want:
        shift += 1
    nb = (span >> shift) + 1
    return shift, nb, (nb + ORDER_BLOCKS - 1) // ORDER_BLOCKS


def split_records(text):
    """(record start, bases line start, bases line end, record end) of every four-line record"""
    out, at = [], 0
    while at < len(text):
        nl = [at - 1]
        for _ in range(4):
            nl.append(text.index(b'\n', nl[-1] + 1))
        out.append((at, nl[1] + 1, nl[2] + 1, nl[4] + 1))
        at = nl[4] + 1
    return out


def records_of(text, file_pos, base=0):
    """the record of every hit: the one whose bases line holds its file_pos"""
    recs = split_records(text)
    starts = [r[1] for r in recs]
    out = []
    for fp in file_pos:
        a, b0, b1, e = recs[bisect.bisect_right(starts, int(fp) - base) - 1]
        assert b0 <= int(fp) - base < b1
        out.append(text[a:e])
    return out


def mismatch_offsets(ref):
    """per hit: the offsets inside the hit at which its bytes differ from the sequence (analyse.py:70-78)"""
    out = []
    for i in range(ref.n):
        s = ref.seqs[int(ref.seq_nr[i])]
        start = max(int(ref.seq_pos[i]), 0)
        hs = ref.hitseqs[i]
        out.append([j for j in range(len(hs)) if hs[j] != s[start + j]])
    return out


def _seq(rng, n, avoid=()):
    """n random bases without any of the words in `avoid`"""
    while True:
        s = cases.randseq(rng, n)
        if not any(w in s for w in avoid):
            return s


# ---- ladder: reads of exactly k hits, k = 1..64 ------------------------------------------------------------------
# Sequences of 1, 2, 3, 15, 16, 17, 31, 32, 33 and 45 bases: as whole sequences inside a read (class C) they give hits of
# those lengths; the long ones overlap a read's end (class A: seq_pos < 0, cut at the read's end) and a read's head (class B).

_rng = random.Random(20240611)
LADDER_SEQS = [b'N', b'GT', b'ACG'] + [_seq(_rng, n, avoid=('GT', 'ACG')).encode() for n in (15, 16, 17, 31, 32, 33, 45)]
LADDER_ROUNDS = 6
LADDER_MIN_BASES = 130


def _ladder_kinds():
    s = [x.decode() for x in LADDER_SEQS]
    kinds = [('', '', ''), ('', 'N', ''), ('', 'GT', ''), ('', 'NNGT', '')]
    kinds += [('', x, '') for x in s[3:]]                           # a whole sequence inside the read: class C
    kinds += [('', '', s[9][:27]), ('', '', s[8][:22]), ('', '', s[6][:30])]      # the read's tail on a sequence's head: class A
    kinds += [(s[9][-24:], '', ''), (s[7][-21:], '', '')]           # the read's head on a sequence's tail: class B
    return kinds


def _ladder_read(kind, j):
    head, mid, tail = kind
    body = head + 'ACG' * j + mid
    return body + 'C' * max(0, LADDER_MIN_BASES - len(body) - len(tail)) + tail


def _text_of(reads, prefix):
    return b''.join(cases.rec('%s%d' % (prefix, i), r, 'I' * len(r)) for i, r in enumerate(reads))


def _counts_per_read(reads, seqs, cfg=CFG):
    """hits of every read of `reads` (the oracle's count)"""
    text = _text_of(reads, 'c')
    o = oracle(text, seqs, cfg)
    per = dict(hits_per_read([h.file_pos for h in o['hits']]))
    return [per.get(b0, 0) for _, b0, _, _ in split_records(text)]


@functools.lru_cache(maxsize=None)
def ladder_reads():
    """LADDER_ROUNDS x 64 reads: round r holds a read of exactly k hits for every k in 1..64, of rotating make"""
    kinds = _ladder_kinds()
    cand = [(ki, j) for ki in range(len(kinds)) for j in range(66)]
    counts = _counts_per_read([_ladder_read(kinds[ki], j) for ki, j in cand], LADDER_SEQS)
    by_count = {}
    for (ki, j), c in zip(cand, counts):
        by_count.setdefault(c, []).append((ki, j))
    reads = []
    for r in range(LADDER_ROUNDS):
        for k in range(1, 65):
            want = (k * 5 + r * 7) % len(kinds)
            ki, j = min(by_count[k], key=lambda c: ((c[0] - want) % len(kinds), c[1]))
            reads.append(_ladder_read(kinds[ki], j))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def ladder():
    """-> (text, sequences): occupancies 1..64, none above"""
    return _text_of(ladder_reads(), 'L'), LADDER_SEQS


READ65 = 'ACG' * 65          # 65 hits of b'ACG' and no other


@functools.lru_cache(maxsize=None)
def ladder65(where):
    """the ladder with one read of 65 hits 'first', in the 'middle' or 'last' in the stream: one crowded bucket"""
    reads = list(ladder_reads())
    at = {'first': 0, 'middle': len(reads) // 2, 'last': len(reads)}[where]
    reads.insert(at, READ65)
    return _text_of(reads, 'L'), LADDER_SEQS


# ---- ties: hits of one read on one sequence that differ only in class or ordinal -----------------------------------

TIES_SEQS = {'wave': [b'ACGT' * 12, b'ACGT' * 6], 'network': [b'ACGT' * 6]}


@functools.lru_cache(maxsize=None)
def ties(regime):
    """'wave': every read has 9..64 hits, 'network': 2..8; periodic reads on periodic sequences: classes A, B and C
    on one (file_pos, seq_nr).  Reads the oracle counts outside the regime are left out."""
    seqs = TIES_SEQS[regime]
    lo, hi, reps = (9, 64, (13, 14, 15)) if regime == 'wave' else (2, 8, (7, 8))
    reads = [p + 'ACGT' * m + q for m in reps for p in ('', 'G', 'CC', 'TTT') for q in ('', 'A', 'AC')] * 8
    keep = [r for r, c in zip(reads, _counts_per_read(reads, seqs)) if lo <= c <= hi]
    return _text_of(keep, 'T'), seqs


# ---- dense corner: one contiguous sixteenth of the reads carries 32 hits each --------------------------------------

DENSE_READS, DENSE_HOT = 16384, (7 * 1024, 8 * 1024)
DENSE_HOT_READ = 'ACG' * 4 + 'GT' * 4 + 'N' * 24 + 'CC'        # 4 + 4 + 24 hits
DENSE_COLD_READ = 'C' * len(DENSE_HOT_READ)


@functools.lru_cache(maxsize=None)
def dense_corner():
    recs = [cases.rec('d', DENSE_HOT_READ if DENSE_HOT[0] <= i < DENSE_HOT[1] else DENSE_COLD_READ, 'I' * len(DENSE_HOT_READ))
            for i in range(DENSE_READS)]
    return b''.join(recs), LADDER_SEQS


# ---- tiny: 0, 1 and 2 hits ------------------------------------------------------------------------------------------

TINY = ('zero', 'one', 'two_in_one', 'first_and_last')


@functools.lru_cache(maxsize=None)
def tiny(which):
    cold, one, two = 'C' * 60, 'C' * 20 + 'ACG' + 'C' * 37, 'C' * 20 + 'ACG' + 'CCC' + 'GT' + 'C' * 32
    reads = [cold] * 500
    if which == 'one':
        reads[250] = one
    elif which == 'two_in_one':
        reads[250] = two
    elif which == 'first_and_last':
        reads[0] = reads[-1] = one
        # the last read's hit is to fall into the LAST bucket (plan_geometry): a longer name in the middle moves it there
        for pad in range(256):
            recs = [cases.rec('t%d%s' % (i, 'x' * pad if i == 250 else ''), r, 'I' * len(r)) for i, r in enumerate(reads)]
            text = b''.join(recs)
            last_fpos = len(text) - len(recs[-1]) + recs[-1].index(b'\n') + 1
            shift, nb, _ = plan_geometry(0, len(text), 2)
            if last_fpos >> shift == nb - 1:
                return text, LADDER_SEQS
        raise AssertionError('no padding puts the last hit into the last bucket')
    else:
        assert which == 'zero'
    return _text_of(reads, 't'), LADDER_SEQS


# ---- offset batches: the ladder in two batches far from 0, with a gap between them ------------------------------------

OFFSET_BASE = (1 << 33) + 12345
OFFSET_GAP = 5 * (1 << 20) + 4321


@functools.lru_cache(maxsize=None)
def offset_batches():
    """-> ([(piece, fpos_base), (piece, fpos_base)], sequences)"""
    text, seqs = ladder()
    cut = [r[0] for r in split_records(text)]
    cut = cut[len(cut) // 2 + 3]
    return [(text[:cut], OFFSET_BASE), (text[cut:], OFFSET_BASE + cut + OFFSET_GAP)], seqs


@functools.lru_cache(maxsize=None)
def offset_reference():
    pieces, seqs = offset_batches()
    return Ref(seqs, [oracle(p, seqs, CFG, fpos_base=base) for p, base in pieces])


# ---- fold: mismatches at the seams of the fold's 16-byte step, every mutation class, the coverage end marks ----------

FOLD_LENGTHS = (64, 65, 127, 128)
FOLD_OFFSETS = ((0,), (3,), (4,), (15,), (16,), (-1,), (0, -1), (3, 4), (15, 16))
FOLD_LETTERS = 'ACGTNR'


@functools.lru_cache(maxsize=None)
def fold():
    """-> (text, sequences), FOLD_CFG (maxerrors 2): whole sequences inside reads (class C), reads on the sequences'
    tails (class B, 40 bases: they end on the last base) and heads (class A, seq_pos < 0), with one or two planted
    mismatches at hit offsets 0, 3, 4, 15, 16 and the last, of every letter.  Only the reads the oracle confirms."""
    rng = random.Random(977)
    seqs = [_seq(rng, n) for n in FOLD_LENGTHS]
    reads = []
    for s in seqs:
        for make in ('C', 'B', 'A'):
            part = s if make == 'C' else s[-40:] if make == 'B' else s[:40]
            for offs in FOLD_OFFSETS:
                for letter in FOLD_LETTERS:
                    p = list(part)
                    for o in offs:
                        o %= len(p)
                        p[o] = letter if p[o] != letter else FOLD_LETTERS[(FOLD_LETTERS.index(letter) + 1) % 6]
                    p = ''.join(p)
                    a, b = cases.randseq(rng, rng.randint(5, 12)), cases.randseq(rng, rng.randint(5, 12))
                    reads.append(a + p + b if make == 'C' else p + b + 'CATCATCATCATCAT' if make == 'B' else 'CATCATCATCATCAT' + a + p)
    seqs = [s.encode() for s in seqs]
    keep = [r for r, c in zip(reads, _counts_per_read(reads, seqs, FOLD_CFG)) if c > 0]
    if sum(_counts_per_read(keep, seqs, FOLD_CFG)) % 64 == 0:
        keep.pop()
    return _text_of(keep, 'F'), seqs


# ---- the references, one per text -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ref_of(name, arg=None):
    if name == 'fold':
        return reference(*fold(), cfg=FOLD_CFG)
    text, seqs = {'ladder': ladder, 'dense_corner': dense_corner}[name]() if arg is None else \
        {'ladder65': ladder65, 'ties': ties, 'tiny': tiny}[name](arg)
    return reference(text, seqs)
