#!/usr/bin/env python3
"""
Generated files through every input pass and every route, against the plain statements.  Not a test module:
the cases, their references and the checks that tests/test_fuzz_passes_host.py (CPU) and tests/test_gpu_fuzz_passes.py (MI355X)
run over a fixed slice.  Building the cases and their references needs no GPU; the legs do.

usage: python tests/fuzz_passes.py FIRST COUNT [seeded]

runs the legs of the GPU test over any seed range, prints one line per failing seed and exits with status 1 if any failed.

A case is a case of ``tools/fuzz_parity.make_case`` (ragged reads, N and stray bytes, headers and '+' lines with text, CR LF,
score lines of another length than their bases line or that start with '@' or '+', truncated tails, blank lines behind the last
record, now and then a malformed record) with, from ``random.Random(seed ^ 0x5EED)``: adapter probes cut from its own reads, a
block of extra records IN FRONT of the text (planted probes, tails, near-misses, score lines one byte short or long, a probe cut
in two by a record's end, repeated records, a line of 9000 bases beside lines of 0 and 7 in one wave), 0 to 8 cutoffs, and sizes for
the duplication table and the candidates of the overrepresented sequences.  The yardsticks are the plain Python statements of the passes (``profile_ref``, ``cycles_ref``, ``reads_ref``, ``over_ref``, ``adapt_ref``,
``clip_ref``) and the oracle; every comparison is exact.

From a stream of its own (``random.Random(seed ^ 0xE317)``: the draws above stay where they were, ``SLICE_DIGEST``) a case also has
an ``emit_min`` and a ``per`` of ``adapter_mismatches``.  Four more legs (``NEW_LEGS``, in NGROUPS_NEW groups of their own) take the
emit, its deflate to BGZF and the tolerant probes through the same files: against ``emit_ref.emit``, the Hamming loop of
``adapt_mm_ref``, the deflate's CPU twin for the bytes of a member (which the host test holds to zlib and ``deflate_ref.check``)
and ``deflate_ref.parse`` for its tokens.
"""
import bisect
import collections
import functools
import gzip
import hashlib
import os
import random
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'tools'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adapt_mm_ref as AM                                      # noqa: E402
import adapt_ref as A                                          # noqa: E402
import clip_ref as CR                                          # noqa: E402
import cycles_ref as CY                                        # noqa: E402
import deflate_ref as D                                        # noqa: E402
import emit_ref as E                                           # noqa: E402
import fuzz_parity as F                                        # noqa: E402
import over_ref as OV                                          # noqa: E402
import profile_ref as R                                        # noqa: E402
import reads_ref as RR                                         # noqa: E402
from kvarq_amd import profile as P                             # noqa: E402
from oracle import oracle as O                                 # noqa: E402

SLICES = ((False, 1, 60), (True, 2000, 90))                    # the seeds of tests/test_gpu_fuzz.py
SMALL, CHUNK = 300000, 1 << 20                                 # the slice: texts up to SMALL bytes, and two above KVQ_SCANBUFSIZE
PROBE_LENGTHS = (8, 12, 20, 31, 32)
CODE_MATES = b'BDHKMRSUVWY'                                    # letters that share (byte >> 1) & 3 with one of A C G T
STAT_KEYS = ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed')

EMIT_MINS, PERS = (None, 0, 1, 30), (10, 12, 16, 32)           # emit_min (None: the configured minreadlength) and adapter_mismatches

Case = collections.namedtuple('Case', 'seed seeded text seqs cfg probes cuts dup_slots over_records eol block_bytes emit_min per')


# ---- the cases ---------------------------------------------------------------------------------------------------------------

def _bases_lines(text):
    return [text[n0 + 1:n1].rstrip(b'\r') for n0, n1, _, _ in R.records_of(text, [0, len(text)])]


def _score_bytes(text):
    seen = set()
    for _, _, n2, n3 in R.records_of(text, [0, len(text)]):
        seen.update(text[n2 + 1:n3])
    return bytes(sorted(seen - {10, 13})) or b'I'


def _probes(rnd, seed, lines):
    pure = [l for l in lines if len(l) >= 40 and not l.strip(b'ACGT')]
    if not pure:
        return list(A.EIGHT[:2])
    probes = []
    for _ in range(rnd.randint(1, 3)):
        line, m = rnd.choice(pure), rnd.choice(PROBE_LENGTHS)
        at = rnd.randrange(len(line) - m + 1)
        probes.append(line[at:at + m])
    if seed % 3 == 0:
        probes.append(A.POLY_A)
    if seed % 5 == 0:
        probes += A.EIGHT
    out = []
    for p in probes:
        if p not in out:
            out.append(p)
    return out[:A.MAX_PROBES]


def _block(rnd, seed, lines, probes, eol, alphabet, dense):
    """the extra records: bytes.  ``dense``: a case whose records have hits at most of their positions (reads of a base or two pass
    the length gate, or a sequence of a few bases): a small block, so that the hits stay a number a test can compare in seconds"""
    stock = [l for l in lines if l]

    def material(n):
        out = b''
        while len(out) < n:
            more = rnd.choice(stock) if stock else bytes(rnd.choice(b'ACGT') for _ in range(n))
            out += more[rnd.randrange(len(more)):] if not out else more         # (from anywhere in a line: many different keys)
        return out[:n]

    def line_of(least):
        base = rnd.choice(stock) if stock else b''
        if len(base) < max(least, 40):
            base = material(max(least, rnd.randint(40, 150)))
        return base[:max(least, rnd.choice([50, 100, 150, 151, 300]))]

    def plant(probe, how=None):
        base = bytearray(line_of(len(probe)))
        L, m = len(base), len(probe)
        p = rnd.choice([0, L - m, rnd.randint(0, L - m)])
        put = bytearray(probe)
        if how is not None:
            i = rnd.randrange(m)
            if how == 'lower':
                put[i] |= 0x20
            elif how == 'N':
                put[i] = ord('N')
            else:
                put[i] = rnd.choice([c for c in CODE_MATES if (c >> 1) & 3 == (put[i] >> 1) & 3])
        base[p:p + m] = put
        return bytes(base)

    def tail(probe):
        base = line_of(40)
        t = rnd.randint(A.T, len(probe) - 1)
        return base[:len(base) - t] + probe[:t]

    def record(i, bases, delta=None):
        if delta is None:
            delta = rnd.choice([-1, 1]) if rnd.random() < 0.15 else 0
        scores = bytes(rnd.choice(alphabet) for _ in range(max(0, len(bases) + delta)))
        head = b'@b%d' % i + (b' ' + bytes(rnd.choice(b'abc:/ 0123456789#+-') for _ in range(rnd.randint(0, 12))) if rnd.random() < 0.3 else b'')
        return head + eol + bases + eol + (b'+' if rnd.random() < 0.8 else b'+' + head[1:]) + eol + scores + eol

    crowd = seed % 4 == 1 and not dense                    # many short records of different keys: a small duplication table leaves level 0
    n = rnd.randint(900, 1200) if crowd else rnd.randint(20, 40) if dense else rnd.randint(20, 200)
    recs = []
    for i in range(n):
        kind = rnd.random()
        probe = rnd.choice(probes)
        if crowd and kind >= 0.3:
            bases = material(rnd.randint(20, 40))
        elif kind < 0.40:
            bases = plant(probe)
        elif kind < 0.60:
            bases = tail(probe)
        elif kind < 0.75:
            bases = plant(probe, rnd.choice(['lower', 'N', 'mate']))
        else:
            bases = line_of(0)
        recs.append(record(i, bases))
    for j in range(rnd.randint(2, 4)):                     # a few records many times: the duplication bins and the overrepresented list
        again = record(n + 10 + j, (plant(rnd.choice(probes)) if j % 2 else line_of(20))[:rnd.choice([30, 64, 65, 90])])
        recs += [again] * rnd.choice([2, 3, 9, 10] if dense else [2, 3, 9, 10, 50, 120, 300])
    # a probe cut in two by a record's end: a line of exactly 256 bases (one round of the search's sixteen lanes) ends with the
    # probe's first h bases, the NEXT record's line begins with the rest -- a tail (h >= 6) or nothing, never a full occurrence
    longer = [p for p in probes if len(p) >= 18]
    for i in range(0 if not longer else 1 if dense else 4):
        probe = rnd.choice(longer)
        h = 32 - rnd.randint(max(0, 33 - len(probe)), 15)
        recs.append(record(n + 20 + 2 * i, material(256 - h) + probe[:h], 0) + record(n + 21 + 2 * i, probe[h:] + material(rnd.randint(20, 60)), 0))
    rnd.shuffle(recs)
    if seed % 7 == 2 and not dense:
        # a line of 9000 bases beside lines of 0 and 7: one entry of four records, put in behind the shuffle at a multiple of four
        # records from the start of the text, where a wave of kvq_adapt_records / kvq_clip_records takes them as its four quarters
        quad = record(n, material(9000), 0) + record(n + 1, b'', 0) + record(n + 2, material(7), 0) + record(n + 3, plant(probes[0]), 0)
        before, slots = 0, [0]
        for i, entry in enumerate(recs):
            before += entry.count(b'\n') // 4                  # (an entry is one record, or the two of a split pair)
            if before % 4 == 0:
                slots.append(i + 1)
        recs.insert(rnd.choice(slots), quad)
    return b''.join(recs)


@functools.lru_cache(maxsize=None)
def case(seed, seeded=False):
    """the case of a seed, or None where make_case draws an empty file (tests/test_gpu_fuzz.py skips those)"""
    data, seqs, cfg = F.make_case(seed, seeded)
    if not data:
        return None
    rnd = random.Random(seed ^ 0x5EED)
    lines = _bases_lines(data)
    eol = b'\r\n' if b'\r\n' in data else b'\n'
    probes = _probes(rnd, seed, lines)
    dense = cfg['minreadlength'] < 8 or min(len(s) for s in seqs) < 8
    block = _block(rnd, seed, lines, probes, eol, _score_bytes(data), dense)
    k = rnd.choice([0, 1, 2, 4, 5, 8])
    pool = R.CUTOFFS8 + [ord(cfg['Amin'])]
    cuts = tuple(rnd.choice(pool) for _ in range(k))
    dup_slots, over_records = rnd.choice([None, 64, 1024]), rnd.choice([None, 50, 1000])
    later = random.Random(seed ^ 0xE317)                   # (a stream of its own: the draws above stay where they were, SLICE_DIGEST)
    emit_min, per = later.choice(EMIT_MINS), later.choice(PERS)
    return Case(seed, seeded, block + data, tuple(seqs), cfg, tuple(probes), cuts, dup_slots, over_records, eol, len(block), emit_min, per)


def environ(c):
    """the environment of a case: name -> value, None: unset"""
    return {'KVQ_DUP_SLOTS': None if c.dup_slots is None else str(c.dup_slots),
            'KVQ_OVER_RECORDS': None if c.over_records is None else str(c.over_records),
            'KVQ_STRIDE': str(random.Random(c.seed).choice([2, 4, 8, 8])) if c.seeded else None}


# ---- the references: computed once per case, left unchanged ----------------------------------------------------------------------

def oracle_outcome(text, seqs, cfg):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, 'o.fastq')
        with open(p, 'wb') as f:
            f.write(text)
        return F.outcome(lambda: O.findseqs(p, list(seqs), **cfg))


class Passes(object):
    """the plain statements of every pass over a text"""

    def __init__(self, c, text, co, per=0, like=None):
        """``per``: the adapters entry is the tolerant one (``adapt_mm_ref.adapt``); ``like``: the ``Passes`` of the same text under
        the same cuts, whose other entries are taken as they are"""
        self.co = co = [int(v) for v in co]
        self.per = per
        if like is not None:
            assert like.co == co
            self.words, self.cycles, self.reads, self.dup, self.over = like.words, like.cycles, like.reads, like.dup, like.over
        else:
            self.words = R.profile(text, list(c.cuts), co)
            self.cycles = CY.cycles(text, co)
            self.reads = RR.reads(text, co)
            self.dup = RR.dup(text, co, c.dup_slots or 0)
            self.over = OV.over(text, co, c.over_records or 0)
        self.adapt = AM.adapt(text, co, list(c.probes), per) if per else A.adapt(text, co, list(c.probes))
        for a in (self.words, self.cycles, self.reads, self.dup, self.over, self.adapt):
            a.flags.writeable = False

    def check_identities(self, c, text):
        R.check_identities(self.words, len(c.cuts), R.long_counts(text, list(c.cuts), self.co))
        CY.check_identities(self.cycles, self.words, CY.score_facts(text, self.co))
        RR.check_identities(self.reads, self.dup, self.words)
        OV.check_identities(self.over, self.words)
        if self.per:
            AM.check_identities(self.adapt)
        else:
            A.check_identities(self.adapt, self.words)


def same_passes(p, want, what=''):
    """a ``Profile`` with every pass against the plain statements, word for word"""
    assert p is not None and p.cycles is not None and p.reads is not None and p.duplication is not None and p.over is not None and p.adapters is not None, what
    dup = np.array([p.duplication[k] for k in P.DUP_HEADER] + [0, 0] + p.duplication['distinct'] + p.duplication['records'], dtype=np.int64)
    for name, got, ref in (('profile', p.words, want.words), ('cycles', p.cycles, want.cycles), ('reads', p.reads, want.reads),
                           ('duplication', dup, want.dup), ('overrepresented', p.over, want.over), ('adapters', p.adapters.words, want.adapt)):
        got = np.asarray(got)
        assert got.shape == ref.shape, '%s %s: %r words, not %r' % (what, name, got.shape, ref.shape)
        bad = np.nonzero(got != ref)[0][:6]
        assert bad.size == 0, '%s %s: words %r are %r, not %r' % (what, name, bad, got[bad], ref[bad])


def min_length(c, emit_min='drawn'):
    """the shortest read the emit keeps under an ``emit_min`` option (the case's drawn one): None is the configured minreadlength"""
    emit_min = c.emit_min if emit_min == 'drawn' else emit_min
    return c.cfg['minreadlength'] if emit_min is None else emit_min


def _key(text):
    return len(text), zlib.crc32(text)


@functools.lru_cache(maxsize=None)
def twin(text):
    """(BGZF(text) without the EOF member, the eight words) by the CPU twin, the yardstick for the bytes of a deflated batch as in
    tests/test_gpu_deflate.py; zlib inflates it to the text.  (tests/test_fuzz_passes_host.py holds every stream the legs compare
    to ``deflate_ref.check`` as well, which takes seconds a batch)"""
    out, words = P.deflate_bgzf_host(text)
    words.flags.writeable = False
    assert gzip.decompress(out + D.EOF) == text
    return out, words


def bgzf_of(batches):
    """the BGZF of a feeding: the twin's members of every batch that is not empty, one behind the other, and one EOF member"""
    return b''.join(twin(b)[0] for b in batches if b) + D.EOF


class Refs(object):
    def __init__(self, c):
        text = c.text
        self.c, self._emits, self._under, self._outcomes = c, {}, {}, {}
        self.outcome = oracle_outcome(text, c.seqs, c.cfg)
        self.accepted = self.outcome[0] == 'ok'
        self.co = self.passes = self.masked = self.clip_words = self.masked_outcome = self.masked_passes = None
        if not self.accepted:
            return
        self.co = [int(v) for v in O.chunk_offsets(text)]
        self.passes = Passes(c, text, self.co)
        self.recs = R.records_of(text, self.co)
        if ord(c.cfg['Amin']) > ord('!'):
            self.masked, self.clip_words = CR.mask(text, self.co, list(c.probes))
            self.masked_outcome = oracle_outcome(self.masked, c.seqs, c.cfg)
            self.masked_passes = Passes(c, self.masked, self.co)

    def record_of(self, text, file_pos):
        """the record whose bases line holds file_pos: from its start to its fourth newline (a last record that lacks it: to the end)"""
        if not hasattr(self, '_spans'):
            spans, at = [], 0
            for n0, n1, _, n3 in self.recs:
                at = max([at] + [o for o in self.co if at < o <= n0])       # (a chunk begins where its first record does)
                spans.append((n0, n1, at, n3 + 1)); at = n3 + 1
            self._spans, self._n0 = spans, [s[0] for s in spans]
        i = bisect.bisect_left(self._n0, file_pos) - 1
        if i >= 0 and self._spans[i][0] < file_pos <= self._spans[i][1]:
            return text[self._spans[i][2]:self._spans[i][3]]
        assert file_pos > (self._spans[-1][3] if self._spans else 0), file_pos
        return text[self._spans[-1][3] if self._spans else 0:]

    # ---- the emit and the tolerant probes: built when first asked for, once, from the plain statements ----
    def emit_of(self, text, co, m=None):
        """``emit_ref.emit(text, co, Amin, m)``: (the emitted text, the eight words); m None: the case's drawn ``emit_min``"""
        m = min_length(self.c) if m is None else m
        key = _key(text) + (tuple(int(v) for v in co), m)
        if key not in self._emits:
            out, words = E.emit(text, [int(v) for v in co], ord(self.c.cfg['Amin']), m)
            words.flags.writeable = False
            self._emits[key] = (out, words)
        return self._emits[key]

    def emit_batches(self, text, batches, m=None):
        """a feeding of several batches [(first byte, end, chunk offsets in the text)] -> ([the emitted text of each], the words)"""
        parts = [self.emit_of(text[x:y], [o - x for o in co], m) for x, y, co in batches]
        words = np.sum([w for _, w in parts], axis=0)
        words[E.N] = parts[0][1][E.N]
        return [p for p, _ in parts], words

    def outcome_of(self, text):
        """the oracle's outcome on another text than the case's (a masked one, an emitted one)"""
        if _key(text) not in self._outcomes:
            self._outcomes[_key(text)] = oracle_outcome(text, self.c.seqs, self.c.cfg)
        return self._outcomes[_key(text)]

    def under(self, co, per=0):
        """the ``Passes`` of the text under other chunk cuts than the reader's (``scanner_cuts``)"""
        key = (tuple(int(v) for v in co), per)
        if key not in self._under:
            if per:
                self._under[key] = Passes(self.c, self.c.text, co, per, like=self.under(co))
            else:
                self._under[key] = self.passes if key[0] == tuple(self.co) else Passes(self.c, self.c.text, co)
        return self._under[key]

    @property
    def tolerant(self):
        """``adapt_mm_ref.adapt(text, co, probes, per)``"""
        return self.passes_mm.adapt

    @property
    def passes_mm(self):
        """the passes of the text with the tolerant adapters entry"""
        return self.under(self.co, self.c.per)

    def _mask_mm(self):
        if not hasattr(self, '_masked_mm'):
            assert ord(self.c.cfg['Amin']) > ord('!')
            self._masked_mm = AM.mask(self.c.text, self.co, list(self.c.probes), self.c.per)
            self._masked_mm[1].flags.writeable = False
        return self._masked_mm

    masked_mm = property(lambda self: self._mask_mm()[0])
    clip_words_mm = property(lambda self: self._mask_mm()[1])
    masked_mm_outcome = property(lambda self: self.outcome_of(self.masked_mm))

    @property
    def masked_mm_passes(self):
        """the passes of the tolerantly masked text, its adapters entry the tolerant one of that text"""
        if not hasattr(self, '_masked_mm_passes'):
            self._masked_mm_passes = Passes(self.c, self.masked_mm, self.co, self.c.per)
        return self._masked_mm_passes

    @property
    def virtual(self):
        """the case as a BAM, where ``bam_records`` gives records: (the file's bytes, its virtual FastQ text, the oracle's outcome
        on that, its chunk offsets), else None"""
        if not hasattr(self, '_virtual'):
            import bam_writer as W
            from kvarq_amd import bam
            records, self._virtual = bam_records(self.c, self), None
            if records is not None:
                with tempfile.TemporaryDirectory() as d:
                    data = W.write(os.path.join(d, 'm.bam'), W.header(), records)      # (the BAM stream; the file is its BGZF)
                    written = _read(os.path.join(d, 'm.bam'))
                vtext = bytes(bam.to_fastq_host(data))
                self._virtual = (written, vtext, self.outcome_of(vtext), [int(v) for v in O.chunk_offsets(vtext)])
        return self._virtual


@functools.lru_cache(maxsize=None)
def refs(seed, seeded=False):
    return Refs(case(seed, seeded))


# ---- the slice -----------------------------------------------------------------------------------------------------------------

# the slice as the rule below gives it, written out so that listing the cases builds none of the large ones the rule leaves out
# (tests/test_fuzz_passes_host.py asserts that the two agree)
SLICE_GENERAL = (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24, 26, 27, 28, 29, 30, 32, 34, 37, 38, 39, 40, 41, 42, 43,
                 45, 46, 47, 48, 49, 51, 52, 53, 54, 56, 57, 59, 60, 33)
SLICE_SEEDED = (2000, 2002, 2003, 2004, 2005, 2007, 2008, 2009, 2010, 2012, 2013, 2014, 2015, 2018, 2019, 2021, 2022, 2023, 2024, 2025, 2026,
                2027, 2028, 2029, 2030, 2031, 2032, 2033, 2034, 2035, 2036, 2037, 2038, 2039, 2040, 2041, 2042, 2044, 2046, 2047, 2048, 2050,
                2051, 2052, 2053, 2054, 2055, 2059, 2060, 2061, 2062, 2064, 2065, 2066, 2067, 2068, 2070, 2071, 2072, 2075, 2078, 2079, 2080,
                2082, 2083, 2084, 2086, 2089, 2076)


def slice_():
    """[(seed, seeded)] of the test"""
    return tuple((seed, False) for seed in SLICE_GENERAL) + tuple((seed, True) for seed in SLICE_SEEDED)


def slice_by_rule():
    """of the seeds of tests/test_gpu_fuzz.py every case -- accepted or refused -- up to SMALL bytes, and behind them the two smallest
    accepted cases above KVQ_SCANBUFSIZE (the reader's own chunk cut; looked for among the texts up to 8 MiB).  Draws every file of
    those seeds, the largest of 30 MB"""
    small, big = [], []
    for seeded, first, count in SLICES:
        for seed in range(first, first + count):
            data = F.make_case(seed, seeded)[0]
            c = case(seed, seeded) if data and len(data) <= 8 * CHUNK else None
            if c is None:
                continue
            if len(c.text) <= SMALL:
                small.append((seed, seeded))
            elif len(c.text) > CHUNK:
                big.append((len(c.text), seed, seeded))
    big = [(seed, seeded) for _, seed, seeded in sorted(big) if refs(seed, seeded).accepted][:2]
    return tuple(s for s in small if not s[1]) + tuple(b for b in big if not b[1]) + tuple(s for s in small if s[1]) + tuple(b for b in big if b[1])


NGROUPS = 8                                                    # (a constant: collecting the tests builds no case)


NGROUPS_NEW = 24                                               # the legs of the emit and the tolerant probes (NEW_LEGS): their references take longer


def ngroups(leg):
    return NGROUPS_NEW if leg in NEW_LEGS else NGROUPS


def group(i, n=NGROUPS):
    """every n-th case of the slice from the i-th on: about 15 cases in each of NGROUPS groups, 5 in each of NGROUPS_NEW"""
    return slice_()[i::n]


def leads_its_group(c):
    """whether the case is the first of one of the NGROUPS_NEW groups"""
    return (c.seed, c.seeded) in slice_()[:NGROUPS_NEW]


# SHA-256 over (seed, seeded, text, seqs, sorted cfg items, probes, cuts, dup_slots, over_records) of every case of the slice, taken
# before ``Case`` gained ``emit_min`` and ``per``: the draws that were there have not moved
SLICE_DIGEST = 'c779aab2b6c4abd95ea4ad9f43e001f404d10ac51fa0cf592baa473b947f0496'


def slice_digest():
    h = hashlib.sha256()
    for s in slice_():
        c = case(*s)
        h.update(repr((c.seed, c.seeded, c.text, c.seqs, sorted(c.cfg.items()), c.probes, c.cuts, c.dup_slots, c.over_records)).encode())
    return h.hexdigest()


def wave_of_9000_0_7(text, recs):
    """whether four records that one wave of the adapter kernels takes (the 4 i-th to the 4 i + 3rd of the text, which the block is in
    front of) begin with a line of at least 9000 bases, one of none and one of 7"""
    lens = [len(text[n0 + 1:n1].rstrip(b'\r')) for n0, n1, _, _ in recs]
    return any(lens[i] >= 9000 and lens[i + 1:i + 3] == [0, 7] for i in range(0, len(lens) - 3, 4))


def census():
    """what the slice holds, from the references alone"""
    n = collections.Counter()
    for seed, seeded in slice_():
        c, r = case(seed, seeded), refs(seed, seeded)
        n['cases'] += 1; n['bytes'] += len(c.text)
        n['accepted' if r.accepted else 'refused'] += 1
        if not r.accepted:
            continue
        n['crlf'] += c.eol == b'\r\n'
        n['chunks>1'] += len(r.co) > 2
        n['hits'] += len(r.outcome[1])
        n['records'] += int(r.passes.words[R.RECORDS])
        n['with_full'] += int(r.passes.adapt[A.A_WITH_FULL]); n['tail_only'] += int(r.passes.adapt[A.A_TAIL_ONLY])
        n['clipped S!=L'] += sum(1 for _, L, clip, S in CR.per_record(c.text, r.co, list(c.probes)) if clip < L and S != L)
        n['mismatched'] += int(r.passes.words[R.MISMATCHED])
        n['dup level>0'] += r.passes.dup[RR.D_LEVEL] > 0
        n['over listed'] += r.passes.over[OV.O_LISTED] > 0
        n['line>1024'] += r.passes.words[R.LONGEST] - 1 > CY.CYCLES
        n['9000 beside 0 and 7'] += wave_of_9000_0_7(c.text, r.recs)
        n['spread' if len(c.cuts) <= 4 else 'wave'] += 1
        n['clip legs'] += r.masked is not None
        n['probes'] += len(c.probes)
    return n


FLOORS = {'accepted': 100, 'refused': 1, 'crlf': 3, 'chunks>1': 2, 'with_full': 2001, 'tail_only': 301, 'clipped S!=L': 51, 'mismatched': 201,
          'dup level>0': 10, 'over listed': 30, 'line>1024': 3, 'spread': 30, 'wave': 30, 'hits': 1001, '9000 beside 0 and 7': 3}


def emit_census():
    """what the slice holds for the emit, its deflate and the tolerant probes, from the references alone; the emit at the configured
    minreadlength (``emit_min=None``), the probes at the drawn ``per``"""
    n = collections.Counter()
    for seed, seeded in slice_():
        c, r = case(seed, seeded), refs(seed, seeded)
        n['emit_min %r' % (c.emit_min,)] += 1; n['per %d' % c.per] += 1
        if not r.accepted:
            n['refused'] += 1
            continue
        text, amin, m = c.text, ord(c.cfg['Amin']), c.cfg['minreadlength']
        for r0, n0, n1, n2, n3, cls, start, length in E.per_record(text, r.co, amin, m):
            n[cls] += 1
            if cls != 'mismatched':
                n['scores 256 .. 1023'] += 256 <= n3 - n2 - 1 < 1024; n['scores >= 1024'] += n3 - n2 - 1 >= 1024
            if cls == 'emitted':
                n['start > 0'] += start > 0; n['cut behind'] += start + length < n1 - n0 - 1
                n['name with \\r'] += text[r0:n0].endswith(b'\r'); n['third line with text'] += len(text[n1 + 1:n2].rstrip(b'\r')) > 1
                n['emitted length >= 1024'] += length >= 1024
        want = r.emit_of(text, r.co, m)[0]
        n['text without final newline'] += not text.endswith(b'\n')
        # the deflate: of the text the legs deflate, the emit at the DRAWN emit_min (the figures at the configured minreadlength beside it)
        drawn = r.emit_of(text, r.co)[0]
        n['emitted text > 65 280 bytes'] += len(drawn) > D.BLOCK; n['emitted text > 65 280 bytes at minreadlength'] += len(want) > D.BLOCK
        ms = D.members(twin(drawn)[0])
        n['members'] += len(ms); n['members stored'] += sum((m_[2][0] >> 1) & 3 == 0 for m_ in ms)
        n['members at minreadlength'] += (len(want) + D.BLOCK - 1) // D.BLOCK
        # the tolerant probes against the exact ones: the array less the words only the tolerant rule writes, the mask, the records
        exact = r.passes.adapt
        mm = r.tolerant.copy()
        mm[AM.PER] = 0
        for k in range(len(c.probes)):
            mm[A.BLOCKS + k * A.BLOCK_WORDS + AM.B_DIST:A.BLOCKS + k * A.BLOCK_WORDS + AM.B_DIST + 4] = 0
        n['adapters differ'] += bool((mm != exact).any())
        n['FIRST at distance >= 1: records'] += sum(1 for rec in AM.per_record(text, r.co, list(c.probes), c.per) if any(dist for dist in rec[6]))
        n['FIRST at distance >= 1: pairs'] += tolerant_firsts(r.tolerant)
        if r.masked is not None:
            n['mask differs'] += r.masked_mm != r.masked
            n['the clip changes the emit'] += r.emit_of(r.masked_mm, r.co, m)[0] != want
    return n


EMIT_FLOORS = {'emitted': 20000, 'short': 30000, 'mismatched': 8000, 'start > 0': 4000, 'cut behind': 4000, 'name with \\r': 300, 'third line with text': 5000,
               'emitted length >= 1024': 50, 'scores 256 .. 1023': 2000, 'scores >= 1024': 150, 'text without final newline': 5,
               'emitted text > 65 280 bytes': 20, 'the clip changes the emit': 70}
# three quarters of what the slice holds (profiles/fuzz_emit_tests.txt); the first two are to be a quarter of the accepted cases at least
TOLERANT_FLOORS = {'adapters differ': 48, 'mask differs': 45, 'FIRST at distance >= 1: records': 850}       # (of 65, 61 and 1134)


# ---- the checks on the GPU -------------------------------------------------------------------------------------------------------

def every_option(c):
    return dict(records=True, profile=list(c.cuts), cycles=True, per_read=True, duplication=True, overrepresented=True, adapters=list(c.probes))


def _write(d, name, data):
    p = os.path.join(str(d), name)
    with open(p, 'wb') as f:
        f.write(data)
    return p


def _same_stats(got, want, what):
    assert tuple(got['hits']) == tuple(want['hits']) and [bytes(h) for h in got['hitseqs']] == [bytes(h) for h in want['hitseqs']], what
    for k in STAT_KEYS:
        assert got['stats'][k] == want['stats'][k], (what, k)


def same_outcome(g, want, what):
    """``F.outcome`` of a call on a compressed file or a BAM against the oracle's on the text: the kind, the message of a refusal, the
    hits, their bytes and every statistic but parsed and total, which count the file's bytes"""
    assert g[0] == want[0], (what, g[:2] if g[0] == 'format' else g[0], want[:2] if want[0] == 'format' else want[0])
    if g[0] == 'format':
        assert g[1] == want[1], (what, g[1], want[1])
    else:
        assert g[1] == want[1] and g[2] == want[2], what + ': hits'
        for k in STAT_KEYS:
            assert g[3][k] == want[3][k], (what, k)


def leg_everything(c, r, d, tally):
    """every pass on one call of findseqs, and the kept scan object without them"""
    from kvarq_amd import engine
    p = _write(d, 'c%d.fastq' % c.seed, c.text)
    engine.config(**c.cfg)
    got = {}
    g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), **every_option(c))) or got)
    assert g == r.outcome, 'every pass on: outcome'
    tally['formats'] += g[0] == 'format'
    if g[0] != 'ok':
        return
    tally['hits'] += len(g[1])
    same_passes(got['profile'], r.passes, 'every pass on:')
    assert len(got['records']) == len(got['hits'])
    for h, rec in zip(got['hits'], got['records']):
        assert bytes(rec) == r.record_of(c.text, h.file_pos), 'the record of %r' % (h,)
    none = engine.findseqs(p, list(c.seqs))
    assert 'profile' not in none and 'records' not in none and F.outcome(lambda: none) == r.outcome, 'the kept scan object'


def leg_clip(c, r, d, tally):
    from kvarq_amd import engine
    p = _write(d, 'c%d.fastq' % c.seed, c.text)
    engine.config(**c.cfg)
    if ord(c.cfg['Amin']) <= ord('!'):
        try:
            engine.findseqs(p, list(c.seqs), clip=list(c.probes))
        except RuntimeError as e:
            assert "not above '!'" in str(e)
            tally['clip refused'] += 1
            return
        raise AssertionError("clip= at an Amin of '!' was not refused")
    if not r.accepted:
        g = F.outcome(lambda: engine.findseqs(p, list(c.seqs), clip=list(c.probes)))
        assert g == r.outcome, 'clip: outcome of a refused case'
        tally['formats'] += 1
        return
    got = engine.findseqs(p, list(c.seqs), clip=list(c.probes))
    assert F.outcome(lambda: got) == r.masked_outcome, 'clip: outcome'
    assert (got['clip'].words == r.clip_words).all(), ('clip: words', got['clip'].words, r.clip_words)
    tally['hits'] += len(got['hits']); tally['clipped'] += got['clip'].clipped
    got = engine.findseqs(p, list(c.seqs), clip=list(c.probes), profile=list(c.cuts), adapters=list(c.probes), cycles=True, per_read=True, duplication=True,
                          overrepresented=True)
    assert F.outcome(lambda: got) == r.masked_outcome and (got['clip'].words == r.clip_words).all(), 'clip beside the profile'
    same_passes(got['profile'], r.masked_passes, 'the profile of the masked text:')


def bam_records(c, r, bam_limit=SMALL):
    """the BAM records of an accepted case, or None where bam_writer.from_fastq does not give the records of the text: a text that
    ends in a cut record, which the writer reads by lines"""
    import bam_writer as W
    if not r.accepted or len(c.text) > bam_limit:
        return None
    records = W.from_fastq(c.text)
    return records if records and len(records) == len(r.recs) else None


def leg_routes(c, r, d, tally, bam_limit=SMALL):
    """the same text as BGZF, as plain gzip and, where bam_writer takes it, as BAM"""
    import bam_writer as W
    from kvarq_amd import bam, engine
    from test_host_logic import bgzf
    engine.config(**c.cfg)
    for name, data, inflate, route in (('b%d.fastq.gz' % c.seed, bgzf(c.text), 'device', 'device'),
                                       ('g%d.fastq.gz' % c.seed, gzip.compress(c.text, 6), 'device_any', 'device_gzip')):
        p = _write(d, name, data)
        got = {}
        g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), inflate=inflate, **every_option(c))) or got)
        same_outcome(g, r.outcome, route)
        assert engine.last_inflate() == route, (route, engine.last_inflate())
        tally[route] += 1; tally[route + ' formats'] += g[0] == 'format'
        if g[0] == 'ok':
            tally['hits'] += len(g[1])
            same_passes(got['profile'], r.passes, '%s:' % route)
        os.unlink(p)
    records = bam_records(c, r, bam_limit)
    if records is None:
        return
    data = W.write(os.path.join(str(d), 'm%d.bam' % c.seed), W.header(), records)
    vtext = bytes(bam.to_fastq_host(data))
    vo = oracle_outcome(vtext, c.seqs, c.cfg)
    got = {}
    g = F.outcome(lambda: got.update(engine.findseqs(os.path.join(str(d), 'm%d.bam' % c.seed), list(c.seqs), **every_option(c))) or got)
    assert engine.last_inflate() == 'device_bam'
    same_outcome(g, vo, 'device_bam')
    tally['device_bam'] += 1
    if g[0] == 'ok':
        tally['hits of the BAM'] += len(g[1])
        same_passes(got['profile'], Passes(c, vtext, O.chunk_offsets(vtext)), 'device_bam:')
    os.unlink(os.path.join(str(d), 'm%d.bam' % c.seed))


def table_is_seeded(c):
    """whether the table of the case's sequences has a seed index, without which ``long_reads`` changes nothing (needs a GPU)"""
    from kvarq_amd import scan
    t = scan.Table(list(c.seqs), **c.cfg)
    try:
        return any(t.seeded)
    finally:
        t.close()


def leg_long_reads(c, r, d, tally):
    from kvarq_amd import engine
    p = _write(d, 'c%d.fastq' % c.seed, c.text)
    engine.config(**c.cfg)
    got = {}
    g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), long_reads=True, **every_option(c))) or got)
    assert g == r.outcome, 'long_reads: outcome'
    tally['formats'] += g[0] == 'format'
    if g[0] != 'ok':
        return
    assert engine.last_long_reads() is table_is_seeded(c), 'long_reads: the route ran: %r' % (engine.last_long_reads(),)
    tally['read list'] += engine.last_long_reads()
    tally['hits'] += len(g[1])
    same_passes(got['profile'], r.passes, 'long_reads:')
    for h, rec in zip(got['hits'], got['records']):
        assert bytes(rec) == r.record_of(c.text, h.file_pos), 'long_reads: the record of %r' % (h,)


def scanner_cuts(c, r):
    """(the chunk offsets of the device batch: the oracle's and 1 to 6 record starts; where the two host batches part)"""
    rnd = random.Random(c.seed ^ 0xC075)
    starts = [n3 + 1 for _, _, _, n3 in r.recs[:-1]] or [0]
    co = sorted(set(r.co) | set(rnd.choice(starts) for _ in range(rnd.randint(1, 6))))
    return co, rnd.choice(starts)


def leg_scanner(c, r, d, tally):
    """``scan.Scanner`` with every option: one device batch under chunk cuts of the test's choosing, then two host batches, and after
    a reset the other way round; against the same feeding without options, the oracle, and the plain statements under those cuts.
    In every fourth case an arena of 64 hits (KVQ_ARENA_CAP, read when a scan object is made): the replay counts every record once"""
    from kvarq_amd import scan
    if not r.accepted or len(r.recs) < 2:
        return
    text, arr = c.text, np.frombuffer(c.text, dtype=np.uint8)
    co, half = scanner_cuts(c, r)
    want_dev, want_host = Passes(c, text, co), Passes(c, text, sorted(set(r.co) | {half}))
    assert int(want_dev.words[R.RECORDS]) == int(want_host.words[R.RECORDS]) == len(r.recs)
    host_co = [[o for o in r.co if o < half] + [half], [half] + [o for o in r.co if o > half]]
    oracle = dict(hits=r.outcome[1], hitseqs=r.outcome[2], stats=r.outcome[3])
    arena = os.environ.get('KVQ_ARENA_CAP')
    if c.seed % 4 == 0:
        os.environ['KVQ_ARENA_CAP'] = '64'; tally['small arena'] += 1
    try:
        t = scan.Table(list(c.seqs), **c.cfg)
        dbuf = scan.DeviceBuffer(arr.nbytes); dbuf.upload(arr)
        plain, full = scan.Scanner(t), scan.Scanner(t, **every_option(c))
    finally:
        os.environ.pop('KVQ_ARENA_CAP', None)
        if arena is not None:
            os.environ['KVQ_ARENA_CAP'] = arena

    def device(s):
        s.scan_device(dbuf.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        return s.finish()

    def host(s):
        s.scan_host(arr[:half], chunk_off=np.array(host_co[0], dtype=np.int64))
        s.scan_host(arr[half:], chunk_off=np.array(host_co[1], dtype=np.int64) - half, fpos_base=half)
        return s.finish()
    try:
        for feed in (device, host, host, device):
            want = want_dev if feed is device else want_host
            what = 'Scanner, %s:' % ('a device batch' if feed is device else 'two host batches')
            a, b = feed(plain), feed(full)
            assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and (b['counters'] == a['counters']).all(), what
            assert 'profile' not in a and 'records' not in a
            _same_stats(b, oracle, what + ' the oracle')
            same_passes(b['profile'], want, what)
            for h, rec in zip(b['hits'], b['records']):
                assert bytes(rec) == r.record_of(text, h.file_pos), what + ' the record of %r' % (h,)
            tally['hits'] += len(b['hits']); tally['scanner'] += 1
            plain.reset(); full.reset()
    finally:
        plain.close(); full.close(); dbuf.free(); t.close()


# ---- the emit, its BGZF and the tolerant probes ----------------------------------------------------------------------------------

def _read(path):
    with open(path, 'rb') as f:
        return f.read()


def same_bytes(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        at = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        raise AssertionError('%s: %d bytes, not %d; the first difference at %d: %r, not %r' % (what, len(got), len(want), at, got[at:at + 40], want[at:at + 40]))


def same_emit(res, want, words, what):
    """the eight words of a result against the reference's, and their identities"""
    assert (res['emit'].words == words).all(), (what + ': the emit words', res['emit'].words.tolist(), words.tolist())
    E.check_identities(res['emit'].words, len(want))


def same_bgzf(got, res, want, small, what):
    """a deflated emit against the emitted text ``want``.  One batch (``small``: a text up to SMALL bytes): the twin's members and
    one EOF member, byte for byte, and the twin's words.  A text the reader cuts into batches of its own: zlib inflates the stream
    to ``want``, ``bgzf.index`` walks it, its last 28 bytes are the EOF member and no other member is empty"""
    from kvarq_amd import bgzf
    z = res['emit_compress']
    assert z['bytes_in'] == len(want) == res['emit'].bytes_out and z['bytes_out'] + 28 == len(got), (what, z['bytes_in'], z['bytes_out'], len(want), len(got))
    if small:
        same_bytes(got, bgzf_of([want]), what + ': the BGZF')
        assert z['words'].tolist() == (twin(want)[1].tolist() if want else [0] * D.LEN), (what, z['words'].tolist())
        return
    assert gzip.decompress(got) == want, what + ': the BGZF inflated'
    ms, walked = D.members(got), bgzf.index(got)
    assert walked is not None and walked[0].tolist() == [m[0] for m in ms] and walked[2].tolist() == [m[4] for m in ms], what
    assert got[-28:] == D.EOF and ms[-1][4] == 0 and all(m[4] > 0 and m[1] <= 65536 for m in ms[:-1]) and z['members'] == len(ms) - 1, what


def leg_emit(c, r, d, tally):
    """``findseqs`` with ``emit=`` beside every pass: the written file against the plain statement of the emit, under the drawn
    ``emit_min``; beside the tolerant clip; deflated; and on the read-list route"""
    from kvarq_amd import engine
    p, out = _write(d, 'c%d.fastq' % c.seed, c.text), os.path.join(str(d), 'e%d.fastq' % c.seed)
    engine.config(**c.cfg)
    got = {}
    g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), emit=out, emit_min=c.emit_min, **every_option(c))) or got)
    assert g == r.outcome, 'emit: outcome'
    tally['formats'] += g[0] == 'format'
    if g[0] != 'ok':
        return                                                 # (what a refused call has written is unspecified: DESIGN section 21)
    want, words = r.emit_of(c.text, r.co)
    same_passes(got['profile'], r.passes, 'emit beside every pass:')
    same_bytes(_read(out), want, 'emit: the file')
    same_emit(got, want, words, 'emit')
    assert 'emitted' not in got and 'emit_compress' not in got
    assert len(got['records']) == len(got['hits'])
    tally['hits'] += len(g[1]); tally['emitted'] += int(words[E.EMITTED]); tally['emitted bytes'] += len(want)
    if ord(c.cfg['Amin']) > ord('!'):
        got = engine.findseqs(p, list(c.seqs), emit=out, emit_min=c.emit_min, clip=list(c.probes), adapter_mismatches=c.per, **every_option(c))
        assert F.outcome(lambda: got) == r.masked_mm_outcome, 'emit beside the tolerant clip: outcome'
        assert (got['clip'].words == r.clip_words_mm).all(), ('emit beside the tolerant clip: clip words', got['clip'].words, r.clip_words_mm)
        cwant, cwords = r.emit_of(r.masked_mm, r.co)
        same_bytes(_read(out), cwant, 'emit beside the tolerant clip: the file')
        same_emit(got, cwant, cwords, 'emit beside the tolerant clip')
        same_passes(got['profile'], r.masked_mm_passes, 'emit beside the tolerant clip:')
        tally['clip legs'] += 1; tally['clipped'] += int(r.clip_words_mm[AM.C_CLIPPED])
    got = engine.findseqs(p, list(c.seqs), emit=out, emit_min=c.emit_min, emit_compress=True, **every_option(c))
    assert F.outcome(lambda: got) == r.outcome, 'emit_compress: outcome'
    same_emit(got, want, words, 'emit_compress')
    same_bgzf(_read(out), got, want, len(c.text) <= SMALL, 'emit_compress')
    same_passes(got['profile'], r.passes, 'emit_compress beside every pass:')
    tally['compressed'] += 1
    if c.seeded:
        got = engine.findseqs(p, list(c.seqs), emit=out, emit_min=c.emit_min, long_reads=True)
        assert F.outcome(lambda: got) == r.outcome, 'emit with long_reads: outcome'
        assert engine.last_long_reads() is table_is_seeded(c), 'emit with long_reads: the route ran: %r' % (engine.last_long_reads(),)
        same_bytes(_read(out), want, 'emit with long_reads: the file')
        same_emit(got, want, words, 'emit with long_reads')
        tally['long_reads'] += 1; tally['read list'] += engine.last_long_reads()


def leg_emit_routes(c, r, d, tally):
    """the emit on text that came from the device walk: the same text as BGZF, as plain gzip and, where bam_writer takes it, as BAM
    (its virtual text); deflated on odd seeds; and the round trip: the BGZF the emit wrote goes back in on the device-inflate
    route and gives the oracle's outcome on the emitted text"""
    from kvarq_amd import engine
    from test_host_logic import bgzf
    engine.config(**c.cfg)
    z = c.seed % 2 == 1
    out = os.path.join(str(d), 'e%d.fastq.gz' % c.seed)      # (the suffix decides nothing for the emit; for the round trip the input's route goes by its name)
    inputs = [('b%d.fastq.gz' % c.seed, lambda: bgzf(c.text), dict(inflate='device'), 'device', c.text, r.outcome, r.co),
              ('g%d.fastq.gz' % c.seed, lambda: gzip.compress(c.text, 6), dict(inflate='device_any'), 'device_gzip', c.text, r.outcome, r.co)]
    if r.virtual is not None:
        bam_file, vtext, vo, vco = r.virtual
        inputs.append(('m%d.bam' % c.seed, lambda: bam_file, {}, 'device_bam', vtext, vo, vco))
    for name, make, kw, route, text, outcome, co in inputs:
        p = _write(d, name, make())
        got = {}
        g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), emit=out, emit_min=c.emit_min, emit_compress=z, **dict(every_option(c), **kw))) or got)
        os.unlink(p)
        same_outcome(g, outcome, 'emit, ' + route)
        assert engine.last_inflate() == route, (route, engine.last_inflate())
        tally[route] += 1; tally[route + ' formats'] += g[0] == 'format'
        if g[0] != 'ok':
            continue
        tally['hits' if route != 'device_bam' else 'hits of the BAM'] += len(g[1])
        want, words = r.emit_of(text, co)
        same_emit(got, want, words, 'emit, ' + route)
        if z:
            same_bgzf(_read(out), got, want, len(text) <= SMALL, 'emit, ' + route)
            tally['compressed'] += 1
        else:
            same_bytes(_read(out), want, 'emit, %s: the file' % route)
            assert 'emit_compress' not in got
        if route != 'device_bam':
            same_passes(got['profile'], r.passes, 'emit, %s:' % route)
        if route == 'device' and c.seed % 4 == 1 and want:
            back = F.outcome(lambda: engine.findseqs(out, list(c.seqs), inflate='device'))
            assert engine.last_inflate() == 'device', engine.last_inflate()
            same_outcome(back, r.outcome_of(want), 'the round trip')
            tally['round trips'] += 1; tally['round trip hits'] += len(back[1]) if back[0] == 'ok' else 0


def leg_emit_scanner(c, r, d, tally):
    """``leg_scanner`` with the emit on: a device batch under ``scanner_cuts``' chunk cuts, two host batches, and after a reset the
    other way round, the second and the fourth feeding deflated (a scan object is plain or deflating for its life: two of them,
    each fed both ways round a reset); in every fourth case an arena of 64 hits, whose replay emits once.  In the case that
    leads its group the first member of the deflated device feeding is held to ``deflate_ref.parse``, token for token"""
    from kvarq_amd import _lib, scan
    if not r.accepted or len(r.recs) < 2:
        return
    text, arr = c.text, np.frombuffer(c.text, dtype=np.uint8)
    co, half = scanner_cuts(c, r)
    host_co = [[o for o in r.co if o < half] + [half], [half] + [o for o in r.co if o > half]]
    want_passes = {'device': r.under(co), 'host': r.under(sorted(set(r.co) | {half}))}
    want_emit = {'device': r.emit_batches(text, [(0, len(text), co)]), 'host': r.emit_batches(text, [(0, half, host_co[0]), (half, len(text), host_co[1])])}
    oracle = dict(hits=r.outcome[1], hitseqs=r.outcome[2], stats=r.outcome[3])
    arena = os.environ.get('KVQ_ARENA_CAP')
    if c.seed % 4 == 0:
        os.environ['KVQ_ARENA_CAP'] = '64'; tally['small arena'] += 1
    try:
        t = scan.Table(list(c.seqs), **c.cfg)
        dbuf = scan.DeviceBuffer(arr.nbytes); dbuf.upload(arr)
        plain = scan.Scanner(t)
        full = [scan.Scanner(t, emit=True, emit_min=c.emit_min, **every_option(c)), scan.Scanner(t, emit=True, emit_min=c.emit_min, emit_compress=True, **every_option(c))]
    finally:
        os.environ.pop('KVQ_ARENA_CAP', None)
        if arena is not None:
            os.environ['KVQ_ARENA_CAP'] = arena

    def device(s):
        s.scan_device(dbuf.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        return s.finish()

    def host(s):
        s.scan_host(arr[:half], chunk_off=np.array(host_co[0], dtype=np.int64))
        s.scan_host(arr[half:], chunk_off=np.array(host_co[1], dtype=np.int64) - half, fpos_base=half)
        return s.finish()
    try:
        for i, feed in enumerate((device, host, host, device)):
            how = 'device' if feed is device else 'host'
            what = 'Scanner with the emit, %s%s:' % ('a device batch' if feed is device else 'two host batches', ', deflated' if i % 2 else '')
            s = full[i % 2]
            a, b = feed(plain), feed(s)
            assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and (b['counters'] == a['counters']).all(), what
            _same_stats(b, oracle, what + ' the oracle')
            same_passes(b['profile'], want_passes[how], what)
            parts, words = want_emit[how]
            whole = b''.join(parts)
            same_emit(b, whole, words, what)
            assert b['emit'].records == len(r.recs) == int(b['counters'][_lib.CTR_RECORDS]), (what, b['emit'].records, len(r.recs))
            assert _lib.lib().kvq_scan_emit_guard(s.h) == 0, what + ' the guards of the store'
            got = b['emitted'].tobytes()
            if i % 2:
                same_bytes(got, bgzf_of(parts), what + ' the BGZF')
                assert got.count(D.EOF) >= 1 and got[-28:] == D.EOF and gzip.decompress(got) == whole, what
                tw = [twin(x)[1] for x in parts if x]
                zw = b['emit_compress']['words'].tolist()
                assert zw == ((np.sum(tw, axis=0)[:6].tolist() + np.max(tw, axis=0)[6:].tolist()) if tw else [0] * D.LEN), (what, zw)
                tally['compressed feedings'] += 1
                if feed is device and leads_its_group(c) and whole:
                    first = D.members(got)[0]
                    toks = D.tokens(first[2])
                    if toks['btype'] == 2:
                        assert toks['tokens'] == D.parse(whole[:D.BLOCK]), what + ' the tokens of the first member are not those of the parse as stated'
                        tally['parsed'] += 1
            else:
                same_bytes(got, whole, what + ' the emitted text')
                assert 'emit_compress' not in b
            tally['hits'] += len(b['hits']); tally['scanner'] += 1; tally['emitted'] += int(words[E.EMITTED])
            plain.reset(); s.reset()
    finally:
        plain.close(); full[0].close(); full[1].close(); dbuf.free(); t.close()


def tolerant_firsts(w):
    """the (record, probe) pairs of an adapters array whose FIRST lies at a distance of 1 or more"""
    return int(sum(w[A.BLOCKS + k * A.BLOCK_WORDS + AM.B_DIST + 1:A.BLOCKS + k * A.BLOCK_WORDS + AM.B_DIST + 4].sum() for k in range(int(w[A.A_N]))))


def leg_tolerant(c, r, d, tally):
    """``adapter_mismatches=per`` against the Hamming loop of ``adapt_mm_ref``: the adapter content beside the other passes, the
    clip beside the profile (the oracle and the plain statements on the tolerantly masked text), and a ``Scanner`` device batch
    under chunk cuts of the test's choosing"""
    from kvarq_amd import engine, scan
    p = _write(d, 'c%d.fastq' % c.seed, c.text)
    engine.config(**c.cfg)
    opts = dict(profile=list(c.cuts), cycles=True, per_read=True, duplication=True, overrepresented=True, adapters=list(c.probes), adapter_mismatches=c.per)
    got = {}
    g = F.outcome(lambda: got.update(engine.findseqs(p, list(c.seqs), **opts)) or got)
    assert g == r.outcome, 'tolerant: outcome'
    tally['formats'] += g[0] == 'format'
    if g[0] != 'ok':
        return
    same_passes(got['profile'], r.passes_mm, 'tolerant (1 per %d):' % c.per)
    assert got['profile'].adapters.words[AM.PER] == c.per
    tally['hits'] += len(g[1]); tally['tolerant hits'] += tolerant_firsts(r.tolerant)
    if ord(c.cfg['Amin']) > ord('!'):
        got = engine.findseqs(p, list(c.seqs), clip=list(c.probes), **opts)
        assert F.outcome(lambda: got) == r.masked_mm_outcome, 'the tolerant clip beside the profile: outcome'
        assert (got['clip'].words == r.clip_words_mm).all(), ('the tolerant clip: words', got['clip'].words, r.clip_words_mm)
        same_passes(got['profile'], r.masked_mm_passes, 'the profile of the tolerantly masked text:')
        tally['clip legs'] += 1; tally['clipped'] += int(r.clip_words_mm[AM.C_CLIPPED])
    if len(r.recs) < 2:
        return
    arr = np.frombuffer(c.text, dtype=np.uint8)
    co, _ = scanner_cuts(c, r)
    t = scan.Table(list(c.seqs), **c.cfg)
    dbuf = scan.DeviceBuffer(arr.nbytes); dbuf.upload(arr)
    s = scan.Scanner(t, **opts)
    try:
        s.scan_device(dbuf.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        b = s.finish()
        _same_stats(b, dict(hits=r.outcome[1], hitseqs=r.outcome[2], stats=r.outcome[3]), 'Scanner, tolerant: the oracle')
        same_passes(b['profile'], r.under(co, c.per), 'Scanner, tolerant (1 per %d):' % c.per)
        tally['scanner'] += 1
    finally:
        s.close(); dbuf.free(); t.close()


def scanner_batches(c, r):
    """the feedings of ``leg_emit_scanner``: ([the device batch], [the two host batches]), each (first byte, end, chunk offsets)"""
    co, half = scanner_cuts(c, r)
    return ([(0, len(c.text), co)],
            [(0, half, [o for o in r.co if o < half] + [half]), (half, len(c.text), [half] + [o for o in r.co if o > half])])


def deflated_batches(c, r):
    """every emitted text of an accepted case that a leg compares in its deflated form, each once"""
    texts = [r.emit_of(c.text, r.co)[0]]
    if c.seed % 2 and r.virtual is not None and r.virtual[2][0] == 'ok':
        texts.append(r.emit_of(r.virtual[1], r.virtual[3])[0])
    if len(r.recs) >= 2:
        for feeding in scanner_batches(c, r):
            texts += r.emit_batches(c.text, feeding)[0]
    return sorted(set(t for t in texts if t))


LEGS = (('everything', leg_everything), ('clip', leg_clip), ('routes', leg_routes), ('long_reads', leg_long_reads), ('scanner', leg_scanner),
        ('emit', leg_emit), ('emit_routes', leg_emit_routes), ('emit_scanner', leg_emit_scanner), ('tolerant', leg_tolerant))
NEW_LEGS = ('emit', 'emit_routes', 'emit_scanner', 'tolerant')


def expected(leg, cases):
    """what a leg's tally must hold once it has run over the cases [(seed, seeded)], from the references alone: a leg that left a case,
    a refusal or a route out does not end with these figures.  ('read list' and 'hits of the BAM' are not among them: the first
    takes the library's table, the second the library's virtual text; ``leg_long_reads`` and ``leg_routes`` assert them case by case)"""
    n = collections.Counter()
    for seed, seeded in cases:
        c, r = case(seed, seeded), refs(seed, seeded)
        hits = len(r.outcome[1]) if r.accepted else 0
        if leg == 'everything' or leg == 'long_reads' and seeded:
            n['formats'] += not r.accepted; n['hits'] += hits
        elif leg == 'clip':
            if ord(c.cfg['Amin']) <= ord('!'):
                n['clip refused'] += 1
            elif not r.accepted:
                n['formats'] += 1
            else:
                n['hits'] += len(r.masked_outcome[1]); n['clipped'] += int(r.clip_words[CR.C_CLIPPED])
        elif leg == 'routes':
            n['device'] += 1; n['device_gzip'] += 1
            n['device formats'] += not r.accepted; n['device_gzip formats'] += not r.accepted
            n['hits'] += 2 * hits; n['device_bam'] += bam_records(c, r) is not None
        elif leg == 'scanner' and r.accepted and len(r.recs) >= 2:
            n['scanner'] += 4; n['hits'] += 4 * hits; n['small arena'] += c.seed % 4 == 0
        elif leg in ('emit', 'tolerant'):
            n['formats'] += not r.accepted
            if not r.accepted:
                continue
            n['hits'] += hits
            if ord(c.cfg['Amin']) > ord('!'):
                n['clip legs'] += 1; n['clipped'] += int(r.clip_words_mm[AM.C_CLIPPED])
            if leg == 'emit':
                want, words = r.emit_of(c.text, r.co)
                n['emitted'] += int(words[E.EMITTED]); n['emitted bytes'] += len(want); n['compressed'] += 1; n['long_reads'] += seeded
            else:
                n['tolerant hits'] += tolerant_firsts(r.tolerant); n['scanner'] += len(r.recs) >= 2
        elif leg == 'emit_routes':
            n['device'] += 1; n['device_gzip'] += 1
            n['device formats'] += not r.accepted; n['device_gzip formats'] += not r.accepted
            if not r.accepted:
                continue
            want = r.emit_of(c.text, r.co)[0]
            n['hits'] += 2 * hits; n['compressed'] += 2 * (c.seed % 2)
            if r.virtual is not None:
                n['device_bam'] += 1; n['compressed'] += c.seed % 2 and r.virtual[2][0] == 'ok'
                n['device_bam formats'] += r.virtual[2][0] == 'format'
            if c.seed % 4 == 1 and want:
                back = r.outcome_of(want)
                n['round trips'] += 1; n['round trip hits'] += len(back[1]) if back[0] == 'ok' else 0
        elif leg == 'emit_scanner' and r.accepted and len(r.recs) >= 2:
            dev, hst = (r.emit_batches(c.text, feeding) for feeding in scanner_batches(c, r))
            n['scanner'] += 4; n['hits'] += 4 * hits; n['small arena'] += c.seed % 4 == 0; n['compressed feedings'] += 2
            n['emitted'] += 2 * int(dev[1][E.EMITTED]) + 2 * int(hst[1][E.EMITTED])
            n['parsed'] += bool(leads_its_group(c) and dev[0][0] and (D.members(twin(dev[0][0])[0])[0][2][0] >> 1) & 3 == 2)
    return n


# what every leg must have compared over the whole slice (tests/test_fuzz_passes_host.py asserts it of ``expected``; the GPU test
# asserts of every group that the leg's tally is the group's ``expected``)
LEG_FLOORS = {'everything': {'hits': 1001, 'formats': 1},
              'clip': {'hits': 1001, 'formats': 1, 'clip refused': 1, 'clipped': 1001},
              'routes': {'hits': 1001, 'device': 100, 'device_gzip': 100, 'device_bam': 100, 'device formats': 1, 'device_gzip formats': 1},
              'long_reads': {'hits': 1001, 'formats': 1},
              'scanner': {'hits': 1001, 'scanner': 400, 'small arena': 10},
              'emit': {'hits': 1001, 'formats': 1, 'emitted': 20000, 'clip legs': 70, 'compressed': 100, 'long_reads': 30},
              'emit_routes': {'hits': 1001, 'device': 100, 'device_gzip': 100, 'device_bam': 100, 'round trips': 15, 'compressed': 100},
              'emit_scanner': {'hits': 1001, 'scanner': 400, 'small arena': 10, 'compressed feedings': 200, 'parsed': 8},
              'tolerant': {'hits': 1001, 'formats': 1, 'tolerant hits': 1134, 'clip legs': 70, 'scanner': 100}}       # (1134: the census's records with a FIRST at distance >= 1)


# ---- a campaign by hand ----------------------------------------------------------------------------------------------------------

def main(argv):
    first, count = int(argv[1]), int(argv[2])
    seeded = len(argv) > 3 and argv[3] == 'seeded'
    bad, tally = 0, collections.Counter()
    with tempfile.TemporaryDirectory() as d:
        for seed in range(first, first + count):
            c = case(seed, seeded)
            if c is None or len(c.text) > 8 * CHUNK:
                continue
            r = refs(seed, seeded)
            saved = {k: os.environ.get(k) for k in environ(c)}
            for k, v in environ(c).items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            for name, leg in LEGS:
                if name == 'long_reads' and not seeded:
                    continue
                try:
                    leg(c, r, d, tally)
                except AssertionError as e:
                    bad += 1
                    print('MISMATCH seed=%d (%s) leg=%s: %s' % (seed, 'seeded' if seeded else 'general', name, str(e)[:300]))
                    sys.stdout.flush()
            for k, v in saved.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            refs.cache_clear(); case.cache_clear()
    print('%d seeds from %d: %d mismatches (%r)' % (count, first, bad, dict(tally)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
