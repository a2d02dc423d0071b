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
"""
import bisect
import collections
import functools
import gzip
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'tools'), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adapt_ref as A                                          # noqa: E402
import clip_ref as CR                                          # noqa: E402
import cycles_ref as CY                                        # noqa: E402
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

Case = collections.namedtuple('Case', 'seed seeded text seqs cfg probes cuts dup_slots over_records eol block_bytes')


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
    return Case(seed, seeded, block + data, tuple(seqs), cfg, tuple(probes), cuts, dup_slots, over_records, eol, len(block))


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

    def __init__(self, c, text, co):
        self.co = co = [int(v) for v in co]
        self.words = R.profile(text, list(c.cuts), co)
        self.cycles = CY.cycles(text, co)
        self.reads = RR.reads(text, co)
        self.dup = RR.dup(text, co, c.dup_slots or 0)
        self.over = OV.over(text, co, c.over_records or 0)
        self.adapt = A.adapt(text, co, list(c.probes))
        for a in (self.words, self.cycles, self.reads, self.dup, self.over, self.adapt):
            a.flags.writeable = False

    def check_identities(self, c, text):
        R.check_identities(self.words, len(c.cuts), R.long_counts(text, list(c.cuts), self.co))
        CY.check_identities(self.cycles, self.words, CY.score_facts(text, self.co))
        RR.check_identities(self.reads, self.dup, self.words)
        OV.check_identities(self.over, self.words)
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


class Refs(object):
    def __init__(self, c):
        text = c.text
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


def group(i):
    """every NGROUPS-th case of the slice from the i-th on: about 15 cases"""
    return slice_()[i::NGROUPS]


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


LEGS = (('everything', leg_everything), ('clip', leg_clip), ('routes', leg_routes), ('long_reads', leg_long_reads), ('scanner', leg_scanner))


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
    return n


# what every leg must have compared over the whole slice (tests/test_fuzz_passes_host.py asserts it of ``expected``; the GPU test
# asserts of every group that the leg's tally is the group's ``expected``)
LEG_FLOORS = {'everything': {'hits': 1001, 'formats': 1},
              'clip': {'hits': 1001, 'formats': 1, 'clip refused': 1, 'clipped': 1001},
              'routes': {'hits': 1001, 'device': 100, 'device_gzip': 100, 'device_bam': 100, 'device formats': 1, 'device_gzip formats': 1},
              'long_reads': {'hits': 1001, 'formats': 1},
              'scanner': {'hits': 1001, 'scanner': 400, 'small arena': 10}}


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
