"""
The profile of a whole input, taken on the GPU during the scan (include/kvarq_hip.h): which bytes
the score and bases lines hold, how long the reads are, and what the engine's quality trim leaves of them at a few
cutoffs -- the questions the reference answers from a sample of the file with ``kvarq show -Q q -i``
(kvarq/cli.py:201-221) and in ``Fastq.__init__``, answered here for every record.  With ``cycles=True`` it also tells
WHERE IN THE READ the bytes stand: a count per position ("cycle") and byte value of the score and of the bases lines
(``Profile.cycle_scores`` and the methods behind it).

``profile(fnames, cutoffs)`` scans files with no sequences; ``engine.findseqs(..., profile=...)``,
``scan.Scanner(..., profile=...)``, ``Fastq.profile()``, ``Bam.profile()`` and ``Analyser.scan(..., profile=...)``
take the profile along with a scan.  ``profile_host`` is the CPU twin of the kernel (the definition in running code
and test infrastructure, not a fallback).  ``python -m kvarq_amd.profile FILE [-Q q ...]`` prints the summary,
``--cycles [--cycle-step N]`` a line per cycle (or per N cycles) behind it.

With ``per_read=True`` the profile tells what the INDIVIDUAL READS look like: the histograms of the
per-read GC share, mean quality and N count (``Profile.gc_hist`` and what follows it) -- a contaminant shows as a second
GC peak that no sum over reads can show --, with ``duplication=True`` how often the reads' first 64 bases repeat
(``Profile.duplication``, ``Profile.duplicate_share()``); ``--per-read`` and ``--duplication`` print them.

With ``overrepresented=True`` it tells WHICH SEQUENCES the duplicates are: ``Profile.overrepresented``
lists every sequence (a read's first 64 bases) that makes up 0.1 % of the reads and more, with its exact count in the whole
input and a label of where it may come from (``KNOWN_SOURCES``); ``--overrepresented`` prints the list.  The candidates are
the sequences among the first 2^18 records: a sequence that first shows up behind them is not found, which in a file that is
not sorted has a probability of e^-262 at a share of 0.1 %.

With ``adapters=`` it tells HOW MUCH OF THE INPUT IS ADAPTER, AND FROM WHICH CYCLE ON: per read and probe
the first full occurrence of the probe on the bases line, else the longest prefix of the probe, 6 bases and more, that ends the
line (read-through whose adapter the read cuts off), and the histogram of the length an adapter clip would leave
(``Profile.adapters``, ``Profile.adapter_content()`` and what follows it); ``--adapters [NAME=SEQ ...]`` prints them.  Matching
is on bytes, without mismatches: 1 to 8 probes of 8 to 32 upper-case A C G T.

Out of scope: profiles across ranks, and what ``Fastq`` guesses by default.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib
from .fastq import ASCII, PhredScale, FastqFileFormatException

MAX_CUTOFFS = 8
# the layout of the flat array (include/kvarq_hip.h)
RECORDS, BASE_LINE_BYTES, SCORE_LINE_BYTES, MISMATCHED, LONGEST = 0, 1, 2, 3, 4
SCORE_BYTES, BASE_BYTES, RAW_LENGTHS, RAW_BINS, CUTOFFS, CUT_WORDS = 8, 264, 520, 1025, 1545, 1025


CYCLES = 1024                                   # KVQ_CYCLES
CYCLES_LEN = 2 * CYCLES * 256                   # kvq_cycles_len(): score[p][b] at p * 256 + b, base[p][b] behind them


# the per-read distributions and the duplication (include/kvarq_hip.h: kvq_reads_len(), kvq_dup_len())
READS_RECORDS, READS_GC_NONE, READS_MEANQ_NONE, READS_GC, READS_GC_BINS, READS_MEANQ, READS_NCOUNT, READS_LEN = 0, 1, 2, 8, 101, 109, 365, 621
DUP_HEADER = ('level', 'slots', 'keyed', 'unkeyed', 'tracked_records', 'tracked_distinct')
DUP_DISTINCT, DUP_RECORDS, DUP_BINS, DUP_LEN = 8, 24, 16, 40
DUP_BOUNDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)        # the lower bounds of the count bins


# the overrepresented sequences (include/kvarq_hip.h: kvq_over_len()): the header words, then rows {hash, count, n, w0 .. w7}
OVER_HEADER = ('records_limit', 'slots', 'keyed', 'unkeyed', 'candidates', 'counted', 'listed')
OVER_ROWS, OVER_ROW_WORDS, OVER_MAX_ROWS = 8, 11, 1000
OVER_LEN = OVER_ROWS + OVER_MAX_ROWS * OVER_ROW_WORDS

# the adapter content (include/kvarq_hip.h: kvq_adapt_len()): the header words, a block per probe, the clip histogram
ADAPT_N, ADAPT_RECORDS, ADAPT_WITH_FULL, ADAPT_TAIL_ONLY, ADAPT_BLOCKS, ADAPT_BLOCK_WORDS = 0, 1, 2, 3, 8, 1064
ADAPT_B_M, ADAPT_B_FIRST, ADAPT_B_BEYOND, ADAPT_B_TAIL, ADAPT_B_FIRST_BINS, ADAPT_B_TAIL_BINS = 0, 1, 2, 3, 8, 1032
ADAPT_MAX_PROBES, ADAPT_MIN_PROBE, ADAPT_MAX_PROBE, ADAPT_MIN_TAIL, ADAPT_POSITIONS = 8, 8, 32, 6, 1024
ADAPT_CLIP, ADAPT_CLIP_BINS = ADAPT_BLOCKS + ADAPT_MAX_PROBES * ADAPT_BLOCK_WORDS, 1025
ADAPT_LEN = ADAPT_CLIP + ADAPT_CLIP_BINS
ADAPT_PER, ADAPT_B_DIST = 4, 4                                     # (written only with adapter_mismatches: DESIGN section 20)

Overrepresented = collections.namedtuple('Overrepresented', 'sequence count share hash source')


def _poly(base):
    def probe(sequence):
        return 10 * sequence.count(base) >= 9 * len(sequence)
    return probe


# Where an overrepresented sequence may come from: label -> probe, in the order they are tried; the first that matches is the
# row's ``source``.  A probe of bytes matches when it or its reverse complement occurs in the sequence, a callable when it
# returns true for the sequence.  The adapter probes (the first twelve bases of each) were written down from memory of FastQC's
# public adapter list, not copied from it: check them against your kit before you rely on a label.  poly-X: one byte makes up
# 90 % of the sequence or more (poly-G: the tail of a two-colour instrument that reads no signal).  Replace or extend the
# mapping, or pass one as ``sources=``.
KNOWN_SOURCES = collections.OrderedDict([
    ('Illumina universal adapter', b'AGATCGGAAGAG'),
    ("Illumina small RNA 3' adapter", b'TGGAATTCTCGG'),
    ("Illumina small RNA 5' adapter", b'GATCGTCGGACT'),
    ('Nextera transposase', b'CTGTCTCTTATA'),
    ('poly-A', _poly(b'A')), ('poly-C', _poly(b'C')), ('poly-G', _poly(b'G')), ('poly-T', _poly(b'T')), ('poly-N', _poly(b'N')),
])

_COMPLEMENT = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')


def source_of(sequence, sources=None):
    """the label of the first entry of ``sources`` (None: ``KNOWN_SOURCES``) that matches ``sequence``, or None"""
    for label, probe in (KNOWN_SOURCES if sources is None else sources).items():
        if callable(probe):
            if probe(sequence):
                return label
        else:
            probe = probe.encode('latin-1') if isinstance(probe, str) else bytes(probe)
            if probe and (probe in sequence or probe.translate(_COMPLEMENT)[::-1] in sequence):
                return label
    return None


def as_adapters(adapters):
    """the probes of the adapter content as ``(names, probes)``, two lists: ``True``: the entries of ``KNOWN_SOURCES`` whose
    value is bytes, in their order; a mapping name -> bytes; or a list of bytes (named 'probe 0', 'probe 1', ...).  1 to 8
    probes of 8 to 32 bytes, every byte one of upper-case A C G T -- ValueError otherwise"""
    if adapters is True:
        adapters = collections.OrderedDict((k, v) for k, v in KNOWN_SOURCES.items() if isinstance(v, (bytes, bytearray)))
    if isinstance(adapters, (str, bytes, bytearray)):
        adapters = [adapters]
    if hasattr(adapters, 'items'):
        names, probes = [str(k) for k in adapters], list(adapters.values())
    else:
        probes = list(adapters)
        names = ['probe %d' % k for k in range(len(probes))]
    probes = [p.encode('latin-1') if isinstance(p, str) else bytes(p) for p in probes]
    if not 1 <= len(probes) <= ADAPT_MAX_PROBES:
        raise ValueError('1 to %d adapter probes' % ADAPT_MAX_PROBES)
    for p in probes:
        if not ADAPT_MIN_PROBE <= len(p) <= ADAPT_MAX_PROBE or p.strip(b'ACGT'):
            raise ValueError('an adapter probe is %d to %d bytes, every byte one of upper-case A C G T: %r' % (ADAPT_MIN_PROBE, ADAPT_MAX_PROBE, p))
    return names, probes


class Adapters(object):
    """the adapter content of a profile (kvq_scan_adapters; the definition: include/kvarq_hip.h): ``names`` and ``probes`` (bytes)
    of the n probes; ``first`` (n x 1024): the records whose first full occurrence of probe k starts at position p, ``beyond``
    (n): those where it starts at 1024 and further; ``tail`` (n x 32): the records without a full occurrence of probe k whose
    line ends with its first t bases (t >= 6, the longest such t); ``clip`` (1025): the records by the length an adapter clip
    would leave, 1024 and more in the last bin; ``records``, ``with_adapter`` (records with a full occurrence of any probe),
    ``tail_only`` (records with none but a tail match); ``words``: the flat array.  ``mismatch_per``: 0 when the probes matched
    byte for byte, else the ``per`` of ``adapter_mismatches``, and ``first_mismatches`` (n x 4): the records
    whose first occurrence of probe k differs from it in 0, 1, 2, 3 positions (all zero with ``mismatch_per`` 0)"""

    def __init__(self, words, names=None, probes=None):
        self.words = w = np.array(words, dtype=np.int64)
        assert w.shape == (ADAPT_LEN,)
        n = int(w[ADAPT_N])
        blocks = w[ADAPT_BLOCKS:ADAPT_CLIP].reshape(ADAPT_MAX_PROBES, ADAPT_BLOCK_WORDS)[:n]
        self.lengths = [int(v) for v in blocks[:, ADAPT_B_M]]
        self.names = list(names) if names is not None else ['probe %d' % k for k in range(n)]
        self.probes = [bytes(p) for p in probes] if probes is not None else [None] * n
        assert len(self.names) == n and len(self.probes) == n
        self.records, self.with_adapter, self.tail_only = int(w[ADAPT_RECORDS]), int(w[ADAPT_WITH_FULL]), int(w[ADAPT_TAIL_ONLY])
        self.found, self.beyond, self.tailed = blocks[:, ADAPT_B_FIRST], blocks[:, ADAPT_B_BEYOND], blocks[:, ADAPT_B_TAIL]
        self.first = blocks[:, ADAPT_B_FIRST_BINS:ADAPT_B_FIRST_BINS + ADAPT_POSITIONS]
        self.tail = blocks[:, ADAPT_B_TAIL_BINS:ADAPT_B_TAIL_BINS + 32]
        self.clip = w[ADAPT_CLIP:ADAPT_CLIP + ADAPT_CLIP_BINS]
        self.mismatch_per = int(w[ADAPT_PER])
        self.first_mismatches = blocks[:, ADAPT_B_DIST:ADAPT_B_DIST + 4]

    def __eq__(self, other):
        return isinstance(other, Adapters) and bool((self.words == other.words).all())

    def __ne__(self, other):
        return not self == other

    def as_dict(self):
        def bins(h):
            return {int(b): int(h[b]) for b in np.nonzero(h)[0]}
        d = {'records': self.records, 'with_adapter': self.with_adapter, 'tail_only': self.tail_only, 'clip': bins(self.clip),
             'probes': [{'name': self.names[k], 'sequence': self.probes[k].decode('latin-1') if self.probes[k] is not None else None,
                         'length': self.lengths[k], 'found': int(self.found[k]), 'beyond': int(self.beyond[k]), 'tailed': int(self.tailed[k]),
                         'first': bins(self.first[k]), 'tail': bins(self.tail[k])} for k in range(len(self.names))]}
        if self.mismatch_per:
            d['mismatch_per'] = self.mismatch_per
            for k, probe in enumerate(d['probes']):
                probe['first_mismatches'] = [int(v) for v in self.first_mismatches[k]]
        return d


def profile_len(ncut):
    return CUTOFFS + ncut * CUT_WORDS


def as_cutoffs(cutoffs, amin=None):
    """an iterable of cutoffs (characters, bytes or ints) as a list of byte values; ``True``: the configured Amin alone"""
    if cutoffs is True:
        if amin is None:
            from . import engine
            amin = engine.get_config()['Amin']
        cutoffs = [amin]
    if isinstance(cutoffs, (str, bytes, bytearray)):
        cutoffs = list(cutoffs)
    out = []
    for c in cutoffs:
        if isinstance(c, str):
            c = c.encode('latin-1')
        if isinstance(c, (bytes, bytearray)):
            if len(c) != 1:
                raise TypeError('a cutoff must be a single character')
            c = c[0]
        c = int(c)
        if not -128 <= c <= 255:
            raise ValueError('a cutoff must be a byte value')
        out.append(c & 0xFF)
    if len(out) > MAX_CUTOFFS:
        raise ValueError('at most %d cutoffs' % MAX_CUTOFFS)
    return out


def _cut_array(cutoffs):
    return (C.c_uint8 * MAX_CUTOFFS)(*cutoffs)


def _share(part, total):
    """part / total, nan where total is 0"""
    out = np.full(np.shape(part), np.nan)
    np.divide(part, total, out=out, where=np.asarray(total) > 0)
    return out


def _without_cr(rows):
    n = rows.copy()
    n[:, 13] = 0
    return n


def _rows_mean_quality(rows, dQ):
    n = _without_cr(rows)
    return _share((n * (np.arange(256) - 33 - dQ)).sum(axis=1), n.sum(axis=1))


def _rows_quantile(rows, q, dQ):
    if not 0.0 <= q <= 1.0:
        raise ValueError('a quantile lies in 0 .. 1')
    cum = np.cumsum(_without_cr(rows), axis=1)
    total = cum[:, -1]
    byte = (cum >= np.maximum(q * total, 1)[:, None]).argmax(axis=1)          # (at least one score: q = 0 is the lowest score seen)
    return np.where(total > 0, byte - 33.0 - dQ, np.nan)


def _rows_quantile_raw(rows, q, dQ):
    """``_rows_quantile`` over rows in which byte 13 is a value like the others (a mean, not a '\\r')"""
    if not 0.0 <= q <= 1.0:
        raise ValueError('a quantile lies in 0 .. 1')
    cum = np.cumsum(rows, axis=1)
    total = cum[:, -1]
    byte = (cum >= np.maximum(q * total, 1)[:, None]).argmax(axis=1)
    return np.where(total > 0, byte - 33.0 - dQ, np.nan)


def _rows_base_share(rows):
    acgtn = rows[:, [ord(c) for c in 'ACGTN']]
    total = rows.sum(axis=1)
    return _share(np.concatenate([acgtn, (total - acgtn.sum(axis=1))[:, None]], axis=1), total[:, None])


class Profile(object):
    """a finished profile: ``records``, ``score_bytes`` / ``base_bytes`` (256 counts each), ``raw_lengths`` (1025 bins,
    the last one holding the lines of 1024 bytes and more), ``mismatched`` (records whose score and bases lines differ
    in length), ``longest`` (the longest bases line, -1: none), ``cutoffs`` (byte values), ``words`` (the flat array);
    ``cycles``: the flat per-cycle array (kvq_cycles_len() words) when the scan took it, else None;
    ``reads``: the flat array of the per-read distributions (kvq_reads_len() words) when the scan took it, else None --
    ``gc_hist`` (101 bins: the reads by their GC share in per cent), ``gc_none`` (reads without A C G T),
    ``mean_quality_hist`` (256 bins: the reads by their mean score BYTE), ``n_hist`` (256 bins: the reads by their N
    count, 255 and more in the last);
    ``duplication``: a dict of the header words of kvq_scan_dup (``DUP_HEADER``) and its two rows of 16 bins,
    'distinct' and 'records' (``DUP_BOUNDS``: their lower bounds), or None;
    ``over``: the flat array of kvq_scan_over (kvq_over_len() words) when the scan took it, else None -- ``over_info``: its
    header words by name (``OVER_HEADER``), ``overrepresented``: its rows in their canonical order (count descending, ties by
    hash ascending) as named tuples ``(sequence: bytes, count, share = count / keyed, hash, source)``, ``source`` the label
    of ``source_of`` under ``sources`` (None: ``KNOWN_SOURCES``);
    ``adapters``: the adapter content (``Adapters``: ``names``, ``probes``, ``first``, ``tail``, ``beyond``, ``clip``, ``records``,
    ``with_adapter``, ``tail_only``) when the scan took it, else None"""

    def __init__(self, words, cutoffs, cycles=None, reads=None, dup=None, over=None, sources=None, adapters=None):
        self.cutoffs = list(cutoffs)
        self.adapters = adapters
        self.clipped = None                     # the ``Clip`` of a scan with ``clip=`` (set by ``profile`` and ``profile_host``)
        self.emitted = None                     # the ``Emit`` of a scan with ``emit=`` (set by ``profile``)
        self.emit_compressed = None             # what the emit's deflate did, with ``emit_compress=True`` (set by ``profile``)
        self.over = self.over_info = self.overrepresented = None
        if over is not None:
            self.over = np.array(over, dtype=np.int64)
            assert self.over.shape == (OVER_LEN,)
            self.over_info = dict(zip(OVER_HEADER, (int(v) for v in self.over[:len(OVER_HEADER)])))
            self.relabel(sources)
        self.reads = self.duplication = None
        if reads is not None:
            self.reads = np.array(reads, dtype=np.int64)
            assert self.reads.shape == (READS_LEN,)
        if dup is not None:
            dup = np.array(dup, dtype=np.int64)
            assert dup.shape == (DUP_LEN,)
            self.duplication = dict(zip(DUP_HEADER, (int(v) for v in dup[:len(DUP_HEADER)])))
            self.duplication['distinct'] = [int(v) for v in dup[DUP_DISTINCT:DUP_DISTINCT + DUP_BINS]]
            self.duplication['records'] = [int(v) for v in dup[DUP_RECORDS:DUP_RECORDS + DUP_BINS]]
        self.cycles = None
        if cycles is not None:
            self.cycles = np.array(cycles, dtype=np.int64)
            assert self.cycles.shape == (CYCLES_LEN,)
        self.words = np.array(words, dtype=np.int64)
        assert self.words.shape == (profile_len(len(self.cutoffs)),)
        w = self.words
        self.records, self.base_line_bytes, self.score_line_bytes = int(w[RECORDS]), int(w[BASE_LINE_BYTES]), int(w[SCORE_LINE_BYTES])
        self.mismatched, self.longest = int(w[MISMATCHED]), int(w[LONGEST]) - 1
        self.score_bytes = w[SCORE_BYTES:SCORE_BYTES + 256]
        self.base_bytes = w[BASE_BYTES:BASE_BYTES + 256]
        self.raw_lengths = w[RAW_LENGTHS:RAW_LENGTHS + RAW_BINS]

    def __eq__(self, other):
        if not (isinstance(other, Profile) and self.cutoffs == other.cutoffs and (self.words == other.words).all()):
            return False
        if self.duplication != other.duplication or self.over_info != other.over_info:
            return False
        if (self.adapters is None) != (other.adapters is None) or (self.adapters is not None and self.adapters != other.adapters):
            return False
        if self.over is not None and [r[:4] for r in self.overrepresented] != [r[:4] for r in other.overrepresented]:
            return False                                  # (the labels are the host's reading of the rows, not a part of them)
        for a, b in ((self.reads, other.reads), (self.cycles, other.cycles)):
            if (a is None) != (b is None) or (a is not None and not (a == b).all()):
                return False
        return True

    def __ne__(self, other):
        return not self == other

    def _cut(self, cutoff):
        c = as_cutoffs([cutoff])[0]
        if c not in self.cutoffs:
            raise KeyError('no such cutoff in this profile: %r' % (cutoff,))
        at = CUTOFFS + self.cutoffs.index(c) * CUT_WORDS
        return int(self.words[at]) - 1, self.words[at + 1:at + CUT_WORDS]

    def readlengths(self, cutoff):
        """the quality-trimmed read lengths at ``cutoff`` in the shape of ``stats['readlengths']``: what a scan with
        ``Amin = cutoff`` reports (reads of 1024 and more in no bin, but in the tuple's length)"""
        longest, bins = self._cut(cutoff)
        return tuple(int(bins[i]) if i < _lib.MAX_READLENGTH else 0 for i in range(longest + 1))

    def score_range(self):
        """the lowest and the highest score character as indices into ``ASCII`` -- what
        ``Fastq.min_max_score_check_file`` returns, from every record (a '\\r' at the end of a line is no score);
        (999, -999) when there is none"""
        seen = [b for b in np.nonzero(self.score_bytes)[0].tolist() if b != 13]
        return (seen[0] - 33, seen[-1] - 33) if seen else (999, -999)

    def variants(self):
        """the vendor scales that hold every score of the input (``PhredScale.holding``)"""
        return PhredScale.holding(*self.score_range())

    def dQ(self):
        """the PHRED offset as ``Fastq`` states it (the offset of Q = 0 in ``ASCII``), by ``Fastq._scale``'s rules:
        FastqFileFormatException when no scale fits or the fitting ones disagree (Sanger / Illumina 1.3+)"""
        fitting = self.variants()
        offsets = {PhredScale.offset(name) for name in fitting}
        if not offsets:
            raise FastqFileFormatException('could not find any suitable fastq vendor variant')
        if len(offsets) > 1:
            raise FastqFileFormatException('cannot determine dQ with guessed vendor variants "%s"' % fitting)
        return offsets.pop()

    def mean_quality(self, dQ=None):
        """the mean PHRED score over every score character ('\\r' left out); ``dQ`` None: :meth:`dQ`"""
        dQ = self.dQ() if dQ is None else dQ
        n = self.score_bytes.copy(); n[13] = 0
        total = int(n.sum())
        return float((n * (np.arange(256) - 33 - dQ)).sum()) / total if total else float('nan')

    def kept(self, cutoff, minreadlength):
        """the share of records whose trimmed read the length gate lets through (workhorse.c:1100)"""
        longest, bins = self._cut(cutoff)
        if not self.records:
            return 0.0
        if minreadlength > _lib.MAX_READLENGTH:
            raise ValueError('lengths of %d and more are not binned' % _lib.MAX_READLENGTH)
        dropped = int(bins[:max(int(minreadlength), 0)].sum())
        return (self.records - dropped) / float(self.records)

    # -- per cycle ---------------------------------------------------------------

    def _cycles(self):
        if self.cycles is None:
            raise ValueError('this profile was taken without cycles=True')
        return self.cycles

    @property
    def cycle_scores(self):
        """(1024, 256): records whose score line has byte b at position p"""
        return self._cycles()[:CYCLES * 256].reshape(CYCLES, 256)

    @property
    def cycle_bases(self):
        """(1024, 256): the same for the bases line"""
        return self._cycles()[CYCLES * 256:].reshape(CYCLES, 256)

    def cycles_reached(self, kind='score'):
        """per cycle, the lines of that kind ('score' / 'base') that reach it"""
        if kind not in ('score', 'base'):
            raise ValueError("kind is 'score' or 'base'")
        return (self.cycle_scores if kind == 'score' else self.cycle_bases).sum(axis=1)

    @property
    def last_cycle(self):
        """the highest cycle any line reaches (-1: none)"""
        reached = np.nonzero(self.cycles_reached('score') + self.cycles_reached('base'))[0]
        return int(reached[-1]) if reached.size else -1

    def cycle_mean_quality(self, dQ=None):
        """per cycle, the mean PHRED score ('\\r' left out); nan where no record reaches the cycle"""
        return _rows_mean_quality(self.cycle_scores, self.dQ() if dQ is None else dQ)

    def cycle_quantile(self, q, dQ=None):
        """per cycle, the lowest PHRED value whose cumulative count reaches ``q`` (0 .. 1) of the cycle's scores
        ('\\r' left out); nan where no record reaches the cycle"""
        return _rows_quantile(self.cycle_scores, q, self.dQ() if dQ is None else dQ)

    def cycle_below(self, cutoff):
        """per cycle, the share of its score bytes below ``cutoff``, compared as signed char as ``Amin`` is; nan where
        no record reaches the cycle"""
        c = as_cutoffs([cutoff])[0]
        signed = np.arange(256) - 256 * (np.arange(256) >= 128)
        n = self.cycle_scores
        return _share(n[:, signed < (c - 256 if c >= 128 else c)].sum(axis=1), n.sum(axis=1))

    def cycle_base_share(self):
        """(1024, 6): per cycle the shares of A, C, G, T, N (upper case only) and of every other byte; nan where no
        record reaches the cycle"""
        return _rows_base_share(self.cycle_bases)

    def cycle_lines(self, step=1, dQ=None):
        """the per-cycle table of the command line, a line per ``step`` cycles up to ``last_cycle``: the score lines
        reaching the (first) cycle, the mean Q, its 10 % / 50 % / 90 % quantiles, the shares of A C G T N"""
        if dQ is None:
            try:
                dQ = self.dQ()
            except FastqFileFormatException:
                dQ = 0
        step = max(int(step), 1)
        starts = np.arange(0, self.last_cycle + 1, step)
        lines = ['cycle reads meanQ Q10 Q50 Q90 A C G T N (dQ=%d)' % dQ]
        if not starts.size:
            return lines
        scores, bases = np.add.reduceat(self.cycle_scores, starts, axis=0), np.add.reduceat(self.cycle_bases, starts, axis=0)
        reached, mean, share = self.cycles_reached('score'), _rows_mean_quality(scores, dQ), _rows_base_share(bases)
        quant = [_rows_quantile(scores, q, dQ) for q in (0.1, 0.5, 0.9)]
        for i, a in enumerate(starts.tolist()):
            b = min(a + step, CYCLES) - 1
            lines.append('%s %d %.2f %s %s' % (a if b == a else '%d-%d' % (a, b), reached[a], mean[i], ' '.join('%g' % v[i] for v in quant),
                                              ' '.join('%.3f' % v for v in share[i, :5])))
        return lines

    # -- per read ----------------------------------------------------------------

    def _reads(self):
        if self.reads is None:
            raise ValueError('this profile was taken without per_read=True')
        return self.reads

    @property
    def gc_hist(self):
        """(101,): the reads by their GC share in per cent (G + C among A C G T, round half up)"""
        return self._reads()[READS_GC:READS_GC + READS_GC_BINS]

    @property
    def gc_none(self):
        """the reads whose bases line holds no A C G T"""
        return int(self._reads()[READS_GC_NONE])

    @property
    def mean_quality_hist(self):
        """(256,): the reads by the mean byte of their score line (round half up); ``mean_quality_per_read`` in PHRED"""
        return self._reads()[READS_MEANQ:READS_MEANQ + 256]

    @property
    def n_hist(self):
        """(256,): the reads by the number of N on their bases line, 255 and more in the last bin"""
        return self._reads()[READS_NCOUNT:READS_NCOUNT + 256]

    def gc_mean(self):
        """the mean of the reads' GC shares in per cent (of the bins); nan when no read has A C G T"""
        n = int(self.gc_hist.sum())
        return float((self.gc_hist * np.arange(READS_GC_BINS)).sum()) / n if n else float('nan')

    def mean_quality_per_read(self, dQ=None):
        """{PHRED value: reads whose mean score rounds to it} over the bins that are not empty; ``dQ`` None: :meth:`dQ`"""
        dQ = self.dQ() if dQ is None else dQ
        return {int(b) - 33 - dQ: int(self.mean_quality_hist[b]) for b in np.nonzero(self.mean_quality_hist)[0]}

    def mean_quality_quantile(self, q, dQ=None):
        """the lowest PHRED value whose cumulative count reaches ``q`` (0 .. 1) of the reads' mean scores; nan: no read has scores"""
        return float(_rows_quantile_raw(self.mean_quality_hist[None, :], q, self.dQ() if dQ is None else dQ)[0])

    def duplicate_share(self):
        """1 - tracked distinct keys / tracked records: the share of the (sampled) reads that repeat an earlier one;
        nan when no read has a key"""
        d = self.duplication
        if d is None:
            raise ValueError('this profile was taken without duplication=True')
        return 1.0 - d['tracked_distinct'] / float(d['tracked_records']) if d['tracked_records'] else float('nan')

    def per_read_lines(self, dQ=None):
        """the per-read part of the command line: the GC histogram in 5 % steps with its mean, the quantiles of the reads'
        mean quality, the share of reads with any N"""
        if dQ is None:
            try:
                dQ = self.dQ()
            except FastqFileFormatException:
                dQ = 0
        gc, n = self.gc_hist, int(self.gc_hist.sum())
        lines = ['per-read GC: mean=%.1f%% reads=%d none=%d' % (self.gc_mean(), n, self.gc_none)]
        for a in range(0, READS_GC_BINS, 5):
            part = int(gc[a:a + 5].sum())
            lines.append('GC %3d-%3d%% %d %.4f' % (a, min(a + 4, 100), part, part / float(n) if n else 0.0))
        lines.append('per-read mean quality (dQ=%d): %s' % (dQ, ' '.join('Q%d=%g' % (int(q * 100), self.mean_quality_quantile(q, dQ)) for q in (0.1, 0.25, 0.5, 0.75, 0.9))))
        total = int(self.n_hist.sum())
        lines.append('reads with any N: %d of %d (%.4f)' % (total - int(self.n_hist[0]), total, (total - int(self.n_hist[0])) / float(total) if total else 0.0))
        return lines

    def duplication_lines(self):
        """the duplication part of the command line: level and sample size, then a line per count bin"""
        d = self.duplication
        if d is None:
            raise ValueError('this profile was taken without duplication=True')
        lines = ['duplication: level=%d (1 of %d distinct sequences) slots=%d keyed=%d unkeyed=%d tracked: %d reads, %d distinct, duplicate share %.4f'
                 % (d['level'], 1 << d['level'], d['slots'], d['keyed'], d['unkeyed'], d['tracked_records'], d['tracked_distinct'], self.duplicate_share())]
        for i, lo_ in enumerate(DUP_BOUNDS):
            hi = '%d' % (DUP_BOUNDS[i + 1] - 1) if i + 1 < len(DUP_BOUNDS) else ''
            span = '%d' % lo_ if hi == '%d' % lo_ else '%d+' % lo_ if not hi else '%d-%s' % (lo_, hi)
            lines.append('copies %s: distinct=%d reads=%d' % (span, d['distinct'][i], d['records'][i]))
        return lines

    # -- overrepresented sequences -----------------------------------------------

    def relabel(self, sources=None):
        """read the rows again, their ``source`` from ``sources`` (None: ``KNOWN_SOURCES``); returns the list"""
        if self.over is None:
            raise ValueError('this profile was taken without overrepresented=True')
        keyed = self.over_info['keyed']
        rows = self.over[OVER_ROWS:OVER_ROWS + OVER_ROW_WORDS * self.over_info['listed']].reshape(-1, OVER_ROW_WORDS)
        self.overrepresented = []
        for row in rows:
            sequence = row[3:].astype('<i8').tobytes()[:int(row[2])]
            self.overrepresented.append(Overrepresented(sequence, int(row[1]), int(row[1]) / float(keyed), int(row[0]) & 0xFFFFFFFFFFFFFFFF,
                                                        source_of(sequence, sources)))
        return self.overrepresented

    def overrepresented_lines(self):
        """the overrepresented part of the command line: what was looked at, then a line per listed sequence"""
        if self.over is None:
            raise ValueError('this profile was taken without overrepresented=True')
        o = self.over_info
        lines = ['overrepresented: %d sequences of 0.1 %% and more among the %d candidates of the first %d records (keyed=%d unkeyed=%d counted=%d)'
                 % (o['listed'], o['candidates'], o['records_limit'], o['keyed'], o['unkeyed'], o['counted'])]
        for r in self.overrepresented:
            lines.append('%s %d %.4f%% %s' % (r.sequence.decode('latin-1').encode('unicode_escape').decode('ascii'), r.count, 100 * r.share,
                                             r.source or 'no known source'))
        return lines

    # -- adapter content -----------------------------------------------------------

    def _adapters(self):
        if self.adapters is None:
            raise ValueError('this profile was taken without adapters=')
        return self.adapters

    def adapter_content(self, k=None):
        """(1024,): per cycle p, the share of all records whose first full occurrence of probe ``k`` (an index or a name) starts
        at p or before it -- FastQC's curve; ``k`` None: the sum over the probes.  nan without records"""
        a = self._adapters()
        if k is None:
            first = a.first.sum(axis=0)
        else:
            first = a.first[a.names.index(k) if not isinstance(k, int) else k]
        return _share(np.cumsum(first), a.records)

    def adapter_share(self):
        """the share of the records that hold a full occurrence of any probe; nan without records"""
        a = self._adapters()
        return a.with_adapter / float(a.records) if a.records else float('nan')

    def clipped_share(self):
        """the share of the records an adapter clip would shorten: those with a full occurrence of a probe or, failing that,
        with a tail match; nan without records"""
        a = self._adapters()
        return (a.with_adapter + a.tail_only) / float(a.records) if a.records else float('nan')

    def clip_quantile(self, q):
        """the smallest length whose cumulative count reaches ``q`` (0 .. 1) of the records by the length an adapter clip would
        leave (1024: that and more); nan without records"""
        if not 0.0 <= q <= 1.0:
            raise ValueError('a quantile lies in 0 .. 1')
        a = self._adapters()
        cum = np.cumsum(a.clip)
        return float((cum >= max(q * cum[-1], 1)).argmax()) if cum[-1] else float('nan')

    def adapter_lines(self):
        """the adapter part of the command line: the shares, the quantiles of the clipped length, then a line per probe"""
        a = self._adapters()
        lines = ['adapters: records=%d with_adapter=%d (%.4f) tail_only=%d clipped share %.4f'
                 % (a.records, a.with_adapter, self.adapter_share(), a.tail_only, self.clipped_share()),
                 'clipped length: %s' % ' '.join('Q%d=%g' % (int(q * 100), self.clip_quantile(q)) for q in (0.1, 0.25, 0.5, 0.75, 0.9))]
        for k, name in enumerate(a.names):
            at = np.nonzero(a.first[k])[0]
            lines.append('%s %s: found=%d (%.4f) first cycle=%s beyond=%d tails=%d'
                         % (name, a.probes[k].decode('latin-1') if a.probes[k] is not None else '?', int(a.found[k]),
                            int(a.found[k]) / float(a.records) if a.records else 0.0, int(at[0]) if at.size else '-', int(a.beyond[k]), int(a.tailed[k])))
            if a.mismatch_per:
                lines[-1] += ' mismatches(1 per %d)=%s' % (a.mismatch_per, '/'.join(str(int(v)) for v in a.first_mismatches[k]))
        return lines

    def summary(self):
        lines = ['records=%d mismatched=%d longest=%d' % (self.records, self.mismatched, self.longest)]
        lo_, hi = self.score_range()
        try:
            lines.append('dQ=%d' % self.dQ())
        except FastqFileFormatException as e:
            lines.append('dQ=? (%s)' % e)
        span = '?' if lo_ > hi else '%r..%r' % (chr(lo_ + 33), chr(hi + 33))
        lines.append('variants=%s scores=%s' % (self.variants(), span))
        for c in self.cutoffs:
            rl = self.readlengths(c)
            n = sum(rl)
            mean = sum(i * v for i, v in enumerate(rl)) / float(n) if n else 0.0
            lines.append('cutoff=%s readlengths: longest=%d mean=%.1f binned=%d' % (repr(chr(c)) if 33 <= c < 127 else hex(c), len(rl) - 1, mean, n))
        return '\n'.join(lines)

    def as_dict(self):
        """what ``Analyser.encode`` stores"""
        d = {'records': self.records, 'mismatched': self.mismatched, 'longest': self.longest,
             'score_bytes': {int(b): int(self.score_bytes[b]) for b in np.nonzero(self.score_bytes)[0]},
             'base_bytes': {int(b): int(self.base_bytes[b]) for b in np.nonzero(self.base_bytes)[0]},
             'readlengths': {str(c): list(self.readlengths(c)) for c in self.cutoffs}}
        if self.cycles is not None:
            def sparse(rows):
                return [{int(b): int(row[b]) for b in np.nonzero(row)[0]} for row in rows[:self.last_cycle + 1]]
            d['cycles'] = {'score': sparse(self.cycle_scores), 'base': sparse(self.cycle_bases)}
        if self.reads is not None:
            def bins(h):
                return {int(b): int(h[b]) for b in np.nonzero(h)[0]}
            d['per_read'] = {'records': int(self.reads[READS_RECORDS]), 'gc_none': self.gc_none, 'meanq_none': int(self.reads[READS_MEANQ_NONE]),
                             'gc': bins(self.gc_hist), 'mean_quality_byte': bins(self.mean_quality_hist), 'n': bins(self.n_hist)}
        if self.duplication is not None:
            d['duplication'] = dict(self.duplication, bounds=list(DUP_BOUNDS))
        if self.over is not None:
            d['overrepresented'] = dict(self.over_info, rows=[dict(r._asdict(), sequence=r.sequence.decode('latin-1')) for r in self.overrepresented])
        if self.adapters is not None:
            d['adapters'] = self.adapters.as_dict()
        return d


CLIP_N, CLIP_RECORDS, CLIP_CLIPPED, CLIP_MASKED, CLIP_BASES_CUT, CLIP_LEN = 0, 1, 2, 3, 4, 8      # (include/kvarq_hip.h: kvq_clip_len())
CLIP_PER = 5                                                       # (written only with adapter_mismatches)


class Clip(object):
    """what the adapter clip of a scan did (kvq_scan_clip; the definition: include/kvarq_hip.h): ``records``,
    ``clipped`` (records whose adapter begins inside the read), ``masked`` (score positions set to '!'), ``bases_cut`` (bases
    behind the clips), ``words`` (the eight words), ``names`` and ``probes``"""

    def __init__(self, words, names=None, probes=None):
        w = self.words = np.asarray(words, dtype=np.int64)
        assert w.shape == (CLIP_LEN,)
        self.records, self.clipped, self.masked, self.bases_cut = int(w[CLIP_RECORDS]), int(w[CLIP_CLIPPED]), int(w[CLIP_MASKED]), int(w[CLIP_BASES_CUT])
        self.names, self.probes = names, probes
        self.mismatch_per = int(w[CLIP_PER])    # 0: the probes matched byte for byte; else the ``per`` of ``adapter_mismatches``

    def __eq__(self, other):
        return isinstance(other, Clip) and np.array_equal(self.words, other.words)

    def __ne__(self, other):
        return not self == other

    def __getitem__(self, key):
        if key not in ('records', 'clipped', 'masked', 'bases_cut', 'words'):
            raise KeyError(key)
        return getattr(self, key)

    def line(self):
        return 'clip: records=%d clipped=%d (%.4f) masked=%d bases_cut=%d' % (
            self.records, self.clipped, self.clipped / float(self.records) if self.records else float('nan'), self.masked, self.bases_cut) + (
            ' mismatches=1 per %d' % self.mismatch_per if self.mismatch_per else '')


def clip_from_scan(L, h, clip=None):
    """the ``Clip`` of a finished scan object, None when the option is off; ``clip``: ``(names, probes)`` of ``ScanOptions``"""
    ptr = L.kvq_scan_clip(h)
    names, probes = clip if clip is not None else (None, None)
    return Clip(np.ctypeslib.as_array(ptr, shape=(CLIP_LEN,)).copy(), names, probes) if ptr else None


def clip_host(text, clip, chunk_off=None, into=None, adapter_mismatches=None):
    """the CPU twin of the adapter clip (kvq_clip_host; with ``adapter_mismatches``: kvq_clip_host_mm) over a text in host memory:
    (MASK(text) as a new uint8 array, the eight words); ``into``: words to add to, as the twin does"""
    from . import scan
    from .options import as_mismatch_per
    _, probes = as_adapters(clip)
    per = as_mismatch_per(adapter_mismatches)
    arr = (np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text)).copy()
    co = scan.chunk_offsets(arr) if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.int64)
    n = len(probes)
    words = np.zeros(CLIP_LEN, dtype=np.int64) if into is None else into
    args = (arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1,
            (C.c_char_p * n)(*probes), (C.c_int32 * n)(*[len(p) for p in probes]), n)
    out = words.ctypes.data_as(C.POINTER(C.c_int64))
    if _lib.lib().kvq_clip_host_mm(*(args + (per, out))) if per else _lib.lib().kvq_clip_host(*(args + (out,))):
        raise RuntimeError(_lib.last_error()[1])
    return arr, words


EMIT_N, EMIT_RECORDS, EMIT_EMITTED, EMIT_SHORT, EMIT_MISMATCHED, EMIT_BASES_IN, EMIT_BASES_OUT, EMIT_BYTES_OUT, EMIT_LEN = 0, 1, 2, 3, 4, 5, 6, 7, 8      # (include/kvarq_hip.h: kvq_emit_len())
EMIT_FIELDS = ('records', 'emitted', 'short', 'mismatched', 'bases_in', 'bases_out', 'bytes_out')


class Emit(object):
    """what the emit of a scan wrote (kvq_scan_emit; the definition: include/kvarq_hip.h): ``records``, of them
    ``emitted``, ``short`` (the trim left less than ``min_length``) and ``mismatched`` (bases and scores of different lengths);
    ``bases_in`` (on all bases lines), ``bases_out`` (on the emitted ones), ``bytes_out`` (the emitted text), ``words`` (the eight
    words) and ``min_length``, the shortest read that was kept"""

    def __init__(self, words):
        w = self.words = np.asarray(words, dtype=np.int64)
        assert w.shape == (EMIT_LEN,)
        self.min_length = int(w[EMIT_N])
        for k, name in enumerate(EMIT_FIELDS):
            setattr(self, name, int(w[EMIT_RECORDS + k]))

    def __eq__(self, other):
        return isinstance(other, Emit) and np.array_equal(self.words, other.words)

    def __ne__(self, other):
        return not self == other

    def __getitem__(self, key):
        if key not in EMIT_FIELDS + ('words',):
            raise KeyError(key)
        return getattr(self, key)

    def line(self):
        return 'emit: records=%d emitted=%d (%.4f) short=%d mismatched=%d bases %d -> %d bytes_out=%d min_length=%d' % (
            self.records, self.emitted, self.emitted / float(self.records) if self.records else float('nan'), self.short, self.mismatched,
            self.bases_in, self.bases_out, self.bytes_out, self.min_length)


def emit_from_scan(L, h):
    """the ``Emit`` of a finished scan object, None when the option is off"""
    ptr = L.kvq_scan_emit(h)
    return Emit(np.ctypeslib.as_array(ptr, shape=(EMIT_LEN,)).copy()) if ptr else None


def emitted_from_scan(L, h):
    """the emitted text of a finished scan object whose sink is the library's host buffer, a new uint8 array"""
    ptr, n = C.c_void_p(), C.c_int64()
    if L.kvq_scan_emitted(h, C.byref(ptr), C.byref(n)):
        raise RuntimeError(_lib.last_error()[1])
    return np.frombuffer(C.string_at(ptr.value, n.value) if n.value else b'', dtype=np.uint8)


DEFLATE_LEN = 8                                              # (include/kvarq_hip.h: kvq_deflate_len())
DEFLATE_FIELDS = ('members', 'bytes_in', 'bytes_out', 'stored', 'matches', 'literals', 'max_distance', 'max_length')


def deflate_words(w):
    """the words of a deflate as a dict: ``DEFLATE_FIELDS``, ``ratio`` (bytes in per byte out; nan for an empty text), ``words``"""
    w = np.asarray(w, dtype=np.int64)
    assert w.shape == (DEFLATE_LEN,)
    d = dict((name, int(w[k])) for k, name in enumerate(DEFLATE_FIELDS))
    d['ratio'] = d['bytes_in'] / float(d['bytes_out']) if d['bytes_out'] else float('nan')
    d['words'] = w
    return d


def emit_compress_from_scan(L, h):
    """what the emit's deflate of a finished scan object did (kvq_scan_emit_compress), None when it is off"""
    ptr = L.kvq_scan_emit_compress(h)
    return deflate_words(np.ctypeslib.as_array(ptr, shape=(DEFLATE_LEN,)).copy()) if ptr else None


def bgzf_eof():
    """the 28 bytes of the BGZF EOF member (kvq_bgzf_eof)"""
    return C.string_at(_lib.lib().kvq_bgzf_eof(), 28)


def deflate_bgzf_host(text, cap=None):
    """the CPU twin of the emit's deflate (kvq_deflate_bgzf_host) over a text in host memory: (BGZF(text) as bytes -- the members,
    without the EOF member --, the eight words).  The output buffer is exactly kvq_deflate_bound(len(text)) long, or ``cap``"""
    L = _lib.lib()
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, dtype=np.uint8)
    out = np.empty(L.kvq_deflate_bound(arr.nbytes) if cap is None else cap, dtype=np.uint8)
    words = np.zeros(DEFLATE_LEN, dtype=np.int64)
    n = L.kvq_deflate_bgzf_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, out.ctypes.data if out.nbytes else None, out.nbytes,
                                words.ctypes.data_as(C.POINTER(C.c_int64)))
    if n < 0:
        raise RuntimeError(_lib.last_error()[1])
    return out[:n].tobytes(), words


def deflate_lengths_host(freq, limit):
    """the length-limited code builder on its own (kvq_deflate_lengths_host): the code lengths of a histogram, a uint8 array"""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.zeros(len(f), dtype=np.uint8)
    if _lib.lib().kvq_deflate_lengths_host(f.ctypes.data, len(f), limit, lens.ctypes.data):
        raise RuntimeError(_lib.last_error()[1])
    return lens


def emit_host(text, amin, min_length, chunk_off=None, into=None):
    """the CPU twin of the emit (kvq_emit_host) over a text in host memory: (EMIT(text) as a new uint8 array, the eight words).
    ``amin``: a byte value, a character or a byte; ``into``: words to add to, as the twin does.  The output buffer is exactly the
    text's bytes plus its records long"""
    from . import scan
    a = amin & 0xFF if isinstance(amin, int) else (amin.encode('latin-1') if isinstance(amin, str) else bytes(amin))[0]
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text)
    co = scan.chunk_offsets(arr) if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.int64)
    raw = arr.tobytes()
    nrec = sum(raw.count(b'\n', int(x), int(y)) // 4 for x, y in zip(co, co[1:]))
    out = np.empty(arr.nbytes + nrec, dtype=np.uint8)
    words = np.zeros(EMIT_LEN, dtype=np.int64) if into is None else into
    n = _lib.lib().kvq_emit_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1,
                                 (a ^ 0x80) - 0x80, min_length, out.ctypes.data if out.nbytes else None, out.nbytes,
                                 words.ctypes.data_as(C.POINTER(C.c_int64)))
    if n < 0:
        raise RuntimeError(_lib.last_error()[1])
    return out[:n].copy(), words


def from_scan(L, h, sources=None, adapters=None):
    """the profile of a finished scan object (kvq_scan_profile), None when it keeps none; ``sources``: as for ``Profile``;
    ``adapters``: ``(names, probes)`` of the scan's adapter probes (``ScanOptions``), which the flat array does not hold"""
    cuts = (C.c_uint8 * MAX_CUTOFFS)()
    n = L.kvq_scan_profile_cutoffs(h, cuts)
    ptr = L.kvq_scan_profile(h)
    if n < 0 or not ptr:
        return None
    cyc, reads, dup, over = L.kvq_scan_cycles(h), L.kvq_scan_reads(h), L.kvq_scan_dup(h), L.kvq_scan_over(h)
    ada = L.kvq_scan_adapters(h)
    names, probes = adapters if adapters is not None else (None, None)
    return Profile(np.ctypeslib.as_array(ptr, shape=(profile_len(n),)).copy(), list(cuts)[:n],
                   np.ctypeslib.as_array(cyc, shape=(CYCLES_LEN,)).copy() if cyc else None,
                   np.ctypeslib.as_array(reads, shape=(READS_LEN,)).copy() if reads else None,
                   np.ctypeslib.as_array(dup, shape=(DUP_LEN,)).copy() if dup else None,
                   np.ctypeslib.as_array(over, shape=(OVER_LEN,)).copy() if over else None, sources,
                   Adapters(np.ctypeslib.as_array(ada, shape=(ADAPT_LEN,)).copy(), names, probes) if ada else None)


def profile_host(text, cutoffs=(), chunk_off=None, cycles=False, per_read=False, duplication=False, slots=0, overrepresented=False,
                 over_records=0, sources=None, adapters=None, clip=None, adapter_mismatches=None):
    """the CPU twin (kvq_profile_host; cycles: and kvq_cycles_host; per_read / duplication: and kvq_reads_host, with a
    table of ``slots`` slots, 0: the default; overrepresented: and kvq_over_host, with the first ``over_records`` records
    making the candidates, 0: the default; adapters: and kvq_adapt_host, with the probes of ``as_adapters``) over a text in host memory; chunk_off None: the reader's chunk cuts;
    clip: the profile of a copy of the text that kvq_clip_host has masked with these probes (``Profile.clipped``: the ``Clip``);
    adapter_mismatches: the probes of both tolerate mismatches (kvq_adapt_host_mm, kvq_clip_host_mm; as for ``ScanOptions``)"""
    from . import scan
    from .options import as_mismatch_per
    if as_mismatch_per(adapter_mismatches) and adapters in (None, False) and clip in (None, False):
        raise ValueError('adapter_mismatches= is the rule of the probes of adapters= or clip=: give one of them')
    cuts = as_cutoffs(cutoffs)
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text)
    co = scan.chunk_offsets(arr) if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.int64)
    clipped = None
    if clip is not None and clip is not False:
        arr, words = clip_host(arr, clip, co, adapter_mismatches=adapter_mismatches)
        clipped = Clip(words, *as_adapters(clip))
    out = np.zeros(profile_len(len(cuts)), dtype=np.int64)
    rc = _lib.lib().kvq_profile_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)),
                                     len(co) - 1, _cut_array(cuts), len(cuts), out.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc:
        raise RuntimeError(_lib.last_error()[1])
    cyc = None
    if cycles:
        cyc = np.zeros(CYCLES_LEN, dtype=np.int64)
        if _lib.lib().kvq_cycles_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)),
                                      len(co) - 1, cyc.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError(_lib.last_error()[1])
    reads = np.zeros(READS_LEN, dtype=np.int64) if per_read else None
    dup = np.zeros(DUP_LEN, dtype=np.int64) if duplication else None
    if per_read or duplication:
        if _lib.lib().kvq_reads_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1, int(slots),
                                     reads.ctypes.data_as(C.POINTER(C.c_int64)) if per_read else None,
                                     dup.ctypes.data_as(C.POINTER(C.c_int64)) if duplication else None):
            raise RuntimeError(_lib.last_error()[1])
    over = None
    if overrepresented:
        over = np.zeros(OVER_LEN, dtype=np.int64)
        if _lib.lib().kvq_over_host(arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1,
                                    int(over_records), over.ctypes.data_as(C.POINTER(C.c_int64))):
            raise RuntimeError(_lib.last_error()[1])
    ada = None
    if adapters is not None and adapters is not False:
        ada = adapt_host(arr, adapters, co, adapter_mismatches=adapter_mismatches)
    p = Profile(out, cuts, cyc, reads, dup, over, sources, ada)
    p.clipped = clipped
    return p


def adapt_host(text, adapters, chunk_off=None, adapter_mismatches=None):
    """the CPU twin of the adapter content alone (kvq_adapt_host; with ``adapter_mismatches``: kvq_adapt_host_mm) over a text in
    host memory: an ``Adapters``"""
    from . import scan
    from .options import as_mismatch_per
    names, probes = as_adapters(adapters)
    per = as_mismatch_per(adapter_mismatches)
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text)
    co = scan.chunk_offsets(arr) if chunk_off is None else np.ascontiguousarray(chunk_off, dtype=np.int64)
    n = len(probes)
    words = np.zeros(ADAPT_LEN, dtype=np.int64)
    args = (arr.ctypes.data if arr.nbytes else None, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1,
            (C.c_char_p * n)(*probes), (C.c_int32 * n)(*[len(p) for p in probes]), n)
    out = words.ctypes.data_as(C.POINTER(C.c_int64))
    if _lib.lib().kvq_adapt_host_mm(*(args + (per, out))) if per else _lib.lib().kvq_adapt_host(*(args + (out,))):
        raise RuntimeError(_lib.last_error()[1])
    return Adapters(words, names, probes)


def profile(fnames, cutoffs=True, inflate='host', sources=None, **options):
    """the profile of one file or several (plain, gzip, BGZF, BAM), by a scan with no sequences; ``cycles``: with the
    per-cycle counts; ``per_read`` / ``duplication``: with the per-read distributions / the duplication; ``overrepresented``:
    with the overrepresented sequences, labelled from ``sources`` (None: ``KNOWN_SOURCES``); ``adapters``: with the adapter
    content of these probes (``as_adapters``); ``clip``: of the input with the scores of its adapters masked (DESIGN section 19;
    ``Profile.clipped``: the ``Clip``); ``adapter_mismatches``: the probes of both tolerate mismatches;
    ``emit`` (a path) / ``emit_min``: the input's reads, trimmed (and clipped, with ``clip``), are written there as FastQ (DESIGN
    section 21; ``Profile.emitted``: the ``Emit``) -- a BAM thereby becomes trimmed FastQ; ``emit_compress``: that file is BGZF,
    deflated on the GPU (``Profile.emit_compressed``: the dict of ``deflate_words``);
    ``long_reads``: as for
    ``engine.findseqs``, which takes the ``options``"""
    from . import engine
    r = engine.findseqs(fnames, [], inflate=inflate, profile=cutoffs, **options)
    p = r['profile']
    p.clipped = r.get('clip')
    p.emitted = r.get('emit')                   # the ``Emit`` of a call with ``emit=`` (the text is in the file)
    p.emit_compressed = r.get('emit_compress')  # what its deflate did, with ``emit_compress=True``
    if sources is not None and p.over is not None:
        p.relabel(sources)
    return p


def main(argv=None):
    import argparse
    from . import engine
    ap = argparse.ArgumentParser(prog='python -m kvarq_amd.profile', description='profile of a FastQ / BAM file, taken on the GPU')
    ap.add_argument('files', nargs='+')
    ap.add_argument('-Q', '--quality', type=int, action='append', help='PHRED cutoff(s); default: the configured Amin')
    ap.add_argument('--inflate', default='host', choices=sorted(engine.INFLATE_FLAGS))
    ap.add_argument('--cycles', action='store_true', help='a line per cycle: reads reaching it, mean Q, 10/50/90 %% quantiles, shares of A C G T N')
    ap.add_argument('--cycle-step', type=int, default=1, metavar='N', help='a line per N cycles')
    ap.add_argument('--per-read', action='store_true', help='the per-read GC histogram in 5 %% steps with its mean, the quantiles of the per-read mean quality, the share of reads with any N')
    ap.add_argument('--duplication', action='store_true', help='how often the first 64 bases of the reads repeat: level, sample size and a line per count bin')
    ap.add_argument('--overrepresented', action='store_true', help='the sequences (first 64 bases) that make up 0.1 %% of the reads and more, among those of the first 2^18 records: count, share, known source')
    ap.add_argument('--adapters', nargs='*', metavar='NAME=SEQ', help='the adapter content: how many reads hold each probe and from which cycle on, tails of 6 bases and more, the length a clip would leave; without arguments: the known adapters')
    ap.add_argument('--clip', nargs='*', metavar='NAME=SEQ', help="the profile of the input with the scores of its adapters set to '!' ahead of the trim, and how much was clipped; without arguments: the known adapters (with --adapters: the same probes)")
    ap.add_argument('--adapter-mismatches', nargs='?', type=int, const=10, default=None, metavar='PER',
                    help='with --adapters or --clip: the probes tolerate one mismatch per PER bases (10 .. 32; without a value: 10); the adapter lines gain the counts of first occurrences with 0/1/2/3 mismatches')
    ap.add_argument('--emit', metavar='OUT', help='write the reads as the scan saw them -- cut to the quality trim at the configured Amin, behind --clip to the adapter too -- to OUT as FastQ, all files to the one output')
    ap.add_argument('--emit-min', type=int, default=None, metavar='N', help='with --emit: keep reads of N bases and more (default: the configured minreadlength; 0 keeps every record, so that the files of two mates stay in step)')
    ap.add_argument('--emit-bgzf', action='store_true', help='with --emit: OUT is BGZF (.fastq.gz as samtools, bwa and minimap2 read it), deflated on the GPU; the name of OUT decides nothing')
    a = ap.parse_args(argv)
    if a.emit_min is not None and (a.emit is None or a.emit_min < 0):
        ap.error('--emit-min takes N >= 0 and needs --emit')
    if a.emit_bgzf and a.emit is None:
        ap.error('--emit-bgzf needs --emit')
    if a.adapter_mismatches is not None and a.adapters is None and a.clip is None:
        ap.error('--adapter-mismatches needs --adapters or --clip')
    if a.adapter_mismatches is not None and not 10 <= a.adapter_mismatches <= 32:
        ap.error('--adapter-mismatches takes 10 .. 32')
    more = dict(cycles=a.cycles, per_read=a.per_read, duplication=a.duplication, overrepresented=a.overrepresented)
    if a.adapters is not None:
        for item in a.adapters:
            if '=' not in item:
                ap.error('--adapters takes NAME=SEQ')
        more['adapters'] = collections.OrderedDict((i.split('=', 1)[0], i.split('=', 1)[1].encode('latin-1')) for i in a.adapters) if a.adapters else True
    if a.clip is not None:
        for item in a.clip:
            if '=' not in item:
                ap.error('--clip takes NAME=SEQ')
        more['clip'] = collections.OrderedDict((i.split('=', 1)[0], i.split('=', 1)[1].encode('latin-1')) for i in a.clip) if a.clip else True
    if a.adapter_mismatches is not None:
        more['adapter_mismatches'] = a.adapter_mismatches
    if a.emit is not None:
        more['emit'] = a.emit
        if a.emit_min is not None:
            more['emit_min'] = a.emit_min
        if a.emit_bgzf:
            more['emit_compress'] = True
    p = profile(a.files, cutoffs=True, inflate=a.inflate, **({} if a.quality else more))
    if a.quality:
        dQ = p.dQ()
        p = profile(a.files, cutoffs=[ASCII[q + dQ] for q in a.quality], inflate=a.inflate, **more)
    print(p.summary())
    if a.cycles:
        print('\n'.join(p.cycle_lines(a.cycle_step)))
    if a.per_read:
        print('\n'.join(p.per_read_lines()))
    if a.duplication:
        print('\n'.join(p.duplication_lines()))
    if a.overrepresented:
        print('\n'.join(p.overrepresented_lines()))
    if a.adapters is not None:
        print('\n'.join(p.adapter_lines()))
    if a.clip is not None:
        print(p.clipped.line())
    if a.emit is not None:
        print(p.emitted.line())
        if a.emit_bgzf:
            z = p.emit_compressed
            print('emit bgzf: members=%d stored=%d bytes %d -> %d (%.3f)' % (z['members'], z['stored'], z['bytes_in'], z['bytes_out'] + 28, z['ratio']))


if __name__ == '__main__':
    main()
