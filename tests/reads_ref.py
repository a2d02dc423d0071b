"""
The per-read distributions and the duplication of a FastQ text (include/kvarq_hip.h) as a plain Python
statement of their definition: the yardstick of tests/test_reads_host.py (the CPU twin) and tests/test_gpu_reads.py (the
kernels).  And the texts both run on.

They cover the records the profile covers (``profile_ref.records_of``); a trailing '\\r' is not part of its line.  The hash
is restated here, not imported; the level is "the smallest s with at most C / 2 distinct tracked keys".
"""
import functools

import numpy as np

import profile_ref as R

RECORDS, GC_NONE, MEANQ_NONE, GC, GC_BINS, MEANQ, NCOUNT, LEN = 0, 1, 2, 8, 101, 109, 365, 621
D_LEVEL, D_SLOTS, D_KEYED, D_UNKEYED, D_TRACKED_RECORDS, D_TRACKED_KEYS, D_DISTINCT, D_RECORDS, D_LEN = 0, 1, 2, 3, 4, 5, 8, 24, 40
BOUNDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)
DEFAULT_SLOTS, MIN_SLOTS = 1 << 24, 1024
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


def lines_of(text, chunk_off):
    """(bases line, score line) of every record, the trailing '\\r' taken off"""
    text = bytes(text)
    out = []
    for n0, n1, n2, n3 in R.records_of(text, [int(c) for c in chunk_off]):
        b, s = text[n0 + 1:n1], text[n2 + 1:n3]
        out.append((b[:-1] if b.endswith(b'\r') else b, s[:-1] if s.endswith(b'\r') else s))
    return out


def reads(text, chunk_off, into=None):
    """the flat int64 array of the per-read distributions; ``into``: add to it, as kvq_reads_host does"""
    out = np.zeros(LEN, dtype=np.int64) if into is None else into
    for b, s in lines_of(text, chunk_off):
        out[RECORDS] += 1
        a = sum(b.count(c) for c in b'ACGT')
        g = b.count(b'G') + b.count(b'C')
        if a:
            out[GC + (200 * g + a) // (2 * a)] += 1
        else:
            out[GC_NONE] += 1
        if s:
            out[MEANQ + (2 * sum(s) + len(s)) // (2 * len(s))] += 1
        else:
            out[MEANQ_NONE] += 1
        out[NCOUNT + min(b.count(b'N'), 255)] += 1
    return out


def _m(x):
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    return x ^ x >> 31


def dup_hash(line):
    """the hash of the key of a bases line (its first 64 bytes), restated from the header"""
    key = bytes(line[:64])
    n = len(key)
    assert n >= 1
    key += b'\0' * (64 - n)
    h = _m(n + G & M64)
    for i in range(8):
        h ^= _m(int.from_bytes(key[8 * i:8 * i + 8], 'little') + (i + 1) * G & M64)
    return _m(h) or 1


def slots_of(wish):
    if wish <= 0 or wish >= DEFAULT_SLOTS:
        return DEFAULT_SLOTS
    c = MIN_SLOTS
    while 2 * c <= wish:
        c *= 2
    return c


def level_of(hashes, slots):
    """the smallest s for which at most slots / 2 of the distinct hashes have s zero low bits"""
    s = 0
    while sum(1 for h in hashes if h & ((1 << s) - 1) == 0) > slots // 2:
        s += 1
    return s


def bin_of(count):
    return max(i for i, lo in enumerate(BOUNDS) if count >= lo)


def dup(text, chunk_off, slots=0):
    """the result array of the duplication with a table of ``slots`` slots (0: the default)"""
    out = np.zeros(D_LEN, dtype=np.int64)
    counts = {}
    for b, _ in lines_of(text, chunk_off):
        if b:
            h = dup_hash(b)
            counts[h] = counts.get(h, 0) + 1
            out[D_KEYED] += 1
        else:
            out[D_UNKEYED] += 1
    C = slots_of(slots)
    s = level_of(counts, C)
    out[D_LEVEL], out[D_SLOTS] = s, C
    for h, n in counts.items():
        if h & ((1 << s) - 1) == 0:
            out[D_DISTINCT + bin_of(n)] += 1; out[D_RECORDS + bin_of(n)] += n
            out[D_TRACKED_KEYS] += 1; out[D_TRACKED_RECORDS] += n
    return out


def check_identities(reads_words, dup_words, profile_words):
    """the identities of the header, against the profile of the same text (another kernel's counts)"""
    n = profile_words[R.RECORDS]
    if reads_words is not None:
        w = reads_words
        assert w.shape == (LEN,) and (w >= 0).all() and (w[3:8] == 0).all()
        assert w[RECORDS] == n == w[GC_NONE] + w[GC:GC + GC_BINS].sum() == w[MEANQ_NONE] + w[MEANQ:MEANQ + 256].sum() == w[NCOUNT:NCOUNT + 256].sum()
    if dup_words is not None:
        d = dup_words
        assert d.shape == (D_LEN,) and (d >= 0).all() and (d[6:8] == 0).all()
        assert d[D_KEYED] + d[D_UNKEYED] == n
        assert d[D_RECORDS:D_RECORDS + 16].sum() == d[D_TRACKED_RECORDS] and d[D_DISTINCT:D_DISTINCT + 16].sum() == d[D_TRACKED_KEYS]
        assert d[D_TRACKED_KEYS] <= d[D_SLOTS] // 2 and (d[D_RECORDS:D_RECORDS + 16] >= d[D_DISTINCT:D_DISTINCT + 16] * np.array(BOUNDS)).all()
        if d[D_LEVEL] == 0:
            assert d[D_TRACKED_RECORDS] == d[D_KEYED]


# ---- the texts -------------------------------------------------------------------------------------------------------

def rec(bases, scores, name=b'r', nl=b'\n'):
    return b'@' + name + nl + bases + nl + b'+' + nl + scores + nl


def _rng_bases(rng, n, alphabet=b'ACGT'):
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n).tobytes()


def _rng_scores(rng, n):
    return rng.randint(33, 127, n).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def rounding_text():
    """GC shares on the exact halves and at the ends (1/8, 3/8, 1/200, 199/200, 0/1, 1/1 -- also with bytes around them that
    are no A C G T), mean scores of exactly x.5, the score bytes 0x7F, 0x80 and 0xFF"""
    t = b''
    for g, a in ((1, 8), (3, 8), (1, 200), (199, 200), (0, 1), (1, 1)):
        t += rec(b'G' * g + b'A' * (a - g), b'I' * a)
        t += rec(b'N' + b'C' * g + b'nacgt.' + b'T' * (a - g) + b'NN', b'5' * (a + 9))
    for s in (b'IJ', b'!"', b'IJ' * 5, b'\x7f\x80', b'\xff', b'\xff' * 300, b'\x7f' * 33, b'\x80' * 65, b'\xfe\xff' * 600, b'!' + b'~' * 1):
        t += rec(b'ACGT', s)
    return t


@functools.lru_cache(maxsize=None)
def nothing_text():
    """nothing to count: an empty bases line, all N, lower case only, an empty score line, both lines ending in '\\r', a line
    that is only '\\r'"""
    return (rec(b'', b'III') + rec(b'NNNNNNNN', b'IIIIIIII') + rec(b'acgtacgt', b'IIIIIIII') + rec(b'ACGT', b'') + rec(b'', b'')
            + rec(b'ACGT\r', b'IIIJ\r') + rec(b'GC' * 40 + b'\r', b'#' * 80 + b'\r') + rec(b'\r', b'II') + rec(b'AC', b'\r') + rec(b'\r', b'\r')
            + rec(b'G' * 1500 + b'\r', b'I' * 1500 + b'\r') + rec(b'\r\r', b'\r\r'))


@functools.lru_cache(maxsize=None)
def ncount_text():
    rng = np.random.RandomState(161)
    t = b''
    for n in (0, 1, 254, 255, 256, 1000):
        b = bytearray(_rng_bases(rng, n + 40))
        for at in rng.permutation(n + 40)[:n]:
            b[at] = ord('N')
        t += rec(bytes(b), _rng_scores(rng, n + 40))
    return t


LENGTHS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 9000)


@functools.lru_cache(maxsize=None)
def lengths_text():
    """lines at the lane and path seams; bases and score lines of different lengths in one record; the counted bytes in the
    first and in the last lane's share alone"""
    rng = np.random.RandomState(162)
    t = b''
    for i, n in enumerate(LENGTHS):
        m = LENGTHS[(i + 5) % len(LENGTHS)]
        t += rec(_rng_bases(rng, n, b'ACGTN'), _rng_scores(rng, n))
        t += rec(_rng_bases(rng, n, b'ACGTNacgt'), _rng_scores(rng, m))
        edge = b'G' + b'a' * (n - 2) + b'C' if n > 1 else b'G'
        t += rec(edge, b'!' * (m - 1) + b'~')
        t += rec(b'n' * (n - 1) + b'N', b'~' + b'!' * (n - 1))
    return t + b'@part\nACGT\n+\nIII'


@functools.lru_cache(maxsize=None)
def keys_text():
    """pairs equal in bytes 0 .. 63 and different at byte 64 (duplicates), pairs different at byte 63 (none); one prefix at
    every length 1 .. 65; a difference in each of the eight words, in the first and in the last byte of a word"""
    rng = np.random.RandomState(163)
    t = b''
    for n in (65, 100, 300, 1500):
        k = _rng_bases(rng, 64)
        t += rec(k + b'A' * (n - 64), b'I' * n) + rec(k + b'C' * (n - 64), b'I' * n)                 # duplicates
        t += rec(k[:63] + b'N' + b'G' * (n - 64), b'I' * n) + rec(k[:63] + b'n' + b'G' * (n - 64), b'I' * n)      # not
    p = _rng_bases(rng, 65)
    for n in range(1, 66):
        t += rec(p[:n], b'I' * n)
    t += rec(p[:64], b'I' * 64) + rec(p[:10] + b'\r', b'I' * 10)              # (64 and 65 bytes are one key; so are 10 and 10 + '\r')
    base = bytearray(_rng_bases(rng, 80))
    for w in range(8):
        for at in (8 * w, 8 * w + 7):
            b = bytearray(base); b[at] = ord('N')
            t += rec(bytes(b), b'I' * 80)
    t += rec(bytes(base), b'I' * 80) * 2
    t += rec(b'A', b'I') + rec(b'A\0', b'II') + rec(b'', b'')              # (a zero byte in the key and the padding: the length tells them apart)
    return t


COPIES = (1, 2, 9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000)


@functools.lru_cache(maxsize=None)
def bins_text():
    """keys with exactly COPIES copies, short records, shuffled"""
    rng = np.random.RandomState(164)
    recs = []
    for i, n in enumerate(COPIES):
        recs += [rec(_rng_bases(rng, 12) + b'ACGT'[i % 4:i % 4 + 1] * (i + 1), b'I' * (13 + i))] * n
    order = rng.permutation(len(recs))
    return b''.join(recs[i] for i in order)


@functools.lru_cache(maxsize=None)
def levels_text(distinct=3000, seed=165):
    """``distinct`` keys, a third of them twice and a few five times, shuffled: with a table of 1024 slots 3000 keys end at
    a level of 2 at least (the reference says so below: checked when the text is built)"""
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(distinct):
        r = rec(_rng_bases(rng, 30), _rng_scores(rng, 30))
        recs += [r] * (5 if i % 50 == 0 else 2 if i % 3 == 0 else 1)
    order = rng.permutation(len(recs))
    text = b''.join(recs[i] for i in order)
    if distinct >= 3000:
        assert dup(text, [0, len(text)], 1024)[D_LEVEL] >= 2
    else:
        assert dup(text, [0, len(text)], 1024)[D_LEVEL] == 0
    return text


def small_texts():
    """name -> text: the texts a few KB small"""
    return {'rounding': rounding_text(), 'nothing': nothing_text(), 'ncount': ncount_text(), 'lengths': lengths_text(), 'keys': keys_text()}
