"""
The overrepresented sequences of a FastQ text (include/kvarq_hip.h) as a plain Python statement of their
definition: the yardstick of tests/test_over_host.py (the CPU twin) and tests/test_gpu_over.py (the kernels).  And the texts
both run on, each aimed at one way the kernels can go wrong.

Records, lines, key and hash are the duplication's (``reads_ref.lines_of``, ``reads_ref.dup_hash``).  The records of a text are
numbered in text order; the candidates are the keys of the keyed records with a number below M; a candidate's count is taken
over the whole text; a candidate is listed when count >= 2 and 1000 count >= keyed.  Two keys with equal hashes would be one
key: ``over`` asserts that no text here holds such a pair.
"""
import functools

import numpy as np

import reads_ref as RR

O_M, O_SLOTS, O_KEYED, O_UNKEYED, O_CANDIDATES, O_COUNTED, O_LISTED, O_ROWS, O_ROW_WORDS, O_MAX_ROWS = 0, 1, 2, 3, 4, 5, 6, 8, 11, 1000
O_LEN = O_ROWS + O_MAX_ROWS * O_ROW_WORDS
DEFAULT_RECORDS, MIN_RECORDS, MAX_RECORDS = 1 << 18, 16, 1 << 22
M64 = (1 << 64) - 1


def records_of(wish):
    """M from a wish (KVQ_OVER_RECORDS, or the twin's argument): 0 and below the default, else clamped"""
    return DEFAULT_RECORDS if wish <= 0 else min(max(wish, MIN_RECORDS), MAX_RECORDS)


def slots_of(M):
    """four times M rounded up to a power of two, at least 1024"""
    c = 1
    while c < M:
        c *= 2
    return max(4 * c, 1024)


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def over(text, chunk_off, records=0):
    """the result array with the first ``records`` records making the candidates (0: the default)"""
    M = records_of(records)
    out = np.zeros(O_LEN, dtype=np.int64)
    out[O_M], out[O_SLOTS] = M, slots_of(M)
    keys, counts, seen = {}, {}, {}
    for number, (b, _) in enumerate(RR.lines_of(text, chunk_off)):
        if not b:
            out[O_UNKEYED] += 1
            continue
        out[O_KEYED] += 1
        key = b[:64]
        h = RR.dup_hash(key)
        assert seen.setdefault(h, key) == key, 'two keys of this text share a hash: not a text for these tests'
        if number < M:
            keys.setdefault(h, key)
        if h in keys:
            counts[h] = counts.get(h, 0) + 1
    out[O_CANDIDATES], out[O_COUNTED] = len(keys), sum(counts.values())
    listed = sorted((h for h, c in counts.items() if c >= 2 and 1000 * c >= out[O_KEYED]), key=lambda h: (-counts[h], h))
    assert len(listed) <= O_MAX_ROWS
    out[O_LISTED] = len(listed)
    for r, h in enumerate(listed):
        key = keys[h]
        padded = key + b'\0' * (64 - len(key))
        row = [_signed(h), counts[h], len(key)] + [_signed(int.from_bytes(padded[8 * i:8 * i + 8], 'little')) for i in range(8)]
        out[O_ROWS + r * O_ROW_WORDS:O_ROWS + (r + 1) * O_ROW_WORDS] = row
    return out


def rows_of(words):
    """[(hash as unsigned, count, key bytes)] of a result array"""
    rows = []
    for r in range(int(words[O_LISTED])):
        row = words[O_ROWS + r * O_ROW_WORDS:O_ROWS + (r + 1) * O_ROW_WORDS]
        rows.append((int(row[0]) & M64, int(row[1]), b''.join((int(w) & M64).to_bytes(8, 'little') for w in row[3:])[:int(row[2])]))
    return rows


def check_identities(words, profile_words, dup=None):
    """the identities of the header: against the profile of the same text (another kernel's counts), and against the duplication of
    the same scan (``Profile.duplication``) where there is one"""
    w = words
    assert w.shape == (O_LEN,) and (w[:O_ROWS] >= 0).all() and w[7] == 0
    assert w[O_KEYED] + w[O_UNKEYED] == profile_words[RR.R.RECORDS]
    assert w[O_COUNTED] <= w[O_KEYED] and w[O_CANDIDATES] <= min(w[O_M], w[O_COUNTED]) and w[O_LISTED] <= O_MAX_ROWS
    if profile_words[RR.R.RECORDS] <= w[O_M]:
        assert w[O_COUNTED] == w[O_KEYED]
    rows = rows_of(w)
    assert not w[O_ROWS + len(rows) * O_ROW_WORDS:].any()
    assert [(-c, h) for h, c, _ in rows] == sorted((-c, h) for h, c, _ in rows) and len({h for h, _, _ in rows}) == len(rows)
    for h, c, key in rows:
        assert c >= 2 and 1000 * c >= w[O_KEYED] and 1 <= len(key) <= 64 and h == RR.dup_hash(key)
    assert sum(c for _, c, _ in rows) <= w[O_COUNTED]
    if dup is not None:
        assert dup['keyed'] == w[O_KEYED] and dup['unkeyed'] == w[O_UNKEYED]
        if dup['level'] == 0 and profile_words[RR.R.RECORDS] <= w[O_M]:
            assert w[O_CANDIDATES] == dup['tracked_distinct']
        if dup['level'] == 0:
            for _, c, _ in rows:            # (every listed key is tracked at level 0: its count lies in a bin that holds a key)
                assert dup['distinct'][RR.bin_of(c)] >= 1


# ---- the texts -------------------------------------------------------------------------------------------------------

def _distinct(rng, n, length=24):
    """n different keys of `length` bases"""
    out = set()
    while len(out) < n:
        out.add(RR._rng_bases(rng, length))
    return sorted(out)


def _shuffled(rng, recs):
    return b''.join(recs[i] for i in rng.permutation(len(recs)))


@functools.lru_cache(maxsize=None)
def threshold_text(keyed, copies, unkeyed=0):
    """`keyed` keyed records: one key `copies` times, every other key once; `unkeyed` records with no key among them (an empty
    bases line, a lone '\\r').  1000 * copies >= keyed decides"""
    rng = np.random.RandomState(1700 + keyed + copies)
    keys = _distinct(rng, keyed - copies + 1)
    recs = [RR.rec(keys[0], b'I' * 24)] * copies + [RR.rec(k, b'I' * 24) for k in keys[1:]]
    recs += [RR.rec(b'', b'II') if i % 2 else RR.rec(b'\r', b'I\r') for i in range(unkeyed)]
    return _shuffled(rng, recs)


@functools.lru_cache(maxsize=None)
def bound_text(nkeys):
    """`nkeys` keys twice each: 1000 keys are all listed (2000 keyed records), of 1001 none is"""
    rng = np.random.RandomState(171)
    return _shuffled(rng, [RR.rec(k, b'5' * 24) for k in _distinct(rng, nkeys)] * 2)


BOUNDARY_M = 64


@functools.lru_cache(maxsize=None)
def boundary_text():
    """for M = 64.  Records 0 .. 62: different keys; record 63: key A; record 64: key B; behind them 200 more of each, shuffled
    among 300 records of other keys -- one of which (record 5's) comes five more times.  A is listed with 201, B is absent"""
    rng = np.random.RandomState(172)
    keys = _distinct(rng, 63 + 2 + 300, 30)
    head, a, b, rest = keys[:63], keys[63], keys[64], keys[65:]
    def r(k): return RR.rec(k, b'I' * len(k))
    tail = [r(a)] * 200 + [r(b)] * 199 + [r(k) for k in rest] + [r(head[5])] * 5
    return b''.join(r(k) for k in head) + r(a) + r(b) + _shuffled(rng, tail), a, b, head[5]


@functools.lru_cache(maxsize=None)
def keys_text():
    """reads_ref's keys twice over, so that every key repeats (every length 1 .. 64, 65 bytes, differences at byte 63 and behind byte
    64, the '\\r' cases, the zero byte, the first and last byte of each of the eight words), and lines of reads_ref.LENGTHS, twice"""
    rng = np.random.RandomState(173)
    t = RR.keys_text() * 2
    for n in RR.LENGTHS:
        t += RR.rec(RR._rng_bases(rng, n, b'ACGTN'), RR._rng_scores(rng, n)) * 2
        t += RR.rec(RR._rng_bases(rng, n) + b'\r', b'I' * n + b'\r') * 2
    return t


@functools.lru_cache(maxsize=None)
def order_text():
    """eight keys five times, five keys three times, three keys twice, forty once: the ties come out in hash order"""
    rng = np.random.RandomState(174)
    keys = _distinct(rng, 56, 40)
    recs = []
    for i, k in enumerate(keys):
        recs += [RR.rec(k, b'I' * 40)] * (5 if i < 8 else 3 if i < 13 else 2 if i < 16 else 1)
    return _shuffled(rng, recs)


@functools.lru_cache(maxsize=None)
def contention_text():
    return RR.rec(b'ACGTTGCA' * 10, b'I' * 80) * 20000


def small_texts():
    """name -> (text, M; 0: the default)"""
    t = {'threshold_%d_%d' % (k, c): (threshold_text(k, c), 0) for k, c in ((2999, 3), (3000, 3), (3001, 3), (2000, 2), (2001, 2), (10, 1))}
    t['threshold_unkeyed'] = (threshold_text(3000, 3, 57), 0)
    t['bound_1000'], t['bound_1001'] = (bound_text(1000), 0), (bound_text(1001), 0)
    t['boundary'], t['boundary_default'] = (boundary_text()[0], BOUNDARY_M), (boundary_text()[0], 0)
    t['keys'], t['order'], t['contention'] = (keys_text(), 0), (order_text(), 0), (contention_text(), 0)
    t['levels'] = (RR.levels_text(), 0)
    return t
