"""
The emitted reads of a FastQ text (include/kvarq_hip.h) as a plain Python statement of their definition: the
yardstick of tests/test_emit_host.py (the CPU twin) and, through the twin, of tests/test_gpu_emit.py (the kernels).

EMIT(text, chunk_off, amin, min_length) covers the profile's record set (``profile_ref.records_of``).  Per record: the name is
``text[r0:n0]`` less one trailing '\\r' (r0: the byte behind the record in front, or the chunk's first byte), bases and scores are
the raw lines.  Lines of different lengths: dropped, *mismatched*.  Else ``(start, length) = trim_matrix.trim(scores, amin)``;
``length < min_length``: dropped, *short*; else the record is emitted as name, bases[start:start + length], a bare '+',
scores[start:start + length].

The texts, each with a census that is asserted before anything is compared on it:
``copies``  every (source address mod 16, destination address mod 16, length 0 .. 48) of the three pieces a record is copied in;
``trims``   the trim at its seams, the '\\r's, the classes, the line lengths at which the sizing kernel changes its path;
``counts``  record counts at the seams of the prefix sum.
"""
import functools
import random

import numpy as np

import clip_ref as CR
import profile_ref as R
from trim_matrix import trim

N, RECORDS, EMITTED, SHORT, MISMATCHED, BASES_IN, BASES_OUT, BYTES_OUT, LEN = 0, 1, 2, 3, 4, 5, 6, 7, 8
CFG = dict(CR.CFG)                                          # Amin '.', minreadlength 25
AMIN = CR.AMIN
MINLEN = CFG['minreadlength']
SEQ = [b'ACGTACGTACGTACGTACGTACGTA']
SCAN_BLOCK = 256                                            # KVQ_EMIT_SCAN_BLOCK: records a workgroup of the prefix sum takes, and block sums a step of its second level
GOOD, BAD = b'IJHK5/.~', b'#!"-'                            # scores at or above Amin '.', and below it


def per_record(text, chunk_off, amin, min_length):
    """(r0, n0, n1, n2, n3, class, start, length) of every record; class: 'emitted', 'short' or 'mismatched'"""
    text = bytes(text)
    out, trims = [], {}
    for a, b in zip(chunk_off, chunk_off[1:]):
        r0 = int(a)
        for n0, n1, n2, n3 in R.records_of(text, [int(a), int(b)]):
            bases, scores = text[n0 + 1:n1], text[n2 + 1:n3]
            if len(bases) != len(scores):
                out.append((r0, n0, n1, n2, n3, 'mismatched', 0, 0))
            else:
                if scores not in trims:
                    trims[scores] = trim(scores, amin)
                start, length = trims[scores]
                out.append((r0, n0, n1, n2, n3, 'short' if length < min_length else 'emitted', start, length))
            r0 = n3 + 1
    return out


def emit(text, chunk_off, amin=AMIN, min_length=MINLEN, into=None):
    """(EMIT(text) as bytes, the eight words); ``into``: words to add to, as kvq_emit_host does"""
    text = bytes(text)
    w = np.zeros(LEN, dtype=np.int64) if into is None else into
    w[N] = min_length
    parts = []
    for r0, n0, n1, n2, n3, cls, start, length in per_record(text, chunk_off, amin, min_length):
        w[RECORDS] += 1; w[BASES_IN] += n1 - n0 - 1
        if cls != 'emitted':
            w[SHORT if cls == 'short' else MISMATCHED] += 1
            continue
        name = text[r0:n0]
        if name.endswith(b'\r'):
            name = name[:-1]
        rec = name + b'\n' + text[n0 + 1 + start:n0 + 1 + start + length] + b'\n+\n' + text[n2 + 1 + start:n2 + 1 + start + length] + b'\n'
        parts.append(rec)
        w[EMITTED] += 1; w[BASES_OUT] += length; w[BYTES_OUT] += len(rec)
    return b''.join(parts), w


def check_identities(words, text_len=None):
    w = [int(v) for v in words]
    assert w[RECORDS] == w[EMITTED] + w[SHORT] + w[MISMATCHED] and w[BASES_OUT] <= w[BASES_IN]
    assert text_len is None or w[BYTES_OUT] == text_len


def record_ends(text):
    return CR.record_ends(text)


# ---- copies ----------------------------------------------------------------------------------------------------------------------
# A record is copied in three pieces -- name, bases slice, scores slice --, each from an arbitrary address to an arbitrary address:
# the copy kernel's three kinds of store (16 bytes, a dword, a byte) and its two aligned loads depend on both addresses modulo 16
# and on the length.  The text is built record by record so that every cell (piece, source mod 16, destination mod 16, length)
# with 0 <= length <= 48 is there (a name has its '@': 1 .. 48; an empty slice has no source: every destination).  Steering: the name's length moves every later address of the
# record in both texts; `start` (bad scores in front of the run) moves the sources of bases and scores; bad scores behind the run
# and the length of the third line ("+" and what follows it: the emit writes a bare '+') move sources only.  Emitted with
# min_length 0 as ONE chunk in a 16-byte aligned buffer, text offsets are addresses modulo 16.
MAXLEN = 48


def _cells_required():
    req = np.ones((3, 16, 16, MAXLEN + 1), dtype=bool)
    req[0, :, :, 0] = False
    return req


@functools.lru_cache(maxsize=None)
def copies_text():
    """-> (text, the cells (piece, src, dst, len) of its records in order, three a record)"""
    rng = random.Random(2101)
    lens = range(MAXLEN + 1)
    open_name = [[set(range(1, MAXLEN + 1)) for _ in range(16)] for _ in range(16)]       # [src][dst] -> lengths
    open_b = [[set(range(16)) for _ in lens] for _ in range(16)]                          # [dst][len] -> sources
    open_s = [[set(range(16)) for _ in lens] for _ in range(16)]
    left = 16 * 16 * (MAXLEN + 2 * (MAXLEN + 1))
    parts, cells = [], []
    r0 = o = 0
    for _ in range(40000):
        if not left:
            break
        sr, so = r0 % 16, o % 16
        # the name's length: a name cell of this state that is open, and a destination at which a bases cell is
        names = open_name[sr][so]
        nl = max(range(1, MAXLEN + 1), key=lambda n: 2 * (n in names) + any(open_b[(so + n + 1) % 16]))
        db = (so + nl + 1) % 16
        # the run's length: open cells of bases and scores, and a next record whose name has cells open at its destination
        ln = max(lens, key=lambda n: 2 * bool(open_b[db][n]) + 2 * bool(open_s[(db + n + 3) % 16][n]) + any(open_name[x][(o + nl + 2 * n + 5) % 16] for x in range(16)))
        ds = (db + ln + 3) % 16
        sb = min(open_b[db][ln]) if open_b[db][ln] else rng.randrange(16)
        ss = min(open_s[ds][ln]) if open_s[ds][ln] else rng.randrange(16)
        st = (sb - (r0 + nl + 1)) % 16                        # bad scores in front of the run: the source of the bases slice
        no = (o + nl + 2 * ln + 5) % 16
        nr = max(range(16), key=lambda x: len(open_name[x][no]))
        tl = (nr - ss - ln - 1) % 16                          # bad scores behind the run and the third line's extra bytes: the source
        ex = (ss - (r0 + nl + st + ln + tl + 4 + st)) % 16    # of the scores slice, and the next record's first byte
        name = b'@' + bytes(rng.choice(b'abcdefghijklmnopqrstuvwxyz0123456789:/ _') for _ in range(nl - 1))
        L = st + ln + tl
        bases = bytes(rng.choice(b'ACGT') for _ in range(L))
        scores = (bytes(rng.choice(BAD) for _ in range(st)) + bytes(rng.choice(GOOD) for _ in range(ln)) + bytes(rng.choice(BAD) for _ in range(tl)))
        third = b'+' + bytes(rng.choice(b'xyz') for _ in range(ex))
        rec = name + b'\n' + bases + b'\n' + third + b'\n' + scores + b'\n'
        three = [(0, sr, so, nl), (1, (r0 + nl + 1 + st) % 16, db, ln), (2, (r0 + nl + 1 + L + 1 + len(third) + 1 + st) % 16, ds, ln)]
        assert three[1][1] == sb and three[2][1] == ss and (r0 + len(rec)) % 16 == nr
        for (piece, src, dst, n), opened in zip(three, (open_name[sr][so], open_b[db][ln], open_s[ds][ln])):
            if piece and n == 0:                              # (an empty slice has no source: every source of the cell's destination is done)
                left -= len(opened); opened.clear()
            elif (n if piece == 0 else src) in opened:
                opened.discard(n if piece == 0 else src); left -= 1
        cells += three
        parts.append(rec)
        r0 += len(rec); o += nl + 2 * ln + 5
    assert not left, left
    return b''.join(parts), tuple(cells)


def copies_census():
    """every required cell is there -- counted from the text itself, by the plain statement, not from the builder's notes"""
    text, noted = copies_text()
    seen = np.zeros((3, 16, 16, MAXLEN + 1), dtype=bool)
    o = 0
    for r0, n0, n1, n2, n3, cls, start, length in per_record(text, [0, len(text)], AMIN, 0):
        assert cls == 'emitted'
        nl = n0 - r0
        seen[0, r0 % 16, o % 16, nl] = True
        src = slice(None) if length == 0 else None          # (an empty slice has no source)
        seen[1, src if src else (n0 + 1 + start) % 16, (o + nl + 1) % 16, length] = True
        seen[2, src if src else (n2 + 1 + start) % 16, (o + nl + length + 4) % 16, length] = True
        o += nl + 2 * length + 5
    req = _cells_required()
    assert (seen & req).sum() == req.sum() == 16 * 16 * (48 + 49 + 49)
    assert o == len(emit(text, [0, len(text)], AMIN, 0)[0])
    return dict(records=len(noted) // 3, cells=int(req.sum()), bytes=len(text))


# ---- trims -----------------------------------------------------------------------------------------------------------------------
def _rec(name, bases, scores, third=b'+', eol=b'\n'):
    return name + eol + bases + eol + third + eol + scores + eol


def _bases(rng, n):
    return bytes(rng.choice(b'ACGT') for _ in range(n))


@functools.lru_cache(maxsize=None)
def trims_text():
    """-> (text, labels of its records in order); Amin '.', min_length 25 (and 0).  The last record has no final newline: no record"""
    rng = random.Random(2102)
    G, B = b'I', b'#'
    recs, labels = [], []

    def add(label, scores, name=None, bases=None, **kw):
        labels.append(label)
        recs.append(_rec(name if name is not None else b'@t%d %s' % (len(recs), label.encode()), bases if bases is not None else _bases(rng, len(scores)), scores, **kw))
    add('equal-first-wins', G * 30 + B + G * 30)
    add('equal-three', B * 2 + G * 27 + B + G * 27 + B * 3 + G * 27)
    add('later-longer', G * 26 + B + G * 27 + B)
    add('ends-with-line', B * 5 + G * 40)
    add('whole-line', G * 50)
    add('no-good', B * 40)
    add('empty-lines', b'')
    add('exactly-min', B + G * MINLEN + B)
    add('one-short', B + G * (MINLEN - 1) + B)
    add('one-base', B * 3 + G + B * 3)
    # the signed compare: 0x7f is the best score there is, 0x80 and 0xff are below every cutoff above them; Amin itself and the byte below it
    add('wide-bytes', b'\x7f' * 13 + b'\x80' + b'\x7f' * 26 + b'\xff' + b'.' * 27 + b'-' + b'/' * 10)
    add('wide-all-high', b'\x80\xff' * 20)
    # '\r': the name loses one, bases and scores keep theirs -- a low score at Amin '.', which closes the run in front of it
    add('cr-everywhere', G * 30, eol=b'\r\n')
    add('cr-name-only', G * 30, name=b'@cr name\r')
    add('cr-cr-name', G * 30, name=b'@two\r\r')
    add('cr-scores-and-bases', G * 29 + b'\r', bases=_bases(rng, 29) + b'\r')
    add('mismatched-bases-longer', G * 30, bases=_bases(rng, 31))
    add('mismatched-scores-longer', G * 31, bases=_bases(rng, 30))
    add('mismatched-empty-scores', b'', bases=_bases(rng, 30))
    add('empty-name', G * 30, name=b'@')
    add('long-name', G * 30, name=b'@' + bytes(rng.choice(b'abcdefgh ') for _ in range(700)))
    add('third-line-long', G * 30, third=b'+' + b'same name again' * 3)
    # the line lengths at which the sizing kernel changes its path: 256 and 1024 scores
    for q in (255, 256, 257, 1023, 1024, 1025):
        cut = q // 3
        add('q%d' % q, G * cut + B + G * (q - cut - 1))
        add('q%d-ends-with-line' % q, B * (q - cut) + G * cut)
        add('q%d-whole' % q, G * q)
    # a 12 kb line and a line above 64 KiB: equal runs (the first wins), a run across many KiB, a run that ends with the line
    add('hifi-12k', B * 7 + G * 4000 + B + G * 4000 + B * 3 + G * 3989)
    add('hifi-12k-whole', G * 12000)
    add('above-64k', B * 1000 + G * 30000 + B * 5 + G * 39000)
    add('above-64k-no-good', B * 66000)
    text = b''.join(recs) + b'@tail no newline\nACGT\n+\nIIII'
    return text, tuple(labels)


def trims_census():
    text, labels = trims_text()
    for min_length in (MINLEN, 0):
        recs = per_record(text, [0, len(text)], AMIN, min_length)
        assert len(recs) == len(labels)                                    # (the tail without its newline is no record)
        by = {lab: r for lab, r in zip(labels, recs)}

        def got(lab):
            return by[lab][5:]
        assert got('equal-first-wins') == ('emitted', 0, 30) and got('equal-three') == ('emitted', 2, 27) and got('later-longer') == ('emitted', 27, 27)
        assert got('ends-with-line') == ('emitted', 5, 40) and got('whole-line') == ('emitted', 0, 50)
        assert got('exactly-min') == ('emitted', 1, MINLEN)
        short = 'short' if min_length else 'emitted'
        assert got('one-short') == (short, 1, MINLEN - 1) and got('no-good') == (short, 0, 0) and got('empty-lines') == (short, 0, 0)
        assert got('one-base') == (short, 3, 1) and got('wide-all-high') == (short, 0, 0)
        assert got('wide-bytes') == ('emitted', 41, 27)
        assert got('cr-everywhere') == ('emitted', 0, 30) and got('cr-scores-and-bases') == ('emitted', 0, 29)
        for lab in ('mismatched-bases-longer', 'mismatched-scores-longer', 'mismatched-empty-scores'):
            assert got(lab)[0] == 'mismatched'
        assert got('hifi-12k') == ('emitted', 7, 4000) and got('hifi-12k-whole') == ('emitted', 0, 12000)
        assert got('above-64k') == ('emitted', 31005, 39000) and got('above-64k-no-good')[0] == short
        for q in (255, 256, 257, 1023, 1024, 1025):
            cut = q // 3
            assert got('q%d' % q) == ('emitted', cut + 1, q - cut - 1) and got('q%d-ends-with-line' % q) == ('emitted', q - cut, cut) and got('q%d-whole' % q) == ('emitted', 0, q)
    out, w = emit(text, [0, len(text)], AMIN, MINLEN)
    assert b'@cr name\n' in out and b'@two\r\n' in out and b'\n@\n' in out and out.count(b'\r') == 1 and w[MISMATCHED] == 3
    return dict(records=len(labels), bytes=len(text))


# ---- counts ----------------------------------------------------------------------------------------------------------------------
# the seams of the prefix sum: one record; a block less one / exactly / plus one; a block of blocks less one / exactly / plus one
# and well beyond (the second level carries from step to step)
COUNTS = (1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_BLOCK * SCAN_BLOCK - 1, SCAN_BLOCK * SCAN_BLOCK, SCAN_BLOCK * SCAN_BLOCK + 1, 70001)


@functools.lru_cache(maxsize=None)
def _counts_pool():
    """a few hundred distinct records of a few dozen bytes: emitted ones of several sizes, short ones, a mismatched one"""
    rng = random.Random(2103)
    pool = []
    for i in range(389):
        ln = (25, 26, 27, 31, 0, 24)[i % 6]
        st = i % 3
        scores = b'#' * st + bytes(rng.choice(GOOD) for _ in range(ln)) + b'#' * (i % 2)
        bases = _bases(rng, len(scores) + (1 if i % 97 == 5 else 0))
        pool.append(_rec(b'@c%d' % i, bases, scores))
    return tuple(pool)


@functools.lru_cache(maxsize=None)
def counts_text(n):
    pool = _counts_pool()
    return b''.join(pool[(7 * i) % len(pool)] for i in range(n))


def counts_census(n):
    text = counts_text(n)
    recs = R.records_of(text, [0, len(text)])
    assert len(recs) == n and len(text) <= 80 * n
    if n >= 389:
        _, w = emit(text, [0, len(text)], AMIN, MINLEN)
        assert w[EMITTED] > n // 2 and w[SHORT] > n // 4 and w[MISMATCHED] >= n // 400
    return dict(records=n, bytes=len(text))


@functools.lru_cache(maxsize=None)
def dropped_text():
    """every record is dropped at min_length 25: short ones and mismatched ones"""
    rng = random.Random(2104)
    return b''.join(_rec(b'@d%d' % i, _bases(rng, 30 + i % 2), b'I' * 24 + b'#' * 6) for i in range(600))


def dropped_census():
    text = dropped_text()
    out, w = emit(text, [0, len(text)], AMIN, MINLEN)
    assert out == b'' and w[RECORDS] == 600 and w[SHORT] == 300 and w[MISMATCHED] == 300 and w[BYTES_OUT] == 0


def empty_chunk_case():
    """(text, chunk offsets): an empty chunk between two full ones, and one at either end"""
    text = counts_text(SCAN_BLOCK + 1)
    mid = record_ends(text)[99]
    return text, (0, 0, mid, mid, len(text), len(text))
