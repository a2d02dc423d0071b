"""
The profile of a FastQ text (include/kvarq_hip.h) as a plain Python statement of its definition: the
yardstick of tests/test_profile_host.py (the CPU twin) and tests/test_gpu_profile.py (the kernel).

The profile covers the complete four-newline records of every chunk (a partial tail is dropped).  For a record with
newlines n0..n3 the bases line is the bytes strictly between n0 and n1, the score line those strictly between n2 and n3,
raw.  The trim is ``trim_matrix.trim`` (workhorse.c:1055-1068), counted like add_rl (workhorse.c:394-402).
"""
import numpy as np

from trim_matrix import trim

RECORDS, BASE_LINE_BYTES, SCORE_LINE_BYTES, MISMATCHED, LONGEST = 0, 1, 2, 3, 4
SCORE_BYTES, BASE_BYTES, RAW_LENGTHS, RAW_BINS, CUTOFFS, CUT_WORDS = 8, 264, 520, 1025, 1545, 1025
MAX_READLENGTH = 1024
# the cutoffs of the issue: '!' '.' 'I' '~', bytes at the edges of the signed comparison, and one duplicate
CUTOFFS8 = [ord('!'), ord('.'), ord('I'), ord('~'), 0x05, 0x80, 0xFF, ord('.')]


def profile_len(ncut):
    return 8 + 256 + 256 + 1025 + ncut * 1025


def records_of(text, chunk_off):
    """(n0, n1, n2, n3) of every complete record of every chunk"""
    text = bytes(text)
    out = []
    for a, b in zip(chunk_off, chunk_off[1:]):
        nl, at = [], text.find(b'\n', a, b)
        while at >= 0:
            nl.append(at); at = text.find(b'\n', at + 1, b)
        out += [tuple(nl[i:i + 4]) for i in range(0, len(nl) - len(nl) % 4, 4)]
    return out


def profile(text, cutoffs, chunk_off=None, into=None):
    """the flat int64 array; ``into``: add to it (maxima as maxima), as kvq_profile_host does"""
    text = bytes(text)
    if chunk_off is None:
        from oracle import oracle as O
        chunk_off = O.chunk_offsets(text) if text else [0]
    out = np.zeros(profile_len(len(cutoffs)), dtype=np.int64) if into is None else into
    score, base = bytearray(), bytearray()
    trims = {}
    for n0, n1, n2, n3 in records_of(text, [int(c) for c in chunk_off]):
        bases, scores = text[n0 + 1:n1], text[n2 + 1:n3]
        out[RECORDS] += 1
        out[BASE_LINE_BYTES] += len(bases); out[SCORE_LINE_BYTES] += len(scores)
        out[MISMATCHED] += len(bases) != len(scores)
        out[LONGEST] = max(out[LONGEST], len(bases) + 1)
        out[RAW_LENGTHS + min(len(bases), 1024)] += 1
        base += bases; score += scores
        for k, c in enumerate(cutoffs):
            if (scores, c) not in trims:
                trims[scores, c] = trim(scores, c)[1]
            ln = trims[scores, c]
            at = CUTOFFS + k * CUT_WORDS
            if ln < MAX_READLENGTH:
                out[at + 1 + ln] += 1
            out[at] = max(out[at], ln + 1)
    out[SCORE_BYTES:SCORE_BYTES + 256] += np.bincount(np.frombuffer(bytes(score), dtype=np.uint8), minlength=256)
    out[BASE_BYTES:BASE_BYTES + 256] += np.bincount(np.frombuffer(bytes(base), dtype=np.uint8), minlength=256)
    return out


def readlengths(words, k):
    """cutoff k's part in the shape of stats['readlengths']"""
    at = CUTOFFS + k * CUT_WORDS
    return tuple(int(words[at + 1 + i]) if i < MAX_READLENGTH else 0 for i in range(int(words[at])))


def long_counts(text, cutoffs, chunk_off):
    """per cutoff, the records whose trimmed read has 1024 bases and more (in no bin)"""
    text = bytes(text)
    recs = records_of(text, [int(c) for c in chunk_off])
    return [sum(1 for _, _, n2, n3 in recs if n3 - n2 - 1 >= MAX_READLENGTH and trim(text[n2 + 1:n3], c)[1] >= MAX_READLENGTH) for c in cutoffs]


def check_identities(words, ncut, longs=None):
    assert words[RECORDS] == words[RAW_LENGTHS:RAW_LENGTHS + RAW_BINS].sum()
    assert words[SCORE_BYTES:SCORE_BYTES + 256].sum() == words[SCORE_LINE_BYTES]
    assert words[BASE_BYTES:BASE_BYTES + 256].sum() == words[BASE_LINE_BYTES]
    assert (words[5:8] == 0).all()
    for k in range(ncut):
        at = CUTOFFS + k * CUT_WORDS
        assert words[at + 1:at + CUT_WORDS].sum() <= words[RECORDS]
        if longs is not None:
            assert words[at + 1:at + CUT_WORDS].sum() + longs[k] == words[RECORDS]
        if words[at] <= MAX_READLENGTH:                 # no read of 1024 and more at this cutoff: every record is in a bin
            assert words[at + 1:at + CUT_WORDS].sum() == words[RECORDS]
