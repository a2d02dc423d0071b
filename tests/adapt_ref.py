"""
The adapter content (include/kvarq_hip.h) in plain Python -- ``bytes.find`` and a loop for the tail --, the
texts that take the GPU kernel and the CPU twin to their seams, and for every text a CENSUS of which seams its records reach:
a test asserts the census before it compares, so a builder that stops reaching a seam fails instead of passing quietly.
Not a test module.
"""
import functools

import numpy as np

import profile_ref as R

MAX_PROBES, MIN_PROBE, MAX_PROBE, T = 8, 8, 32, 6
BLOCKS, BLOCK_WORDS, B_M, B_FIRST, B_BEYOND, B_TAIL, B_FIRST_BINS, B_TAIL_BINS, POSITIONS = 8, 1064, 0, 1, 2, 3, 8, 1032, 1024
CLIP, CLIP_BINS = 8 + 8 * 1064, 1025
LEN = CLIP + CLIP_BINS
A_N, A_RECORDS, A_WITH_FULL, A_TAIL_ONLY = 0, 1, 2, 3


def per_record(text, chunk_off, probes):
    """for every record (start of the bases line, L, [FIRST_k or None], [TAIL_k or None], CLIP, the line ends in '\\r')"""
    text = bytes(text)
    out = []
    for n0, n1, _, _ in R.records_of(text, chunk_off):
        line = text[n0 + 1:n1]
        cr = line.endswith(b'\r')
        if cr:
            line = line[:-1]                                  # a trailing '\r' is not part of its line
        L = len(line)
        firsts, tails, clip = [], [], L
        for probe in probes:
            p = line.find(probe)
            first, tail = (p if p >= 0 else None), None
            if first is None:
                for t in range(min(len(probe) - 1, L), T - 1, -1):
                    if line[L - t:] == probe[:t]:
                        tail = t
                        break
            firsts.append(first); tails.append(tail)
            if first is not None:
                clip = min(clip, first)
            elif tail is not None:
                clip = min(clip, L - tail)
        out.append((n0 + 1, L, firsts, tails, clip, cr))
    return out


def adapt(text, chunk_off, probes, into=None):
    """the flat int64 array; ``into``: add to it, as kvq_adapt_host does"""
    assert 1 <= len(probes) <= MAX_PROBES and all(MIN_PROBE <= len(p) <= MAX_PROBE and not p.strip(b'ACGT') for p in probes)
    w = np.zeros(LEN, dtype=np.int64) if into is None else into
    w[A_N] = len(probes)
    for k, probe in enumerate(probes):
        w[BLOCKS + k * BLOCK_WORDS + B_M] = len(probe)
    for _, L, firsts, tails, clip, _ in per_record(text, chunk_off, probes):
        w[A_RECORDS] += 1
        for k in range(len(probes)):
            blk = BLOCKS + k * BLOCK_WORDS
            if firsts[k] is not None:
                w[blk + B_FIRST] += 1
                w[blk + (B_FIRST_BINS + firsts[k] if firsts[k] < POSITIONS else B_BEYOND)] += 1
            elif tails[k] is not None:
                w[blk + B_TAIL] += 1
                w[blk + B_TAIL_BINS + tails[k]] += 1
        if any(f is not None for f in firsts):
            w[A_WITH_FULL] += 1
        elif any(t is not None for t in tails):
            w[A_TAIL_ONLY] += 1
        w[CLIP + min(clip, CLIP_BINS - 1)] += 1
    return w


def check_identities(w, profile_words=None):
    n = int(w[A_N])
    assert 1 <= n <= MAX_PROBES and not w[4:8].any()
    for k in range(MAX_PROBES):
        blk = w[BLOCKS + k * BLOCK_WORDS:BLOCKS + (k + 1) * BLOCK_WORDS]
        if k >= n:
            assert not blk.any()
            continue
        m = int(blk[B_M])
        assert MIN_PROBE <= m <= MAX_PROBE and not blk[4:8].any()
        first, tail = blk[B_FIRST_BINS:B_FIRST_BINS + POSITIONS], blk[B_TAIL_BINS:B_TAIL_BINS + 32]
        assert first.sum() + blk[B_BEYOND] == blk[B_FIRST] and tail.sum() == blk[B_TAIL]
        assert not tail[:T].any() and not tail[m:].any()
    assert w[CLIP:CLIP + CLIP_BINS].sum() == w[A_RECORDS] and w[A_WITH_FULL] + w[A_TAIL_ONLY] <= w[A_RECORDS]
    if profile_words is not None:
        assert w[A_RECORDS] == profile_words[R.RECORDS]


# ---- the texts ---------------------------------------------------------------------------------------------------------------
# every probe below starts with A or G and the filler holds only C and T: a filler byte is no start of a match or of a tail, so
# a record matches where its builder planted something and nowhere else
P8, P12, P16, P31, P32 = b'AGGTCATC', b'AGATCGGAAGAG', b'AGATCGGAAGAGCACA', b'GATCGTCGGACTGTAGAACTCTGAACGTGTA', b'AATGATACGGCGACCACCGAGATCTACACTCT'
PERIODIC = b'AGAGAGAGTTCC'
POLY_A = b'AAAAAAAA'
EIGHT = [P8, P12, P31, P32, b'GGAATTCTCGGG', b'ACTGTCTCTTATACACATCT', POLY_A, PERIODIC]


def filler(rng, n):
    return rng.choice(np.frombuffer(b'CT', dtype=np.uint8), n).tobytes() if n > 0 else b''


def rec(bases, name=b'r', nl=b'\n', scores=None):
    return b'@' + name + nl + bases + nl + b'+' + nl + (b'I' * len(bases) if scores is None else scores) + nl


def planted(rng, p, probe, behind=20):
    return filler(rng, p) + probe + filler(rng, behind)


def every_start_text():
    """every FIRST in 0 .. 40 x every residue modulo 16 of the address of the bases line (the name line's length sets it)"""
    rng = np.random.RandomState(18)
    out, at = [], 0
    for p in range(41):
        for r in range(16):
            nlen = (r - at - 2) % 16 or 16                      # '@' + name + '\n' in front of the bases line
            out.append(rec(planted(rng, p, P12), name=b'n' * nlen))
            at += len(out[-1])
    return b''.join(out), [P12, P32]


def edges_text():
    rng = np.random.RandomState(19)
    m, out = len(P12), []
    for L in (40, 150, 300):
        out += [rec(planted(rng, 0, P12, L - m)), rec(planted(rng, L - m, P12, 0))]           # p = 0, p = L - m
    out += [rec(P12), rec(P12[:m - 1]), rec(b''), rec(P12[:T - 1]), rec(b'C'), rec(P32), rec(P32[:31])]   # L = m, m - 1, 0, < T
    for S in (224, 256, 448, 512, 672, 768):                                                  # the seams of the rounds, whatever their stride
        for probe in (P12, P32):
            for p in (S - len(probe) - 1, S - len(probe), S - len(probe) + 1, S - 17, S - 16, S - 15, S - 1, S, S + 1):
                out.append(rec(planted(rng, p, probe, 40)))
    out += [rec(planted(rng, 1023, P12)), rec(planted(rng, 1024, P12)), rec(planted(rng, 1023, P32)), rec(planted(rng, 1500, P32))]
    out.append(rec(planted(rng, 11000, P12, 1000 - m) + P12 + filler(rng, 100)))             # 12 kb, its first match at 11 000
    out.append(rec(filler(rng, 12000)))
    return b''.join(out), [P12, P32]


def cr_text():
    rng = np.random.RandomState(20)
    out = []
    for L in (30, 150, 260):
        out += [rec(planted(rng, L - 12, P12, 0), nl=b'\r\n'), rec(filler(rng, L - 8) + P12[:8], nl=b'\r\n'), rec(filler(rng, L), nl=b'\r\n'),
                rec(planted(rng, L - 32, P32, 0) if L >= 32 else P32[:L], nl=b'\r\n')]
    out += [rec(b'', nl=b'\r\n'), rec(P12, nl=b'\r\n'), rec(P12[:7], nl=b'\r\n')]
    return b''.join(out), [P12, P32]


def several_text():
    rng = np.random.RandomState(21)
    out = [rec(planted(rng, 10, P12, 30) + P12 + filler(rng, 5)),                             # twice: the first one counts
           rec(b'A' * 50), rec(filler(rng, 5) + b'A' * 20 + filler(rng, 9)), rec(filler(rng, 40) + b'A' * 7), rec(filler(rng, 40) + b'A' * 6),
           rec(planted(rng, 33, P16)),                                                       # P12 is a prefix of P16: both at 33
           rec(planted(rng, 33, P12)),                                                       # ... and P12 alone
           rec(planted(rng, 60, P12, 10) + P32 + filler(rng, 3)), rec(planted(rng, 5, P32, 10) + P12)]   # different positions: the smaller
    return b''.join(out) * 3, [P12, P16, POLY_A, P32]


def tails_text():
    rng = np.random.RandomState(22)
    out = []
    for L in (20, 150, 270):
        out += [rec(filler(rng, L - t) + P12[:t]) for t in range(T - 1, len(P12))]            # t = T - 1 (none), T .. m - 1
        out += [rec(filler(rng, L - t) + P32[:t]) for t in (T - 1, T, 15, 16, 17, 30, 31)]
        out.append(rec(filler(rng, L - 8) + PERIODIC[:8]))                                    # AGAGAGAG: t = 6 matches too, 8 counts
        out.append(rec(planted(rng, 3, P32, L - 45) + P12[:9]))                               # a tail of one beside a full match of another
        out.append(rec(planted(rng, 2, P12, L - 22) + P12[:8]))                               # its own full occurrence elsewhere: no tail
    out += [rec(P12[:7]), rec(P12[:6]), rec(P12[1:7]), rec(b'C' + P12[:7]), rec(P32[:10])]    # a tail as long as the line; none longer
    return b''.join(out), [P12, P32, PERIODIC]


def alias(probe, i, how):
    b = probe[i]
    new = {'lower': b | 0x20, 'N': ord('N'), 'dot': ord('.'), 'high': b | 0x80}[how]
    return probe[:i] + bytes([new]) + probe[i + 1:]


def aliases_text():
    """one base of an otherwise full match (or tail) is another byte with the same 2-bit code, or any other: no match anywhere"""
    rng = np.random.RandomState(23)
    out = []
    for probe in (P12, P32):
        g = [i for i in range(len(probe)) if probe[i] == ord('G')]
        for how in ('lower', 'N', 'dot', 'high'):
            for i in ({0, len(probe) // 2, len(probe) - 1} if how != 'N' else {g[0], g[-1]}):
                out.append(rec(planted(rng, 7, alias(probe, i, how), 30)))
                if i < 10:
                    out.append(rec(filler(rng, 50) + alias(probe[:10], i, how)))
    return b''.join(out) * 2, [P12, P32]


def shapes_text():
    rng = np.random.RandomState(24)
    out = []
    for k, probe in enumerate(EIGHT):
        out += [rec(planted(rng, 3 + 17 * k, probe)), rec(planted(rng, 250 - k, probe)), rec(filler(rng, 100 + k) + probe[:7])]
    out.append(rec(b''.join(EIGHT)))
    return b''.join(out) * 2, EIGHT


def none_text():
    """no match at all, no '\\r': clip is the profile's raw_lengths"""
    rng = np.random.RandomState(25)
    return b''.join(rec(filler(rng, L)) for L in list(range(0, 300, 7)) + [1023, 1024, 1025, 3000]), [P12, P32]


def end_text():
    """the last record of the text ends the buffer: a match flush with the end of its bases line, and as little behind it as a record can have"""
    rng = np.random.RandomState(26)
    return b''.join(rec(planted(rng, p, P12, 0)) for p in (0, 30, 140)) + rec(planted(rng, 100, P32, 0), scores=b''), [P12, P32]


def split_text():
    """a probe cut in two by a record's end: a line of exactly 256 bases -- one round of the search's sixteen lanes -- ends with the
    first h bases of P32 and the NEXT record's line begins with the rest.  A tail of h and never a full occurrence, whatever a lane
    takes from the quarter-wave beside its own (the pairs lie in quarters 0 and 1 or 2 and 3 of one wave)"""
    rng = np.random.RandomState(28)
    out = []
    for h in range(16, 32):
        out += [rec(filler(rng, 256 - h) + P32[:h]), rec(P32[h:] + filler(rng, 40))]
    return b''.join(out), [P12, P32]


@functools.lru_cache(maxsize=None)
def texts():
    return {'split': split_text(), 'every_start': every_start_text(), 'edges': edges_text(), 'cr': cr_text(), 'several': several_text(), 'tails': tails_text(),
            'aliases': aliases_text(), 'shapes': shapes_text(), 'none': none_text(), 'end': end_text()}


@functools.lru_cache(maxsize=None)
def random_text(nrec=2000, seed=27):
    """random records over A C G T N with planted probes, whole or cut off by the line's end (accidental matches welcome)"""
    rng = np.random.RandomState(seed)
    probes, out = [P12, b'TGGAATTCTCGG', P8, P32], []
    for i in range(nrec):
        L = int(rng.choice([0, 5, 36, 75, 150, 151, 250, 600]))
        line = bytearray(rng.choice(np.frombuffer(b'ACGTACGTACGTACGTN', dtype=np.uint8), L).tobytes())
        for _ in range(int(rng.randint(0, 3))):
            probe, p = probes[rng.randint(len(probes))], int(rng.randint(0, L + 1))
            line[p:p + len(probe)] = probe[:max(L - p, 0)]
        out.append(rec(bytes(line[:L]), nl=b'\r\n' if i % 50 == 0 else b'\n'))
    return b''.join(out), probes


@functools.lru_cache(maxsize=None)
def census(name):
    """which seams the records of a text reach"""
    text, probes = texts()[name]
    c = dict(first=set(), tail=set(), L=set(), start16=set(), cr_full=0, cr_tail=0, cr_L=set(), both=0, tail_beside_full=0, matched=0, longest_first=-1)
    for start, L, firsts, tails, clip, cr in per_record(text, [0, len(text)], probes):
        c['L'].add(L)
        for k in range(len(probes)):
            if firsts[k] is not None:
                c['first'].add((k, firsts[k])); c['start16'].add((firsts[k], start % 16)); c['longest_first'] = max(c['longest_first'], firsts[k])
            if tails[k] is not None:
                c['tail'].add((k, tails[k]))
        full, tailed = any(f is not None for f in firsts), any(t is not None for t in tails)
        c['matched'] += full or tailed
        c['both'] += sum(f is not None for f in firsts) >= 2
        c['tail_beside_full'] += full and tailed
        if cr:
            c['cr_full'] += full; c['cr_tail'] += tailed and not full; c['cr_L'].add(L)
    c['last_flush'] = per_record(text, [0, len(text)], probes)[-1][2:4] if text else None
    return c


def check_census(name):
    c = census(name)
    text, probes = texts()[name]
    firsts = {p for _, p in c['first']}
    if name == 'every_start':
        assert c['start16'] >= {(p, r) for p in range(41) for r in range(16)}
    elif name == 'edges':
        assert {0, 12, 11, T - 1, 32, 31} <= c['L'] and {(0, 0), (0, 28), (0, 138), (0, 288), (1, 0)} <= c['first']
        for S in (224, 256, 448, 512, 672, 768):
            for k, m in ((0, 12), (1, 32)):
                assert {(k, p) for p in (S - m - 1, S - m, S - m + 1, S - 17, S - 16, S - 15, S - 1, S, S + 1)} <= c['first']
        assert {(0, 1023), (0, 1024), (1, 1023), (1, 1500), (0, 11000)} <= c['first'] and max(c['L']) >= 12000
        assert (0, 11) in c['tail'] and (1, 31) in c['tail']              # L = m - 1: the line is a tail
    elif name == 'cr':
        assert c['cr_full'] >= 6 and c['cr_tail'] >= 4 and {0, 12, 7, 30, 150, 260} <= c['cr_L']
    elif name == 'several':
        assert {(0, 10), (2, 0), (2, 5), (0, 33), (1, 33), (0, 60), (3, 5)} <= c['first'] and {(2, 7), (2, 6)} <= c['tail'] and c['both'] >= 3
    elif name == 'tails':
        assert {(0, t) for t in range(T, 12)} | {(1, t) for t in (T, 15, 16, 17, 30, 31)} | {(2, 8)} <= c['tail']
        assert (0, T - 1) not in c['tail'] and (2, 6) not in c['tail'] and c['tail_beside_full'] >= 3 and {6, 7, 8, 10} <= c['L']
    elif name in ('aliases', 'none'):
        assert c['matched'] == 0 and len(c['L']) >= 2
    elif name == 'shapes':
        assert sorted(len(p) for p in probes)[:1] == [8] and {8, 12, 31, 32} <= {len(p) for p in probes} and len(probes) == 8
        assert {k for k, _ in c['first']} == set(range(8)) and {k for k, _ in c['tail']} >= {0, 1, 2, 3}
    elif name == 'split':
        assert {(1, h) for h in range(16, 32)} == c['tail'] and not c['first'] and c['matched'] == 16 and 256 in c['L'] and len(c['L']) == 17
    elif name == 'end':
        assert text.endswith(b'\n+\n\n') and c['last_flush'][0][1] == 100 and 100 + 32 == sorted(c['L'])[-2]
    return c
