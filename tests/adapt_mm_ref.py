"""
Adapter probes that tolerate mismatches (include/kvarq_hip.h) in plain Python -- a Hamming loop over
``profile_ref.records_of`` --, the texts that take the GPU kernels and the CPU twins to the seams of the rule, and for every text
a CENSUS, asserted before any comparison: every builder writes down what it planted and what the definition must make of it, and
the census holds the plain statement to that.  ``per_record`` and what is built on it take ``wrong=``, one of the WRONG statements
of the rule (``MUTATIONS``): each is visible on the text named beside it (tests/test_adapt_mm_host.py asserts that; the list is
also profiles/adapt_mm_tests.txt).  Not a test module.
"""
import functools
import operator

import numpy as np

import adapt_ref as A
import profile_ref as R

PER, B_DIST, CLIP_PER = 4, 4, 5                             # adapters array [4], its blocks' +4 .. +7, clip array [5]
MIN_PER, MAX_PER = 10, 32
C_N, C_RECORDS, C_CLIPPED, C_MASKED, C_BASES_CUT, C_LEN = 0, 1, 2, 3, 4, 8

# a wrong statement of the rule -> (the text whose result it changes, the words of the adapters array that differ there at per = 10)
MUTATIONS = {'overhang': ('overhang', 35),                        # a window that hangs over the line's end accepted
             'tail_Em': ('tails', 20),                            # E(m_k) used for tails
             'alias': ('kinds', 51),                              # a 2-bit alias taken for a match
             'lt': ('budget/0', 150),                              # < for <=
             'drop31': ('budget/1', 34),                          # base 31 of a 32-base window dropped
             'fewest': ('earliest', 39),                          # fewest mismatches instead of smallest p
             'exact_tail': ('tails', 4),                          # an exact shorter tail preferred
             'tail_beside_first': ('tails', 2),                   # a tail counted beside a tolerant FIRST
             'cr_base': ('overhang', 31)}                         # '\r' counted as a base


def E(n, per):
    return n // per if per else 0


def ham(a, b, wrong=None):
    assert len(a) == len(b)
    if wrong == 'alias':
        return sum(((x >> 1) & 3) != ((y >> 1) & 3) for x, y in zip(a, b))
    if wrong == 'drop31':
        a, b = a[:31], b[:31]
    return sum(map(operator.ne, a, b))


def per_record(text, chunk_off, probes, per, wrong=None):
    """for every record (start of the bases line, L, [FIRST_k or None], [TAIL_k or None], CLIP, the line ends in '\\r', [DIST_k or None])"""
    assert per == 0 or MIN_PER <= per <= MAX_PER
    assert wrong is None or wrong in MUTATIONS
    text = bytes(text)
    out = []

    def within(d, n):
        return d < E(n, per) if wrong == 'lt' else d <= E(n, per)
    for n0, n1, _, _ in R.records_of(text, [int(c) for c in chunk_off]):
        line = text[n0 + 1:n1]
        cr = line.endswith(b'\r')
        if cr and wrong != 'cr_base':
            line = line[:-1]                                  # a trailing '\r' is not part of its line
        L = len(line)
        hay = line + (text[n0 + 1 + L:n0 + 1 + L + 32] + bytes(32))[:32]       # (what lies behind the line: only 'overhang' looks at it)
        firsts, tails, dists, clip = [], [], [], L
        for probe in probes:
            m = len(probe)
            first = dist = tail = None
            for p in range(L if wrong == 'overhang' else max(L - m + 1, 0)):  # the window lies inside the line: p + m <= L
                d = ham(hay[p:p + m], probe, wrong)
                if within(d, m) and (first is None or (wrong == 'fewest' and d < dist)):
                    first, dist = p, d
                    if wrong != 'fewest':
                        break                                 # the smallest p, not the p with the fewest mismatches
            exact_first = line.find(probe) >= 0
            if first is None or (wrong == 'tail_beside_first' and not exact_first):
                cand = [t for t in range(min(m - 1, L), A.T - 1, -1)
                        if (ham(line[L - t:], probe[:t], wrong) < E(m, per) + 1 if wrong == 'tail_Em' else within(ham(line[L - t:], probe[:t], wrong), t))]
                if wrong == 'exact_tail' and any(line[L - t:] == probe[:t] for t in cand):
                    cand = [t for t in cand if line[L - t:] == probe[:t]]
                tail = cand[0] if cand else None              # the largest t, E of t
            firsts.append(first); tails.append(tail); dists.append(dist)
            if first is not None:
                clip = min(clip, first)
            if tail is not None:
                clip = min(clip, L - tail)
        out.append((n0 + 1, L, firsts, tails, clip, cr, dists))
    return out


def adapt(text, chunk_off, probes, per, into=None, wrong=None):
    """the flat int64 array of the adapter content under ``per``; ``into``: add to it, as kvq_adapt_host_mm does"""
    assert 1 <= len(probes) <= A.MAX_PROBES and all(A.MIN_PROBE <= len(p) <= A.MAX_PROBE and not p.strip(b'ACGT') for p in probes)
    w = np.zeros(A.LEN, dtype=np.int64) if into is None else into
    w[A.A_N] = len(probes)
    if per:
        w[PER] = per
    for k, probe in enumerate(probes):
        w[A.BLOCKS + k * A.BLOCK_WORDS + A.B_M] = len(probe)
    for _, L, firsts, tails, clip, _, dists in per_record(text, chunk_off, probes, per, wrong):
        w[A.A_RECORDS] += 1
        for k in range(len(probes)):
            blk = A.BLOCKS + k * A.BLOCK_WORDS
            if firsts[k] is not None:
                w[blk + A.B_FIRST] += 1
                w[blk + (A.B_FIRST_BINS + firsts[k] if firsts[k] < A.POSITIONS else A.B_BEYOND)] += 1
                if per:
                    w[blk + B_DIST + dists[k]] += 1
            if tails[k] is not None:                          # (beside a FIRST_k only under wrong='tail_beside_first')
                w[blk + A.B_TAIL] += 1
                w[blk + A.B_TAIL_BINS + tails[k]] += 1
        if any(f is not None for f in firsts):
            w[A.A_WITH_FULL] += 1
        elif any(t is not None for t in tails):
            w[A.A_TAIL_ONLY] += 1
        w[A.CLIP + min(clip, A.CLIP_BINS - 1)] += 1
    return w


def mask(text, chunk_off, probes, per, into=None, wrong=None):
    """(MASK_per(text), the eight words); ``into``: add to them, as kvq_clip_host_mm does"""
    text = bytes(text)
    co = [int(c) for c in chunk_off]
    out = bytearray(text)
    w = np.zeros(C_LEN, dtype=np.int64) if into is None else into
    w[C_N] = len(probes)
    if per:
        w[CLIP_PER] = per
    for (_, _, n2, n3), (_, L, _, _, clip, _, _) in zip(R.records_of(text, co), per_record(text, co, probes, per, wrong)):
        S = n3 - n2 - 1
        if S and text[n3 - 1] == 13:
            S -= 1                                            # a trailing '\r' is not part of its line
        w[C_RECORDS] += 1
        if clip < L:
            w[C_CLIPPED] += 1; w[C_MASKED] += max(0, S - clip); w[C_BASES_CUT] += L - clip
            if S > clip:
                out[n2 + 1 + clip:n2 + 1 + S] = b'!' * (S - clip)
    return bytes(out), w


def check_identities(w):
    """what holds of the adapters array with per > 0"""
    n, per = int(w[A.A_N]), int(w[PER])
    assert 1 <= n <= A.MAX_PROBES and MIN_PER <= per <= MAX_PER and not w[5:8].any()
    for k in range(A.MAX_PROBES):
        blk = w[A.BLOCKS + k * A.BLOCK_WORDS:A.BLOCKS + (k + 1) * A.BLOCK_WORDS]
        if k >= n:
            assert not blk.any()
            continue
        m = int(blk[A.B_M])
        first, tail = blk[A.B_FIRST_BINS:A.B_FIRST_BINS + A.POSITIONS], blk[A.B_TAIL_BINS:A.B_TAIL_BINS + 32]
        assert first.sum() + blk[A.B_BEYOND] == blk[A.B_FIRST] and tail.sum() == blk[A.B_TAIL]
        assert blk[B_DIST:B_DIST + 4].sum() == blk[A.B_FIRST] and not blk[B_DIST + E(m, per) + 1:B_DIST + 4].any()
        assert not tail[:A.T].any() and not tail[m:].any()
    assert w[A.CLIP:A.CLIP + A.CLIP_BINS].sum() == w[A.A_RECORDS] and w[A.A_WITH_FULL] + w[A.A_TAIL_ONLY] <= w[A.A_RECORDS]


# ---- the texts ---------------------------------------------------------------------------------------------------------------
# probes of 8, 9, 10, 12, 19, 20, 29, 30, 31 and 32 bases: E = 0, 0, 1, 1, 1, 2, 2, 3, 3, 3 at per = 10 -- both sides of every step.
# Each starts with A or G and holds A and G enough that the C/T filler is nowhere within its budget.
P8, P12, P16, P31, P32 = A.P8, A.P12, A.P16, A.P31, A.P32
P9, P10, P19 = b'GAAGTGCAG', b'ACGAGGTAAC', b'GTGACTGGAGTTCAGACGT'
P20, P29, P30 = b'ACTGTCTCTTATACACATCT', b'GTTCGTCTTCTGCCGTATGCTCTAGCACT', b'AGACGTGTGCTCTTCCGATCTGAAGGTACA'
LO, HI = [P8, P9, P10, P12, P19], [P20, P29, P30, P31, P32]
PER2 = b'AGAGAGAGAGAT'                                        # periodic: the window two bases early is one mismatch away
assert [len(p) for p in LO + HI] == [8, 9, 10, 12, 19, 20, 29, 30, 31, 32]
rec, filler = A.rec, A.filler


def other_base(b):
    return b'CGTA'[b'ACGT'.index(bytes([b]))]


def wrong_byte(b, how):
    return {'base': other_base(b), 'N': ord('N'), 'lower': b | 0x20, 'dot': ord('.'), 'high': b | 0x80}[how]


def subst(probe, at, how='base'):
    s = bytearray(probe)
    for i in at:
        s[i] = wrong_byte(probe[i], how)
    assert ham(bytes(s), probe) == len(set(at))
    return bytes(s)


class _Text(object):
    """records with the start of their bases line on a chosen residue modulo 16 (``every_start_text``'s trick with the name's
    length), and what their builder expects of them: per record {k: (FIRST_k or None, DIST_k)} and {k: TAIL_k or None}"""

    def __init__(self, seed, probes):
        self.rng, self.probes, self.parts, self.at, self.want = np.random.RandomState(seed), probes, [], 0, []

    def add(self, bases, firsts=None, tails=None, nl=b'\n', residue=None):
        residue = len(self.parts) % 16 if residue is None else residue
        nlen = (residue - self.at - 2) % 16 or 16            # '@' + name + nl in front of the bases line
        if len(nl) == 2:
            nlen = (residue - self.at - 3) % 16 or 16
        r = rec(bases, name=b'n' * nlen, nl=nl)
        assert (self.at + 1 + nlen + len(nl)) % 16 == residue
        self.parts.append(r); self.at += len(r); self.want.append((firsts or {}, tails or {}))

    def plant(self, p, what, behind=40):
        return filler(self.rng, p) + what + filler(self.rng, behind)

    def done(self, pers=(10,)):
        return b''.join(self.parts), list(self.probes), tuple(pers), tuple(self.want)


SEAMS = (15, 16, 223, 224, 447, 448, 31, 32, 239, 240, 0, 7)  # line positions either side of lane seams and round seams


def budget_text(probes, seed):
    """every probe with exactly E and exactly E + 1 substitutions: at base 0, m - 1, the bases on window offsets 15 / 16 and 31,
    the first of them on a line position of SEAMS; every residue of the first address"""
    b = _Text(seed, probes)
    i = 0
    for k, probe in enumerate(probes):
        m, e = len(probe), E(len(probe), 10)
        offs = sorted({0, m - 1, m // 2} | {o for o in (15, 16, 31) if o < m})
        for nsub in (e, e + 1):
            for r in range(len(offs) if nsub else 2):
                at = sorted(offs[(r + j) % len(offs)] for j in range(nsub))
                s = SEAMS[i % len(SEAMS)]; i += 1
                p = max(s - (at[0] if at else 0), 0)
                b.add(b.plant(p, subst(probe, at)), {k: (p, nsub) if nsub <= e else (None, None)})
    for s in SEAMS[:10]:                                      # every seam under a substitution, within the budget and one over it
        for k, probe in enumerate(probes):
            m, e = len(probe), E(len(probe), 10)
            for nsub in ((e, e + 1) if e else ()):
                at = sorted([m // 2, m - 1, 0, m // 3][:nsub])
                p = s - at[0]
                b.add(b.plant(p, subst(probe, at)), {k: (p, nsub) if nsub <= e else (None, None)})
    for residue in range(16):                                 # every residue of the first address, with the budget used up
        k = residue % len(probes)
        m, e = len(probes[k]), E(len(probes[k]), 10)
        b.add(b.plant(residue + 1, subst(probes[k], [m - 1, 0, m // 2][:e])), {k: (residue + 1, e)}, residue=residue)
    return b.done()


def kinds_text():
    """the same with the wrong byte being another base, 'N' (also in place of a 'G'), the lower-case letter, '.' and the byte | 0x80"""
    probes = [P8, P12, P20, P32]
    b = _Text(31, probes)
    for k, probe in enumerate(probes):
        m, e = len(probe), E(len(probe), 10)
        g = [i for i in range(m) if probe[i] == ord('G')]
        spread = [0, m - 1, m // 2, m // 3]
        for how in ('base', 'N', 'N_for_G', 'lower', 'dot', 'high'):
            pool = g if how == 'N_for_G' else spread
            for nsub in (e, e + 1):
                if nsub == 0 or nsub > len(pool):
                    continue
                p = 5 + 3 * len(b.parts) % 29
                b.add(b.plant(p, subst(probe, pool[:nsub], 'N' if how == 'N_for_G' else how)), {k: (p, nsub) if nsub <= e else (None, None)})
    return b.done()


def overhang_text():
    """lines that end with probe[:m - j], j = 1 .. E + 1, bare and with '\\r\\n', and pairs whose next record begins with the
    rest: never a FIRST, TAIL = m - j"""
    probes = [P8, P12, P20, P32]
    b = _Text(32, probes)
    for k, probe in enumerate(probes):
        m, e = len(probe), E(len(probe), 10)
        for j in range(1, e + 2):
            for nl in (b'\n', b'\r\n'):
                for L in (m - j, 40 + m, 256):
                    b.add(filler(b.rng, L - (m - j)) + probe[:m - j], {k: (None, None)}, {k: m - j}, nl=nl)
            # the pair lies in two neighbouring quarters of one wave (an even record and the one behind it)
            if len(b.parts) % 2:
                b.add(filler(b.rng, 30))
            b.add(filler(b.rng, 256 - (m - j)) + probe[:m - j], {k: (None, None)}, {k: m - j})
            b.add(probe[m - j:] + filler(b.rng, 40), {k: (None, None)})
    return b.done()


def earliest_text():
    probes = [P12, P16, PER2]
    b = _Text(33, probes)
    for p in (0, 9, 100, 215, 230):
        # a one-mismatch occurrence in front of an exact one: FIRST is the earlier, DIST 1
        b.add(b.plant(p, subst(P12, [4]) + filler(b.rng, 7) + P12), {0: (p, 1)})
        # the periodic probe: exact at p + 2, within budget at p
        b.add(b.plant(p, b'AG' + PER2), {2: (p, 1)})
        # P12 is P16's prefix: a mismatch in the shared part, in P16's own part, and one in each
        b.add(b.plant(p, subst(P16, [3])), {0: (p, 1), 1: (p, 1)})
        b.add(b.plant(p, subst(P16, [13])), {0: (p, 0), 1: (p, 1)})
        b.add(b.plant(p, subst(P16, [3, 13])), {0: (p, 1), 1: (None, None)})
    return b.done()


def tails_text():
    probes = [P32, P12, PER2]
    b = _Text(34, probes)
    for t in (9, 10, 19, 20, 29, 30, 31):
        e = E(t, 10)
        offs = [0, t - 1, t // 2, t // 3]                     # the tail's first byte, the line's last byte, two between
        for nsub in (e, e + 1):
            for r in range(2):
                at = [offs[(r + j) % 4] for j in range(nsub)]
                for L in (t + 30, 250):
                    b.add(filler(b.rng, L - t) + subst(P32[:t], at), {0: (None, None)}, {0: t} if nsub <= e else {0: ('not', t)})
    # a t whose shorter suffix matches exactly: the larger t wins (t = 10 with one mismatch, t = 8 exact)
    b.add(filler(b.rng, 30) + b'CGAGAGAGAG', {2: (None, None)}, {2: 10})
    # t = L, exact and with its one mismatch
    b.add(P32[:10], {0: (None, None)}, {0: 10})
    b.add(subst(P32[:10], [9]), {0: (None, None)}, {0: 10})
    b.add(subst(P32[:20], [0, 19]), {0: (None, None)}, {0: 20})
    # the exact search gives a tail of 8; the tolerant one has a FIRST, which suppresses it
    for p in (3, 120):
        b.add(filler(b.rng, p) + subst(P12, [6]) + filler(b.rng, 25) + P12[:8], {1: (p, 1)}, {1: None})
    return b.done()


def bounds_text(n):
    """per = 10 and 32 on the same text, n probes; two 12 kb lines in one wave with short ones"""
    probes = [P12, P32, P20, P8, P30, P19, P10, P29][:n]
    b = _Text(35, probes)
    for k, probe in enumerate(probes):
        m = len(probe)
        for nsub in (0, 1, 2, 3, 4):
            at = [0, m - 1, m // 2, m // 3][:nsub]
            p = 11 * k + nsub
            b.add(b.plant(p, subst(probe, at)), {k: (p, nsub) if nsub <= E(m, 10) else (None, None)})
    while len(b.parts) % 4:
        b.add(filler(b.rng, 20))
    b.add(b.plant(11000, subst(probes[0], [5]), 1000), {0: (11000, 1)})
    b.add(filler(b.rng, 50))
    b.add(b.plant(230, probes[0], 12000 - 250) + subst(probes[0], [0])[:9], {0: (230, 0)})
    b.add(filler(b.rng, 150) + probes[0][:7], {}, {0: 7})
    return b.done(pers=(10, 32))


@functools.lru_cache(maxsize=None)
def random_text(nrec=500, seed=36):
    """``adapt_ref.random_text``'s recipe with each planted probe given 0 .. E + 1 substitutions (accidental matches welcome)"""
    rng = np.random.RandomState(seed)
    probes, out = [P12, b'TGGAATTCTCGG', P8, P32], []
    for i in range(nrec):
        L = int(rng.choice([0, 5, 36, 75, 150, 151, 250, 600]))
        line = bytearray(rng.choice(np.frombuffer(b'ACGTACGTACGTACGTN', dtype=np.uint8), L).tobytes())
        for _ in range(int(rng.randint(0, 3))):
            probe, p = probes[rng.randint(len(probes))], int(rng.randint(0, L + 1))
            nsub = int(rng.randint(0, E(len(probe), 10) + 2))
            probe = subst(probe, [int(v) for v in rng.choice(len(probe), nsub, replace=False)])
            line[p:p + len(probe)] = probe[:max(L - p, 0)]
        out.append(rec(bytes(line[:L]), nl=b'\r\n' if i % 50 == 0 else b'\n'))
    return b''.join(out), probes, (10,), None


@functools.lru_cache(maxsize=None)
def reveal_text():
    """``clip_ref.reveal_text`` with every other adapter carrying one substitution: records of ``trim_matrix``'s template whose
    bases turn into adapter at an insert length, so that every record whose trim of MASK_per leaves ``minreadlength`` is a hit
    that carries (file_pos, readlength) -- the exact mask gives another set -> (text, read offsets, insert lengths)"""
    import clip_ref as CR
    b = CR._Reveal(200)
    while b.nbytes < (128 << 10) + 8192 + 3 * CR.TM.TILE_OWNS:
        n = len(b.parts)
        c = CR.REVEAL_INS[n % len(CR.REVEAL_INS)]
        form = CR.FORMS[(n // len(CR.REVEAL_INS)) % len(CR.FORMS)]
        a = b.rng.randrange(0, CR.TM.TEMPLATE_LEN - c + 1)
        adapter = subst(P12, [(n // 2) % 12], ('base', 'N', 'lower')[(n // 2) % 3]) if n % 2 else P12
        b.add(b.T[a:a + c] + adapter + filler(b.nrng, CR.REVEAL_L - c - 12), CR.reveal_scores(form, c), c)
    return b.text(), tuple(b.read_off), tuple(b.ins)


@functools.lru_cache(maxsize=None)
def reveal_census():
    """the adapter begins where the builder put it under per = 10, and nowhere earlier; the exact rule misses half of them"""
    import clip_ref as CR
    text, read_off, ins = reveal_text()
    co = [0, len(text)]
    probes = CR.PROBES[2]
    tolerant = [r[4] for r in per_record(text, co, probes, 10)]
    exact = [r[4] for r in A.per_record(text, co, probes)]
    assert tolerant == list(ins) and len(ins) > 700
    missed = sum(a != b for a, b in zip(tolerant, exact))
    assert 3 * missed >= len(ins), (missed, len(ins))
    return dict(records=len(ins), missed=missed)


@functools.lru_cache(maxsize=None)
def texts():
    """name -> (text, probes, the rates it is run at, what its builder expects per record at per = 10)"""
    t = {'budget/0': budget_text(LO, 29), 'budget/1': budget_text(HI, 30), 'kinds': kinds_text(), 'overhang': overhang_text(),
         'earliest': earliest_text(), 'tails': tails_text(), 'random': random_text()}
    for n in (1, 2, 4, 6, 7, 8):
        t['bounds/%d' % n] = bounds_text(n)
    return t


@functools.lru_cache(maxsize=None)
def reference(name, per):
    """per_record of a text, computed once"""
    text, probes, pers, _ = texts()[name]
    assert per in pers
    return tuple(per_record(text, [0, len(text)], probes, per))


@functools.lru_cache(maxsize=None)
def check_census(name):
    """the plain statement gives what the builder planted, and the text reaches the seams it is built for"""
    text, probes, pers, want = texts()[name]
    recs = reference(name, 10)
    c = dict(dists=set(), tails=set(), start16=set(), seams=set(), cr_tail=0, none_over_budget=0, suppressed=0, L=set(), sub_at=set(), sub_off=set())
    assert want is None or len(want) == len(recs)
    for i, (start, L, firsts, tails, clip, cr, dists) in enumerate(recs):
        c['L'].add(L)
        for k, probe in enumerate(probes):
            if firsts[k] is not None:
                c['dists'].add((len(probe), dists[k])); c['start16'].add(start % 16); c['seams'].add(firsts[k])
                for j in range(len(probe)):                   # where the accepted window differs: line position, (m, window offset)
                    if text[start + firsts[k] + j] != probe[j]:
                        c['sub_at'].add(firsts[k] + j); c['sub_off'].add((len(probe), j))
            if tails[k] is not None:
                c['tails'].add((k, tails[k])); c['cr_tail'] += cr
        if want is None:
            continue
        wf, wt = want[i]
        for k, (p, d) in wf.items():
            assert (firsts[k], dists[k]) == (p, d), (name, i, k, firsts[k], dists[k], p, d)
            c['none_over_budget'] += p is None
        for k in range(len(probes)):                          # what the builder did not plant is not there
            if k not in wf:
                assert firsts[k] is None, (name, i, k, firsts[k])
            t = wt.get(k)
            if isinstance(t, tuple):                          # ('not', t): over budget at t, whatever a shorter tail makes of it
                assert tails[k] != t[1], (name, i, k, tails[k])
            else:
                assert tails[k] == t, (name, i, k, tails[k], t)
                c['suppressed'] += k in wt and t is None
    if name.startswith('budget'):
        for probe in probes:
            m = len(probe)
            assert (m, E(m, 10)) in c['dists'], (name, m)     # the budget used up
            if E(m, 10):                                      # accepted with a substitution at base 0, at m - 1, on window offsets 15 / 16 and 31
                assert {(m, o) for o in (0, m - 1, 15, 16, 31) if o < m} <= c['sub_off'], (name, m, sorted(c['sub_off']))
        assert c['start16'] == set(range(16)) and c['none_over_budget'] >= 12 * sum(E(len(p), 10) > 0 for p in probes)
        assert set(SEAMS[:10]) <= c['sub_at'], sorted(c['sub_at'])       # accepted with a substitution on either side of every seam
    elif name == 'kinds':
        assert {(12, 1), (20, 2), (32, 3)} <= c['dists'] and c['none_over_budget'] >= 20
    elif name == 'overhang':
        assert not c['dists'] and {(0, 7), (1, 11), (1, 10), (2, 19), (2, 18), (2, 17), (3, 31), (3, 30), (3, 29), (3, 28)} <= c['tails'] and c['cr_tail'] >= 10
    elif name == 'earliest':
        assert {(12, 1), (12, 0), (16, 1)} <= c['dists'] and c['none_over_budget'] == 5 and {0, 9, 100, 215, 230} <= c['seams']
    elif name == 'tails':
        assert {(0, t) for t in (9, 10, 19, 20, 29, 30, 31)} | {(2, 10)} <= c['tails'] and c['suppressed'] == 2 and {10, 20} <= c['L']
    elif name.startswith('bounds'):
        assert max(c['L']) >= 12000 and 11000 in c['seams'] and 230 in c['seams'] and (0, 7) in c['tails']
        # at per = 32 only the 32-base probe has a budget, of one
        for _, _, firsts, _, _, _, dists in reference(name, 32):
            assert all(d is None or d <= E(len(p), 32) for p, d in zip(probes, dists))
    elif name == 'random':
        assert {(12, 0), (12, 1), (32, 3), (8, 0)} <= c['dists'] and len(c['tails']) >= 5
    return c
