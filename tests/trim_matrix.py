"""
Texts in which every record reveals its quality trim.

The trim (workhorse.c:1055-1068: the first-longest run of score bytes >= Amin, compared as signed char, the closing
newline ending the last run) has two outputs per record, (start, length).  A hit carries both: ``file_pos`` is the
stream offset of the trimmed read's first base (workhorse.c:1070) and ``readlength`` the trimmed length.  So every
record here is built to hit whatever its trim:

 * template reads: the bases are a slice T[a : a + L] of one 700-base sequence T of the table; any trimmed window of
   at least ``minreadlength`` bases lies inside T without an error;
 * probe reads (long records): random bases with a 40-base sequence P of the table planted inside the run the trim
   must pick; another run or another length gives another (file_pos, readlength), or no hit.

``trim`` is the plain statement of the loop; the score-line families aim at the slices the scan kernel gives the
lanes of a read (G lanes, ``per = ceil(Q / G)`` scores each) and at the three ways it sums a slice up (closed form for
up to 3 bad bytes in every slice of a wave, a walk for up to 8, shift-descent beyond).  tests/test_trim_host.py checks
without a GPU that the texts are what they claim to be and that the oracle reveals every record;
tests/test_gpu_trim.py runs them on the GPU.
"""
import functools
import random

import numpy as np

import kernel_matrix as KM
from kvarq_amd import synth

HEADER_FMT = '@TRM.%09d 1:N:0\n'             # as long as synth.HEADER_FMT: a record of L bases has synth.record_bytes(L) bytes
TEMPLATE_LEN, PROBE_LEN, N_AT = 700, 40, 350
MAX_TEMPLATE_READ = 600
MAX_READLENGTH = 1024                        # bins of the read-length histogram (workhorse.c:107)
TILE_OWNS = 39760                            # bytes a tile of short reads owns (kernels_seeded.hip: ST_TILE + ST_OV - 1040)
TILE_NEWLINES = 1920                         # newlines a tile's table holds; beyond, the tile leaves all its records to the redo (BP_NLCAP)
LOOKAHEAD = 1040
FAMILIES = ('clean', 'closed', 'walk', 'descent', 'ties', 'bytes', 'tiny')
BANDED = ('clean', 'closed', 'walk', 'descent', 'ties', 'bytes')
# (lane group, draining kernel) of the six scan-kernel cells
CELLS = [(-1, False), (1, False), (2, False), (3, False), (-1, True), (2, True)]
AMINS = (ord('!'), ord('I'), 0x7E)


def cell_id(cell):
    return 'lg%s-%s' % (cell[0] if cell[0] >= 0 else 'x', 'drain' if cell[1] else 'halve')


def signed(c):
    return c - 256 if c > 127 else c


def trim(scores, amin):
    """(start, length) of the trimmed read: workhorse.c:1055-1068 over the score line and its newline"""
    amin = signed(amin)
    start, length = 0, 0
    run = 0                                   # qtr starts at startscore
    for i, c in enumerate(bytes(scores) + b'\n'):
        if signed(c) >= amin:
            if run is None:
                run = i
        else:
            if run is not None:
                if i - run > length:
                    length, start = i - run, run
                run = None
    return start, length


# ---------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------

def template(with_n=False):
    rng = random.Random(700)
    t = bytearray(rng.choice(b'ACGT') for _ in range(TEMPLATE_LEN))
    if with_n:
        t[N_AT] = ord('N')
    return bytes(t)


def probe():
    rng = random.Random(40)
    return bytes(rng.choice(b'ACGT') for _ in range(PROBE_LEN))


def table(with_n=False):
    return synth.both_strands([template(with_n), probe()])


# ---------------------------------------------------------------------------------------------------------------
# score lines: patterns (1 = good score) and their bytes
# ---------------------------------------------------------------------------------------------------------------

def slices(Q, G):
    """the score ranges the G lanes of a read take (kernels_bp.hip, P3)"""
    per = -(-Q // G)
    return [(min(per * l, Q), min(per * (l + 1), Q)) for l in range(G)]


def bad_counts(pat, G):
    return [e - b - sum(pat[b:e]) for b, e in slices(len(pat), G)]


def runs_of(pat):
    """[(start, length)] of the maximal runs of good scores"""
    out, at = [], None
    for i, v in enumerate(list(pat) + [0]):
        if v and at is None:
            at = i
        elif not v and at is not None:
            out.append((at, i - at)); at = None
    return out


def good_bytes(amin):
    return [c for c in (amin, 0x7F, ord('I')) if signed(c) >= signed(amin)]


def bad_bytes(amin):
    return [c for c in (amin - 1, 0x80, 0xFF, 13, 9, 32, 1) if signed(c) < signed(amin)]


def render(pat, amin, rng, wide):
    """the score bytes of a pattern: 'I' / '#' (plain) or drawn from the bytes at the edges of the comparison (wide)"""
    if not wide:
        assert signed(amin) <= ord('I') and signed(amin) > ord('#')
        return bytes(ord('I') if v else ord('#') for v in pat)
    good, bad = good_bytes(amin), bad_bytes(amin)
    return bytes(rng.choice(good) if v else rng.choice(bad) for v in pat)


CLOSED_CASES = ('c0', 'c1', 'c2', 'c3', 'bit0', 'last', 'adj2', 'adj3', 'straddle', 'gap0', 'gap1', 'gap2', 'gap3')
TIES_CASES = ('in-slice', 'three', 'diff-slices', 'cross-later', 'cross-first', 'span3', 'at-end')


def closed_cases(G):
    return [c for c in CLOSED_CASES if G > 1 or c != 'straddle']


def ties_cases(G):
    need = {'diff-slices': 2, 'cross-later': 2, 'cross-first': 2, 'span3': 3}
    return [c for c in TIES_CASES if G >= need.get(c, 1)]


def tiny_lengths(G):
    qs = [0, 1, 2, G - 1, G, G + 1, 63 * G, 64 * G, 65 * G]
    return sorted(set(q for q in qs if 0 <= q <= MAX_TEMPLATE_READ))


def tiny_cases(G):
    return ['Q=%d' % q for q in tiny_lengths(G)] + (['empty-slice'] if G > 1 else [])


def fam_clean(Q, G, rng, case=None):
    return [1] * Q


def fam_closed(Q, G, rng, case):
    pat = [1] * Q
    sl = slices(Q, G)
    roomy = [l for l, (b, e) in enumerate(sl) if e - b >= 8]

    def fill(l, rel):
        b, e = sl[l]
        for i in range(b, e):
            pat[i] = 1
        for r in rel:
            pat[b + r if r >= 0 else e + r] = 0
    for l in roomy:
        n = sl[l][1] - sl[l][0]
        fill(l, rng.sample(range(n), rng.randrange(0, 4)))
    if not roomy:
        return pat
    t = rng.choice(roomy)
    n = sl[t][1] - sl[t][0]
    if case in ('c0', 'c1', 'c2', 'c3'):
        fill(t, rng.sample(range(n), int(case[1])))
    elif case == 'bit0':
        fill(t, [0] + rng.sample(range(1, n), rng.randrange(0, 3)))
    elif case == 'last':
        fill(t, [-1] + rng.sample(range(0, n - 1), rng.randrange(0, 3)))
    elif case == 'adj2':
        p = rng.randrange(0, n - 1); fill(t, [p, p + 1])
    elif case == 'adj3':
        p = rng.randrange(0, n - 2); fill(t, [p, p + 1, p + 2])
    elif case == 'straddle':
        pairs = [l for l in roomy if l + 1 in roomy]
        if pairs:
            l = rng.choice(pairs)
            fill(l, [-1] + rng.sample(range(0, sl[l][1] - sl[l][0] - 1), rng.randrange(0, 3)))
            fill(l + 1, [0] + rng.sample(range(1, sl[l + 1][1] - sl[l + 1][0]), rng.randrange(0, 3)))
    elif case.startswith('gap'):
        # short runs everywhere else, the slice's gap number K the longest run of the line
        for l in roomy:
            m = sl[l][1] - sl[l][0]
            fill(l, [0, m // 2, -1])
        fill(t, {0: [-5, -3, -1], 1: [0, -3, -1], 2: [0, 2, -1], 3: [0, 2, 4]}[int(case[3])])
    return pat


def fam_walk(Q, G, rng, case=None):
    pat = [1] * Q
    sl = slices(Q, G)
    lanes = [l for l, (b, e) in enumerate(sl) if e - b >= 4]
    must = rng.choice(lanes) if lanes else None
    for l, (b, e) in enumerate(sl):
        n = e - b
        c = rng.randrange(4, min(8, n) + 1) if l == must else rng.randrange(0, min(8, n) + 1)
        for p in rng.sample(range(n), c):
            pat[b + p] = 0
    return pat


DESCENT_CASES = ('alternating', 'random', 'all-bad', 'all-bad-but-one')


def fam_descent(Q, G, rng, case):
    if case == 'alternating':
        k = rng.randrange(2)
        return [(i + k) & 1 for i in range(Q)]
    if case == 'random':
        return [rng.randrange(2) for _ in range(Q)]
    pat = [0] * Q
    if case == 'all-bad-but-one' and Q:
        pat[rng.randrange(Q)] = 1
    return pat


def _noise(Q, rng):
    """random scores without a run of three good ones"""
    pat = [rng.randrange(2) for _ in range(Q)]
    for i in range(2, Q):
        if pat[i - 2] and pat[i - 1]:
            pat[i] = 0
    return pat


def _carve(pat, s, r):
    Q = len(pat)
    assert 0 <= s and s + r <= Q
    for i in range(s, s + r):
        pat[i] = 1
    if s > 0:
        pat[s - 1] = 0
    if s + r < Q:
        pat[s + r] = 0


def fam_ties(Q, G, rng, case):
    """equally long best runs placed against the slice bounds; what a line really holds is counted by ties_census"""
    pat = _noise(Q, rng)
    sl = slices(Q, G)
    per = -(-Q // G)
    if case == 'in-slice':
        t = rng.choice([l for l, (b, e) in enumerate(sl) if e - b == max(e_ - b_ for b_, e_ in sl)])
        b, e = sl[t]
        r = (e - b - 3) // 2
        if r >= 3:
            _carve(pat, b + 1, r); _carve(pat, b + 2 + r, r)
    elif case == 'three':
        r = (Q - 4) // 3
        if r >= 3:
            for k in range(3):
                _carve(pat, 1 + k * (r + 1), r)
    elif case == 'diff-slices':
        roomy = [l for l, (b, e) in enumerate(sl) if e - b >= 5]
        if len(roomy) >= 2:
            i, j = sorted(rng.sample(roomy, 2))
            r = min(sl[i][1] - sl[i][0], sl[j][1] - sl[j][0]) - 2
            _carve(pat, sl[i][0] + 1, r); _carve(pat, sl[j][0] + 1, r)
    elif case in ('cross-later', 'cross-first'):
        # the longest pair that fits: r scores each, the crossing run x scores in front of its bound
        fits = []
        for r in range(min(per - 2, (Q - 3) // 2), 2, -1):
            for x in sorted(set((max(1, r // 2), max(1, r // 4), 1, r - 1))):
                if case == 'cross-later':
                    # a run inside the first slice, an equally long one across a later bound
                    fits += [(1, per * l - x) for l in range(1, G) if per * l < Q and per * l - x >= r + 2 and per * l - x + r <= Q]
                else:
                    # a run across the first bound, an equally long one inside a later slice (or what is left of the second)
                    s1 = per - x
                    if s1 >= 1 and per < Q:
                        fits += [(s1, max(b, s1 + r + 1)) for b, e in sl[1:] if max(b, s1 + r + 1) + r <= e]
            if fits:
                a, b = rng.choice(fits)
                _carve(pat, a, r); _carve(pat, b, r)
                break
    elif case == 'span3':
        mids = [l for l in range(1, G - 1) if sl[l][1] - sl[l][0] == per and sl[l + 1][1] - sl[l + 1][0] >= 3]
        if mids:
            l = rng.choice(mids)
            x, y = rng.randrange(1, min(per, 9)), rng.randrange(1, sl[l + 1][1] - sl[l + 1][0] - 1)
            _carve(pat, sl[l][0] - x, per + x + y)
    elif case == 'at-end':
        r = Q // 2 + 1
        if Q >= 6:
            _carve(pat, Q - r, r)
    return pat


def fam_bytes(Q, G, rng, case=None):
    pat, v = [], rng.randrange(2)
    while len(pat) < Q:
        pat.extend([v] * rng.randrange(1, max(2, Q // 3)))
        v ^= 1
    return pat[:Q]


def fam_tiny(Q, G, rng, case):
    if case == 'good':
        return [1] * Q
    if case == 'bad':
        return [0] * Q
    return [rng.randrange(4) > 0 for _ in range(Q)]


FAMILY = dict(clean=(fam_clean, (None,)), closed=(fam_closed, None), walk=(fam_walk, (None,)), descent=(fam_descent, DESCENT_CASES),
              ties=(fam_ties, None), bytes=(fam_bytes, (None,)), tiny=(fam_tiny, ('good', 'random', 'bad')))


def closed_census(pat, G):
    """the named cases of the closed form a score line holds (none when a slice has more than 3 bad bytes)"""
    Q = len(pat)
    sl = slices(Q, G)
    counts = bad_counts(pat, G)
    if max(counts) > 3:
        return set()
    out = set()
    for l, (b, e) in enumerate(sl):
        if e == b:
            continue
        out.add('c%d' % counts[l])
        if not pat[b]:
            out.add('bit0')
        if not pat[e - 1]:
            out.add('last')
        if not pat[e - 1] and e < Q and not pat[e]:
            out.add('straddle')
        bad = [i for i in range(b, e) if not pat[i]]
        if any(y == x + 1 for x, y in zip(bad, bad[1:])):
            out.add('adj2')
        if len(bad) == 3 and bad[2] == bad[0] + 2:
            out.add('adj3')
    pat01 = [1 if v else 0 for v in pat]
    runs = runs_of(pat01)
    if runs:
        s, ln = max(runs, key=lambda r: (r[1], -r[0]))          # the first of the longest
        for l, (b, e) in enumerate(sl):
            if b <= s and s + ln <= e and counts[l] == 3:
                out.add('gap%d' % sum(1 for i in range(b, s) if not pat[i]))
    return out


def ties_census(pat, G):
    Q = len(pat)
    sl = slices(Q, G)
    runs = runs_of([1 if v else 0 for v in pat])
    if not runs:
        return set()
    best = max(ln for _, ln in runs)
    win = [(s, ln) for s, ln in runs if ln == best]

    def inside(s, ln):
        for l, (b, e) in enumerate(sl):
            if b <= s and s + ln <= e:
                return l
        return None

    def touched(s, ln):
        return sum(1 for b, e in sl if b < s + ln and s < e)
    out = set()
    where = [inside(s, ln) for s, ln in win]
    if len(win) >= 2:
        if len(win) >= 3:
            out.add('three')
        ins = [w for w in where if w is not None]
        if len(ins) != len(set(ins)):
            out.add('in-slice')
        if len(set(ins)) >= 2:
            out.add('diff-slices')
        if where[0] is not None and any(w is None for w in where[1:]):
            out.add('cross-later')
        if where[0] is None and any(w is not None for w in where[1:]):
            out.add('cross-first')
    if touched(*win[0]) >= 3:
        out.add('span3')
    if win[0][0] + win[0][1] == Q:
        out.add('at-end')
    return out


def tiny_census(pat, G):
    Q = len(pat)
    out = {'Q=%d' % Q}
    if G > 1 and any(b >= Q for b, _ in slices(Q, G)[1:]):
        out.add('empty-slice')
    return out


# ---------------------------------------------------------------------------------------------------------------
# texts
# ---------------------------------------------------------------------------------------------------------------

class Record(object):
    __slots__ = ('start', 'read_off', 'scores', 'family', 'case', 'band', 'pat', 'long')

    def __init__(self, start, read_off, scores, family, case, band, pat, long_=False):
        self.start, self.read_off, self.scores, self.family, self.case, self.band, self.pat, self.long = start, read_off, scores, family, case, band, pat, long_


class Text(object):
    """a FastQ text and what is known of its records; G: the lanes a read of the head's length gets; pad_to: shorter
    records get a longer identifier line, so that a tile holds as many records as the head's and the general kernel,
    which picks the lanes per tile from that number, stays at G"""

    def __init__(self, cfg, G, with_n=False, seed=0, pad_to=0):
        self.cfg, self.G, self.pad_to = dict(cfg), G, pad_to
        self.amin = cfg['Amin'][0] if isinstance(cfg['Amin'], bytes) else ord(cfg['Amin'])
        self.wide = self.amin != ord('.')          # (the plain bytes 'I' / '#' are a good and a bad score at '.' only)
        self.T, self.P = template(with_n), probe()
        self.rng = random.Random(seed)
        self.parts, self.nbytes, self.records, self.bands = [], 0, [], []
        self.next_case = {}

    def add(self, bases, scores, family, case, band, pat, long_=False):
        head = (HEADER_FMT % len(self.records)).encode()
        rest = bases + b'\n+\n' + scores + b'\n'
        if len(head) + len(rest) < self.pad_to:
            head = head[:-1] + b' ' + b'p' * (self.pad_to - len(head) - len(rest) - 1) + b'\n'
        self.records.append(Record(self.nbytes, self.nbytes + len(head), scores, family, case, band, pat, long_))
        self.parts.append(head + rest); self.nbytes += len(head) + len(rest)

    def cases_of(self, family):
        if family == 'closed':
            return closed_cases(self.G)
        if family == 'ties':
            return ties_cases(self.G)
        return FAMILY[family][1]

    def template_read(self, family, L, band):
        """one record of a family: L template bases (the tiny family has lengths of its own)"""
        rng = self.rng
        cases = self.cases_of(family)
        n = self.next_case.get(family, 0); self.next_case[family] = n + 1
        case = cases[n % len(cases)]
        if family == 'tiny':
            qs = tiny_lengths(self.G)
            L = qs[(n // len(cases)) % len(qs)]
        pat = FAMILY[family][0](L, self.G, rng, case)
        scores = bytearray(render(pat, self.amin, rng, self.wide or family == 'bytes'))
        if family == 'bytes' and L and n % 3 == 0:
            # a score line that begins like a record or like its third line
            head = [c for c in b'@+' if signed(c) >= signed(self.amin)]
            if head:
                scores[0] = head[(n // 3) % len(head)]; pat[0] = 1
        a = rng.randrange(0, TEMPLATE_LEN - L + 1)
        self.add(self.T[a:a + L], bytes(scores), family, case, band, pat)

    def band(self, families, L, nbytes=0, nrec=0, name=None):
        """records of the families in turn, until both the bytes and the records are there"""
        band = len(self.bands)
        begin, first, i = self.nbytes, len(self.records), 0
        while self.nbytes - begin < nbytes or len(self.records) - first < nrec:
            self.template_read(families[i % len(families)], L, band); i += 1
        self.bands.append((name or (families[0] if len(families) == 1 else 'mixed'), first, len(self.records), L))

    def long_read(self, pat, band):
        """random bases with the probe planted inside the run the trim must pick"""
        rng = self.rng
        Q = len(pat)
        scores = render(pat, self.amin, rng, False)
        s, ln = trim(scores, self.amin)
        assert ln >= 64
        bases = bytearray(rng.choice(b'ACGT') for _ in range(Q))
        at = s + rng.randrange(0, ln - PROBE_LEN + 1)
        bases[at:at + PROBE_LEN] = self.P
        self.add(bytes(bases), scores, 'long', None, band, pat, True)

    def finish(self):
        self.data = np.frombuffer(b''.join(self.parts), dtype=np.uint8)
        self.parts = None
        assert self.data.nbytes == self.nbytes
        return self

    # what the plain statement predicts
    def trims(self):
        if not hasattr(self, '_trims'):
            self._trims = [trim(r.scores, self.amin) for r in self.records]
        return self._trims

    def readlengths(self):
        """the read-length histogram in the oracle's shape (stats['readlengths'])"""
        tr = self.trims()
        longest = max(ln for _, ln in tr)
        h = [0] * (longest + 1)
        for _, ln in tr:
            if ln < MAX_READLENGTH:
                h[ln] += 1
        return tuple(h)

    def revealed(self):
        """{(file_pos, readlength)} of the records the length gate lets through"""
        mrl = self.cfg['minreadlength']
        return set((r.read_off + s, ln) for r, (s, ln) in zip(self.records, self.trims()) if ln >= mrl)


def lanes_of_uniform_reads(L):
    """lanes a read gets in the general kernel on a text of L-base records: the library's tile for such a text
    (kvq_tile_for_text, as tests/test_kernel_dispatch.py asks it), then the widest group that gives each of the
    tile's records its own lanes"""
    import ctypes as C
    from kvarq_amd import _lib
    rb = synth.record_bytes(L)
    head = np.frombuffer(b''.join((HEADER_FMT % i).encode() + b'A' * L + b'\n+\n' + b'I' * L + b'\n' for i in range((130 << 10) // rb + 1)), dtype=np.uint8)
    got = C.c_uint32()
    tile = _lib.lib().kvq_tile_for_text(head.ctypes.data, min(head.nbytes, 128 << 10), C.byref(got))
    return lanes_of_a_tile(tile // rb + 1)


def lanes_of_a_tile(nrec):
    """kernels_bp.hip, LG < 0: lg = 9 - ceil(log2(records the tile owns)), 0 .. 6"""
    return 1 << max(0, min(6, 9 - (nrec - 1).bit_length()))


class Workload(object):
    """the texts of one scan-kernel cell: a head of L-base records that sets tile and lane group, a band of each family
    long enough to hold a whole tile, a band of all families in turn; for the fixed lane groups a second text whose
    body has other lengths"""

    def __init__(self, lg, dense, with_n=False):
        self.lg, self.dense, self.with_n = lg, dense, with_n
        self.cfg = dict(KM.CONFIGS[5 if dense else 8])
        self.seqs = table(with_n)
        self.texts = []
        seed = 1000 * (lg + 2) + (500 if dense else 0)
        if lg > 0:
            L, G = KM.READ_LEN[lg], 1 << lg
            self.texts.append(self._banded(L, G, seed))
            t = Text(self.cfg, G, with_n, seed + 1)
            t.band(BANDED, L, nbytes=(128 << 10) + 8192)
            short, long_ = KM.BODY_LEN[lg]
            t.band(FAMILIES, short, nrec=1200)
            t.band(FAMILIES, long_, nrec=420)
            self.texts.append(t.finish())
        else:
            for i, L in enumerate((40, 600)):
                # (every record as long as the head's: the tiles hold what the head's do, and so do the lanes)
                self.texts.append(self._banded(L, lanes_of_uniform_reads(L), seed + i, synth.record_bytes(L)))

    def _banded(self, L, G, seed, pad_to=0):
        t = Text(self.cfg, G, self.with_n, seed, pad_to)
        t.band(BANDED, L, nbytes=(128 << 10) + 8192)
        for fam in BANDED:
            t.band((fam,), L, nbytes=3 * TILE_OWNS)
        t.band(FAMILIES, L, nbytes=3 * TILE_OWNS, nrec=7 * 30)
        # (the last tile of a chunk is a short one: where the kernel picks the lanes per tile it has lanes of its own)
        t.band(('clean',), L, nbytes=TILE_OWNS + 8192, name='tail')
        return t.finish()


@functools.lru_cache(maxsize=None)
def workload(lg, dense, with_n=False):
    return Workload(lg, dense, with_n)


@functools.lru_cache(maxsize=None)
def amin_text(amin):
    """150-base records of the bytes family at another Amin (the product's other settings)"""
    cfg = dict(KM.CONFIGS[8], Amin=bytes([amin]))
    t = Text(cfg, 4, seed=amin)
    t.band(('bytes',), 150, nbytes=(128 << 10) + 8192 + 4 * TILE_OWNS)
    return t.finish()


# the long records of the redo text: (scores, kind)
LONG_RECORDS = [(1023, 'dips'), (1023, 'flush'), (1024, 'big'), (1024, 'seam16'), (1025, 'ties'), (1025, 'big'),
                (2047, 'seam1k'), (2047, 'big'), (2048, 'flush'), (2048, 'ties'), (2049, 'seam1k'), (2049, 'dips'),
                (4095, 'big'), (4095, 'seam16'), (4096, 'seam1k'), (4096, 'flush'), (4097, 'ties'), (4097, 'seam1k'),
                (8191, 'seam4k'), (8191, 'big'), (9000, 'seam4k'), (9000, 'dips')]


def long_pattern(Q, kind, rng):
    if kind == 'dips':
        pat = [1] * Q
        for _ in range(Q // 40):
            pat[rng.randrange(Q)] = 0
        return pat
    if kind == 'ties':                                        # two equally long best runs: the first one wins
        run = Q // 3
        pat = [0] * Q
        a = rng.randrange(1, Q - 2 * run - 2)
        b = a + run + 1 + rng.randrange(0, Q - a - 2 * run - 1)
        pat[a:a + run] = [1] * run; pat[b:b + run] = [1] * run
        return pat
    if kind == 'flush':                                       # the best run ends with the line: the last vector, shifted into place
        pat = _noise(Q, rng)
        _carve(pat, Q - Q // 2, Q // 2)
        return pat
    if kind == 'big':                                         # a best run of 1024 scores or more (all of them where the line has no more)
        pat = [1] * Q
        if Q > 1100:
            for _ in range(Q // 100):
                pat[rng.randrange(Q - 1100)] = 0
            pat[Q - 1100] = 0
        return pat
    pat = _noise(Q, rng)
    if kind == 'seam16':                                      # the best run across the bound of two lanes' 16 scores
        _carve(pat, 16 * rng.randrange(2, Q // 16 - 6) - 5, 70)
    elif kind == 'seam1k':                                    # ... across a KiB row
        _carve(pat, 1024 * rng.randrange(1, (Q - 60) // 1024 + 1) - 37, 90)
    elif kind == 'seam4k':                                    # ... across the 4 KiB of one turn of the outer loop
        _carve(pat, 4096 - 50, 100)
    return pat


@functools.lru_cache(maxsize=None)
def redo_text(k):
    """150-base template reads with long probe records placed where their tile cannot hold them (their start inside a
    chunk's first tile, their end beyond its look-ahead: the tile leaves them to the redo), and a stretch of records so
    short that a tile holds more of them than its tables do (it leaves them all: kvq_trim_records' short path).
    -> (text, chunk offsets)"""
    cfg = dict(KM.CONFIGS[k])
    t = Text(cfg, 4, seed=4242 + k)
    rb = synth.record_bytes(150)
    fams = ('clean', 'closed', 'walk', 'descent', 'ties', 'bytes')
    co = [0]
    t.band(fams, 150, nbytes=(128 << 10) + 8192)              # the head: tile and lane group of ordinary reads
    for Q, kind in LONG_RECORDS:
        co.append(t.nbytes)
        # the record starts inside the chunk's first tile and ends beyond its look-ahead
        before = 108 if 108 * rb + 2 * Q + 25 > TILE_OWNS + LOOKAHEAD + 160 else 120
        assert before * rb < TILE_OWNS - 160 and before * rb + 2 * Q + 25 > TILE_OWNS + LOOKAHEAD + 160
        t.band(fams, 150, nrec=before)
        t.long_read(long_pattern(Q, kind, t.rng), len(t.bands))
        t.band(fams, 150, nrec=10)
    co.append(t.nbytes)
    band = len(t.bands)
    first = len(t.records)
    t.G = 1
    n = 0
    while t.nbytes - co[-1] < 3 * TILE_OWNS:
        L = 16 + n % 9
        fam = ('ties', 'bytes', 'clean', 'descent')[n % 4]
        case = ('in-slice', None, None, 'random')[n % 4]
        pat = FAMILY[fam][0](L, 1, t.rng, case)
        a = t.rng.randrange(0, TEMPLATE_LEN - L + 1)
        t.add(t.T[a:a + L], render(pat, t.amin, t.rng, fam == 'bytes'), fam, case, band, pat)
        n += 1
    t.bands.append(('short', first, len(t.records), 0))
    t.G = 4
    co.append(t.nbytes)
    t.band(fams, 150, nrec=60)
    co.append(t.nbytes)
    return t.finish(), np.array(co, dtype=np.int64)
