"""
Texts in which every record aims one alignment at one seam of the matchers' compare loops.

Whether a read is a hit is decided by counting the mismatches of an overlap and by knowing which of the loops of
workhorse.c:1112-1174 visit it.  The library has five statements of that (kvq_verify_survivors, bp_verify_rest,
kvq_match_all / within_budget, kvq_match_long / within_budget_lds, the seed filter in front of the first two); they
share no code, and each walks an overlap in steps of its own: 128, 64, 16 and 8 bytes, one reach-back vector over the
last 16 bytes, tails of 4 and of single bytes.  Miscounting by one on either side of such a step loses a hit or invents
one, and only a read with exactly ``maxerrors`` or ``maxerrors + 1`` mismatches, one of them on the seam, shows it.

``alignments`` is the plain statement of the four loops.  A *spec* describes one alignment: the cell (configuration),
the target sequence, the geometry (which loop visits it and where), the overlap length L, the offsets of its mismatches
inside the overlap, the bytes they put there, and what the statement makes of it (the hits planned, none for the twin
with one mismatch more).  ``Cell`` builds the specs, one named record ``@M<cell>.<n>`` each (n indexes ``Cell.specs``),
and the texts: a head of plain synthetic records that sets tile and lane group, the spec records behind it.

tests/test_match_host.py checks without a GPU that the statement, the plan and the oracle agree on every spec and
counts what the cells cover; tests/test_gpu_match.py runs the texts through every route of the library.
"""
import bisect
import functools
import itertools
import random

import numpy as np

import kernel_matrix as KM
from kvarq_amd import synth

# cell -> (configuration, seed length or 0)
CONFIGS = {
    'P': (dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.'), 8),       # the product's configuration; halving kernel
    'S': (dict(maxerrors=1, minoverlap=10, minreadlength=10, Amin='.'), 5),       # overlaps under 16 bytes
    'E4': (dict(maxerrors=4, minoverlap=25, minreadlength=25, Amin='.'), 5),      # maxerrors 4 .. 6 on the seed filter
    'E6': (dict(maxerrors=6, minoverlap=35, minreadlength=35, Amin='.'), 5),
    'X': (dict(maxerrors=6, minoverlap=34, minreadlength=34, Amin='.'), 0),       # E6's specs, one base of overlap less: no seed index
}
CELLS = ('P', 'S', 'E4', 'E6', 'X')
BACKGROUNDS = {'P': (150,), 'S': (150,), 'E4': (75, 150), 'E6': (75, 150), 'X': (150,)}
LONG_OVERLAPS = (47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 271)
KINDS = ('sub', 'keep', 'high')
GENERAL = ('A', 'B', 'Cs')                  # the geometries every seam class is crossed with
PAD_TO = 200                                # bytes of a spec record at least: a tile never holds more records than its tables do


def alignments(read, seq, cfg):
    """[(seq_pos, length)] of one read on one sequence in the order of emission: workhorse.c:1112-1174"""
    r, q = np.frombuffer(bytes(read), dtype=np.uint8), np.frombuffer(bytes(seq), dtype=np.uint8)
    rl, seql, mo, me = len(r), len(q), cfg['minoverlap'], cfg['maxerrors']
    out = []

    def within(a, b):
        return int(np.count_nonzero(a != b)) <= me
    if rl > mo and seql > mo:
        i = rl - mo                                             # A: the read's tail over the sequence's head
        while i > 0 and rl - i <= seql - 1:
            if within(r[i:], q[:rl - i]):
                out.append((-i, rl - i))
            i -= 1
        i = seql - mo                                           # B: the read's head over the sequence's tail
        while i > 0 and seql - i <= rl:
            if within(q[i:], r[:seql - i]):
                out.append((i, seql - i))
            i -= 1
    if rl > seql:                                               # C: the sequence inside the read
        for i in range(rl - seql + 1):
            if within(r[i:i + seql], q):
                out.append((-i, seql))
    else:                                                       # ... the read inside the sequence
        for i in range(seql - rl + 1):
            if within(q[i:i + rl], r):
                out.append((i, rl))
    return out


def hit_bytes(read, seq_pos, length):
    """the bytes a hit carries (the last argument of add_hit)"""
    at = -seq_pos if seq_pos < 0 else 0
    return read[at:at + length]


# ---------------------------------------------------------------------------------------------------------------
# seams
# ---------------------------------------------------------------------------------------------------------------

def seam_places(L, rng):
    """{seam class: [offsets that carry a mismatch]} for an overlap of L bytes; for 'dword' and 'lastdword' the offsets
    of one whole dword (as many of the mismatches as there are go inside, four at the most)"""
    out = {'first': [0], 'last': [L - 1]}
    for m, sub in ((8, 16), (16, 64), (64, 128), (128, 0)):
        mult = [x for x in range(m, L + 1, m) if not (sub and x % sub == 0)]
        if mult:
            out['m%d-' % m] = [rng.choice(mult) - 1]            # the last byte of a step
        mult = [x for x in mult if x < L]
        if mult:
            out['m%d' % m] = [rng.choice(mult)]                 # the first byte behind it
    if L >= 16:
        out['rb0'], out['rb1'] = [L - 16], [L - 15]             # the first bytes of the reach-back vector
        out['dbl-'] = [16 * (L // 16) - 1]                      # the last byte it covers twice
        if L % 16:
            out['dbl'] = [16 * (L // 16)]                       # the first it alone covers
    out['dword'] = [4 * rng.randrange(L // 4) + k for k in range(4)]
    out['lastdword'] = list(range(L - 4, L))
    return out


def seam_classes(ls):
    """the seam classes overlaps of these lengths have"""
    rng = random.Random(0)
    return sorted(set(c for L in ls for c in seam_places(L, rng)))


def write_byte(kind, n, base):
    """the byte a mismatch of a kind puts in the place of a base"""
    if kind == 'sub':                                           # another code
        return b'ACGT'[(b'ACGT'.index(base) + 1 + n % 3) % 4]
    if kind == 'keep':                                          # the same 2-bit code: G / N / . share one, a base and its lower-case letter
        return (ord('N'), ord('.'), ord('g'))[n % 3] if base == ord('G') else base | 0x20
    return (0x80 | base, 0xFF)[n % 2]


class Spec(object):
    __slots__ = ('n', 'cell', 'target', 'geom', 'L', 'seam', 'kind', 'offs', 'wrote', 'hit', 'plan', 'read', 'ro', 'bases', 'scores', 'lead', 'long', 'shift')

    def __repr__(self):
        return 'M%s.%d(%s on seq %d, L=%d, %s/%s at %s: %s)' % (self.cell, self.n, self.geom, self.target, self.L, self.seam, self.kind, list(self.offs), self.plan)


def _rand(rng, n):
    return bytes(rng.choice(b'ACGT') for _ in range(n))


class Cell(object):
    """table, specs and texts of one configuration"""

    def __init__(self, name):
        self.name = name
        self.cfg, self.k = dict(CONFIGS[name][0]), CONFIGS[name][1]
        e, mo = self.cfg['maxerrors'], self.cfg['minoverlap']
        self.e, self.mo = e, mo
        assert (KM.seed_k(self.cfg) if KM.seed_k(self.cfg) >= 5 else 0) == self.k
        k = self.k or CONFIGS['E6'][1]                          # (X: the lengths of E6)
        rng = self.rng = random.Random(sum(ord(c) for c in name) * 7919)
        span = KM.span_of(k, e, 2)
        lens = sorted(set([mo, mo + 1, span - 1, span, 63, 64, 65, 129, 300, 4095, 4096]))
        by_len = dict((n, _rand(rng, n)) for n in lens)
        twin = bytearray(by_len[129]); twin[70] = ord('N')
        kept = [n for n in lens if span <= n <= 4095]
        refused = [n for n in lens if n not in kept]
        # the sequences the seed index takes stand in front: the table without the others has the same numbers for them
        self.seqs_kept = [by_len[n] for n in kept]
        self.seqs = self.seqs_kept + [by_len[n] for n in refused] + [bytes(twin)]
        self.nr = dict((n, i) for i, n in enumerate(kept + refused))            # length -> number
        self.nr_twin = len(self.seqs) - 1
        self.refused = list(range(len(kept), len(self.seqs)))
        if self.k:
            assert all(KM.seedable(q, k, e) for q in self.seqs_kept) and not any(KM.seedable(self.seqs[i], k, e) for i in self.refused)
            self.stride = KM.index_stride(self.seqs_kept, k, e)
            assert name != 'P' or not KM.index_dense(self.seqs_kept, k, e, self.stride)
        else:
            self.stride = 2
        self.pitch = KM.pitch_of(k, self.stride)
        self.kseed = k
        self.overlaps = list(range(10, 34)) if name == 'S' else list(range(mo, mo + 17)) + list(LONG_OVERLAPS)
        self.specs = []
        self.turn = {}
        self._general()
        self._special()
        self.texts = dict((bg, self._text(bg)) for bg in BACKGROUNDS[name])

    # ---- one spec -------------------------------------------------------------------------------------------

    def _offsets(self, L, seam, n):
        """n mismatch offsets of an overlap of L bytes, the seam's among them"""
        rng = self.rng
        place = closed = seam_places(L, rng)[seam] if seam else []
        if seam in ('dword', 'lastdword'):
            place = rng.sample(closed, min(n, 4))
        assert len(place) <= n, (L, seam, n)
        rest = [x for x in range(L) if x not in closed]
        return sorted(place + rng.sample(rest, n - len(place))), place

    def spec(self, geom, target, L, seam, kind, n, at=None, flank=None, offsets=None, keep_all=False, into=None):
        """a record whose read meets sequence `target` on one alignment of `geom` with n mismatches; the flanks are drawn
        again until the statement finds on the pair what was planned and nothing else"""
        rng, q, mo = self.rng, self.seqs[target], self.mo
        seql = len(q)
        into = self.specs if into is None else into
        for attempt in range(50):
            if offsets is not None:
                offs, place = list(offsets), list(offsets)
            else:
                offs, place = self._offsets(L, seam, n) if L > 0 else ([], [])
            fl = rng.randrange(5, 40) if flank is None else flank
            if geom in ('A', 'A-mo', 'A-mo-1', 'A-max', 'big-A'):
                qa, lead, tail = 0, _rand(rng, fl), b''
                plan = [(-fl, L)]
            elif geom in ('B', 'B-mo', 'B-mo-1', 'B-max', 'big-B'):
                qa, lead, tail = seql - L, b'', _rand(rng, fl)
                plan = [(seql - L, L)]
            elif geom in ('Cs', 'Cs-0', 'Cs-mid', 'big-C', 'BC', 'G-rl=mo', 'G-rl=mo+1'):
                qa, lead, tail = (rng.randrange(1, seql - L) if at is None else at), b'', b''
                plan = [(qa, L)] * (2 if qa == seql - L and qa > 0 and L > mo else 1)
            else:                                              # the sequence inside the read, or as long as the read
                assert L == seql
                qa, lead, tail = 0, _rand(rng, at or 0), _rand(rng, (flank or 0))
                plan = [(-len(lead), L)]
            assert 0 <= qa and qa + L <= seql, (geom, target, L, qa)
            ov = bytearray(q[qa:qa + L])
            wrote = []
            for j, o in enumerate(offs):
                kd = kind if o in place or keep_all else KINDS[rng.randrange(3)]
                base = ov[o] if ov[o] in b'ACGT' else ord('A')          # (the N of the twin)
                ov[o] = write_byte(kd, len(into) + j, base)
                assert ov[o] != q[qa + o]
                wrote.append(ov[o])
            read = lead + bytes(ov) + tail
            hit = n <= self.e and not geom.endswith('mo-1')
            if not hit:
                plan = []
            if alignments(read, q, self.cfg) == plan:
                break
        else:
            raise AssertionError('no flanks for %s on %d, L=%d' % (geom, target, L))
        s = Spec()
        s.n, s.cell, s.target, s.geom, s.L, s.seam, s.kind = len(into), self.name, target, geom, L, seam, kind
        s.offs, s.wrote, s.hit, s.plan, s.read, s.ro = tuple(offs), bytes(wrote), hit, plan, read, len(lead)
        # flanks with scores below Amin: the trim leaves exactly the read
        a, b = (_rand(rng, rng.randrange(0, 9)), _rand(rng, rng.randrange(0, 9))) if s.n % 2 else (b'', b'')
        s.bases, s.scores, s.lead = a + read + b, b'#' * len(a) + b'I' * len(read) + b'#' * len(b), len(a)
        s.long, s.shift = False, None
        into.append(s)
        return s

    def twins(self, geom, target, L, seam, kind, **kw):
        """e mismatches (a hit) and e + 1 (none), one of them on the seam"""
        self.spec(geom, target, L, seam, kind, self.e, **kw)
        self.spec(geom, target, L, seam, kind, self.e + 1, **kw)

    def _next(self, key, choices):
        n = self.turn.get(key, 0); self.turn[key] = n + 1
        return choices[n % len(choices)]

    # ---- the specs ------------------------------------------------------------------------------------------

    def _general(self):
        """every overlap length x every seam class it has, geometry and byte kind in turn per seam class"""
        combos = list(itertools.product(GENERAL, KINDS))
        for L in self.overlaps:
            targets = [self.nr[n] for n in (63, 64, 65, 129, 300, 4095) if n > L + 1]
            for seam in sorted(seam_places(L, self.rng)):
                geom, kind = self._next(seam, combos)
                self.twins(geom, self._next('target', targets), L, seam, kind)

    def _special(self):
        e, mo, nr = self.e, self.mo, self.nr
        seams = lambda L: sorted(seam_places(L, self.rng))

        def some(geom, target, L, count=3, **kw):
            for _ in range(count):
                self.twins(geom, target, L, self._next(('sp', geom), seams(L)), self._next(('spk', geom), KINDS), **kw)
        for t in (nr[65], nr[300], self.nr_twin):
            # the first alignment visited, and the one in front of it (never visited: no hit without any mismatch)
            some('A-mo', t, mo); some('B-mo', t, mo)
            self.spec('A-mo-1', t, mo - 1, None, None, 0); self.spec('B-mo-1', t, mo - 1, None, None, 0)
        # the largest overlap a pair has: the read longer than the sequence (seql - 1), and shorter (A: rl - 1; B: rl, where
        # the read inside the sequence emits the same diagonal again -- B first)
        some('A-max', nr[65], 64, flank=36); some('B-max', nr[65], 64, flank=36)
        some('A-max', nr[300], 119, flank=1)
        some('BC', nr[300], 120, at=180); some('BC', nr[65], mo + 3, at=65 - mo - 3)
        # the sequence inside the read: read offsets 0, rl - seql and every residue modulo 8 in between
        for t in (nr[64], nr[129], nr[mo + 1], self.nr_twin, nr[min(n for n in nr if n != mo and n != mo + 1)]):
            seql = len(self.seqs[t])
            for i in [0, 40] + list(range(9, 17)):
                some('Cr-0' if i == 0 else 'Cr-end' if i == 40 else 'Cr-r%d' % (i % 8), t, seql, count=1, at=i, flank=40 - i)
        for t in (nr[63], nr[64], nr[65], nr[129]):
            some('Ceq', t, len(self.seqs[t]), count=2, at=0, flank=0)
        # the read inside the sequence: sequence offsets 0, seql - rl (BC above) and between
        for t, L in ((nr[129], 100), (nr[300], 271), (nr[65], mo + 1)):
            some('Cs-0', t, L, count=2, at=0); some('Cs-mid', t, L, count=2)
        # the guards: rl == minoverlap (only the last loop runs: one hit where rl == minoverlap + 1 has two), seql == minoverlap
        some('G-rl=mo', nr[129], mo, at=129 - mo); some('G-rl=mo+1', nr[129], mo + 1, at=128 - mo)
        some('G-seql=mo', nr[mo], mo, at=31, flank=0)
        # the longest sequence the seed index takes and the shortest it refuses
        for n in (4095, 4096):
            t = nr[n]
            for L in (mo, 129, 271):
                some('big-C', t, L, count=2, at=self.rng.randrange(n - 300, n - L)); some('big-C', t, L, count=1, at=n - 300)
            some('big-B', t, mo); some('big-A', t, mo); some('big-A', t, 129, count=1); some('big-B', t, 257, count=1)
        # whole sequences copied with code-keeping substitutions only, one in each of e (e + 1) seed blocks: every seed
        # stays alive by its codes, only the bytes tell e substitutions (a hit) from e + 1
        for t in (nr[129], nr[300], nr[65]):
            seql = len(self.seqs[t])
            for n in (e, e + 1):
                blocks = self.rng.sample(range(e + 1), n)
                offs = sorted(self.pitch * j + self.rng.randrange(self.kseed) for j in blocks)
                self.spec('keep-in-read', t, seql, None, 'keep', n, at=self.rng.randrange(1, 30), flank=self.rng.randrange(1, 30), offsets=offs, keep_all=True)
                self.spec('keep-eq', t, seql, None, 'keep', n, at=0, flank=0, offsets=offs, keep_all=True)

    # ---- texts ----------------------------------------------------------------------------------------------

    def record(self, s, at=0):
        """(the record of a spec, the offset of its read in it); a long spec's read starts at a stream offset with the
        residue modulo 4 it asks for when the record is put at stream offset `at`"""
        head = b'@%s%s.%d' % (b'L' if s.long else b'M', self.name.encode(), s.n)
        rest = b'\n' + s.bases + b'\n+\n' + s.scores + b'\n'
        pad = max(1 if s.shift is not None else 0, PAD_TO - len(head) - len(rest) - 1)
        if s.shift is not None:
            pad += (s.shift - (at + len(head) + 1 + pad + 1 + s.lead)) % 4
        if pad:
            head += b' ' + b'p' * pad
        return head + rest, len(head) + 1 + s.lead

    def _text(self, bg):
        """a head of bg-base records (it sets the tile and the lane group), the spec records, a tile of the same behind them"""
        g = synth.genome()
        rb = synth.record_bytes(bg)
        nhead, ntail = ((128 << 10) + 8192) // rb + 1, (48 << 10) // rb + 1
        back = synth.reads(g, 1000 * (bg + len(self.name)), nhead + ntail, bg)
        t = Text(self)
        t.add(back[:nhead * rb].tobytes())
        for s in self.specs:
            t.add_spec(s)
        t.add(back[nhead * rb:].tobytes())
        return t.finish()

    # ---- long texts: records that outgrow their tile's look-ahead, planted in the first tile of a chunk ----------

    def long_spec(self, into, geom, where, target, L, seam, kind, n, rl, offsets=None, shift=None, filler=None):
        """a read of rl bases that holds the read of a short spec at its head, at its tail or inside; random bases around it
        (or what filler(rng, n) gives)"""
        rng, q = self.rng, self.seqs[target]
        around = filler or _rand
        assert (geom, where) in (('A', 'tail'), ('B', 'head')) or geom == 'Cr'
        for attempt in range(20):
            tmp = []
            p = self.spec(geom if geom != 'Cr' else 'Cr-0', target, L, seam, kind, n, into=tmp, offsets=offsets, **(dict(at=0, flank=0) if geom == 'Cr' else {}))
            fill = rl - len(p.read)
            a = 0 if where == 'head' else fill if where == 'tail' else rng.randrange(1, fill)
            read = around(rng, a) + p.read + around(rng, fill - a)
            plan = [(sp - a, ln) for sp, ln in p.plan]
            if alignments(read, q, self.cfg) == plan:
                break
        else:
            raise AssertionError('no filling for %s@%s on %d' % (geom, where, target))
        p.n, p.geom, p.plan, p.read, p.ro = len(into), '%s@%s' % (geom, where), plan, read, p.ro + a
        c = self._next(('shift', geom, where), range(1 << 20))              # (hits and their twins both go through the four residues)
        p.bases, p.scores, p.lead, p.long, p.shift = read, b'I' * rl, 0, True, (c + c // 2) % 4 if shift is None else shift
        into.append(p)
        return p

    def lds_spec(self, into, target, rl, shift):
        """a read around the bound of the long matcher's LDS buffer: the sequence at its head and flush with its tail,
        maxerrors mismatches each"""
        rng, q = self.rng, self.seqs[target]
        tmp = []
        for seam in ('first', 'last'):
            self.spec('Cr-0', target, len(q), seam, self._next('ldsk', KINDS), self.e, into=tmp, at=0, flank=0)
        while True:
            read = tmp[0].read + _rand(rng, rl - 2 * len(q)) + tmp[1].read
            plan = [(0, len(q)), (-(rl - len(q)), len(q))]
            if alignments(read, q, self.cfg) == plan:
                break
        p = tmp[0]
        p.n, p.geom, p.plan, p.read, p.ro = len(into), 'lds', plan, read, 0
        p.bases, p.scores, p.lead, p.long, p.shift = read, b'I' * rl, 0, True, shift
        into.append(p)
        return p

    def long_specs(self):
        rng = self.rng = random.Random(4711)
        e, mo, nr = self.e, self.mo, self.nr
        out = []
        # around rl + (ro & 3) <= 16384, the bytes of the staged read
        for rl, shift in LDS_READS:
            self.lds_spec(out, nr[65], rl, shift)
        lens = itertools.cycle((1024, 1025, 1026, 1100, 1027, 2047, 1024, 2048, 1029, 2049, 1031, 3000, 1028))
        # overlap lengths and seams at the read's tail (A: the overlap ends on the read's last byte) and head (B)
        # (every overlap length with one of its seams, then every seam class at an overlap length that has it)
        ls = list(range(mo, mo + 17)) + list(LONG_OVERLAPS)
        pairs = [(L, self._next('lgs', sorted(seam_places(L, rng)))) for L in ls]
        pairs += [(self._next(('lgl', seam), [L for L in ls if seam in seam_places(L, rng)]), seam) for seam in seam_classes(ls)]
        for L, seam in pairs:
            for geom, where in (('A', 'tail'), ('B', 'head')):
                kind = self._next(('lgk', geom), KINDS)
                t = self._next('lgt', [nr[n] for n in (300, 4095) if n > L + 1])
                rl = next(lens)
                for n in (e, e + 1):
                    self.long_spec(out, geom, where, t, L, seam, kind, n, rl)
        # whole sequences at the head, at the tail and inside
        for t in (nr[63], nr[64], nr[65], nr[129], nr[300]):
            L = len(self.seqs[t])
            for where in ('head', 'tail', 'inside'):
                seam, kind = self._next(('lg', 'Cr'), sorted(seam_places(L, rng))), self._next(('lgk', 'Cr'), KINDS)
                rl = next(lens)
                for n in (e, e + 1):
                    self.long_spec(out, 'Cr', where, t, L, seam, kind, n, rl)
        # the prefilter: mismatches inside the first eight bases of the sequence
        for offs in ((0, 7), (3, 4), (0, 3, 7), (1, 2, 6), (4, 5, 6, 7)):
            offs = offs[:e + 1]
            for geom, where, t, L in (('Cr', 'inside', nr[129], 129), ('Cr', 'tail', nr[64], 64), ('A', 'tail', nr[300], 100)):
                self.long_spec(out, geom, where, t, L, None, self._next('pfk', KINDS), len(offs), next(lens), offsets=offs)
        return out

    def _head(self, t, back, nback):
        while t.nbytes < (128 << 10) + 8192:
            t.add(back[next(nback)].tobytes())

    def long_text(self):
        """-> (text, chunk offsets): behind the head, chunks whose first tile leaves records to the redo of skipped tiles.  A tile
        that cannot hold its last record (it ends beyond the tile's look-ahead) keeps the others and leaves that one: a chunk
        for each read around the LDS bound.  A tile whose window holds more newlines than its table leaves all its records:
        a chunk of one tile each, one-base records (too short to be scanned) among the other long reads and the short spec records"""
        g = synth.genome()
        rb = synth.record_bytes(150)
        back = synth.reads(g, 777000, 1200, 150).reshape(1200, rb)
        nback = iter(range(1200))
        t = Text(self)
        co = [0]
        self._head(t, back, nback)
        longs = self.long_specs()
        # (the short spec records: every fifth pair of a hit and its twin with one mismatch more)
        shorts = [s for s in self.specs if s.n % 10 < 2]
        payload = [s for s in longs if s.geom != 'lds'] + shorts
        t.n_long, t.n_short, t.n_left = len(longs), len(shorts), 0
        for last in (s for s in longs if s.geom == 'lds'):
            co.append(t.nbytes)
            begin = t.nbytes
            rec_len = len(self.record(last, 0)[0]) + 3                    # (the padding for its shift: up to three bytes)
            lo, hi = TILE_OWNS + LOOKAHEAD + 160 - rec_len + 8, TILE_OWNS - 160 - 8
            while t.nbytes - begin <= lo:
                t.add(back[next(nback)].tobytes())
            assert lo < t.nbytes - begin < hi
            t.add_spec(last); t.n_left += 1
            assert t.nbytes - begin > TILE_OWNS + LOOKAHEAD + 160
            for _ in range(10):
                t.add(back[next(nback)].tobytes())
        ntiny = BP_NLCAP // 4 + 20
        while payload:
            co.append(t.nbytes)
            begin = t.nbytes
            room = TILE_OWNS - 64 - ntiny * len(TINY1)
            group = []
            while payload and sum(len(self.record(s, 0)[0]) + 3 for s in group + payload[-1:]) <= room:
                group.append(payload.pop())
            for i, s in enumerate(group):
                for _ in range(ntiny * (i + 1) // len(group) - ntiny * i // len(group)):
                    t.add(TINY1)
                t.add_spec(s)
            t.n_left += ntiny + len(group)
            assert t.nbytes - begin < TILE_OWNS - 16 and 4 * (ntiny + len(group)) > BP_NLCAP
        co.append(t.nbytes)
        return t.finish(), np.array(co, dtype=np.int64)

    def flood_table(self):
        """the table of the cap text: the seeded sequences, and behind them eight that begin with 40 bases of one repeat in its eight
        phases -- a read made of that repeat has a candidate at every position the seed filter looks at, many times what a
        wave's queue holds (96)"""
        rng = random.Random(4713)
        seqs = self.seqs_kept + [(FLOOD_UNIT * 6)[ph:ph + 40] + _rand(rng, 20) for ph in range(8)]
        assert all(KM.seedable(q, self.k, self.e) for q in seqs) and KM.index_stride(seqs, self.k, self.e) == self.stride
        assert not KM.index_dense(seqs, self.k, self.e, self.stride)                # (the halving kernel: the draining ones empty their queues)
        return seqs

    def cap_text(self):
        """-> (text, long reads): one read of 1024 bases more than the list of long reads holds, in one launch, one behind the
        other: reads made of the repeat of flood_table (every eighth holds a spec's sequence at its head, at its tail or
        inside).  Such a read floods its wave's queue even alone and the scan kernel puts it on the redo's list of long reads
        itself; the last record of a tile outgrows the look-ahead and reaches the same list, and the same counter, through
        kvq_trim_records.  What comes when the list is full stays an ordinary record of the redo, for kvq_match_all"""
        g = synth.genome()
        rb = synth.record_bytes(150)
        back = synth.reads(g, 779000, 500, 150).reshape(500, rb)
        nback = iter(range(500))
        rng = self.rng = random.Random(4714)
        t = Text(self)
        self._head(t, back, nback)
        specs = []
        total = KVQ_LONG_CAP + 1
        targets = [self.nr[n] for n in (63, 64, 65, 129, 300)]

        def repeat(rng, n):
            ph = rng.randrange(8)
            return (FLOOD_UNIT * (n // 8 + 2))[ph:ph + n]
        for i in range(total):
            if i % 8 == 0:
                tg = targets[(i // 8) % len(targets)]
                L = len(self.seqs[tg])
                s = self.long_spec(specs, 'Cr', ('head', 'tail', 'inside')[(i // 8) % 3], tg, L, self._next('floodseam', sorted(seam_places(L, rng))),
                                   self._next('floodkind', KINDS), self.e + (i // 8) % 2, 1024, filler=repeat)
                s.shift = None
                t.add_spec(s, name=b'@C%07d' % i)
            else:
                t.add(b'@C%07d\n' % i + repeat(rng, 1024) + b'\n+\n' + b'I' * 1024 + b'\n')
        for _ in range(20):
            t.add(back[next(nback)].tobytes())
        return t.finish(), total

    def overflow_text(self):
        """-> (text, chunk offsets, long reads): tiles that leave more records than the redo's list holds.  2049 reads of 1024
        bases, seventeen a tile among 490 one-base records that overflow the tile's newline table, are 61000 records where the
        list holds 14336: kvq_dev_count fails the batch, and it is redone as a whole by the exhaustive kernels"""
        g = synth.genome()
        rb = synth.record_bytes(150)
        back = synth.reads(g, 778000, 500, 150).reshape(500, rb)
        nback = iter(range(500))
        rng = self.rng = random.Random(4712)
        t = Text(self)
        co = [0]
        self._head(t, back, nback)
        specs = []
        total, per, ntiny = KVQ_LONG_CAP + 1, 17, 490
        targets = [self.nr[n] for n in (63, 64, 65, 129, 300)]
        for i in range(total):
            if i % per == 0:
                co.append(t.nbytes)
                begin = t.nbytes
                t.add(TINY1 * ntiny)
            if i % 8 == 0:
                tg = targets[(i // 8) % len(targets)]
                L = len(self.seqs[tg])
                s = self.long_spec(specs, 'Cr', ('head', 'tail', 'inside')[(i // 8) % 3], tg, L, self._next('capseam', sorted(seam_places(L, rng))),
                                   'sub', self.e + (i // 8) % 2, 1024)
                s.shift = None
                t.add_spec(s, name=b'@C%07d' % i)
            else:
                t.add(b'@C%07d\n' % i + _rand(rng, 1024) + b'\n+\n' + b'I' * 1024 + b'\n')
            assert t.nbytes - begin < TILE_OWNS - 16
        t.n_left = total + ntiny * (len(co) - 1)
        co.append(t.nbytes)
        return t.finish(), np.array(co, dtype=np.int64), total


TILE_OWNS, LOOKAHEAD = 39760, 1040          # bytes a tile of 150-base records owns, and what it may look at behind them (tests/trim_matrix.py)
BP_NLCAP = 1920                             # newlines a tile's table holds (kernels_bp.hip)
KVQ_REDO_RECORDS = 16384 - 2048             # records the skipped tiles of one launch may leave (KVQ_REDO_CAP - KVQ_LONG_CAP)
FLOOD_UNIT = b'ACGTTGCA'
TINY1 = b'@\nA\n+\nI\n'                  # the shortest record there is
KVQ_LONG_READ, KVQ_LONG_CAP, KVQ_LONG_LDS = 1024, 2048, 16384          # kvq_device.h, kernels_general.hip
# (read length, residue of its stream offset modulo 4): on both sides of rl + residue <= KVQ_LONG_LDS
LDS_READS = ((16380, 0), (16380, 3), (16381, 3), (16382, 2), (16383, 1), (16384, 0),
             (16381, 0), (16382, 3), (16383, 2), (16384, 1), (16385, 0), (16385, 3), (16386, 2))
assert sum(rl + sh <= KVQ_LONG_LDS for rl, sh in LDS_READS) >= 6 and sum(rl + sh > KVQ_LONG_LDS for rl, sh in LDS_READS) >= 6
assert set(sh for rl, sh in LDS_READS if rl + sh <= KVQ_LONG_LDS) == set(range(4)) == set(sh for rl, sh in LDS_READS if rl + sh > KVQ_LONG_LDS)


class Text(object):
    """a FastQ text; its spec records: where each starts, ends and where its trimmed read starts"""

    def __init__(self, cell):
        self.cell, self.parts, self.nbytes = cell, [], 0
        self.specs, self.starts, self.ends, self.reads = [], [], [], []

    def add(self, raw):
        self.parts.append(raw); self.nbytes += len(raw)

    def add_spec(self, s, name=None):
        rec, off = self.cell.record(s, self.nbytes)
        if name is not None:
            head = rec[:rec.index(b'\n')]
            rec, off = name + rec[len(head):], off - len(head) + len(name)
        assert s.shift is None or (self.nbytes + off) % 4 == s.shift
        self.specs.append(s); self.starts.append(self.nbytes); self.reads.append(self.nbytes + off)
        self.add(rec); self.ends.append(self.nbytes)

    def finish(self):
        self.data = np.frombuffer(b''.join(self.parts), dtype=np.uint8)
        self.parts = None
        assert self.data.nbytes == self.nbytes
        return self

    def spec_at(self, file_pos):
        """the number, in this text, of the spec whose record holds a stream offset, or None"""
        i = bisect.bisect_right(self.starts, file_pos) - 1
        return i if i >= 0 and file_pos < self.ends[i] else None

    def by_spec(self, hits):
        """{number of the spec in this text: [(file_pos, seq_pos, length, readlength)]} of the hits of the spec records on
        their targets, in order"""
        out = {}
        for h in hits:
            i = self.spec_at(h.file_pos)
            if i is not None and h.seq_nr == self.specs[i].target:
                out.setdefault(i, []).append((h.file_pos, h.seq_pos, h.length, h.readlength))
        return out

    def planned(self, nseq):
        """the same from the statement's plan, for the targets a table of nseq sequences holds"""
        return dict((i, [(self.reads[i], p, ln, len(s.read)) for p, ln in s.plan]) for i, s in enumerate(self.specs) if s.plan and s.target < nseq)


@functools.lru_cache(maxsize=None)
def cell(name):
    return Cell(name)


@functools.lru_cache(maxsize=None)
def long_text():
    return cell('P').long_text()


@functools.lru_cache(maxsize=None)
def cap_text():
    return cell('P').cap_text()


@functools.lru_cache(maxsize=None)
def overflow_text():
    return cell('P').overflow_text()
