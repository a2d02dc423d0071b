"""
Tables that take the seed index (kvq_seed_index_build, kernels_seeded.hip) to its seams, and texts aimed at them.

Every hit of the product path comes through that index, and three kernels that share no code (bp_verify_rest,
kvq_verify_survivors, kvq_seed_list) must each emit every diagonal exactly once from it: each states "the canonical
discoverer" -- the first live seed in the order fixed read blocks, then anchor blocks -- for itself, and each unpacks the
entry word ``pos:12 | seq_nr:20 | table offset:20 | length:12`` on its own.  On unique random sequences all seeds of a
diagonal are live and no second diagonal exists, so the other matrices cannot see a wrong dedup; no other table has 65 536
sequences or a megabase.  Three families:

R   tandem repeats of periods 1, 2, 3, 4, 5, 7, 8 and 16 on both strands, in the product's cell (K = 8, halving kernel) and
    the draining cells of K = 6 and K = 5, each at the index strides 2, 4 and 8.  Two texts a cell: *light* reads hold 25 to
    60 bases of a repeat between random flanks and at most 64 positions with a K-mer in either bitmap (below ST_QW: they
    cannot flood a wave's queue); *heavy* reads are 150 bases (one: 1500) of pure repeat, hundreds of hits each.
T   twins and nesting: one sequence at two numbers far apart, a sequence beside its prefix, suffix and infix, pairs that
    differ in one base (in anchor block 0, in block maxerrors, outside every block), a reverse-complement palindrome, a
    G-rich sequence (G has code 3: its entries close ent[]) and A x 64 (code 0, as the padding of SeedEntry.ctx).
F   the 20-bit fields: F-offset fills the table to offset 2^20 with 256 sequences of 4095 bases, so that one seeded sequence
    straddles 2^20, the next are refused for their offset alone, and the index holds more than 2^20 entries; F-number holds
    87 500 sequences of 12 bases: number 87 381 is the last one below offset 2^20.

A record (``@T<family>.<n>``, n indexes ``Make.specs``) aims one diagonal of one sequence: with maxerrors mismatches, and its
twin with one more.  The mismatches kill the first 0 .. maxerrors blocks of the canonical order on the head side, the tail
side or the anchor blocks, on the first or the last base of a block, with the byte kinds of match_matrix.write_byte.  What a
record hits, on the aimed sequence and on every other target it names, is what match_matrix.alignments says (the plain
statement of workhorse.c:1112-1174; the length gate of workhorse.c:1100 in front of it): on repeats that is dozens of
diagonals.  tests/test_table_seams_host.py holds the oracle to that and counts what the families reach;
tests/test_gpu_table_seams.py runs them through the library's routes.

For the census only, ``Index`` restates the bitmaps, the work items and the canonical order; no assertion on the library's
results depends on it.
"""
import bisect
import collections
import functools
import random

import numpy as np

import kernel_matrix as KM
import match_matrix as MM
from kvarq_amd import synth

ST_QW, ST_Q2W = 112, 256            # candidates and work items a wave's queues hold (kernels_seeded.hip)
LIGHT_BOUND = 64                    # positions with a K-mer in either bitmap a light read may have
UNITS = (b'A', b'AC', b'ACG', b'ACGT', b'ACGTT', b'ACGTTGC', b'ACGTTGCA', b'ACGGTCATTGCAAGTC')
CONFIGS = {'P': KM.CONFIGS[8], 'K6': KM.CONFIGS[6], 'K5': KM.CONFIGS[5]}
STRIDES = (2, 4, 8)
SIDES = ('head', 'tail', 'anchor')
KINDS = MM.KINDS
TRIMMED = {8: (16, 24, 32, 40), 5: (10, 15, 20)}        # read lengths at which head and tail blocks coincide
PAD_TO = 200                        # bytes of a record at least: a tile never holds more records than its tables do
R_CELLS = [(c, s) for c in ('P', 'K6', 'K5') for s in STRIDES]
T_CELLS = [('P', 8), ('K6', 4), ('K5', 2)]


def planned(read, seq, cfg):
    """match_matrix.alignments behind the length gate (workhorse.c:1100)"""
    return MM.alignments(read, seq, cfg) if len(read) >= cfg['minreadlength'] else []


def codes(b):
    """the 2-bit codes of bytes: (byte >> 1) & 3"""
    return bytes((c >> 1) & 3 for c in b)


def _rand(rng, n):
    return bytes(rng.choice(b'ACGT') for _ in range(n))


def offsets_of(seqs):
    out = [0]
    for q in seqs:
        out.append(out[-1] + len(q))
    return out


def seeded_of(seqs, k, e):
    """which sequences the seed index takes: KM.seedable, a table offset and a number below 2^20"""
    off = offsets_of(seqs)
    return [KM.seedable(q, k, e) and off[i] < (1 << 20) and i < (1 << 20) for i, q in enumerate(seqs)]


class Index(object):
    """kvq_seed_index_build restated for the census: the entries each K-mer code has in the anchors' index and in the index
    of all positions (a code is in a bitmap when it has an entry there), and the canonical order"""

    def __init__(self, seqs, k, e):
        self.k, self.e = k, e
        kept = [q for q, sd in zip(seqs, seeded_of(seqs, k, e)) if sd]
        self.stride = KM.index_stride(kept, k, e)
        self.pitch = KM.pitch_of(k, self.stride)
        self.anc, self.all = collections.Counter(), collections.Counter()
        for q in kept:
            c = codes(q)
            for j in range(e + 1):
                for sft in range(self.stride):
                    o = j * self.pitch + sft
                    self.anc[c[o:o + k]] += 1
            for p in range(len(q) - k + 1):
                self.all[c[p:p + k]] += 1
        self.entries = sum(self.anc.values()) + sum(self.all.values())

    def fixed(self, rl):
        """read positions of the fixed blocks looked up in the index of all positions: head blocks, and the tail blocks that
        are not head blocks too"""
        k, e = self.k, self.e
        head = [j * k for j in range(e + 1) if (j + 1) * k <= rl]
        tail = [rl - (j + 1) * k for j in range(e + 1)]
        return head + [p for p in tail if p >= 0 and not (p % k == 0 and p <= e * k)]

    def candidates(self, read):
        """positions of the read with a K-mer in either bitmap (what the light reads are bounded by)"""
        c, k = codes(read), self.k
        return sum(1 for p in range(len(c) - k + 1) if c[p:p + k] in self.anc or c[p:p + k] in self.all)

    def work_items(self, read):
        """(candidate, index entry) pairs of a read: its lookups at multiples of the stride in the anchors' index, its fixed
        blocks in the index of all positions"""
        c, k = codes(read), self.k
        return (sum(self.anc.get(c[p:p + k], 0) for p in range(0, len(c) - k + 1, self.stride)) +
                sum(self.all.get(c[p:p + k], 0) for p in self.fixed(len(c))))

    def discoverer(self, r, q, d):
        """the first live seed of diagonal d (sequence index = read index + d) of coded read r on coded sequence q: ('F', read
        position) of a fixed block, by position, then ('A', sequence offset) of an anchor block, by offset; None: no seed"""
        k = self.k

        def live(rp, sq):
            return rp >= 0 and rp + k <= len(r) and sq >= 0 and sq + k <= len(q) and r[rp:rp + k] == q[sq:sq + k]
        for p in sorted(self.fixed(len(r))):
            if live(p, p + d):
                return ('F', p)
        for j in range(self.e + 1):
            for sft in range(self.stride):
                o = j * self.pitch + sft
                if (o - d) % self.stride == 0 and live(o - d, o):
                    return ('A', o)
        return None


class Spec(object):
    __slots__ = ('n', 'fam', 'side', 'dead', 'kind', 'nmis', 'target', 'targets', 'd', 'trimmed', 'offs', 'read', 'bases', 'scores', 'lead',
                 'plan', 'hit', 'unit', 'phase')

    def __repr__(self):
        return 'T%s.%d(%s, %d dead, %s, %d mismatches at %s, diagonal %d of seq %d, rl=%d: %s)' % (
            self.fam, self.n, self.side, self.dead, self.kind, self.nmis, list(self.offs), self.d, self.target, len(self.read),
            'hit' if self.hit else 'none')

    @property
    def cls(self):
        return (self.dead, self.side, self.kind)


class Make(object):
    """a table, its configuration and one text of records aimed at it"""

    def __init__(self, fam, cell, cfg, seqs, seed, index=True):
        self.fam, self.cell, self.cfg, self.seqs = fam, cell, dict(cfg), list(seqs)
        self.e, self.mo, self.mrl = cfg['maxerrors'], cfg['minoverlap'], cfg['minreadlength']
        self.k = KM.seed_k(cfg)
        self.seeded = seeded_of(self.seqs, self.k, self.e)
        kept = [q for q, sd in zip(self.seqs, self.seeded) if sd]
        self.stride = KM.index_stride(kept, self.k, self.e)
        self.pitch = KM.pitch_of(self.k, self.stride)
        self.index = Index(self.seqs, self.k, self.e) if index else None
        self.rng = random.Random(seed)
        self.specs = []
        self.bound = None               # positions with a K-mer in either bitmap a read may have
        self.turn = {}

    def _next(self, key, choices):
        n = self.turn.get(key, 0); self.turn[key] = n + 1
        return choices[n % len(choices)]

    # ---- geometry: (read without mismatches, the aimed overlap [lo, hi) of it, the diagonal) -------------------------

    def around(self, t, side, total=None, phase=None, bare=None):
        """the read of a spec between random flanks: the sequence's tail at its head (head), the sequence's head at its tail
        (tail), a piece of the sequence and nothing else (either, no flank), the whole sequence inside (anchor).  `total`:
        the read's length; `phase`: (period, wanted offset of the piece in the sequence modulo the period); `bare`: no flank"""
        rng, q = self.rng, self.seqs[t]
        L = len(q)
        if side == 'anchor':
            if total is not None:
                f1 = rng.randrange(0, total - L + 1); f2 = total - L - f1
            else:
                f1, f2 = rng.choice((0, rng.randrange(1, 21))), rng.choice((0, rng.randrange(1, 21)))
                if f1 + f2 == 0:
                    f2 = rng.randrange(1, 21)
            return _rand(rng, f1) + q + _rand(rng, f2), f1, f1 + L, -f1
        lo_ov, hi_ov = max(self.mo, (self.e + 1) * self.k + 1), min(60, L)        # (room for the twin's mismatch behind the blocks)
        assert lo_ov <= hi_ov, (t, L)
        ovs = list(range(lo_ov, hi_ov + 1))
        f = 0 if (rng.randrange(2) if bare is None else bare) and total is None else rng.randrange(5, 21)
        if f == 0:
            places = [(a, ov) for ov in ovs for a in range(L - ov + 1)]
            if phase is not None:
                places = [x for x in places if x[0] % phase[0] == phase[1]] or places
            a, ov = rng.choice(places)
            return q[a:a + ov], 0, ov, a
        if side == 'head' and phase is not None:
            ovs = [ov for ov in ovs if (L - ov) % phase[0] == phase[1]] or ovs
        ov = rng.choice(ovs)
        if total is not None:
            f = total - ov
        if side == 'head':
            return q[L - ov:] + _rand(rng, f), 0, ov, L - ov
        return _rand(rng, f) + q[:ov], f, f + ov, -f

    def pure(self, unit, t, side, rl):
        """a read of rl bases of the repeat alone, in the phase of one diagonal of sequence t (a cut of the same repeat)"""
        rng, q, P = self.rng, self.seqs[t], len(unit)
        L = len(q)
        rep = lambda ph: (unit * (rl // P + 3))[ph:ph + rl]
        if side == 'anchor':
            a = rng.randrange(0, rl - L + 1)
            return rep((-a) % P), a, a + L, -a
        ov = rng.randrange(max(self.mo, (self.e + 1) * self.k + 1), L)
        if side == 'head':
            return rep((L - ov) % P), 0, ov, L - ov
        return rep((ov - rl) % P), rl - ov, rl, ov - rl

    # ---- mismatches ------------------------------------------------------------------------------------------------

    def aim(self, side, dead, kind, target, targets, geom, counts=None, trimmed=False, unit=None):
        """the specs of one aimed diagonal, one for each number of mismatches in `counts` (maxerrors and maxerrors + 1): the
        first `dead` blocks of the side each take one, on their first or last base, the others fall behind block `dead`,
        which stays alive; the spec with more mismatches has those of the one with fewer"""
        rng, k, e = self.rng, self.k, self.e
        body, lo, hi, d = geom
        rl = len(body)
        counts = (e, e + 1) if counts is None else counts
        if side == 'head':
            blocks = [j * k for j in range(e + 1)]
        elif side == 'tail':
            blocks = [rl - (j + 1) * k for j in range(e + 1)]
        else:
            blocks = [j * self.pitch + d % self.stride - d for j in range(e + 1)]
        inside = [b for b in blocks if lo <= b and b + k <= hi]
        dead = min(dead, max(0, len(inside) - 1), min(counts))
        turn = self._next('edge', (0, 1))
        offs = [inside[j] + (0 if (j + turn) % 2 == 0 else k - 1) for j in range(dead)]
        closed = set(x for b in inside[:dead + 1] for x in range(b, b + k))
        free = [x for x in range(lo, hi) if x not in closed]
        rng.shuffle(free)
        spare = [x for x in range(lo, hi) if x not in offs and x not in free]
        rng.shuffle(spare)
        offs += (free + spare)[:max(counts) - dead]
        assert len(offs) == max(counts), (side, dead, lo, hi)
        out = []
        for nmis in counts:
            s = Spec()
            s.n = len(self.specs) + len(out)
            b = bytearray(body)
            for j, o in enumerate(offs[:nmis]):
                b[o] = MM.write_byte(kind, s.n - len(out) + j, body[o])
                assert b[o] != body[o]
            s.fam, s.side, s.dead, s.kind, s.nmis, s.target, s.targets, s.d = self.fam, side, dead, kind, nmis, target, tuple(targets), d
            s.trimmed, s.offs, s.read, s.unit, s.phase = trimmed, tuple(sorted(offs[:nmis])), bytes(b), unit, None
            s.plan = dict((t, planned(s.read, self.seqs[t], self.cfg)) for t in s.targets)
            s.hit = any(sp == d for sp, ln in s.plan[target])
            assert s.hit == (nmis <= e and rl >= self.mrl), s
            # flanks with scores below Amin: the trim leaves exactly the read
            fl = (rng.randrange(3, 9), rng.randrange(3, 9)) if trimmed else (rng.randrange(0, 9), rng.randrange(0, 9)) if (s.n // 2) % 2 else (0, 0)
            a, z = _rand(rng, fl[0]), _rand(rng, fl[1])
            s.bases, s.scores, s.lead = a + s.read + z, b'#' * len(a) + b'I' * rl + b'#' * len(z), len(a)
            out.append(s)
        return out

    def add(self, make):
        """the specs make() gives, drawn again until every read stays within the bound"""
        for attempt in range(60):
            got = make()
            if self.bound is None or all(self.index.candidates(s.read) <= self.bound for s in got):
                break
        else:
            raise AssertionError('no read within %d candidates' % self.bound)
        for s in got:
            assert s.n == len(self.specs)
            self.specs.append(s)
        return got

    def classes(self):
        return [(dead, side, kind) for dead in range(self.e + 1) for side in SIDES for kind in KINDS]

    # ---- the text --------------------------------------------------------------------------------------------------

    def record(self, s):
        head = b'@T%s.%d' % (self.fam.encode(), s.n)
        rest = b'\n' + s.bases + b'\n+\n' + s.scores + b'\n'
        pad = PAD_TO - len(head) - len(rest) - 1
        if pad >= 0:
            head += b' ' + b'p' * pad
        return head + rest, len(head) + 1 + s.lead

    def finish(self):
        self.starts, self.ends, self.reads, parts, at = [], [], [], [], 0
        for s in self.specs:
            rec, off = self.record(s)
            self.starts.append(at); self.reads.append(at + off)
            parts.append(rec); at += len(rec)
            self.ends.append(at)
        self.data = np.frombuffer(b''.join(parts), dtype=np.uint8)
        self.cut = self.starts[len(self.specs) // 2]            # where the text is cut in two batches
        return self

    def spec_at(self, file_pos):
        i = bisect.bisect_right(self.starts, file_pos) - 1
        return i if i >= 0 and file_pos < self.ends[i] else None

    def by_spec(self, hits):
        """{(spec, target): [(file_pos, seq_pos, length, readlength)]} of the hits of the records on their targets, in order"""
        out = {}
        for h in hits:
            i = self.spec_at(h.file_pos)
            if i is not None and h.seq_nr in self.specs[i].targets:
                out.setdefault((i, h.seq_nr), []).append((h.file_pos, h.seq_pos, h.length, h.readlength))
        return out

    def planned(self):
        """the same from the statement's plans"""
        return dict(((i, t), [(self.reads[i], p, ln, len(s.read)) for p, ln in pl]) for i, s in enumerate(self.specs)
                    for t, pl in s.plan.items() if pl)

    # ---- the census ------------------------------------------------------------------------------------------------

    def differing(self, s):
        """has the read two valid diagonals on one sequence whose canonical discoverers differ?"""
        r = codes(s.read)
        for t, pl in s.plan.items():
            diags = sorted(set(p for p, ln in pl))
            if len(diags) < 2:
                continue
            q, seen = codes(self.seqs[t]), set()
            for d in diags:
                seen.add(self.index.discoverer(r, q, d))
                if len(seen) > 1:
                    return True
        return False

    def census(self):
        hits = [sum(len(pl) for pl in s.plan.values()) for s in self.specs]
        out = collections.OrderedDict()
        out['sequences'], out['seeded'], out['bases'] = len(self.seqs), sum(self.seeded), sum(len(q) for q in self.seqs)
        out['K'], out['stride'] = self.k, self.stride
        out['records'], out['hit'], out['twins without'] = len(self.specs), sum(s.hit for s in self.specs), sum(not s.hit for s in self.specs)
        out['classes'] = len(set(s.cls for s in self.specs))
        out['planned hits'], out['most a read'] = sum(hits), max(hits)
        if self.index is not None:
            out['index entries'] = self.index.entries
            out['most candidates'] = max(self.index.candidates(s.read) for s in self.specs)
            out['most work items'] = max(self.index.work_items(s.read) for s in self.specs)
            out['reads with differing discoverers'] = sum(self.differing(s) for s in self.specs)
        return out


# ---------------------------------------------------------------------------------------------------------------
# R: repeats
# ---------------------------------------------------------------------------------------------------------------

def repeat_table(cfg, stride):
    """-> (both strands, {unit: numbers of its plus-strand cuts, and of the minus-strand ones where the unit is its own
    reverse complement}): every unit cut to span_of(2), span_of(4), span_of(8), 64 and 100 bases, without the cuts shorter
    than the stride's span; a repeat stands first and a repeat stands last"""
    k, e = KM.seed_k(cfg), cfg['maxerrors']
    lens = sorted(set([KM.span_of(k, e, s) for s in STRIDES if s >= stride] + [64, 100]))
    plus, of = [], {}
    for u in UNITS:
        for L in lens:
            of.setdefault(u, []).append(len(plus))
            plus.append((u * (L // len(u) + 1))[:L])
    seqs = synth.both_strands(plus)
    for u in UNITS:
        if synth.revcomp(u) in u + u:
            of[u] += [n + len(plus) for n in of[u]]
    return seqs, of


class Repeats(Make):
    def __init__(self, cell, stride, heavy):
        cfg = CONFIGS[cell]
        seqs, self.of = repeat_table(cfg, stride)
        Make.__init__(self, 'Rh' if heavy else 'Rl', (cell, stride), cfg, seqs, 1000 * stride + 10 * len(cell) + heavy)
        self.heavy = heavy
        assert self.stride == stride and all(self.seeded)
        assert cell != 'P' or not KM.index_dense(self.seqs, self.k, self.e, stride)
        if not heavy:
            self.bound = LIGHT_BOUND
        for rep in range(3 if self.e == 1 else 2):
            for dead, side, kind in self.classes():
                self.add(lambda: self._pair(self._next('unit', UNITS), side, dead, kind))
        if not heavy:
            # every phase of every unit: a piece of the repeat that begins there, for those the classes have left out
            have = set((s.unit, s.phase) for s in self.specs)
            for u, ph in [(u, ph) for u in UNITS for ph in range(len(u)) if (u, ph) not in have]:
                dead, side, kind = self._next('cover', self.classes())
                self.add(lambda: self._pair(u, side if side != 'anchor' else 'head', dead, kind, ph))
        # reads whose head and tail blocks coincide: trimmed by their scores to 2, 3, 4 and 5 blocks
        for rl in TRIMMED.get(self.k, ()):
            for side in ('head', 'tail'):
                for dead in range(self.e + 1):
                    self.add(lambda: self._trimmed(rl, side, dead))
        if heavy:
            u = UNITS[6]
            t = self.of[u][0]
            self.add(lambda: self.aim('anchor', 1, 'sub', t, self.of[u], self.pure(u, t, 'anchor', 1500), unit=u))
        self.finish()

    def _pair(self, u, side, dead, kind, ph=None):
        nrs = self.of[u]
        plus = [t for t in nrs if t < len(self.seqs) // 2]
        if side != 'anchor':
            plus = [t for t in plus if len(self.seqs[t]) >= 64]
        elif not self.heavy:
            plus = [t for t in plus if len(self.seqs[t]) <= 60]
        t = self.rng.choice(plus)
        if self.heavy:
            got = self.aim(side, dead, kind, t, nrs, self.pure(u, t, side, 150), unit=u)
        else:
            got = self.aim(side, dead, kind, t, nrs, self.around(t, side, phase=None if ph is None else (len(u), ph), bare=None if ph is None else 1), unit=u)
        for s in got:
            s.phase = s.d % len(u) if s.d > 0 else 0         # the phase of the unit the read's first repeat base stands on
        assert ph is None or got[0].phase == ph
        return got

    def _trimmed(self, rl, side, dead):
        u = self._next('tu', UNITS)
        t = [t for t in self.of[u] if len(self.seqs[t]) == 100][0]
        a = self.rng.randrange(0, 100 - rl + 1)
        q = self.seqs[t]
        return self.aim(side, dead, self._next('tk', KINDS), t, self.of[u], (q[a:a + rl], 0, rl, a), trimmed=True, unit=u)


# ---------------------------------------------------------------------------------------------------------------
# T: twins and nesting
# ---------------------------------------------------------------------------------------------------------------

class Twins(Make):
    def __init__(self, cell, stride):
        cfg = CONFIGS[cell]
        k, e = KM.seed_k(cfg), cfg['maxerrors']
        rng = random.Random(77 + stride)
        pitch = KM.pitch_of(k, stride)
        base = _rand(rng, 120)
        names, plus = [], []

        def put(name, q):
            names.append(name); plus.append(bytes(q))
        put('twin', base)
        put('prefix', base[:50]); put('suffix', base[-50:]); put('infix', base[30:80])
        for name, at in (('block0', 3), ('blocke', e * pitch + 3), ('outside', 72)):
            q = _rand(rng, 80)
            other = bytearray(q); other[at] = b'ACGT'[(b'ACGT'.index(q[at]) + 1) % 4]
            put(name, q); put(name + "'", other)
        half = _rand(rng, 30)
        put('palindrome', half + synth.revcomp(half))
        put('g-rich', b'G' * 12 + b''.join(b'GGG' + bytes([rng.choice(b'ACGT')]) for _ in range(13)))
        put('a64', b'A' * 64)
        if stride < 8:
            put('setter', _rand(rng, KM.span_of(k, e, stride)))
        put('twin-far', base)
        seqs = synth.both_strands(plus)
        self.names = names
        Make.__init__(self, 'T', (cell, stride), cfg, seqs, 500 + stride)
        assert self.stride == stride and all(self.seeded)
        assert seqs[names.index('palindrome')] == seqs[names.index('palindrome') + len(plus)]
        everything = list(range(len(seqs)))
        aims = [names.index(n) for n in names if n != 'setter']
        aims += [names.index('twin-far') + len(plus), names.index('g-rich') + len(plus)]
        for dead, side, kind in self.classes():
            for rep in range(2):
                t = self._next('aim', aims)
                self.add(lambda: self.aim(side, dead, kind, t, everything, self.around(t, side)))
        # A x 45 behind a flank: every shorter overlap with A x 64 is a diagonal of its own, and the read's fixed blocks leave
        # the sequence one after the other
        t = names.index('a64')
        f = k - 1                                                # (head block 1 lies on the sequence for two diagonals)
        for kind in KINDS:
            self.add(lambda: self.aim('tail', 1, kind, t, everything, (_rand(self.rng, f) + b'A' * 45, f, f + 45, -f)))
        self.finish()


# ---------------------------------------------------------------------------------------------------------------
# F: the 20-bit fields
# ---------------------------------------------------------------------------------------------------------------

class FOffset(Make):
    """256 sequences of 4095 bases, then one of 255 at offset 2^20 - 256, one of 60 at 2^20 - 1 (seeded: it begins below
    2^20) whose last 30 bases are G, and three of 60 at 2^20 + 59 and beyond (refused for their offset alone)"""

    def __init__(self):
        rs = np.random.RandomState(2020)
        fill = [np.frombuffer(b'ACGT', dtype=np.uint8)[rs.randint(0, 4, 4095)].tobytes() for _ in range(256)]
        rng = random.Random(2021)
        seqs = fill + [_rand(rng, 255), _rand(rng, 30) + b'G' * 30] + [_rand(rng, 60) for _ in range(3)]
        Make.__init__(self, 'Fo', 'offset', CONFIGS['P'], seqs, 2022, index=False)
        off = offsets_of(seqs)
        self.named = dict(s255=256, straddler=257, refused=(258, 259, 260), fillers=(0, 128, 255))
        assert off[256] == (1 << 20) - 256 and off[257] == (1 << 20) - 1 and off[258] == (1 << 20) + 59
        assert self.seeded == [True] * 258 + [False] * 3 and self.stride == 8
        aims = [256, 257, 258, 259, 0, 128, 255]
        for rep in range(2):
            for dead, side, kind in self.classes():
                t = self._next(side, [t for t in aims if side != 'anchor' or len(seqs[t]) <= 255])
                self.add(lambda: self.aim(side, dead, kind, t, (t,), self.around(t, side)))
        # the G-rich end of ent[]: reads whose first block is G x 8, the last code of the index of all positions
        for ov in (27, 30):
            self.add(lambda: self.aim('head', 0, 'sub', 257, (257,), (seqs[257][-ov:] + _rand(self.rng, 12), 0, ov, 60 - ov)))
        self.finish()


class FNumber(Make):
    """87 500 sequences of 12 bases (span_of(5, 1, 2)): number 87 381 at offset 1 048 572 is the last one the index takes"""
    PLANTED = (4095, 4096, 65535, 65536, 87381, 87382)

    def __init__(self):
        rs = np.random.RandomState(2023)
        a = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.randint(0, 4, (87500, 12))]
        seqs = [r.tobytes() for r in a]
        Make.__init__(self, 'Fn', 'number', CONFIGS['K5'], seqs, 2024, index=False)
        assert offsets_of(seqs)[87381] == 1048572 and self.seeded == [True] * 87382 + [False] * 118 and self.stride == 2
        for t in self.PLANTED:                                   # no mismatch at all
            self.add(lambda: self.aim('anchor', 0, 'sub', t, (t,), self.around(t, 'anchor', total=100), counts=(0,)))
        for dead, side, kind in self.classes():                  # maxerrors (1) and its twin
            t = self._next('aim', self.PLANTED)
            self.add(lambda: self.aim(side, dead, kind, t, (t,), self.around(t, side, total=100)))
        self.finish()


@functools.lru_cache(maxsize=None)
def repeats(cell, stride, heavy):
    return Repeats(cell, stride, heavy)


@functools.lru_cache(maxsize=None)
def twins(cell, stride):
    return Twins(cell, stride)


@functools.lru_cache(maxsize=None)
def f_offset():
    return FOffset()


@functools.lru_cache(maxsize=None)
def f_number():
    return FNumber()


# every text there is: (family, cell, stride, heavy)
MAKES = ([('R', c, s, h) for c, s in R_CELLS for h in (False, True)] + [('T', c, s, None) for c, s in T_CELLS] +
         [('Fo', None, None, None), ('Fn', None, None, None)])


def make_of(fam, c, s, h):
    return repeats(c, s, h) if fam == 'R' else twins(c, s) if fam == 'T' else f_offset() if fam == 'Fo' else f_number()


def make_id(m):
    fam, c, s, h = m
    return '-'.join([fam] + ([c, 's%d' % s] if c else []) + ([] if h is None else ['heavy' if h else 'light']))


def census_lines(makes):
    """the lines of profiles/table_seam_tests.txt for some texts"""
    out = []
    for w in makes:
        c = w.census()
        out.append('%-3s %-12s ' % (w.fam, '%s-s%s' % w.cell if isinstance(w.cell, tuple) else w.cell) + '  '.join('%s %s' % (k, v) for k, v in c.items()))
    return out
