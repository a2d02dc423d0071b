"""
Workloads that land the seed-filter scan on each instantiation of kvq_scan_bp the launcher can pick (a "cell":
seed length K, index stride, lane group, halving or draining kernel), the way production reaches it: through the
configuration (K, kvq_seed_k), the table (its shortest seeded sequence sets the stride, its density the kernel
family) and the head of the text (the average record sets the lane group).

Every text is synthetic background (synth.reads) plus planted records aimed at the places where a seed filter or
a lane split goes wrong; each planted record is named after its class (``@P<class>.<n>``) so that the oracle's
hits can be traced back to it (tests/test_kernel_dispatch.py checks that the workloads are not vacuous,
tests/test_gpu_kernel_matrix.py runs them on the GPU against the oracle).

``tiles_of`` counts the tiles of a text the way the launcher does, and ``long_walk`` is a text for the launches in
which one workgroup walks hundreds of tiles (a small KVQ_GRID): see LongWalk.
"""
import bisect
import ctypes as C
import random

import numpy as np

from kvarq_amd import _lib, scan, synth

CONFIGS = {
    8: dict(maxerrors=2, minoverlap=25, minreadlength=25, Amin='.'),        # the product's configuration
    7: dict(maxerrors=2, minoverlap=21, minreadlength=21, Amin='.'),
    6: dict(maxerrors=3, minoverlap=25, minreadlength=25, Amin='.'),
    5: dict(maxerrors=1, minoverlap=10, minreadlength=10, Amin='.'),
}

# (K, stride, lane group, draining kernel): 12 halving cells at K = 8, 6 draining ones, 6 for each K < 8
CELLS = ([(8, s, lg, False) for lg in (-1, 1, 2, 3) for s in (2, 4, 8)] +
         [(8, s, lg, True) for lg in (-1, 2) for s in (2, 4, 8)] +
         [(k, s, lg, True) for k in (7, 6, 5) for lg in (-1, 2) for s in (2, 4, 8)])

# read length of the background that gives a lane group (kvq_scan_kernel_pick: records a tile can own)
READ_LEN = {1: 75, 2: 150, 3: 300}
# a body that does not match the head: shorter reads (more than 512 >> LG records a tile, several passes), longer ones
BODY_LEN = {1: (40, 150), 2: (50, 300), 3: (100, 600)}


def cell_id(cell):
    k, s, lg, dense = cell
    return 'k%d-s%d-lg%s-%s' % (k, s, lg if lg >= 0 else 'x', 'drain' if dense else 'halve')


def seed_k(cfg):
    """kvq_seed_k"""
    return min(8, min(cfg['minoverlap'], cfg['minreadlength']) // (cfg['maxerrors'] + 1))


def pitch_of(k, stride):
    return (k + stride - 1) // stride * stride


def span_of(k, e, stride):
    """the shortest sequence whose `stride` shifted copies of the anchor blocks fit (kvq_seed_index_build)"""
    return pitch_of(k, stride) * e + k + stride - 1


def seedable(q, k, e):
    return span_of(k, e, 2) <= len(q) <= 4095 and all(c in b'ACGT' for c in q)


# index_stride and index_dense restate kvq_seed_index_build: on the CPU they only say that a workload was built as
# intended; that the library's own index lands on the cell is pinned by the GPU matrix (r['kernel'])
def index_stride(seqs, k, e):
    """the stride kvq_seed_index_build gives a table"""
    minlen = min(len(q) for q in seqs if seedable(q, k, e))
    return 8 if minlen >= span_of(k, e, 8) else 4 if minlen >= span_of(k, e, 4) else 2


def index_dense(seqs, k, e, stride):
    """SeedIndex::dense: the candidates a 150-base read of random bases would give exceed what a wave's queue holds"""
    code = {ord('A'): 0, ord('C'): 1, ord('G'): 2, ord('T'): 3}
    pitch = pitch_of(k, stride)
    anc, anywhere = set(), set()
    for q in seqs:
        if not seedable(q, k, e):
            continue
        codes = [code[c] for c in q]
        kmer = lambda p: tuple(codes[p:p + k])
        for j in range(e + 1):
            for sft in range(stride):
                anc.add(kmer(j * pitch + sft))
        for p in range(len(q) - k + 1):
            anywhere.add(kmer(p))
    nc = float(4 ** k)
    return len(anc) / nc * (150.0 / stride) + len(anywhere) / nc * 2 * (e + 1) > 5.0


def _rec(name, bases, quals=None):
    return b'@' + name.encode() + b'\n' + bases + b'\n+\n' + (quals if quals is not None else b'I' * len(bases)) + b'\n'


def _rand(rng, n):
    return bytes(rng.choice(b'ACGT') for _ in range(n))


def _mutate(rng, q, positions):
    b = bytearray(q)
    for p in positions:
        b[p] = b'ACGT'[(b'ACGT'.index(b[p]) + 1 + rng.randrange(3)) % 4]
    return bytes(b)


class Workload(object):
    """one cell's table, configuration and texts; `classes` maps each planted class to the table indices it aims at
    and whether the oracle must report a hit of them in its records (True) or must not (False)"""

    def __init__(self, cell, g=None, n_reads=None):
        self.cell = cell
        k, stride, lg, dense = cell
        self.k, self.stride, self.lg, self.dense = k, stride, lg, dense
        self.cfg = dict(CONFIGS[k])
        e, mo, mrl = self.cfg['maxerrors'], self.cfg['minoverlap'], self.cfg['minreadlength']
        assert seed_k(self.cfg) == k
        g = synth.genome() if g is None else g
        rng = random.Random(sum(ord(c) * 31 ** i for i, c in enumerate(cell_id(cell))))
        # the table: the MTBC templates (x 8 for the draining cells at K = 8) without the 25-base spacers, so that the
        # stride is set by one sequence of span_of(stride) bases; a sequence with an N and one shorter than span_of(2),
        # which the seed index refuses (the exhaustive kernels serve them)
        plus = [q for q in synth.table(g, 'MTBC', scale=8 if (k == 8 and dense) else 1) if len(q) >= 31]
        self.targets = list(range(0, 85, 7))                   # 51-base SNP templates the planted reads aim at
        at = 2000000 + 1000 * k + 100 * stride
        if stride < 8:
            plus.append(g[at:at + span_of(k, e, stride)].tobytes())
        self.setter = len(plus) - 1 if stride < 8 else None
        nq = bytearray(g[at + 200:at + 240].tobytes()); nq[17] = ord('N')
        plus.append(bytes(nq)); self.refused_n = len(plus) - 1
        plus.append(g[at + 400:at + 400 + span_of(k, e, 2) - 1].tobytes()); self.refused_short = len(plus) - 1
        self.plus = plus
        self.seqs = synth.both_strands(plus)
        self.np = len(plus)
        assert index_stride(self.seqs, k, e) == stride
        assert (k < 8) or index_dense(self.seqs, k, e, stride) == dense

        # planted records
        self.classes = {}
        planted = []
        pitch = pitch_of(k, stride)

        def add(cls, bases, tgt, want, quals=None, strand=0):
            aim = {tgt, tgt + self.np}
            prev = self.classes.get(cls)
            self.classes[cls] = ((prev[0] | aim) if prev else aim, want)
            if strand:
                bases = synth.revcomp(bases)
                quals = quals[::-1] if quals is not None else None
            planted.append(_rec('P%s.%d' % (cls, len(planted)), bases, quals))

        n = 0
        for rep in range(4):
            strand = rep & 1
            # seed blocks: e substitutions, one in every block but block j (its first base, its last, the middle)
            for j in range(e + 1):
                for where, off in (('first', 0), ('last', k - 1), ('mid', k // 2)):
                    ti = self.targets[n % len(self.targets)]; n += 1
                    q = _mutate(rng, plus[ti], [pitch * jj + off for jj in range(e + 1) if jj != j])
                    add('blk%d-%s' % (j, where), _rand(rng, rng.randrange(1, 30)) + q + _rand(rng, rng.randrange(1, 30)), ti, True, strand=strand)
            # e + 1 substitutions, one in every block: no hit
            ti = self.targets[n % len(self.targets)]; n += 1
            q = _mutate(rng, plus[ti], [pitch * jj + 1 for jj in range(e + 1)])
            add('over', _rand(rng, rng.randrange(1, 30)) + q + _rand(rng, rng.randrange(1, 30)), ti, False, strand=strand)
            # every residue of the read offset modulo the stride (8 covers 2 and 4), with e substitutions
            for d in range(8):
                ti = self.targets[n % len(self.targets)]; n += 1
                q = _mutate(rng, plus[ti], [pitch * jj + (d % k) for jj in range(e + 1) if jj != d % (e + 1)])
                lead, tail = _rand(rng, 8 * rng.randrange(1, 4) + d), _rand(rng, rng.randrange(1, 20))
                # (a reverse-strand record is complemented and reversed by add: its offset then comes from what stands behind)
                add('res%d' % d, (tail + q + lead) if strand else (lead + q + tail), ti, True, strand=strand)
            # read ends: class A (read tail = sequence head) and B (read head = sequence tail), overlaps around minoverlap,
            # e substitutions inside the overlap; the read end fixes the overlap, so minoverlap - 1 must not hit
            for ov in (mo - 1, mo, mo + 1):
                ti = self.targets[n % len(self.targets)]; n += 1
                q = plus[ti]
                errs = rng.sample(range(ov), e)
                add('endA%+d' % (ov - mo), _rand(rng, rng.randrange(20, 60)) + _mutate(rng, q[:ov], errs), ti, ov >= mo, strand=strand)
                add('endB%+d' % (ov - mo), _mutate(rng, q[-ov:], errs) + _rand(rng, rng.randrange(20, 60)), ti, ov >= mo, strand=strand)
            # class C: a read shorter than the sequence, e substitutions
            ti = self.targets[n % len(self.targets)]; n += 1
            q = plus[ti]
            rl = rng.randrange(mrl, len(q))
            a = rng.randrange(0, len(q) - rl + 1)
            add('inseq', _mutate(rng, q[a:a + rl], rng.sample(range(rl), e)), ti, True, strand=strand)
            # trimming: the first-longest run of good scores cuts into the planted sequence, or ends just past it
            ti = self.targets[n % len(self.targets)]; n += 1
            q = plus[ti]
            cut = rng.randrange(3, len(q) - mo - 3)
            b = _rand(rng, 10) + q + _rand(rng, 60)
            quals = bytearray(b'I' * len(b)); quals[10 + cut] = ord('#')
            add('trim-into', b, ti, True, bytes(quals), strand=strand)
            b = _rand(rng, 70) + q + _rand(rng, 10)
            quals = bytearray(b'I' * len(b)); quals[70 + len(q)] = ord('#')
            add('trim-past', b, ti, True, bytes(quals), strand=strand)
            # the length gate after trimming: minreadlength - 1 (no hit) and minreadlength good bases inside the sequence
            for extra, want in ((-1, False), (0, True)):
                ti = self.targets[n % len(self.targets)]; n += 1
                q = plus[ti]
                rl = mrl + extra
                a = rng.randrange(0, len(q) - rl + 1)
                b = _rand(rng, 15) + q[a:a + rl] + _rand(rng, 15)
                add('minrl%+d' % extra, b, ti, want, b'#' * 15 + b'I' * rl + b'#' * 15, strand=strand)
            # an N inside an otherwise matching window
            ti = self.targets[n % len(self.targets)]; n += 1
            q = bytearray(plus[ti]); q[rng.randrange(len(q))] = ord('N')
            add('nbase', _rand(rng, rng.randrange(1, 30)) + bytes(q) + _rand(rng, rng.randrange(1, 30)), ti, True, strand=strand)
            # the sequences the seed index refuses, and the one that sets the stride
            add('refused-n', _rand(rng, rng.randrange(1, 30)) + plus[self.refused_n] + _rand(rng, 20), self.refused_n, True, strand=strand)
            add('refused-short', _rand(rng, rng.randrange(1, 30)) + plus[self.refused_short] + _rand(rng, 20), self.refused_short, True, strand=strand)
            if self.setter is not None:
                q = _mutate(rng, plus[self.setter], [pitch * jj + 1 for jj in range(e)])
                add('setter', _rand(rng, rng.randrange(1, 30)) + q + _rand(rng, 20), self.setter, True, strand=strand)
        rng.shuffle(planted)
        self.planted = planted

        # the texts: background of the lane group's read length with the planted records behind the head (the first
        # 128 KiB set the tile and the lane group); for the fixed lane groups a second text whose body does not match its head
        L = READ_LEN.get(lg, 40 if stride != 4 else 600)
        if n_reads is None:
            n_reads = 20000 if L <= 75 else 12000 if L <= 150 else 6000 if L <= 300 else 2500
            if k == 8 and dense:
                n_reads //= 2                                  # (eight times the sequences: the oracle's time)
        self.read_len = L
        self.texts = [self._text(g, [(L, n_reads)], 7 * k + stride)]
        if lg > 0:
            short, long_ = BODY_LEN[lg]
            head = 140000 // synth.record_bytes(L) + 1
            self.texts.append(self._text(g, [(L, head), (short, 6000 // (2 if k == 8 and dense else 1)), (long_, 1000 if long_ <= 300 else 500)], 11 * k + stride))

    def _text(self, g, parts, first):
        """background parts [(read length, records)], the planted records spread over everything behind the first 128 KiB"""
        recs = []
        for L, n in parts:
            a = synth.reads(g, 1000 * first, n, L).reshape(n, synth.record_bytes(L))
            recs.extend(bytes(r) for r in a)
            first += 1
        head, nb = 0, 0
        while nb < (128 << 10) + 4096:
            nb += len(recs[head]); head += 1
        body = recs[head:]
        step = max(1, len(body) // (len(self.planted) + 1))
        out = recs[:head]
        for i, p in enumerate(self.planted):
            out.extend(body[i * step:(i + 1) * step])
            out.append(p)
        out.extend(body[len(self.planted) * step:])
        return np.frombuffer(b''.join(out), dtype=np.uint8)

    def record_names(self, text):
        """the record starts of a text and their names"""
        raw = text.tobytes()
        starts, names, at = [], [], 0
        while at < len(raw):
            nl = raw.index(b'\n', at)
            starts.append(at); names.append(raw[at + 1:nl].decode())
            for _ in range(4):
                at = raw.index(b'\n', at) + 1
        return starts, names

    def hits_by_class(self, text, hits):
        """{class: number of hits of the sequences it aims at in its records}, from an engine-shaped hit list"""
        starts, names = self.record_names(text)
        out = dict((c, 0) for c in self.classes)
        for h in hits:
            name = names[bisect.bisect_right(starts, h.file_pos) - 1]
            if name.startswith('P'):
                cls = name[1:].rsplit('.', 1)[0]
                if h.seq_nr in self.classes[cls][0]:
                    out[cls] += 1
        return out


# ---------------------------------------------------------------------------
# many tiles per workgroup
# ---------------------------------------------------------------------------

BP_SHARDS = 64                  # kernels_bp.hip: the shares the tiles of a launch are dealt into
ST_HIST_TILES = 100             # kernels_seeded.hip: tiles between two flushes of a workgroup's read-length histogram
ST_RCAP, BP_NLCAP = 512, 1920   # records and newlines a tile's tables hold (beyond: the tile leaves its records to the redo chain)
BP_WINDOW = 36640 + 4160 + 80   # bytes of text a tile looks at (ST_TILE + ST_OV behind its first byte, ST_PRE in front)


def tiles_of(text):
    """(bytes a tile owns, [tiles of every chunk]) of a text scanned as ONE host batch: kvq_tile_for_text on its first
    128 KiB, the chunk cuts of kvq_chunk_offsets and kvq_seeded_launch's count per chunk"""
    arr = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    tile = _lib.lib().kvq_tile_for_text(arr.ctypes.data, min(arr.nbytes, 128 << 10), None)
    co = [int(x) for x in scan.chunk_offsets(arr)]
    return tile, [((b - (a & ~15)) + tile - 1) // tile if b > a else 0 for a, b in zip(co[:-1], co[1:])]


def shard_begin(sh, ntiles):
    """bp_shard_begin: the first tile of share sh"""
    return sh * ntiles // BP_SHARDS


class LongWalk(object):
    """One text of at least 256 tiles of the most records a tile holds, for launches in which a workgroup walks all of
    them (KVQ_GRID=1) or a fifth: every share of the tiles holds four or more, so a workgroup stays in its share for
    several tiles before it looks for another, and a lone workgroup flushes its read-length histogram twice.

    The records are 88 bytes (a two-character name, 40 bases, all scores 'I'), one in a hundred 90 (41 bases): that is
    about 452 records a tile and 1860 newlines in a tile's window, as close to BP_NLCAP as four-line records of an
    even read length get (38 bases: 1943) -- BP_NLCAP, not ST_RCAP, is what a tile of short records runs into.  40 is
    even, so its counts sit in the LOW half of a histogram word (two 16-bit bins a word): without the flush every
    ST_HIST_TILES tiles a lone workgroup counts all the text's 40-base reads, more than 65535, in that half and the
    carry lands in the bin of 41.

    Every hundredth read is cut from a template (inside it with 0, 1 or 2 substitutions, or overlapping one of its
    ends by 10..39 bases), the rest are random bases; the table holds seedable sequences only (40 SNP templates and
    their reverse complements), so no other kernel sees a record.  Two configurations: K = 5 (draining) and the
    product's (K = 8, halving); both land on the kernel that works the lane group out per tile."""

    READ, ODD = 40, 41
    CELLS = ((5, 8, -1, True), (8, 8, -1, False))

    def __init__(self, g=None, n_reads=120000):
        g = synth.genome() if g is None else g
        self.plus = [q for q in synth.table(g) if len(q) == 51][:40]
        self.seqs = synth.both_strands(self.plus)
        self.cfgs = [dict(CONFIGS[k]) for k, _, _, _ in self.CELLS]
        for (k, stride, _, dense), cfg in zip(self.CELLS, self.cfgs):
            e = cfg['maxerrors']
            assert seed_k(cfg) == k and all(seedable(q, k, e) for q in self.seqs)
            assert index_stride(self.seqs, k, e) == stride and (k < 8 or index_dense(self.seqs, k, e, stride) == dense)
        rng = random.Random(20240)
        bases = np.frombuffer(b'ACGT', dtype=np.uint8)[np.random.RandomState(20240).randint(0, 4, (n_reads, self.ODD))]
        names = b'0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
        out, self.n_even, self.n_planted = [], 0, 0
        for i in range(n_reads):
            L = self.ODD if i % 100 == 37 else self.READ
            b = bases[i, :L].tobytes()
            if i % 100 == 50:
                j = i // 100
                q = self.seqs[rng.randrange(len(self.seqs))]
                if j % 4 < 3:
                    a = rng.randrange(0, len(q) - L + 1)
                    b = _mutate(rng, q[a:a + L], rng.sample(range(L), j % 4))
                else:
                    ov = 10 + (j // 4) % 30
                    b = (b[:L - ov] + q[:ov]) if (j // 4) & 1 else (q[-ov:] + b[ov:])
                self.n_planted += 1
            self.n_even += L == self.READ
            out.append(_rec(chr(names[i % 62]) + chr(names[i // 62 % 62]), b))
        self.n_reads = n_reads
        self.text = np.frombuffer(b''.join(out), dtype=np.uint8)


_long_walk = []


def long_walk(g=None):
    """the LongWalk, built once a process (nothing may change it)"""
    if not _long_walk:
        _long_walk.append(LongWalk(g))
    return _long_walk[0]
