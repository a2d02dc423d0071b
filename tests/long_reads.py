"""
Texts and tables for the read-list route (``long_reads``): reads of thousands of bases cut from random
bases with sequences planted where ``kvq_seed_list`` can go wrong -- every class of alignment, every subset of a job's seed
blocks broken, the seams of its 1 KiB walk and of its 16-byte lanes, bytes that share a 2-bit code, reads beyond 65535
bases, a read that floods the candidate queue, every stride and seed length of the index.

A ``Text`` holds the FastQ bytes, the sequence list, the engine config and ``want``: the hits its builder planted on purpose,
as (label, Hit fields, how often the oracle must report exactly these fields).  The oracle is the judge of everything else a
text happens to contain (with errors allowed, a planted alignment has neighbours that are hits too).
"""
import functools
import itertools
import random

import cases
from oracle import oracle as O

CFG = dict(cases.PRODUCT, Amin='!')                                    # maxerrors 2, minoverlap 25, minreadlength 25: K = 8
CFG_K6 = dict(CFG, maxerrors=3)                                        # K = 25 // 4 = 6
CFG_K5 = dict(CFG, maxerrors=1, minoverlap=10, minreadlength=10)       # K = 10 // 2 = 5
QUEUE = 256                                                            # KVQ_LIST_Q: candidates a wave's queue holds
SIZE_CAP = 2 << 20

S60 = (cases.QUIRK_SEQ + 'TCCAGTCAG').encode()                         # G at 0, A at 1: the odd-bytes cases rely on it
SHORT31 = b'CTGAACGTTAGCCATAGGTCAACGTTGACCA'
NONSEEDED = b'ACGTNNACGTTGCAACGTACGTAGCTAGCTAA'                        # an 'N': the exhaustive matcher's
BIG = bytes(random.Random(4000).choices(b'ACGT', k=4000))
assert len(S60) == 60 and len(SHORT31) == 31 and S60[0:2] == b'GA' and S60[21:22] == b'G' and S60[32:33] == b'G'


def seed_geometry(seqs, cfg):
    """K, stride and pitch of the seed index for a table (kvq_seed_k, kvq_seed_index_build), None where it has none"""
    e = cfg['maxerrors']
    K = min(min(cfg['minoverlap'], cfg['minreadlength']) // (e + 1), 8)
    if K < 5:
        return None
    pitch_of = lambda st: (K + st - 1) // st * st
    span_of = lambda st: pitch_of(st) * e + K + st - 1
    seeded = [i for i, s in enumerate(seqs) if span_of(2) <= len(s) <= 4095 and set(s) <= set(b'ACGT')]
    if not seeded:
        return None
    minlen = min(len(seqs[i]) for i in seeded)
    stride = 8 if minlen >= span_of(8) else 4 if minlen >= span_of(4) else 2
    return dict(K=K, e=e, stride=stride, pitch=pitch_of(stride), seeded=seeded)


def anchor_candidates(read, seqs, geo):
    """read positions 0 (mod stride) whose K-mer has the 2-bit codes of an anchor block: what the walk puts on the queue"""
    K, code = geo['K'], lambda b: bytes((c >> 1) & 3 for c in b)
    anchors = {code(seqs[i][j * geo['pitch'] + sft:][:K]) for i in geo['seeded'] for j in range(geo['e'] + 1) for sft in range(geo['stride'])}
    return sum(code(read[p:p + K]) in anchors for p in range(0, len(read) - K + 1, geo['stride']))


class Text(object):
    def __init__(self, name, seqs, cfg=CFG, seed=1):
        self.name, self.seqs, self.cfg = name, list(seqs), dict(cfg)
        self.rng = random.Random(seed)
        self.parts, self.size, self.n, self.want = [], 0, 0, []
        self.geo = seed_geometry(self.seqs, self.cfg)

    def rand(self, n):
        return bytearray(self.rng.choices(b'ACGT', k=n))

    def next_fpos(self, pad=''):
        """file_pos of the first base of the read added next"""
        return self.size + len('@r%d%s\n' % (self.n, pad))

    def add(self, bases, quals=None, pad=''):
        head = ('@r%d%s\n' % (self.n, pad)).encode()
        fpos = self.size + len(head)
        rec = head + bytes(bases) + b'\n+\n' + (quals if quals is not None else b'I' * len(bases)) + b'\n'
        self.parts.append(rec); self.size += len(rec); self.n += 1
        return fpos

    def expect(self, label, seq_nr, fpos, seq_pos, length, rl, count=1):
        self.want.append((label, (seq_nr, fpos, seq_pos, length, rl), count))

    def mutate(self, buf, at):
        buf[at] = self.rng.choice([c for c in b'ACGT' if c != buf[at]])

    @property
    def text(self):
        return b''.join(self.parts)


def subsets_of_blocks(e):
    """every set of at most e of a job's e + 1 blocks"""
    return [b for k in range(e + 1) for b in itertools.combinations(range(e + 1), k)]


# ---- the pieces: each adds reads to a Text whose table starts with S60, BIG ------------------------------------------

def add_classes(T, rl=2000):
    mo, sl = T.cfg['minoverlap'], len(S60)
    # class C, the sequence inside the read: at the read's head, at its tail, at every residue of i mod 8
    for i in [0, rl - sl] + [1000 + r for r in range(8)]:
        b = T.rand(rl); b[i:i + sl] = S60
        T.expect('C in read i=%d' % i, 0, T.add(b), -i, sl, rl)
    for ov in (mo, mo + 1, sl - 1):
        # class A: the read's tail over the sequence's head; class B: the read's head over the sequence's tail
        b = T.rand(rl); b[rl - ov:] = S60[:ov]
        T.expect('A overlap %d' % ov, 0, T.add(b), -(rl - ov), ov, rl)
        b = T.rand(rl); b[:ov] = S60[sl - ov:]
        T.expect('B overlap %d' % ov, 0, T.add(b), sl - ov, ov, rl)
    # class C, the read inside the 4000-base sequence: in its middle, at its head, and at its tail (there class B holds the same alignment:
    # the reference's duplicate hit)
    for n, d in ((1024, 1500), (3000, 0), (2047, 313)):
        T.expect('read in sequence d=%d' % d, 1, T.add(BIG[d:d + n]), d, n, n)
    for n in (1024, 3000):
        T.expect('B/C duplicate n=%d' % n, 1, T.add(BIG[4000 - n:]), 4000 - n, n, n, count=2)


def add_subsets(T, rl=3000):
    geo, sl = T.geo, len(S60)
    K, e, pitch, stride = geo['K'], geo['e'], geo['pitch'], geo['stride']
    for broken in subsets_of_blocks(e):
        # family S: the sequence inside the read at i = 1003; its blocks are those of the copy (-i) mod stride
        i = 1003; sft = -i % stride
        b = T.rand(rl); b[i:i + sl] = S60
        for t in broken:
            T.mutate(b, i + t * pitch + sft + 3)
        T.expect('S broken %s' % (broken,), 0, T.add(b), -i, sl, rl)
        # family H, class B: the read's head over the sequence's last 40 bases; blocks at read positions K t
        b = T.rand(rl); b[:40] = S60[20:]
        for t in broken:
            T.mutate(b, K * t + 3)
        T.expect('H/B broken %s' % (broken,), 0, T.add(b), 20, 40, rl)
        # family H, class C: the read inside the long sequence
        b = bytearray(BIG[700:2200])
        for t in broken:
            T.mutate(b, K * t + 3)
        T.expect('H/C broken %s' % (broken,), 1, T.add(b), 700, 1500, 1500)
        # family T, class A: the read's tail over the sequence's first 40 bases; blocks at rl - K (t + 1)
        b = T.rand(rl); b[rl - 40:] = S60[:40]
        for t in broken:
            T.mutate(b, rl - K * (t + 1) + 3)
        T.expect('T broken %s' % (broken,), 0, T.add(b), -(rl - 40), 40, rl)


def add_seams(T):
    sl = len(S60)
    # the walk loads 1 KiB at a time from the 16-byte boundary in front of the read: a planted sequence ends in front of
    # every seam, lies across it (its blocks too), starts on it and behind it
    for k, delta in enumerate((-sl, -33, -8, -4, 0, 3)):
        pad = 'x' * k                                     # (another offset of the read inside its 16 bytes)
        sh = T.next_fpos(pad) & 15
        b = T.rand(5200); at = []
        for c in range(1, 5):
            i = 1024 * c - sh + delta
            b[i:i + sl] = S60; at.append(i)
        fpos = T.add(b, pad=pad)
        assert fpos & 15 == sh
        for i in at:
            T.expect('walk seam %d%+d' % ((i + sh - delta) // 1024, delta), 0, fpos, -i, sl, 5200)
    # ... and starts at every offset inside a lane's 16 bytes
    sh = T.next_fpos() & 15
    b = T.rand(2400); at = []
    for k in range(16):
        i = 16 * (13 + 7 * k) - sh + k
        b[i:i + sl] = S60; at.append(i)
    fpos = T.add(b)
    for k, i in enumerate(at):
        assert (fpos + i) & 15 == k
        T.expect('lane seam +%d' % k, 0, fpos, -i, sl, 2400)


def add_odd_bytes(T, rl=2000):
    sl = len(S60)
    # 'N' has the 2-bit code of 'G', a lower-case base that of its capital: inside a seed block the lookup still answers,
    # the bytes differ; elsewhere in the overlap they are plain mismatches
    for label, at, byte in (('N in block', 0, b'N'), ('lower case in block', 1, b'a'), ('N in overlap', 40, b'N'), ('lower case in overlap', 41, S60[41:42].lower())):
        b = T.rand(rl); b[1000:1000 + sl] = S60; b[1000 + at:1001 + at] = byte
        T.expect('S ' + label, 0, T.add(b), -1000, sl, rl)
    b = T.rand(rl); b[:40] = S60[20:]; b[1:2] = b'N'
    T.expect('H N in block', 0, T.add(b), 20, 40, rl)
    b = T.rand(rl); b[:40] = S60[20:]; b[30:31] = b[30:31].lower()
    T.expect('H lower case in overlap', 0, T.add(b), 20, 40, rl)
    b = T.rand(rl); b[rl - 40:] = S60[:40]; b[rl - 8:rl - 7] = b'N'
    T.expect('T N in block', 0, T.add(b), -(rl - 40), 40, rl)
    b = T.rand(rl); b[rl - 40:] = S60[:40]; b[rl - 39:rl - 38] = b'a'
    T.expect('T lower case in overlap', 0, T.add(b), -(rl - 40), 40, rl)


def add_huge(T):
    sl = len(S60)
    for rl, plants, tail in ((70000, (66000, 70000 - sl), 0), (200000, (70000, 150003, 199000), 30)):
        b = T.rand(rl)
        for i in plants:
            b[i:i + sl] = S60
        if tail:
            b[rl - tail:] = S60[:tail]
        fpos = T.add(b)
        for i in plants:
            T.expect('read of %d, i=%d' % (rl, i), 0, fpos, -i, sl, rl)
        if tail:
            T.expect('read of %d, class A' % rl, 0, fpos, -(rl - tail), tail, rl)


def add_mixed(T):
    sl = len(S60)
    for k in range(12):
        b = T.rand(150)
        if k % 3 == 0:
            b[40 + k:40 + k + sl] = S60
            T.expect('150 bases, i=%d' % (40 + k), 0, T.add(b), -(40 + k), sl, 150)
        elif k % 3 == 1:
            b[:30] = S60[30:]
            T.expect('150 bases, class B', 0, T.add(b), 30, 30, 150)
        else:
            T.add(b)
    for n in (1, 10, 24):                              # below minreadlength (where it is 25)
        T.add(S60[:n])
    # the trim cuts the read out of its line: the longest run of good scores starts at 700
    b = T.rand(3000); b[1500:1500 + sl] = S60
    q = b'I' * 600 + b'!' + b'I' * 99 + b'!' + b'I' * 2200 + b'!' + b'I' * 98
    if T.cfg['Amin'] > '!':
        fpos = T.add(b, q)
        T.expect('trimmed read', 0, fpos + 701, -(1500 - 701), sl, 2200)


# ---- the texts ---------------------------------------------------------------------------------------------------------

def _classes(name, cfg, seqs=(S60, BIG), seed=2):
    T = Text(name, seqs, cfg, seed)
    add_classes(T); add_subsets(T); add_mixed(T)
    return T


def _strides(n):
    """the shortest seeded sequence has n bases: stride 2 (25), 4 (27 .. 30) or 8 (31 and more)"""
    short = SHORT31[:n]
    T = Text('stride_%d' % n, [short, S60], CFG, seed=n)
    assert T.geo['stride'] == (2 if n < 27 else 4 if n < 31 else 8)
    rl = 2000
    for i in [0, rl - n] + [1000 + r for r in range(8)]:
        b = T.rand(rl); b[i:i + n] = short; b[300:360] = S60
        fpos = T.add(b)
        T.expect('short sequence i=%d' % i, 0, fpos, -i, n, rl)
        T.expect('S60 beside it', 1, fpos, -300, 60, rl)
    for broken in subsets_of_blocks(2):
        i = 1003; sft = -i % T.geo['stride']
        b = T.rand(rl); b[i:i + n] = short
        for t in broken:
            T.mutate(b, i + t * T.geo['pitch'] + sft + 3)
        T.expect('short sequence broken %s' % (broken,), 0, T.add(b), -i, n, rl)
    return T


def _flood():
    seqs = [b'ACGT' * 10, b'GTAC' * 12, S60]
    T = Text('flood', seqs, CFG, seed=5)
    b = T.rand(1500); b[700:760] = S60
    T.expect('in front of the flood', 2, T.add(b), -700, 60, 1500)
    T.flood_read = b'ACGT' * 5000
    fpos = T.add(T.flood_read)
    for i in (0, 4, 10000, 20000 - 40):
        T.expect('repeat i=%d' % i, 0, fpos, -i, 40, 20000)
    T.expect('repeat, other phase', 1, fpos, -2, 48, 20000)
    b = T.rand(1500); b[100:160] = S60
    T.expect('behind the flood', 2, T.add(b), -100, 60, 1500)
    return T


def _main():
    T = Text('main', [S60, BIG], dict(CFG, Amin='5'), seed=7)
    add_classes(T); add_seams(T); add_odd_bytes(T); add_mixed(T); add_huge(T)
    return T


def _with_n():
    T = Text('with_n', [S60, NONSEEDED, BIG], CFG, seed=8)
    # (the table's second sequence has no seeds: the pieces speak of sequence 1 = BIG, so they are built on a table in their order and renumbered)
    U = Text('u', [S60, BIG], CFG, seed=8)
    add_classes(U); add_odd_bytes(U)
    T.parts, T.size, T.n = U.parts, U.size, U.n
    T.want = [(label, ((0, 2)[h[0]],) + h[1:], count) for label, h, count in U.want]
    b = T.rand(2000); b[500:500 + len(NONSEEDED)] = NONSEEDED
    T.expect('the sequence without seeds', 1, T.add(b), -500, len(NONSEEDED), 2000)
    return T


def _short150():
    """2000 reads of 150 bases, the main text's table and config: what the scan kernel's tiles are made for"""
    T = Text('short150', [S60, BIG], dict(CFG, Amin='5'), seed=9)
    for k in range(2000):
        b = T.rand(150)
        if k % 10 == 0:
            i = k // 10 % 90
            b[i:i + 60] = S60
            T.expect('read %d' % k, 0, T.add(b), -i, 60, 150)
        else:
            T.add(b)
    return T


def _one(name, adder, cfg=CFG, seed=3):
    T = Text(name, [S60, BIG], cfg, seed)
    adder(T)
    return T


BUILDERS = {
    'classes': lambda: _classes('classes', CFG),
    'seams': lambda: _one('seams', add_seams),
    'odd_bytes': lambda: _one('odd_bytes', add_odd_bytes),
    'huge': lambda: _one('huge', add_huge),
    'flood': _flood,
    'stride_25': lambda: _strides(25), 'stride_27': lambda: _strides(27), 'stride_30': lambda: _strides(30), 'stride_31': lambda: _strides(31),
    'k6': lambda: _classes('k6', CFG_K6, seed=4),
    'k5': lambda: _classes('k5', CFG_K5, seed=6),
    'with_n': _with_n,
    'main': _main,
    'short150': _short150,
}
NAMES = sorted(BUILDERS)


@functools.lru_cache(maxsize=None)
def text(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's scan of a text, with the fold of its hits (computed once, shared, left unchanged)"""
    T = text(name)
    return O.scan_memory(T.text, T.seqs, fold=True, **dict(T.cfg, nthreads=2))


def check_wanted(T, hits):
    """every hit the builder planted is among `hits` exactly as often as it says"""
    count = {}
    for h in hits:
        count[tuple(h)] = count.get(tuple(h), 0) + 1
    bad = [(label, h, n, count.get(h, 0)) for label, h, n in T.want if count.get(h, 0) != n]
    assert not bad, bad[:5]
