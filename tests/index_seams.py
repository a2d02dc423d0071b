"""
The seams of the record index, in plain Python and without a GPU: where are the four newlines of each
record?  Two pieces of device code answer it -- the exact index (kvq_count_lines, kvq_scan_segments, kvq_index_records) and
kvq_collect_skipped, which finds the records of the tiles the fused scan left alone -- and this module holds what both owe:

  ``index_of``      the statement of the exact index: ``profile_ref.records_of`` (nl4), the records per chunk and rec_start;
  ``skipped_of``    the statement of what one skipped-tile descriptor must leave on the redo list, written from the index;
  the cases         texts and cuts that put newlines, cuts and records on the seams of the kernels' geometry (16-byte block,
                    dword, lane, 1 KiB round, 4 KiB segment, 64-segment round, 260-segment grid, 32 768-chunk launch), each
                    with the seams it names; ``seams_of`` finds the seams a text reaches from the text alone;
  ``WRONG``         name -> the statement with ONE plausible kernel slip: the matrix is worth what it tells apart.

tests/test_index_seams_host.py asserts all of it on the CPU; tests/test_gpu_index_seams.py holds the kernels against the
statements.  ``python tests/index_seams.py`` prints the census (profiles/index_seam_tests.txt).
"""
import collections
import functools
import os
import random
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                          # (run as a script: the census)
    sys.path.insert(0, ROOT)

from profile_ref import records_of                # noqa: E402

DWORD, LANE, ROUND, SEG = 4, 16, 1024, 4096       # bytes: a dword, a lane's share of a round, a round of a wave, a segment (KVQ_SEG_BYTES)
SEG_ROUND = 64                                    # segments per round of kvq_scan_segments
GRID_SEGS = 260                                   # segments one pass of the index kernels' grid covers (65 blocks of 4 waves)
LAUNCH_CHUNKS = 32768                             # chunks per launch of the index kernels
UNITS = (('dword', DWORD), ('lane', LANE), ('round', ROUND), ('segment', SEG))
NEAR_MISSES = bytes([0x8A, 0x0B, 0x09, 0x1A, 0x00, 0xFF, 0x0D, 0x0A])
NL = 10

Case = collections.namedtuple('Case', 'name text co seams')
Index = collections.namedtuple('Index', 'per nl4 rec_start')


def case(name, buf, co, seams):
    return Case(name, np.frombuffer(bytes(buf), dtype=np.uint8), [int(c) for c in co], tuple(seams))


# ---- the statement of the exact index -------------------------------------------------------------------------------

def index_of(text, co):
    """per[c] the complete records of chunk c; nl4[g] the four newlines of record g (records_of); rec_start[g] its first
    byte: the chunk's begin for a chunk's first record, else one behind the newline that ends the record in front"""
    recs = records_of(bytes(text), co)
    nl4 = np.array(recs, dtype=np.int64).reshape(-1, 4)
    cuts = np.asarray(co, dtype=np.int64)
    # (a record lies in the chunk that holds its first newline: the last of equal cuts begins the chunk that is not empty)
    chunk = np.searchsorted(cuts, nl4[:, 0], side='right') - 1
    per = np.bincount(chunk, minlength=len(co) - 1)[:len(co) - 1]
    rec_start = np.empty(len(recs), dtype=np.int64)
    if len(recs):
        first = np.ones(len(recs), dtype=bool)
        first[1:] = chunk[1:] != chunk[:-1]
        rec_start[1:] = nl4[:-1, 3] + 1
        rec_start[first] = cuts[chunk[first]]
    return Index(per.astype(np.int64), nl4, rec_start)


def index_numpy(text, co):
    """a second, independent statement of nl4 and per: the positions of the byte 10, restricted to [a, b), four at a time"""
    text = np.asarray(text)
    out, per = [], []
    for a, b in zip(co, co[1:]):
        p = a + np.flatnonzero(text[a:b] == NL)
        per.append(len(p) // 4)
        out.append(p[:len(p) // 4 * 4])
    nl4 = np.concatenate(out).reshape(-1, 4) if out else np.zeros((0, 4), dtype=np.int64)
    return np.array(per, dtype=np.int64), nl4.astype(np.int64)


# ---- the statement in the shape of the kernels, with room for one slip -----------------------------------------------

def index_shaped(text, co, slip=None):
    """The index as the three kernels put it together -- newlines numbered within their chunk, an entry written where its
    number says, what no newline writes left at zero -- with one slip, or none (then it equals ``index_of``: asserted)."""
    text = np.asarray(text)
    cuts = np.asarray(co, dtype=np.int64)
    a, b = cuts[:-1].copy(), cuts[1:].copy()
    nch = len(a)
    isnl = (text & 0x7F) == NL if slip == 'low seven bits' else text == NL
    P = np.flatnonzero(isnl).astype(np.int64)
    lo_at, hi_at = a.copy(), b.copy()
    if slip == 'b inclusive':
        hi_at = np.where(b > a, b + 1, b)
    if slip == 'a exclusive':
        lo_at = np.where(b > a, a + 1, a)
    if slip == 'block in front of a counted':
        lo_at = np.where(b > a, a & ~15, a)
    lo, hi = np.searchsorted(P, lo_at), np.searchsorted(P, np.maximum(hi_at, lo_at))
    n = hi - lo
    ch = np.repeat(np.arange(nch), n)
    rank = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    pos = P[np.repeat(lo, n) + rank]
    A = (a & ~15)[ch]
    seg = (pos - A) // SEG
    num, total = rank, n
    if slip == 'carry between rounds dropped':
        # every round of a segment numbers its newlines from the segment's base
        rnd = (pos - A) // ROUND
        num = _first_of(ch * (1 << 24) + seg, rank) + rank - _first_of(ch * (1 << 24) + rnd, rank)
    if slip == 'segments beyond the 64th lost':
        # kvq_scan_segments starts every round of 64 segments at zero: the bases of the later segments, and the chunk's count
        grp = ch * (1 << 24) + seg // SEG_ROUND
        num = rank - _first_of(grp, rank)
        nseg = np.where(b > a, (b - (a & ~15) + SEG - 1) // SEG, 0)
        last = np.zeros(nch, dtype=np.int64)
        in_last = seg // SEG_ROUND == ((nseg - 1) // SEG_ROUND)[ch]
        np.add.at(last, ch[in_last], 1)
        total = last
    per = (total + 3) // 4 if slip == 'tail kept' else total // 4
    limit = 4 * per
    g0 = np.cumsum(per) - per
    if slip == 'chunk base restarts at chunk 32768' and nch > LAUNCH_CHUNKS:
        g0[LAUNCH_CHUNKS:] -= g0[LAUNCH_CHUNKS]
    R = int(per.sum())
    nl4, rec_start = np.zeros(4 * R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    has = per > 0
    rec_start[g0[has]] = (a & ~15)[has] if slip == 'first rec_start aligned down' else a[has]
    w = num < limit[ch]
    nl4[(4 * g0[ch] + num)[w]] = pos[w]
    w &= ((num & 3) == 3) & (num + 1 < limit[ch])
    rec_start[(g0[ch] + (num + 1) // 4)[w]] = pos[w] + 1
    return Index(per, nl4.reshape(-1, 4), rec_start)


def _first_of(key, value):
    """value of the first element of every run of equal keys (keys ascending), at every element"""
    if not len(key):
        return value
    start = np.ones(len(key), dtype=bool)
    start[1:] = key[1:] != key[:-1]
    return value[np.flatnonzero(start)][np.cumsum(start) - 1]


INDEX_SLIPS = ('b inclusive', 'a exclusive', 'block in front of a counted', 'tail kept', 'low seven bits', 'first rec_start aligned down',
               'carry between rounds dropped', 'segments beyond the 64th lost', 'chunk base restarts at chunk 32768')


def same_index(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


# ---- the statement of what a skipped tile must leave ------------------------------------------------------------------

Tile = collections.namedtuple('Tile', 'a b own_begin own_end seen first')


def skipped_of(text, tile, slip=None):
    """{(rec_start, n0, n1, n2, n3)}: the complete records of the chunk [a, b) that start one behind a newline of
    [own_begin, own_end), and the chunk's first record when ``first`` is set.  A partial tile's descriptor names the chunk
    re-based at the first record it left (a == own_begin == z - 1, seen == 0, first == 1): the same rule.  From the index,
    not from the kernel's walk; ``seen`` is what the rule implies, and is held against it (``seen_of``)."""
    t = Tile(*[int(x) for x in tile])
    a, own_end = t.a, t.own_end
    if slip == 'own_end inclusive':
        own_end += 1
    rebased = slip == 'seen ignored' and not t.first
    if rebased:
        a = t.own_begin                 # (the walk numbers the newlines from the tile's own first byte)
    ix = _chunk_index(text, a, t.b)
    out = set()
    for g in range(len(ix.rec_start)):
        rs = int(ix.rec_start[g])
        if t.own_begin <= rs - 1 < own_end if g else bool(t.first) and not rebased:
            out.add((rs,) + tuple(int(x) for x in ix.nl4[g]))
    return out


_chunk_indexes = {}


def _chunk_index(text, a, b):
    """index_of(text, [a, b]), kept: the tiles of a chunk share it"""
    text = np.asarray(text)
    key = (len(text), zlib.crc32(text), a, b)
    if key not in _chunk_indexes:
        if len(_chunk_indexes) > 64:
            _chunk_indexes.clear()
        _chunk_indexes[key] = index_of(text, [a, b])
    return _chunk_indexes[key]


def seen_of(text, tile):
    """newlines of [a, own_begin): what kvq_validate_tiles must have counted in front of the tile"""
    t = Tile(*[int(x) for x in tile])
    return int((np.asarray(text)[t.a:t.own_begin] == NL).sum())


def tiles_of(co, tile_bytes):
    """every tile of every chunk as a descriptor of a tile skipped whole (the geometry of kvq_seeded_launch); seen is filled
    in by the caller"""
    out = []
    for a, b in zip(co, co[1:]):
        if b <= a:
            continue
        g0, tn = a & ~15, 0
        while g0 < b:
            out.append(Tile(a, b, a if tn == 0 else g0, min(g0 + tile_bytes, b), 0, 1 if tn == 0 else 0))
            g0 += tile_bytes; tn += 1
    return out


def without_z(text, co, tile_bytes, tile):
    """the slip 'z ignored': the descriptor kvq_validate_tiles would write for a partial tile had it not looked at z -- the
    tile's own geometry: the records it has scanned itself are collected again"""
    t = Tile(*[int(x) for x in tile])
    for a, b in zip(co, co[1:]):
        if a <= t.a < b:
            tn = (t.a - (a & ~15)) // tile_bytes
            g0 = (a & ~15) + tn * tile_bytes
            full = Tile(a, b, a if tn == 0 else g0, min(g0 + tile_bytes, b), 0, 1 if tn == 0 else 0)
            return full._replace(seen=seen_of(text, full))
    raise ValueError('no chunk holds the tile')


def is_partial(text, co, tile):
    """a descriptor that begins at a record inside its chunk (z was set)"""
    t = Tile(*[int(x) for x in tile])
    return t.first == 1 and t.a not in set(co)


SKIP_SLIPS = ('own_end inclusive', 'seen ignored', 'z ignored')
# what the descriptors of the dense_region sweep must show between them
DENSE_REGION_SEAMS = ('seen & 3 == 0', 'seen & 3 == 1', 'seen & 3 == 2', 'seen & 3 == 3', 'an owned newline at own_end - 1 ends a record',
                      'a newline at own_end', 'a record over two 4 KiB rounds of the walk')


def skip_seams(text, tile):
    """the seams of kvq_collect_skipped one descriptor reaches"""
    t = Tile(*[int(x) for x in tile])
    text = np.asarray(text)
    out = set()
    if not t.first:
        out.add('seen & 3 == %d' % (t.seen & 3))
    ix = _chunk_index(text, t.a, t.b)
    ends = set(int(x) for x in ix.nl4[:, 3])
    if t.own_end - 1 in ends and t.own_end - 1 >= t.own_begin:
        out.add('an owned newline at own_end - 1 ends a record')
    if t.own_end < t.b and text[t.own_end] == NL:
        out.add('a newline at own_end')
    if t.own_end in ends:
        out.add('the newline at own_end ends a record')
    p0 = t.own_begin & ~15
    for rs, n4 in zip(ix.rec_start, ix.nl4):
        if t.own_begin <= rs - 1 < t.own_end or (t.first and rs == t.a):
            if (n4[0] - p0) // SEG != (n4[3] - p0) // SEG:
                out.add('a record over two 4 KiB rounds of the walk')
            if n4[3] == t.b - 1:
                out.add('a record runs to b')
            if n4[3] >= t.own_end:
                out.add('a record ends behind own_end')
    if t.b % 16:
        out.add('b not a multiple of 16')
    if -(-(t.b - p0) // 16) * 16 % SEG:            # (the last round of the walk has vectors at or behind b)
        out.add('the clamped load at last_v')
    return out


# ---- the seams a text reaches, found from the text -------------------------------------------------------------------

def seams_of(text, co):
    """names of the seams of the exact index that (text, co) reaches"""
    text = np.asarray(text)
    nb = len(text)
    ix = index_of(text, co)
    out = set()
    pairs = set((a % 16, b % 16) for a, b in zip(co, co[1:]) if b > a)
    if len(pairs) == 256:
        out.add('every (a mod 16, b mod 16)')
    full = [(a, b) for a, b in zip(co, co[1:]) if b > a]
    for name, at in (('a - 1', lambda a, b: a - 1), ('a', lambda a, b: a), ('b - 1', lambda a, b: b - 1), ('b', lambda a, b: b)):
        if full and all(0 <= at(a, b) < nb and text[at(a, b)] == NL for a, b in full):
            out.add('a newline at %s of every chunk' % name)
    if co[0] > 0:
        out.add('chunk_off[0] > 0')
    if co[-1] < nb:
        out.add('the last cut in front of nbytes')
    if (text[:co[0]] == NL).any() and (text[co[-1]:] == NL).any():
        out.add('newlines outside the chunks')
    empty = [b == a for a, b in zip(co, co[1:])]
    if empty and empty[0]:
        out.add('an empty chunk first')
    if empty and empty[-1]:
        out.add('an empty chunk last')
    if any(e and not all(empty[:i]) and not all(empty[i:]) for i, e in enumerate(empty)):
        out.add('an empty chunk in the middle')
    if any(empty[i] and empty[i + 1] and empty[i + 2] for i in range(len(empty) - 2)):
        out.add('three empty chunks in a row')
    at, starts = 0, []
    for c, (a, b) in enumerate(zip(co, co[1:])):
        if b <= a:
            continue
        A = a & ~15
        nl = a + np.flatnonzero(text[a:b] == NL)
        k, per = len(nl), int(ix.per[c])
        if k <= 8:
            out.add('a chunk of %d newlines' % k)
        if k and k == (b - a):
            out.add('a chunk of nothing but newlines')
            out.add('a dense chunk at a mod 16 == %d' % (a % 16))
            for d in (-1, 0, 1):
                if (b - a - d) % SEG == 0 and b - a > 1:
                    out.add('a dense chunk of 4096 k %+d bytes' % d if d else 'a dense chunk of 4096 k bytes')
            if b - a == 3 * SEG + 5:
                out.add('a dense chunk of 3 * 4096 + 5 bytes')
        nseg = (b - A + SEG - 1) // SEG
        if nseg in (64, 65, 128, 129, 260, 261, 300):
            out.add('a chunk of %d segments' % nseg)
        if nseg > SEG_ROUND and ((nl - A) // SEG >= SEG_ROUND).any():
            out.add('newlines behind the 64th segment')
        if nseg > GRID_SEGS and ((nl - A) // SEG >= GRID_SEGS).any():
            out.add('newlines behind the 260th segment')
        if k and nseg > 1:
            cnt = np.bincount((nl - A) // SEG, minlength=nseg)
            if (cnt == 0).any() and len(set(cnt.tolist())) > 3:
                out.add('segments of different counts, some of none')
        # the kinds of newline on the last byte of a unit and on the first byte behind it, counted from a & ~15
        for j, p in enumerate(nl[:4 * per].tolist()):
            for uname, u in UNITS:
                if (p - A) % u == u - 1:
                    out.add('newline %d of a record on the last byte of a %s, a mod 16 == %d' % (j % 4 + 1, uname, a % 16))
                if (p - A) % u == 0 and p > A:
                    out.add('newline %d of a record on the first byte behind a %s, a mod 16 == %d' % (j % 4 + 1, uname, a % 16))
        for g in range(at + 1, at + per):
            rs = int(ix.rec_start[g])
            for uname, u in UNITS:
                if (rs - A) % u == 0:
                    out.add('rec_start across a %s' % uname)
        # the dropped tail
        tail = nl[4 * per:]
        if len(tail) and per:
            out.add('a tail of %d dropped' % len(tail))
            n3 = int(nl[4 * per - 1])
            t0, t1 = int(tail[0]), int(tail[-1])
            where = ('in the lane of the last record\'s 4th newline' if (t1 - A) // LANE == (n3 - A) // LANE else
                     'in a later lane of the same round' if (t1 - A) // ROUND == (n3 - A) // ROUND and (t0 - A) // LANE > (n3 - A) // LANE else
                     'in a later round' if (t1 - A) // SEG == (n3 - A) // SEG and (t0 - A) // ROUND > (n3 - A) // ROUND else
                     'in a later segment that holds only tail' if (t0 - A) // SEG > (n3 - A) // SEG else None)
            if where:
                out.add('the tail ' + where)
                if (b - 1 - A) // SEG > (t1 - A) // SEG:
                    out.add('the tail followed by segments without a newline')
        if per and len(nl) >= 8 and (np.diff(nl) > 10000).any() and (np.diff(nl)[np.flatnonzero(np.diff(nl) > 10000)[0] + 1:][:3] == 1).all():
            out.add('a 10 000-byte line, four newlines in a row behind it')
        at += per
    if len(co) - 1 > LAUNCH_CHUNKS and ix.per[LAUNCH_CHUNKS:].sum() and ix.per[:LAUNCH_CHUNKS].sum():
        out.add('records behind chunk 32768')
    if len(co) - 1 == LAUNCH_CHUNKS:
        out.add('exactly 32768 chunks')
    if len(co) - 1 == LAUNCH_CHUNKS - 1:
        out.add('32767 chunks')
    if not len(ix.rec_start):
        out.add('no record')
    if not (text == NL).any():
        out.add('no newline')
    # byte values beside a newline, in every byte position of a dword
    if nb >= 8:
        w = text[:nb // 4 * 4].reshape(-1, 4)
        seen = set()
        for j in range(4):
            rows = w[w[:, j] == NL]
            for i in range(4):
                if i != j:
                    seen.update((j, int(v)) for v in np.unique(rows[:, i]))
        if len(seen) == 4 * 256:
            out.add('all 256 byte values beside a newline, in each byte of a dword')
    if bytes(text).find(NEAR_MISSES * 4) >= 0:
        out.add('runs of the near misses')
    return out


# ---- the index cases -------------------------------------------------------------------------------------------------

class Builder(object):
    """a text put together chunk by chunk (the cuts are consecutive: what lies between two chunks of interest is a chunk too,
    of filler without a newline)"""

    def __init__(self, front=b''):
        self.buf, self.co = bytearray(front), [len(front)]

    def chunk(self, data):
        self.buf += data; self.co.append(len(self.buf))
        return self

    def align(self, r, filler=b'x'):
        """a filler chunk, so that the next chunk begins at r mod 16 (none when it does already)"""
        k = (r - len(self.buf)) % 16
        return self.chunk(filler * k) if k else self

    def done(self, name, seams, behind=b''):
        return case(name, self.buf + behind, self.co, seams)


def _de_bruijn16():
    """a cyclic sequence of 256 residues in which every ordered pair of residues is adjacent once"""
    k, n = 16, 2
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    return seq


CUT_VARIANTS = (None, 'a - 1', 'a', 'b - 1', 'b')


@functools.lru_cache(maxsize=None)
def cuts_mod16(variant=None):
    rng = random.Random(16)
    seq = _de_bruijn16()
    i5 = seq.index(5)
    res = seq[i5:] + seq[:i5] + [5]                 # 257 residues, beginning at 5: the 256 pairs of neighbours
    co = [5]
    for r0, r1 in zip(res, res[1:]):
        co.append(co[-1] + ((r1 - r0) % 16 or 16) + 16 * rng.randrange(0, 6))
    nb = co[-1] + 7
    buf = bytearray(rng.choice(b'xy\n\nz\n') for _ in range(nb))
    buf[0:5] = b'\n\nq\n\n'; buf[nb - 6:nb] = b'\n\n\n\n\n\n'
    seams = ['every (a mod 16, b mod 16)', 'chunk_off[0] > 0', 'the last cut in front of nbytes', 'newlines outside the chunks']
    if variant:
        for a, b in zip(co, co[1:]):
            buf[{'a - 1': a - 1, 'a': a, 'b - 1': b - 1, 'b': b}[variant]] = NL
        seams.append('a newline at %s of every chunk' % variant)
    return case('cuts_mod16[%s]' % (variant or 'plain'), buf, co, seams)


def _lines(rng, k, tail=True):
    """bytes that hold exactly k newlines"""
    out = b''.join(bytes(rng.choice(b'abc') for _ in range(rng.randrange(0, 9))) + b'\n' for _ in range(k))
    return out + (bytes(rng.choice(b'abc') for _ in range(rng.randrange(0, 9))) if tail else b'')


@functools.lru_cache(maxsize=None)
def empty_and_tiny():
    rng = random.Random(7)
    B = Builder()
    for k in (None, 0, 1, 2, 3, None, 4, 5, 6, 7, None, None, None, 8, 4, 1, None):
        B.chunk(b'' if k is None else (_lines(rng, k) or b'q'))
    return B.done('empty_and_tiny', ['an empty chunk first', 'an empty chunk in the middle', 'an empty chunk last', 'three empty chunks in a row'] +
                  ['a chunk of %d newlines' % k for k in range(9)] + ['a tail of %d dropped' % k for k in (1, 2, 3)])


@functools.lru_cache(maxsize=None)
def dense():
    B = Builder()
    seams = ['a chunk of nothing but newlines', 'a dense chunk of 4096 k -1 bytes', 'a dense chunk of 4096 k bytes', 'a dense chunk of 4096 k +1 bytes',
             'a dense chunk of 3 * 4096 + 5 bytes', 'rec_start across a segment', 'rec_start across a round', 'rec_start across a lane']
    for r in (0, 7, 15):
        for n in (SEG - 1, SEG, SEG + 1, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + 5):
            B.align(r).chunk(b'\n' * n)
        seams.append('a dense chunk at a mod 16 == %d' % r)
    return B.done('dense', seams, b'xx')


@functools.lru_cache(maxsize=None)
def byte_values():
    buf = bytearray()
    for v in range(256):
        for j in range(4):
            w = bytearray([v] * 4); w[j] = NL
            buf += w
    buf += NEAR_MISSES * 64
    for j in range(4):                              # the near misses in every byte position of a dword
        buf += b'q' * (j + 1) + NEAR_MISSES * 8
    n = len(buf)
    return case('byte_values', buf, [0, 1027, 4096, n - 3, n], ['all 256 byte values beside a newline, in each byte of a dword', 'runs of the near misses'])


@functools.lru_cache(maxsize=None)
def segment_seams():
    B = Builder()
    seams = []
    for r in (0, 1, 15):
        for uname, u in UNITS:
            for side, off in (('on the last byte of', -1), ('on the first byte behind', 0)):
                for k in range(1, 5):
                    B.align(r)
                    a = len(B.buf); A = a & ~15
                    T = A + u * (-(-(a + 8 - A) // u)) + off        # the least such place at or behind a + 8 (+ off)
                    if T < a + 7:
                        T += u
                    ch = bytearray(b'x' * (T - a + 60))
                    nls = [T - 2 * (k - 1 - i) for i in range(k)] + [T + 2 * i for i in range(1, 5 - k)]
                    nls += [nls[-1] + 3 * i for i in range(1, 5)]    # the record behind it
                    for p in nls:
                        ch[p - a] = NL
                    B.chunk(ch[:nls[-1] - a + 1 + (r % 3)])
                    seams.append('newline %d of a record %s a %s, a mod 16 == %d' % (k, side, uname, r))
    seams += ['rec_start across a %s' % uname for uname, _ in UNITS]
    return B.done('segment_seams', seams, b'\n')


@functools.lru_cache(maxsize=None)
def limit():
    B = Builder()
    seams = []
    places = (('in the lane of the last record\'s 4th newline', 102, 0), ('in a later lane of the same round', 132, 0), ('in a later round', 100 + ROUND + 30, 0),
              ('in a later segment that holds only tail', SEG + 50, 0), ('in a later segment that holds only tail', SEG + 50, 2 * SEG))
    for where, at, trail in places:
        for t in (1, 2, 3):
            B.align(0)
            ch = bytearray(b'x' * (at + 2 * t + 3 + trail))
            for p in (10, 20, 30, 40, 70, 80, 90, 100):            # two records; the second one's 4th newline in lane 6
                ch[p] = NL
            for i in range(t):
                ch[at + 2 * i] = NL
            B.chunk(ch)
            seams += ['the tail ' + where, 'a tail of %d dropped' % t]
        if trail:
            seams.append('the tail followed by segments without a newline')
    return B.done('limit', sorted(set(seams)))


SEGMENT_COUNTS = (64, 65, 128, 129, 260, 261, 300)


@functools.lru_cache(maxsize=None)
def segments(nseg):
    """one chunk of nseg segments beside a one-segment chunk (the grid is sized by the largest)"""
    rng = np.random.RandomState(nseg)
    n = nseg * SEG - 17
    big = np.full(n, ord('x'), dtype=np.uint8)
    for s in range(nseg):
        k = 0 if s % 5 == 3 else (s * 7) % 11 + (s == nseg - 1)
        span = min(SEG, n - s * SEG)
        big[s * SEG + rng.choice(span, size=k, replace=False)] = NL
    small = np.full(900, ord('y'), dtype=np.uint8)
    small[rng.choice(900, size=23, replace=False)] = NL
    order = [small, big] if nseg % 2 else [big, small]
    buf = np.concatenate(order + [np.full(3, NL, dtype=np.uint8)])
    co = [0, len(order[0]) // 16 * 16 if nseg % 2 else len(order[0]), len(order[0]) + len(order[1])]
    seams = ['a chunk of %d segments' % nseg, 'segments of different counts, some of none']
    seams += ['newlines behind the 64th segment'] if nseg > 64 else []
    seams += ['newlines behind the 260th segment'] if nseg > 260 else []
    return Case('segments[%d]' % nseg, buf, co, tuple(seams))


CHUNK_COUNTS = (32767, 32768, 32769, 40000)


@functools.lru_cache(maxsize=None)
def chunks_32769(nchunks):
    rng = random.Random(nchunks)
    B = Builder(b'\n')
    for c in range(nchunks):
        k = rng.randrange(0, 16)
        if k == 0:
            B.chunk(b'')
            continue
        rec = bytearray(b'r' * rng.randrange(8, 25))
        for p in rng.sample(range(len(rec) - 1), 3):
            rec[p] = NL
        rec[-1] = NL
        B.chunk(bytes(rec) + (b't\nt' if k < 4 else b''))
    seams = ['chunk_off[0] > 0', 'an empty chunk in the middle']
    seams += ['records behind chunk 32768'] if nchunks > LAUNCH_CHUNKS else ['exactly 32768 chunks'] if nchunks == LAUNCH_CHUNKS else ['32767 chunks']
    return B.done('chunks_32769[%d]' % nchunks, seams, b'\n\n')


@functools.lru_cache(maxsize=None)
def long_lines():
    rng = random.Random(3)
    B = Builder(b'\nab')
    body = _lines(rng, 8, False) + b'L' * 10001 + b'\n\n\n\n' + _lines(rng, 9)
    B.chunk(body)
    B.chunk(_lines(rng, 5, False) + b'M' * 10000 + b'\n\n\n\n\n' + _lines(rng, 6))
    return B.done('long_lines', ['a 10 000-byte line, four newlines in a row behind it', 'chunk_off[0] > 0'])


@functools.lru_cache(maxsize=None)
def none(three=False):
    buf = bytearray(b'n' * 9000)
    if three:
        buf[1] = buf[4200] = buf[8999] = NL
    return case('none[%s]' % ('three' if three else 'zero'), buf, [0, 5000, 9000], ['no record'] + ([] if three else ['no newline']))


def random_case(seed):
    rng = random.Random(1000 + seed)
    nb = rng.randrange(1, 20 << 10)
    dens = rng.choice((2, 3, 8, 40, 150, 500))
    arr = np.random.RandomState(seed).randint(0, 256, size=nb).astype(np.uint8)
    arr[arr == NL] = 0x8A
    arr[np.random.RandomState(seed + 1).randint(0, dens, size=nb) == 0] = NL
    ncut = rng.randrange(2, 12)
    co = sorted(rng.randrange(0, nb + 1) for _ in range(ncut))
    for _ in range(rng.randrange(0, 3)):             # empty chunks
        co.append(rng.choice(co))
    if rng.random() < 0.3:
        co[0:0] = [0]
    if rng.random() < 0.3:
        co.append(nb)
    return Case('random[%d]' % seed, arr, sorted(co), ())


def random_cases(seed=0, n=200):
    return [random_case(seed * n + i) for i in range(n)]


def index_cases():
    out = [cuts_mod16(v) for v in CUT_VARIANTS]
    out += [empty_and_tiny(), dense(), byte_values(), segment_seams(), limit()]
    out += [segments(n) for n in SEGMENT_COUNTS]
    out += [chunks_32769(n) for n in CHUNK_COUNTS]
    out += [long_lines(), none(False), none(True)]
    return out


# ---- the skipped-tile cases: well-formed FastQ ---------------------------------------------------------------------------

# text: the trim_matrix.Text the case was made with; oracle_bytes: the text without a partial record at its end
SkipCase = collections.namedtuple('SkipCase', 'name data co cfg text oracle_bytes')
SHORT_RECORDS = (b'@\nA\n+\nI\n', b'@s\nAC\n+\nII\n', b'@sh\nACG\n+\nIII\n', b'@r1\nACGT\n+\nIIII\n', b'@\nACGTA\n+\nIIIII\n')      # 8, 10, 12, 14 and 14 bytes
SHORT_16 = b'@xy\nACGTA\n+\nIIIII\n'        # 16 bytes


def default_tile(data):
    """the tile the library gives a scan whose text begins like this (kvq_tile_for_text)"""
    import ctypes as C
    from kvarq_amd import _lib
    arr = np.frombuffer(bytes(data[:128 << 10]), dtype=np.uint8)
    rec = C.c_uint32()
    return int(_lib.lib().kvq_tile_for_text(arr.ctypes.data, arr.nbytes, C.byref(rec)))


def _reads(seed):
    import trim_matrix as TM
    import kernel_matrix as KM
    return TM.Text(dict(KM.CONFIGS[8]), 4, seed=seed)


FAMS = ('clean', 'closed', 'walk', 'descent', 'ties', 'bytes')


def _raw(t, data):
    t.parts.append(bytes(data)); t.nbytes += len(data)


def _stretch(t, nbytes, mix):
    """records of eight to sixteen bytes, `nbytes` of them; mix: which lengths take turns"""
    begin, i = t.nbytes, 0
    kinds = SHORT_RECORDS + (SHORT_16,)
    while t.nbytes - begin < nbytes:
        _raw(t, kinds[(i * (mix + 1) + i // 7) % len(kinds)]); i += 1


def _finish(name, t, co, oracle_bytes=None):
    t.finish()
    return SkipCase(name, t.data, [int(c) for c in co], t.cfg, t, t.nbytes if oracle_bytes is None else oracle_bytes)


TILE_GUESS = 39760                                 # (sizes the texts only: the tests read the geometry off the descriptors)


@functools.lru_cache(maxsize=None)
def dense_region(shift, mix=None):
    """150-base reads, a stretch of short records two and a half tiles long in their middle (it touches three or four tiles, and
    whichever of them it gives more newlines than a tile's table holds skips whole), reads again; shift: bytes
    the stretch is moved by (a longer first identifier line); mix: the turn the short records' lengths take"""
    mix = shift % 4 if mix is None else mix
    t = _reads(100 + shift)
    _raw(t, b'@' + b's' * shift + b'\nACGT\n+\nIIII\n')
    t.band(FAMS, 150, nbytes=TILE_GUESS + 9000)
    _stretch(t, 2 * TILE_GUESS + TILE_GUESS // 2, mix)
    t.band(FAMS, 150, nbytes=TILE_GUESS // 2)
    return _finish('dense_region[%d]' % shift, t, [0, t.nbytes])


@functools.lru_cache(maxsize=None)
def dense_to_the_end(bmod, cut):
    """a chunk of reads, then the chunk of interest, whose stretch runs to its end -- the text's end -- at b mod 16 == bmod and
    half a tile into the chunk's last tile; the last record complete, or cut (the oracle is asked about the text without
    that tail: ``oracle_bytes``)"""
    t = _reads(200 + bmod)
    t.band(FAMS, 150, nrec=40)
    a = t.nbytes
    t.band(FAMS, 150, nbytes=TILE_GUESS + 5000)
    _stretch(t, 2 * TILE_GUESS + TILE_GUESS // 2 - 5000, bmod % 5)
    whole = t.nbytes
    if cut:
        _raw(t, b'@cut\nAC' + b'G' * ((bmod - t.nbytes - 7) % 16))
    elif (bmod - t.nbytes) % 16:
        _raw(t, b'@' + b'p' * ((bmod - t.nbytes) % 16 + 8) + b'\nA\n+\nI\n')
        whole = t.nbytes
    assert t.nbytes % 16 == bmod
    return _finish('dense_to_the_end[%d,%s]' % (bmod, 'cut' if cut else 'whole'), t, [0, a, t.nbytes], whole)


@functools.lru_cache(maxsize=None)
def dense_first_tile(amod):
    """the stretch begins the (second) chunk, at a mod 16 == amod by way of a first chunk of chosen length"""
    t = _reads(300 + amod)
    t.band(FAMS, 150, nbytes=(128 << 10) + 8192)
    _raw(t, b'@' + b'p' * ((amod - t.nbytes - 8) % 16 + 16) + b'\nA\n+\nI\n')
    assert t.nbytes % 16 == amod
    a = t.nbytes
    _stretch(t, 2 * TILE_GUESS + 1000, amod % 5)
    t.band(FAMS, 150, nbytes=TILE_GUESS)
    return _finish('dense_first_tile[%d]' % amod, t, [0, a, t.nbytes])


LONG_VARIANTS = ('plain', 'last 16 owned bytes', 'to the end', 'two in a row')


@functools.lru_cache(maxsize=None)
def long_interior(variant):
    """5 kB and 9 kB records that start in an interior tile of their chunk"""
    import trim_matrix as TM
    t = _reads(400 + LONG_VARIANTS.index(variant))
    t.band(FAMS, 150, nbytes=(128 << 10) + 8192)
    tile = default_tile(b''.join(t.parts))
    rng = t.rng

    def long_(Q):
        t.long_read(TM.long_pattern(Q, 'big', rng), len(t.bands))

    def reads_up_to(at):
        """150-base reads, the last one padded so that the next record begins at `at`"""
        while at - t.nbytes > 2 * 360:
            t.band(FAMS, 150, nrec=1)
        gap = at - t.nbytes
        _raw(t, b'@' + b'p' * (gap - 8) + b'\nA\n+\nI\n')
        assert t.nbytes == at
    a = t.nbytes                                   # the chunk of interest begins here (a multiple of nothing in particular)
    A = a & ~15
    # (a tile leaves a record that begins in it and ends beyond its look-ahead, and keeps the records in front of it)
    if variant == 'plain':
        reads_up_to(A + 2 * tile - 2000); long_(2500); t.band(FAMS, 150, nrec=30); reads_up_to(A + 4 * tile - 3000); long_(4500)
        t.band(FAMS, 150, nrec=30)
    elif variant == 'last 16 owned bytes':
        reads_up_to(A + 2 * tile - 9); long_(2500); t.band(FAMS, 150, nrec=30)
    elif variant == 'to the end':
        reads_up_to(A + 2 * tile - 3000); long_(4500)
    else:
        reads_up_to(A + 2 * tile - 2000); long_(2500); long_(4500); t.band(FAMS, 150, nrec=30)
    return _finish('long_interior[%s]' % variant, t, [0, a, t.nbytes])


def skip_cases():
    out = [dense_region(s) for s in range(20)]
    out += [dense_to_the_end(m, False) for m in range(1, 16)] + [dense_to_the_end(m, True) for m in (1, 8, 15)]
    out += [dense_first_tile(m) for m in (0, 1, 15)]
    out += [long_interior(v) for v in LONG_VARIANTS]
    return out


def hypothetical_tiles(sc, tile_bytes):
    """every tile of the case as if it had been skipped whole, and -- for the records of 2 KiB and more -- the partial
    descriptor of the tile such a record starts in: what the sensitivity of the skipped statement is shown on without a GPU"""
    text = sc.data
    out = [t._replace(seen=seen_of(text, t)) for t in tiles_of(sc.co, tile_bytes)]
    ix = index_of(text, sc.co)
    for rs, n4 in zip(ix.rec_start, ix.nl4):
        if n4[3] - rs > 2048:
            for a, b in zip(sc.co, sc.co[1:]):
                if a < rs < b:
                    g0 = (a & ~15) + (rs - (a & ~15)) // tile_bytes * tile_bytes
                    out.append(Tile(int(rs), b, int(rs), min(g0 + tile_bytes, b), 0, 1))
    return out


def wrong_skipped(sc, tile_bytes, tile, slip):
    if slip == 'z ignored':
        if not is_partial(sc.data, sc.co, tile):
            return skipped_of(sc.data, tile)
        return skipped_of(sc.data, without_z(sc.data, sc.co, tile_bytes, tile))
    return skipped_of(sc.data, tile, slip)


WRONG = collections.OrderedDict((s, functools.partial(index_shaped, slip=s)) for s in INDEX_SLIPS)              # (text, co) -> Index
WRONG_SKIPPED = collections.OrderedDict((s, functools.partial(wrong_skipped, slip=s)) for s in SKIP_SLIPS)      # (case, tile bytes, descriptor) -> set


# ---- the text of the routes: every record reveals itself (tests/trim_matrix.py) -----------------------------------------

@functools.lru_cache(maxsize=None)
def routes_text():
    """-> (trim_matrix.Text, cuts): records of every family, cut at record starts so that a mod 16 takes all 16 values, with two
    empty chunks, records in front of the first cut and bytes behind the last"""
    import trim_matrix as TM
    import kernel_matrix as KM
    t = TM.Text(dict(KM.CONFIGS[8]), 4, seed=77)
    t.band(TM.FAMILIES, 150, nrec=3)
    co, want = [t.nbytes], [r for r in range(16) if r != t.nbytes % 16]
    while want:
        t.band(TM.FAMILIES, 150, nrec=25)
        for _ in range(64):
            if t.nbytes % 16 in want:
                break
            t.band(('tiny', 'clean'), 150, nrec=1)
        want.remove(t.nbytes % 16)
        co.append(t.nbytes)
        if len(want) in (9, 4):
            co.append(t.nbytes)                        # an empty chunk
    t.band(TM.FAMILIES, 150, nrec=25)                  # the chunk that begins at the last of the sixteen
    co.append(t.nbytes)
    t.band(TM.FAMILIES, 150, nrec=2)
    t.parts.append(b'@cut off\nACGT'); t.nbytes += 13
    t.finish()
    assert set(a % 16 for a, b in zip(co, co[1:]) if b > a) == set(range(16)) and sum(a == b for a, b in zip(co, co[1:])) == 2
    return t, co


# ---- the census --------------------------------------------------------------------------------------------------------

def census(out=print, randoms=200):
    cases = index_cases()
    out('The seam matrix of the record index (tests/index_seams.py; DESIGN.md section 4.2)')
    out('=' * 82)
    out('')
    out('1. The index cases and the seams they reach (each asserted in tests/test_index_seams_host.py)')
    out('')
    rights = {}
    for c in cases:
        ix = rights[c.name] = index_of(c.text, c.co)
        reached = seams_of(c.text, c.co)
        missing = [s for s in c.seams if s not in reached]
        out('%-22s %9d bytes %6d chunks %7d records   %d seams named%s' % (c.name, len(c.text), len(c.co) - 1, len(ix.rec_start), len(c.seams),
                                                                          '' if not missing else '   MISSING: %s' % missing))
        for s in _summary(c.seams):
            out('    ' + s)
    rnd = random_cases(0, randoms)
    out('%-22s %d texts, %d bytes, %d records; empty chunks in %d, chunk_off[0] > 0 in %d, bytes behind the last cut in %d'
        % ('random(0)', len(rnd), sum(len(c.text) for c in rnd), sum(len(index_of(c.text, c.co).rec_start) for c in rnd),
           sum(any(a == b for a, b in zip(c.co, c.co[1:])) for c in rnd), sum(c.co[0] > 0 for c in rnd), sum(c.co[-1] < len(c.text) for c in rnd)))
    out('')
    out('2. The wrong statements of the index, and the cases that tell each from the right one')
    out('')
    for slip in INDEX_SLIPS:
        tell = [c.name for c in cases if not same_index(index_shaped(c.text, c.co, slip), rights[c.name])]
        tell_r = sum(1 for c in rnd if not same_index(index_shaped(c.text, c.co, slip), index_of(c.text, c.co)))
        out('%-36s %2d cases and %3d of the %d random texts: %s' % (slip, len(tell), tell_r, len(rnd), ', '.join(tell) if tell else 'NONE'))
    out('')
    out('3. The skipped-tile cases: every tile taken as skipped whole, every record of 2 KiB and more as left by a partial tile')
    out('')
    tells = {s: [] for s in SKIP_SLIPS}
    reached_all = set()
    for sc in skip_cases():
        tile = default_tile(sc.data)
        tiles = hypothetical_tiles(sc, tile)
        reached = set()
        for t in tiles:
            reached |= skip_seams(sc.data, t)
        reached_all |= reached
        for s in SKIP_SLIPS:
            if any(wrong_skipped(sc, tile, t, s) != skipped_of(sc.data, t) for t in tiles):
                tells[s].append(sc.name)
        out('%-34s %8d bytes  tile %d  %3d tiles  seen & 3 in {%s}' % (sc.name, sc.data.nbytes, tile, len(tiles),
                                                                        ', '.join(sorted(s[-1] for s in reached if s.startswith('seen')))))
    out('')
    out('seams the hypothetical descriptors reach: ' + '; '.join(sorted(reached_all)))
    out('')
    for s in SKIP_SLIPS:
        out('%-36s %2d cases: %s' % (s, len(tells[s]), ', '.join(tells[s][:6]) + (' ...' if len(tells[s]) > 6 else '') if tells[s] else 'NONE'))


def _summary(seams):
    """the named seams, the families of the segment seams folded into a line each"""
    fam = collections.OrderedDict()
    for s in seams:
        if s.startswith('newline ') and ' of a record on the ' in s:
            key = 'newline 1..4 of a record on the last byte of / the first byte behind a dword, lane, round, segment; a mod 16 in {0, 1, 15}'
            fam[key] = fam.get(key, 0) + 1
        else:
            fam[s] = 0
    return ['%s (%d)' % (k, v) if v else k for k, v in fam.items()]


if __name__ == '__main__':
    census()
