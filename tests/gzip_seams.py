"""
The seam corpus of the gzip chunk decoder: gzip files written token by token
with deflate_writer, each built to take the device's kernels through one family of edges that a
stream from zlib cannot reach -- zlib never emits a distance above 32 768 - 262 = 32 506, a copy of
258 at the window's full reach, or stored blocks at will --, and a plain statement of the
bookkeeping the device does on them, which says for a run which edges it went through.

A chunk can only start at a dynamic block that is not the final one, and the finder puts it at the
first such header at or behind a nominal start (every chunk_bytes).  So a dynamic block behind a
stretch of at least chunk_bytes without such a header starts a chunk for certain: the streams put
one block of literals of MAX_CHUNK bytes and more in front of every block that has to start one
(an anchor), which holds at every chunk size of CHUNKS at once.  Positions counted in a chunk
(o, the ring's flush point f) are then known when the stream is written; seams() never relies on
that: it takes the chunk starts the run reports and counts what those chunks went through.

seams(stream, chunks, chunk_bytes) -> Counter over the classes of CLASSES, from
gzip_spec.last_chunks() of a run of stream.data at that chunk size.
"""
import bisect
import collections
import gzip
import random
import struct

import deflate_writer as W

WINDOW = 32768
CHUNKS = (64, 256, 1024)
MAX_CHUNK = max(CHUNKS)
STORED_LENS = (0, 1, 4095, 4096, 4097, 32768, 65535)
NSYMS = (0, 32767, 32768, 32769)
FIND_OFFSETS = (0, 255, 256, 257)
MARKER_OVERLAPS = (1, 63, 64, 65)
BIG = 1024 * 4096                            # symbols one pass of kvq_gz_replace's grid covers

CLASSES = (['copy_overwrites_source', 'copy_overwrites_source_dist_32768', 'copy_overwrites_source_multi_pass',
            'copy_crosses_wrap_write', 'copy_crosses_wrap_source', 'copy_straddles_chunk_start'] +
           ['overlap_of_markers_%d' % d for d in MARKER_OVERLAPS] +
           ['flush_at_equality', 'flush_one_past', 'flush_inside_stored'] +
           ['stored_len_%d' % n for n in STORED_LENS] +
           ['stored_crosses_wrap', 'ref_into_stored_across_wrap'] +
           ['chunk_nsym_%d' % n for n in NSYMS] +
           ['short_chunk_hops', 'member_at_chunk_end', 'member_inside_chunk', 'ref_to_member_first_byte', 'ref_before_member'] +
           ['find_offset_%d' % d for d in FIND_OFFSETS] +
           ['find_offset_last', 'find_offset_unaligned', 'find_offset_odd_range', 'two_candidates_in_one_round', 'big_chunk'])

ALPHABET = bytes(range(48, 112))             # 64 symbols: a literal of about 6 bits


def gz_member(raw):
    return b'\x1f\x8b\x08\x00\0\0\0\0\x00\xff' + raw + struct.pack('<II', 0, 0)


Stream = collections.namedtuple('Stream', 'name data text table chunk_sizes reaches fail_block')
# data: the file; text: what it inflates to (up to the failing block for a stream that fails); table: per block a dict (bit: its
# start in the file, out: its text offset, mout: the text offset of its member's start, first: the first block of a member,
# kind, final, tokens or data), None for a stream from zlib; reaches: chunk size -> the classes a run at that size must count;
# fail_block: the index in table of the block zlib refuses ("too far back"), None for a valid stream


# ---- writing a file block by block, the bit position at hand -----------------------------------------------------

class _File(object):
    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.members, self.cur = [], None
        self.nbytes = 0                      # of the members closed
        self.bit = 0                         # where the next block starts, in bits of the file
        self.member()

    def member(self):
        """close the member (its last block becomes the final one) and start the next"""
        if self.cur is not None:
            assert self.cur, 'an empty member'
            self.nbytes += len(gz_member(W.build(self.cur)[0]))
            self.members.append(self.cur)
        self.cur = []
        self.bit = 8 * (self.nbytes + 10)

    def add(self, block):
        """-> the bit the block starts at"""
        at = self.bit
        if block['kind'] == 'stored':
            self.bit = ((at + 3 + 7) & ~7) + 32 + 8 * len(block['data'])
        else:
            self.bit = at + _bits(block)
        self.cur.append(block)
        return at

    def lits(self, n):
        return [self.rnd.choice(ALPHABET) for _ in range(n)]

    def dyn(self, tokens, **kw):
        return self.add(dict(kind='dynamic', tokens=list(tokens), **kw))

    def anchor(self, tokens, **kw):
        """a dynamic block that starts a chunk at every size of CHUNKS: behind one block of literals longer than the largest"""
        at = self.dyn(self.lits(1450))
        assert self.bit - at >= 8 * (MAX_CHUNK + 8)
        return self.dyn(tokens, **kw)

    def preamble(self):
        """40 000 bytes and more of text nothing repeats in at 32 768: literals, then copies from all over them"""
        self.dyn(self.lits(4000))
        self.dyn([(258, self.rnd.randrange(300, 4000)) for _ in range(150)])

    def goto(self, target, slack=0):
        """blocks that hold no chunk start and end at bit `target`: one dynamic block of literals from here to just short of
        it, which starts at least `slack` bits in front of it, and a fixed block of 8- and 9-bit literals for the rest"""
        assert target - self.bit >= max(slack, 2000), (target, self.bit, slack)
        lo, hi = 1, (target - self.bit) // 4
        lits = self.lits(hi)
        while lo < hi:                       # the most literals that leave 66 bits and more (every gap from 66 on is 10 + 8a + 9b)
            mid = (lo + hi + 1) // 2
            if self.bit + _bits(dict(kind='dynamic', tokens=lits[:mid])) <= target - 66:
                lo = mid
            else:
                hi = mid - 1
        self.dyn(lits[:lo])
        gap = target - self.bit
        assert 66 <= gap < 400, gap
        for b in range(8):
            if (gap - 10 - 9 * b) % 8 == 0:
                a = (gap - 10 - 9 * b) // 8
                self.add(dict(kind='fixed', tokens=[self.rnd.randrange(48, 112) for _ in range(a)] + [self.rnd.randrange(144, 256) for _ in range(b)]))
                break
        assert self.bit == target

    def stream(self, name, reaches, chunk_sizes=CHUNKS, fail_block=None):
        self.member()
        data, text, table = b'', b'', []
        for blocks in self.members:
            st = []
            raw, t = W.build(blocks, st)
            for i, b in enumerate(blocks):
                table.append(dict(bit=8 * (len(data) + 10) + st[i][0], out=len(text) + st[i][1], mout=len(text), first=i == 0,
                                  kind=b['kind'], final=b.get('final', i == len(blocks) - 1), tokens=b.get('tokens', []), data=b.get('data', b'')))
            data += gz_member(raw)
            text += t
        assert data and len(data) == self.nbytes
        if fail_block is not None:
            fail_block %= len(table)
            text = text[:table[fail_block]['out']]
        if not isinstance(reaches, dict):
            reaches = {cb: reaches for cb in chunk_sizes}
        return Stream(name, data, text, table, tuple(chunk_sizes), {cb: frozenset(v) for cb, v in reaches.items()}, fail_block)


def _bits(block):
    """the length in bits of a fixed or dynamic block (it does not depend on where the block starts)"""
    st = []
    W.build([dict(block, final=False)], st)
    return st[-1][0]


class _Toks(object):
    """tokens of a block that starts a chunk, the chunk's output position o at hand"""

    def __init__(self, f):
        self.f, self.t, self.o = f, [], 0

    def lits(self, n):
        self.t += self.f.lits(n); self.o += n
        return self

    def copy(self, length, dist, times=1):
        self.t += [(length, dist)] * times; self.o += length * times
        return self

    def until(self, o, dist=WINDOW):
        """copies of 258 and one shorter up to output position o"""
        n = o - self.o
        assert n >= 3 and n % 258 not in (1, 2), n
        self.copy(258, dist, n // 258)
        if n % 258:
            self.copy(n % 258, dist)
        return self


# ---- the streams ---------------------------------------------------------------------------------------------------

def ring_copies():
    f = _File(11)
    f.preamble()
    # markers copied over themselves, the wave's 64 lanes a side of the distance; a copy half in front of the chunk
    f.anchor(_Toks(f).copy(258, 1).copy(258, 300).lits(5).copy(100, 400).t)
    f.anchor(_Toks(f).lits(4).copy(258, 63).lits(3).t)
    f.anchor(_Toks(f).copy(258, 64).lits(3).t)
    f.anchor(_Toks(f).lits(1).copy(258, 65).lits(3).t)
    # far copies whose writes land on the ring slots of their own sources
    t = _Toks(f).lits(2).until(32766).copy(258, 32768)              # (that one: its source starts 2 in front of the chunk)
    t.until(40000).lits(7)
    for length, dist in ((258, 32768), (258, 32767), (258, 32511), (258, 32510), (258, 32509), (100, 32700), (65, 32750), (64, 32750),
                         (40, 32740), (3, 32768), (3, 32766), (257, 32768), (258, 1), (258, 2), (65, 63), (65, 64), (66, 65), (258, 257)):
        t.copy(length, dist).lits(1)
    # writes across the wrap with the source across it too, then a source alone across it
    t.until(65400, 32767).copy(258, 32768).lits(3)
    t.until(65536 + 300, 32600).copy(258, 400).lits(3)
    t.until(98304 - 100, 32768).copy(258, 32768 - 77).lits(9)
    f.anchor(t.t)
    f.dyn(f.lits(50))
    return f.stream('ring_copies', ['copy_overwrites_source', 'copy_overwrites_source_dist_32768', 'copy_overwrites_source_multi_pass',
                                    'copy_crosses_wrap_write', 'copy_crosses_wrap_source', 'copy_straddles_chunk_start'] +
                    ['overlap_of_markers_%d' % d for d in MARKER_OVERLAPS])


def flush():
    f = _File(12)
    f.preamble()
    # exactly full with a copy, then with a literal; one past with a literal
    t = _Toks(f).lits(2).copy(258, 32768, 127)                    # o + len - f == 32768 at the last one
    t.copy(258, 32100)                                            # flushes: f = 32768
    t.copy(258, 32768, 126).lits(4)                               # ... == 32768 at the second literal, 32769 at the third
    f.anchor(t.t)
    # one past with a copy (not from 32 768 back: that one writes what the slot held)
    f.anchor(_Toks(f).lits(3).copy(258, 32768, 126).copy(258, 32100).lits(5).t)
    f.dyn(f.lits(50))
    return f.stream('flush', ['flush_at_equality', 'flush_one_past'])


def stored():
    f = _File(13)
    f.preamble()
    f.anchor(f.lits(50))
    o = 50
    for n in (0, 1, 4095, 4096, 4097, 65535, 32768):
        f.add(dict(kind='stored', data=bytes(f.lits(n))))
        o += n
    assert 98304 + 300 < o < 98304 + WINDOW
    # copies back into the stored bytes: across the wrap at 98 304, at the window's reach, overlapping
    t = [(258, o - (98304 - 100)), 7, (258, 32768), (258, 32767), (200, 1), (258, 4097)]
    f.add(dict(kind='fixed', tokens=t))
    f.add(dict(kind='stored', data=bytes(f.lits(4097))))
    f.dyn([(258, 4097), (258, 32768)] + f.lits(50))
    return f.stream('stored', ['stored_len_%d' % n for n in STORED_LENS] + ['stored_crosses_wrap', 'flush_inside_stored', 'ref_into_stored_across_wrap'])


def _page(j):
    """the bit of byte 10 + 1024 j: a nominal chunk start at every size of CHUNKS"""
    return 80 + 8192 * j


def finder():
    f = _File(14)
    f.dyn(f.lits(200))
    j = 0

    def true_header_at(bit):
        f.goto(bit)
        f.dyn(f.lits(30))
    for d in FIND_OFFSETS:
        j += 3
        true_header_at(_page(j) + d)
    for cb in CHUNKS:                                               # the last bit of a range of cb bytes, nothing in the range in front of it
        j += 3
        true_header_at(_page(j) + 8 * cb - 1)
    i = (f.bit + 8 * 3072 - 80) // 800 + 1                          # ... and of a range of 100 bytes: three rounds and 32 bits
    true_header_at(80 + 800 * i + 799)
    # a planted header -- the payload of a stored block -- and a true one 160 bits behind it, both in the first round of a range
    j = (f.bit - 80) // 8192 + 3
    fake, _ = W.build([dict(kind='dynamic', tokens=list(b'ACGT' * 20), final=False)])
    fake = (fake + b'ACGTACGTACGTACGTACGT')[:20]
    true = _page(j) + 248
    f.goto(true - 160 - 32 - 3)
    f.add(dict(kind='stored', data=fake))
    assert f.bit == true
    f.dyn(f.lits(300))
    f.dyn(f.lits(1450))
    f.dyn(f.lits(30))
    found = ['find_offset_%d' % d for d in FIND_OFFSETS] + ['find_offset_last', 'find_offset_unaligned', 'two_candidates_in_one_round']
    return f.stream('finder', dict([(cb, found) for cb in CHUNKS] + [(100, ['find_offset_last', 'find_offset_unaligned', 'find_offset_odd_range'])]),
                    chunk_sizes=CHUNKS + (100, ))


def resolve():
    f = _File(15)
    f.preamble()
    # four short chunks in a row; the last one's first copy names a byte of the first
    f.anchor(f.lits(1450))
    f.dyn(f.lits(1450))
    f.dyn(f.lits(1450))
    f.dyn([(258, 2 * 1450 + 700), (258, 32768), (100, 4000)] + f.lits(1450))
    # chunks of 32 767, 32 768 and 32 769 symbols: each starts with a copy of window byte 0 and ends in literals
    for n in (32767, 32768, 32769):
        f.dyn(_Toks(f).until(n - 1450).lits(1450).t)
    # a chunk of no symbols: an empty block (with as long a header as can be) across a nominal start, a chunk start behind it
    empty = dict(kind='dynamic', tokens=[], lit_lens=[9] * 256 + [6] * 28 + [5] * 2, dist_lens=[5] * 28 + [4] * 2)
    n = _bits(empty)
    assert 100 < n < 500, n
    j = (f.bit - 80) // 8192 + 3
    f.goto(_page(j) - n // 2, slack=8192 + 64)
    f.add(empty)
    f.dyn([(258, 32768), (258, 20000), (258, 1)] + f.lits(1450))
    f.dyn(f.lits(50))
    return f.stream('resolve', ['chunk_nsym_%d' % n for n in NSYMS] + ['short_chunk_hops'])


def _members(reach, at_end):
    f = _File(16)
    f.preamble()
    f.dyn(f.lits(1450))                                             # (the final block: no chunk starts at it)
    f.member()
    # a member that starts inside a chunk: 500 bytes of it, then a chunk start whose first copy reaches `reach` back
    f.add(dict(kind='fixed', tokens=f.lits(500)))
    f.dyn([(200, reach)] + f.lits(1450))
    f.dyn([(258, 1950), (258, 2208)] + f.lits(1450))
    f.member()
    # a member whose first block starts a chunk: the chunk in front ends with the member's header
    f.dyn(([(3, at_end)] if at_end else []) + f.lits(1450))
    f.dyn([(258, 1450), (258, 1708)] + f.lits(50))
    return f


def members():
    return _members(500, 0).stream('members', ['member_inside_chunk', 'member_at_chunk_end', 'ref_to_member_first_byte'])


def members_bad_inside():
    f = _members(501, 0)
    return f.stream('members_bad_inside', ['member_inside_chunk', 'ref_before_member'], fail_block=len(f.members[0]) + 1)


def members_bad_at_end():
    f = _members(500, 1)
    return f.stream('members_bad_at_end', ['member_inside_chunk', 'member_at_chunk_end', 'ref_to_member_first_byte', 'ref_before_member'],
                    fail_block=len(f.members[0]) + 3)


def big_chunk():
    text = b'ACGT' * 1100000
    return Stream('big_chunk', gzip.compress(text, 9), text, None, (1 << 24, ), {1 << 24: frozenset(['big_chunk'])}, None)


FAMILIES = collections.OrderedDict([
    ('ring_copies', [ring_copies]), ('stored', [stored]), ('flush', [flush]), ('finder', [finder]), ('resolve', [resolve]),
    ('members', [members, members_bad_inside, members_bad_at_end]), ('big_chunk', [big_chunk])])

_BUILT = {}


def family(name):
    """the streams of a family, built once"""
    if name not in _BUILT:
        _BUILT[name] = [make() for make in FAMILIES[name]]
    return _BUILT[name]


def invalid_behind_valid(blocks, tail=b''):
    """a member of valid dynamic blocks -- chunk starts at chunk size 256 -- and then the given (invalid) blocks -> file bytes.
    tail: bytes behind the last block, for zlib to read on into where it gives its verdict only some bits further"""
    f = _File(17)
    for _ in range(3):
        f.dyn(f.lits(600))
    pre = list(f.cur)
    return gz_member(W.build(pre + [dict(b) for b in blocks])[0] + tail)


# ---- what a run went through ---------------------------------------------------------------------------------------

def seams(stream, chunks, chunk_bytes):
    """the seam classes the run whose gzip_spec.last_chunks() is `chunks` went through, counted.  The chunks must start at
    block starts of the stream and hold the symbols its tokens mean."""
    cand, starts, ends, nsym = (list(map(int, a)) for a in chunks)
    c = collections.Counter()
    for n in nsym:
        if n in NSYMS:
            c['chunk_nsym_%d' % n] += 1
        if n > BIG:
            c['big_chunk'] += 1
    table, text = stream.table, stream.text
    if table is None:
        return c
    by_bit = {b['bit']: i for i, b in enumerate(table)}
    first = [by_bit[s] for s in starts]                             # (KeyError: a chunk that starts off a block boundary)
    assert first == sorted(first) and first[0] == 0                 # (two may start at one block: a refuted chunk moved onto the next one's start)
    stop = len(table) if stream.fail_block is None else stream.fail_block + 1
    cbase = [table[i]['out'] for i in first]

    # the finder: nominal starts every chunk_bytes behind the first block's byte, the last range up to the file's end
    limit = 8 * len(stream.data)
    los = list(range(((starts[0] >> 3) + chunk_bytes) * 8, limit, 8 * chunk_bytes))
    assert len(los) == len(cand)
    for i, lo in enumerate(los):
        hi = los[i + 1] if i + 1 < len(los) else limit
        if cand[i] < 0:
            continue
        assert lo <= cand[i] < hi
        b = table[by_bit[cand[i]]] if cand[i] in by_bit else None
        if b is not None:
            assert b['kind'] == 'dynamic' and not b['final']
            d = cand[i] - lo
            if cand[i] in starts and (d in FIND_OFFSETS or cand[i] == hi - 1):
                c['find_offset_last' if cand[i] == hi - 1 else 'find_offset_%d' % d] += 1
                c['find_offset_unaligned'] += cand[i] & 7 != 0
                c['find_offset_odd_range'] += (hi - lo) % 256 != 0
        elif any(cand[i] < t['bit'] < hi and (t['bit'] - lo) // 256 == (cand[i] - lo) // 256 and t['kind'] == 'dynamic' and not t['final']
                 for t in table):
            c['two_candidates_in_one_round'] += 1                  # a planted header reported, a true one behind it in its round

    for k, i0 in enumerate(first):
        i1 = first[k + 1] if k + 1 < len(first) else len(table)
        base, o, f, mstart, spans, failed = cbase[k], 0, 0, -1, [], False

        def room(o, n):
            nonlocal f
            v = o + n - f
            c['flush_at_equality'] += v == WINDOW
            # (one past: the write takes the ring slot of symbol f, the oldest one not yet in the slot; a flush one symbol
            # late shows where the two differ)
            c['flush_one_past'] += v == WINDOW + 1 and text[base + f] != text[base + f + WINDOW]
            if v > WINDOW:
                f = o
                return True
            return False
        for i in range(i0, min(i1, stop)):
            b = table[i]
            assert b['out'] == base + o
            if b['first'] and i > i0:
                mstart = o
            if b['kind'] == 'stored':
                n = len(b['data'])
                if n in STORED_LENS:
                    c['stored_len_%d' % n] += 1
                c['stored_crosses_wrap'] += n > 0 and o // WINDOW != (o + n - 1) // WINDOW
                for a in range(0, n, 4096):
                    c['flush_inside_stored'] += room(o + a, min(4096, n - a)) and a > 0
                spans.append((o, o + n))
                o += n
                continue
            for t in b['tokens']:
                if isinstance(t, int):
                    room(o, 1)
                    o += 1
                    continue
                n, d = t[0], t[1]
                s0, m = o - d, min(t[0], t[1])
                src = base + s0                                     # the text offset of the first source byte
                if src < b['mout']:
                    assert i == stream.fail_block and src == b['mout'] - 1
                    c['ref_before_member'] += s0 < 0                # (from the chunk behind: else the decoder sees it by itself)
                    failed = True
                    break
                if s0 < 0:
                    c['ref_to_member_first_byte'] += src == b['mout']
                    c['copy_straddles_chunk_start'] += s0 + m > 0
                    if d < n and d in MARKER_OVERLAPS:
                        c['overlap_of_markers_%d' % d] += 1
                    made_in = bisect.bisect_right(cbase, src) - 1
                    c['short_chunk_hops'] += k >= 3 and made_in <= k - 3 and max(nsym[k - 2:k + 1]) < WINDOW
                else:
                    if d >= n and d > WINDOW - n:
                        c['copy_overwrites_source'] += 1
                        c['copy_overwrites_source_dist_32768'] += d == WINDOW
                        c['copy_overwrites_source_multi_pass'] += n > 64
                    c['copy_crosses_wrap_source'] += s0 // WINDOW != (s0 + m - 1) // WINDOW
                    c['ref_into_stored_across_wrap'] += any(a <= s0 and s0 + m <= z for a, z in spans) and s0 // WINDOW != (s0 + m - 1) // WINDOW
                c['copy_crosses_wrap_write'] += o // WINDOW != (o + n - 1) // WINDOW
                room(o, n)
                o += n
            if failed:
                break
        if failed or i1 > stop:
            break
        assert o == nsym[k], 'chunk %d holds %d symbols, its blocks mean %d' % (k, nsym[k], o)
        if i1 < len(table) and table[i1]['first']:
            mstart = o
        c['member_at_chunk_end'] += mstart == o and mstart >= 0
        c['member_inside_chunk'] += 0 < mstart < o
    return +c
