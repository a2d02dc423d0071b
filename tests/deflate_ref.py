"""
The texts and the checks of the emit's deflate (include/kvarq_hip.h; kvq_deflate.h).  Every text has a census
that is asserted before anything is compared: what of the definition it reaches is said there, in plain Python -- the hash, the
final table of a segment, the trigrams of a text.  ``check`` is what any output must pass: zlib inflates it (and so has verified
every CRC-32 and ISIZE), ``kvarq_amd.bgzf.index`` walks it, every member is at most 65 536 bytes with BSIZE right, the last 28 bytes
are the EOF member and no other member is empty, and the project's own decoder (kvq_inflate_raw_host) returns the same bytes.
``tokens`` is a small inflate of its own that keeps the tokens: no match of any member crosses a multiple of 255 bytes, none
reaches further back than the first byte of the segment two in front, and the code lengths are within their limits.
"""
import functools
import gzip
import struct

import numpy as np

BLOCK, SEG, SEGS, SLOTS, REACH = 65280, 255, 256, 128, 2
EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
MEMBERS, BYTES_IN, BYTES_OUT, STORED, MATCHES, LITERALS, MAX_DISTANCE, MAX_LENGTH, LEN = 0, 1, 2, 3, 4, 5, 6, 7, 8
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0] * 4 + [k for k in range(1, 14) for _ in (0, 1)]


# ---- the definition's pieces, in plain Python ----
def hash3(b):
    """kvq_deflate_hash of three bytes"""
    return (((b[0] | b[1] << 8 | b[2] << 16) * 0x9E3779B1) & 0xFFFFFFFF) >> 25


def final_table(block, seg):
    """the final table of a segment: slot -> the last position of the segment (counted from the block's first byte) whose three
    bytes hash there"""
    tab = {}
    for p in range(seg * SEG, min((seg + 1) * SEG, len(block))):
        if p + 3 <= len(block):
            tab[hash3(block[p:p + 3])] = p
    return tab


def parse(block):
    """the parse of one block (at most BLOCK bytes) as kvq_deflate.h states it in words -> its tokens in the form of ``tokens``:
    ints for literals, (length, distance) for matches.  Segment s of SEG bytes is parsed greedily from its first byte.  At a
    position p with p + 3 <= the segment's end the candidates are, in this order, the last position in front of p in the segment
    whose three bytes hash as p's do (its own running table), and what the FINAL tables of the segments s - 1 and s - 2 hold for
    that hash; a candidate's match is the common prefix of the raw block at both positions, cut at the segment's end; the longest
    wins, the first among equals; three bytes or more are a match, else block[p] is a literal.  Every position i with i + 3 <= n
    is entered into the running table, those inside a match too."""
    block = bytes(block)
    n = len(block)
    assert n <= BLOCK
    toks = []
    hashes = [hash3(block[i:i + 3]) for i in range(n - 2)]                        # of every position i with i + 3 <= n
    finals =[final_table(block, s) for s in range((n + SEG - 1) // SEG)]         # (functions of the text, not of any parse)
    for s in range(len(finals)):
        end = min((s + 1) * SEG, n)
        own = {}
        tables = [own] + [finals[s - back] for back in range(1, REACH + 1) if s - back >= 0]
        p = s * SEG
        while p < end:
            best = best_q = 0
            if p + 3 <= end:
                for table in tables:
                    q = table.get(hashes[p])
                    if q is None:
                        continue
                    k = 0
                    while p + k < end and block[q + k] == block[p + k]:
                        k += 1
                    if k > best:
                        best, best_q = k, q
            step = best if best >= 3 else 1
            toks.append((best, p - best_q) if best >= 3 else block[p])
            for i in range(p, min(p + step, n - 2)):
                own[hashes[i]] = i
            p += step
    return toks


def repeats(text):
    """the trigrams of a text that occur more than once"""
    seen, twice = set(), set()
    for i in range(len(text) - 2):
        g = text[i:i + 3]
        (twice if g in seen else seen).add(g)
    return twice


# ---- members and tokens ----
def members(out):
    """[(offset, member bytes, payload, crc, isize)] of a BGZF stream"""
    res, at = [], 0
    while at < len(out):
        assert out[at:at + 16] == EOF[:16], at
        size = struct.unpack_from('<H', out, at + 16)[0] + 1
        crc, isize = struct.unpack_from('<II', out, at + size - 8)
        res.append((at, size, out[at + 18:at + size - 8], crc, isize))
        at += size
    assert at == len(out)
    return res


class _Bits(object):
    def __init__(self, data):
        self.d, self.at = bytes(data), 0

    def get(self, n):
        """the next n <= 16 bits, the first the lowest (bits behind the data's end read as 0)"""
        r = (int.from_bytes(self.d[self.at >> 3:(self.at >> 3) + 4], 'little') >> (self.at & 7)) & ((1 << n) - 1)
        self.at += n
        return r


def _decoder(lens):
    """canonical codes of a length list: {(length, code): symbol}"""
    code, table = 0, {}
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def _sym(bits, table):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.get(1)
        if (l, code) in table:
            return table[(l, code)]
    raise AssertionError('no such code')


def tokens(payload):
    """one final DEFLATE block -> dict(btype, and for BTYPE 2: hlit, hdist, hclen, cl_lens, ll_lens, d_lens, tokens -- ints for
    literals, (length, distance) for matches)"""
    b = _Bits(payload)
    assert b.get(1) == 1                                         # one final block
    btype = b.get(2)
    if btype == 0:
        n, nn = struct.unpack_from('<HH', payload, 1)
        assert n ^ nn == 0xFFFF and len(payload) == 5 + n
        return dict(btype=0, n=n)
    assert btype == 2                                            # (there is no fixed-Huffman block)
    hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = b.get(3)
    ct, lens = _decoder(cl), []
    while len(lens) < hlit + hdist:
        s = _sym(b, ct)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.get(2))
        else:
            lens += [0] * (3 + b.get(3) if s == 17 else 11 + b.get(7))
    assert len(lens) == hlit + hdist
    ll, d = lens[:hlit], lens[hlit:]
    lt, dt, toks = _decoder(ll), _decoder(d), []
    while True:
        s = _sym(b, lt)
        if s < 256:
            toks.append(s)
        elif s == 256:
            break
        else:
            assert s < 286
            length = LEN_BASE[s - 257] + b.get(LEN_EXTRA[s - 257])
            ds = _sym(b, dt)
            assert ds < 30
            toks.append((length, DIST_BASE[ds] + b.get(DIST_EXTRA[ds])))
    assert (b.at + 7) // 8 == len(payload)
    return dict(btype=2, hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl, ll_lens=ll, d_lens=d, tokens=toks)


def kraft(lens, limit):
    """the Kraft sum of a length list times 2^limit"""
    return sum(1 << (limit - l) for l in lens if l)


def check_tokens(t, isize):
    """the parse's rule, read off a member's tokens: no match crosses a segment's end or reaches in front of the segment two
    before its own; the codes are within their limits and complete (or the legal one-code case)"""
    assert max(t['ll_lens']) <= 15 and max(t['d_lens']) <= 15 and max(t['cl_lens']) <= 7
    assert kraft(t['ll_lens'], 15) == 1 << 15 and kraft(t['cl_lens'], 7) == 1 << 7
    assert kraft(t['d_lens'], 15) == 1 << 15 or [l for l in t['d_lens'] if l] == [1]
    at = 0
    for k in t['tokens']:
        if isinstance(k, tuple):
            length, dist = k
            assert 3 <= length <= SEG and at // SEG == (at + length - 1) // SEG, (at, k)
            assert 1 <= dist <= at - max(at // SEG - REACH, 0) * SEG, (at, k)
            at += length
        else:
            at += 1
    assert at == isize


def census(out, deep=None):
    """the words as the stream itself says them (without the EOF member), and the tokens of every member -- of the first ``deep``
    members, when given: of the others only the block type is read, and the words of the parse are not to be compared"""
    w, toks = [0] * LEN, []
    for i, (at, size, payload, crc, isize) in enumerate(members(out)):
        t = tokens(payload) if deep is None or i < deep else dict(btype=(payload[0] >> 1) & 3)
        toks.append(t)
        w[MEMBERS] += 1; w[BYTES_IN] += isize; w[BYTES_OUT] += size; w[STORED] += t['btype'] == 0
        for k in t.get('tokens', ()):
            if isinstance(k, tuple):
                w[MATCHES] += 1; w[MAX_LENGTH] = max(w[MAX_LENGTH], k[0]); w[MAX_DISTANCE] = max(w[MAX_DISTANCE], k[1])
            else:
                w[LITERALS] += 1
    return w, toks


def check(out, text, words=None, deep=None):
    """what any BGZF(text) must pass (``out``: the members without the EOF member) -> the tokens of every member (``deep``: as for
    ``census``; every member is inflated twice whatever it says)"""
    from kvarq_amd import _lib, bgzf
    text = bytes(text)
    whole = bytes(out) + EOF
    assert gzip.decompress(whole) == text                        # (zlib verifies every CRC-32 and ISIZE)
    assert whole[-28:] == EOF
    ms = members(whole)
    assert len(ms) == (len(text) + BLOCK - 1) // BLOCK + 1
    walked = bgzf.index(whole)
    assert walked is not None and walked[0].tolist() == [m[0] for m in ms] and walked[1].tolist() == [m[1] for m in ms] and walked[2].tolist() == [m[4] for m in ms]
    at = 0
    for i, (off, size, payload, crc, isize) in enumerate(ms):
        assert size <= 65536 and isize == (0 if i == len(ms) - 1 else min(BLOCK, len(text) - at)) and (isize > 0) == (i < len(ms) - 1)
        if isize:
            back = np.zeros(isize, dtype=np.uint8)
            assert _lib.lib().kvq_inflate_raw_host(payload, len(payload), back.ctypes.data, isize) == 0
            assert back.tobytes() == text[at:at + isize]
        at += isize
    w, toks = census(out, deep)
    for (off, size, payload, crc, isize), t in zip(ms, toks):
        if t['btype'] == 2 and 'tokens' in t:
            check_tokens(t, isize)
        elif t['btype'] == 0:
            assert size == isize + 5 + 26
    if words is not None:
        assert list(words)[:MATCHES if deep is not None else LEN] == w[:MATCHES if deep is not None else LEN], (list(words), w)
    return toks


# ---- the texts ----
def filler(n, seed=0):
    """n bytes in which no trigram repeats: the 16-bit numbers from ``seed`` on, high byte first (bytes below 0xC0 only)"""
    assert seed + (n + 1) // 2 < 0xC000
    return b''.join(struct.pack('>H', i) for i in range(seed, seed + (n + 1) // 2))[:n]


def _with(base, at, piece):
    return base[:at] + piece + base[at + len(piece):]


def pattern(build, holds):
    """forty different bytes no filler has, the first of a fixed list of candidates for which the text ``build(pattern)`` is one
    where ``holds(text, pattern)``: a table has 128 slots for the 255 positions of a segment, so most three bytes are written over by
    a later position of their segment -- the texts need some that are not"""
    for m in range(1, 64, 2):
        for c in range(64):
            p = bytes(0xC0 + (c + m * i) % 64 for i in range(40))
            t = build(p)
            if holds(t, p):
                return t, p
    raise AssertionError('no pattern')


@functools.lru_cache(maxsize=None)
def fastq(n, seed=7):
    """n bytes of FastQ-like text with names that count, as the emit makes it"""
    rng = np.random.RandomState(seed)
    out, i = [], 0
    while sum(map(len, out)) < n:
        L = int(rng.randint(30, 151))
        out.append(b'@SRR%07d.%d FC:3:%d:%d:%d\n' % (seed, i, 1101 + i // 4000, 1000 + (i * 37) % 19000, 2000 + (i * 101) % 98000))
        out.append(bytes(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), L)) + b'\n+\n')
        out.append(bytes(rng.choice(np.frombuffer(b'IIIIIIHHHGGFFEDCBA@?>=<', dtype=np.uint8), L)) + b'\n')
        i += 1
    return b''.join(out)[:n]


def _segment_end_holds(t, p):
    return final_table(t, 0)[hash3(p[:3])] == 0 and final_table(t, 0)[hash3(p[10:13])] == 10


def _block_end_holds(t, p):
    return final_table(t[:BLOCK], (BLOCK - 700) // SEG)[hash3(p[:3])] == BLOCK - 700


def _farthest_holds(t, p):
    return final_table(t, 0)[hash3(p[:3])] == 0


@functools.lru_cache(maxsize=None)
def text_and_pattern(name):
    if name == 'segment-end':
        # the forty bytes at 0, and again from 500 on: across the end of segment 1 at 510
        return pattern(lambda p: _with(_with(filler(2000), 0, p), 500, p), _segment_end_holds)
    if name == 'block-end':
        # ... and again from twenty bytes in front of the block's end on, into the next block
        return pattern(lambda p: _with(_with(filler(BLOCK + 1000), BLOCK - 700, p), BLOCK - 20, p), _block_end_holds)
    if name == 'reach':
        # three bytes at 254, the last place of segment 0, and again at 1017, where a match of segment 3 may still begin: distance 763,
        # and only a parse that looked three segments back would find it
        return pattern(lambda p: _with(_with(filler(2000, 0x1000), 254, p[:3]), 1017, p[:3]), lambda t, p: final_table(t, 0)[hash3(p[:3])] == 254 and repeats(t) == {p[:3]})
    # three bytes at 0 and again at 762 (the last place of segment 2 a match can begin at: its distance is the farthest there is), or at 763
    at = {'farthest': 762, 'beyond': 763}[name]
    return pattern(lambda p: _with(_with(filler(2000, 0x1000), 0, p[:3]), at, p[:3]), _farthest_holds)


@functools.lru_cache(maxsize=None)
def text(name):
    if name == 'empty':
        return b''
    if name == 'one':
        return b'a'
    if name in ('block-1', 'block', 'block+1', 'two-blocks+1'):
        return fastq({'block-1': BLOCK - 1, 'block': BLOCK, 'block+1': BLOCK + 1, 'two-blocks+1': 2 * BLOCK + 1}[name])
    if name == 'one-byte':
        return b'a' * (BLOCK + 300)
    if name == 'no-repeat':
        return filler(30000)
    if name == 'fibonacci':
        fib = [1, 1]
        while len(fib) < 22:
            fib.append(fib[-1] + fib[-2])
        t = np.repeat(np.arange(22, dtype=np.uint8) + ord('a'), fib)
        np.random.RandomState(22).shuffle(t)
        return t.tobytes()
    if name == 'random':
        return np.random.RandomState(5).randint(0, 256, 70000).astype(np.uint8).tobytes()
    if name in ('segment-end', 'block-end', 'farthest', 'beyond', 'reach'):
        return text_and_pattern(name)[0]
    raise KeyError(name)


NAMES = ('empty', 'one', 'block-1', 'block', 'block+1', 'two-blocks+1', 'one-byte', 'no-repeat', 'fibonacci', 'random', 'segment-end',
         'block-end', 'farthest', 'beyond', 'reach')


def text_census(name):
    """what the text is there for, asserted of the text alone"""
    t = text(name)
    if name in ('empty', 'one'):
        assert len(t) == (0, 1)[name == 'one']
    elif name in ('block-1', 'block', 'block+1', 'two-blocks+1'):
        assert len(t) == {'block-1': 65279, 'block': 65280, 'block+1': 65281, 'two-blocks+1': 130561}[name] and t.count(b'\n+\n') > 200
    elif name == 'one-byte':
        assert set(t) == {ord('a')} and len(t) > BLOCK + SEG
    elif name == 'no-repeat':
        assert not repeats(t) and len(t) == 30000
    elif name == 'fibonacci':
        c = sorted(np.bincount(np.frombuffer(t, dtype=np.uint8))[ord('a'):ord('a') + 22].tolist())
        assert len(set(t)) == 22 and len(t) == 46367 and c[:4] == [1, 1, 2, 3] and all(c[i] == c[i - 1] + c[i - 2] for i in range(2, 22))
    elif name == 'random':
        assert len(t) == 70000 and len(set(t)) == 256
    elif name == 'segment-end':
        p = text_and_pattern(name)[1]
        assert len(set(p)) == 40 and t[:40] == t[500:540] == p and t.count(p[:3]) == 2 and repeats(t) == set(p[i:i + 3] for i in range(38))
        # the tables still point at the pattern where the parse looks: at 500 the one of segment 0, at 510 -- the pattern's byte 10 -- too
        assert _segment_end_holds(t, p)
    elif name == 'block-end':
        p = text_and_pattern(name)[1]
        assert t[BLOCK - 20:BLOCK + 20] == p and t[BLOCK - 700:BLOCK - 660] == p and repeats(t[:BLOCK]) == set(p[i:i + 3] for i in range(18))
        assert _block_end_holds(t, p) and (BLOCK - 20) // SEG - (BLOCK - 700) // SEG == REACH
        assert not repeats(t[BLOCK:])
    elif name == 'reach':
        p = text_and_pattern(name)[1]
        assert t[254:257] == t[1017:1020] == p[:3] and repeats(t) == {p[:3]} and final_table(t, 0)[hash3(p[:3])] == 254
        assert 254 // SEG == 0 and 1017 // SEG == REACH + 1 and 1017 + 3 <= (REACH + 2) * SEG and 1017 - 254 == 763
    else:
        at, p = 762 if name == 'farthest' else 763, text_and_pattern(name)[1]
        assert t[:3] == t[at:at + 3] == p[:3] and repeats(t) == {p[:3]} and _farthest_holds(t, p)
        assert at // SEG == REACH and (at + 3 <= 3 * SEG) == (name == 'farthest')


def stream_census(name, toks, w):
    """what the text must have made of the definition, read off the stream's own tokens and words"""
    t = text(name)
    if name == 'empty':
        assert w == [0] * LEN
    elif name == 'one':
        assert w[:4] == [1, 1, 32, 1]                            # (a dynamic block of one literal is longer than six stored bytes)
    elif name in ('block-1', 'block', 'block+1', 'two-blocks+1'):
        assert w[MEMBERS] == (len(t) + BLOCK - 1) // BLOCK and all(k['btype'] == 2 for k in toks[:len(t) // BLOCK]) and w[BYTES_OUT] < len(t) // 2
    elif name == 'one-byte':
        # distance 1 and the longest match the rule allows at every chance: a literal a block, then every segment one match to its end
        assert w[STORED] == 0 and w[LITERALS] == 2 and w[MAX_DISTANCE] == 1 and w[MAX_LENGTH] == SEG
        assert toks[0]['tokens'] == [ord('a'), (SEG - 1, 1)] + [(SEG, 1)] * (SEGS - 1) and toks[1]['tokens'] == [ord('a'), (SEG - 1, 1), (300 - SEG, 1)]
        for k in toks:
            assert k['hdist'] == 1 and k['d_lens'] == [1]        # a single distance code, of one bit
            assert [s for s, l in enumerate(k['ll_lens']) if l and s < 257] == [ord('a'), 256]      # one literal and end-of-block
    elif name == 'no-repeat':
        assert w[MATCHES] == 0 and w[LITERALS] == len(t) and toks[0]['hdist'] == 1 and toks[0]['d_lens'] == [1]
    elif name == 'fibonacci':
        assert w[STORED] == 0 and max(toks[0]['ll_lens']) <= 15
    elif name == 'random':
        assert w[STORED] == w[MEMBERS] == 2 and w[BYTES_OUT] == len(t) + 2 * 31
    elif name == 'segment-end':
        # the match at 500 ends with segment 1, and segment 2 goes on with the pattern's byte 10 from segment 0
        at, found = 0, {}
        for k in toks[0]['tokens']:
            found[at] = k
            at += k[0] if isinstance(k, tuple) else 1
        assert found[500] == (10, 500) and found[510] == (30, 500) and w[MATCHES] == 2
    elif name == 'block-end':
        # the match is cut at the block's end, and the next member begins with literals: it knows nothing of the block before it
        assert toks[0]['tokens'][-1] == (20, 680) and all(not isinstance(k, tuple) for k in toks[1]['tokens']) and w[MATCHES] == 1
    elif name == 'farthest':
        assert w[MATCHES] == 1 and w[MAX_DISTANCE] == 762 == SEG * (REACH + 1) - 3 and w[MAX_LENGTH] == 3
    else:
        # 'beyond': three bytes no longer fit in front of the segment's end; 'reach': the source lies three segments back
        assert w[MATCHES] == 0


# ---- the code builder, as a plain statement of the same rule ----
def lengths(freq, limit):
    """kvq_deflate_lengths: the Huffman tree of the used symbols sorted by (count, symbol), two queues, the leaf first among equals;
    depths cut at the limit, the Kraft sum repaired from the longest length below the limit that has a code; the lengths to the
    symbols in sorted order, the longest to the rarest"""
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    lens = [0] * len(freq)
    n = len(order)
    if n == 1:
        lens[order[0][1]] = 1
    if n < 2:
        return lens
    weight, parent = [f for f, _ in order], {}
    leaf, inner = 0, n
    for k in range(n, 2 * n - 1):
        total = 0
        for _ in (0, 1):
            if leaf < n and (inner >= k or weight[leaf] <= weight[inner]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, inner = inner, inner + 1
            total += weight[pick]
            parent[pick] = k
        weight.append(total)
    depth = {2 * n - 2: 0}
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    count = [0] * (limit + 2)
    for i in range(n):
        count[min(depth[i], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1; count[l + 1] += 2
                break
        total -= 1
    at = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[order[at][1]] = l
            at += 1
    return lens
