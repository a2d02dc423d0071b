"""
A raw-DEFLATE (RFC 1951) writer and a plain reference inflater, both for tests and both standard
library only.

The writer takes a list of blocks and writes exactly what they say, valid or not: it never checks
a distance against the bytes written, a code set for completeness or a header count against its
limit, so invalid streams are made by overriding one field of a valid block.  A block is a dict:

  kind      'stored', 'fixed' or 'dynamic'
  final     BFINAL (default: True for the last block only)
  data      stored: the payload; stored_len / stored_nlen override LEN / NLEN
  tokens    fixed/dynamic: literals (ints), copies (length, dist) or (length, dist, 284) -- the last
            codes length 258 as symbol 284 with extra bits 31 -- and raw pieces ('sym', s) (a
            literal/length symbol), ('dsym', s) (a distance symbol), ('bits', value, n)
  eob       write end-of-block (default True)
  lit_lens, dist_lens   dynamic: code lengths (default: from the tokens' frequencies, 15-bit limit)
  hlit, hdist, hclen    dynamic: the header counts (default: trailing zero lengths trimmed)
  rle       dynamic: the code-length symbols as [(sym, extra)] (default: greedy 16/17/18 runs that
            may cross from literal/length into distance lengths)
  cl_lens   dynamic: the 19 code-length code lengths, indexed by symbol (default: from rle)

A symbol without a code is written as nothing.  build(blocks) -> (payload, text): text is what the
tokens mean (a copy reaching before the start reads zeros), the bytes a decoder must produce when
the stream is valid.  build(blocks, starts=[]) also reports where each block starts, in bits of the
payload and in bytes of the text.

inflate(payload, isize) is a slow puff.c-style inflater under zlib's rules (its one exception for an
incomplete code: a single code of one bit in a literal/length or distance code) and the host reader's
success rule: the final block reached and exactly isize bytes.  Besides the verdict it returns a census
of what the stream used, which is how a corpus proves the edges it covers.
"""
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0] * 4 + [k // 2 for k in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WINDOW = 32768


def len_symbol(length):
    """length 3..258 -> (symbol 257..285, extra value, extra bits)"""
    for s in range(28, -1, -1):
        if length >= LEN_BASE[s]:
            return 257 + s, length - LEN_BASE[s], LEN_EXTRA[s]
    raise ValueError(length)


def dist_symbol(dist):
    """distance 1..32768 -> (code 0..29, extra value, extra bits)"""
    for s in range(29, -1, -1):
        if dist >= DIST_BASE[s]:
            return s, dist - DIST_BASE[s], DIST_EXTRA[s]
    raise ValueError(dist)


def huffman_lengths(freqs, limit=15):
    """length-limited Huffman code lengths (package-merge); one used symbol gets a second one so the code is complete"""
    used = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        used.append(1 if used[0] == 0 else 0)
    leaves = sorted((max(1, freqs[s]), [s]) for s in used)
    cur = leaves
    for _ in range(limit - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = list(heapq.merge(leaves, pk, key=lambda x: x[0]))
    for _, ss in cur[:2 * len(used) - 2]:
        for s in ss:
            lens[s] += 1
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 codes, bit-reversed for the LSB-first stream: symbol -> (reversed code, length); over-subscribed
    sets still get codes (masked to their length)"""
    bl_count = [0] * 16
    for n in lens:
        if n:
            bl_count[n] += 1
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl_count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            c = nxt[n] & ((1 << n) - 1)
            nxt[n] += 1
            out[s] = (int(format(c, '0%db' % n)[::-1], 2), n)
    return out


def rle_lengths(lens):
    """greedy run-length form of code lengths: [(sym, extra)]"""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        if v == 0 and r >= 3:
            k = r
            while k >= 11:
                m = min(k, 138)
                out.append((18, m - 11)); k -= m
            if k >= 3:
                out.append((17, k - 3)); k = 0
            out += [(0, 0)] * k
        else:
            out.append((v, 0))
            k = r - 1
            while k >= 3:
                m = min(k, 6)
                out.append((16, m - 3)); k -= m
            out += [(v, 0)] * k
        i += r
    return out


RLE_EXTRA = {16: 2, 17: 3, 18: 7}


class BitWriter(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF); self.acc >>= 8; self.n -= 8

    def code(self, table, s):
        if s in table:
            self.put(*table[s])

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def _expand(tokens, text):
    for t in tokens:
        if isinstance(t, int):
            text.append(t)
        elif isinstance(t[0], int):
            length, dist = t[0], t[1]
            for _ in range(length):
                text.append(text[len(text) - dist] if dist <= len(text) else 0)


def dynamic_header(b):
    """a dynamic block's header fields, defaults filled in: (lit_lens, dist_lens, hlit, hdist, all_lens, rle, cl_lens, hclen)"""
    tokens = b.get('tokens', [])
    lf, df = [0] * 286, [0] * 30
    if b.get('eob', True):
        lf[256] += 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        elif isinstance(t[0], int):
            lf[284 if len(t) > 2 and t[2] == 284 else len_symbol(t[0])[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
    lit_lens = list(b['lit_lens']) if 'lit_lens' in b else huffman_lengths(lf)
    dist_lens = list(b['dist_lens']) if 'dist_lens' in b else (huffman_lengths(df) if any(df) else [1, 1])
    hlit = b.get('hlit', max(257, max([s + 1 for s, n in enumerate(lit_lens) if n] + [0])))
    hdist = b.get('hdist', max(1, max([s + 1 for s, n in enumerate(dist_lens) if n] + [0])))
    all_lens = (lit_lens + [0] * 300)[:hlit] + (dist_lens + [0] * 40)[:hdist]
    rle = b['rle'] if 'rle' in b else rle_lengths(all_lens)
    if 'cl_lens' in b:
        cl_lens = list(b['cl_lens'])
    else:
        cf = [0] * 19
        for s, _ in rle:
            cf[s] += 1
        cl_lens = huffman_lengths(cf, 7)
    hclen = b.get('hclen', max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]]))
    return lit_lens, dist_lens, hlit, hdist, all_lens, rle, cl_lens, hclen


def build(blocks, starts=None):
    """-> (payload, text).  starts (a list, filled in): per block the (bit offset in the payload, offset in the text) at
    which it starts, and one more pair for the end of the last block"""
    bw, text = BitWriter(), bytearray()
    for bi, b in enumerate(blocks):
        final = b.get('final', bi == len(blocks) - 1)
        kind = b['kind']
        if starts is not None:
            starts.append((8 * len(bw.out) + bw.n, len(text)))
        bw.put(1 if final else 0, 1)
        if kind == 'stored':
            data = b.get('data', b'')
            bw.put(0, 2)
            bw.align()
            ln = b.get('stored_len', len(data))
            bw.put(ln, 16)
            bw.put(b.get('stored_nlen', ln ^ 0xFFFF), 16)
            bw.out += data
            text += data
            continue
        tokens = b.get('tokens', [])
        if kind == 'fixed':
            bw.put(1, 2)
            lit, dist = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)
        else:
            bw.put(2, 2)
            lit_lens, dist_lens, hlit, hdist, all_lens, rle, cl_lens, hclen = dynamic_header(b)
            bw.put(hlit - 257, 5)
            bw.put(hdist - 1, 5)
            bw.put(hclen - 4, 4)
            for i in range(hclen):
                bw.put(cl_lens[CL_ORDER[i]] if i < 19 else 0, 3)
            clc = canonical_codes(cl_lens)
            for s, e in rle:
                bw.code(clc, s)
                if s in RLE_EXTRA:
                    bw.put(e, RLE_EXTRA[s])
            lit, dist = canonical_codes(lit_lens), canonical_codes(dist_lens)
        for t in tokens:
            if isinstance(t, int):
                bw.code(lit, t)
            elif t[0] == 'sym':
                bw.code(lit, t[1])
            elif t[0] == 'dsym':
                bw.code(dist, t[1])
            elif t[0] == 'bits':
                bw.put(t[1], t[2])
            else:
                length, d = t[0], t[1]
                if len(t) > 2 and t[2] == 284:
                    bw.code(lit, 284); bw.put(31, 5)
                else:
                    s, e, n = len_symbol(length)
                    bw.code(lit, s); bw.put(e, n)
                s, e, n = dist_symbol(d)
                bw.code(dist, s); bw.put(e, n)
        if b.get('eob', True):
            bw.code(lit, 256)
        _expand(tokens, text)
    if starts is not None:
        starts.append((8 * len(bw.out) + bw.n, len(text)))
    return bw.bytes(), bytes(text)


# ---- the reference inflater ------------------------------------------------------------------------------

class Bad(Exception):
    """an invalid stream: .args[0] is the reason ('truncated' when the payload ends early)"""


FAST = 9


class _Huff(object):
    """a canonical code: a FAST-bit table, longer codes by puff.c's walk"""

    def __init__(self, lens):
        self.count = [0] * 16
        for n in lens:
            self.count[n] += 1
        self.count[0] = 0
        offs = [0] * 16
        for n in range(1, 15):
            offs[n + 1] = offs[n] + self.count[n]
        self.symbol = [0] * len(lens)
        for s, n in enumerate(lens):
            if n:
                self.symbol[offs[n]] = s; offs[n] += 1
        self.maxlen = max([n for n in lens if n] + [0])
        self.fast = [None] * (1 << FAST)
        for s, (rc, n) in canonical_codes(lens).items():
            if n <= FAST:
                for k in range(1 << (FAST - n)):
                    self.fast[rc | k << n] = (s, n)

    def left(self):
        """codes left unused: < 0 over-subscribed, > 0 incomplete"""
        left = 1
        for n in range(1, 16):
            left = (left << 1) - self.count[n]
            if left < 0:
                return left
        return left


class _Bits(object):
    def __init__(self, data):
        self.data, self.nbits, self.pos = bytes(data) + b'\0' * 8, 8 * len(data), 0

    def peek(self, n):
        b = self.pos >> 3
        return (int.from_bytes(self.data[b:b + 5], 'little') >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        v = self.peek(n)
        self.pos += n
        if self.pos > self.nbits:
            raise Bad('truncated')
        return v

    def decode(self, h):
        e = h.fast[self.peek(FAST)]
        if e is None:
            bits, code, first, index = self.peek(15), 0, 0, 0
            for n in range(1, 16):
                code |= bits & 1; bits >>= 1
                c = h.count[n]
                if code - c < first:
                    e = (h.symbol[index + code - first], n)
                    break
                index += c; first = (first + c) << 1; code <<= 1
            if e is None:
                self.pos += h.maxlen + 1
                if self.pos > self.nbits:
                    raise Bad('truncated')
                raise Bad('invalid code')
        self.pos += e[1]
        if self.pos > self.nbits:
            raise Bad('truncated')
        return e


def _tree(lens, kind, what):
    h = _Huff(lens)
    left = h.left()
    if left < 0:
        raise Bad('over-subscribed ' + what)
    if h.maxlen == 0:
        if kind == 'cl':
            raise Bad('empty ' + what)
        return h
    if left > 0 and (kind == 'cl' or h.maxlen != 1):
        raise Bad('incomplete ' + what)
    return h


def _new_census():
    return dict(blocks=[], max_dist=0, dists=set(), dist_ends=set(), lengths=set(), len258_284=0, len258_285=0,
                overlap=set(), straddle=0, start_at_wrap=0, end_at_wrap=0, lit_bits=set(), dist_bits=set(),
                single_dist_used=0, empty_dist_tree=0, eob_only_lit_tree=0, headers=[], rep16_cross=0,
                rep16=set(), rep17=set(), rep18=set(), stored=[], far_copies=set(), far_after_flush=set(),
                ref_into_stored=set(), flushes=0, copies=0, out_len=0)


class _Ring(object):
    """the flush points of the device's 32 KiB ring (KvqRingOut): before each write that would overwrite bytes not yet stored"""

    def __init__(self, c):
        self.f, self.c, self.since = 0, c, False

    def room(self, o, n):
        if o + n - self.f > WINDOW:
            self.f = o; self.c['flushes'] += 1; self.since = True


def inflate(payload, isize):
    """-> (ok, text or None, reason or None, census).  ok: the stream is valid up to its final block and gives exactly
    isize bytes (bytes behind the final block are ignored)"""
    c = _new_census()
    out, br = bytearray(), _Bits(payload)
    ring = _Ring(c)
    stored_spans = []
    cap = isize + 1
    try:
        last = 0
        while not last:
            last, kind = br.get(1), br.get(2)
            o0 = len(out)
            if kind == 3:
                raise Bad('block type 3')
            if kind == 0:
                br.pos = (br.pos + 7) & ~7
                ln, nln = br.get(16), br.get(16)
                if ln != nln ^ 0xFFFF:
                    raise Bad('stored length')
                b = br.pos >> 3
                if br.pos + 8 * ln > br.nbits:
                    raise Bad('truncated')
                c['stored'].append((o0, ln, c['blocks'][-1] if c['blocks'] else None))
                c['blocks'].append('stored')
                for a in range(0, ln, 4096):
                    ring.room(o0 + a, min(4096, ln - a))
                out += br.data[b:b + ln]
                br.pos += 8 * ln
                stored_spans.append((o0, o0 + ln))
                if len(out) > cap:
                    raise Bad('too long')
                continue
            if kind == 1:
                c['blocks'].append('fixed')
                lit, dist = _Huff(FIXED_LIT), _Huff(FIXED_DIST)
            else:
                c['blocks'].append('dynamic')
                nlen, ndist, ncode = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                c['headers'].append((nlen, ndist, ncode))
                if nlen > 286 or ndist > 30:
                    raise Bad('too many length or distance symbols')
                cl = [0] * 19
                for i in range(ncode):
                    cl[CL_ORDER[i]] = br.get(3)
                clh = _tree(cl, 'cl', 'code lengths set')
                lens = []
                while len(lens) < nlen + ndist:
                    sym, _ = br.decode(clh)
                    if sym < 16:
                        lens.append(sym)
                        continue
                    if sym == 16:
                        if not lens:
                            raise Bad('repeat with no first length')
                        v, r = lens[-1], 3 + br.get(2)
                        c['rep16'].add(r)
                        if len(lens) < nlen < len(lens) + r:
                            c['rep16_cross'] += 1
                    elif sym == 17:
                        v, r = 0, 3 + br.get(3)
                        c['rep17'].add(r)
                    else:
                        v, r = 0, 11 + br.get(7)
                        c['rep18'].add(r)
                    if len(lens) + r > nlen + ndist:
                        raise Bad('too many lengths')
                    lens += [v] * r
                if lens[256] == 0:
                    raise Bad('missing end-of-block')
                lit = _tree(lens[:nlen], 'lit', 'literal/length code')
                dist = _tree(lens[nlen:], 'dist', 'distance code')
                if sum(lit.count) == 1:
                    c['eob_only_lit_tree'] += 1
                if dist.maxlen == 0:
                    c['empty_dist_tree'] += 1
            single = sum(dist.count) == 1
            while True:
                sym, n = br.decode(lit)
                c['lit_bits'].add(n)
                if sym < 256:
                    ring.room(len(out), 1)
                    out.append(sym)
                    if len(out) > cap:
                        raise Bad('too long')
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    raise Bad('invalid literal/length code')
                s = sym - 257
                length = LEN_BASE[s] + br.get(LEN_EXTRA[s])
                if length == 258:
                    c['len258_284' if s == 27 else 'len258_285'] += 1
                ds, n = br.decode(dist)
                c['dist_bits'].add(n)
                if ds > 29:
                    raise Bad('invalid distance code')
                e = br.get(DIST_EXTRA[ds])
                d = DIST_BASE[ds] + e
                o = len(out)
                if d > o:
                    raise Bad('distance too far back')
                if single:
                    c['single_dist_used'] += 1
                c['lengths'].add(length)
                c['dists'].add(d)
                c['max_dist'] = max(c['max_dist'], d)
                if DIST_EXTRA[ds] == 0 or e == 0:
                    c['dist_ends'].add((ds, 'lo'))
                if DIST_EXTRA[ds] == 0 or e == (1 << DIST_EXTRA[ds]) - 1:
                    c['dist_ends'].add((ds, 'hi'))
                if d < length:
                    c['overlap'].add((d, length))
                if o // WINDOW != (o + length - 1) // WINDOW:
                    c['straddle'] += 1
                if o and o % WINDOW == 0:
                    c['start_at_wrap'] += 1
                if (o + length) % WINDOW == 0:
                    c['end_at_wrap'] += 1
                if d > WINDOW - 263:
                    c['far_copies'].add((o, d))
                    if ring.since:
                        c['far_after_flush'].add(d)
                ring.room(o, length)
                ring.since = False
                for a, z in stored_spans:
                    if a <= o - d and o - d + min(d, length) <= z:
                        c['ref_into_stored'].add(d)
                c['copies'] += 1
                for k in range(length):
                    out.append(out[o - d + k])
                if len(out) > cap:
                    raise Bad('too long')
    except Bad as e:
        c['out_len'] = len(out)
        return False, None, e.args[0], c
    c['out_len'] = len(out)
    if len(out) != isize:
        return False, None, 'isize', c
    return True, bytes(out), None, c


def far_tokens(data, window=WINDOW):
    """tokens of data that reach as far back as the window allows: at each position the earliest match of at least
    3 bytes no more than window bytes back, as long as it goes (at most 258), else a literal"""
    heads, toks, o, n = {}, [], 0, len(data)

    def insert(i):
        if i + 3 <= n:
            e = heads.get(data[i:i + 3])
            if e is None:
                heads[data[i:i + 3]] = [[i], 0]
            else:
                e[0].append(i)
    while o < n:
        e = heads.get(data[o:o + 3]) if o + 3 <= n else None
        if e:
            lst, k = e
            while k < len(lst) and lst[k] < o - window:
                k += 1
            e[1] = k
        if e and k < len(lst):
            p, ln, m = lst[k], 3, min(258, n - o)
            while ln < m and data[p + ln] == data[o + ln]:
                ln += 1
            toks.append((ln, o - p))
            for i in range(o, o + ln):
                insert(i)
            o += ln
        else:
            toks.append(data[o])
            insert(o)
            o += 1
    return toks
