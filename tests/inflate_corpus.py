"""
Seeded DEFLATE corpora for the BGZF inflate tests (tests/test_inflate_host.py on the CPU,
tests/test_gpu_inflate.py on the GPU): raw DEFLATE payloads of one BGZF member each, valid
ones made by zlib with every level and strategy, and corrupted ones, plus zlib's verdict
under the host reader's success rule (final block reached and exactly ISIZE bytes).
"""
import random
import struct
import zlib

import deflate_writer as _W

STRATEGIES = [('default', zlib.Z_DEFAULT_STRATEGY), ('fixed', zlib.Z_FIXED), ('huffman', zlib.Z_HUFFMAN_ONLY),
              ('rle', zlib.Z_RLE), ('filtered', zlib.Z_FILTERED)]


def fastq_text(n_bytes, seed=7):
    rnd = random.Random(seed)
    out, i, total = [], 0, 0
    while total < n_bytes:
        s = bytes(rnd.choice(b'ACGT') for _ in range(150))
        q = bytes(rnd.choice(b'#,:FFFF') for _ in range(150))
        rec = b'@read_%d/1\n%s\n+\n%s\n' % (i, s, q)
        out.append(rec); total += len(rec); i += 1
    return b''.join(out)[:n_bytes]


def texts():
    """name -> bytes, each at most 64 KiB"""
    rnd = random.Random(11)
    far = bytes(rnd.getrandbits(8) for _ in range(32768))
    return {
        'fastq': fastq_text(65536),
        'random': bytes(rnd.getrandbits(8) for _ in range(40000)),
        'one_byte': b'A' * 65536,                                 # distance 1, length 258
        'far_refs': far + far,                                    # 64 KiB of period 32 KiB: zlib writes it as literals
                                                                  # (no match of zlib's reaches 32 768 - 262); the copies
                                                                  # of 32 KiB are in edge_valid()'s far_refs_64k
        'short': b'@r\nACGT\n+\nIIII\n',
        'empty': b'',
    }


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    parts = []
    for i in range(0, len(data), flush_every):
        parts.append(co.compress(data[i:i + flush_every]) + co.flush(zlib.Z_FULL_FLUSH))
    return b''.join(parts) + co.flush()


def valid_corpus():
    """[(label, payload, text)] over texts x levels 0 1 6 9 x strategies, and members of several blocks"""
    out = []
    for name, t in sorted(texts().items()):
        for level in (0, 1, 6, 9):
            for sname, strat in STRATEGIES:
                out.append(('%s/l%d/%s' % (name, level, sname), deflate(t, level, strat), t))
        if len(t) > 4096:
            out.append(('%s/full_flush' % name, deflate(t, 6, flush_every=5000), t))
            out.append(('%s/full_flush_fixed' % name, deflate(t, 1, zlib.Z_FIXED, flush_every=3000), t))
    return out


def zlib_verdict(payload, isize):
    """(ok, bytes) as the host reader decides: the final block reached and exactly isize bytes"""
    d = zlib.decompressobj(-15)
    try:
        got = d.decompress(payload, isize) if isize > 0 else d.decompress(payload)
    except zlib.error:
        return False, None
    ok = d.eof and len(got) == isize
    return ok, (got if ok else None)


def corrupt_corpus(n=4000, seed=1951):
    """[(payload, isize)]: bit flips, truncations, forged stored lengths, forged ISIZE of valid members"""
    rnd = random.Random(seed)
    base = []
    t = fastq_text(16384, seed=3)
    rb = bytes(rnd.getrandbits(8) for _ in range(3000))
    for data in (t, t[:700], rb, b'A' * 5000, b'', t[:5000] + t[:5000]):
        for level in (0, 1, 6, 9):
            for _, strat in STRATEGIES:
                base.append((deflate(data, level, strat), len(data), level))
        base.append((deflate(data, 6, flush_every=1500), len(data), 6))
    out = []
    while len(out) < n:
        p, isize, level = rnd.choice(base)
        p = bytearray(p)
        kind = rnd.randrange(5)
        if kind <= 1 and p:                                   # flip 1-3 bits, often near the front (the headers)
            for _ in range(rnd.randint(1, 3)):
                at = rnd.randrange(min(len(p), 64)) if rnd.random() < 0.6 else rnd.randrange(len(p))
                p[at] ^= 1 << rnd.randrange(8)
        elif kind == 2 and p:                                 # truncate
            p = p[:rnd.randrange(len(p))]
        elif kind == 3 and level == 0 and len(p) >= 5:        # forge LEN or NLEN of the first stored block
            at = 1 + rnd.randrange(4)
            p[at] = rnd.getrandbits(8)
            if rnd.random() < 0.5:                            # ... consistently: LEN and NLEN agree, LEN is wrong
                ln = rnd.randrange(65536)
                p[1:5] = struct.pack('<HH', ln, ln ^ 0xFFFF)
        else:                                                 # forge ISIZE (or append bytes behind the final block)
            if rnd.random() < 0.3:
                p += bytes(rnd.getrandbits(8) for _ in range(rnd.randint(1, 9)))
            else:
                isize = max(0, min(65536, isize + rnd.choice([-100, -1, 1, 7, 4096])))
        out.append((bytes(p), isize))
    return out


def bgzf_parse(z):
    """the blocks of BGZF bytes by a plain walk of the format: [(offset, block bytes, isize)]"""
    out, off = [], 0
    while len(z) - off > 10:
        xlen, = struct.unpack_from('<H', z, off + 10)
        extra = z[off + 12:off + 12 + xlen]
        i, bsize = 0, None
        while i + 4 <= xlen:
            slen, = struct.unpack_from('<H', extra, i + 2)
            if extra[i:i + 2] == b'BC' and slen == 2:
                bsize = struct.unpack_from('<H', extra, i + 4)[0] + 1
            i += 4 + slen
        isize, = struct.unpack_from('<I', z, off + bsize - 4)
        out.append((off, bsize, isize))
        off += bsize
    return out


# ---- the structured corpus: members made by tests/deflate_writer.py, each built for edges zlib's encoder never reaches ----

def _lits(rnd, n, alphabet=None):
    return [rnd.choice(alphabet) if alphabet else rnd.getrandbits(8) for _ in range(n)]


def _chain(symbols):
    """code lengths 1, 2, ..., k-1, k-1 for the k symbols in order: a complete code whose last symbols are the longest"""
    lens = {}
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, len(symbols) - 1)
    return lens


def _lens(n, assign):
    out = [0] * n
    for s, v in assign.items():
        out[s] = v
    return out


# a complete code over all 286 literal/length and all 30 distance symbols whose length runs cross from one into the other
FULL_LIT = [9] * 256 + [6] * 28 + [5] * 2
FULL_DIST = [5] * 28 + [4] * 2


def _edge_valid_blocks():
    """name -> (blocks, features the member is built to hit: keys of EDGE_FEATURES)"""
    rnd = random.Random(1951)
    m = {}
    lit32k = _lits(rnd, 32768)
    # distances 32 506 ... 32 768 (32 768 is the whole window, the ring's size: source slot = destination slot)
    m['far_dists_at_32768'] = ([dict(kind='dynamic', tokens=lit32k + [(258, 32768)] + [(3, d) for d in range(32506, 32769)])],
                               ['dist_32768_at_32768', 'far_dists_all'])
    # 64 KiB of period 32 KiB, as copies of 32 KiB (what the far_refs text was meant to be); the last copy at 65 536 - 258
    m['far_refs_64k'] = ([dict(kind='dynamic', tokens=lit32k + [(258, 32768)] * 125 + [(130, 32768)] * 2 + [(258, 32768)])],
                         ['dist_32768_last_copy', 'end_at_wrap', 'isize_65536'])
    # the device ring flushes at the literal that reaches o = 32 768; the first copy behind it reaches back the whole window
    m['far_after_flush'] = ([dict(kind='dynamic', tokens=_lits(rnd, 32773) + [(258, 32768), (3, 32700), (200, 32767)])],
                            ['dist_32768_after_flush'])
    m['lengths_3_258'] = ([dict(kind='dynamic', tokens=_lits(rnd, 300) + [(n, 1 + n * 37 % 300) for n in range(3, 259)])],
                          ['lengths_all'])
    m['lengths_3_258_fixed'] = ([dict(kind='fixed', tokens=_lits(rnd, 300) + [(n, 1 + n * 53 % 300) for n in range(3, 259)])],
                                ['lengths_all'])
    ends = []
    for k, (base, extra) in enumerate(zip(_W.DIST_BASE, _W.DIST_EXTRA)):
        ends += [(3 + k % 7, base), (4 + k % 5, base + (1 << extra) - 1)]
    # every distance code at both ends of its extra bits, behind 32 KiB stored; the dynamic block uses the full tree:
    # HLIT 286, HDIST 30, HCLEN 19 (written out with trailing zeros), a 16 repeat from literal into distance lengths
    m['dist_code_ends'] = ([dict(kind='stored', data=bytes(_lits(rnd, 32768))),
                            dict(kind='dynamic', tokens=ends, lit_lens=FULL_LIT, dist_lens=FULL_DIST, hclen=19)],
                           ['dist_ends_all', 'header_max', 'rep16_cross', 'ref_into_stored_32768', 'stored_32768'])
    m['dist_code_ends_fixed'] = ([dict(kind='stored', data=bytes(_lits(rnd, 32768))), dict(kind='fixed', tokens=ends[::-1])],
                                 ['dist_ends_all'])
    alt = _lits(rnd, 300) + [(258, 100, 284), (258, 200), (258, 5, 284), (258, 1), (258, 1, 284), (258, 300, 284)]
    m['len258_dynamic'] = ([dict(kind='dynamic', tokens=alt)], ['len258_284', 'len258_285'])
    m['len258_fixed'] = ([dict(kind='fixed', tokens=alt)], ['len258_284', 'len258_285'])
    # overlapping copies below, at and above the 64-lane wave width
    m['overlap_1_65'] = ([dict(kind='dynamic', tokens=_lits(rnd, 65) + [(258, d, 284) if d % 3 == 0 else (258, d) for d in range(1, 66)])],
                         ['overlap_1_65'])
    m['wrap_end_then_start'] = ([dict(kind='dynamic', tokens=_lits(rnd, 32768 - 258) + [(258, 1000), (258, 700)] + _lits(rnd, 9))],
                                ['end_at_wrap', 'start_at_wrap'])
    m['wrap_straddle_far'] = ([dict(kind='fixed', tokens=_lits(rnd, 32768 - 100) + [(258, 5000)] + _lits(rnd, 3))], ['straddle'])
    m['wrap_straddle_overlap'] = ([dict(kind='dynamic', tokens=_lits(rnd, 32768 - 129) + [(258, 7), (258, 32768)])],
                                  ['straddle'])
    # stored blocks of 0, 1, 4095, 4096, 4097 bytes behind Huffman blocks at unaligned offsets, one across the ring wrap,
    # and copies into them from up to 32 KiB
    blocks = [dict(kind='fixed', tokens=_lits(rnd, 13)), dict(kind='stored', data=b''), dict(kind='stored', data=b'\x5a'),
              dict(kind='dynamic', tokens=_lits(rnd, 50) + [(20, 51)]), dict(kind='stored', data=bytes(_lits(rnd, 4095))),
              dict(kind='fixed', tokens=_lits(rnd, 3)), dict(kind='stored', data=bytes(_lits(rnd, 4096))),
              dict(kind='stored', data=bytes(_lits(rnd, 4097)))]
    o = 13 + 1 + 71 + 4095 + 3 + 4096 + 4097
    blocks.append(dict(kind='dynamic', tokens=[(258, 4097), (100, 4096 + 4097 + 258), (37, o - 13 + 258 + 100)]))
    o += 258 + 100 + 37
    blocks.append(dict(kind='fixed', tokens=_lits(rnd, 32768 - 2001 - o)))
    o = 32768 - 2001
    blocks.append(dict(kind='stored', data=bytes(_lits(rnd, 4097))))                  # [30 767, 34 864): across the wrap
    o += 4097
    s4096 = 13 + 1 + 71 + 4095 + 3                                                   # where the 4096-byte block starts
    blocks.append(dict(kind='dynamic', tokens=[(258, o - s4096 - 5000)] + [(258, 32768)] + [(3, 32768 - k) for k in range(5)]))
    m['stored_sizes'] = (blocks, ['stored_0', 'stored_1', 'stored_4095', 'stored_4096', 'stored_4097', 'stored_after_huffman',
                                  'stored_unaligned', 'stored_across_wrap', 'ref_into_stored_32768'])
    m['stored_65535'] = ([dict(kind='fixed', tokens=[0x41]), dict(kind='stored', data=bytes(_lits(rnd, 65535)))],
                         ['stored_65535', 'stored_after_huffman', 'stored_unaligned', 'stored_across_wrap', 'isize_65536'])
    # codes of 11..15 bits that the tokens use, past the decoder's 10-bit fast table; HCLEN 19 as the encoder gives it
    lsyms = [65, 67, 71, 84, 256, 257, 258, 259, 260, 97, 98, 99, 100, 262, 101, 285]
    dsyms = [4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    ll, dl = _chain(lsyms), _chain(dsyms)
    toks = _lits(rnd, 400, [65, 67, 71, 84])
    for i in range(200):
        toks.append(rnd.choice([97, 98, 99, 100, 101]))
        n = rnd.choice([3, 4, 5, 6, 8, 258])                # (symbols 257..260, 262, 285)
        ds = rnd.choice(dsyms[9:])
        toks.append((n, _W.DIST_BASE[ds] + rnd.randrange(1 << _W.DIST_EXTRA[ds])))
    m['long_codes'] = ([dict(kind='dynamic', tokens=toks, lit_lens=_lens(286, ll), dist_lens=_lens(30, dl), hlit=286, hdist=30)],
                       ['lit_codes_11_15', 'dist_codes_11_15', 'header_max'])
    # a distance code of a single 1-bit code (zlib's one incomplete code), used
    m['single_dist_code'] = ([dict(kind='dynamic', tokens=_lits(rnd, 20) + [(10, 7), (40, 8), (3, 7)], dist_lens=_lens(6, {5: 1}))],
                             ['single_dist_used'])
    m['empty_dist_tree'] = ([dict(kind='dynamic', tokens=_lits(rnd, 500), dist_lens=[0])], ['empty_dist_tree'])
    m['eob_only_lit_tree'] = ([dict(kind='fixed', tokens=_lits(rnd, 30)), dict(kind='dynamic', tokens=[], lit_lens=_lens(257, {256: 1}), dist_lens=[0]),
                               dict(kind='fixed', tokens=_lits(rnd, 5) + [(10, 30)])], ['eob_only_lit_tree'])
    # the smallest header a valid block has: HLIT 257, HDIST 1, HCLEN 5 (with HCLEN 4 every length is 0: edge_invalid)
    m['header_min'] = ([dict(kind='dynamic', tokens=_lits(rnd, 3000, list(range(1, 256))), lit_lens=[0] + [8] * 256, dist_lens=[0])],
                       ['header_min', 'empty_dist_tree'])
    # zero runs of 3, 10 (17) and 11, 138 (18) in the literal lengths; 16 runs of 3 and 6 in the distance lengths
    used = [0, 4, 15, 27, 166]
    rl = _lens(258, dict([(s, 3) for s in used] + [(256, 2), (257, 3)]))
    rd = [4] * 8 + [3] * 4
    m['rle_runs'] = ([dict(kind='dynamic', tokens=_lits(rnd, 40, used) + [(3, 1 + k) for k in range(12)] * 3, lit_lens=rl, dist_lens=rd)],
                     ['rep16_3', 'rep16_6', 'rep17_3', 'rep17_10', 'rep18_11', 'rep18_138'])
    # many blocks per member, fixed, dynamic and stored in turn (the tables rebuilt each time), to exactly 64 KiB
    blocks, o, k = [], 0, 0
    while o < 65536:
        kind = ('fixed', 'dynamic', 'stored')[k % 3]
        n = min(65536 - o, rnd.randint(1500, 5000))
        if kind == 'stored':
            blocks.append(dict(kind='stored', data=bytes(_lits(rnd, n))))
        else:
            toks, t = [], 0
            while t < n:
                if o + t > 300 and n - t >= 3 and rnd.random() < 0.3:
                    ln = min(n - t, rnd.choice([3, 17, 100, 258]))
                    toks.append((ln, rnd.randint(1, min(o + t, 32768))))
                    t += ln
                else:
                    toks.append(rnd.getrandbits(8)); t += 1
            blocks.append(dict(kind=kind, tokens=toks))
        o += n; k += 1
    m['alternating_64k'] = (blocks, ['blocks_alternate', 'isize_65536'])
    # random members: every block kind, copies of every reach
    for seed in range(6):
        r = random.Random(seed)
        blocks, o = [], 0
        for _ in range(r.randint(1, 6)):
            kind = r.choice(['fixed', 'dynamic', 'stored'])
            if kind == 'stored':
                n = min(65536 - o, r.choice([0, 1, 7, 300, 9000]))
                blocks.append(dict(kind='stored', data=bytes(_lits(r, n)))); o += n
                continue
            toks = []
            for _ in range(r.randint(0, 4000)):
                if o > 0 and r.random() < 0.4:
                    ln = r.randint(3, 258)
                    if o + ln > 65536:
                        break
                    toks.append((ln, r.randint(1, min(o, 32768)))); o += ln
                elif o < 65536:
                    toks.append(r.choice(b'ACGT@+\n#F')); o += 1
            blocks.append(dict(kind=kind, tokens=toks))
        m['random_%d' % seed] = (blocks, [])
    return m


def _small_dynamic(**kw):
    """a small valid dynamic block (literals and copies) with the fields in kw overriding"""
    rnd = random.Random(7)
    b = dict(kind='dynamic', tokens=_lits(rnd, 40, list(b'ACGT')) + [(10, 5), (30, 17), 65, (258, 1)])
    b.update(kw)
    return b


def _edge_invalid_blocks():
    """name -> (blocks, isize or None for the text's length, the reference inflater's reason)"""
    rnd = random.Random(4)
    m = {}
    m['hlit_287'] = ([_small_dynamic(hlit=287)], None, 'too many length or distance symbols')
    m['hlit_288'] = ([_small_dynamic(hlit=288)], None, 'too many length or distance symbols')
    m['hdist_31'] = ([_small_dynamic(hdist=31)], None, 'too many length or distance symbols')
    m['hdist_32'] = ([_small_dynamic(hdist=32)], None, 'too many length or distance symbols')
    # the lengths, their run-length form and the code-length code of the valid block, then bent
    _, _, _, _, lens_all, rle, cl, _ = _W.dynamic_header(_small_dynamic())
    assert sum(1 for v in cl if v) >= 3
    m['cl_incomplete'] = ([_small_dynamic(cl_lens=[4 if v else 0 for v in cl])], None, 'incomplete code lengths set')
    m['cl_oversubscribed'] = ([_small_dynamic(cl_lens=[1 if v else 0 for v in cl])], None, 'over-subscribed code lengths set')
    m['cl_all_zero'] = ([_small_dynamic(cl_lens=[0] * 19, hclen=19)], None, 'empty code lengths set')
    m['rep16_first'] = ([_small_dynamic(rle=[(16, 0)] + rle)], None, 'repeat with no first length')
    # a repeat one length past HLIT + HDIST
    m['rep16_past_end'] = ([_small_dynamic(rle=_W.rle_lengths(lens_all[:-2]) + [(16, 0)])], None, 'too many lengths')
    m['rep17_past_end'] = ([_small_dynamic(rle=_W.rle_lengths(lens_all[:-2]) + [(17, 0)])], None, 'too many lengths')
    m['rep18_past_end'] = ([_small_dynamic(rle=_W.rle_lengths(lens_all[:-10]) + [(18, 0)])], None, 'too many lengths')
    m['hclen_4'] = ([_small_dynamic(lit_lens=[0] * 257, dist_lens=[0], hclen=4)], None, 'missing end-of-block')
    m['lit_incomplete'] = ([dict(kind='dynamic', tokens=[65, 66, 65], lit_lens=_lens(257, {65: 2, 66: 2, 256: 2}), dist_lens=[0])],
                           None, 'incomplete literal/length code')
    m['lit_oversubscribed'] = ([dict(kind='dynamic', tokens=[65, 66, 65], lit_lens=_lens(257, {65: 1, 66: 1, 256: 1}), dist_lens=[0])],
                               None, 'over-subscribed literal/length code')
    m['dist_oversubscribed'] = ([_small_dynamic(dist_lens=[1, 1, 1, 2, 2, 2, 2, 2])], None, 'over-subscribed distance code')
    m['dist_incomplete'] = ([dict(kind='dynamic', tokens=_lits(rnd, 20) + [(10, 3), (4, 5), (7, 3)], dist_lens=[0, 0, 1, 0, 2])],
                            None, 'incomplete distance code')              # (every distance the tokens use has a code)
    m['eob_length_0'] = ([dict(kind='dynamic', tokens=[65, 66, 65], lit_lens=_lens(257, {65: 1, 66: 1}), dist_lens=[0])],
                         None, 'missing end-of-block')
    single = _lens(258, {65: 1, 256: 2, 257: 2})
    m['single_dist_code_unused_pattern'] = ([dict(kind='dynamic', tokens=[65, 65, ('sym', 257), ('bits', 1, 1)], lit_lens=single,
                                                  dist_lens=[1])], 3, 'invalid code')
    m['empty_dist_tree_then_length'] = ([dict(kind='dynamic', tokens=[65, 65, ('sym', 257), ('bits', 0, 5)], lit_lens=single,
                                              dist_lens=[0])], 3, 'invalid code')
    m['dist_o_plus_1_at_32767'] = ([dict(kind='dynamic', tokens=_lits(rnd, 32767) + [(3, 32768)])], None, 'distance too far back')
    m['dist_o_plus_1_at_32767_fixed'] = ([dict(kind='fixed', tokens=_lits(rnd, 32767) + [(258, 32768)])], None, 'distance too far back')
    m['copy_overruns_isize'] = ([dict(kind='dynamic', tokens=_lits(rnd, 100) + [(50, 60)])], 149, 'isize')
    m['copy_overruns_isize_across_wrap'] = ([dict(kind='fixed', tokens=_lits(rnd, 65536 - 257) + [(258, 32768)])], 65536, 'isize')
    m['stored_len_past_payload'] = ([dict(kind='fixed', tokens=[65, 66], final=False),
                                     dict(kind='stored', data=bytes(_lits(rnd, 100)), stored_len=101, stored_nlen=101 ^ 0xFFFF)],
                                    102, 'truncated')
    m['no_final_block'] = ([dict(kind='fixed', tokens=_lits(rnd, 100), final=False), dict(kind='stored', data=b'xyz', final=False)],
                           None, 'truncated')
    return m


EDGE_FEATURES = {
    'dist_32768_at_32768': lambda c: (32768, 32768) in c['far_copies'],
    'dist_32768_last_copy': lambda c: (65536 - 258, 32768) in c['far_copies'],
    'dist_32768_after_flush': lambda c: 32768 in c['far_after_flush'],
    'far_dists_all': lambda c: set(range(32506, 32769)) <= c['dists'],
    'lengths_all': lambda c: set(range(3, 259)) <= c['lengths'],
    'dist_ends_all': lambda c: len(c['dist_ends']) == 60,
    'len258_284': lambda c: c['len258_284'] > 0,
    'len258_285': lambda c: c['len258_285'] > 0,
    'overlap_1_65': lambda c: set((d, 258) for d in range(1, 66)) <= c['overlap'],
    'straddle': lambda c: c['straddle'] > 0,
    'start_at_wrap': lambda c: c['start_at_wrap'] > 0,
    'end_at_wrap': lambda c: c['end_at_wrap'] > 0,
    'stored_0': lambda c: any(n == 0 for _, n, _ in c['stored']),
    'stored_1': lambda c: any(n == 1 for _, n, _ in c['stored']),
    'stored_4095': lambda c: any(n == 4095 for _, n, _ in c['stored']),
    'stored_4096': lambda c: any(n == 4096 for _, n, _ in c['stored']),
    'stored_4097': lambda c: any(n == 4097 for _, n, _ in c['stored']),
    'stored_32768': lambda c: any(n == 32768 for _, n, _ in c['stored']),
    'stored_65535': lambda c: any(n == 65535 for _, n, _ in c['stored']),
    'stored_after_huffman': lambda c: any(p in ('fixed', 'dynamic') for _, _, p in c['stored']),
    'stored_unaligned': lambda c: any(o % 4 for o, n, _ in c['stored'] if n),
    'stored_across_wrap': lambda c: any(o < 32768 < o + n for o, n, _ in c['stored']),
    'ref_into_stored_32768': lambda c: 32768 in c['ref_into_stored'],
    'lit_codes_11_15': lambda c: set(range(11, 16)) <= c['lit_bits'],
    'dist_codes_11_15': lambda c: set(range(11, 16)) <= c['dist_bits'],
    'single_dist_used': lambda c: c['single_dist_used'] > 0,
    'empty_dist_tree': lambda c: c['empty_dist_tree'] > 0,
    'eob_only_lit_tree': lambda c: c['eob_only_lit_tree'] > 0,
    'header_min': lambda c: (257, 1, 5) in c['headers'],
    'header_max': lambda c: (286, 30, 19) in c['headers'],
    'rep16_cross': lambda c: c['rep16_cross'] > 0,
    'rep16_3': lambda c: 3 in c['rep16'],
    'rep16_6': lambda c: 6 in c['rep16'],
    'rep17_3': lambda c: 3 in c['rep17'],
    'rep17_10': lambda c: 10 in c['rep17'],
    'rep18_11': lambda c: 11 in c['rep18'],
    'rep18_138': lambda c: 138 in c['rep18'],
    'blocks_alternate': lambda c: len(c['blocks']) >= 12 and all(a != b for a, b in zip(c['blocks'], c['blocks'][1:]))
                                  and set(c['blocks']) == {'fixed', 'dynamic', 'stored'},
    'isize_65536': lambda c: c['out_len'] == 65536,
}


_EDGE = {}


def edge_valid():
    """[(name, payload, text, features)]: zlib and every decoder must inflate payload to exactly text"""
    if 'valid' not in _EDGE:
        _EDGE['valid'] = [(name, ) + _W.build(blocks) + (tuple(feats), ) for name, (blocks, feats) in sorted(_edge_valid_blocks().items())]
    return _EDGE['valid']


def edge_invalid():
    """[(name, payload, isize, reason)]: streams zlib must refuse (checked, never assumed), each built for one rule"""
    if 'invalid' not in _EDGE:
        out = []
        for name, (blocks, isize, reason) in sorted(_edge_invalid_blocks().items()):
            payload, text = _W.build(blocks)
            out.append((name, payload, len(text) if isize is None else isize, reason))
        _EDGE['invalid'] = out
    return _EDGE['invalid']


def writer_bgzf(text, block=60000):
    """text as a BGZF file whose members are written by tests/deflate_writer.py from far_tokens(): copies that reach up to
    the whole 32 KiB window, which zlib's encoder never writes.  -> (file bytes, the largest distance used)"""
    out, far = [], 0
    for i in range(0, len(text), block):
        chunk = text[i:i + block]
        toks = _W.far_tokens(chunk)
        far = max([far] + [t[1] for t in toks if not isinstance(t, int)])
        raw, got = _W.build([dict(kind='dynamic', tokens=toks)])
        assert got == chunk and len(raw) + 26 <= 65536
        out.append(b'\x1f\x8b\x08\x04\0\0\0\0\x00\xff' + struct.pack('<H', 6) + b'BC' + struct.pack('<HH', 2, len(raw) + 25) +
                   raw + struct.pack('<II', zlib.crc32(chunk), len(chunk)))
    out.append(bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000'))
    return b''.join(out), far


def libdeflate():
    """the system's libdeflate through ctypes, or None when it does not load"""
    import ctypes as C
    for name in ('libdeflate.so.0', 'libdeflate.so'):
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        L.libdeflate_alloc_compressor.restype = C.c_void_p
        L.libdeflate_alloc_compressor.argtypes = [C.c_int]
        L.libdeflate_deflate_compress.restype = C.c_size_t
        L.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.libdeflate_free_compressor.argtypes = [C.c_void_p]
        return L
    return None


def libdeflate_corpus():
    """[(label, payload, text)]: texts() raw-deflated by libdeflate at levels 1..12 (its matches reach the whole window),
    or None without libdeflate"""
    import ctypes as C
    L = libdeflate()
    if L is None:
        return None
    out = []
    for level in range(1, 13):
        c = L.libdeflate_alloc_compressor(level)
        assert c
        for name, t in sorted(texts().items()):
            cap = len(t) + len(t) // 8 + 64
            buf = C.create_string_buffer(cap)
            n = L.libdeflate_deflate_compress(c, t, len(t), buf, cap)
            assert n > 0
            out.append(('%s/libdeflate%d' % (name, level), buf.raw[:n], t))
        L.libdeflate_free_compressor(c)
    return out
