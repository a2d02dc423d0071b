"""
Seeded DEFLATE corpora for the BGZF inflate tests (tests/test_inflate_host.py on the CPU,
tests/test_gpu_inflate.py on the GPU): raw DEFLATE payloads of one BGZF member each, valid
ones made by zlib with every level and strategy, and corrupted ones, plus zlib's verdict
under the host reader's success rule (final block reached and exactly ISIZE bytes).
"""
import random
import struct
import zlib

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
        'far_refs': far + far,                                    # 64 KiB, back-references of 32 KiB
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
