"""
A small BAM writer for the BAM tests and tools (SAM/BAM specification v1, sections 4.1-4.2), on
``struct`` and ``zlib`` with BGZF framing as tests/inflate_corpus.writer_bgzf makes it, the block cuts
under the caller's control (so that records can straddle blocks); an independent minimal reader; and
``to_fastq``, the plain-Python statement of the virtual FastQ text the tests
check the library against.
"""
import struct
import zlib

CODES = '=ACMGRSVTWYHKDBN'
COMP = dict(zip(CODES, '=TGKCYSBAWRDMHVN'))
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


# ---- writing -----------------------------------------------------------------------------------------------------

def header(n_ref=0, text=b'@HD\tVN:1.6\tSO:unknown\n', names=None, lengths=None):
    names = names or ['chr%d' % i for i in range(n_ref)]
    lengths = lengths or [1000 + i for i in range(n_ref)]
    out = [b'BAM\x01', struct.pack('<i', len(text)), text, struct.pack('<i', n_ref)]
    for nm, ln in zip(names, lengths):
        b = nm.encode() + b'\x00'
        out += [struct.pack('<i', len(b)), b, struct.pack('<i', ln)]
    return b''.join(out)


def pack_seq(seq):
    codes = [CODES.index(c) for c in seq]
    if len(codes) % 2:
        codes.append(0)
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))


def record(name, seq, qual=None, flag=4, ref=-1, pos=-1, mapq=255, cigar=(), next_ref=-1, next_pos=-1, tlen=0, aux=b'',
           bin_=4680, raw_name=None):
    """one record, block_size included.  name: str; seq: letters of CODES; qual: list of ints (None: absent, 0xFF);
    cigar: [(length, op)]"""
    nm = raw_name if raw_name is not None else name.encode() + b'\x00'
    q = bytes([0xFF] * len(seq)) if qual is None else bytes(qual)
    assert len(q) == len(seq)
    body = struct.pack('<iiBBHHHiiii', ref, pos, len(nm), mapq, bin_, len(cigar), flag, len(seq), next_ref, next_pos, tlen)
    body += nm + b''.join(struct.pack('<I', (ln << 4) | op) for ln, op in cigar) + pack_seq(seq) + q + aux
    return struct.pack('<i', len(body)) + body


def aux_all_types():
    """aux fields of every type: A c C s S i I f Z H and B arrays of every subtype"""
    out = [b'XAA' + b'x', b'XCc' + struct.pack('<b', -5), b'XDC' + struct.pack('<B', 200), b'XEs' + struct.pack('<h', -300),
           b'XFS' + struct.pack('<H', 60000), b'XGi' + struct.pack('<i', -70000), b'XHI' + struct.pack('<I', 4000000000),
           b'XIf' + struct.pack('<f', 1.5), b'XJZ' + b'hello world\x00', b'XKH' + b'1AE301\x00']
    for sub, fmt, vals in (('c', 'b', [-1, 2]), ('C', 'B', [1, 255]), ('s', 'h', [-2, 3]), ('S', 'H', [9, 65535]),
                           ('i', 'i', [-9, 7]), ('I', 'I', [1, 2]), ('f', 'f', [0.5, 2.0])):
        out.append(b'XLB' + sub.encode() + struct.pack('<i', len(vals)) + struct.pack('<%d%s' % (len(vals), fmt), *vals))
    return b''.join(out)


def aux_b_bytes(payload):
    """a B:C array that holds the given bytes"""
    return b'XBB' + b'C' + struct.pack('<i', len(payload)) + payload


def bgzf_block(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    payload = co.compress(data) + co.flush()
    hdr = struct.pack('<BBBBIBBH', 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b'BC' + struct.pack('<HH', 2, len(payload) + 25)
    return hdr + payload + struct.pack('<II', zlib.crc32(data) & 0xFFFFFFFF, len(data))


def bgzf(data, block=65280, cuts=None, level=6, eof=True):
    """BGZF members of `block` inflated bytes each, or cut at the given inflated offsets"""
    if cuts is None:
        cuts = list(range(block, len(data), block))
    edges = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    out = [bgzf_block(data[a:b], level) for a, b in zip(edges, edges[1:]) if b > a or len(data) == 0]
    return b''.join(out) + (BGZF_EOF if eof else b'')


def write(path, hdr, records, **kw):
    """writes header + records as BGZF; returns the inflated stream"""
    data = hdr + b''.join(records)
    with open(path, 'wb') as f:
        f.write(bgzf(data, **kw))
    return data


def from_fastq(text, flag=4):
    """unaligned records of a FastQ text's records: the identifier line without '@' up to its first blank (other
    characters outside '!'..'~' become '_'), the bases upper-cased (others 'N'), the qualities as Phred + 33"""
    lines = text.split(b'\n')
    out = []
    for i in range(0, len(lines) - 3, 4):
        ident, bases, qual = lines[i], lines[i + 1].rstrip(b'\r'), lines[i + 3].rstrip(b'\r')
        if not ident.startswith(b'@'):
            break
        nm = ident[1:].rstrip(b'\r').split(b' ')[0] or b'r%d' % i
        nm = bytes(c if 33 <= c <= 126 else 95 for c in nm)[:250].decode()
        seq = ''.join(c if c in CODES else 'N' for c in bases.decode('latin-1').upper())
        q = [max(0, min(93, c - 33)) for c in qual[:len(seq)]]
        q += [30] * (len(seq) - len(q))
        out.append(record(nm, seq, q if seq else [], flag=flag))
    return out


# ---- reading, independently of the library ---------------------------------------------------------------------

def inflate(blob):
    """the inflated stream of BGZF bytes, member by member"""
    out, o = [], 0
    while o < len(blob):
        xlen, = struct.unpack('<H', blob[o + 10:o + 12])
        bsize, = struct.unpack('<H', blob[o + 16:o + 18])
        out.append(zlib.decompress(blob[o + 12 + xlen:o + bsize + 1 - 8], -15))
        o += bsize + 1
    return b''.join(out)


def read(data):
    """(n_ref, [record dict]) of an inflated BAM stream"""
    assert data[:4] == b'BAM\x01'
    l_text, = struct.unpack('<i', data[4:8])
    o = 8 + l_text
    n_ref, = struct.unpack('<i', data[o:o + 4])
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack('<i', data[o:o + 4])
        o += 8 + l_name
    recs = []
    while o < len(data):
        bs, = struct.unpack('<i', data[o:o + 4])
        ref, pos, lrn, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack('<iiBBHHHiiii', data[o + 4:o + 36])
        p = o + 36
        name = data[p:p + lrn - 1]
        p += lrn
        cigar = [(v >> 4, v & 15) for v in struct.unpack('<%dI' % ncig, data[p:p + 4 * ncig])]
        p += 4 * ncig
        packed = data[p:p + (lseq + 1) // 2]
        p += (lseq + 1) // 2
        seq = ''.join(CODES[(packed[i // 2] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(lseq))
        qual = list(data[p:p + lseq])
        p += lseq
        recs.append(dict(offset=o, name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, cigar=cigar, seq=seq, qual=qual,
                         next_ref=nref, next_pos=npos, tlen=tlen, aux=data[p:o + 4 + bs]))
        o += 4 + bs
    return n_ref, recs


# ---- the contract ------------------------------------------------------------------------------------------------

class Malformed(Exception):
    def __init__(self, offset):
        super().__init__('malformed BAM record : offset=%d' % offset)
        self.offset = offset


def first_record(data):
    """(n_ref, offset of the first record)"""
    l_text, = struct.unpack('<i', data[4:8])
    o = 8 + l_text
    n_ref, = struct.unpack('<i', data[o:o + 4])
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack('<i', data[o:o + 4])
        o += 8 + l_name
    return n_ref, o


def to_fastq(data):
    """the virtual FastQ text of an inflated BAM stream; Malformed at the first record that breaks a rule"""
    n_ref, o = first_record(data)
    out = []
    while o < len(data):
        if o + 4 > len(data):
            raise Malformed(o)
        bs, = struct.unpack('<i', data[o:o + 4])
        if bs < 0 or o + 4 + bs > len(data) or bs < 32:
            raise Malformed(o)
        ref, pos, lrn, mapq, bin_, ncig, flag, lseq, nref, npos, tlen = struct.unpack('<iiBBHHHiiii', data[o + 4:o + 36])
        if lrn < 2 or not -1 <= ref < n_ref or not -1 <= nref < n_ref or pos < -1 or npos < -1 or lseq < 0:
            raise Malformed(o)
        if 32 + lrn + 4 * ncig + (lseq + 1) // 2 + lseq > bs:
            raise Malformed(o)
        name = data[o + 36:o + 36 + lrn]
        if name[-1] != 0 or any(c < 33 or c > 126 for c in name[:-1]):
            raise Malformed(o)
        s = o + 36 + lrn + 4 * ncig
        q = s + (lseq + 1) // 2
        if not flag & 0x900 and lseq > 0:
            bases = ''.join(CODES[(data[s + i // 2] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(lseq))
            if data[q] == 0xFF:
                quals = '"' * lseq
            else:
                quals = ''.join(chr((data[q + i] + 33) % 256) for i in range(lseq))
            if flag & 0x10:
                bases = ''.join(COMP[c] for c in reversed(bases))
                quals = quals[::-1]
            suffix = {0x40: '/1', 0x80: '/2'}.get(flag & 0xC0, '')
            out.append(b'@' + name[:-1] + suffix.encode() + b'\n' + bases.encode() + b'\n+\n' + quals.encode('latin-1') + b'\n')
        o += 4 + bs
    return b''.join(out)
