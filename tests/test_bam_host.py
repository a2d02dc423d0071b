"""
BAM records as FastQ text on the CPU: the test writer against an independent
reader, and the library's host twin (kvq_bam_header_host, kvq_bam_to_fastq_host, the source the GPU
route shares) against the Python statement of the contract, tests/bam_writer.to_fastq, including
adversarial files and every rule a malformed record can break.
"""
import ctypes as C
import functools
import random
import struct

import pytest

import bam_writer as W
from kvarq_amd import _lib, bam


def mixed_records(seed=3, n=300, n_ref=3):
    """flags of every kind, cigars and aux of every type, IUPAC and '=' bases, absent qualities, l_seq 0, q 93 and 100"""
    rnd = random.Random(seed)
    flags = [0x4, 0x10, 0x40, 0x80, 0x100, 0x800, 0x200, 0x400, 0x4 | 0x10 | 0x40, 0x80 | 0x10, 0x40 | 0x80, 0x900, 0]
    out = []
    for i in range(n):
        ln = rnd.choice([0, 1, 2, 7, 50, 151, 300])
        seq = ''.join(rnd.choice('ACGT' * 6 + W.CODES) for _ in range(ln))
        qual = None if rnd.random() < 0.15 else [rnd.choice([0, 2, 30, 40, 93, 100, 222]) for _ in range(ln)]
        cig = [(rnd.randint(1, 50), rnd.randint(0, 8)) for _ in range(rnd.randint(0, 4))]
        aux = W.aux_all_types() if rnd.random() < 0.3 else b''
        ref = rnd.randint(-1, n_ref - 1)
        out.append(W.record('r%d:%s' % (i, 'x' * rnd.randint(0, 40)), seq, qual, flag=rnd.choice(flags), ref=ref,
                            pos=rnd.randint(-1, 10 ** 6), cigar=cig, next_ref=rnd.randint(-1, n_ref - 1),
                            next_pos=rnd.randint(-1, 5000), aux=aux))
    return out


def chain_bait(n=6):
    """records whose aux holds a B array of bytes that parse as a chain of >= 4 well-formed records"""
    fake = b''.join(W.record('fake%d' % i, 'ACGT' * 5, [30] * 20) for i in range(5))
    return [W.record('bait%d' % i, 'ACGTN' * 20, [35] * 100, aux=W.aux_b_bytes(fake * 3)) for i in range(n)]


@functools.lru_cache(None)
def corpus():
    """name -> inflated BAM stream"""
    return {
        'mixed': W.header(3) + b''.join(mixed_records(n_ref=3)),
        'unaligned': W.header(0) + b''.join(W.record('q%d' % i, 'ACGT' * 30, [30 + i % 10] * 120) for i in range(50)),
        'header_only': W.header(2),
        'big_header': W.header(4000, names=['contig_%05d_%s' % (i, 'y' * 20) for i in range(4000)]) +
                      b''.join(W.record('h%d' % i, 'ACGTTGCA' * 10, [20] * 80) for i in range(20)),
        'long_read': W.header(0) + W.record('long', ''.join(random.Random(5).choice('ACGT') for _ in range(200000)),
                                            [random.Random(6).randint(0, 60) for _ in range(200000)], flag=0x10),
        'bait': W.header(0) + b''.join(chain_bait()),
        'empty_seq': W.header(0) + b''.join(W.record('e%d' % i, '', []) for i in range(10)),
    }


def host_text(data):
    L = _lib.lib()
    n_ref = C.c_int32(0)
    first = L.kvq_bam_header_host(data, len(data), C.byref(n_ref))
    assert first >= 0
    consumed = C.c_int64(0)
    n = L.kvq_bam_to_fastq_host(data, len(data), n_ref.value, first, None, 0, C.byref(consumed))
    return n, first, n_ref.value, consumed.value


def test_writer_round_trips_through_the_independent_reader(tmp_path):
    recs = mixed_records(seed=11, n=120)
    p = str(tmp_path / 'm.bam')
    data = W.write(p, W.header(3), recs, cuts=[100, 5000, 5001, 20000])
    with open(p, 'rb') as f:
        assert W.inflate(f.read()) == data
    n_ref, got = W.read(data)
    assert n_ref == 3 and len(got) == len(recs)
    for r, blob in zip(got, recs):
        assert W.record(r['name'].decode(), r['seq'], r['qual'] if r['qual'][:1] != [0xFF] else None, flag=r['flag'],
                        ref=r['ref'], pos=r['pos'], mapq=r['mapq'], cigar=r['cigar'], next_ref=r['next_ref'],
                        next_pos=r['next_pos'], tlen=r['tlen'], aux=r['aux']) == blob


@pytest.mark.parametrize('name', sorted(corpus()))
def test_host_twin_equals_the_python_converter(name):
    data = corpus()[name]
    want = W.to_fastq(data)
    n, first, n_ref, consumed = host_text(data)
    assert (n_ref, first) == W.first_record(data)
    assert n == len(want) and consumed == len(data)
    assert bam.to_fastq_host(data) == want


def test_header_host_needs_the_whole_header_and_refuses_a_bad_one():
    h = W.header(50)
    L = _lib.lib()
    nr = C.c_int32(0)
    assert L.kvq_bam_header_host(h, len(h), C.byref(nr)) == len(h) and nr.value == 50
    assert L.kvq_bam_header_host(h, len(h) - 1, C.byref(nr)) == -2
    assert L.kvq_bam_header_host(b'BAM\x02' + h[4:], len(h), C.byref(nr)) == -1
    l_text, = struct.unpack_from('<i', h, 4)
    bad = h[:8 + l_text] + struct.pack('<i', -1) + h[12 + l_text:]          # n_ref = -1, every byte that is passed at hand
    assert L.kvq_bam_header_host(bad, len(bad), C.byref(nr)) in (-1, -2)


def _broken(field):
    """a stream of 5 good records whose third breaks one rule; returns (data, offset of the third)"""
    good = [W.record('g%d' % i, 'ACGT' * 10, [30] * 40) for i in range(5)]
    hdr = W.header(2)
    at = len(hdr) + len(good[0]) + len(good[1])
    r = bytearray(good[2])
    if field == 'l_read_name':
        r = bytearray(W.record('', 'ACGT' * 10, [30] * 40, raw_name=b'\x00'))
    elif field == 'name_char':
        r = bytearray(W.record('g 2', 'ACGT' * 10, [30] * 40))
    elif field == 'name_nul':
        r = bytearray(W.record('', 'ACGT' * 10, [30] * 40, raw_name=b'g2x'))
    elif field == 'ref':
        r[4:8] = struct.pack('<i', 2)
    elif field == 'ref_low':
        r[4:8] = struct.pack('<i', -2)
    elif field == 'next_ref':
        r[24:28] = struct.pack('<i', 5)
    elif field == 'pos':
        r[8:12] = struct.pack('<i', -2)
    elif field == 'next_pos':
        r[28:32] = struct.pack('<i', -7)
    elif field == 'l_seq':
        r[20:24] = struct.pack('<i', -1)
    elif field == 'block_size':
        r[0:4] = struct.pack('<i', 20)
    elif field == 'sizes':
        r[20:24] = struct.pack('<i', 41)              # l_seq one more than block_size holds
    elif field == 'past_end':
        return bytes(hdr + b''.join(good[:2]) + good[2][:-3]), at
    return bytes(hdr + good[0] + good[1] + bytes(r) + good[3] + good[4]), at


RULES = ['l_read_name', 'name_char', 'name_nul', 'ref', 'ref_low', 'next_ref', 'pos', 'next_pos', 'l_seq', 'block_size',
         'sizes', 'past_end']


@pytest.mark.parametrize('field', RULES)
def test_each_rule_gives_the_named_error_at_its_record(field):
    data, at = _broken(field)
    with pytest.raises(W.Malformed) as e:
        W.to_fastq(data)
    assert e.value.offset == at
    with pytest.raises(IOError) as e2:
        bam.to_fastq_host(data)
    assert str(e2.value) == 'malformed BAM record : offset=%d' % at


def test_is_bam_looks_at_the_bytes_not_the_name(tmp_path):
    p = str(tmp_path / 'x.fastq')
    W.write(p, W.header(0), [W.record('a', 'ACGT', [30] * 4)])
    assert bam.is_bam(p)
    q = str(tmp_path / 'y.bam')
    with open(q, 'wb') as f:
        f.write(b'@r\nACGT\n+\nIIII\n')
    assert not bam.is_bam(q)
    g = str(tmp_path / 'z.fastq.gz')
    with open(g, 'wb') as f:
        f.write(W.bgzf(b'@r\nACGT\n+\nIIII\n'))
    assert not bam.is_bam(g)
    assert bam.header(p)['n_ref'] == 0
