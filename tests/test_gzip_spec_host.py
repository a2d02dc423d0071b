"""
CPU checks of plain-gzip inflate by speculative chunk decoding through
kvq_inflate_gzip_host: the decoder source of kvq_inflate.h and the chunked algorithm of
kernels_gzip.hip that the GPU runs -- block finder, speculative decode with markers, chain check
with refutations and re-decodes, window resolution, marker replacement -- against zlib under the
host reader's rules (GzSerial in kvq_reader.hip): members crossed when more than 10 bytes follow
a final block, the next header searched within 10 bytes, a file cut short ends the text, no CRC32.
"""
import gzip
import random
import struct
import zlib

import pytest

import deflate_writer as W
import inflate_corpus as IC
from kvarq_amd import gzip_spec as G


def _skip_header(data, p, dist):
    """GzSerial::skip_gz_header on bytes: the byte behind the header, or None"""
    n = len(data)

    def getc():
        nonlocal p
        if p >= n:
            return -1
        p += 1
        return data[p - 1]
    state, y = 0, 0
    c = getc()
    while state != 2 and y <= dist and c != -1:
        if c == 0x1F and state == 0:
            state = 1
        elif c == 0x8B and state == 1:
            state = 2
        else:
            state, y = 0, y + 1
        c = getc()
    if state != 2 or c != 8:
        return None
    flags = getc()
    if flags & (0x02 | 0x20 | 0xC0):
        return None
    for _ in range(6):
        getc()
    if flags & 4:
        k = getc()
        k |= getc() << 8
        for _ in range(max(0, k)):
            getc()
    for f in (8, 16):
        if flags & f:
            c = getc()
            while c > 0:
                c = getc()
    return p


def host_reader(data):
    """what the host route's reader makes of a .gz file's bytes: text, or raises zlib.error"""
    p = _skip_header(data, 0, 0)
    assert p is not None, 'no gzip header at byte 0'
    out = []
    while True:
        d = zlib.decompressobj(-15)
        out.append(d.decompress(data[p:]))
        if not d.eof:
            return b''.join(out)                      # cut short: the text ends
        e = len(data) - len(d.unused_data)
        if len(data) - e <= 10:
            return b''.join(out)
        p = _skip_header(data, e, 10)
        if p is None:
            return b''.join(out)


def gz_member(raw, mtime=0):
    return b'\x1f\x8b\x08\x00' + struct.pack('<I', mtime) + b'\x00\xff' + raw + struct.pack('<II', 0, 0)


def check(data, chunk_bytes):
    """the chunked inflate equals the host reader, a failure included -> the report"""
    try:
        want = host_reader(data)
    except zlib.error:
        with pytest.raises(G.GzipError) as ei:
            G.inflate_host(data, chunk_bytes)
        assert ei.value.status == -3
        return G.last_report()
    got, rep = G.inflate_host(data, chunk_bytes)
    assert got == want
    return rep


TEXTS = {
    'fastq': IC.fastq_text(120000),
    'random': bytes(random.Random(3).getrandbits(8) for _ in range(50000)),
    'one_byte': b'G' * 150000,
}


@pytest.mark.parametrize('name', sorted(TEXTS))
@pytest.mark.parametrize('level', range(10))
def test_levels(name, level):
    z = gzip.compress(TEXTS[name], level)
    for cb in (1024, 8192, 1 << 24):
        check(z, cb)


@pytest.mark.parametrize('strategy', [s for _, s in IC.STRATEGIES], ids=[n for n, _ in IC.STRATEGIES])
@pytest.mark.parametrize('mem', [1, 9])
@pytest.mark.parametrize('wbits', [9, 12, 15])
def test_strategies_memlevels_windows(strategy, mem, wbits):
    co = zlib.compressobj(6, zlib.DEFLATED, -wbits, mem, strategy)
    raw = co.compress(TEXTS['fastq']) + co.flush()
    rep = check(gz_member(raw), 1024)
    assert rep['chunks'] >= 1


def test_chunks_report_markers_and_the_text_is_exact():
    z = gzip.compress(IC.fastq_text(400000), 6)
    rep = check(z, 4096)
    assert rep['runs'] == 1 and rep['chunks'] >= 2 and rep['marker_symbols'] > 0
    cand, starts, ends, nsym = G.last_chunks()
    assert len(starts) == rep['chunks']
    assert list(ends[:-1]) == list(starts[1:]), 'every chunk ends where the next one starts'
    assert ends[-1] == -1 and sum(nsym) == len(host_reader(z))


def test_members_concatenated_empty_and_inside_chunks():
    t = IC.fastq_text(90000)
    parts = [gzip.compress(t[:30000], 6), gzip.compress(b'', 6), gzip.compress(t[30000:31000], 1),
             gzip.compress(t[31000:], 9), gzip.compress(b'', 0)]
    z = b''.join(parts)
    for cb in (700, 2048, 1 << 20):
        check(z, cb)
    assert G.inflate_host(z, 2048)[0] == t


@pytest.mark.parametrize('tail', [b'', b'\0' * 8, b'x' * 10, b'y' * 11, b'\0' * 40, b'  \x1f\x8b\x08\x00' + b'\0' * 30])
def test_trailing_bytes(tail):
    z = gzip.compress(TEXTS['fastq'], 6) + tail
    check(z, 1024)


def test_member_header_within_ten_bytes_and_beyond():
    a, b = gzip.compress(b'A' * 5000), gzip.compress(b'B' * 5000)
    near, far = a + b'\0' * 2 + b, a + b'\0' * 3 + b              # the trailer is 8 of the 10 bytes the search may skip
    assert G.inflate_host(near, 512)[0] == host_reader(near) == b'A' * 5000 + b'B' * 5000
    assert G.inflate_host(far, 512)[0] == host_reader(far) == b'A' * 5000


@pytest.mark.parametrize('cut', [1, 7, 9, 100, 5000, 30001])
def test_truncated_stream_ends_the_text(cut):
    z = gzip.compress(TEXTS['fastq'], 6)
    check(z[:len(z) - cut], 1024)


def test_bgzf_file_decoded_as_plain_gzip():
    from test_host_logic import bgzf
    z = bgzf(IC.fastq_text(200000))
    check(z, 1024)
    check(z, 1 << 20)


def test_only_fixed_or_stored_blocks_find_no_candidates():
    t = IC.fastq_text(60000)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    for z in (gz_member(co.compress(t) + co.flush()), gzip.compress(t, 0)):
        rep = check(z, 1024)
        assert rep['chunks'] == 1 and rep['refuted'] == 0


def test_window_edge_members_joined_across_chunks():
    edge = IC.edge_valid()
    text = b''.join(t for _, _, t, _ in edge)
    # the whole text's far-reaching copies cut into many dynamic blocks: copies of up to 32 768 back cross the chunk starts
    toks = W.far_tokens(text)
    assert max(t[1] for t in toks if not isinstance(t, int)) == 32768
    blocks = [dict(kind='dynamic', tokens=toks[i:i + 3000]) for i in range(0, len(toks), 3000)]
    raw, got = W.build(blocks)
    assert got == text and len(blocks) > 4
    z = gz_member(raw)
    marks = 0
    for cb in (1024, 4096, 16384):
        marks += check(z, cb)['marker_symbols']
    assert marks > 0
    for _, payload, t, _ in edge:
        check(gz_member(payload), 256)


def _planted_stream():
    """stored blocks whose payload is a valid dynamic header with decodable data behind it, between real blocks"""
    rnd = random.Random(5)
    t = IC.fastq_text(30000)
    fake, _ = W.build([dict(kind='dynamic', tokens=list(b'ACGT' * 300), final=False)])
    blocks = []
    for i in range(0, len(t), 3000):
        blocks.append(dict(kind='dynamic', tokens=list(t[i:i + 3000]), final=False))
        blocks.append(dict(kind='stored', data=b'\x04' + fake + bytes(rnd.getrandbits(8) for _ in range(40)), final=False))
    blocks.append(dict(kind='fixed', tokens=list(b'\n'), final=True))
    raw, text = W.build(blocks)
    return gz_member(raw), text


def test_planted_false_positives_are_refuted():
    z, text = _planted_stream()
    seen = 0
    for cb in (256, 512, 1000, 1500):
        rep = check(z, cb)
        seen += rep['refuted']
        assert G.inflate_host(z, cb)[0] == text
    assert seen >= 1


def test_small_slots_overflow_and_are_decoded_again():
    z = gzip.compress(b'ACGT' * 200000, 9)                        # >300:1, far past the first slot guess
    rep = check(z, 64)
    assert rep['slot_overflows'] >= 1


@pytest.mark.parametrize('seed', range(40))
def test_corrupt_streams_fail_like_the_host_route(seed):
    rnd = random.Random(seed)
    z = bytearray(gzip.compress(IC.fastq_text(60000), rnd.choice([1, 6, 9])))
    for _ in range(rnd.randint(1, 4)):
        z[rnd.randrange(10, len(z) - 8)] ^= 1 << rnd.randrange(8)
    z = bytes(z)
    try:
        want = host_reader(z)
    except zlib.error:
        want = None
    for cb in (512, 1 << 20):
        if want is None:
            with pytest.raises(G.GzipError) as ei:
                G.inflate_host(z, cb)
            assert ei.value.status == -3
            assert str(ei.value).startswith('error while inflating compressed data : status=-3 fpos=')
        else:
            assert G.inflate_host(z, cb)[0] == want


def test_error_position_is_the_failing_blocks_output_start():
    t = IC.fastq_text(20000)
    good, _ = W.build([dict(kind='dynamic', tokens=list(t), final=False)])
    bad, _ = W.build([dict(kind='stored', data=b'abc', stored_nlen=0, final=True)])
    # (byte-aligned join: the first stream's last block ends on a byte boundary only by chance, so use a stored block to align)
    raw, _ = W.build([dict(kind='dynamic', tokens=list(t), final=False), dict(kind='stored', data=b'xy', final=False),
                      dict(kind='stored', data=b'abc', stored_nlen=0, final=True)])
    with pytest.raises(G.GzipError) as ei:
        G.inflate_host(gz_member(raw), 1 << 20)
    assert ei.value.status == -3 and ei.value.fpos == len(t) + 2
    assert good and bad


def test_no_header_at_byte_zero():
    with pytest.raises(IOError, match='no valid gzip header found at beginning of file : magic bytes not found'):
        G.inflate_host(b'\0' * 100, 1024)


def test_no_decode_writes_outside_its_slot():
    """every slot between canaries: refutations, overflowing slots, members, truncation and errors"""
    z, _ = _planted_stream()
    t = IC.fastq_text(90000)
    streams = [z, gzip.compress(b'ACGT' * 200000, 9), gzip.compress(t[:40000]) + gzip.compress(t[40000:], 1),
               gzip.compress(t, 6)[:-3000], gzip.compress(TEXTS['random'], 9)]
    G.slot_canaries(512)
    try:
        for data in streams:
            for cb in (64, 1024):
                check(data, cb)
    finally:
        assert G.slot_canaries(0) == 0

