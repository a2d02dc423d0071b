"""
CPU checks of the library's raw-DEFLATE decoder (kvarq_amd/csrc/kvq_inflate.h, the code the GPU's
inflate kernel runs) through its host entry kvq_inflate_raw_host, and of the BGZF block index
kvq_bgzf_index: byte-exact against zlib on valid members, the same verdict as zlib under the host
reader's success rule on corrupted ones and on the structured corpus of tests/deflate_writer.py
(distances of the whole window, stored blocks across the ring wrap, zlib's rules at the edges of the
Huffman headers).  Every call's output slot lies between canary bytes that must stay untouched.
"""
import ctypes as C
import gzip

import pytest

import inflate_corpus as IC
from kvarq_amd import _lib, bgzf as B
from test_host_logic import bgzf

CANARY = 0xC5
PAD = 64


def _inflate_padded(payload, isize):
    """kvq_inflate_raw_host into an isize-byte slot with PAD canary bytes on both sides -> (status, bytes or None);
    asserts the canaries are untouched"""
    payload = bytes(payload)
    buf = C.create_string_buffer(bytes([CANARY]) * (isize + 2 * PAD), isize + 2 * PAD)
    st = _lib.lib().kvq_inflate_raw_host(payload, len(payload), C.addressof(buf) + PAD, isize)
    raw = buf.raw
    assert raw[:PAD] == bytes([CANARY]) * PAD and raw[PAD + isize:] == bytes([CANARY]) * PAD, 'write outside the slot'
    return st, (raw[PAD:PAD + isize] if st == B.Z_OK else None)


@pytest.mark.parametrize('label,payload,text', IC.valid_corpus(), ids=[c[0] for c in IC.valid_corpus()])
def test_valid_member_equals_zlib(label, payload, text):
    ok, want = IC.zlib_verdict(payload, len(text))
    assert ok and want == text
    st, got = _inflate_padded(payload, len(text))
    assert st == 0, (label, st)
    assert got == text


def test_trailing_bytes_behind_the_final_block_are_ignored():
    t = IC.fastq_text(20000)
    p = IC.deflate(t) + b'\x01\x02\x03garbage'
    assert IC.zlib_verdict(p, len(t)) == (True, t)
    assert B.inflate_raw_host(p, len(t)) == (0, t)


def test_output_must_be_exactly_isize():
    t = IC.fastq_text(5000)
    p = IC.deflate(t)
    assert B.inflate_raw_host(p, len(t) - 1)[0] == B.Z_BUF_ERROR         # would write past ISIZE
    assert B.inflate_raw_host(p, len(t) + 1)[0] == B.Z_BUF_ERROR         # ends short of ISIZE
    assert B.inflate_raw_host(p[:-1], len(t))[0] < 0                     # final block never reached
    assert B.inflate_raw_host(p, 65537)[0] == B.Z_STREAM_ERROR


@pytest.mark.parametrize('payload,why', [
    (bytes([0x07]), 'block type 3'),
    (bytes([0x01, 0x05, 0x00, 0xFA, 0xFE]) + b'x' * 5, 'stored LEN/NLEN mismatch'),
    (IC.deflate(b'abc', 6, IC.zlib.Z_FIXED)[:1] + b'\xff\xff\xff\xff', 'fixed block, symbols past 285'),
])
def test_hand_made_invalid_members(payload, why):
    assert IC.zlib_verdict(payload, 3)[0] is False, why
    assert B.inflate_raw_host(payload, 3)[0] < 0, why


def test_distance_too_far_back_and_distance_code_30():
    # fixed block: literal 'a', then length 3 at distance 2 (only one byte written) -> too far back
    def bits(fields):
        acc, n = 0, 0
        for v, w, rev in fields:
            if rev:
                v = int(format(v, '0%db' % w)[::-1], 2)
            acc |= v << n; n += w
        return acc.to_bytes((n + 7) // 8 + 1, 'little')
    lit_a = (0x30 + ord('a'), 8, True)
    len3 = (1, 7, True)                                                  # symbol 257
    eob = (0, 7, True)
    far = bits([(1, 1, False), (1, 2, False), lit_a, len3, (1, 5, True), eob])          # distance code 1 = distance 2
    ok_near = bits([(1, 1, False), (1, 2, False), lit_a, len3, (0, 5, True), eob])      # distance 1
    code30 = bits([(1, 1, False), (1, 2, False), lit_a, len3, (30, 5, True), eob])
    assert IC.zlib_verdict(ok_near, 4) == (True, b'aaaa')
    assert B.inflate_raw_host(ok_near, 4) == (0, b'aaaa')
    for p in (far, code30):
        assert IC.zlib_verdict(p, 4)[0] is False
        assert B.inflate_raw_host(p, 4)[0] == B.Z_DATA_ERROR


def test_corrupt_members_fail_exactly_when_zlib_fails():
    corpus = IC.corrupt_corpus()
    assert len(corpus) >= 4000
    n_bad = 0
    for i, (p, isize) in enumerate(corpus):
        ok, want = IC.zlib_verdict(p, isize)
        st, got = _inflate_padded(p, isize)
        assert (st == 0) == ok, (i, st, ok)
        if ok:
            assert got == want, i
        else:
            assert st in (B.Z_DATA_ERROR, B.Z_BUF_ERROR), (i, st)
            n_bad += 1
    assert 1000 < n_bad < len(corpus)                    # the corpus holds both kinds


EDGE_VALID = IC.edge_valid()
EDGE_INVALID = IC.edge_invalid()


@pytest.mark.parametrize('name,payload,text,features', EDGE_VALID, ids=[m[0] for m in EDGE_VALID])
def test_edge_valid_member_equals_zlib(name, payload, text, features):
    assert IC.zlib_verdict(payload, len(text)) == (True, text)
    assert _inflate_padded(payload, len(text)) == (B.Z_OK, text)
    assert B.inflate_raw_host(payload, len(text)) == (B.Z_OK, text)


@pytest.mark.parametrize('name,payload,isize,reason', EDGE_INVALID, ids=[m[0] for m in EDGE_INVALID])
def test_edge_invalid_member_fails_as_zlib_fails(name, payload, isize, reason):
    assert IC.zlib_verdict(payload, isize)[0] is False
    st, _ = _inflate_padded(payload, isize)
    assert st in (B.Z_DATA_ERROR, B.Z_BUF_ERROR), (name, st)
    if reason not in ('truncated', 'isize'):
        assert st == B.Z_DATA_ERROR, (name, st)              # the bits are no valid DEFLATE stream, not merely short


def test_edge_valid_member_one_byte_short_or_long_of_isize():
    for name, payload, text, _ in EDGE_VALID:
        if text:
            assert _inflate_padded(payload, len(text) - 1)[0] == B.Z_BUF_ERROR, name
        if len(text) < 65536:
            assert _inflate_padded(payload, len(text) + 1)[0] == B.Z_BUF_ERROR, name


def test_libdeflate_members_equal_zlib():
    corpus = IC.libdeflate_corpus()
    if corpus is None:
        pytest.skip('libdeflate does not load on this machine')
    for label, payload, text in corpus:
        assert IC.zlib_verdict(payload, len(text)) == (True, text), label
        assert _inflate_padded(payload, len(text)) == (B.Z_OK, text), label


def test_writer_made_bgzf_members_equal_zlib():
    import cases
    t = cases.ragged(11, 500, cases.RAGGED_TARGETS, maxlen=500)
    z, far = IC.writer_bgzf(t)
    assert far == 32768
    off, cs, isz = B.index(z)
    got = []
    for o, c, i in zip(off, cs, isz):
        st, b = _inflate_padded(B.payload(z, o, c), int(i))
        assert st == 0
        got.append(b)
    assert b''.join(got) == gzip.decompress(z) == t


def _files():
    t = IC.fastq_text(300000, seed=5)
    return {
        'blocks': bgzf(t),
        'small_blocks': bgzf(t[:50000], block=7000, level=1),
        'trailing': bgzf(t[:9000]) + b'\0' * 10,
        'tiny': bgzf(b'@tail\nACGT', block=7),
    }


@pytest.mark.parametrize('name', sorted(_files()))
def test_bgzf_index_agrees_with_a_walk_of_the_format(name):
    z = _files()[name]
    off, cs, isz = B.index(z)
    assert list(zip(off.tolist(), cs.tolist(), isz.tolist())) == IC.bgzf_parse(z)
    text = b''.join(B.inflate_raw_host(B.payload(z, o, c), i)[1] for o, c, i in zip(off, cs, isz))
    assert text == gzip.decompress(z)


def test_bgzf_index_refuses_what_is_not_bgzf_to_the_end():
    t = IC.fastq_text(20000)
    z = bgzf(t)
    assert B.index(gzip.compress(t, mtime=0)) is None                     # a plain gzip member
    assert B.index(bgzf(t[:9000])[:-28] + gzip.compress(t[9000:], mtime=0)) is None    # a plain member mid-file
    assert B.index(z + b'\0' * 11) is None                               # more than 10 trailing bytes
    assert B.index(z + b'\0' * 10) is not None
    assert B.index(z[:-30]) is None                                      # a block cut short
    assert B.index(b'') is None
