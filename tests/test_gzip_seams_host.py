"""
CPU checks of the seam corpus (gzip_seams.py) of the gzip chunk decoder, DESIGN section 10: every
stream means what zlib makes of it (or fails in zlib as it is built to), the CPU run of the
chunked algorithm (kvq_inflate_gzip_host) agrees at every chunk size, every run goes through the
seams its stream was written for, and all runs together go through every class of seam.  The last
two are conditions on the corpus: test_gpu_gzip_seams.py runs the same streams through the kernels.
"""
import collections
import zlib

import pytest

import deflate_writer as W
import gzip_seams as S
import inflate_corpus as IC
from kvarq_amd import gzip_spec as G
from test_gzip_spec_host import check, host_reader

COUNTS = collections.Counter()               # over all the runs of this module
RUNS = set()


def run_host(st, cb):
    """the CPU run of stream st at chunk size cb equals zlib, a failure and its place included -> the seams it went through"""
    G.slot_canaries(256)
    try:
        if st.fail_block is None:
            assert host_reader(st.data) == st.text
            got, rep = G.inflate_host(st.data, cb)
            assert got == st.text
        else:
            with pytest.raises(zlib.error, match='too far back'):
                host_reader(st.data)
            with pytest.raises(G.GzipError) as ei:
                G.inflate_host(st.data, cb)
            assert (ei.value.status, ei.value.fpos) == (-3, st.table[st.fail_block]['out'])
        c = S.seams(st, G.last_chunks(), cb)
    finally:
        assert G.slot_canaries(0) == 0, 'a decode wrote outside its slot'
    missing = st.reaches[cb] - set(c)
    assert not missing, '%s at chunk size %d does not reach %s' % (st.name, cb, sorted(missing))
    return c


@pytest.mark.parametrize('name', list(S.FAMILIES))
def test_streams_equal_zlib_and_reach_their_seams(name):
    for st in S.family(name):
        assert st.table is None or len(st.data) < 300 << 10
        for cb in st.chunk_sizes:
            COUNTS.update(run_host(st, cb))
            RUNS.add((st.name, cb))


def test_every_seam_class_is_reached():
    """(behind the test above in the file: it counts what that one ran, and runs what it did not)"""
    for name in S.FAMILIES:
        for st in S.family(name):
            for cb in st.chunk_sizes:
                if (st.name, cb) not in RUNS:
                    COUNTS.update(run_host(st, cb))
                    RUNS.add((st.name, cb))
    print('seam counts over %d runs:' % len(RUNS))
    for k in S.CLASSES:
        print('  %-40s %d' % (k, COUNTS[k]))
    assert set(COUNTS) <= set(S.CLASSES)
    assert [k for k in S.CLASSES if COUNTS[k] < 1] == []


def test_model_sees_a_chunk_that_is_not_there():
    """a merged chunk shows: the counts of a run come from its own chunks"""
    st = S.family('resolve')[0]
    G.inflate_host(st.data, 1 << 20)
    assert G.last_report()['chunks'] == 1
    c = S.seams(st, G.last_chunks(), 1 << 20)
    assert not any(k.startswith('chunk_nsym') or k == 'short_chunk_hops' for k in c)


def test_build_reports_where_blocks_start():
    """deflate_writer.build(blocks, starts): a pair per block and one for the end, and the same bytes as without it"""
    blocks = [dict(kind='dynamic', tokens=list(b'ACGTTGCA' * 9) + [(30, 8)]), dict(kind='stored', data=b'xyz'), dict(kind='fixed', tokens=[65, (5, 1)])]
    st = []
    payload, text = W.build(blocks, st)
    assert (payload, text) == W.build(blocks) and zlib.decompress(payload, -15) == text
    assert len(st) == 4 and st[0] == (0, 0) and [o for _, o in st] == [0, 102, 105, 111]
    at = (st[1][0] + 3 + 7) >> 3                                  # the stored block: 3 bits, then LEN and NLEN on a byte boundary
    assert payload[at:at + 7] == b'\x03\x00\xfc\xffxyz' and st[2][0] == 8 * (at + 7)
    assert 8 * (len(payload) - 1) < st[3][0] <= 8 * len(payload)
    assert S._bits(blocks[0]) == st[1][0] and S._bits(blocks[2]) == st[3][0] - st[2][0]


INVALID = sorted(IC._edge_invalid_blocks().items())


@pytest.mark.parametrize('name,case', INVALID, ids=[n for n, _ in INVALID])
def test_invalid_blocks_behind_chunk_starts(name, case):
    """the streams of inflate_corpus.edge_invalid(), each behind valid dynamic blocks: the chunked run fails where zlib does
    (a few are valid, or merely cut short, behind other blocks: then the text is zlib's), the block in chunk 1 or later"""
    for tail in (b'', b'\xff' * 64):
        data = S.invalid_behind_valid(case[0], tail)
        check(data, 256)
        assert len(G.last_chunks()[1]) >= 2
