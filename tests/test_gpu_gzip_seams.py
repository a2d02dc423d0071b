"""
GPU checks of the gzip chunk decoder's kernels on the seam corpus of
gzip_seams.py -- streams zlib never emits, one family per test so that a failure names its seam:
the LDS ring's copies, stored runs and flush rule, the finder's rounds, the window walk over short
chunks, members, invalid blocks, a chunk longer than one pass of the replace grid.  Each run is the
comparison of test_gpu_gzip_spec (device == CPU twin == zlib: text, report, candidates, chunks,
canaries), and before it the seams are counted from the device run's own chunks: a chunk merged or
moved without notice fails there.  Then the window carried from run to run of findseqs(...,
inflate='device_any'), full and cut short by a member, against inflate='host'.
"""
import random
import zlib

import pytest

import cases
import deflate_writer as W
import gzip_seams as S
import inflate_corpus as IC
from kvarq_amd import engine, gzip_spec as G
from test_gpu_gzip_spec import _device, _same_as_host, _write
from test_gzip_spec_host import host_reader

pytestmark = pytest.mark.gpu


def _reaches(st, cb):
    """a check of the device run's chunks: they went through the seams st was written for"""
    def seen(chunks):
        missing = st.reaches[cb] - set(S.seams(st, chunks, cb))
        assert not missing, '%s at chunk size %d: the device run does not reach %s' % (st.name, cb, sorted(missing))
    return seen


def _fails_as_host(data, cb, seen=None):
    """the device run fails as the host run does: status, place and message, the held chunks, every slot between canaries"""
    G.slot_canaries(256)
    try:
        with pytest.raises(G.GzipError) as eh:
            G.inflate_host(data, cb)
        h_chunks = G.last_chunks()
        with pytest.raises(G.GzipError) as ed:
            _device(data, cb)
        d_chunks = G.last_chunks()
    finally:
        assert G.slot_canaries(0) == 0, 'a decode wrote outside its slot'
    if seen:
        seen(d_chunks)
    assert (ed.value.status, ed.value.fpos, str(ed.value)) == (eh.value.status, eh.value.fpos, str(eh.value))
    for a, b in zip(d_chunks, h_chunks):
        assert list(a) == list(b)
    return eh.value


def _family(name):
    for st in S.family(name):
        for cb in st.chunk_sizes:
            if st.fail_block is None:
                rep = _same_as_host(st.data, cb, seen=_reaches(st, cb))
                assert st.table is None or rep['chunks'] > 1
            else:
                with pytest.raises(zlib.error, match='too far back'):
                    host_reader(st.data)
                e = _fails_as_host(st.data, cb, seen=_reaches(st, cb))
                assert (e.status, e.fpos) == (-3, st.table[st.fail_block]['out'])


def test_ring_copies_over_their_own_sources_the_wrap_and_the_chunk_start():
    _family('ring_copies')


def test_ring_stored_runs_every_piece_size_across_the_wrap_and_read_back():
    _family('stored')


def test_ring_flush_rule_exactly_full_and_one_past():
    _family('flush')


def test_finder_round_seams_and_two_candidates_in_a_round():
    _family('finder')


def test_resolve_hops_over_short_chunks_and_chunk_sizes_around_the_window():
    _family('resolve')


def test_members_at_a_chunk_end_inside_a_chunk_and_references_at_their_first_byte():
    _family('members')


def test_replace_strides_over_a_chunk_longer_than_its_grid():
    _family('big_chunk')


def test_invalid_blocks_behind_chunk_starts_fail_as_on_the_host():
    for name, (blocks, _, _) in sorted(IC._edge_invalid_blocks().items()):
        for tail in (b'', b'\xff' * 64):
            data = S.invalid_behind_valid(blocks, tail)
            try:
                host_reader(data)
            except zlib.error:
                e = _fails_as_host(data, 256)
                assert e.status == -3, name
            else:
                _same_as_host(data, 256)
            assert len(G.last_chunks()[1]) >= 2, name


# ---- the window carried from run to run of findseqs(inflate='device_any') ----

SEQ = 'GATTACAGGCTTAACGTCCATGAGTTCAGC'
RUN = 512 << 10                              # compressed bytes of a run at KVQ_INFLATE_BATCH_MB=2
REC = 211                                    # bytes of a record of _period() but the first


def _period():
    """32 768 bytes of whole FastQ records, every read with SEQ in it; the first record's name padded to make it so"""
    rnd = random.Random(21)
    recs = []
    for i in range(155):
        at = rnd.randrange(0, 70)
        bases = ''.join(rnd.choice('ACGT') for _ in range(at)) + SEQ + ''.join(rnd.choice('ACGT') for _ in range(70 - at))
        quals = ''.join(rnd.choice('FGHI') for _ in range(100))
        recs.append(cases.rec('r%04d' % i + ('_' * 63 if i == 0 else ''), bases, quals))
    t = b''.join(recs)
    assert len(t) == 32768 and all(len(r) == REC for r in recs[1:])
    return t


def _carried_file(split, further=0):
    """a gzip file whose second run starts with a copy that reaches the whole window carried into it (and `further` bytes
    more): a dynamic block of literals (one period of the text), stored blocks up to the first block boundary past RUN -- split:
    the last 100 records of them a member of their own, so that the window is that short --, then dynamic blocks of copies
    alone, all from as far back as the window reaches -> (file bytes, text, the text the first run ends at, the window)"""
    T = _period()
    bounds = [32768 * m + b for m in range(12, 24) for b in range(274, 32769, REC)]      # where records end
    head = [dict(kind='dynamic', tokens=list(T), final=False)]
    st = []
    W.build(head, st)
    data0 = 10 + ((st[-1][0] + 3 + 7) >> 3) + 4                   # the file offset of the first stored block's payload

    def layout(r1, w):
        """a first run of r1 bytes of text -> (the stored blocks' sizes in member 1, the file offset of the last stored block's
        payload, its size)"""
        n1 = r1 - 32768 - (w if split else 0)
        sizes = [65535] * (n1 // 65535) + ([n1 % 65535] if n1 % 65535 else [])
        end = data0 + n1 + 5 * (len(sizes) - 1)
        return (sizes, end + 8 + 10 + 5, w) if split else (sizes, end - sizes[-1], sizes[-1])
    for k in range(100, len(bounds)):                               # the first record boundary whose last stored block ends past RUN
        r1 = bounds[k]
        w = r1 - bounds[k - 100] if split else 32768
        sizes, at, last = layout(r1, w)
        if at + last >= RUN + 64 and last > 1000:
            break
    assert at - 5 < RUN, 'the last stored block starts in the first run'
    piece = lambda a, n: (T * 4)[a % 32768:a % 32768 + n]
    blocks, o = head, 32768
    for n in sizes:
        blocks.append(dict(kind='stored', data=piece(o, n), final=False))
        o += n
    members = [blocks]
    if split:
        blocks[-1]['final'] = True
        members.append([dict(kind='stored', data=piece(o, w), final=False)])
        o += w
    assert o == r1
    ncopy = 6 * w if split else 258 * 520
    toks = [(258, w)] * (ncopy // 258) + ([(ncopy % 258, w)] if ncopy % 258 else [])
    toks[0] = (258, w + further)
    first_copy = len(members[-1])
    for i in range(0, len(toks), 200):
        members[-1].append(dict(kind='dynamic', tokens=toks[i:i + 200], final=i + 200 >= len(toks)))
    data, text = b'', b''
    for m in members:
        st = []
        raw, t = W.build(m, st)
        if m is members[-1]:
            # the first run ends where the stored blocks' sizes say: at the copies' first block, past RUN, the block in front of it not
            assert len(text) + st[first_copy][1] == r1
            assert (8 * (len(data) + 10) + st[first_copy][0]) >> 3 == at + last >= RUN
            assert (8 * (len(data) + 10) + st[first_copy - 1][0]) >> 3 < RUN
        data += S.gz_member(raw)
        text += t
    return data, text, r1, w


def _route(path, inflate):
    try:
        r = engine.findseqs(path, [SEQ.encode()], inflate=inflate, records=True)
        return ('ok', r['hits'], r['hitseqs'], r['stats'], r['records']), engine.last_inflate()
    except Exception as e:
        return ('err', type(e).__name__, str(e)), engine.last_inflate()


def _both_routes(tmp_path, name, data):
    p = _write(tmp_path, name, data)
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    host, h_route = _route(p, 'host')
    dev, d_route = _route(p, 'device_any')
    assert (h_route, d_route) == ('host', 'device_gzip')
    return host, dev


def test_first_copy_of_a_run_reaches_the_whole_carried_window(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')            # runs of 512 KiB compressed
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '32')
    data, text, r1, w = _carried_file(False)
    assert w == 32768 and host_reader(data) == text == (_period() * 30)[:len(text)] and len(text) == r1 + 258 * 520
    host, dev = _both_routes(tmp_path, 'full_window.fastq.gz', data)
    rep = engine.last_inflate_report()
    assert rep['runs'] >= 2 and rep['marker_symbols'] >= 32768, rep
    assert dev[0] == 'ok' and dev == host
    assert len(dev[4]) >= len(text) // (REC + 1)


def test_first_copy_of_a_run_reaches_a_carried_window_a_member_cut_short(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    monkeypatch.setenv('KVQ_GZIP_CHUNK_KB', '32')
    data, text, r1, w = _carried_file(True)
    assert w < 32768 and host_reader(data) == text and text[:r1] == (_period() * 30)[:r1] and text[r1:] == text[r1 - w:r1] * 6
    host, dev = _both_routes(tmp_path, 'short_window.fastq.gz', data)
    rep = engine.last_inflate_report()
    assert rep['runs'] >= 2 and rep['marker_symbols'] >= 6 * w, rep
    assert dev[0] == 'ok' and dev == host
    assert len(dev[4]) >= len(text) // (REC + 1)
    # one byte further back: in front of the member
    data, _, _, _ = _carried_file(True, further=1)
    with pytest.raises(zlib.error, match='too far back'):
        host_reader(data)
    host, dev = _both_routes(tmp_path, 'short_window_bad.fastq.gz', data)
    assert host[0] == dev[0] == 'err' and host[1] == dev[1] == 'OSError'
    pre = lambda m: m.rsplit(' fpos=', 1)[0]
    assert pre(dev[2]) == pre(host[2]) and 'status=-3' in dev[2]
