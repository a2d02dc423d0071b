"""
GPU checks of the BGZF device-inflate route: the inflate kernel (kvq_inflate_bgzf_device) against
zlib and against the host decoder on corrupt members, the device chunk cuts against
kvq_chunk_offsets, and findseqs(..., inflate='device') against inflate='host' (and the oracle) on
the same bgzip'ed files.  Every findseqs test asserts last_inflate(), so that a silent fall-back to
the host reader cannot pass.
"""
import ctypes as C
import gzip
import threading
import time

import numpy as np
import pytest

import cases
import inflate_corpus as IC
from kvarq_amd import _lib, bgzf as B, engine, scan, synth
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

BLOCK = np.dtype([('in_off', '<i8'), ('out_off', '<i8'), ('in_len', '<u4'), ('isize', '<u4')])     # kvq_bgzf_block


def _inflate_on_device(members, fill=0xAB):
    """members: [(payload, isize)] -> (statuses, [bytes of each member's output slot]).  Slot i is followed by a gap of
    i % 13 bytes (slots at every alignment) filled with `fill`; asserts that no member wrote into a gap, failing or not"""
    comp = b''.join(p for p, _ in members)
    n = len(members)
    in_len = np.array([len(p) for p, _ in members], np.int64)
    isize = np.array([i for _, i in members], np.int64)
    span = isize + np.arange(n, dtype=np.int64) % 13
    tab = np.zeros(n, BLOCK)
    tab['in_off'] = np.cumsum(in_len) - in_len
    tab['out_off'] = np.cumsum(span) - span
    tab['in_len'] = in_len
    tab['isize'] = isize
    o = int(span.sum())
    d_in, d_tab = scan.DeviceBuffer(max(1, len(comp))), scan.DeviceBuffer(tab.nbytes)
    d_out, d_st = scan.DeviceBuffer(max(1, o)), scan.DeviceBuffer(4 * n)
    d_in.upload(np.frombuffer(comp, np.uint8)) if comp else None
    d_tab.upload(tab.view(np.uint8))
    d_out.upload(np.full(max(1, o), fill, np.uint8))
    scan.inflate_bgzf_device(d_in.ptr, len(comp), d_tab.ptr, n, d_out.ptr, o, d_st.ptr)
    out = d_out.download()[:o]
    st = d_st.download().view(np.int32)[:n].tolist()
    for d in (d_in, d_tab, d_out, d_st):
        d.free()
    edge = np.zeros(o + 1, np.int64)                           # +1 over each slot, 0 over the gaps
    np.add.at(edge, tab['out_off'], 1)
    np.add.at(edge, tab['out_off'] + isize, -1)
    gap = np.cumsum(edge[:o]) == 0
    bad = np.flatnonzero(gap & (out != fill))
    assert bad.size == 0, 'member output outside its slot at byte %d' % bad[0]
    out = out.tobytes()
    return st, [out[int(a):int(a) + int(b)] for a, b in zip(tab['out_off'], isize)]


def test_inflate_kernel_equals_zlib_on_the_valid_corpus():
    corpus = IC.valid_corpus()
    st, got = _inflate_on_device([(p, len(t)) for _, p, t in corpus])
    for (label, _, t), s, g in zip(corpus, st, got):
        assert s == 0, label
        assert g == t, label


def test_inflate_kernel_mixed_good_and_corrupt_members():
    bad = IC.corrupt_corpus()
    good = [(p, len(t)) for _, p, t in IC.valid_corpus()]
    members = []
    for i, m in enumerate(bad):                               # good members between the corrupt ones
        members.append(m)
        if i % 40 == 0:
            members.append(good[(i // 40) % len(good)])
    want = [B.inflate_raw_host(p, isize) for p, isize in members]
    st, got = _inflate_on_device(members)
    assert st == [w[0] for w in want]
    for (p, isize), (s, w), g in zip(members, want, got):
        if s == 0:
            assert g == w
    assert sum(1 for s in st if s) > 1000


def test_entries_outside_the_buffers_are_refused():
    p = IC.deflate(b'@r\nACGT\n+\nIIII\n')
    tab = np.zeros(2, BLOCK)
    tab[0] = (0, 0, len(p), 15)
    tab[1] = (0, 10, len(p), 15)                              # output past the end of d_out
    d_in, d_tab, d_out, d_st = scan.DeviceBuffer(len(p)), scan.DeviceBuffer(tab.nbytes), scan.DeviceBuffer(16), scan.DeviceBuffer(8)
    d_in.upload(np.frombuffer(p, np.uint8)); d_tab.upload(tab.view(np.uint8))
    scan.inflate_bgzf_device(d_in.ptr, len(p), d_tab.ptr, 2, d_out.ptr, 16, d_st.ptr)
    assert d_st.download().view(np.int32).tolist() == [0, -2]
    assert d_out.download()[:15].tobytes() == b'@r\nACGT\n+\nIIII\n'


EDGE_VALID = IC.edge_valid()
EDGE_INVALID = IC.edge_invalid()


def test_inflate_kernel_on_the_structured_corpus():
    """the writer-made edges: distances up to the ring's 32 KiB, copies and stored blocks across its wrap, zlib's
    rules at the edges of the Huffman headers; statuses equal to the host decoder's, bytes equal to zlib's"""
    members = [(p, len(t)) for _, p, t, _ in EDGE_VALID] + [(p, isize) for _, p, isize, _ in EDGE_INVALID]
    want = [B.inflate_raw_host(p, isize)[0] for p, isize in members]
    st, got = _inflate_on_device(members)
    names = [m[0] for m in EDGE_VALID] + [m[0] for m in EDGE_INVALID]
    assert list(zip(names, st)) == list(zip(names, want))
    for (name, p, t, _), s, g in zip(EDGE_VALID, st, got):
        assert s == 0, name
        assert g == t == IC.zlib_verdict(p, len(t))[1], name
    assert all(s < 0 for s in st[len(EDGE_VALID):])


def test_inflate_kernel_second_member_of_a_workgroup():
    """the grid stops at 2^20 workgroups: a workgroup decodes member b and then member b + 2^20 over the ring and the
    tables b left.  The head holds the corpus reversed, then empty members (03 00, isize 0); the tail the corpus"""
    corpus = [(p, len(t)) for _, p, t, _ in EDGE_VALID] + [(p, isize) for _, p, isize, _ in EDGE_INVALID]
    k = len(corpus)
    members = corpus[::-1] + [(b'\x03\x00', 0)] * ((1 << 20) - k) + corpus
    want = [B.inflate_raw_host(p, isize)[0] for p, isize in corpus]
    st, got = _inflate_on_device(members)
    assert want[:len(EDGE_VALID)] == [0] * len(EDGE_VALID)
    assert st[:k] == want[::-1]
    assert not any(st[k:1 << 20]) and all(g == b'' for g in got[k:1 << 20])
    assert st[1 << 20:] == want
    for (p, isize), s, g in zip(corpus, st[1 << 20:], got[1 << 20:]):
        if s == 0:
            assert g == IC.zlib_verdict(p, isize)[1]


def test_inflate_kernel_on_libdeflate_members():
    corpus = IC.libdeflate_corpus()
    if corpus is None:
        pytest.skip('libdeflate does not load on this machine')
    st, got = _inflate_on_device([(p, len(t)) for _, p, t in corpus])
    for (label, _, t), s, g in zip(corpus, st, got):
        assert (s, g) == (0, t), label


def test_device_route_on_a_writer_made_bgzf_file(tmp_path):
    """FastQ text whose members copy from as far back as the 32 KiB window allows (distance 32 768 included):
    the device route equals the host route (zlib) and the oracle, hits in order, counters and stats"""
    t = cases.ragged(11, 2500, cases.RAGGED_TARGETS, maxlen=500)           # two 1 MiB chunks
    z, far = IC.writer_bgzf(t)
    assert far == 32768 and gzip.decompress(z) == t
    p = str(tmp_path / 'far.fastq.gz')
    open(p, 'wb').write(z)
    cfg = dict(cases.PRODUCT, nthreads=4)
    engine.config(**cfg)
    host, dev = _both([p], cases.RAGGED_SEQS)
    assert dev[0] == 'ok' and len(dev[1]) > 0
    assert dev == host
    o = O.findseqs([p], cases.RAGGED_SEQS, **cfg)
    assert tuple(dev[1]) == tuple(o['hits'])
    assert [bytes(h) for h in dev[2]] == o['hitseqs']
    assert dev[3] == o['stats']
    dev_flag, dev_ctr = _counters([p], cases.RAGGED_SEQS, engine.INFLATE_FLAGS['device'])
    host_flag, host_ctr = _counters([p], cases.RAGGED_SEQS, engine.INFLATE_FLAGS['host'])
    assert dev_flag and not host_flag
    assert dev_ctr.sum() > 0 and (dev_ctr == host_ctr).all()


def _device_cuts(text):
    L = _lib.lib()
    d = scan.DeviceBuffer(max(1, len(text)))
    if text:
        d.upload(np.frombuffer(text, np.uint8))
    cap = len(text) // (512 << 10) + 8
    out = np.zeros(cap + 1, np.int64)
    n = L.kvq_chunk_offsets_device(d.ptr, len(text), out.ctypes.data_as(C.POINTER(C.c_int64)), cap)
    d.free()
    return None if n < 0 else out[:n + 1].tolist()


def _host_cuts(text):
    arr = np.frombuffer(text, np.uint8)
    return scan.chunk_offsets(arr).tolist()


def test_device_chunk_cuts_equal_the_host_cuts():
    at_quals = b''.join(cases.rec('r%d' % i, 'ACGT' * 30, ('@' if i % 3 else '+') + 'I' * 119) for i in range(20000))
    plus_at = b''.join(cases.rec('r%d' % i, 'ACGT' * 30, '+@' * 60, plus='+r%d' % i) for i in range(20000))
    for text in (cases.multichunk(), at_quals, plus_at, cases.ragged(3, 20000, cases.RAGGED_TARGETS, nl='\r\n'),
                 cases.multichunk()[:(1 << 20)], cases.multichunk()[:(1 << 20) - 1], b'', b'@a\nA\n+\nI\n'):
        assert _device_cuts(text) == _host_cuts(text)


def _write_bgzf(tmp_path, name, data, **kw):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(bgzf(data, **kw))
    return p


def _run(files, seqs, inflate):
    try:
        r = engine.findseqs(files, seqs, inflate=inflate)
        return ('ok', r['hits'], r['hitseqs'], r['stats']), engine.last_inflate()
    except Exception as e:
        return ('err', type(e).__name__, str(e)), engine.last_inflate()


def _both(files, seqs):
    host, h_route = _run(files, seqs, 'host')
    dev, d_route = _run(files, seqs, 'device')
    assert h_route == 'host'
    assert d_route == 'device'
    return host, dev


GOLDEN = ['findseqs', 'paired', 'maxerror2', 'Amin_H', 'cover_hits', 'bad_at', 'bad_plus', 'spoligo_5k', 'spoligo_500_pair',
          'quirk', 'empty_file', 'partial_tail', 'long_reads', 'ragged', 'ragged_crlf', 'ragged_two_files', 'multichunk',
          'synth20k_mtbc', 'synth4k_300_barcodes']


@pytest.mark.parametrize('name', GOLDEN)
def test_device_route_equals_the_host_route_on_golden_cases(tmp_path, name):
    case = cases.by_name()[name]
    files = []
    for k, p in enumerate(case.materialize(tmp_path)):
        with open(p, 'rb') as f:
            data = f.read()
        if p.endswith('.gz'):
            data = gzip.decompress(data)
        files.append(_write_bgzf(tmp_path, '%s_%d.fastq.gz' % (name, k), data))
    engine.config(**case.config)
    host, dev = _both(files, case.seq_bytes())
    assert dev == host


def test_device_route_over_several_batches_equals_host_and_oracle(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')            # ~10 device batches, chunks carried across them
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    a = _write_bgzf(tmp_path, 'r_1.fastq.gz', synth.reads(g, 0, 40000, 150).tobytes(), level=1)
    b = _write_bgzf(tmp_path, 'r_2.fastq.gz', synth.reads(g, 90000, 30000, 150).tobytes(), level=6)
    cfg = dict(cases.PRODUCT, nthreads=8)
    engine.config(**cfg)
    host, dev = _both([a, b], seqs)
    assert dev == host and dev[0] == 'ok' and len(dev[1]) > 50
    o = O.findseqs([a, b], seqs, **cfg)
    assert tuple(dev[1]) == tuple(o['hits'])
    assert [bytes(h) for h in dev[2]] == o['hitseqs']
    assert dev[3] == o['stats']


def test_empty_bgzf_file_between_files_over_several_batches(tmp_path, monkeypatch):
    """a file whose text is empty hands no batch to the scan: the batch in flight keeps its text buffer"""
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    a = _write_bgzf(tmp_path, 'a.fastq.gz', cases.multichunk())
    e = _write_bgzf(tmp_path, 'e.fastq.gz', b'')
    b = _write_bgzf(tmp_path, 'b.fastq.gz', cases.ragged(9, 3000, cases.RAGGED_TARGETS), level=1)
    engine.config(**cases.PRODUCT)
    for files in ([a, e, b], [a, e, e, a], [e, a, e]):
        host, dev = _both(files, cases.MULTI_SEQS)
        assert dev[0] == 'ok' and dev == host


def _counters(files, seqs, flags):
    """the whole counter array (read lengths, hits per sequence, coverage, mutations) of a call through the C ABI"""
    L = _lib.lib()
    bf = [f.encode() for f in files]
    farr = (C.c_char_p * len(bf))(*bf)
    bufs = [C.create_string_buffer(q, len(q) + 1) for q in seqs]
    sarr = (C.c_char_p * len(seqs))(*[C.cast(q, C.c_char_p) for q in bufs])
    lens = (C.c_int32 * len(seqs))(*[len(q) for q in seqs])
    h = L.kvq_findseqs_ex(farr, len(bf), sarr, lens, len(seqs), flags)
    try:
        assert h and _lib.last_error()[0] == 0, _lib.last_error()
        n = _lib.CTR_READLENGTHS + _lib.MAX_READLENGTH + 2 * len(seqs) + 7 * sum(len(q) for q in seqs)
        return L.kvq_scan_path(h) & engine.PATH_DEVICE_INFLATE, np.ctypeslib.as_array(L.kvq_scan_counters(h), shape=(n,)).copy()
    finally:
        L.kvq_findseqs_free(h)


def test_device_route_counter_array_equals_the_host_route(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    files = [_write_bgzf(tmp_path, 'c_1.fastq.gz', synth.reads(g, 5000, 30000, 150).tobytes()),
             _write_bgzf(tmp_path, 'c_2.fastq.gz', synth.reads(g, 70000, 20000, 150).tobytes(), level=1)]
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    dev_flag, dev = _counters(files, seqs, engine.INFLATE_FLAGS['device'])
    host_flag, host = _counters(files, seqs, engine.INFLATE_FLAGS['host'])
    assert dev_flag and not host_flag
    assert dev.sum() > 0 and (dev == host).all()


def test_device_route_hit_arena_overflow_takes_the_rescan_pass(tmp_path):
    read = 'ACG' * 60
    data = cases.rec('x', read, 'I' * len(read)) * 40000        # 2.4M hits: more than the first arena holds
    p = _write_bgzf(tmp_path, 'acg.fastq.gz', data)
    engine.config(**dict(cases.DEFAULTS, minreadlength=10))
    host, dev = _both([p], [b'ACG'])
    assert dev[0] == 'ok' and len(dev[1]) == 40000 * 60
    assert dev == host


def test_a_plain_gz_or_plain_file_among_bgzf_takes_the_host_route(tmp_path):
    t = cases.ragged(8, 300, cases.RAGGED_TARGETS)
    a = _write_bgzf(tmp_path, 'a.fastq.gz', t)
    plain_gz = str(tmp_path / 'b.fastq.gz')
    open(plain_gz, 'wb').write(gzip.compress(t, mtime=0))
    plain = str(tmp_path / 'c.fastq')
    open(plain, 'wb').write(t)
    engine.config(**cases.PRODUCT)
    for files in ([a, plain_gz], [plain, a]):
        want, _ = _run(files, cases.RAGGED_SEQS, 'host')
        got, route = _run(files, cases.RAGGED_SEQS, 'device')
        assert route == 'host'
        assert got == want


def test_corrupt_block_raises_ioerror_naming_the_block(tmp_path):
    t = cases.multichunk()
    z = bytearray(bgzf(t))
    off, cs, isz = B.index(bytes(z))
    k = 5
    at = int(off[k]) + 18 + 3
    z[at] ^= 0xFF                                              # (inside the 6th block's payload, near its block header)
    p = str(tmp_path / 'bad.fastq.gz')
    open(p, 'wb').write(bytes(z))
    st, _ = B.inflate_raw_host(B.payload(bytes(z), off[k], cs[k]), isz[k])
    assert st != 0
    engine.config(**cases.PRODUCT)
    dev, route = _run([p], cases.MULTI_SEQS, 'device')
    assert route == 'device'
    assert dev[:2] == ('err', 'OSError')
    assert dev[2] == 'error while inflating compressed data : status=%d fpos=%d' % (st, int(isz[:k].sum()))
    host, _ = _run([p], cases.MULTI_SEQS, 'host')
    assert host[2].startswith('error while inflating compressed data : status=')


def test_no_record_start_in_a_chunk_gives_the_host_message(tmp_path):
    junk = (b'x' * 1000 + b'\n') * 3000                         # 3 MB without a record
    p = _write_bgzf(tmp_path, 'junk.fastq.gz', junk)
    engine.config(**cases.PRODUCT)
    host, dev = _both([p], cases.MULTI_SEQS)
    assert dev[0] == 'err' and dev == host
    assert 'could find beginning of record' in dev[2]


def test_stop_ends_a_device_route_call(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    data = cases.multichunk() * 30
    p = _write_bgzf(tmp_path, 'big.fastq.gz', data, level=1)
    engine.config(**dict(cases.PRODUCT, nthreads=4))
    empty = _write_bgzf(tmp_path, 'empty.fastq.gz', b'')
    engine.findseqs(empty, cases.MULTI_SEQS)                   # (the live stats start from nothing)
    out = {}

    def run():
        try:
            out['r'] = engine.findseqs(p, cases.MULTI_SEQS, inflate='device')
        except Exception as e:
            out['e'] = e
    th = threading.Thread(target=run)
    th.start()
    t0 = time.time()
    while th.is_alive() and time.time() - t0 < 60:
        if engine.stats()['records_parsed'] > 0:
            break
        time.sleep(0.0005)
    engine.stop()
    th.join()
    assert 'e' not in out, out.get('e')
    assert engine.last_inflate() == 'device'
    st = out['r']['stats']
    assert 0 < st['records_parsed'] < 9000 * 30
    assert 0 < st['parsed'] < len(data)
    full = engine.findseqs(p, cases.MULTI_SEQS, inflate='device')
    assert engine.last_inflate() == 'device'
    assert tuple(full['hits'][:len(out['r']['hits'])]) == tuple(out['r']['hits'])
