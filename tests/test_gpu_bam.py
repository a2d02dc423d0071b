"""
BAM input on an MI355X: findseqs on a BAM equals findseqs and the oracle on its virtual FastQ text
(tests/bam_writer.to_fastq, the contract in plain Python), for the golden fixtures, a 20 k-read MTBC-shaped sample, a mixed
corpus, block and run layouts, a speculation adversary, several files and the error paths; the route's kernels alone
(bam.to_fastq_device) equal the host twin and the converter byte for byte; Analyser.scan(Bam(...), records=True) feeds
extract_hits.
"""
import ctypes as C
import gzip
import os
import threading
import time

import numpy as np
import pytest

import bam_writer as W
import cases
from kvarq_amd import _lib, analyse, bam, engine, synth
from kvarq_amd.bam import Bam
from oracle import oracle as O
from test_bam_host import chain_bait, corpus, mixed_records

pytestmark = pytest.mark.gpu


def _make(tmp_path, name, hdr, records, **kw):
    """the BAM file and a FastQ file of its virtual text"""
    p = str(tmp_path / (name + '.bam'))
    data = W.write(p, hdr, records, **kw)
    q = str(tmp_path / (name + '_virtual.fastq'))
    with open(q, 'wb') as f:
        f.write(W.to_fastq(data))
    return p, q


def _result(files, seqs, **kw):
    r = engine.findseqs(files, seqs, **kw)
    return r, engine.last_inflate()


def _same(a, b):
    """hits in order, hitseqs, records and every stat but total / progress"""
    assert tuple(a['hits']) == tuple(b['hits'])
    assert [bytes(h) for h in a['hitseqs']] == [bytes(h) for h in b['hitseqs']]
    sa, sb = dict(a['stats']), dict(b['stats'])
    for k in ('total', 'progress'):
        sa.pop(k), sb.pop(k)
    assert sa == sb
    assert a.get('records') == b.get('records')


def _three_way(bams, fqs, seqs, cfg):
    engine.config(**cfg)
    got, route = _result(bams, seqs, records=True)
    assert route == 'device_bam'
    want, r2 = _result(fqs, seqs, records=True)
    assert r2 == 'host'
    _same(got, want)
    o = O.findseqs(fqs, seqs, **cfg)
    assert tuple(got['hits']) == tuple(o['hits'])
    assert [bytes(h) for h in got['hitseqs']] == o['hitseqs']
    ost = dict(o['stats'])
    st = dict(got['stats'])
    for k in ('total', 'progress'):
        ost.pop(k), st.pop(k)
    assert st == ost
    assert _counters(bams, seqs) == _counters(fqs, seqs)
    return got


def _counters(files, seqs):
    """the whole counter array of a call through the C ABI, and its kvq_scan_path bit 6"""
    L = _lib.lib()
    bf = [f.encode() for f in files]
    farr = (C.c_char_p * len(bf))(*bf)
    bufs = [C.create_string_buffer(q, len(q) + 1) for q in seqs]
    sarr = (C.c_char_p * max(1, len(seqs)))(*[C.cast(q, C.c_char_p) for q in bufs])
    lens = (C.c_int32 * max(1, len(seqs)))(*[len(q) for q in seqs])
    h = L.kvq_findseqs_ex(farr, len(bf), sarr, lens, len(seqs), 0)
    try:
        assert h and _lib.last_error()[0] == 0, _lib.last_error()
        n = _lib.CTR_READLENGTHS + _lib.MAX_READLENGTH + 2 * len(seqs) + 7 * sum(len(q) for q in seqs)
        return np.ctypeslib.as_array(L.kvq_scan_counters(h), shape=(n,)).tolist()
    finally:
        L.kvq_findseqs_free(h)


GOLDEN = ['findseqs', 'paired', 'spoligo_analyser', 'spoligo_5k', 'spoligo_500_pair', 'synth20k_mtbc']


@pytest.mark.parametrize('name', GOLDEN)
def test_bam_equals_its_virtual_fastq_and_the_oracle(tmp_path, name):
    case = cases.by_name()[name]
    bams, fqs = [], []
    for k, p in enumerate(case.materialize(tmp_path)):
        with open(p, 'rb') as f:
            text = f.read()
        if p.endswith('.gz'):
            text = gzip.decompress(text)
        b, q = _make(tmp_path, '%s_%d' % (name, k), W.header(0), W.from_fastq(text, flag=0x4 | (0x40 << k if len(case.inputs) > 1 else 0)))
        bams.append(b); fqs.append(q)
    seqs = case.seq_bytes()
    got = _three_way(bams, fqs, seqs, case.config)
    assert got['stats']['records_parsed'] > 0


def test_mixed_corpus_device_equals_host_twin_and_converter(tmp_path):
    for name, data in sorted(corpus().items()):
        want = W.to_fastq(data)
        assert bam.to_fastq_host(data) == want, name
        for sb in (None, 1024, 4096):
            assert bam.to_fastq_device(data, sb) == want, (name, sb)
    rep = bam.last_report()
    assert rep['runs'] == 1 and rep['text_bytes'] == len(W.to_fastq(data))
    b, q = _make(tmp_path, 'mixed', W.header(3), mixed_records(n=400), block=5000)
    seqs = [b'ACGTACGTAC', b'GTTGCAACGT', b'NNNNN', b'ACGT' * 5]
    _three_way([b], [q], seqs, dict(cases.PRODUCT, minreadlength=5, minoverlap=5, Amin='!'))
    assert engine.last_bam_report()['records_noqual'] > 0


def test_layouts(tmp_path, monkeypatch):
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(cases.PRODUCT, nthreads=4)
    text = synth.reads(g, 0, 3000, 150).tobytes()
    recs = W.from_fastq(text)
    # records straddling blocks, one record per block
    sizes = np.cumsum([len(W.header(0))] + [len(r) for r in recs]).tolist()
    for name, kw in (('straddle', dict(block=1000)), ('per_record', dict(cuts=sizes))):
        b, q = _make(tmp_path, name, W.header(0), recs, **kw)
        _three_way([b], [q], seqs, cfg)
    # a 200 kb read over several blocks, a header over several blocks, a header-only BAM
    long_rec = W.record('long', 'ACGT' * 50000, [30] * 200000, flag=0x10)
    b, q = _make(tmp_path, 'long', W.header(0), recs[:50] + [long_rec] + recs[50:100])
    _three_way([b], [q], seqs, cfg)
    b, q = _make(tmp_path, 'bighead', W.header(30000, names=['c%06d' % i for i in range(30000)]), recs[:200])
    _three_way([b], [q], seqs, cfg)
    e, eq = _make(tmp_path, 'empty', W.header(5), [])
    r, route = _result([e], seqs)
    assert route == 'device_bam' and r['hits'] == () and r['stats']['records_parsed'] == 0 and r['stats']['parsed'] == 0
    # records and chunks straddling runs
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    big = W.from_fastq(synth.reads(g, 50000, 20000, 150).tobytes())
    b, q = _make(tmp_path, 'runs', W.header(0), big, block=30011)
    _three_way([b], [q], seqs, cfg)
    assert engine.last_bam_report()['runs'] > 2


def test_speculation_adversary(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_BAM_SEGMENT_KB', '1')
    g = synth.genome()
    recs = W.from_fastq(synth.reads(g, 100, 400, 150).tobytes())
    mixed = []
    for i, r in enumerate(recs):
        mixed.append(r)
        if i % 7 == 0:
            mixed += chain_bait(1)
    b, q = _make(tmp_path, 'bait', W.header(0), mixed)
    seqs = synth.both_strands(synth.table(g))
    _three_way([b], [q], seqs, dict(cases.PRODUCT, nthreads=4))
    rep = engine.last_bam_report()
    assert rep['refuted'] > 0 and rep['check_passes'] > rep['runs']
    with open(b, 'rb') as f:
        data = W.inflate(f.read())
    assert bam.to_fastq_device(data, 1024) == W.to_fastq(data)
    assert bam.last_report()['refuted'] > 0


def test_several_files_and_mixes(tmp_path):
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(cases.PRODUCT, nthreads=4)
    made = [_make(tmp_path, 'f%d' % k, W.header(k), W.from_fastq(synth.reads(g, 1000 * k, 1500, 150).tobytes(), flag=4 | 0x10 * k))
            for k in range(3)]
    for n in (2, 3):
        bams, fqs = [m[0] for m in made[:n]], [m[1] for m in made[:n]]
        cat = str(tmp_path / ('cat%d.fastq' % n))
        with open(cat, 'wb') as f:
            for q in fqs:
                f.write(open(q, 'rb').read())
        got = _three_way(bams, fqs, seqs, cfg)
        one, _ = _result([cat], seqs, records=True)
        _same(got, one)
    with pytest.raises(IOError, match='cannot scan BAM and FastQ files in one call'):
        engine.findseqs([made[0][0], made[1][1]], seqs)
    named = str(tmp_path / 'plain.bam')
    with open(named, 'wb') as f:
        f.write(open(made[0][1], 'rb').read())
    a, route = _result([named], seqs)
    assert route == 'host'
    _same(a, _result([made[0][1]], seqs)[0])


def test_errors(tmp_path):
    g = synth.genome()
    recs = W.from_fastq(synth.reads(g, 0, 2000, 150).tobytes())
    seqs = synth.both_strands(synth.table(g))
    engine.config(**cases.PRODUCT)
    p = str(tmp_path / 't.bam')
    W.write(p, W.header(0), recs, block=20000)
    blob = open(p, 'rb').read()
    cut = str(tmp_path / 'cut.bam')
    with open(cut, 'wb') as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(IOError, match='truncated BAM file'):
        engine.findseqs(cut, seqs)
    # a corrupt block_size in the middle
    hdr = W.header(0)
    k = len(recs) // 2 + 3
    at = len(hdr) + sum(len(r) for r in recs[:k])
    bad = recs[:k] + [b'\x14\x00\x00\x00' + recs[k][4:]] + recs[k + 1:]
    q = str(tmp_path / 'bad.bam')
    W.write(q, hdr, bad, block=7001)
    with pytest.raises(IOError) as e:
        engine.findseqs(q, seqs)
    assert str(e.value) == 'malformed BAM record : offset=%d' % at
    # a block that does not inflate: the message names its offset in the inflated stream
    blocks = W.bgzf(hdr + b''.join(recs), block=20000, eof=False)
    xlen = 6
    o, offs = 0, []
    while o < len(blocks):
        bsize = int.from_bytes(blocks[o + 16:o + 18], 'little') + 1
        offs.append(o); o += bsize
    third = offs[2]
    broken = bytearray(blocks + W.BGZF_EOF)
    broken[third + 12 + xlen: third + 12 + xlen + 8] = b'\xff' * 8
    r = str(tmp_path / 'noinf.bam')
    with open(r, 'wb') as f:
        f.write(bytes(broken))
    with pytest.raises(IOError) as e:
        engine.findseqs(r, seqs)
    assert 'error while inflating compressed data' in str(e.value) and str(e.value).endswith('fpos=%d' % 40000)


def test_analyser_extract_hits_stop_and_rescan(tmp_path, monkeypatch):
    g = synth.genome()
    text = synth.reads(g, 0, 20000, 150).tobytes()
    b, q = _make(tmp_path, 'an', W.header(0), W.from_fastq(text, flag=0x4 | 0x40))
    engine.config(**cases.PRODUCT)
    templates = {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}
    a = analyse.Analyser()
    a.scan(Bam(b, quiet=True), templates, records=True)
    assert len(a.hits) > 0 and len(a.records) == len(a.hits)
    out = tmp_path / 'bam.hits'
    a.extract_hits(str(out))
    # every written entry is one whole record of the converter's text
    lines = open(q, 'rb').read().split(b'\n')
    records = set(b'\n'.join(lines[i:i + 4]) + b'\n' for i in range(0, len(lines) - 4, 4))
    got = out.read_bytes().split(b'\n')
    entries = [b'\n'.join(got[i:i + 4]) + b'\n' for i in range(0, len(got) - 1, 4)]
    assert len(entries) == len(a.hits) and all(e in records for e in entries)
    f2 = analyse.Analyser()
    f2.scan(Bam(b, quiet=True), templates)
    with pytest.raises(IOError):
        f2.extract_hits(str(tmp_path / 'none.hits'))
    # stop() returns partial results
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    big_text = synth.reads(g, 0, 60000, 150).tobytes()
    bb, _ = _make(tmp_path, 'big', W.header(0), W.from_fastq(big_text), level=1)
    seqs = synth.both_strands(synth.table(g))
    e, _ = _make(tmp_path, 'empty', W.header(0), [])
    engine.findseqs(e, seqs)                                   # (the live stats start from nothing)
    res = {}

    def run():
        try:
            res['r'] = engine.findseqs(bb, seqs)
        except Exception as e:
            res['e'] = e
    th = threading.Thread(target=run)
    th.start()
    t0 = time.time()
    while th.is_alive() and time.time() - t0 < 60:
        if engine.stats()['records_parsed'] > 0:
            break
        time.sleep(0.0005)
    engine.stop()
    th.join()
    assert 'e' not in res, res.get('e')
    assert engine.last_inflate() == 'device_bam'
    part = res['r']
    full = engine.findseqs(bb, seqs)
    assert 0 < part['stats']['records_parsed'] < full['stats']['records_parsed'] == 60000
    assert 0 < part['stats']['parsed'] < full['stats']['parsed']
    assert tuple(full['hits'][:len(part['hits'])]) == tuple(part['hits'])
    # a small record store: the rescan gives the same records
    monkeypatch.setenv('KVQ_RECORD_CAP', '512')
    one = engine.findseqs(b, seqs, records=True)
    monkeypatch.delenv('KVQ_RECORD_CAP')
    two = engine.findseqs(q, seqs, records=True)
    _same(one, two)


def test_file_that_hands_over_nothing_between_files_of_several_runs(tmp_path, monkeypatch):
    """a header-only BAM hands no batch to the scan: the batch in flight keeps its text buffer"""
    monkeypatch.setenv('KVQ_INFLATE_BATCH_MB', '2')
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    cfg = dict(cases.PRODUCT, nthreads=4)
    a, aq = _make(tmp_path, 'a', W.header(0), W.from_fastq(synth.reads(g, 50000, 20000, 150).tobytes()), block=30011)
    b, bq = _make(tmp_path, 'b', W.header(0), W.from_fastq(synth.reads(g, 300000, 20000, 150).tobytes()), block=30011)
    e, eq = _make(tmp_path, 'e', W.header(5), [])
    for bams, fqs in (([a, e, b], [aq, eq, bq]), ([e, a, e], [eq, aq, eq])):
        _three_way(bams, fqs, seqs, cfg)
        assert engine.last_bam_report()['runs'] > 2
