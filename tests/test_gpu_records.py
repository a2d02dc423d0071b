"""
The FastQ records of the hits (``findseqs(records=True)``, ``Scanner(records=True)``, ``Analyser.extract_hits``;
include/kvarq_hip.h), on an MI355X, against a host restatement of the definition: a hit's record is
the four-line record whose bases line holds its file_pos, raw bytes, identifier line to the quality line's newline
(to the end of the text when that newline is missing).  Every call is also compared with the same call without
records: hits, hit bytes, stats and counters must not change.
"""
import gzip
import os
import random

import numpy as np
import pytest

import cases
from kvarq_amd import _lib, analyse, engine, scan, synth
from kvarq_amd.fastq import Fastq
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu


def split_records(text, base=0):
    """(start, bases line start, bases line end, end) of every four-line record of one file's text at stream offset base"""
    lines, at = [], 0
    while at < len(text):
        e = text.find(b'\n', at)
        e = len(text) if e < 0 else e + 1
        lines.append((at, e)); at = e
    return [(base + lines[i][0], base + lines[i + 1][0], base + lines[i + 1][1], base + lines[min(i + 3, len(lines) - 1)][1])
            for i in range(0, len(lines) - 1, 4)]


def record_of(stream, file_pos, recs=None):
    """the record whose bases line holds file_pos (stream: the texts of the files; recs: split_records of all of them)"""
    for a, b0, b1, e in recs:
        if b0 <= file_pos < b1:
            return stream[a:e]
    raise AssertionError('no record holds file_pos %d' % file_pos)


def stream_of(files):
    texts = []
    for f in files:
        with (gzip.open(f, 'rb') if f.endswith('.gz') else open(f, 'rb')) as fd:
            texts.append(fd.read())
    recs, base = [], 0
    for t in texts:
        recs += split_records(t, base); base += len(t)
    return b''.join(texts), recs


def as_bytes(x):
    return x.encode('latin-1') if isinstance(x, str) else bytes(x)


def check_findseqs(files, seqs, inflate='host', route=None):
    """findseqs with records == without; every record == record_of; returns the result"""
    arg = files[0] if len(files) == 1 else files
    plain = engine.findseqs(arg, seqs, inflate=inflate)
    r = engine.findseqs(arg, seqs, inflate=inflate, records=True)
    if route:
        assert engine.last_inflate() == route
    assert r['hits'] == plain['hits'] and r['hitseqs'] == plain['hitseqs'] and r['stats'] == plain['stats']
    assert 'records' not in plain and len(r['records']) == len(r['hits'])
    stream, recs = stream_of(files)
    for h, rec in zip(r['hits'], r['records']):
        assert type(rec) is type(r['hitseqs'][0]) if r['hitseqs'] else True
        assert as_bytes(rec) == record_of(stream, h.file_pos, recs), h
    return r


FINDSEQS_CASES = ['findseqs', 'findseqs_gz', 'paired', 'paired_gz', 'maxerror2', 'cover_hits', 'spoligo_5k', 'spoligo_500_pair',
                  'quirk', 'partial_tail', 'blank_tail', 'long_reads', 'ragged', 'ragged_tiny', 'ragged_crlf', 'ragged_two_files',
                  'multichunk', 'multichunk_gz', 'synth4k_300_barcodes'] + ['forward_n%d_p%d_c%d' % (n, p, c) for n in (7, 133) for p in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize('name', FINDSEQS_CASES)
def test_every_record_is_the_one_whose_bases_line_holds_the_hit(tmp_path, name):
    case = cases.by_name()[name]
    files = case.materialize(tmp_path)
    engine.config(**case.config)
    r = check_findseqs(files, case.seq_bytes())
    if name not in ('partial_tail',):
        assert r['hits'], name


def test_extract_hits_writes_what_readrecordat_reads(tmp_path, fastqs):
    """single plain files: for every hit outside record 0 the entry extract_hits writes equals Fastq.readrecordat's (the
    reference's way); the whole file equals the one the fallback writes, but for hits in record 0"""
    for name in ('test_analyser.fastq', 'L3_N1014_hits_5k.fastq', 'N0116_1_hits_1k.fastq'):
        path = os.path.join(fastqs, name)
        fq = Fastq(path, variant='Sanger', quiet=True)
        engine.config(**cases.PRODUCT)
        templates = {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}
        a = analyse.Analyser()
        a.scan(fq, templates, records=True)
        assert a.records is not None and len(a.records) == len(a.hits) > 0
        with open(path, 'rb') as f:                              # (the end of record 0's bases line)
            first_bases_end = len(f.readline()) + len(f.readline())
        out = tmp_path / (name + '.hits')
        a.extract_hits(str(out))
        got = out.read_bytes()
        entries = [analyse.format_record(rec) for rec in a.records]
        assert got == b''.join(entries)
        n_checked = 0
        for h, e in zip(a.hits, entries):
            if h.file_pos >= first_bases_end:
                assert e == fq.readrecordat(h).encode('latin-1'), h
                n_checked += 1
        assert n_checked > 0


def test_hit_in_the_first_record_gets_that_record(tmp_path):
    r1 = cases.rec('first', cases.QUIRK_SEQ, 'I' * 51)
    r2 = cases.rec('second', 'T' * 60, 'I' * 60)
    p = tmp_path / 'first.fastq'; p.write_bytes(r1 + r2 + r1.replace(b'first', b'third'))
    engine.config(**dict(cases.PRODUCT, Amin='!'))
    r = check_findseqs([str(p)], [cases.QUIRK_SEQ.encode()])
    assert [h.file_pos for h in r['hits']] == [7, len(r1) + len(r2) + 7]
    assert r['records'] == [r1, r1.replace(b'first', b'third')]


def test_hit_in_the_mate_file_gets_the_mates_record(tmp_path):
    a = cases.rec('m1/1', 'T' * 60, 'I' * 60) + cases.rec('m2/1', 'G' * 60, 'I' * 60)
    b = cases.rec('m1/2', 'A' * 5 + cases.QUIRK_SEQ, 'I' * 56) + cases.rec('m2/2', cases.QUIRK_SEQ + 'C' * 9, 'I' * 60)
    (tmp_path / 'p_1.fastq').write_bytes(a); (tmp_path / 'p_2.fastq').write_bytes(b)
    engine.config(**dict(cases.PRODUCT, Amin='!'))
    r = check_findseqs([str(tmp_path / 'p_1.fastq'), str(tmp_path / 'p_2.fastq')], [cases.QUIRK_SEQ.encode()])
    m1 = cases.rec('m1/2', 'A' * 5 + cases.QUIRK_SEQ, 'I' * 56); m2 = b[len(m1):]
    assert len(r['hits']) == 2 and all(h.file_pos >= len(a) for h in r['hits'])
    assert r['records'] == [m1, m2]
    # extract_hits: the mate's record (the reference reads past the end of the first file)
    an = analyse.Analyser()
    an.scan(Fastq(str(tmp_path / 'p_1.fastq'), variant='Sanger', paired=True, quiet=True), {'q': cases.QUIRK_SEQ}, do_reverse=False, records=True)
    out = tmp_path / 'mate.hits'; an.extract_hits(str(out))
    assert out.read_bytes() == m1 + m2


def test_last_record_without_a_trailing_newline(tmp_path):
    """the reader drops a last record whose quality line has no newline (no hit comes from it, as in the reference); the
    hit in the record in front of it gets its own record, not the tail behind it -- through findseqs and a device batch"""
    r1 = cases.rec('a', 'T' * 60, 'I' * 60)
    r2 = b'@hit\r\n' + cases.QUIRK_SEQ.encode() + b'\r\n+\r\n' + b'I' * 51 + b'\r\n'
    last = b'@z\n' + cases.QUIRK_SEQ.encode() + b'\n+\n' + b'I' * 51
    p = tmp_path / 'nonl.fastq'; p.write_bytes(r1 + r2 + last)
    engine.config(**dict(cases.PRODUCT, Amin='!'))
    r = check_findseqs([str(p)], [cases.QUIRK_SEQ.encode()])
    assert r['records'] == [r2]
    arr = np.frombuffer(r1 + r2 + last, dtype=np.uint8)
    t = scan.Table([cases.QUIRK_SEQ.encode()], **dict(cases.PRODUCT, Amin='!'))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b, _, _ = _scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr)))
    assert b['records'] == [r2]
    d.free(); t.close()
    assert analyse.format_record(r2) == b'@hit\n' + cases.QUIRK_SEQ.encode() + b'\n+\n' + b'I' * 51 + b'\n'


def test_the_three_inflate_routes_agree_byte_for_byte(tmp_path):
    case = cases.by_name()['multichunk']
    text = cases.multichunk()
    engine.config(**case.config)
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
    seqs = case.seq_bytes()
    host = check_findseqs([str(tmp_path / 'm.fastq')], seqs, 'host', 'host')
    dev = check_findseqs([str(tmp_path / 'b.fastq.gz')], seqs, 'device', 'device')
    anyg = check_findseqs([str(tmp_path / 'g.fastq.gz')], seqs, 'device_any', 'device_gzip')
    assert host['records'] == dev['records'] == anyg['records'] and len(host['records']) > 100


def _scanner_pair(t, feed, force=False):
    """(result without records, result with records, hit_arrays with records) of the same feeding"""
    out = []
    for rec in (False, True):
        s = scan.Scanner(t, records=rec)
        if force:
            s.force_exhaustive()
        feed(s)
        r = s.finish()
        out.append(r)
        if rec:
            out.append(s.hit_arrays())
            out.append(_lib.lib().kvq_scan_record_bytes(s.h))
        s.close()
    a, b = out[0], out[1]
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all()
    assert 'records' not in a
    return out


def _check_records(r, text, recs, base=0):
    for h, rec in zip(r['hits'], r['records']):
        assert rec == record_of(text, h.file_pos - base, recs), h


def test_scanner_device_batches_and_host_batches_split_at_a_record(monkeypatch):
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    host = synth.reads(g, 0, 40000, 150)
    text = host.tobytes(); recs = split_records(text)
    t = scan.Table(seqs, **cases.PRODUCT)
    d = scan.DeviceBuffer(host.nbytes); d.upload(host)
    co = scan.chunk_offsets(host)
    a, b, arrs, nbytes = _scanner_pair(t, lambda s: s.scan_device(d.ptr, host.nbytes, co))
    assert len(b['hits']) > 50
    _check_records(b, text, recs)
    # stored once per read: the store holds the distinct records, nothing more
    distinct = {h.file_pos: rec for h, rec in zip(b['hits'], b['records'])}
    assert nbytes == sum(len(x) for x in distinct.values()) == arrs['record_blob'].nbytes
    assert [bytes(arrs['record_blob'][o:o + n]) for o, n in zip(arrs['record_off'], arrs['record_len'])] == b['records']
    half = int(co[len(co) // 2])
    a2, b2, _, _ = _scanner_pair(t, lambda s: (s.scan_host(host[:half]), s.scan_host(host[half:], fpos_base=half)))
    assert b2['hits'] == b['hits'] and b2['records'] == b['records']
    # force_exhaustive
    a3, b3, _, _ = _scanner_pair(t, lambda s: s.scan_device(d.ptr, host.nbytes, co), force=True)
    assert b3['path']['exhaustive'] and not b3['path']['seeded']
    assert b3['hits'] == b['hits'] and b3['records'] == b['records']
    # KVQ_SURV_CAP=0: every survivor verified in place
    monkeypatch.setenv('KVQ_SURV_CAP', '0')
    a4, b4, _, _ = _scanner_pair(t, lambda s: s.scan_device(d.ptr, host.nbytes, co))
    assert b4['hits'] == b['hits'] and b4['records'] == b['records']
    d.free(); t.close()


def test_speculation_failure_and_long_records_through_the_redo():
    rng = random.Random(99)
    target = cases.QUIRK_SEQ
    recs_ = []
    for i in range(4000):
        bases = cases.randseq(rng, rng.randint(60, 200))
        if i % 7 == 0:
            bases = '@' + bases[1:]
        if i % 11 == 0:
            bases = '+' + bases[1:]
        if i % 5 == 0:
            at = rng.randint(1, len(bases) - 1)
            bases = (bases[:at] + target)[:230]
        q = ''.join(rng.choice('@+IIII') for _ in bases)
        recs_.append(cases.rec('r%d' % i, bases, q))
    data = np.frombuffer(b''.join(recs_), dtype=np.uint8)
    t = scan.Table(synth.both_strands([target.encode()]), **dict(cases.PRODUCT, Amin='!'))
    a, b, _, _ = _scanner_pair(t, lambda s: s.scan_host(data))
    assert len(b['hits']) > 100
    _check_records(b, data.tobytes(), split_records(data.tobytes()))
    t.close()
    # records of 1.1 .. 9 kB that outgrow their tiles (the redo of skipped tiles), and reads of 5 000 bases
    g = synth.genome()
    tabs = synth.table(g)
    seqs = synth.both_strands(tabs)
    n, L = 60000, 150
    rb = synth.record_bytes(L)
    plain = synth.reads(g, 0, n, L)
    co_plain = scan.chunk_offsets(plain)
    pieces, at = [], 0
    lens = [1100, 2049, 4097, 5000, 5000, 9000]
    for i, ln in enumerate(lens):
        c = 1 + i * ((len(co_plain) - 2) // len(lens))
        cut = int(co_plain[c]) + 108 * rb
        st = rng.randrange(0, len(g) - ln - 1)
        bases = bytearray(g[st:st + ln])
        piece = bytes(tabs[i % len(tabs)][:60])
        bases[ln - 100:ln - 100 + len(piece)] = piece              # (a hit far from both ends of the record)
        pieces.append(plain[at:cut].tobytes()); at = cut
        pieces.append(b'@long%d 1:N:0\n' % i + bytes(bases) + b'\n+\n' + b'I' * ln + b'\n')
    pieces.append(plain[at:].tobytes())
    text = b''.join(pieces)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(seqs, **cases.PRODUCT)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b, _, _ = _scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr)))
    _check_records(b, text, split_records(text))
    longs = [r for r in b['records'] if r.startswith(b'@long')]
    assert len(longs) >= 3 and max(len(r) for r in longs) > 10000
    d.free(); t.close()


def test_hit_dense_input_stores_each_read_once():
    """60 hits per read, 2.4 M hits (the arena overflows and the scan goes again): every hit gets its record, and the
    store holds the 40 000 distinct records once"""
    read = 'ACG' * 60
    one = cases.rec('x', read, 'I' * len(read))
    data = one * 40000
    arr = np.frombuffer(data, dtype=np.uint8)
    t = scan.Table([b'ACG'], **dict(cases.DEFAULTS, minreadlength=10))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    s = scan.Scanner(t, records=True)
    s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr))
    r = s.finish(hits=False)
    assert r['n_hits'] == 40000 * 60
    h = s.hit_arrays()
    assert _lib.lib().kvq_scan_record_bytes(s.h) == 40000 * len(one) == h['record_blob'].nbytes
    assert (h['record_len'] == len(one)).all()
    blob = h['record_blob'].tobytes()
    # the 60 hits of a read share one stored record, and each read has its own
    assert len(set(h['record_off'].tolist())) == 40000
    assert (np.diff(h['file_pos'].reshape(-1, 60), axis=1) == 0).all() and (np.diff(h['record_off'].reshape(-1, 60), axis=1) == 0).all()
    assert all(blob[o:o + len(one)] == one for o in set(h['record_off'].tolist()))
    s.close(); d.free(); t.close()


def test_a_small_record_store_forces_a_rescan_with_the_same_results(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_RECORD_CAP', '512')
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    host = synth.reads(g, 0, 20000, 150)
    text = host.tobytes(); recs = split_records(text)
    t = scan.Table(seqs, **cases.PRODUCT)
    d = scan.DeviceBuffer(host.nbytes); d.upload(host)
    co = scan.chunk_offsets(host)
    a, b, _, nb = _scanner_pair(t, lambda s: s.scan_device(d.ptr, host.nbytes, co))
    assert nb > 512 and len(b['hits']) > 20
    _check_records(b, text, recs)
    half = int(co[len(co) // 2])
    a2, b2, _, _ = _scanner_pair(t, lambda s: (s.scan_host(host[:half]), s.scan_host(host[half:], fpos_base=half)))
    assert b2['records'] == b['records']
    # a C caller that feeds host batches itself is told to go again; records stay on across the reset
    s = scan.Scanner(t, records=True, retain_limit=0)
    s.scan_host(host)
    with pytest.raises(scan.RescanRequired):
        s.finish()
    s.reset(); s.scan_host(host)
    r = s.finish()
    assert r['records'] == b['records']
    s.close()
    # findseqs reads its file again (a fresh scan object: the kept one has its store already)
    _lib.lib().kvq_release_cached()
    p = tmp_path / 's.fastq'; p.write_bytes(text)
    engine.config(**cases.PRODUCT)
    rr = check_findseqs([str(p)], seqs)
    assert [as_bytes(x) for x in rr['records']] == b['records']
    _lib.lib().kvq_release_cached()
    d.free(); t.close()


def test_finish_begin_with_two_scanners_in_flight():
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    host = synth.reads(g, 0, 30000, 150)
    co = scan.chunk_offsets(host)
    t = scan.Table(seqs, **cases.PRODUCT)
    d = scan.DeviceBuffer(host.nbytes); d.upload(host)
    ref = scan.Scanner(t, records=True); ref.scan_device(d.ptr, host.nbytes, co); want = ref.finish(); ref.close()
    _check_records(want, host.tobytes(), split_records(host.tobytes()))
    ring = [scan.Scanner(t, records=True), scan.Scanner(t, records=True)]
    flying = []
    for i in range(5):
        sc = ring[i % 2]; sc.reset(); sc.scan_device(d.ptr, host.nbytes, co); sc.finish_begin(); flying.append(sc)
        if len(flying) == 2:
            r = flying.pop(0).finish()
            assert r['hits'] == want['hits'] and r['records'] == want['records']
    while flying:
        r = flying.pop(0).finish()
        assert r['records'] == want['records']
    for sc in ring:
        sc.close()
    d.free(); t.close()


def test_records_and_a_communicator_are_refused():
    L = _lib.lib()
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    comm = L.kvq_comm_create_local(1, 0, 0x7265636f7264)
    assert comm
    s = scan.Scanner(t, records=True)
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME
    code, msg = _lib.last_error()
    assert code == _lib.ERR_RUNTIME and 'across ranks' in msg
    s.close()
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_records(s.h, 1) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    # only before the first batch or after a reset
    arr = np.frombuffer(cases.rec('a', 'ACGTACGTACGT' * 3, 'I' * 36), dtype=np.uint8)
    s.scan_host(arr)
    assert L.kvq_scan_set_records(s.h, 1) == _lib.ERR_RUNTIME
    s.finish()
    assert not L.kvq_scan_record_blob(s.h) and L.kvq_scan_record_bytes(s.h) == 0
    s.reset()
    assert L.kvq_scan_set_records(s.h, 1) == 0
    s.close()
    L.kvq_comm_destroy(comm)
    t.close()
