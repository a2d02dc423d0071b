"""
The profile of the input on an MI355X (``kvq_profile_records``; include/kvarq_hip.h): every device
profile against the CPU twin (``kvq_profile_host``) AND against the plain statement of the definition
(tests/profile_ref.py), over every way a batch's text reaches ``run_batch`` and every way a scan goes round again.  A scan
with the profile must give the hits, hit bytes, stats, counters and path of the same scan without it.
"""
import gzip
import os

import numpy as np
import pytest

import bam_writer as W
import cases
import kernel_matrix as KM
import profile_ref as R
import trim_matrix as TM
from kvarq_amd import _lib, bam, engine, profile as P, scan, synth
from kvarq_amd.fastq import Fastq
from oracle import oracle as O
from test_host_logic import bgzf
from test_profile_host import matrix_texts

pytestmark = pytest.mark.gpu

CUTS = R.CUTOFFS8


def want_of(text, chunk_off=None, cuts=CUTS):
    """the twin's profile of a text, checked against the plain statement"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    twin = P.profile_host(text, cuts, co)
    assert (twin.words == R.profile(text, cuts, co)).all()
    return twin


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all()
    assert 'profile' not in a


def scanner_pair(t, feed, cuts=CUTS, force=False, **kw):
    """(result without the profile, result with it) of the same feeding"""
    out = []
    for prof in (None, cuts):
        s = scan.Scanner(t, profile=prof, **kw)
        if force:
            s.force_exhaustive()
        feed(s)
        out.append(s.finish())
        s.close()
    same_scan(out[0], out[1])
    return out


def check_profile(r, want):
    got = r['profile']
    bad = np.nonzero(got.words != want.words)[0]
    assert got.cutoffs == want.cutoffs and bad.size == 0, (bad[:8], got.words[bad[:8]], want.words[bad[:8]])
    assert got.records == r['counters'][_lib.CTR_RECORDS]
    R.check_identities(got.words, len(got.cutoffs))


MATRIX_CFG = {'amin_I': dict(KM.CONFIGS[8], Amin=b'I'), 'redo': dict(KM.CONFIGS[8]), 'families': dict(KM.CONFIGS[8])}


@pytest.mark.parametrize('mode', ['seeded', 'exhaustive', 'shared-index'])
@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_device_batch_of_the_trim_matrix(name, mode):
    text, co = matrix_texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr) if co is None else co
    want = want_of(text, co)
    seqs = TM.table() + ([b'ACGTNNACGTTGCAACGTACGTAGCTAGCTAA'] if mode == 'shared-index' else [])
    t = scan.Table(seqs, **MATRIX_CFG[name])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, co), force=mode == 'exhaustive')
    check_profile(b, want)
    if mode == 'seeded':
        assert b['path']['seeded'] and len(b['hits']) > 100
    elif mode == 'exhaustive':
        assert b['path']['exhaustive'] and not b['path']['seeded']
    else:
        assert not t.seeded[-1] and b['path']['seeded'] and b['path']['exhaustive']
    # the trim at the scan's own Amin: the profile's lengths are the scan's
    amin = MATRIX_CFG[name]['Amin']
    amin = amin[0] if isinstance(amin, bytes) else ord(amin)
    if amin in CUTS:
        assert b['profile'].readlengths(amin) == b['stats']['readlengths']
    d.free(); t.close()


def test_skipped_tiles_and_long_records_are_counted_once():
    text, co = matrix_texts()['redo']
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(TM.table(), **MATRIX_CFG['redo'])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, co))
    assert b['path']['tiles_rescanned'] and not b['path']['rescanned']
    check_profile(b, want_of(text, co))
    assert b['profile'].longest == 9000 and b['profile'].records == len(R.records_of(text, [int(c) for c in co]))
    d.free(); t.close()


@pytest.mark.parametrize('every', [False, True])
def test_a_batch_whose_speculation_fails_is_counted_once(every):
    """every=False: the text of test_gpu_records.py:228-247 (base lines that may start with '@' or '+') through scan_host.
    The seed-filter pass gets through that text without a failed validation today (tests/test_gpu_parity.py says why), so
    path['rescanned'] is asserted on the variation that suite uses to make the failure sure (every=True: EVERY quality
    line starts with '@'): the batch is rolled back and redone as a whole, and the profile -- taken by the first pass,
    from the exact index -- counts its 4000 records once."""
    from test_gpu_parity import QUIRK_CFG, _quirk_text
    data = np.frombuffer(b''.join(_quirk_text(0, every)), dtype=np.uint8)
    t = scan.Table(synth.both_strands([cases.QUIRK_SEQ.encode()]), **QUIRK_CFG)
    a, b = scanner_pair(t, lambda s: s.scan_host(data))
    assert b['path']['rescanned'] == every and len(b['hits']) > 100
    check_profile(b, want_of(data.tobytes()))
    assert b['profile'].records == 4000
    t.close()


def _dense():
    read = 'ACG' * 60
    return np.frombuffer(cases.rec('x', read, 'I' * len(read)) * 40000, dtype=np.uint8)


@pytest.mark.parametrize('how', ['device', 'host', 'device-records'])
def test_arena_overflow_counts_every_record_once(how, monkeypatch):
    """2.4 M hits: the arena overflows; the library replays a device batch, Scanner feeds host batches again"""
    if how == 'device-records':
        monkeypatch.setenv('KVQ_RECORD_CAP', '512')
    arr = _dense()
    cuts = [ord('!'), ord('I'), ord('J')]
    want = want_of(arr.tobytes(), cuts=cuts)
    t = scan.Table([b'ACG'], **dict(cases.DEFAULTS, minreadlength=10))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = scan.chunk_offsets(arr)
    res = []
    for prof in (None, cuts):
        s = scan.Scanner(t, profile=prof, records=how == 'device-records')
        if how == 'host':
            s.scan_host(arr)
        else:
            s.scan_device(d.ptr, arr.nbytes, co)
        r = s.finish(hits=False)
        res.append((r, s.hit_arrays()))
        s.close()
    (a, ha), (b, hb) = res
    assert a['n_hits'] == b['n_hits'] == 40000 * 60
    assert (a['counters'] == b['counters']).all() and a['stats'] == b['stats'] and a['path'] == b['path']
    # (where a record lies in the store is the order its read was gathered in: not the same from scan to scan)
    assert all((ha[k] == hb[k]).all() for k in ha if k not in ('record_off', 'record_blob'))
    if how == 'device-records':
        assert ha['record_blob'].nbytes == hb['record_blob'].nbytes == arr.nbytes and len(set(hb['record_off'].tolist())) == 40000
    check_profile(b, want)
    assert b['profile'].records == 40000 and b['profile'].readlengths('J') == (40000,)
    d.free(); t.close()


def findseqs_pair(files, seqs, cuts, inflate='host', route=None, records=False):
    arg = files[0] if len(files) == 1 else files
    a = engine.findseqs(arg, seqs, inflate=inflate, records=records)
    b = engine.findseqs(arg, seqs, inflate=inflate, records=records, profile=cuts)
    if route:
        assert engine.last_inflate() == route
    assert 'profile' not in a
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b.get('records') == a.get('records')
    assert b['profile'].records == b['stats']['records_parsed']
    return b


def test_every_route_gives_the_profile_of_its_text(tmp_path):
    case = cases.by_name()['multichunk']
    text = cases.multichunk()
    engine.config(**case.config)
    seqs = case.seq_bytes()
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'h.fastq.gz').write_bytes(gzip.compress(text, 1, mtime=0))
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
    want = want_of(text)
    assert want.records > 8000
    for name, inflate, route in (('m.fastq', 'host', 'host'), ('h.fastq.gz', 'host', 'host'), ('b.fastq.gz', 'device', 'device'),
                                 ('g.fastq.gz', 'device_any', 'device_gzip')):
        r = findseqs_pair([str(tmp_path / name)], seqs, CUTS, inflate, route, records=name == 'm.fastq')
        assert r['profile'] == want, name
    # two files: one stream, the sum of their profiles
    head = text[:O.chunk_offsets(text)[1]]
    (tmp_path / 'second.fastq').write_bytes(head)
    r = findseqs_pair([str(tmp_path / 'm.fastq'), str(tmp_path / 'second.fastq')], seqs, CUTS)
    both = P.Profile(R.profile(head, CUTS, into=want.words.copy()), CUTS)
    assert r['profile'] == both and r['profile'].records == want.records + want_of(head).records
    # BAM: the profile of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    r = findseqs_pair([str(tmp_path / 'm.bam')], seqs, CUTS, route='device_bam')
    assert r['profile'] == want_of(vtext) and r['profile'].records > 8000


def test_two_host_batches_give_the_one_batch_profile():
    g = synth.genome()
    t = scan.Table(synth.both_strands(synth.table(g)), **cases.PRODUCT)
    host = synth.reads(g, 0, 30000, 150)
    co = scan.chunk_offsets(host)
    assert len(co) > 3
    a, one = scanner_pair(t, lambda s: s.scan_host(host))
    half = int(co[len(co) // 2])
    a2, two = scanner_pair(t, lambda s: (s.scan_host(host[:half]), s.scan_host(host[half:], fpos_base=half)))
    check_profile(one, want_of(host.tobytes()))
    assert two['profile'] == one['profile'] and two['hits'] == one['hits'] and one['profile'].records == 30000
    # True: the table's own Amin alone
    s = scan.Scanner(t, profile=True); s.scan_host(host); r = s.finish(); s.close()
    assert r['profile'].cutoffs == [ord('.')] and r['profile'].readlengths('.') == r['stats']['readlengths']
    t.close()


def test_profile_of_a_file_without_sequences(tmp_path, fastqs):
    path = os.path.join(fastqs, 'L3_N1014_hits_5k.fastq')
    engine.config(**cases.PRODUCT)
    with open(path, 'rb') as f:
        text = f.read()
    p = P.profile(path, cutoffs=CUTS)
    assert p == want_of(text) and p.records == 1250
    # the default: the configured Amin alone
    p1 = P.profile(path)
    assert p1.cutoffs == [ord('.')] and p1.readlengths('.') == p.readlengths('.')
    r = engine.findseqs(path, [], profile='.')
    assert r['hits'] == () and r['stats']['readlengths'] == p.readlengths('.')
    # the command line prints the summary
    import contextlib, io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([path, '-Q', '13', '-Q', '30'])
    assert out.getvalue().strip() == P.profile(path, cutoffs=['.', '?']).summary()
    assert 'dQ=0' in out.getvalue() and "cutoff='.'" in out.getvalue() and "cutoff='?'" in out.getvalue()


def test_fastq_profile_agrees_with_the_sampled_guess(fastqs):
    engine.config(**cases.PRODUCT)
    fq = Fastq(os.path.join(fastqs, 'test_analyser.fastq'), quiet=True)
    p = fq.profile()
    assert p.dQ() == fq.dQ and p.variants() == fq.variants and p.cutoffs == [ord('.')]
    assert p.score_range() == fq.min_max_score_check_file()
    from kvarq_amd import analyse
    a = analyse.Analyser()
    a.scan(fq, {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}, profile='.I')
    assert a.profile.cutoffs == [ord('.'), ord('I')] and a.profile.readlengths('.') == a.stats['readlengths']
    assert a.encode()['info']['profile']['records'] == a.stats['records_parsed']
    b = analyse.Analyser()
    b.scan(fq, {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)})
    assert b.profile is None and 'profile' not in b.encode()['info'] and b.hits == a.hits


def test_refusals():
    L = _lib.lib()
    import ctypes as C
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    cuts = (C.c_uint8 * 9)(*range(40, 49))
    comm = L.kvq_comm_create_local(1, 0, 0x70726f66)
    assert comm
    s = scan.Scanner(t, profile='.')
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    s.close()
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_profile(s.h, cuts, 1) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    # nine cutoffs
    assert L.kvq_scan_set_profile(s.h, cuts, 9) == _lib.ERR_RUNTIME and 'at most 8' in _lib.last_error()[1]
    assert L.kvq_scan_profile_cutoffs(s.h, None) == -1
    with pytest.raises(ValueError):
        scan.Scanner(t, profile=range(9))
    # only before the first batch or after a reset
    arr = np.frombuffer(cases.rec('a', 'ACGTACGTACGT' * 3, 'I' * 36), dtype=np.uint8)
    s.scan_host(arr)
    assert L.kvq_scan_set_profile(s.h, cuts, 2) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    s.finish()
    assert not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_profile(s.h, cuts, 2) == 0 and L.kvq_scan_profile_cutoffs(s.h, None) == 2
    s.scan_host(arr); s.finish()
    words = np.ctypeslib.as_array(L.kvq_scan_profile(s.h), shape=(R.profile_len(2),))
    assert (words == R.profile(arr.tobytes(), [40, 41], [0, arr.nbytes])).all() and words[R.RECORDS] == 1
    # off again, and zero cutoffs
    s.reset()
    assert L.kvq_scan_set_profile(s.h, None, -1) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_profile(s.h, None, 0) == 0
    s.scan_host(arr); s.finish()
    words = np.ctypeslib.as_array(L.kvq_scan_profile(s.h), shape=(R.profile_len(0),))
    assert (words == R.profile(arr.tobytes(), [], [0, arr.nbytes])).all()
    s.close()
    L.kvq_comm_destroy(comm)
    t.close()


def test_finish_begin_with_two_scanners_in_flight():
    g = synth.genome()
    seqs = synth.both_strands(synth.table(g))
    host = synth.reads(g, 0, 30000, 150)
    co = scan.chunk_offsets(host)
    t = scan.Table(seqs, **cases.PRODUCT)
    d = scan.DeviceBuffer(host.nbytes); d.upload(host)
    plain = scan.Scanner(t); plain.scan_device(d.ptr, host.nbytes, co); base = plain.finish(); plain.close()
    want = want_of(host.tobytes())
    ring = [scan.Scanner(t, profile=CUTS), scan.Scanner(t, profile=CUTS)]
    flying = []
    for i in range(5):
        sc = ring[i % 2]; sc.reset(); sc.scan_device(d.ptr, host.nbytes, co); sc.finish_begin(); flying.append(sc)
        if len(flying) == 2:
            r = flying.pop(0).finish()
            assert r['hits'] == base['hits'] and (r['counters'] == base['counters']).all()
            check_profile(r, want)
    while flying:
        check_profile(flying.pop(0).finish(), want)
    for sc in ring:
        sc.close()
    d.free(); t.close()
