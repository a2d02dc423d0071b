"""
The overrepresented sequences on an MI355X (``kvq_over_records``, ``kvq_over_select``; include/kvarq_hip.h):
the device array against the CPU twin (``kvq_over_host``) AND against the plain statement of the definition
(tests/over_ref.py), word for word, and tied to the profile and the duplication OF THE SAME SCAN by the identities of the header
-- over the threshold's seams, the bound of 1000 rows, the candidate boundary under every cut of the batches, the key bytes, the
order, one key for every record, every way a batch's text reaches ``run_batch`` and every way a scan goes round again.  A scan
with the option must give the hits, hit bytes, stats, counters and path of the same scan without it.
"""
import contextlib
import ctypes as C
import functools
import gzip
import io
import os

import numpy as np
import pytest

import bam_writer as W
import cases
import kernel_matrix as KM
import over_ref as OR
import reads_ref as RR
import trim_matrix as TM
from kvarq_amd import _lib, analyse, bam, engine, profile as P, scan, synth
from kvarq_amd.fastq import Fastq
from oracle import oracle as O
from test_host_logic import bgzf
from test_profile_host import matrix_texts

pytestmark = pytest.mark.gpu

CUTS = [ord('.'), ord('I')]
SEQ = [b'ACGTACGTACGTACGTACGTACGTA']


@functools.lru_cache(maxsize=None)
def _want(text, co, M, slots, cuts):
    twin = P.profile_host(text, list(cuts), list(co), duplication=slots >= 0, slots=max(slots, 0), overrepresented=True, over_records=M)
    assert (twin.over == OR.over(text, co, M)).all()
    return twin


def want_of(text, chunk_off=None, M=0, slots=-1, cuts=CUTS):
    """the twin's profile of a text with the option (slots >= 0: and the duplication), checked against the plain statement;
    computed once per text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    return _want(text, tuple(int(c) for c in co), M, slots, tuple(cuts))


def check_over(r, twin):
    got = r['profile']
    assert got.over is not None
    bad = np.nonzero(got.over != twin.over)[0]
    assert bad.size == 0, (bad[:8], got.over[bad[:8]], twin.over[bad[:8]])
    assert got.overrepresented == twin.overrepresented and got.over_info == twin.over_info
    assert (got.words == twin.words).all() and got.records == r['counters'][_lib.CTR_RECORDS]
    OR.check_identities(got.over, got.words, got.duplication)       # the profile (and the duplication) of the same scan: other kernels' counts
    assert r['over_kernel_ms'] > 0 or got.records == 0


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all()
    assert 'profile' not in a and 'over_kernel_ms' not in a


def scanner_pair(t, feed, cuts=CUTS, force=False, **kw):
    """(result with no profile, result with the profile and the option) of the same feeding"""
    out = []
    for on in (False, True):
        s = scan.Scanner(t, profile=cuts if on else None, overrepresented=on, **kw)
        if force:
            s.force_exhaustive()
        feed(s)
        out.append(s.finish())
        s.close()
    same_scan(out[0], out[1])
    return out


@pytest.mark.parametrize('how', ['host', 'device'])
@pytest.mark.parametrize('name', sorted(OR.small_texts()))
def test_the_texts(name, how, monkeypatch):
    """the threshold's seams, the bound, the boundary, the key bytes, the order, one key for every record: over_ref's texts,
    whose hand counts tests/test_over_host.py holds"""
    text, M = OR.small_texts()[name]
    if M:
        monkeypatch.setenv('KVQ_OVER_RECORDS', str(M))
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = [0, len(text)]
    feed = (lambda s: s.scan_host(arr, chunk_off=co)) if how == 'host' else (lambda s: s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64)))
    a, b = scanner_pair(t, feed)
    check_over(b, want_of(text, co, M))
    o = b['profile'].over_info
    assert o['records_limit'] == (M or 1 << 18) and (o['counted'] == o['keyed']) == (name != 'boundary')
    if name == 'bound_1000':
        assert o['listed'] == 1000
    if name == 'contention':
        assert [(r.count, r.share) for r in b['profile'].overrepresented] == [(20000, 1.0)]
    d.free(); t.close()


def test_the_candidate_boundary_under_every_cut(monkeypatch):
    """M = 64: key A, first seen at record 63, is listed with its 201 records, key B, first seen at record 64, is absent --
    whether the boundary lies inside a batch, between two batches or in front of whole batches, and again after a reset"""
    monkeypatch.setenv('KVQ_OVER_RECORDS', str(OR.BOUNDARY_M))
    text, a_key, b_key, five = OR.boundary_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = [0, len(text)]
    twin = want_of(text, co, OR.BOUNDARY_M)
    assert [r.sequence for r in twin.overrepresented] == [a_key, five] and twin.over_info['counted'] < twin.over_info['keyed']
    ends = [n3 + 1 for _, _, _, n3 in RR.R.records_of(text, co)]            # ends[i]: the first byte behind record i
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    s = scan.Scanner(t, profile=CUTS, overrepresented=True)
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    one = s.finish()
    check_over(one, twin)
    # cut before (behind record 62: A still makes it), exactly at (behind record 63) and behind the boundary (behind record 64); a batch of
    # one record; batches that lie wholly behind the batch the boundary falls into
    for recs in ((63,), (64,), (65,), (10, 63, 64, 65, 300), (1, 200, 400, 600)):
        cuts = [0] + [ends[i - 1] for i in recs] + [len(text)]
        s.reset()
        for x, y in zip(cuts, cuts[1:]):
            s.scan_host(arr[x:y], chunk_off=[0, y - x], fpos_base=x)
        many = s.finish()
        check_over(many, twin)
        assert many['profile'] == one['profile'], recs
    s.reset()
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    assert s.finish()['profile'] == one['profile']
    # a part of the text behind a reset: the table starts empty, the numbering at 0
    s.reset()
    s.scan_host(arr[ends[69]:], chunk_off=[0, len(text) - ends[69]])
    check_over(s.finish(), want_of(text[ends[69]:], [0, len(text) - ends[69]], OR.BOUNDARY_M))
    s.close(); d.free(); t.close()


def test_beside_the_duplication_of_the_same_scan(monkeypatch):
    """1024 slots put the duplication at a level of 2 and more: the list is what it is at level 0"""
    text = RR.levels_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = [0, len(text)]
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    res = []
    for slots in (0, 1024):
        if slots:
            monkeypatch.setenv('KVQ_DUP_SLOTS', str(slots))
        twin = want_of(text, co, slots=slots)
        s = scan.Scanner(t, profile=CUTS, duplication=True, overrepresented=True)
        s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        r = s.finish()
        check_over(r, twin)
        p = r['profile']
        assert p == twin and p.duplication['level'] == twin.duplication['level'] and (p.duplication['level'] >= 2) == bool(slots)
        assert p.over_info['candidates'] == 3000 and (slots or p.over_info['candidates'] == p.duplication['tracked_distinct'])
        assert len(p.overrepresented) == 60 and all(p.duplication['distinct'][RR.bin_of(x.count)] >= 1 for x in p.overrepresented)
        res.append(p)
        s.close()
    assert (res[0].over == res[1].over).all()
    d.free(); t.close()


MATRIX_CFG = {'amin_I': dict(KM.CONFIGS[8], Amin=b'I'), 'redo': dict(KM.CONFIGS[8])}


@pytest.mark.parametrize('mode', ['seeded', 'exhaustive', 'long_reads'])
@pytest.mark.parametrize('name', ['amin_I', 'redo'])
def test_device_batch_of_the_trim_matrix(name, mode, monkeypatch):
    monkeypatch.setenv('KVQ_OVER_RECORDS', '100')
    text, co = matrix_texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr) if co is None else co
    t = scan.Table(TM.table(), **MATRIX_CFG[name])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, co), force=mode == 'exhaustive', **({'long_reads': True} if mode == 'long_reads' else {}))
    assert len(b['hits']) > 100
    check_over(b, want_of(text, co, 100))
    if mode == 'seeded':
        assert b['path']['seeded']
    elif mode == 'exhaustive':
        assert b['path']['exhaustive'] and not b['path']['seeded']
    else:
        assert b['path']['read_list']
    d.free(); t.close()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_arena_overflow_counts_every_record_once(how, monkeypatch):
    """an arena of 64 hits overflows: the library replays a device batch, Scanner feeds host batches again -- the numbering
    starts at 0 again, the candidates are the same and every record counts once"""
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    monkeypatch.setenv('KVQ_OVER_RECORDS', '400')
    read = 'ACG' * 60
    arr = np.frombuffer(cases.rec('x', read, 'I' * len(read)) * 500 + cases.rec('y', 'GGCC' * 20, '5' * 80) * 3, dtype=np.uint8)
    twin = want_of(arr.tobytes(), M=400)
    t = scan.Table([b'ACG'], **dict(cases.DEFAULTS, minreadlength=10))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = scan.chunk_offsets(arr)
    res = []
    for on in (False, True):
        s = scan.Scanner(t, profile=CUTS if on else None, overrepresented=on)
        if how == 'host':
            s.scan_host(arr)
        else:
            s.scan_device(d.ptr, arr.nbytes, co)
        res.append(s.finish(hits=False))
        s.close()
    a, b = res
    assert a['n_hits'] == b['n_hits'] == 500 * 60 > 64
    assert (a['counters'] == b['counters']).all() and a['stats'] == b['stats'] and a['path'] == b['path']
    check_over(b, twin)
    assert [(r.count, r.sequence) for r in b['profile'].overrepresented] == [(500, read.encode()[:64])] and b['profile'].over_info['counted'] == 500
    d.free(); t.close()


def findseqs_pair(files, seqs, inflate='host', route=None, **kw):
    arg = files[0] if len(files) == 1 else files
    a = engine.findseqs(arg, seqs, inflate=inflate)
    b = engine.findseqs(arg, seqs, inflate=inflate, profile=CUTS, overrepresented=True, **kw)
    if route:
        assert engine.last_inflate() == route
    assert 'profile' not in a
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats']
    assert b['profile'].records == b['stats']['records_parsed']
    return b


def test_every_route_gives_the_list_of_its_text(tmp_path, monkeypatch):
    monkeypatch.setenv('KVQ_OVER_RECORDS', '1000')            # (the boundary inside the text: both modes of the kernel on every route)
    case = cases.by_name()['multichunk']
    # the case's text, and every hundredth of its records forty times more behind it: keys that repeat -- ten of them candidates, the
    # others first seen behind the boundary
    text = cases.multichunk()
    ends = [n3 + 1 for _, _, _, n3 in RR.R.records_of(text, [0, len(text)])]
    text = text + b''.join(text[a:b] for a, b in list(zip([0] + ends, ends))[::100]) * 40
    engine.config(**case.config)
    seqs = case.seq_bytes()
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'h.fastq.gz').write_bytes(gzip.compress(text, 1, mtime=0))
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
    want = want_of(text, M=1000)
    assert want.records > 8000 and want.over_info['counted'] < want.over_info['keyed'] and len(want.overrepresented) >= 10
    for name, inflate, route in (('m.fastq', 'host', 'host'), ('h.fastq.gz', 'host', 'host'), ('b.fastq.gz', 'device', 'device'),
                                 ('g.fastq.gz', 'device_any', 'device_gzip')):
        r = findseqs_pair([str(tmp_path / name)], seqs, inflate, route)
        assert r['profile'] == want and (r['profile'].over == want.over).all(), name
    # the same file read again: the kept scan object's table is cleared with its profile, beside the other passes
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile=CUTS, overrepresented=True, duplication=True, cycles=True)
    assert (r['profile'].over == want.over).all() and r['profile'].duplication is not None and r['profile'].cycles is not None
    OR.check_identities(r['profile'].over, r['profile'].words, r['profile'].duplication)
    # ... and without the option it gives it up
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile=CUTS)
    assert r['profile'].over is None and r['profile'].overrepresented is None and (r['profile'].words == want.words).all()
    # BAM: the list of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    r = findseqs_pair([str(tmp_path / 'm.bam')], seqs, route='device_bam')
    vwant = want_of(vtext, M=1000)
    assert r['profile'] == vwant and (r['profile'].over == vwant.over).all() and r['profile'].records > 8000
    assert bam.Bam(str(tmp_path / 'm.bam')).profile(cutoffs=CUTS, overrepresented=True) == vwant
    # profile-only calls
    assert P.profile(str(tmp_path / 'm.fastq'), cutoffs=CUTS, overrepresented=True) == want
    only = engine.findseqs(str(tmp_path / 'm.fastq'), [], overrepresented=True)['profile']
    assert only.cutoffs == [] and only.reads is None and (only.over == want.over).all()


def test_analyser_command_line_and_labels(fastqs, tmp_path):
    engine.config(**cases.PRODUCT)
    path = os.path.join(fastqs, 'test_analyser.fastq')
    fq = Fastq(path, quiet=True)
    with open(path, 'rb') as f:
        want = want_of(f.read(), cuts=[ord('.')])
    templates = {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}
    a = analyse.Analyser()
    a.scan(fq, templates, profile='.', overrepresented=True)
    assert a.profile == want
    info = a.encode()['info']['profile']
    assert info['overrepresented'] == want.as_dict()['overrepresented']
    b = analyse.Analyser()
    b.scan(fq, templates, profile='.')
    assert b.profile.over is None and 'overrepresented' not in b.encode()['info']['profile'] and 'overrepresented' not in b.profile.as_dict()
    assert b.hits == a.hits
    assert fq.profile(overrepresented=True) == want
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([path, '--overrepresented'])
    assert out.getvalue().strip() == '\n'.join([want.summary()] + want.overrepresented_lines())
    # the labels: a planted adapter, its reverse complement, a poly-G key, a user's mapping, none
    from test_over_host import labelled
    keys, text = labelled()
    (tmp_path / 'l.fastq').write_bytes(text)
    p = P.profile(str(tmp_path / 'l.fastq'), cutoffs=CUTS, overrepresented=True)
    assert [r.sequence for r in p.overrepresented] == keys
    assert [r.source for r in p.overrepresented] == ['Illumina universal adapter', 'Illumina universal adapter', 'poly-G', None, None]
    p = P.profile(str(tmp_path / 'l.fastq'), cutoffs=CUTS, overrepresented=True, sources={'mine': b'GATTACA'})
    assert [r.source for r in p.overrepresented] == [None, None, None, None, 'mine']
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 'l.fastq'), '--overrepresented'])
    assert out.getvalue().strip().split('\n')[-6:] == P.profile_host(text, (), [0, len(text)], overrepresented=True).overrepresented_lines()


def test_refusals_and_off():
    L = _lib.lib()
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    arr = np.frombuffer(cases.rec('a', 'ACGTACGTACGT' * 3, 'I' * 36) * 2, dtype=np.uint8)
    # no profile: no option
    s = scan.Scanner(t)
    assert L.kvq_scan_set_overrepresented(s.h, 1) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_overrepresented(s.h, 0) == 0
    # only before the first batch or after a reset
    assert L.kvq_scan_set_profile(s.h, None, 0) == 0
    s.scan_host(arr)
    assert L.kvq_scan_set_overrepresented(s.h, 1) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    r = s.finish()
    assert not L.kvq_scan_over(s.h) and L.kvq_scan_over_kernel_ms(s.h) == 0
    off = P.from_scan(L, s.h)
    assert 'overrepresented' not in off.as_dict() and off.over is None and 'over_kernel_ms' not in r
    s.reset()
    assert L.kvq_scan_set_overrepresented(s.h, 1) == 0
    assert not L.kvq_scan_over(s.h)                                # (not finished)
    s.scan_host(arr); s.finish()
    over = np.ctypeslib.as_array(L.kvq_scan_over(s.h), shape=(OR.O_LEN,))
    assert (over == OR.over(arr.tobytes(), [0, arr.nbytes])).all() and over[OR.O_LISTED] == 1 and over[OR.O_ROWS + 1] == 2
    assert L.kvq_scan_over_kernel_ms(s.h) > 0
    # off again; the profile off takes it along
    s.reset()
    assert L.kvq_scan_set_overrepresented(s.h, 0) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_over(s.h) and L.kvq_scan_over_kernel_ms(s.h) == 0 and L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_overrepresented(s.h, 1) == 0 and L.kvq_scan_set_profile(s.h, None, -1) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_over(s.h) and not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_overrepresented(s.h, 1) == _lib.ERR_RUNTIME
    s.close()
    # with a communicator: the scan keeps no profile, so no option (the rule is the profile's, inherited)
    comm = L.kvq_comm_create_local(1, 0, 0x6f766572)
    assert comm
    s = scan.Scanner(t, overrepresented=True)
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    s.close()
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_overrepresented(s.h, 1) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    s.close()
    L.kvq_comm_destroy(comm)
    # the flag of kvq_findseqs_opts / kvq_findseqs_ex without the profile's
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_OVERREPRESENTED, 0, (C.c_uint8 * 8)())
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_OVERREPRESENTED)
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    # kvq_scan_set_read_stats takes no bit for it
    s = scan.Scanner(t, profile=CUTS)
    assert L.kvq_scan_set_read_stats(s.h, 4) == _lib.ERR_RUNTIME
    s.close(); t.close()
