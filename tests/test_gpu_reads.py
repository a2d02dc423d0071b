"""
The per-read distributions and the duplication on an MI355X (``kvq_reads_records``, ``kvq_dup_plan``, ``kvq_dup_purge``,
``kvq_dup_levels``; include/kvarq_hip.h): every device array against the CPU twin (``kvq_reads_host``)
AND against the plain statement of the definition (tests/reads_ref.py), word for word, and tied to the profile OF THE SAME
SCAN by the identities of the header -- over the rounding, the empty lines, the lane and path seams, the keys, the count
bins, levels above 0, every way a batch's text reaches ``run_batch`` and every way a scan goes round again.  A scan with
the options must give the hits, hit bytes, stats, counters and path of the same scan without them.
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
def _want(text, co, slots, cuts):
    twin = P.profile_host(text, list(cuts), list(co), per_read=True, duplication=True, slots=slots)
    assert (twin.reads == RR.reads(text, co)).all()
    d = twin.duplication
    assert [d[k] for k in P.DUP_HEADER] + [0, 0] + d['distinct'] + d['records'] == RR.dup(text, co, slots).tolist()
    return twin


def want_of(text, chunk_off=None, slots=0, cuts=CUTS):
    """the twin's profile of a text with both options, checked against the plain statement; computed once per text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    return _want(text, tuple(int(c) for c in co), slots, tuple(cuts))


def check_reads(r, twin):
    got = r['profile']
    assert got.reads is not None and got.duplication is not None
    bad = np.nonzero(got.reads != twin.reads)[0]
    assert bad.size == 0, (bad[:8], got.reads[bad[:8]], twin.reads[bad[:8]])
    assert got.duplication == twin.duplication
    assert (got.words == twin.words).all() and got.records == r['counters'][_lib.CTR_RECORDS]
    d = got.duplication
    dup_words = np.array([d[k] for k in P.DUP_HEADER] + [0, 0] + d['distinct'] + d['records'], dtype=np.int64)
    RR.check_identities(got.reads, dup_words, got.words)          # the profile of the same scan: another kernel's counts


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all()
    assert 'profile' not in a and 'reads_kernel_ms' not in a


def scanner_pair(t, feed, cuts=CUTS, force=False, **kw):
    """(result with no profile, result with the profile and both options) of the same feeding"""
    out = []
    for on in (False, True):
        s = scan.Scanner(t, profile=cuts if on else None, per_read=on, duplication=on, **kw)
        if force:
            s.force_exhaustive()
        feed(s)
        out.append(s.finish())
        s.close()
    same_scan(out[0], out[1])
    assert out[1]['reads_kernel_ms'] > 0
    return out


@pytest.mark.parametrize('how', ['host', 'device'])
@pytest.mark.parametrize('name', sorted(RR.small_texts()))
def test_the_seams_by_hand(name, how):
    """rounding, nothing to count, N counts, line lengths, keys: reads_ref's texts, whose hand counts tests/test_reads_host.py holds"""
    text = RR.small_texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = [0, len(text)]
    feed = (lambda s: s.scan_host(arr)) if how == 'host' else (lambda s: s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64)))
    a, b = scanner_pair(t, feed)
    twin = want_of(text, co if how == 'device' else None)
    check_reads(b, twin)
    assert b['profile'].duplication['level'] == 0 and b['profile'].records == len(RR.lines_of(text, co)) > 5
    d.free(); t.close()


def test_either_option_alone():
    text = RR.lengths_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    twin = want_of(text, cuts=[])
    t = scan.Table(SEQ, **cases.DEFAULTS)
    for per_read, duplication in ((True, False), (False, True)):
        s = scan.Scanner(t, per_read=per_read, duplication=duplication)
        s.scan_host(arr); r = s.finish()
        p = r['profile']
        assert p.cutoffs == [] and (p.words == twin.words).all() and r['reads_kernel_ms'] > 0
        assert (p.reads is not None) == per_read and (p.duplication is not None) == duplication
        assert bool(_lib.lib().kvq_scan_reads(s.h)) == per_read and bool(_lib.lib().kvq_scan_dup(s.h)) == duplication
        if per_read:
            assert (p.reads == twin.reads).all()
        else:
            assert p.duplication == twin.duplication
        s.close()
    t.close()


def test_the_count_bins():
    text = RR.bins_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, np.array([0, arr.nbytes], dtype=np.int64)))
    check_reads(b, want_of(text, [0, len(text)]))
    dd = b['profile'].duplication
    assert dd['distinct'] == [1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 1] and dd['level'] == 0 and dd['keyed'] == sum(RR.COPIES)
    # the contention case: one key, every record of it
    one = np.frombuffer(RR.rec(b'ACGTTGCA' * 10, b'I' * 80) * 20000, dtype=np.uint8)
    s = scan.Scanner(t, per_read=True, duplication=True)
    s.scan_host(one); r = s.finish()
    assert r['profile'].duplication['distinct'] == [0] * 15 + [1] and r['profile'].duplication['records'][15] == 20000
    assert r['profile'].gc_hist[50] == 20000 and r['profile'].duplicate_share() == pytest.approx(1 - 1 / 20000.)
    s.close(); d.free(); t.close()


def test_levels_above_zero_do_not_depend_on_batches_and_slices(monkeypatch):
    """1024 slots: slices of 256 records, the plan and the purge run many times; 3000 keys end at a level of 2 at least"""
    monkeypatch.setenv('KVQ_DUP_SLOTS', '1024')
    text = RR.levels_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = [0, len(text)]
    twin = want_of(text, co, slots=1024)
    level = twin.duplication['level']
    assert level >= 2 and twin.duplication['slots'] == 1024 and twin.duplication['keyed'] > 4000
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, one = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64)))
    assert one['profile'].duplication['level'] == level
    check_reads(one, twin)
    # several host batches, cut at record boundaries: other slices, other moments for the level to move
    recs = [n3 + 1 for _, _, _, n3 in RR.R.records_of(text, co)]
    cuts = [0] + [recs[i] for i in (len(recs) // 7, len(recs) // 3, len(recs) // 2 + 5, len(recs) - 2)] + [len(text)]
    s = scan.Scanner(t, profile=CUTS, per_read=True, duplication=True)
    for x, y in zip(cuts, cuts[1:]):
        s.scan_host(arr[x:y], chunk_off=[0, y - x], fpos_base=x)
    many = s.finish()
    assert many['profile'].duplication['level'] == level
    check_reads(many, twin)
    assert many['profile'] == one['profile']
    # behind a reset: the table starts empty, at level 0
    s.reset()
    s.scan_host(arr[:cuts[2]], chunk_off=[0, cuts[2]])
    part = s.finish()
    check_reads(part, want_of(text[:cuts[2]], [0, cuts[2]], slots=1024))
    s.reset()
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    again = s.finish()
    assert again['profile'] == one['profile']
    s.close()
    # fewer than 512 keys in the same table: level 0, the plan and the purge return at once
    few = RR.levels_text(400, 166)
    farr = np.frombuffer(few, dtype=np.uint8)
    s = scan.Scanner(t, profile=CUTS, per_read=True, duplication=True)
    s.scan_host(farr, chunk_off=[0, len(few)])
    r = s.finish()
    check_reads(r, want_of(few, [0, len(few)], slots=1024))
    assert r['profile'].duplication['level'] == 0 and r['profile'].duplication['tracked_distinct'] == 400
    s.close(); d.free(); t.close()


MATRIX_CFG = {'amin_I': dict(KM.CONFIGS[8], Amin=b'I'), 'redo': dict(KM.CONFIGS[8])}


@pytest.mark.parametrize('mode', ['seeded', 'exhaustive', 'long_reads', 'cycles+records'])
@pytest.mark.parametrize('name', ['amin_I', 'redo'])
def test_device_batch_of_the_trim_matrix(name, mode):
    text, co = matrix_texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr) if co is None else co
    t = scan.Table(TM.table(), **MATRIX_CFG[name])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    kw = {'long_reads': True} if mode == 'long_reads' else {'records': True, 'cycles': True} if mode == 'cycles+records' else {}
    out = []
    for on in (False, True):
        s = scan.Scanner(t, profile=CUTS if on or mode == 'cycles+records' else None, per_read=on, duplication=on, **kw)
        if mode == 'exhaustive':
            s.force_exhaustive()
        s.scan_device(d.ptr, arr.nbytes, co)
        out.append(s.finish())
        s.close()
    a, b = out
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all() and len(b['hits']) > 100
    twin = want_of(text, co)
    check_reads(b, twin)
    if mode == 'seeded':
        assert b['path']['seeded']
    elif mode == 'exhaustive':
        assert b['path']['exhaustive'] and not b['path']['seeded']
    elif mode == 'long_reads':
        assert b['path']['read_list']
    else:
        # the profile and the cycles of the same scan are what they are without the options; so are the records
        assert a['profile'].reads is None and a['profile'].duplication is None and 'per_read' not in a['profile'].as_dict()
        assert (a['profile'].words == b['profile'].words).all() and (a['profile'].cycles == b['profile'].cycles).all()
        assert a['records'] == b['records']
    d.free(); t.close()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_arena_overflow_counts_every_record_once(how, monkeypatch):
    """an arena of 64 hits overflows: the library replays a device batch, Scanner feeds host batches again"""
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    read = 'ACG' * 60
    arr = np.frombuffer(cases.rec('x', read, 'I' * len(read)) * 500 + cases.rec('y', 'GGCC' * 20, '5' * 80) * 3, dtype=np.uint8)
    twin = want_of(arr.tobytes())
    t = scan.Table([b'ACG'], **dict(cases.DEFAULTS, minreadlength=10))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = scan.chunk_offsets(arr)
    res = []
    for on in (False, True):
        s = scan.Scanner(t, profile=CUTS if on else None, per_read=on, duplication=on)
        if how == 'host':
            s.scan_host(arr)
        else:
            s.scan_device(d.ptr, arr.nbytes, co)
        res.append(s.finish(hits=False))
        s.close()
    a, b = res
    assert a['n_hits'] == b['n_hits'] == 500 * 60 > 64
    assert (a['counters'] == b['counters']).all() and a['stats'] == b['stats'] and a['path'] == b['path']
    check_reads(b, twin)
    dd = b['profile'].duplication
    assert b['profile'].records == 503 and dd['distinct'][2] == 1 and dd['records'][12] == 500 and b['profile'].gc_hist[100] == 3
    d.free(); t.close()


def findseqs_pair(files, seqs, inflate='host', route=None, **kw):
    arg = files[0] if len(files) == 1 else files
    a = engine.findseqs(arg, seqs, inflate=inflate)
    b = engine.findseqs(arg, seqs, inflate=inflate, profile=CUTS, per_read=True, duplication=True, **kw)
    if route:
        assert engine.last_inflate() == route
    assert 'profile' not in a
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats']
    assert b['profile'].records == b['stats']['records_parsed']
    return b


def test_every_route_gives_the_reads_of_its_text(tmp_path):
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
        r = findseqs_pair([str(tmp_path / name)], seqs, inflate, route)
        assert r['profile'] == want and r['profile'].reads is not None and r['profile'].duplication is not None, name
    # the same file read again: the kept scan object's table is cleared with its profile
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile=CUTS, per_read=True, duplication=True, cycles=True)
    assert (r['profile'].reads == want.reads).all() and r['profile'].duplication == want.duplication and r['profile'].cycles is not None
    # ... and without the options it gives them up
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile=CUTS)
    assert r['profile'].reads is None and r['profile'].duplication is None and (r['profile'].words == want.words).all()
    # BAM: the reads of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    r = findseqs_pair([str(tmp_path / 'm.bam')], seqs, route='device_bam')
    vwant = want_of(vtext)
    assert r['profile'] == vwant and r['profile'].records > 8000
    assert bam.Bam(str(tmp_path / 'm.bam')).profile(cutoffs=CUTS, per_read=True, duplication=True) == vwant
    # profile-only calls
    assert P.profile(str(tmp_path / 'm.fastq'), cutoffs=CUTS, per_read=True, duplication=True) == want
    only = engine.findseqs(str(tmp_path / 'm.fastq'), [], duplication=True)['profile']
    assert only.cutoffs == [] and only.reads is None and only.duplication == want.duplication


def test_analyser_and_command_line(fastqs):
    engine.config(**cases.PRODUCT)
    path = os.path.join(fastqs, 'test_analyser.fastq')
    fq = Fastq(path, quiet=True)
    with open(path, 'rb') as f:
        want = want_of(f.read(), cuts=[ord('.')])
    templates = {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}
    a = analyse.Analyser()
    a.scan(fq, templates, profile='.', per_read=True, duplication=True)
    assert a.profile == want
    info = a.encode()['info']['profile']
    assert info['per_read'] == want.as_dict()['per_read'] and info['duplication'] == want.as_dict()['duplication']
    b = analyse.Analyser()
    b.scan(fq, templates, profile='.')
    assert b.profile.reads is None and 'per_read' not in b.encode()['info']['profile'] and 'duplication' not in b.encode()['info']['profile']
    assert b.hits == a.hits
    assert fq.profile(per_read=True, duplication=True) == want
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([path, '--per-read', '--duplication'])
    assert out.getvalue().strip() == '\n'.join([want.summary()] + want.per_read_lines() + want.duplication_lines())


def test_refusals_and_off():
    L = _lib.lib()
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    arr = np.frombuffer(cases.rec('a', 'ACGTACGTACGT' * 3, 'I' * 36), dtype=np.uint8)
    # no profile: neither option
    s = scan.Scanner(t)
    for mode in (1, 2, 3):
        assert L.kvq_scan_set_read_stats(s.h, mode) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_read_stats(s.h, 0) == 0
    # only before the first batch or after a reset; only the two bits
    assert L.kvq_scan_set_profile(s.h, None, 0) == 0
    assert L.kvq_scan_set_read_stats(s.h, 4) == _lib.ERR_RUNTIME
    s.scan_host(arr)
    assert L.kvq_scan_set_read_stats(s.h, 3) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    r = s.finish()
    assert not L.kvq_scan_reads(s.h) and not L.kvq_scan_dup(s.h) and L.kvq_scan_reads_kernel_ms(s.h) == 0
    off = P.from_scan(L, s.h)
    assert 'per_read' not in off.as_dict() and 'duplication' not in off.as_dict() and off.reads is None and 'reads_kernel_ms' not in r
    s.reset()
    assert L.kvq_scan_set_read_stats(s.h, 3) == 0
    s.scan_host(arr); s.finish()
    reads = np.ctypeslib.as_array(L.kvq_scan_reads(s.h), shape=(RR.LEN,))
    dup = np.ctypeslib.as_array(L.kvq_scan_dup(s.h), shape=(RR.D_LEN,))
    assert (reads == RR.reads(arr.tobytes(), [0, arr.nbytes])).all() and reads[RR.GC + 50] == 1
    assert (dup == RR.dup(arr.tobytes(), [0, arr.nbytes])).all() and dup[RR.D_DISTINCT] == 1
    # the profile off takes them with it
    s.reset()
    assert L.kvq_scan_set_profile(s.h, None, -1) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_reads(s.h) and not L.kvq_scan_dup(s.h) and not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_read_stats(s.h, 1) == _lib.ERR_RUNTIME
    s.close()
    # with a communicator: the scan keeps no profile, so neither option (the rule is the profile's, inherited)
    comm = L.kvq_comm_create_local(1, 0, 0x72656164)
    assert comm
    s = scan.Scanner(t, per_read=True, duplication=True)
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    s.close()
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_profile(s.h, None, 0) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    assert L.kvq_scan_set_read_stats(s.h, 3) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    s.close()
    L.kvq_comm_destroy(comm)
    # the flags of kvq_findseqs_opts / kvq_findseqs_ex without the profile's
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    for flag in (_lib.FIND_READ_STATS, _lib.FIND_DUPLICATION):
        opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), flag, 0, (C.c_uint8 * 8)())
        assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
        assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
        assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, flag)
        assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    t.close()
