"""
The per-cycle counts on an MI355X (``kvq_profile_cycles``; include/kvarq_hip.h): every device array
against the CPU twin (``kvq_cycles_host``) AND against the plain statement of the definition (tests/cycles_ref.py), word for
word, and tied to the profile OF THE SAME SCAN by the identities of the header -- over every way a batch's text reaches
``run_batch`` and every way a scan goes round again.  A scan with the cycles must give the hits, hit bytes, stats, counters
and path of the same scan without them.
"""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

import bam_writer as W
import cases
import cycles_ref as CR
import kernel_matrix as KM
import trim_matrix as TM
from kvarq_amd import _lib, analyse, bam, engine, profile as P, scan, synth
from kvarq_amd.fastq import Fastq
from oracle import oracle as O
from test_cycles_host import cold_texts, seams_text
from test_host_logic import bgzf
from test_profile_host import matrix_texts

pytestmark = pytest.mark.gpu

CUTS = [ord('.'), ord('I')]


def want_of(text, chunk_off=None, cuts=CUTS):
    """(the twin's profile with cycles of a text, its score facts), the cycles checked against the plain statement"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    twin = P.profile_host(text, cuts, co, cycles=True)
    assert (twin.cycles == CR.cycles(text, co)).all()
    return twin, CR.score_facts(text, co)


@functools.lru_cache(maxsize=None)
def matrix_want(name):
    """want_of a text of the trim matrix: computed once, shared by the tests that scan it"""
    text, co = matrix_texts()[name]
    return want_of(text, scan.chunk_offsets(np.frombuffer(text, dtype=np.uint8)) if co is None else co)


def check_cycles(r, want):
    twin, facts = want
    got = r['profile']
    assert got.cycles is not None
    bad = np.nonzero(got.cycles != twin.cycles)[0]
    assert bad.size == 0, (bad[:8], got.cycles[bad[:8]], twin.cycles[bad[:8]])
    assert got == twin and got.records == r['counters'][_lib.CTR_RECORDS]
    CR.check_identities(got.cycles, got.words, facts)          # the profile of the same scan: another kernel's counts


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats'] and b['path'] == a['path']
    assert (b['counters'] == a['counters']).all()
    assert 'profile' not in a


def scanner_pair(t, feed, cuts=CUTS, force=False, **kw):
    """(result with neither profile nor cycles, result with both) of the same feeding"""
    out = []
    for cyc in (False, True):
        s = scan.Scanner(t, profile=cuts if cyc else None, cycles=cyc, **kw)
        if force:
            s.force_exhaustive()
        feed(s)
        out.append(s.finish())
        s.close()
    same_scan(out[0], out[1])
    return out


MATRIX_CFG = {'amin_I': dict(KM.CONFIGS[8], Amin=b'I'), 'redo': dict(KM.CONFIGS[8]), 'families': dict(KM.CONFIGS[8])}


@pytest.mark.parametrize('mode', ['seeded', 'exhaustive', 'shared-index'])
@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_device_batch_of_the_trim_matrix(name, mode):
    text, co = matrix_texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr) if co is None else co
    seqs = TM.table() + ([b'ACGTNNACGTTGCAACGTACGTAGCTAGCTAA'] if mode == 'shared-index' else [])
    t = scan.Table(seqs, **MATRIX_CFG[name])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, co), force=mode == 'exhaustive')
    check_cycles(b, matrix_want(name))
    if mode == 'seeded':
        assert b['path']['seeded'] and len(b['hits']) > 100
    elif mode == 'exhaustive':
        assert b['path']['exhaustive'] and not b['path']['seeded']
    else:
        assert not t.seeded[-1] and b['path']['seeded'] and b['path']['exhaustive']
    if name == 'redo':
        assert b['profile'].last_cycle == 1023 and b['profile'].longest == 9000
    assert b['cycles_kernel_ms'] > 0 and 'cycles_kernel_ms' not in a
    d.free(); t.close()


def test_skipped_tiles_are_counted_once():
    text, co = matrix_texts()['redo']
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(TM.table(), **MATRIX_CFG['redo'])
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    a, b = scanner_pair(t, lambda s: s.scan_device(d.ptr, arr.nbytes, co))
    assert b['path']['tiles_rescanned'] and not b['path']['rescanned']
    check_cycles(b, matrix_want('redo'))
    d.free(); t.close()


@pytest.mark.parametrize('how', ['host', 'device'])
def test_the_seams_by_hand(how):
    text, co = seams_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table([b'ACGTACGTACGTACGTACGTACGTA'], **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    feed = (lambda s: s.scan_host(arr)) if how == 'host' else (lambda s: s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64)))
    a, b = scanner_pair(t, feed)
    check_cycles(b, want_of(text, co if how == 'device' else None))
    assert b['profile'].records == 21 and b['profile'].last_cycle == 1023
    d.free(); t.close()


def test_batches_add_up_and_a_reset_clears_them():
    g = synth.genome()
    t = scan.Table(synth.both_strands(synth.table(g)), **cases.PRODUCT)
    host = synth.reads(g, 0, 30000, 150)
    co = scan.chunk_offsets(host)
    assert len(co) > 3
    a, one = scanner_pair(t, lambda s: s.scan_host(host))
    half = int(co[len(co) // 2])
    a2, two = scanner_pair(t, lambda s: (s.scan_host(host[:half]), s.scan_host(host[half:], fpos_base=half)))
    want = want_of(host.tobytes())
    check_cycles(one, want); check_cycles(two, want)
    assert two['hits'] == one['hits'] and one['profile'].records == 30000 and one['profile'].last_cycle == 149
    # cycles alone: a profile with no cutoffs; the same handle again after a reset counts from zero
    s = scan.Scanner(t, cycles=True)
    s.scan_host(host); r = s.finish()
    assert r['profile'].cutoffs == [] and (r['profile'].cycles == want[0].cycles).all()
    s.reset()
    s.scan_host(host[:half]); r = s.finish()
    check_cycles(r, want_of(host[:half].tobytes(), cuts=[]))
    s.close(); t.close()


def test_cold_bytes_cost_speed_never_results():
    t = scan.Table([b'ACGTACGTACGTACGTACGTACGTA'], **cases.DEFAULTS)
    for text in cold_texts():
        arr = np.frombuffer(text, dtype=np.uint8)
        a, b = scanner_pair(t, lambda s: s.scan_host(arr))
        check_cycles(b, want_of(text))
        assert b['profile'].records == 300 and b['profile'].last_cycle == 299
    t.close()


@pytest.mark.parametrize('every', [False, True])
def test_a_batch_whose_speculation_fails_is_counted_once(every):
    from test_gpu_parity import QUIRK_CFG, _quirk_text
    data = np.frombuffer(b''.join(_quirk_text(0, every)), dtype=np.uint8)
    t = scan.Table(synth.both_strands([cases.QUIRK_SEQ.encode()]), **QUIRK_CFG)
    a, b = scanner_pair(t, lambda s: s.scan_host(data))
    assert b['path']['rescanned'] == every and len(b['hits']) > 100
    check_cycles(b, want_of(data.tobytes()))
    assert b['profile'].records == 4000
    t.close()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_arena_overflow_counts_every_record_once(how):
    """2.4 M hits: the arena overflows; the library replays a device batch, Scanner feeds host batches again"""
    from test_gpu_profile import _dense
    arr = _dense()
    want = want_of(arr.tobytes())
    t = scan.Table([b'ACG'], **dict(cases.DEFAULTS, minreadlength=10))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = scan.chunk_offsets(arr)
    res = []
    for cyc in (False, True):
        s = scan.Scanner(t, profile=CUTS if cyc else None, cycles=cyc)
        if how == 'host':
            s.scan_host(arr)
        else:
            s.scan_device(d.ptr, arr.nbytes, co)
        res.append(s.finish(hits=False))
        s.close()
    a, b = res
    assert a['n_hits'] == b['n_hits'] == 40000 * 60
    assert (a['counters'] == b['counters']).all() and a['stats'] == b['stats'] and a['path'] == b['path']
    check_cycles(b, want)
    assert b['profile'].records == 40000 and int(b['profile'].cycle_bases[0, ord('A')]) == 40000
    d.free(); t.close()


def findseqs_pair(files, seqs, inflate='host', route=None):
    arg = files[0] if len(files) == 1 else files
    a = engine.findseqs(arg, seqs, inflate=inflate)
    b = engine.findseqs(arg, seqs, inflate=inflate, profile=CUTS, cycles=True)
    if route:
        assert engine.last_inflate() == route
    assert 'profile' not in a
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats']
    assert b['profile'].records == b['stats']['records_parsed']
    return b


def test_every_route_gives_the_cycles_of_its_text(tmp_path):
    case = cases.by_name()['multichunk']
    text = cases.multichunk()
    engine.config(**case.config)
    seqs = case.seq_bytes()
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'h.fastq.gz').write_bytes(gzip.compress(text, 1, mtime=0))
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
    want, facts = want_of(text)
    assert want.records > 8000
    for name, inflate, route in (('m.fastq', 'host', 'host'), ('h.fastq.gz', 'host', 'host'), ('b.fastq.gz', 'device', 'device'),
                                 ('g.fastq.gz', 'device_any', 'device_gzip')):
        r = findseqs_pair([str(tmp_path / name)], seqs, inflate, route)
        assert r['profile'] == want and r['profile'].cycles is not None, name
        CR.check_identities(r['profile'].cycles, r['profile'].words, facts)
    # the same files again without the cycles: the kept scan object gives them up
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile=CUTS)
    assert r['profile'].cycles is None and (r['profile'].words == want.words).all()
    # BAM: the cycles of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    r = findseqs_pair([str(tmp_path / 'm.bam')], seqs, route='device_bam')
    vwant, vfacts = want_of(vtext)
    assert r['profile'] == vwant and r['profile'].records > 8000
    CR.check_identities(r['profile'].cycles, r['profile'].words, vfacts)
    assert bam.Bam(str(tmp_path / 'm.bam')).profile(cutoffs=CUTS, cycles=True) == vwant
    # profile-only calls
    assert P.profile(str(tmp_path / 'm.fastq'), cutoffs=CUTS, cycles=True) == want
    assert engine.findseqs(str(tmp_path / 'm.fastq'), [], cycles=True)['profile'].cutoffs == []


def test_analyser_and_command_line(fastqs):
    engine.config(**cases.PRODUCT)
    path = os.path.join(fastqs, 'test_analyser.fastq')
    fq = Fastq(path, quiet=True)
    with open(path, 'rb') as f:
        want, facts = want_of(f.read(), cuts=[ord('.')])
    templates = {str(i): s for i, s in enumerate(synth.SPOLIGO_SPACERS)}
    a = analyse.Analyser()
    a.scan(fq, templates, profile='.', cycles=True)
    assert a.profile == want
    info = a.encode()['info']['profile']
    assert len(info['cycles']['score']) == want.last_cycle + 1 and info['cycles'] == want.as_dict()['cycles']
    b = analyse.Analyser()
    b.scan(fq, templates, profile='.')
    assert b.profile.cycles is None and 'cycles' not in b.encode()['info']['profile'] and b.hits == a.hits
    assert fq.profile(cycles=True) == want
    import contextlib, io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([path, '--cycles', '--cycle-step', '10'])
    assert out.getvalue().strip() == want.summary() + '\n' + '\n'.join(want.cycle_lines(10))
    assert out.getvalue().count('\n') == len(want.summary().splitlines()) + 1 + (want.last_cycle + 10) // 10


def test_refusals_and_off():
    L = _lib.lib()
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    arr = np.frombuffer(cases.rec('a', 'ACGTACGTACGT' * 3, 'I' * 36), dtype=np.uint8)
    # no profile: no cycles
    s = scan.Scanner(t)
    assert L.kvq_scan_set_cycles(s.h, 1) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_cycles(s.h, 0) == 0
    # only before the first batch or after a reset
    assert L.kvq_scan_set_profile(s.h, None, 0) == 0
    s.scan_host(arr)
    assert L.kvq_scan_set_cycles(s.h, 1) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    s.finish()
    assert not L.kvq_scan_cycles(s.h) and L.kvq_scan_cycles_kernel_ms(s.h) == 0
    s.reset()
    assert L.kvq_scan_set_cycles(s.h, 1) == 0
    s.scan_host(arr); s.finish()
    words = np.ctypeslib.as_array(L.kvq_scan_cycles(s.h), shape=(CR.LEN,))
    assert (words == CR.cycles(arr.tobytes(), [0, arr.nbytes])).all() and words.sum() == 72
    # the profile off takes the cycles with it
    s.reset()
    assert L.kvq_scan_set_profile(s.h, None, -1) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_cycles(s.h) and not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_cycles(s.h, 1) == _lib.ERR_RUNTIME
    s.close()
    # a profile without cycles
    s = scan.Scanner(t, profile='.')
    s.scan_host(arr); r = s.finish()
    assert r['profile'].cycles is None and not L.kvq_scan_cycles(s.h) and 'cycles_kernel_ms' not in r
    s.close()
    # the flag of kvq_findseqs_opts without the profile's
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_CYCLES, 0, (C.c_uint8 * 8)())
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    t.close()
