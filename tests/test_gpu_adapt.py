"""
The adapter content on an MI355X (``kvq_adapt_records``; include/kvarq_hip.h): the device array against the
CPU twin (``kvq_adapt_host``), which tests/test_adapt_host.py ties to the plain statement of the definition, word for word -- on
every seam text of tests/adapt_ref.py (each asserts its census first), under cuts of the batches, on every way a batch's text
reaches ``run_batch``, beside every other pass, through a rescan and a reset.  A scan with the option gives the hits, stats and
counters of the same scan without it.
"""
import ctypes as C
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adapt_ref as A
import bam_writer as W
import cases
import kernel_matrix as KM
import trim_matrix as TM
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

SEQ = [b'ACGTACGTACGTACGTACGTACGTA']
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'adapt_child.py')


@functools.lru_cache(maxsize=None)
def _want(text, co, probes):
    return P.profile_host(text, (), list(co), adapters=list(probes))


def want_of(text, probes, chunk_off=None):
    """the twin's profile of a text with these probes; computed once per text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    return _want(text, tuple(int(c) for c in co), tuple(probes))


def check_adapt(r, twin):
    got = r['profile']
    assert got.adapters is not None
    bad = np.nonzero(got.adapters.words != twin.adapters.words)[0]
    assert bad.size == 0, (bad[:8], got.adapters.words[bad[:8]], twin.adapters.words[bad[:8]])
    assert got.adapters == twin.adapters and got.adapters.probes == twin.adapters.probes
    assert (got.words == twin.words).all() and got.records == r['counters'][_lib.CTR_RECORDS]
    A.check_identities(got.adapters.words, got.words)              # the profile of the same scan: another kernel's count
    assert r['adapt_kernel_ms'] > 0 or got.records == 0


def record_ends(text):
    return [n3 + 1 for _, _, _, n3 in A.R.records_of(text, [0, len(text)])]


@pytest.mark.parametrize('name', sorted(A.texts()))
def test_every_seam_text_as_one_batch_and_as_three(name):
    """a device batch whose buffer ends with the text's last byte, then the same text as three host batches cut between records"""
    A.check_census(name)
    text, probes = A.texts()[name]
    twin = want_of(text, probes, [0, len(text)])
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array([0, len(text)], dtype=np.int64)
    t = scan.Table(SEQ, **cases.DEFAULTS)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    plain = scan.Scanner(t)
    plain.scan_device(d.ptr, arr.nbytes, co)
    a = plain.finish()
    plain.close()
    s = scan.Scanner(t, adapters=probes)
    s.scan_device(d.ptr, arr.nbytes, co)
    one = s.finish()
    check_adapt(one, twin)
    assert one['hits'] == a['hits'] and one['stats'] == a['stats'] and (one['counters'] == a['counters']).all() and 'adapt_kernel_ms' not in a
    if name == 'none':
        assert (one['profile'].adapters.clip == one['profile'].raw_lengths).all()
    ends = record_ends(text)
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    s.reset()
    for x, y in zip(cuts, cuts[1:]):
        s.scan_host(arr[x:y], chunk_off=[0, y - x], fpos_base=x)
    three = s.finish()
    check_adapt(three, twin)
    assert three['profile'] == one['profile']
    s.close(); d.free(); t.close()


def test_random_records_and_a_second_scan_after_a_reset():
    text, probes = A.random_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **cases.DEFAULTS)
    s = scan.Scanner(t, adapters=probes)
    s.scan_host(arr, chunk_off=[0, len(text)])
    first = s.finish()
    check_adapt(first, want_of(text, probes, [0, len(text)]))
    # a reset and a part of the text: nothing is carried over
    cut = record_ends(text)[699]
    s.reset()
    s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut])
    second = s.finish()
    check_adapt(second, want_of(text[cut:], probes, [0, len(text) - cut]))
    assert second['profile'].adapters.records == 1300
    s.reset()
    s.scan_host(arr, chunk_off=[0, len(text)])
    assert s.finish()['profile'] == first['profile']
    s.close(); t.close()


@pytest.mark.parametrize('mode', ['seeded', 'exhaustive', 'long_reads'])
def test_every_path_of_a_device_batch(mode):
    """the 12 kb lines, the round seams and the '\\r' lines on the seeded path, the exhaustive kernels and the read-list route"""
    probes = [A.P12, A.P32]
    text = b''.join(A.texts()[n][0] for n in ('edges', 'cr', 'every_start'))
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr)
    t = scan.Table(TM.table(), **dict(KM.CONFIGS[8]))
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    s = scan.Scanner(t, adapters=probes, **({'long_reads': True} if mode == 'long_reads' else {}))
    if mode == 'exhaustive':
        s.force_exhaustive()
    s.scan_device(d.ptr, arr.nbytes, co)
    r = s.finish()
    check_adapt(r, want_of(text, probes, co))
    if mode == 'exhaustive':
        assert r['path']['exhaustive'] and not r['path']['seeded']
    elif mode == 'long_reads':
        assert r['path']['read_list']
    s.close(); d.free(); t.close()


def test_every_route_of_findseqs(tmp_path):
    probes = [A.P12, A.P32]
    named = dict(zip(('short', 'long'), probes))
    text = b''.join(A.texts()[n][0] for n in ('every_start', 'edges', 'cr', 'aliases'))
    case = cases.by_name()['multichunk']
    engine.config(**case.config)
    seqs = case.seq_bytes()
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'h.fastq.gz').write_bytes(gzip.compress(text, 1, mtime=0))
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    want = want_of(text, probes)
    assert want.adapters.with_adapter > 700 and want.adapters.tail_only >= 5 and want.adapters.beyond.sum() >= 3
    plain = engine.findseqs(str(tmp_path / 'm.fastq'), seqs)
    for name, kw, route in (('m.fastq', {}, 'host'), ('h.fastq.gz', {}, 'host'), ('b.fastq.gz', {'inflate': 'device'}, 'device'),
                            ('m.fastq', {'long_reads': True}, 'host')):
        r = engine.findseqs(str(tmp_path / name), seqs, adapters=named, **kw)
        assert engine.last_inflate() == route
        p = r['profile']
        assert p.cutoffs == [] and p.adapters == want.adapters and p.adapters.names == ['short', 'long'] and (p.words == want.words).all(), (name, kw)
        assert r['hits'] == plain['hits'] and r['stats'] == plain['stats']
        A.check_identities(p.adapters.words, p.words)
    # the same file read again with every other pass beside it, and without the option, which the kept scan object then gives up
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile='I', adapters=probes, duplication=True, cycles=True, per_read=True, overrepresented=True)
    assert r['profile'].adapters == want.adapters and r['profile'].cycles is not None and r['profile'].over is not None
    r = engine.findseqs(str(tmp_path / 'm.fastq'), seqs, profile='I')
    assert r['profile'].adapters is None and 'adapters' not in r['profile'].as_dict()
    # BAM: the adapter content of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    vwant = want_of(vtext, probes)
    r = engine.findseqs(str(tmp_path / 'm.bam'), seqs, adapters=probes)
    assert engine.last_inflate() == 'device_bam' and r['profile'].adapters == vwant.adapters and vwant.adapters.with_adapter > want.adapters.with_adapter
    assert bam.Bam(str(tmp_path / 'm.bam')).profile(cutoffs='I', adapters=probes).adapters == vwant.adapters
    # profile-only calls, and the known adapters
    assert P.profile(str(tmp_path / 'm.fastq'), cutoffs=(), adapters=probes) == want
    known = P.profile(str(tmp_path / 'm.fastq'), adapters=True).adapters
    assert known == P.adapt_host(text, True, O.chunk_offsets(text)) and known.names[0] == 'Illumina universal adapter' and known.found[0] > 700


def test_beside_every_other_pass():
    """with every other pass on at once the adapter array is unchanged, and the other arrays are what they are without it"""
    text, probes = A.texts()['shapes']
    text = text + A.texts()['tails'][0]
    arr = np.frombuffer(text, dtype=np.uint8)
    co = [0, len(text)]
    t = scan.Table(SEQ, **cases.DEFAULTS)
    others = dict(profile='5I', cycles=True, per_read=True, duplication=True, overrepresented=True)
    res = []
    for kw in (dict(adapters=probes), others, dict(others, adapters=probes)):
        s = scan.Scanner(t, **kw)
        s.scan_host(arr, chunk_off=co)
        res.append(s.finish())
        s.close()
    alone, without, both = res
    assert both['profile'].adapters == alone['profile'].adapters == want_of(text, probes, co).adapters
    assert without['profile'].adapters is None and 'adapt_kernel_ms' not in without
    a, b = without['profile'], both['profile']
    assert (a.words == b.words).all() and (a.cycles == b.cycles).all() and (a.reads == b.reads).all() and a.duplication == b.duplication
    assert (a.over == b.over).all() and both['hits'] == without['hits'] and (both['counters'] == without['counters']).all()
    t.close()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_arena_overflow_counts_every_record_once(how, tmp_path):
    """an arena of 64 hits overflows (KVQ_ARENA_CAP, read when the scan object is made: a process of its own): the library
    replays a device batch, Scanner feeds host batches again -- every record counts once"""
    read = 'ACG' * 60
    probes = [A.P12, A.P32]
    text = (cases.rec('x', read, 'I' * len(read)) * 300 + cases.rec('y', read[:100] + A.P12.decode() + 'CT' * 10, 'I' * 132) * 200 +
            cases.rec('z', 'GGCC' * 20 + A.P32.decode()[:9], '5' * 89) * 3)
    (tmp_path / 't.fastq').write_bytes(text)
    job, res = str(tmp_path / 'job.json'), str(tmp_path / 'res.npz')
    with open(job, 'w') as f:
        json.dump(dict(text=str(tmp_path / 't.fastq'), seqs=['ACG'], cfg=dict(cases.DEFAULTS, minreadlength=10), probes=[p.decode() for p in probes],
                       how=how, result=res), f)
    p = subprocess.run([sys.executable, CHILD, job], env=dict(os.environ, KVQ_ARENA_CAP='64'), capture_output=True, text=True, timeout=120)
    said = p.stdout + p.stderr
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
        pytest.exit('the child ended with status %d\n%s' % (p.returncode, said), 1)
    assert p.returncode == 0 and 'adapt child ok' in p.stdout, said
    z = np.load(res)
    twin = want_of(text, probes)
    assert int(z['n_hits']) > 64 * 100 and int(z['records']) == 503
    assert (z['adapt'] == twin.adapters.words).all() and (z['words'] == twin.words).all()
    assert twin.adapters.found[0] == 200 and twin.adapters.tail[1, 9] == 3 and twin.adapters.clip[100] == 200


def test_refusals_and_off():
    L = _lib.lib()
    t = scan.Table([b'ACGTACGTACGT'], **cases.PRODUCT)
    arr = np.frombuffer(cases.rec('a', 'CC' + A.P12.decode() + 'TTTT', 'I' * 18) * 2, dtype=np.uint8)
    one = (C.c_char_p * 1)(A.P12)
    len1 = (C.c_int32 * 1)(12)
    # no profile: no option
    s = scan.Scanner(t)
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_adapters(s.h, None, None, 0) == 0
    # only before the first batch or after a reset
    assert L.kvq_scan_set_profile(s.h, None, 0) == 0
    s.scan_host(arr)
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    r = s.finish()
    assert not L.kvq_scan_adapters(s.h) and L.kvq_scan_adapt_kernel_ms(s.h) == 0 and 'adapt_kernel_ms' not in r
    assert P.from_scan(L, s.h).adapters is None
    s.reset()
    # refused probes leave the option as it was: off
    for probe, n in ((b'ACGTACG', 1), (b'A' * 33, 1), (b'ACGTACGa', 1), (b'ACGTNCGT', 1), (A.P12, 9), (A.P12, -1)):
        k = max(n, 1)
        assert L.kvq_scan_set_adapters(s.h, (C.c_char_p * k)(*[probe] * k), (C.c_int32 * k)(*[len(probe)] * k), n) == _lib.ERR_RUNTIME
        assert 'upper-case A C G T' in _lib.last_error()[1]
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == 0
    assert not L.kvq_scan_adapters(s.h)                            # (not finished)
    s.scan_host(arr); s.finish()
    words = np.ctypeslib.as_array(L.kvq_scan_adapters(s.h), shape=(A.LEN,))
    assert (words == A.adapt(arr.tobytes(), [0, arr.nbytes], [A.P12])).all() and words[A.BLOCKS + A.B_FIRST_BINS + 2] == 2 and words[A.CLIP + 2] == 2
    assert L.kvq_scan_adapt_kernel_ms(s.h) > 0
    # off again; the profile off takes it along
    s.reset()
    assert L.kvq_scan_set_adapters(s.h, None, None, 0) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_adapters(s.h) and L.kvq_scan_adapt_kernel_ms(s.h) == 0 and L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == 0 and L.kvq_scan_set_profile(s.h, None, -1) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_adapters(s.h) and not L.kvq_scan_profile(s.h)
    s.reset()
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == _lib.ERR_RUNTIME
    s.close()
    # with a communicator: the scan keeps no profile, so no option (the rule is the profile's, inherited)
    comm = L.kvq_comm_create_local(1, 0, 0x61646170)
    assert comm
    s = scan.Scanner(t, adapters=[A.P12])
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    s.close()
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_adapters(s.h, one, len1, 1) == _lib.ERR_RUNTIME and 'keeps no profile' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    s.close()
    L.kvq_comm_destroy(comm)
    # the flag of kvq_findseqs_opts / kvq_findseqs_ex: without the profile's, and without the structure that holds the probes
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_ADAPTERS, 0, (C.c_uint8 * 8)())
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_ADAPTERS)
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'KVQ_FIND_PROFILE' in _lib.last_error()[1]
    opts.flags = _lib.FIND_ADAPTERS | _lib.FIND_PROFILE
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_ADAPTERS | _lib.FIND_PROFILE)
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    big = _lib.FindOptsAdapters(_lib.FindOpts(C.sizeof(_lib.FindOptsAdapters), _lib.FIND_ADAPTERS | _lib.FIND_PROFILE, 0, (C.c_uint8 * 8)()), 0)
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.cast(C.byref(big), C.POINTER(_lib.FindOpts)))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and '1 to 8 probes' in _lib.last_error()[1]
    t.close()
