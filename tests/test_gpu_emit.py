"""
The emitted reads on an MI355X (kernels_emit.hip; include/kvarq_hip.h).  Byte for byte: what a scan with
``emit=`` hands back is EMIT(text) as the CPU twin makes it (tests/test_emit_host.py ties the twin to the plain statement), the
eight words are the twin's, and the guard bytes on either side of the device store are untouched.  On the texts of
tests/emit_ref.py -- every (source, destination, length) of the copy, the trim at its seams, the record counts at the seams of the
prefix sum --, on every path a batch can take (seed filter, exhaustive kernels, read list, the redo of skipped tiles, the redo of
a whole batch, a rescan after an arena overflow, a reset, several batches), beside the records, the profile and the clip, through
every route of ``findseqs``; and the round trip: the emitted text, scanned again, gives the same hits.
"""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_writer as W
import clip_ref as CR
import emit_ref as E
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

PROBES = CR.PROBES[2]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv('KVQ_ARENA_CAP', raising=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, chunk offsets, sequences, config)"""
    if name == 'copies':
        text = E.copies_text()[0]
    elif name == 'trims':
        text = E.trims_text()[0]
    elif name == 'dropped':
        text = E.dropped_text()
    elif name == 'empty-chunks':
        text, co = E.empty_chunk_case()
        return text, co, tuple(E.SEQ), E.CFG
    elif name.startswith('counts-'):
        text = E.counts_text(int(name[7:]))
    elif name == 'reveal':
        text = CR.reveal_text()[0]
        return text, tuple(O.chunk_offsets(text)), tuple(CR.TM.table()), E.CFG
    elif name == 'redo':
        text, _, _, co = CR.redo_text()
        return text, co, tuple(CR.TM.table()), E.CFG
    else:
        text = CR.quirk_text()
        return text, tuple(O.chunk_offsets(text)), tuple(CR.quirk_seqs()), CR.QUIRK_CFG
    return text, (0, len(text)), tuple(E.SEQ), E.CFG


def amin_of(cfg):
    return cfg['Amin'] if isinstance(cfg['Amin'], int) else (cfg['Amin'].encode('latin-1') if isinstance(cfg['Amin'], str) else cfg['Amin'])[0]


@functools.lru_cache(maxsize=None)
def twin(name, min_length=None, clip=False):
    """(EMIT(text) -- of MASK(text) with ``clip`` -- as an array, the eight words) by the CPU twin; computed once, left unchanged"""
    text, co, _, cfg = case(name)
    m = cfg['minreadlength'] if min_length is None else min_length
    if clip:
        text = P.clip_host(text, PROBES, list(co))[0]
    out, words = P.emit_host(text, amin_of(cfg), m, list(co))
    out.flags.writeable = False; words.flags.writeable = False
    return out, words


@functools.lru_cache(maxsize=None)
def oracle(name):
    text, _, seqs, cfg = case(name)
    return O.scan_memory(np.frombuffer(text, dtype=np.uint8), list(seqs), fold=True, **dict(cfg, nthreads=4))


def same_as_oracle(r, o):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], k


def check_emit(r, want, words, scanner=None):
    """the emitted bytes and the eight words are the twin's, the identities hold, the guards are whole"""
    got, e = r['emitted'], r['emit']
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.shape, want.shape, e.words, words)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert (e.words == words).all(), (e.words, words)
    E.check_identities(e.words, got.size)
    assert e.records == int(r['counters'][_lib.CTR_RECORDS]) and e['bytes_out'] == got.size
    assert r['emit_kernel_ms'] > 0 or e.records == 0
    if scanner is not None:
        assert _lib.lib().kvq_scan_emit_guard(scanner.h) == 0


def upload(arr, guard=64):
    d = scan.DeviceBuffer(arr.nbytes + guard - 64)
    d.upload(np.concatenate([arr, np.full(guard, 0xAA, dtype=np.uint8)]))
    return d


def scan_device(t, arr, co, guard=64, exhaustive=False, **kw):
    """-> (result, the buffer's bytes after the scan); the guards of the emit's store are checked here"""
    d = upload(arr, guard)
    s = scan.Scanner(t, **kw)
    if exhaustive:
        s.force_exhaustive()
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    r = s.finish()
    if kw.get('emit'):
        assert _lib.lib().kvq_scan_emit_guard(s.h) == 0
    s.close()
    after = d.download(arr.nbytes + guard)
    d.free()
    return r, after


# ---- byte for byte ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,m', [('copies', 0), ('trims', None), ('trims', 0), ('trims', 1), ('dropped', None), ('empty-chunks', None), ('reveal', None), ('reveal', 0)])
def test_byte_for_byte(name, m):
    if name == 'copies':
        E.copies_census()
    elif name == 'trims':
        E.trims_census()
    elif name == 'dropped':
        E.dropped_census()
    text, co, seqs, cfg = case(name)
    want, words = twin(name, m)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    kw = dict(emit=True) if m is None else dict(emit=True, emit_min=m)
    # the batch's text is only read: it and the 64 bytes of 0xAA behind it are what they were
    r, after = scan_device(t, arr, co, **kw)
    check_emit(r, want, words)
    assert (after[:arr.nbytes] == arr).all() and (after[arr.nbytes:] == 0xAA).all()
    assert r['emit'].min_length == (cfg['minreadlength'] if m is None else m)
    if name == 'dropped':
        assert r['emitted'].size == 0 and r['emit'].emitted == 0 and r['emit'].records == 600
    # a buffer that ends on the text's last byte, and the exhaustive kernels
    r, after = scan_device(t, arr, co, guard=0, exhaustive=True, **kw)
    check_emit(r, want, words)
    assert (after == arr).all()
    t.close()


@pytest.mark.parametrize('n', E.COUNTS)
def test_the_seams_of_the_prefix_sum(n):
    E.counts_census(n)
    name = 'counts-%d' % n
    text, co, seqs, cfg = case(name)
    want, words = twin(name)
    assert words[E.RECORDS] == n
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, np.frombuffer(text, dtype=np.uint8), co, emit=True)
    check_emit(r, want, words)
    t.close()


def test_emit_off_returns_nothing():
    text, co, seqs, cfg = case('reveal')
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, np.frombuffer(text, dtype=np.uint8), co)
    assert 'emit' not in r and 'emitted' not in r and 'emit_kernel_ms' not in r
    s = scan.Scanner(t)
    L = _lib.lib()
    assert not L.kvq_scan_emit(s.h) and L.kvq_scan_emit_kernel_ms(s.h) == 0 and L.kvq_scan_emit_guard(s.h) == -1
    ptr, n = C.c_void_p(), C.c_int64()
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == _lib.ERR_RUNTIME
    s.close(); t.close()


# ---- every path a batch can take ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('route', ['seeded', 'exhaustive', 'long_reads', 'tiles_rescanned', 'rescanned'])
def test_on_every_path(route):
    """the emit is the twin's whatever kernels scan the batch, and the scan is what it is without the emit"""
    name = {'tiles_rescanned': 'redo', 'rescanned': 'quirk'}.get(route, 'reveal')
    text, co, seqs, cfg = case(name)
    want, words = twin(name)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    kw = {'long_reads': True} if route == 'long_reads' else {}
    res = []
    for more in (dict(emit=True), {}):
        d = upload(arr)
        s = scan.Scanner(t, **dict(kw, **more))
        if route == 'exhaustive':
            s.force_exhaustive()
        if route == 'rescanned':
            s.scan_host(arr, chunk_off=list(co))
        else:
            s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        res.append(s.finish())
        if more:
            check_emit(res[-1], want, words, s)                      # (a batch that was redone as a whole is emitted once)
        s.close(); d.free()
    emitted, plain = res
    assert emitted['hits'] == plain['hits'] and emitted['hitseqs'] == plain['hitseqs'] and emitted['stats'] == plain['stats']
    assert (emitted['counters'] == plain['counters']).all() and emitted['path'] == plain['path']
    same_as_oracle(emitted, oracle(name))
    path = emitted['path']
    if route == 'seeded':
        assert path['seeded'] and not path['rescanned']
    elif route == 'exhaustive':
        assert path['exhaustive'] and not path['seeded']
    elif route == 'long_reads':
        assert path['read_list'] and not path['seeded']
    elif route == 'tiles_rescanned':
        assert path['seeded'] and path['tiles_rescanned'] and not path['rescanned']
        assert words[E.BASES_OUT] > 20000                            # (the long records of the skipped tiles are emitted too)
    else:
        assert path['rescanned'] and len(oracle(name)['hits']) > 50
    t.close()


@pytest.mark.parametrize('how', ['device', 'host', 'file'])
def test_a_rescan_after_an_arena_overflow_emits_once(how, monkeypatch, tmp_path):
    """an arena of 64 hits overflows: the library replays a device batch, Scanner feeds host batches again -- the sink was emptied
    with the arena (a file: truncated), and the text is there once"""
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    text, co, seqs, cfg = case('reveal')
    want, words = twin('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    out = str(tmp_path / 'out.fastq')
    s = scan.Scanner(t, emit=out if how == 'file' else True)
    assert s.order_info()['arena_cap'] == 64
    d = upload(arr)
    if how == 'device':
        s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    else:
        cut = E.record_ends(text)[300]
        s.scan_host(arr[:cut], chunk_off=[0, cut])
        s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut], fpos_base=cut)
    r = s.finish()
    assert s.order_info()['arena_cap'] > 64 and len(r['hits']) > 100
    same_as_oracle(r, oracle('reveal'))
    if how == 'file':
        assert 'emitted' not in r and (r['emit'].words == words).all() and _lib.lib().kvq_scan_emit_guard(s.h) == 0
        s.close()
        with open(out, 'rb') as f:
            assert f.read() == want.tobytes()
    else:
        check_emit(r, want, words, s)
        s.close()
    d.free(); t.close()


def test_a_reset_carries_nothing_over_and_batches_add_up():
    text, co, seqs, cfg = case('reveal')
    want, words = twin('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    s = scan.Scanner(t, emit=True)
    # three host batches cut between records, the middle one of two chunks
    ends = E.record_ends(text)
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    for i, (x, y) in enumerate(zip(cuts, cuts[1:])):
        mid = ends[len(ends) // 2] - x
        s.scan_host(arr[x:y], chunk_off=[0, mid, y - x] if i == 1 else [0, y - x], fpos_base=x)
    first = s.finish()
    check_emit(first, want, words, s)
    same_as_oracle(first, oracle('reveal'))
    # a reset, and only the tail of the text
    cut = ends[299]
    pw, pwords = P.emit_host(text[cut:], E.AMIN, E.MINLEN, [0, len(text) - cut])
    s.reset()
    s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut])
    second = s.finish()
    check_emit(second, pw, pwords, s)
    assert second['emit'].records == first['emit'].records - 300
    s.reset()
    s.scan_host(arr, chunk_off=list(co))
    again = s.finish()
    check_emit(again, want, words, s)
    assert again['emit'] == first['emit'] and again['hits'] == first['hits']
    s.close(); t.close()


def test_where_one_workgroup_walks_all_the_tiles(tmp_path):
    """KVQ_GRID=1 is read once per process: a child scans `reveal` with the emit on and hands back what it got"""
    text, co, seqs, cfg = case('reveal')
    want, words = twin('reveal')
    (tmp_path / 'reveal.fastq').write_bytes(text)
    res = str(tmp_path / 'res.npz')
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, 'emit_grid_child.py'), str(tmp_path / 'reveal.fastq'), res],
                           env=dict(os.environ, KVQ_GRID='1'), capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.exit('the emit child under KVQ_GRID=1 did not end within 120 s\n%s\n%s' % (e.stdout, e.stderr), 1)
    said = p.stdout + p.stderr
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
        pytest.exit('the emit child under KVQ_GRID=1 ended with status %d\n%s' % (p.returncode, said), 1)
    assert p.returncode == 0 and 'emit grid child ok' in p.stdout, said
    z = np.load(res)
    assert int(z['grid']) == 1 and bool(z['seeded']) and int(z['guard']) == 0
    assert (z['emitted'] == want).all() and (z['words'] == words).all()
    o = oracle('reveal')
    assert z['file_pos'].tolist() == [h.file_pos for h in o['hits']] and z['readlength'].tolist() == [h.readlength for h in o['hits']]


# ---- beside the other options ------------------------------------------------------------------------------------------------------

def test_beside_the_records():
    text, co, seqs, cfg = case('reveal')
    want, words = twin('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, arr, co, emit=True, records=True)
    check_emit(r, want, words)
    plain, _ = scan_device(t, arr, co, records=True)
    assert r['records'] == plain['records'] and len(r['records']) == len(r['hits']) > 100
    t.close()


def test_beside_the_profile():
    """with emit_min 0 and the cutoff Amin the histogram of the emitted read lengths is the profile's for that cutoff, and the
    scan's ``readlengths`` -- with the clip on too, whose masked text has reads of every length down to none"""
    text, co, seqs, cfg = case('reveal')
    want, words = twin('reveal', 0, clip=True)
    masked = P.clip_host(text, PROBES, list(co))[0]
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, arr, co, emit=True, emit_min=0, profile=[E.AMIN], cycles=True, clip=PROBES)
    check_emit(r, want, words)
    p = r['profile']
    assert p == P.profile_host(masked, [E.AMIN], list(co), cycles=True)
    assert r['emit'].records == p.records == r['emit'].emitted and r['emit'].mismatched == 0 and r['emit'].bases_in == int((np.arange(1025) * p.raw_lengths).sum())
    lengths = [len(b) for b in r['emitted'].tobytes().split(b'\n')[1::4]]
    hist = np.bincount(lengths, minlength=max(lengths) + 1)
    assert tuple(int(v) for v in hist) == tuple(p.readlengths(E.AMIN)) == tuple(r['stats']['readlengths'])
    assert hist[0] >= 5 and hist[1] >= 5 and hist[:E.MINLEN].sum() > 20       # (reads the default min_length drops)
    # ... and with the default min_length the short ones are counted, not written
    r, _ = scan_device(t, arr, co, emit=True, profile=[E.AMIN], clip=PROBES)
    check_emit(r, *twin('reveal', None, clip=True))
    assert r['emit'].short == hist[:E.MINLEN].sum() and r['emit'].emitted == hist[E.MINLEN:].sum()
    t.close()


@pytest.mark.parametrize('per', [None, 10])
def test_beside_the_clip(per):
    """the contract: the emit of the text with the clip on is the emit of MASK(text) without it"""
    text, co, seqs, cfg = case('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    kw = {} if per is None else dict(adapter_mismatches=per)
    masked, cwords = P.clip_host(text, PROBES, list(co), **kw)
    want, words = P.emit_host(masked, E.AMIN, E.MINLEN, list(co))
    assert (want.size, words.tolist()) != (twin('reveal')[0].size, twin('reveal')[1].tolist())
    t = scan.Table(list(seqs), **cfg)
    r, after = scan_device(t, arr, co, emit=True, clip=PROBES, **kw)
    check_emit(r, want, words)
    assert (r['clip'].words == cwords).all() and (after[:arr.nbytes] == masked).all()
    lines = r['emitted'].tobytes().split(b'\n')
    assert not any(b'!' in q for q in lines[3::4]) and not any(PROBES[0] in b for b in lines[1::4])
    # ... and the emit of the masked text, uploaded as it is
    r2, _ = scan_device(t, masked, co, emit=True)
    check_emit(r2, want, words)
    assert r2['hits'] == r['hits']
    t.close()


def test_every_route_of_findseqs(tmp_path):
    text, _, seqs, cfg = case('reveal')
    want, words = twin('reveal')
    saved = engine.get_config()
    engine.config(**cfg)
    try:
        (tmp_path / 'm.fastq').write_bytes(text)
        (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
        (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
        o = oracle('reveal')
        out = str(tmp_path / 'out.fastq')
        for name, kw, route in (('m.fastq', {}, 'host'), ('g.fastq.gz', {}, 'host'), ('b.fastq.gz', {'inflate': 'device'}, 'device'),
                                ('g.fastq.gz', {'inflate': 'device_any'}, 'device_gzip')):
            r = engine.findseqs(str(tmp_path / name), list(seqs), emit=out, **kw)
            assert engine.last_inflate() == route, (name, engine.last_inflate())
            assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs'], name
            assert (r['emit'].words == words).all() and r['emit_kernel_ms'] > 0 and 'emitted' not in r and 'profile' not in r, name
            with open(out, 'rb') as f:
                assert f.read() == want.tobytes(), name
            os.remove(out)
        # several files go to the one output, in order; emit_min as given
        want0, words0 = twin('reveal', 0)
        r = engine.findseqs([str(tmp_path / 'm.fastq'), str(tmp_path / 'g.fastq.gz')], list(seqs), emit=out, emit_min=0)
        with open(out, 'rb') as f:
            assert f.read() == want0.tobytes() * 2
        assert (r['emit'].words[1:] == 2 * words0[1:]).all() and r['emit'].min_length == 0
        # the next call has given the option up, and leaves the file alone
        plain = engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs))
        assert 'emit' not in plain and os.path.getsize(out) == 2 * want0.size
        # a profile-only call with the clip: trimmed, clipped FastQ and what was done
        masked = P.clip_host(text, PROBES, [0, len(text)])[0]
        cw, cwords = P.emit_host(masked, E.AMIN, E.MINLEN, [0, len(text)])
        p = P.profile(str(tmp_path / 'm.fastq'), cutoffs=[E.AMIN], clip=PROBES, emit=out)
        assert (p.emitted.words == cwords).all() and p.clipped.clipped > 600 and p.records == p.emitted.records
        with open(out, 'rb') as f:
            assert f.read() == cw.tobytes()
        # BAM: its virtual FastQ text, trimmed
        data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
        vtext = bam.to_fastq_host(data)
        vw, vwords = P.emit_host(vtext, E.AMIN, E.MINLEN, [0, len(vtext)])
        r = engine.findseqs(str(tmp_path / 'm.bam'), list(seqs), emit=out)
        assert engine.last_inflate() == 'device_bam' and (r['emit'].words == vwords).all() and vwords[E.EMITTED] > 600
        with open(out, 'rb') as f:
            assert f.read() == vw.tobytes()
        # a path that cannot be opened
        with pytest.raises(IOError):
            engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs), emit=str(tmp_path / 'no' / 'such' / 'dir.fastq'))
        with pytest.raises(ValueError):
            engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs), emit=True)
    finally:
        engine.config(**saved)


# ---- the round trip ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [False, True])
def test_the_emitted_text_scans_to_the_same_hits(clip):
    """every emitted read is its own trim: scanning the emitted text with the same table and config gives the same hits in the
    same order -- seq_nr, seq_pos, length, readlength and the hit bytes; file_pos counts another text's bytes -- and the oracle
    says the same of both texts"""
    text, co, seqs, cfg = case('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    src = P.clip_host(text, PROBES, list(co))[0] if clip else arr
    t = scan.Table(list(seqs), **cfg)
    r1, _ = scan_device(t, arr, co, emit=True, **(dict(clip=PROBES) if clip else {}))
    out = r1['emitted']
    assert max(len(b) for b in out.tobytes().split(b'\n')[1::4]) < 1024
    co2 = O.chunk_offsets(out.tobytes())
    r2, _ = scan_device(t, out, co2, emit=True)
    key = lambda hits: [(h.seq_nr, h.seq_pos, h.length, h.readlength) for h in hits]
    assert key(r1['hits']) == key(r2['hits']) and r1['hitseqs'] == r2['hitseqs'] and len(r1['hits']) > (600 if clip else 100)
    o1 = O.scan_memory(src, list(seqs), fold=True, **dict(cfg, nthreads=4))
    o2 = O.scan_memory(out, list(seqs), fold=True, **dict(cfg, nthreads=4))
    same_as_oracle(r1, o1); same_as_oracle(r2, o2)
    assert key(o1['hits']) == key(o2['hits']) and [h.file_pos for h in o1['hits']] != [h.file_pos for h in o2['hits']]
    # emitting the emitted text changes nothing but the names' '\r' (there is none) and the third lines (bare already)
    assert (r2['emitted'] == out).all() and r2['emit'].emitted == r2['emit'].records == r1['emit'].emitted
    t.close()


# ---- the options' rules ------------------------------------------------------------------------------------------------------------

def test_refusals_and_with_a_communicator(tmp_path):
    L = _lib.lib()
    arr = np.frombuffer(b'@r\nACGTACGT\n+\nIIII#III\n' * 2, dtype=np.uint8)
    t = scan.Table(E.SEQ, **E.CFG)
    s = scan.Scanner(t)
    # no profile needed; min_length < 0: the table's minreadlength; only before the first batch or after a reset
    assert L.kvq_scan_set_emit_fd(s.h, 1) == _lib.ERR_RUNTIME and 'kvq_scan_set_emit first' in _lib.last_error()[1]
    assert L.kvq_scan_set_emit(s.h, 1, 3) == 0 and not L.kvq_scan_emit(s.h)
    s.scan_host(arr)
    assert L.kvq_scan_set_emit(s.h, 0, 0) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    assert L.kvq_scan_set_emit_fd(s.h, -1) == _lib.ERR_RUNTIME
    ptr, n = C.c_void_p(), C.c_int64()
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == _lib.ERR_RUNTIME and 'finished' in _lib.last_error()[1]
    s.finish()
    assert np.ctypeslib.as_array(L.kvq_scan_emit(s.h), shape=(E.LEN,)).tolist() == [3, 2, 2, 0, 0, 16, 8, 2 * (2 + 4 + 4 + 5)]
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == 0 and C.string_at(ptr.value, n.value) == b'@r\nACGT\n+\nIIII\n' * 2
    s.reset()
    assert L.kvq_scan_set_emit(s.h, 1, -1) == 0
    s.scan_host(arr); s.finish()
    assert np.ctypeslib.as_array(L.kvq_scan_emit(s.h), shape=(E.LEN,)).tolist() == [E.MINLEN, 2, 0, 2, 0, 16, 0, 0]
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == 0 and n.value == 0
    s.reset()
    assert L.kvq_scan_set_emit(s.h, 0, 0) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_emit(s.h) and L.kvq_scan_emit_kernel_ms(s.h) == 0
    s.close()
    # with a communicator the emit is refused, either way round, as the records are
    comm = L.kvq_comm_create_local(1, 0, 0x656d6974)
    assert comm
    s = scan.Scanner(t)
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    assert L.kvq_scan_set_emit(s.h, 1, 0) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    s.close()
    s = scan.Scanner(t, emit=True)
    assert L.kvq_scan_set_comm(s.h, comm) == _lib.ERR_RUNTIME and 'across ranks' in _lib.last_error()[1]
    s.close()
    L.kvq_comm_destroy(comm)
    t.close()
    # the flag of kvq_findseqs_opts / kvq_findseqs_ex: refused without the structure that holds the path
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_EMIT, 0, (C.c_uint8 * 8)())
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_EMIT)
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    mm = _lib.FindOptsAdaptersMm(_lib.FindOptsAdapters(_lib.FindOpts(C.sizeof(_lib.FindOptsAdaptersMm), _lib.FIND_EMIT, 0, (C.c_uint8 * 8)()), 0), 0)
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.cast(C.byref(mm), C.POINTER(_lib.FindOpts)))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    big = _lib.FindOptsEmit(mm, 0, None)
    big.m.a.base.size = C.sizeof(_lib.FindOptsEmit)
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.cast(C.byref(big), C.POINTER(_lib.FindOpts)))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'path' in _lib.last_error()[1]
