"""
The read-list route on an MI355X (``long_reads``; kvq_scan_set_long_reads, ``kvq_seed_list``): every text
of tests/long_reads.py against the oracle and against the default route, through every way a text reaches ``run_batch``,
with the options that ride on a batch, in auto mode, and where the route must not be taken.
"""
import bisect
import ctypes as C
import gzip

import numpy as np
import pytest

import bam_writer as W
import cases
import long_reads as LR
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu


def feed_device(s, text, keep):
    arr = np.frombuffer(text, dtype=np.uint8)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr); keep.append(d)
    s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr))


def record_cuts(T):
    """the offsets at which the records of a text start, and its end"""
    cuts = [0]
    for p in T.parts:
        cuts.append(cuts[-1] + len(p))
    return cuts


def feed_host(s, T):
    """two host batches cut between records, the first of two chunks"""
    cuts, text = record_cuts(T), T.text
    n = len(T.parts)
    a, b = cuts[max(1, n // 4)], cuts[max(1, n // 2)]
    s.scan_host(np.frombuffer(text[:b], dtype=np.uint8), chunk_off=[0, a, b] if a < b else [0, b])
    s.scan_host(np.frombuffer(text[b:], dtype=np.uint8), chunk_off=[0, len(text) - b], fpos_base=b)


def run(T, long_reads, feed='device', table=None, **kw):
    t = table or scan.Table(T.seqs, **T.cfg)
    s = scan.Scanner(t, long_reads=long_reads, **kw)
    keep = []
    if feed == 'device':
        feed_device(s, T.text, keep)
    else:
        feed_host(s, T)
    r = s.finish()
    s.close()
    for d in keep:
        d.free()
    if table is None:
        t.close()
    return r


def same_as_oracle(r, o):
    assert tuple(r['hits']) == tuple(o['hits'])
    assert r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed', 'parsed', 'total'):
        assert r['stats'][k] == o['stats'][k], k
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations']
    assert int(r['counters'][_lib.CTR_HITS]) == len(o['hits'])


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats']
    assert (b['counters'] == a['counters']).all()


# ---- 1. every text and table ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('feed', ['device', 'host'])
@pytest.mark.parametrize('name', LR.NAMES)
def test_every_text_equals_the_oracle_and_the_default_route(name, feed):
    T, o = LR.text(name), LR.oracle(name)
    r = run(T, True, feed)
    same_as_oracle(r, o)
    LR.check_wanted(T, r['hits'])
    assert r['path']['read_list'] is True and r['path']['seeded'] is False
    assert r['path']['exhaustive'] == (name == 'with_n') and not r['path']['rescanned'] and not r['path']['tiles_rescanned']
    assert r['main_kernel_launches'] == (1 if feed == 'device' else 2)
    d = run(T, False, feed)
    assert 'read_list' not in d['path'] and sorted(d['path']) == ['exhaustive', 'rescanned', 'seeded', 'tiles_rescanned']
    same_scan(d, r)


# ---- 2. the golden cases ----------------------------------------------------------------------------------------------

def _outcome(f):
    try:
        return ('ok', f())
    except Exception as e:                                  # (a malformed file is refused the same way on both routes)
        return ('error', type(e), str(e))


SEEDED_CASES = [c.name for c in cases.all_cases() if LR.seed_geometry(c.seq_bytes(), c.config) is not None]


@pytest.mark.parametrize('name', SEEDED_CASES)
def test_seeded_golden_cases_do_not_change(name, tmp_path):
    case = cases.by_name()[name]
    files = case.materialize(tmp_path)
    arg = files[0] if len(files) == 1 else files
    engine.config(**case.config)
    a = _outcome(lambda: engine.findseqs(arg, case.seq_bytes()))
    assert engine.last_long_reads() in (False, None)
    b = _outcome(lambda: engine.findseqs(arg, case.seq_bytes(), long_reads=True))
    assert a == b
    if b[0] == 'ok' and b[1]['stats']['records_parsed']:
        assert engine.last_long_reads() is True


def test_the_golden_cases_that_count_are_among_them():
    assert {'maxerror0', 'maxerror3', 'spoligo_analyser', 'spoligo_5k', 'quirk_e2', 'long_reads', 'ragged_e0', 'multichunk', 'multichunk_gz',
            'synth20k_mtbc', 'synth4k_300_barcodes', 'forward_n133_p1_c1', 'spoligo_broken', 'ragged_two_files'} <= set(SEEDED_CASES)


# ---- 3. batches, reset, replay ----------------------------------------------------------------------------------------

def test_two_device_batches_and_a_reset():
    T, o = LR.text('main'), LR.oracle('main')
    cuts, text = record_cuts(T), T.text
    cut = cuts[len(T.parts) // 2]
    t = scan.Table(T.seqs, **T.cfg)
    s = scan.Scanner(t, long_reads=True)
    halves = []
    for part in (text[:cut], text[cut:]):
        arr = np.frombuffer(part, dtype=np.uint8)
        d = scan.DeviceBuffer(arr.nbytes); d.upload(arr); halves.append((d, arr))
    for rep in range(2):
        base = 0
        for d, arr in halves:
            s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr), fpos_base=base)
            base += arr.nbytes
        r = s.finish()
        same_as_oracle(r, o)
        assert r['path']['read_list'] and not r['path']['seeded'] and r['main_kernel_launches'] == 2
        s.reset()
    s.close(); t.close()
    for d, _ in halves:
        d.free()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_arena_overflow_is_replayed_on_the_route(how):
    """2.3 M hits: the arena overflows; the library replays a device batch, Scanner feeds host batches again"""
    from test_gpu_profile import _dense
    arr = _dense()
    t = scan.Table([b'ACG' * 10], **dict(cases.DEFAULTS, minreadlength=10))
    assert t.seeded == [True]
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = scan.chunk_offsets(arr)
    res = []
    for lr in (False, True):
        s = scan.Scanner(t, long_reads=lr)
        if how == 'host':
            s.scan_host(arr)
        else:
            s.scan_device(d.ptr, arr.nbytes, co)
        r = s.finish(hits=False)
        res.append((r, s.hit_arrays()))
        s.close()
    (a, ha), (b, hb) = res
    # per read: 51 times inside it, and overlaps of 21, 24 and 27 bases at either end
    assert a['n_hits'] == b['n_hits'] == 40000 * 57 > 1 << 20
    assert (a['counters'] == b['counters']).all() and a['stats'] == b['stats']
    assert all((ha[k] == hb[k]).all() for k in ha)
    assert b['path']['read_list'] and not b['path']['seeded'] and a['path']['seeded']
    d.free(); t.close()


# ---- 4. findseqs ------------------------------------------------------------------------------------------------------

def _same_findseqs(r, o):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):          # (parsed and total count the file's bytes, compressed or not)
        assert r['stats'][k] == o['stats'][k], k


def test_findseqs_on_every_input_route(tmp_path):
    T, o = LR.text('main'), LR.oracle('main')
    text = T.text
    engine.config(**T.cfg)
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'h.fastq.gz').write_bytes(gzip.compress(text, 1, mtime=0))
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    (tmp_path / 'g.fastq.gz').write_bytes(gzip.compress(text, 6, mtime=0))
    for name, inflate, route in (('m.fastq', 'host', 'host'), ('h.fastq.gz', 'host', 'host'), ('b.fastq.gz', 'device', 'device'),
                                 ('g.fastq.gz', 'device_any', 'device_gzip')):
        r = engine.findseqs(str(tmp_path / name), T.seqs, inflate=inflate, long_reads=True)
        assert engine.last_inflate() == route and engine.last_long_reads() is True, name
        _same_findseqs(r, o)
        LR.check_wanted(T, r['hits'])
    # without the option: the same, by the default route
    r = engine.findseqs(str(tmp_path / 'm.fastq'), T.seqs)
    assert engine.last_long_reads() is False
    _same_findseqs(r, o)
    # the records of the hits
    r = engine.findseqs(str(tmp_path / 'm.fastq'), T.seqs, long_reads=True, records=True)
    _same_findseqs(r, o)
    cuts = record_cuts(T)
    assert r['records'] == [T.parts[bisect.bisect_right(cuts, h.file_pos) - 1] for h in r['hits']] and len(r['records']) > 80
    # the profile and the cycles, from the index the route has made
    cutoffs = [ord('5'), ord('I')]
    r = engine.findseqs(str(tmp_path / 'm.fastq'), T.seqs, long_reads=True, profile=cutoffs, cycles=True)
    _same_findseqs(r, o)
    assert r['profile'] == P.profile_host(text, cutoffs, O.chunk_offsets(text), cycles=True)
    assert r['profile'].records == o['stats']['records_parsed'] and r['profile'].longest == 200000


def test_findseqs_on_a_bam_with_a_reverse_strand_long_read(tmp_path):
    T = LR.text('main')
    engine.config(**T.cfg)
    comp = bytes.maketrans(b'ACGT', b'TGCA')
    rng = LR.random.Random(11)
    fwd = bytearray(rng.choices(b'ACGT', k=12000)); fwd[9000:9060] = LR.S60
    rev = W.record('rev', bytes(fwd).translate(comp)[::-1].decode(), [40] * 12000, flag=4 | 16)
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(T.text) + [rev])
    vtext = bam.to_fastq_host(data)
    assert bytes(fwd) in vtext                             # (the strand is restored)
    o = O.scan_memory(vtext, T.seqs, **dict(T.cfg, nthreads=2))
    assert any(h.readlength == 12000 and h.seq_pos == -9000 for h in o['hits']) and len(o['hits']) > 80
    for lr in (True, False):
        r = engine.findseqs(str(tmp_path / 'm.bam'), T.seqs, long_reads=lr)
        assert engine.last_inflate() == 'device_bam' and engine.last_long_reads() is lr
        _same_findseqs(r, o)


# ---- 5. auto ----------------------------------------------------------------------------------------------------------

def test_auto_takes_the_route_for_long_reads_only():
    long_, short = LR.text('main'), LR.text('short150')
    assert long_.seqs == short.seqs and long_.cfg == short.cfg
    r = run(long_, 'auto')
    assert r['path']['read_list'] and not r['path']['seeded']
    same_as_oracle(r, LR.oracle('main'))
    # reads so long that the first 128 KiB hold too few lines for an average
    r = run(LR.text('huge'), 'auto')
    assert r['path']['read_list'] and not r['path']['seeded']
    same_as_oracle(r, LR.oracle('huge'))
    r = run(short, 'auto')
    d = run(short, False)
    assert r['path'] == dict(d['path'], read_list=False) and d['path']['seeded'] and not d['path']['exhaustive']
    same_as_oracle(r, LR.oracle('short150'))
    same_scan(d, r)


@pytest.mark.parametrize('order', ['short-long', 'long-short'])
def test_auto_decides_for_every_batch(order):
    texts = [LR.text('short150'), LR.text('main')]
    if order == 'long-short':
        texts.reverse()
    whole = texts[0].text + texts[1].text
    o = O.scan_memory(whole, texts[0].seqs, **dict(texts[0].cfg, nthreads=2))
    t = scan.Table(texts[0].seqs, **texts[0].cfg)
    res = {}
    for lr in ('auto', False):
        s = scan.Scanner(t, long_reads=lr)
        keep, base = [], 0
        for T in texts:
            arr = np.frombuffer(T.text, dtype=np.uint8)
            d = scan.DeviceBuffer(arr.nbytes); d.upload(arr); keep.append(d)
            s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr), fpos_base=base)
            base += arr.nbytes
        res[lr] = s.finish()
        s.close()
        for d in keep:
            d.free()
    r = res['auto']
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs'] and r['stats']['readlengths'] == o['stats']['readlengths']
    # one batch by the scan kernel, one by the read list: two main kernels, and no tile left to the redo
    assert r['path'] == {'seeded': True, 'exhaustive': False, 'rescanned': False, 'tiles_rescanned': False, 'read_list': True}
    assert r['main_kernel_launches'] == 2
    same_scan(res[False], r)
    t.close()


# ---- 6. refusals and fall-backs ---------------------------------------------------------------------------------------

def test_the_mode_is_set_before_the_first_batch_only():
    L = _lib.lib()
    T = LR.text('odd_bytes')
    t = scan.Table(T.seqs, **T.cfg)
    s = scan.Scanner(t)
    assert L.kvq_scan_set_long_reads(s.h, 3) == _lib.ERR_RUNTIME and L.kvq_scan_set_long_reads(s.h, -1) == _lib.ERR_RUNTIME
    keep = []
    feed_device(s, T.text, keep)
    assert L.kvq_scan_set_long_reads(s.h, 1) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    r = s.finish()
    assert 'read_list' not in r['path'] and not L.kvq_scan_path(s.h) & _lib.PATH_READ_LIST
    s.reset()
    assert L.kvq_scan_set_long_reads(s.h, 1) == 0
    feed_device(s, T.text, keep)
    r2 = s.finish()
    assert L.kvq_scan_path(s.h) & _lib.PATH_READ_LIST and not L.kvq_scan_path(s.h) & 1
    same_scan(r, r2)
    s.reset()                                               # (the mode is kept across a reset, as the records are)
    feed_device(s, T.text, keep)
    s.finish()
    assert L.kvq_scan_path(s.h) & _lib.PATH_READ_LIST
    s.close()
    for d in keep:
        d.free()
    with pytest.raises(ValueError):
        scan.Scanner(t, long_reads='always')
    t.close()
    with pytest.raises(ValueError):
        engine.findseqs('nowhere.fastq', [], long_reads=1)


def test_force_exhaustive_and_a_table_without_seeds_take_the_ordinary_path():
    T, o = LR.text('odd_bytes'), LR.oracle('odd_bytes')
    t = scan.Table(T.seqs, **T.cfg)
    out = []
    for lr in (False, True):
        s = scan.Scanner(t, long_reads=lr)
        s.force_exhaustive()
        keep = []
        feed_device(s, T.text, keep)
        out.append(s.finish())
        s.close(); keep[0].free()
    assert out[1]['path'] == dict(out[0]['path'], read_list=False) and out[1]['path']['exhaustive'] and not out[1]['path']['seeded']
    same_scan(out[0], out[1]); same_as_oracle(out[1], o)
    t.close()
    # minoverlap 4 at two errors: no seed length, no seed index
    cfg = dict(T.cfg, minoverlap=4)
    assert LR.seed_geometry(T.seqs, cfg) is None
    t = scan.Table(T.seqs, **cfg)
    assert t.seed_k == 0 and not any(t.seeded)
    a, b = run(T, False, table=t), run(T, True, table=t)
    assert b['path'] == dict(a['path'], read_list=False) and b['path']['exhaustive'] and len(b['hits']) > len(o['hits'])
    same_scan(a, b)
    t.close()


@pytest.mark.parametrize('flag,taken', [(_lib.FIND_LONG_READS, True), (_lib.FIND_LONG_READS_AUTO, True), (0, False)])
def test_the_flags_of_kvq_findseqs_opts(flag, taken, tmp_path):
    T, o = LR.text('classes'), LR.oracle('classes')
    engine.config(**T.cfg)
    (tmp_path / 'c.fastq').write_bytes(T.text)
    L = _lib.lib()
    farr = (C.c_char_p * 1)(str(tmp_path / 'c.fastq').encode())
    bufs = [C.create_string_buffer(q, len(q) + 1) for q in T.seqs]
    sarr = (C.c_char_p * len(bufs))(*[C.cast(q, C.c_char_p) for q in bufs])
    lens = (C.c_int32 * len(bufs))(*[len(q) for q in T.seqs])
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), flag, 0, (C.c_uint8 * 8)())
    h = L.kvq_findseqs_opts(farr, 1, sarr, lens, len(bufs), C.byref(opts))
    try:
        assert h and _lib.last_error()[0] == 0, _lib.last_error()
        path = L.kvq_scan_path(h)
        assert bool(path & _lib.PATH_READ_LIST) == taken and bool(path & 1) == (not taken)
        nh = L.kvq_scan_n_hits(h)
        assert nh == len(o['hits'])
        assert np.ctypeslib.as_array(L.kvq_scan_hit_file_pos(h), shape=(nh,)).tolist() == [x.file_pos for x in o['hits']]
    finally:
        L.kvq_findseqs_free(h)
    assert C.sizeof(_lib.FindOpts) == 20                     # (kvq_find_opts has not grown)
