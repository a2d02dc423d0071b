"""
The finish tail on an MI355X at its seams: kvq_fold_batch and kvq_cov_apply, the ordering and gather
kernels of kernels_results.hip, the grow-and-rescan logic of kvq_finish.hip, on the inputs of tests/results_matrix.py.

Every comparison is exact and against the oracle: the five hit columns in order, the hit bytes and their offsets
(``off[n]`` included), ``nseqhits``, ``nseqbasehits``, coverage, mutations and ``CTR_HITS``.  Before it compares, every
test asserts that its input REACHED the seam it names: the geometry ``kvq_scan_order_info`` reports, applied to the
oracle's file_pos column (results_matrix.occupancy), gives the hits per bucket and per share.
"""
import ctypes as C

import numpy as np
import pytest

import results_matrix as M
from kvarq_amd import _lib, scan

pytestmark = pytest.mark.gpu

COLUMNS = ('seq_nr', 'file_pos', 'seq_pos', 'length', 'readlength')
KNOBS = ('KVQ_ORDER', 'KVQ_ARENA_CAP', 'KVQ_BLOB_CAP', 'KVQ_RECORD_CAP')


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope='module')
def table():
    """table(seqs, cfg): one device table per sequence list, kept for the module"""
    made = {}

    def get(seqs, cfg=M.CFG):
        key = (tuple(seqs), tuple(sorted(cfg.items())))
        if key not in made:
            made[key] = scan.Table(seqs, **cfg)
        return made[key]
    yield get
    for t in made.values():
        t.close()


def feed(s, pieces, how):
    """the pieces [(text, fpos_base)] as device or host batches; -> the device buffers to free"""
    bufs = []
    for text, base in pieces:
        arr = np.frombuffer(text, dtype=np.uint8)
        if how == 'device':
            d = scan.DeviceBuffer(arr.nbytes)
            d.upload(arr)
            bufs.append(d)
            s.scan_device(d.ptr, arr.nbytes, scan.chunk_offsets(arr), fpos_base=base)
        else:
            s.scan_host(arr, fpos_base=base)
    return bufs


def result_of(s, t):
    """finish -> (everything the comparison looks at, order info)"""
    r = s.finish(hits=False)
    a = s.hit_arrays()
    ctr = r['counters']
    a.update(n_hits=r['n_hits'], ctr_hits=int(ctr[_lib.CTR_HITS]), records_parsed=int(ctr[_lib.CTR_RECORDS]),
             nseqhits=ctr[t.off_nseqhits:t.off_nseqhits + t.nseq].copy(),
             nseqbasehits=ctr[t.off_nseqbasehits:t.off_nseqbasehits + t.nseq].copy(),
             coverage=np.array(r['coverage']), mutations=np.array(r['mutations']))
    return a, s.order_info()


def assert_equals_oracle(a, ref):
    assert a['n_hits'] == ref.n == a['ctr_hits'] and a['records_parsed'] == ref.records_parsed
    for col in COLUMNS:
        assert a[col].dtype == getattr(ref, col).dtype and np.array_equal(a[col], getattr(ref, col)), col
    assert a['offsets'].tolist() == ref.offsets.tolist()                    # (n + 1 of them: [0] when there is no hit)
    assert a['blob'].tobytes() == ref.blob
    for k in ('nseqhits', 'nseqbasehits', 'coverage', 'mutations'):
        assert a[k].tolist() == getattr(ref, k).tolist(), k


def assert_same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def assert_records(a, pieces, ref):
    want, at = [], 0
    for text, base in pieces:
        mine = ref.file_pos[(ref.file_pos >= base) & (ref.file_pos < base + len(text))]
        want += M.records_of(text, mine, base)
        at += len(mine)
    assert at == ref.n
    blob = a['record_blob'].tobytes()
    got = [blob[o:o + n] for o, n in zip(a['record_off'].tolist(), a['record_len'].tolist())]
    assert got == want


def seam(info, ref, pieces, how_ordered):
    """the order info is the plan of this input and says which ordering made the result; -> hits per
    bucket and per share, counted from the oracle's file_pos"""
    lo = min(base for _, base in pieces)
    hi = max(base + len(text) for text, base in pieces)
    assert info['n'] == ref.n and info['lo'] == lo
    assert (info['shift'], info['nb'], info['bc']) == M.plan_geometry(lo, hi, ref.n, info['arena_cap'])
    assert (info['crowded'], info['mergesort']) == {'buckets': (0, 0), 'crowded': (1, 1), 'mergesort': (0, 1)}[how_ordered]
    return M.occupancy(ref.file_pos, lo, info['shift'], info['bc'], info['nb'])


def scan_once(t, pieces, how, records=False):
    s = scan.Scanner(t, records=records)
    bufs = feed(s, pieces, how)
    a, info = result_of(s, t)
    s.close()
    for d in bufs:
        d.free()
    return a, info


@pytest.mark.parametrize('how', ['device', 'host'])
def test_buckets_of_1_to_64_hits_are_ordered_by_the_bucket_path(table, how):
    """the ladder: occupancies on both sides of 1 | 2, 8 | 9 and at 63, 64, none above; no merge sort"""
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    a, info = scan_once(table(seqs), [(text, 0)], how)
    per_bucket, _ = seam(info, ref, [(text, 0)], 'buckets')
    assert {1, 2, 8, 9, 63, 64} <= set(per_bucket.tolist()) and int(per_bucket.max()) == M.BUCKET_MAX
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('records', [False, True])
@pytest.mark.parametrize('where', ['first', 'middle', 'last'])
def test_one_bucket_of_65_hits_sends_the_scan_to_the_merge_sort(table, where, records):
    """... which overwrites what the bucket ordering wrote; the records follow the new order"""
    text, seqs = M.ladder65(where)
    ref = M.ref_of('ladder65', where)
    a, info = scan_once(table(seqs), [(text, 0)], 'device', records=records)
    per_bucket, _ = seam(info, ref, [(text, 0)], 'crowded')
    assert int(per_bucket.max()) == M.BUCKET_MAX + 1 and int((per_bucket > M.BUCKET_MAX).sum()) == 1
    occupied = np.nonzero(per_bucket)[0]
    if where != 'middle':
        assert int(np.argmax(per_bucket)) == int(occupied[0 if where == 'first' else -1])
    assert_equals_oracle(a, ref)
    if records:
        assert_records(a, [(text, 0)], ref)


@pytest.mark.parametrize('name, arg', [('ladder', None), ('ties', 'wave'), ('ties', 'network'), ('dense_corner', None)])
def test_the_merge_sort_and_the_bucket_path_give_the_same_bytes(table, monkeypatch, name, arg):
    """KVQ_ORDER=mergesort, switched inside one process: byte for byte the bucket path's result, both the oracle's"""
    text, seqs = getattr(M, name)() if arg is None else getattr(M, name)(arg)
    ref = M.ref_of(name, arg)
    t = table(seqs)
    by_buckets, info = scan_once(t, [(text, 0)], 'device')
    seam(info, ref, [(text, 0)], 'buckets')
    monkeypatch.setenv('KVQ_ORDER', 'mergesort')
    by_sort, info = scan_once(t, [(text, 0)], 'device')
    seam(info, ref, [(text, 0)], 'mergesort')
    monkeypatch.delenv('KVQ_ORDER')
    again, info = scan_once(t, [(text, 0)], 'device')
    seam(info, ref, [(text, 0)], 'buckets')
    assert_same_bytes(by_sort, by_buckets)
    assert_same_bytes(again, by_buckets)
    assert_equals_oracle(by_buckets, ref)
    assert_equals_oracle(by_sort, ref)


@pytest.mark.parametrize('at_begin, at_finish, how_ordered', [('mergesort', None, 'mergesort'), (None, 'mergesort', 'buckets')])
def test_a_tail_enqueued_ahead_of_time_keeps_the_ordering_it_was_given(table, monkeypatch, at_begin, at_finish, how_ordered):
    """KVQ_ORDER is read when the tail is enqueued (kvq_scan_finish_begin); finish goes by that, whatever it says by then"""
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    t = table(seqs)
    s = scan.Scanner(t)
    bufs = feed(s, [(text, 0)], 'device')
    for value, step in ((at_begin, s.finish_begin), (at_finish, lambda: None)):
        if value is None:
            monkeypatch.delenv('KVQ_ORDER', raising=False)
        else:
            monkeypatch.setenv('KVQ_ORDER', value)
        step()
    a, info = result_of(s, t)
    s.close()
    for d in bufs:
        d.free()
    seam(info, ref, [(text, 0)], how_ordered)
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('regime, lo, hi', [('network', 2, 8), ('wave', 9, 64)])
def test_hits_that_differ_only_in_class_or_ordinal_keep_the_oracles_order(table, regime, lo, hi):
    text, seqs = M.ties(regime)
    ref = M.ref_of('ties', regime)
    a, info = scan_once(table(seqs), [(text, 0)], 'device')
    per_bucket, _ = seam(info, ref, [(text, 0)], 'buckets')
    occupied = per_bucket[per_bucket > 0]
    assert lo <= int(occupied.min()) and int(occupied.max()) <= hi and len(occupied) >= 100
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('how', ['device', 'host'])
def test_shares_of_several_chunks_with_a_ragged_last_one_and_empty_shares_behind_the_last_bucket(table, how):
    text, seqs = M.dense_corner()
    ref = M.ref_of('dense_corner')
    a, info = scan_once(table(seqs), [(text, 0)], how)
    per_bucket, per_share = seam(info, ref, [(text, 0)], 'buckets')
    nb, bc = info['nb'], info['bc']
    assert int(per_share.max()) > 2 * M.GATHER_CHUNK
    assert any(c > 2 * M.GATHER_CHUNK and c % M.GATHER_CHUNK for c in per_share.tolist())
    assert nb % bc != 0 and (M.ORDER_BLOCKS - 1) * bc >= nb and per_share[M.ORDER_BLOCKS - 1] == 0
    assert int((per_share == 0).sum()) > M.ORDER_BLOCKS * 7 // 8
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('order', ['buckets', 'mergesort'])
@pytest.mark.parametrize('which', M.TINY)
def test_no_hit_one_hit_two_hits(table, monkeypatch, which, order):
    text, seqs = M.tiny(which)
    ref = M.ref_of('tiny', which)
    if order == 'mergesort':
        monkeypatch.setenv('KVQ_ORDER', 'mergesort')
    a, info = scan_once(table(seqs), [(text, 0)], 'device')
    # (without hits there is nothing to sort: the merge sort is not run)
    per_bucket, _ = seam(info, ref, [(text, 0)], order if ref.n else 'buckets')
    assert info['nb'] <= 256 and info['bc'] == 1
    if which == 'zero':
        assert a['offsets'].tolist() == [0] and a['n_hits'] == 0
    if which == 'two_in_one':
        assert int(per_bucket.max()) == 2
    if which == 'first_and_last':
        assert per_bucket[info['nb'] - 1] == 1 and int(np.nonzero(per_bucket)[0][0]) == 0
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('how', ['device', 'host'])
def test_two_batches_far_from_zero_with_a_gap_between_them(table, how):
    pieces, seqs = M.offset_batches()
    ref = M.offset_reference()
    a, info = scan_once(table(seqs), pieces, how)
    per_bucket, _ = seam(info, ref, pieces, 'buckets')
    assert info['lo'] == M.OFFSET_BASE > 1 << 33
    gap = ((np.array([pieces[0][1] + len(pieces[0][0]), pieces[1][1]]) - info['lo']) >> info['shift']).tolist()
    assert gap[1] - gap[0] > 1000 and int(per_bucket[gap[0] + 1:gap[1]].sum()) == 0 and per_bucket[gap[1]:].sum() > 0
    assert {1, 2, 8, 9, 63, 64} <= set(per_bucket.tolist())
    assert_equals_oracle(a, ref)


OVERFLOW = {'blob_one_byte_short': (0, -1), 'arena_one_hit_short': (-1, 0), 'both_short': (-1, -1), 'exactly_full': (0, 0)}


def small_caps(monkeypatch, ref, case):
    hits, blob = ref.n + OVERFLOW[case][0], len(ref.blob) + OVERFLOW[case][1]
    assert hits > 64 and blob > 256                                           # (above the knobs' minima)
    monkeypatch.setenv('KVQ_ARENA_CAP', str(hits))
    monkeypatch.setenv('KVQ_BLOB_CAP', str(blob))
    return hits, blob


def assert_caps_after(info, ref, case, hits, blob):
    assert info['arena_cap'] >= ref.n and info['blob_cap'] >= len(ref.blob)
    if case == 'exactly_full':
        assert (info['arena_cap'], info['blob_cap']) == (hits, blob) == (ref.n, len(ref.blob))      # no growth: no rescan
    if OVERFLOW[case][0]:
        assert info['arena_cap'] > hits
    if OVERFLOW[case][1]:
        assert info['blob_cap'] > blob


@pytest.mark.parametrize('how', ['device', 'host'])
@pytest.mark.parametrize('case', sorted(OVERFLOW))
def test_arena_and_blob_exactly_full_and_one_short(table, monkeypatch, case, how):
    """KVQ_ARENA_CAP / KVQ_BLOB_CAP from the oracle's own counts: device batches are replayed by the library, host
    batches fed again by Scanner.finish; exactly full is no overflow"""
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    hits, blob = small_caps(monkeypatch, ref, case)
    t = table(seqs)
    s = scan.Scanner(t)
    before = s.order_info()
    assert (before['arena_cap'], before['blob_cap']) == (hits, blob) and before['n'] == 0
    bufs = feed(s, [(text, 0)], how)
    a, info = result_of(s, t)
    s.close()
    for d in bufs:
        d.free()
    assert_caps_after(info, ref, case, hits, blob)
    seam(info, ref, [(text, 0)], 'buckets')
    assert_equals_oracle(a, ref)


@pytest.mark.parametrize('how', ['device', 'host'])
def test_overflow_with_records_scales_the_record_store_too(table, monkeypatch, how):
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    monkeypatch.setenv('KVQ_ARENA_CAP', str(ref.n // 3))
    monkeypatch.setenv('KVQ_BLOB_CAP', str(len(ref.blob) // 2))
    monkeypatch.setenv('KVQ_RECORD_CAP', '512')
    a, info = scan_once(table(seqs), [(text, 0)], how, records=True)
    assert_caps_after(info, ref, 'both_short', ref.n // 3, len(ref.blob) // 2)
    seam(info, ref, [(text, 0)], 'buckets')
    assert_equals_oracle(a, ref)
    assert_records(a, [(text, 0)], ref)
    assert len(a['record_blob']) == len(text) > 512              # every read of the ladder has a hit: every record is kept, once


def test_a_c_caller_with_host_batches_is_told_to_rescan(table, monkeypatch):
    """without a replay: KVQ_ERR_RESCAN, the arena and the blob grown; reset, the same batch again, and the oracle's result"""
    text, seqs = M.ladder()
    ref = M.ref_of('ladder')
    hits, blob = small_caps(monkeypatch, ref, 'both_short')
    t = table(seqs)
    s = scan.Scanner(t)
    L = _lib.lib()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = scan.chunk_offsets(arr)
    for attempt in range(2):
        assert L.kvq_scan_host(s.h, arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1, 0) == 0
        rc = L.kvq_scan_finish(s.h)
        if attempt == 0:
            assert rc != 0 and _lib.last_error()[0] == _lib.ERR_RESCAN
            info = s.order_info()
            assert info['arena_cap'] > hits and info['blob_cap'] > blob and info['n'] == 0      # (not finished)
            assert L.kvq_scan_reset(s.h) == 0
        else:
            assert rc == 0, _lib.last_error()
    a, info = result_of(s, t)
    s.close()
    assert_caps_after(info, ref, 'both_short', hits, blob)
    assert_equals_oracle(a, ref)


def test_a_reused_handle_takes_the_speculated_copy_from_too_large_to_too_small(table):
    """dense corner, then one hit, then the ladder on one handle: the result bytes fetched ahead of time are sized by the
    scan before"""
    t = table(M.LADDER_SEQS)
    s = scan.Scanner(t)
    sizes = []
    for name, arg in (('dense_corner', None), ('tiny', 'one'), ('ladder', None)):
        text, seqs = getattr(M, name)() if arg is None else getattr(M, name)(arg)
        assert seqs is M.LADDER_SEQS
        ref = M.ref_of(name, arg)
        bufs = feed(s, [(text, 0)], 'device')
        a, info = result_of(s, t)
        seam(info, ref, [(text, 0)], 'buckets')
        assert_equals_oracle(a, ref)
        sizes.append(32 * ref.n + len(ref.blob))
        s.reset()
        for d in bufs:
            d.free()
    s.close()
    assert sizes[0] > 1 << 20 and sizes[1] < 100 and sizes[2] > 4 * (sizes[1] + 65536)      # (first guess: 1 MiB; then the last scan's bytes + 1/8 + 64 KiB)


@pytest.mark.parametrize('how', ['device', 'host'])
def test_the_fold_at_its_seams(table, how):
    """mismatches at hit offsets 0, 3, 4, 15, 16 and the last, all six mutation classes, a partial last wave of hits,
    sequences of 64, 65, 127 and 128 bases covered to their last base (tests/test_results_host.py shows the text has them)"""
    text, seqs = M.fold()
    ref = M.ref_of('fold')
    a, info = scan_once(table(seqs, M.FOLD_CFG), [(text, 0)], how)
    seam(info, ref, [(text, 0)], 'buckets')
    assert info['n'] % 64 != 0 and (ref.mutations.reshape(-1, 6).sum(axis=0) > 0).all()
    assert_equals_oracle(a, ref)
