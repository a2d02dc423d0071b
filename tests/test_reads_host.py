"""
The per-read distributions and the duplication without a GPU (include/kvarq_hip.h): ``kvq_dup_hash``
against its restatement, ``kvq_reads_host`` -- the CPU twin of ``kvq_reads_records`` and the table -- against the plain
statement of the definition (tests/reads_ref.py) on every text the kernels are run on, the identities that tie both to the
profile of the same text, and the arithmetic of the per-read methods of ``kvarq_amd.profile.Profile``.
"""
import ctypes as C
import json

import numpy as np
import pytest

import profile_ref as R
import reads_ref as RR
from kvarq_amd import _lib, profile as P
from oracle import oracle as O
from test_profile_host import golden_texts, matrix_texts


def check(text, chunk_off=None, slots=0):
    """the twin's arrays of a text, equal to the plain statement's and tied to the profile of the same text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    got = P.profile_host(text, (), co, per_read=True, duplication=True, slots=slots)
    want_r, want_d = RR.reads(text, co), RR.dup(text, co, slots)
    bad = np.nonzero(got.reads != want_r)[0]
    assert bad.size == 0, (bad[:8], got.reads[bad[:8]], want_r[bad[:8]])
    d = got.duplication
    assert [d[k] for k in P.DUP_HEADER] + [0, 0] + d['distinct'] + d['records'] == want_d.tolist()
    RR.check_identities(got.reads, want_d, got.words)
    assert (got.words == R.profile(text, [], co)).all()
    return got


def test_hash_equals_its_restatement():
    L = _lib.lib()
    rng = np.random.RandomState(16)
    for n in list(range(1, 66)) + [100, 1000]:
        for _ in range(4):
            key = rng.randint(0, 256, n).astype(np.uint8).tobytes()
            assert L.kvq_dup_hash_host(key, n) == RR.dup_hash(key) == RR.dup_hash(key[:64]) != 0
    # known values pin the restatement itself: the length alone, one byte, the padding is not the key
    assert RR.dup_hash(b'A') != RR.dup_hash(b'A\0') != RR.dup_hash(b'A\0\0')
    assert len({RR.dup_hash(b'ACGT'[:n]) for n in range(1, 5)}) == 4
    # (m is splitmix64's finalizer: the first two outputs of that generator from seed 0)
    assert RR._m(0) == 0 and RR._m(RR.G) == 0xE220A8397B1DCDAF and RR._m(2 * RR.G & RR.M64) == 0x6E789E6AA1B965F4
    assert L.kvq_dup_hash_host(None, 0) == 0


@pytest.mark.parametrize('name', sorted(RR.small_texts()))
def test_twin_equals_the_plain_statement(name):
    text = RR.small_texts()[name]
    O.scan_memory(text, [], Amin='!')                             # (a text the scan takes)
    got = check(text, [0, len(text)])
    assert got.duplication['level'] == 0 and got.duplication['slots'] == 1 << 24
    if name == 'rounding':
        # 1/8 -> 13, 3/8 -> 38, 1/200 -> 1, 199/200 -> 100, 0/1 -> 0, 1/1 -> 100: each twice (plain, and among other bytes)
        assert got.gc_hist[[13, 38, 1, 0]].tolist() == [2, 2, 2, 2] and got.gc_hist[100] == 4 and got.gc_hist[50] == 10
        h = got.mean_quality_hist
        assert h[74] == 2 and h[34] == 1 and h[128] == 2 and h[255] == 3 and h[127] == 1 and h[80] == 1
    if name == 'nothing':
        assert got.gc_none == 7 and int(got.reads[RR.MEANQ_NONE]) == 4 and got.duplication['unkeyed'] == 4
        assert got.gc_hist[100] == 2 and got.gc_hist[50] == 3 and got.mean_quality_hist[73] == 6 and got.mean_quality_hist[13] == 1
    if name == 'ncount':
        assert got.n_hist[[0, 1, 254]].tolist() == [1, 1, 1] and got.n_hist[255] == 3
    if name == 'keys':
        d = got.duplication
        # four duplicate pairs, 64 = 65 bytes of the prefix (and its first 64 once more), 10 = 10 + '\r', the base key twice
        assert d['distinct'][1] == 4 + 1 + 1 and d['distinct'][2] == 1 and d['unkeyed'] == 1
        assert d['distinct'][0] == 8 + 62 + 16 + 2 and sum(d['distinct'][3:]) == 0


def test_twin_on_the_bins_and_the_levels():
    text = RR.bins_text()
    assert len(text) < 3 << 20
    got = check(text, [0, len(text)])
    d = got.duplication
    # every bin's lower bound and the count one below it: 1 | 2 | 9 | 10, 49 | 50, 99 | 100, 499 | ... | 10000
    assert d['distinct'] == [1, 1, 0, 0, 0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 1] and d['level'] == 0
    assert d['records'] == [1, 2, 0, 0, 0, 0, 0, 0, 9, 59, 149, 599, 1499, 5999, 14999, 10000]
    assert got.duplicate_share() == pytest.approx(1 - 16 / float(sum(RR.COPIES)))
    # levels above 0: 3000 keys in 1024 slots; below: 400
    text = RR.levels_text()
    got = check(text, [0, len(text)], 1024)
    d = got.duplication
    assert d['level'] >= 2 and d['slots'] == 1024 and 128 < d['tracked_distinct'] <= 512 and d['keyed'] == len(RR.lines_of(text, [0, len(text)]))
    assert check(text, [0, len(text)]).duplication['level'] == 0
    few = RR.levels_text(400, 166)
    assert check(few, [0, len(few)], 1024).duplication['tracked_distinct'] == 400
    # the slots: clamped, rounded down to a power of two
    for wish, slots in ((1, 1024), (1023, 1024), (2047, 1024), (2048, 2048), (5000, 4096), (1 << 30, 1 << 24), (-5, 1 << 24)):
        assert RR.slots_of(wish) == slots == P.profile_host(few, (), [0, len(few)], duplication=True, slots=wish).duplication['slots']


@pytest.mark.parametrize('name', ['L3_N1014_hits_5k.fastq', 'test_analyser.fastq', 'test_engine.fastq'])
def test_twin_on_the_golden_files(name):
    got = check(golden_texts()[name])
    assert got.records > 0 and got.gc_hist.sum() > 0


@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_twin_on_the_trim_matrix(name):
    text, co = matrix_texts()[name]
    check(text, co)


def test_chunks_and_partial_records():
    a, b = RR.rec(b'ACGT', b'IIII'), RR.rec(b'GG', b'#I')
    mid = a + b'@part\nAC\n' + b + b
    got = check(mid, [0, len(a) + 9, len(mid)])
    assert got.records == 3 and got.gc_hist[100] == 2 and got.gc_hist[50] == 1 and got.duplication['distinct'][:2] == [1, 1]
    for text, co in ((b'', [0]), (b'', [0, 0])):
        e = check(text, co)
        assert not e.reads.any() and e.duplication['keyed'] == 0 and np.isnan(e.duplicate_share()) and np.isnan(e.gc_mean())


def test_twin_adds_and_refuses_bad_arguments():
    L = _lib.lib()
    text = RR.lengths_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array([0, arr.nbytes], dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    assert L.kvq_reads_len() == RR.LEN == P.READS_LEN == 8 + 101 + 256 + 256 and L.kvq_dup_len() == RR.D_LEN == P.DUP_LEN == 40
    out = np.arange(RR.LEN, dtype=np.int64)
    dup = np.full(RR.D_LEN, 77, dtype=np.int64)
    for _ in range(2):
        assert L.kvq_reads_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64), dup.ctypes.data_as(p64)) == 0
    assert (out - np.arange(RR.LEN) == 2 * RR.reads(text, co)).all() and (dup == RR.dup(text, co)).all()
    before = out.copy()
    assert L.kvq_reads_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, 0, None, None) == 0
    assert L.kvq_reads_host(arr.ctypes.data, -1, co.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64), None) == _lib.ERR_RUNTIME
    assert 'kvq_reads_host' in _lib.last_error()[1]
    assert L.kvq_reads_host(arr.ctypes.data, arr.nbytes, None, 1, 0, out.ctypes.data_as(p64), None) == _lib.ERR_RUNTIME
    for bad in ([0, arr.nbytes + 1], [5, 4], [-1, 4]):
        bad = np.array(bad, dtype=np.int64)
        assert L.kvq_reads_host(arr.ctypes.data, arr.nbytes, bad.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64), None) == _lib.ERR_RUNTIME
    assert (out == before).all()


def by_hand():
    """four records on the Sanger scale ('#' = Q2, '+' = Q10, '5' = Q20, '?' = Q30, 'I' = Q40)"""
    lines = [(b'ACGTAC', b'II?5+#'),        # GC 3/6 = 50, mean (40 + 40 + 30 + 20 + 10 + 2) / 6 = 23.67 -> 24
             (b'ACGTN', b'I?5+#'),          # GC 2/4 = 50, mean 20.4 -> 20, one N
             (b'AGgT', b'I?5\r'),           # GC 1/3 = 33.33 -> 33, mean 30 ('\r' is no score)
             (b'ACGTAC', b'######')]        # the first record's key again
    text = b''.join(RR.rec(b, s) for b, s in lines)
    return P.profile_host(text, ['5'], [0, len(text)], per_read=True, duplication=True)


def test_profile_arithmetic_per_read():
    p = by_hand()
    assert p.dQ() == 0 and p.gc_hist.shape == (101,) and p.mean_quality_hist.shape == p.n_hist.shape == (256,)
    assert {int(k): int(p.gc_hist[k]) for k in np.nonzero(p.gc_hist)[0]} == {33: 1, 50: 3} and p.gc_none == 0
    assert p.gc_mean() == pytest.approx((33 + 150) / 4.)
    assert p.mean_quality_per_read() == {24: 1, 20: 1, 30: 1, 2: 1} and p.mean_quality_per_read(dQ=31) == {-7: 1, -11: 1, -1: 1, -29: 1}
    assert p.mean_quality_quantile(0.5) == 20 and p.mean_quality_quantile(1.0) == 30 and p.mean_quality_quantile(0.0) == 2
    assert p.n_hist[0] == 3 and p.n_hist[1] == 1
    d = p.duplication
    assert d == {'level': 0, 'slots': 1 << 24, 'keyed': 4, 'unkeyed': 0, 'tracked_records': 4, 'tracked_distinct': 3,
                 'distinct': [2, 1] + [0] * 14, 'records': [2, 2] + [0] * 14}
    assert p.duplicate_share() == pytest.approx(0.25)
    # equality looks at both
    q = by_hand()
    assert p == q and not p != q
    q.reads[RR.GC + 50] += 1
    assert p != q
    q = by_hand(); q.duplication['distinct'][0] += 1
    assert p != q
    old = P.Profile(p.words, p.cutoffs)
    assert old != p and p != old and old == P.Profile(p.words, p.cutoffs)
    # as_dict: two more keys
    dd = p.as_dict()
    assert set(dd) == set(old.as_dict()) | {'per_read', 'duplication'} and old.as_dict() == {k: v for k, v in dd.items() if k not in ('per_read', 'duplication')}
    assert dd['per_read']['gc'] == {33: 1, 50: 3} and dd['per_read']['n'] == {0: 3, 1: 1} and dd['duplication']['bounds'] == list(RR.BOUNDS)
    json.dumps(dd)
    only = P.profile_host(b'', (), per_read=True)
    assert only.duplication is None and 'duplication' not in only.as_dict() and 'per_read' in only.as_dict()
    # the lines of the command line
    lines = p.per_read_lines()
    assert lines[0] == 'per-read GC: mean=45.8% reads=4 none=0' and len(lines) == 1 + 21 + 2
    assert lines[1 + 6] == 'GC  30- 34% 1 0.2500' and lines[1 + 10] == 'GC  50- 54% 3 0.7500' and lines[1 + 20] == 'GC 100-100% 0 0.0000'
    assert lines[-2] == 'per-read mean quality (dQ=0): Q10=2 Q25=2 Q50=20 Q75=24 Q90=30' and lines[-1] == 'reads with any N: 1 of 4 (0.2500)'
    lines = p.duplication_lines()
    assert len(lines) == 17 and lines[0].startswith('duplication: level=0 (1 of 1 distinct sequences) slots=16777216 keyed=4 unkeyed=0 tracked: 4 reads, 3 distinct')
    assert lines[1] == 'copies 1: distinct=2 reads=2' and lines[10] == 'copies 10-49: distinct=0 reads=0' and lines[16] == 'copies 10000+: distinct=0 reads=0'
    for use in (lambda: old.gc_hist, lambda: old.gc_mean(), lambda: old.n_hist, lambda: old.mean_quality_per_read()):
        with pytest.raises(ValueError, match='per_read=True'):
            use()
    with pytest.raises(ValueError, match='duplication=True'):
        old.duplicate_share()
    assert old.summary() == p.summary()
