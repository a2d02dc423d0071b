"""
The per-cycle counts without a GPU (include/kvarq_hip.h): ``kvq_cycles_host``, the CPU twin of
``kvq_profile_cycles``, against the plain statement of the definition (tests/cycles_ref.py), the identities that tie the
counts to the profile of the same text (tests/profile_ref.py), and the arithmetic of the per-cycle methods of
``kvarq_amd.profile.Profile``.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cycles_ref as CR
import profile_ref as R
from kvarq_amd import _lib, profile as P
from oracle import oracle as O
from test_profile_host import golden_texts, matrix_texts, rec


@functools.lru_cache(maxsize=None)
def seams_text():
    """(text, chunk offsets): lines that end on, one before and one behind every seam a kernel may have (a vector, a wave,
    a slab of 64 or 128 or 256 positions, the last cycle), a record of 10 bases over 700 scores and one the other way
    round, score bytes that are no scores, bases that are no upper-case bases, and a partial record at the end"""
    rng = np.random.RandomState(14)

    def bases(n):
        return rng.choice(np.frombuffer(b'ACGTN', dtype=np.uint8), n).tobytes()

    def scores(n):
        return rng.randint(33, 127, n).astype(np.uint8).tobytes()

    lengths = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)
    text = b''.join(rec(bases(n), scores(n)) for n in lengths)
    text += rec(bases(10), scores(700)) + rec(bases(700), scores(10))
    text += rec(b'ACGT', b'II#I\r') + rec(bases(5), b'\r\x7f\x80\xff!~' * 40) + rec(b'acgtn.ACGTN' * 30, scores(330))
    text += rec(b'', scores(3)) + rec(bases(3), b'')
    text += b'@part\nACGT\n+\nIII'
    return text, [0, len(text)]


def cold_texts():
    """(cold, ordinary): 300 records of 1 .. 300 bytes whose bases are all lower case and whose scores are all 0x80 and
    above -- no byte of them has a column in LDS --, and the same records with ordinary bytes"""
    rng = np.random.RandomState(15)
    cold, plain = [], []
    for n in range(1, 301):
        b = rng.choice(np.frombuffer(b'acgtn', dtype=np.uint8), n)
        s = rng.randint(0x80, 0x100, n).astype(np.uint8)
        cold.append(rec(b.tobytes(), s.tobytes()))
        plain.append(rec((b - 32).astype(np.uint8).tobytes(), (s - 0x80 + 33).clip(33, 126).astype(np.uint8).tobytes()))
    return b''.join(cold), b''.join(plain)


def check(text, chunk_off=None):
    """the twin's counts of a text, equal to the plain statement's and tied to the profile of the same text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    got = P.profile_host(text, (), co, cycles=True)
    want = CR.cycles(text, co)
    bad = np.nonzero(got.cycles != want)[0]
    assert bad.size == 0, (bad[:8], got.cycles[bad[:8]], want[bad[:8]])
    CR.check_identities(got.cycles, R.profile(text, [], co), CR.score_facts(text, co))
    return got


@pytest.mark.parametrize('name', ['L3_N1014_hits_500_1.fastq', 'L3_N1014_hits_500_2.fastq', 'L3_N1014_hits_5k.fastq', 'N0116_1_hits_1k.fastq',
                                  'test_analyser.fastq', 'test_engine.fastq', 'test_engine_1.fastq', 'test_engine_2.fastq'])
def test_twin_equals_the_plain_statement_on_the_golden_files(name):
    got = check(golden_texts()[name])
    assert got.cycles_reached('score')[0] == got.records > 0 and got.last_cycle == got.longest - 1


@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_twin_equals_the_plain_statement_on_the_trim_matrix(name):
    text, co = matrix_texts()[name]
    got = check(text, co)
    if name == 'redo':
        # score lines of 1023 .. 9000 bytes over records of 16 .. 24 bases: the cut at 1024 is crossed from both sides
        assert got.last_cycle == 1023 and got.cycles_reached('score')[1023] >= 18 and got.cycles_reached('score')[1022] > got.cycles_reached('score')[1023]
        assert got.cycle_scores.sum() < got.score_line_bytes and got.cycles_reached('base')[16] > got.cycles_reached('base')[24] > 0


def test_seams_by_hand():
    text, co = seams_text()
    got = check(text, co)
    O.scan_memory(text, [], Amin='!')                             # (a text the scan takes)
    # what seams_text wrote, line by line (the partial record is dropped)
    base_lens = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 10, 700, 4, 5, 330, 0, 3]
    score_lens = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 700, 10, 5, 240, 330, 3, 0]
    assert got.records == 21 and got.mismatched == 6
    assert got.cycles_reached('base').tolist() == [sum(n > p for n in base_lens) for p in range(1024)]
    assert got.cycles_reached('score').tolist() == [sum(n > p for n in score_lens) for p in range(1024)]
    assert got.cycles_reached('score')[699] == 4 and got.cycles_reached('score')[700] == 3 and got.cycles_reached('base')[1023] == 2
    # the bytes that have no column of their own, each at its cycle
    assert got.cycle_scores[4, 13] == 1 and got.cycle_scores[0, 13] == 1 and got.cycle_scores[6, 13] == 1
    assert got.cycle_scores[1, 0x7F] == got.cycle_scores[2, 0x80] == got.cycle_scores[3, 0xFF] == got.cycle_scores[237, 0xFF] == 1
    assert got.cycle_bases[0, ord('a')] == got.cycle_bases[5, ord('.')] == got.cycle_bases[11, ord('a')] == 1 and got.cycle_bases[6, ord('A')] >= 1
    # beyond cycle 1023: counted by the profile, not here
    assert got.base_line_bytes - got.cycle_bases.sum() == 1 == got.score_line_bytes - got.cycle_scores.sum()
    # a partial record in the middle of the text: the tail of ITS chunk is dropped, the next chunk starts a fresh count
    a, b = rec(b'ACGT', b'IIII'), rec(b'GG', b'#I')
    mid = a + b'@part\nAC\n' + b + b
    got = check(mid, [0, len(a) + 9, len(mid)])
    assert got.records == 3 and got.cycle_bases[0, ord('G')] == 2 and got.cycle_bases[:, ord('C')].sum() == 1
    # empty texts
    assert not check(b'', [0]).cycles.any() and not check(b'', [0, 0]).cycles.any() and check(b'', [0]).last_cycle == -1


def test_cold_bytes_count_like_any_other():
    cold, plain = cold_texts()
    a, b = check(cold), check(plain)
    assert a.records == b.records == 300 and a.last_cycle == b.last_cycle == 299
    assert (a.cycles_reached('score') == b.cycles_reached('score')).all() and (a.cycles_reached('base') == b.cycles_reached('base')).all()
    assert a.cycle_scores[:, :0x80].sum() == 0 and a.cycle_bases[:, :ord('a')].sum() == 0


def test_twin_adds_and_refuses_bad_arguments():
    L = _lib.lib()
    text, co = seams_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array(co, dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    assert L.kvq_cycles_len() == CR.LEN == P.CYCLES_LEN == 2 * 1024 * 256
    out = np.arange(CR.LEN, dtype=np.int64)
    assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, out.ctypes.data_as(p64)) == 0
    assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, out.ctypes.data_as(p64)) == 0
    want = CR.cycles(text, co, into=CR.cycles(text, co, into=np.arange(CR.LEN, dtype=np.int64)))
    assert (out == want).all() and (out - np.arange(CR.LEN) == 2 * CR.cycles(text, co)).all()
    # bad arguments: those of kvq_profile_host
    before = out.copy()
    assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, None) == _lib.ERR_RUNTIME
    assert 'kvq_cycles_host' in _lib.last_error()[1]
    assert L.kvq_cycles_host(arr.ctypes.data, -1, co.ctypes.data_as(p64), 1, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, None, 1, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), -1, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    for bad in ([0, arr.nbytes + 1], [5, 4], [-1, 4]):
        bad = np.array(bad, dtype=np.int64)
        assert L.kvq_cycles_host(arr.ctypes.data, arr.nbytes, bad.ctypes.data_as(p64), 1, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    assert (out == before).all()
    assert L.kvq_cycles_host(None, 0, None, 0, out.ctypes.data_as(p64)) == 0 and (out == before).all()


def by_hand():
    """four records on the Sanger scale ('#' = Q2, '+' = Q10, '5' = Q20, '?' = Q30, 'I' = Q40):
         cycle      0 1 2 3 4 5"""
    lines = [(b'ACGTAC', b'II?5+#'),
             (b'ACGTN', b'I?5+#'),
             (b'AGgT', b'I?5\r'),
             (b'CN', b'I#')]
    text = b''.join(rec(b, s) for b, s in lines)
    return P.profile_host(text, ['5'], [0, len(text)], cycles=True)


def test_profile_arithmetic_per_cycle():
    p = by_hand()
    assert p.dQ() == 0 and p.cycle_scores.shape == p.cycle_bases.shape == (1024, 256) and p.last_cycle == 5
    assert p.cycles_reached().tolist()[:7] == p.cycles_reached('score').tolist()[:7] == [4, 4, 3, 3, 2, 1, 0]
    assert p.cycles_reached('base').tolist()[:7] == [4, 4, 3, 3, 2, 1, 0]
    with pytest.raises(ValueError):
        p.cycles_reached('bases')
    # the mean: cycle 1 holds I ? ? # = 40 30 30 2; cycle 3 holds 5 + and a '\r', which is no score
    m = p.cycle_mean_quality()
    assert m[:6] == pytest.approx([40, 25.5, (30 + 20 + 20) / 3., 15, 6, 2]) and np.isnan(m[6:]).all()
    assert p.cycle_mean_quality(dQ=31)[:6] == pytest.approx(m[:6] - 31)
    # quantiles: the lowest value whose cumulative count reaches q of the row
    assert p.cycle_quantile(0.5)[:6].tolist() == [40, 30, 20, 10, 2, 2] and np.isnan(p.cycle_quantile(0.5)[6:]).all()
    assert p.cycle_quantile(0.1)[:6].tolist() == [40, 2, 20, 10, 2, 2]
    assert p.cycle_quantile(0.75)[:6].tolist() == [40, 30, 30, 20, 10, 2] and p.cycle_quantile(1.0)[:4].tolist() == [40, 40, 30, 20]
    assert p.cycle_quantile(0.0)[1] == 2 and p.cycle_quantile(0.5, dQ=31)[0] == 9
    with pytest.raises(ValueError):
        p.cycle_quantile(1.5)
    # below a cutoff, as signed char: '\r' (13) is below '5'; 0x80 is below everything
    assert p.cycle_below('5')[:6] == pytest.approx([0, 0.25, 0, 2 / 3., 1, 1]) and np.isnan(p.cycle_below('5')[6:]).all()
    assert p.cycle_below(0x80)[:6].tolist() == [0] * 6 and p.cycle_below('~')[:6].tolist() == [1] * 6
    hi = P.profile_host(rec(b'AC', b'\xffI'), (), [0, 11], cycles=True)
    assert hi.cycle_below('!')[:2].tolist() == [1, 0] and hi.cycle_below(0xFF)[:2].tolist() == [0, 0] and hi.cycle_below(0)[:2].tolist() == [1, 0]
    # base shares: A C G T N other, upper case only
    s = p.cycle_base_share()
    assert s.shape == (1024, 6) and np.isnan(s[6:]).all()
    assert s[0].tolist() == [0.75, 0.25, 0, 0, 0, 0] and s[1].tolist() == [0, 0.5, 0.25, 0, 0.25, 0]
    assert s[2] == pytest.approx([0, 0, 2 / 3., 0, 0, 1 / 3.]) and s[4].tolist() == [0.5, 0, 0, 0, 0.5, 0]
    # equality looks at the cycles
    q = by_hand()
    assert p == q and not p != q
    q.cycles[5] += 1
    assert p != q
    assert P.Profile(p.words, p.cutoffs) != p and p != P.Profile(p.words, p.cutoffs)
    # as_dict: one more key, sparse, up to the last cycle
    d = p.as_dict()
    assert set(d) == set(P.Profile(p.words, p.cutoffs).as_dict()) | {'cycles'}
    assert len(d['cycles']['score']) == len(d['cycles']['base']) == 6
    assert d['cycles']['score'][1] == {ord('#'): 1, ord('?'): 2, ord('I'): 1} and d['cycles']['base'][2] == {ord('G'): 2, ord('g'): 1}
    import json
    json.dumps(d)
    # the table of the command line
    lines = p.cycle_lines()
    assert len(lines) == 7 and lines[2] == '1 4 25.50 2 30 40 0.000 0.500 0.250 0.000 0.250'
    lines = p.cycle_lines(step=4)
    assert len(lines) == 3 and lines[1].startswith('0-3 4 ') and lines[2].startswith('4-7 2 4.67 2 2 10 ')


def test_a_profile_without_cycles_is_what_it_was():
    p = by_hand()
    old = P.Profile(p.words, p.cutoffs)
    assert old.cycles is None and old == old and old == P.Profile(p.words.copy(), list(p.cutoffs)) and not old != old
    assert 'cycles' not in old.as_dict() and old.as_dict() == {k: v for k, v in p.as_dict().items() if k != 'cycles'}
    assert P.profile_host(b'', ['5']).cycles is None
    for use in (lambda: old.cycle_scores, lambda: old.cycle_mean_quality(), lambda: old.last_cycle, lambda: old.cycle_base_share()):
        with pytest.raises(ValueError, match='cycles=True'):
            use()
    assert old.summary() == p.summary()
