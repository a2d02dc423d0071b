"""
The overrepresented sequences without a GPU (include/kvarq_hip.h): ``kvq_over_host`` -- the CPU twin of
``kvq_over_records`` and ``kvq_over_select`` -- against the plain statement of the definition (tests/over_ref.py) on every text
the kernels are run on, the identities that tie it to the profile and to the duplication of the same text, and the Python
surface: ``ScanOptions``, ``Profile.overrepresented``, the labels, ``as_dict`` and the lines of the command line.
"""
import ctypes as C
import json

import numpy as np
import pytest

import over_ref as OR
import reads_ref as RR
from kvarq_amd import _lib, profile as P
from kvarq_amd.options import ScanOptions
from oracle import oracle as O
from test_profile_host import golden_texts, matrix_texts


def check(text, chunk_off=None, records=0, slots=0):
    """the twin's array of a text, equal to the plain statement's and tied to the profile and the duplication of the same text"""
    text = bytes(text)
    co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    got = P.profile_host(text, (), co, duplication=True, slots=slots, overrepresented=True, over_records=records)
    want = OR.over(text, co, records)
    bad = np.nonzero(got.over != want)[0]
    assert bad.size == 0, (bad[:8], got.over[bad[:8]], want[bad[:8]])
    OR.check_identities(got.over, got.words, got.duplication)
    assert [(r.hash, r.count, r.sequence) for r in got.overrepresented] == OR.rows_of(want)
    assert [got.over_info[k] for k in P.OVER_HEADER] == want[:7].tolist()
    return got


def seqs(p):
    return [r.sequence for r in p.overrepresented]


@pytest.mark.parametrize('name', sorted(OR.small_texts()))
def test_twin_equals_the_plain_statement(name):
    text, M = OR.small_texts()[name]
    got = check(text, [0, len(text)], M)
    o, rows = got.over_info, got.overrepresented
    assert o['records_limit'] == (M or 1 << 18) and o['slots'] == (1024 if M else 1 << 20)
    if name.startswith('threshold_'):
        # 3 of 2999 and of 3000 are listed, of 3001 not; 2 of 2000, not of 2001; a count of 1 never; the unkeyed do not count
        listed = {'threshold_2999_3': 1, 'threshold_3000_3': 1, 'threshold_3001_3': 0, 'threshold_2000_2': 1, 'threshold_2001_2': 0,
                  'threshold_10_1': 0, 'threshold_unkeyed': 1}[name]
        assert o['listed'] == listed and o['unkeyed'] == (57 if name == 'threshold_unkeyed' else 0)
        assert o['keyed'] == (3000 if name == 'threshold_unkeyed' else int(name.split('_')[1])) == o['counted']
        if listed:
            assert rows[0].count == int(name.split('_')[2] if name != 'threshold_unkeyed' else 3) and rows[0].share == rows[0].count / float(o['keyed'])
    if name == 'bound_1000':
        assert o['listed'] == 1000 == o['candidates'] and all(r.count == 2 for r in rows) and [r.hash for r in rows] == sorted(r.hash for r in rows)
    if name == 'bound_1001':
        assert o['listed'] == 0 and o['candidates'] == 1001 and o['counted'] == 2002
    if name in ('boundary', 'boundary_default'):
        _, a, b, five = OR.boundary_text()
        assert seqs(got) == ([a, five] if M else [a, b, five]) and rows[0].count == 201 and rows[-1].count == 6
        assert (o['candidates'], o['counted'] < o['keyed']) == ((64, True) if M else (365, False))
    if name == 'keys':
        want = {b[:64] for b, _ in RR.lines_of(text, [0, len(text)]) if b}
        assert set(seqs(got)) == want and {len(k) for k in want} >= set(range(1, 65)) and o['unkeyed'] == 2
        assert all(r.hash == RR.dup_hash(r.sequence) for r in rows) and b'A\0' in want and b'A' in want
    if name == 'order':
        assert [r.count for r in rows] == [5] * 8 + [3] * 5 + [2] * 3
        for a, b in ((0, 8), (8, 13), (13, 16)):
            assert [r.hash for r in rows[a:b]] == sorted(r.hash for r in rows[a:b])
    if name == 'contention':
        assert len(rows) == 1 and rows[0].count == 20000 and rows[0].share == 1.0 and rows[0].sequence == (b'ACGTTGCA' * 10)[:64]


def test_the_list_does_not_depend_on_the_duplications_level():
    text = RR.levels_text()
    a, b = check(text, [0, len(text)], slots=1024), check(text, [0, len(text)])
    assert a.duplication['level'] >= 2 and b.duplication['level'] == 0 and (a.over == b.over).all()
    assert len(a.overrepresented) == 60 and all(r.count == 5 for r in a.overrepresented)
    for d in (a.duplication, b.duplication):
        assert all(d['distinct'][RR.bin_of(r.count)] >= 1 for r in a.overrepresented)


@pytest.mark.parametrize('name', ['L3_N1014_hits_5k.fastq', 'test_analyser.fastq', 'test_engine.fastq'])
def test_twin_on_the_golden_files(name):
    text = golden_texts()[name]
    assert check(text).records > 0
    check(text, records=100)


@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_twin_on_the_trim_matrix(name):
    text, co = matrix_texts()[name]
    check(text, co)
    check(text, co, records=16)


def test_chunks_partial_records_and_the_clamp():
    a, b = RR.rec(b'ACGT', b'IIII'), RR.rec(b'GG', b'#I')
    mid = a + b'@part\nAC\n' + b + b
    got = check(mid, [0, len(a) + 9, len(mid)])
    assert got.records == 3 and seqs(got) == [b'GG'] and got.over_info['candidates'] == 2
    for text, co in ((b'', [0]), (b'', [0, 0])):
        e = check(text, co)
        assert e.overrepresented == [] and e.over_info['keyed'] == 0
    for wish, M, slots in ((0, 1 << 18, 1 << 20), (-3, 1 << 18, 1 << 20), (1, 16, 1024), (16, 16, 1024), (256, 256, 1024), (257, 257, 2048),
                           (100000, 100000, 1 << 19), (1 << 22, 1 << 22, 1 << 24), (1 << 30, 1 << 22, 1 << 24)):
        o = P.profile_host(mid, (), [0, len(mid)], overrepresented=True, over_records=wish).over_info
        assert (o['records_limit'], o['slots']) == (M, slots) == (OR.records_of(wish), OR.slots_of(OR.records_of(wish)))


def test_twin_writes_and_refuses_bad_arguments():
    L = _lib.lib()
    text = OR.order_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array([0, arr.nbytes], dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    assert L.kvq_over_len() == OR.O_LEN == P.OVER_LEN == 8 + 1000 * 11
    out = np.full(OR.O_LEN, 77, dtype=np.int64)
    for _ in range(2):
        assert L.kvq_over_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64)) == 0
    assert (out == OR.over(text, co)).all()
    before = out.copy()
    assert L.kvq_over_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(p64), 1, 0, None) == _lib.ERR_RUNTIME
    assert 'kvq_over_host' in _lib.last_error()[1]
    assert L.kvq_over_host(arr.ctypes.data, -1, co.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    for bad in ([0, arr.nbytes + 1], [5, 4], [-1, 4]):
        bad = np.array(bad, dtype=np.int64)
        assert L.kvq_over_host(arr.ctypes.data, arr.nbytes, bad.ctypes.data_as(p64), 1, 0, out.ctypes.data_as(p64)) == _lib.ERR_RUNTIME
    assert (out == before).all()


def test_options():
    for kw in ({}, dict(profile='(I', cycles=True, per_read=True, duplication=True, records=True, long_reads=True)):
        off, on = ScanOptions(**kw), ScanOptions(overrepresented=True, **kw)
        assert not off.overrepresented and on.overrepresented and on.profile == (off.profile or [])
        assert on.find_opts(2).flags == off.find_opts(2).flags | 8 | 512 and on.find_opts().size == 20
        names = [(n, a if n != 'kvq_scan_set_profile' else a[1]) for n, a in on.setters()]
        was = [(n, a if n != 'kvq_scan_set_profile' else a[1]) for n, a in off.setters()]
        if not kw:
            assert was == [] and names == [('kvq_scan_set_profile', 0), ('kvq_scan_set_overrepresented', (1,))]
        else:
            assert names == was[:-1] + [('kvq_scan_set_overrepresented', (1,))] + was[-1:] and was[-1][0] == 'kvq_scan_set_long_reads'
    assert _lib.FIND_OVERREPRESENTED == 512


ADAPTER = b'AGATCGGAAGAGCACACGTCTGAACTCCAGTCA'


def labelled():
    revcomp = ADAPTER[:12].translate(bytes.maketrans(b'ACGT', b'TGCA'))[::-1]
    keys = [b'TTGACC' * 5 + ADAPTER, b'CCATGA' * 3 + revcomp + b'GTGT', b'G' * 58 + b'ACGTAC', b'ACGTTGCAAC' * 5, b'GATTACA' * 6]
    text = b''.join(RR.rec(k, b'I' * len(k)) * (9 - i) for i, k in enumerate(keys)) + RR.rec(b'', b'')
    return keys, text


def test_profile_surface_and_labels():
    keys, text = labelled()
    p = P.profile_host(text, ['5'], [0, len(text)], overrepresented=True)
    assert seqs(p) == keys and [r.count for r in p.overrepresented] == [9, 8, 7, 6, 5]
    assert [r.source for r in p.overrepresented] == ['Illumina universal adapter', 'Illumina universal adapter', 'poly-G', None, None]
    assert p.overrepresented[0].share == 9 / 35. and p.over_info == dict(records_limit=1 << 18, slots=1 << 20, keyed=35, unkeyed=1, candidates=5, counted=35, listed=5)
    # a user's mapping: the first entry that matches, a probe or a callable
    mine = {'mine': 'TGTAATC', 'long': lambda s: len(s) > 40, 'never': b'NNNN'}
    assert [r.source for r in p.relabel(mine)] == ['long', None, 'long', 'long', 'mine']
    q = P.profile_host(text, ['5'], [0, len(text)], overrepresented=True, sources=mine)
    assert [r.source for r in q.overrepresented] == ['long', None, 'long', 'long', 'mine'] and p == q
    assert list(P.KNOWN_SOURCES)[:4] == ['Illumina universal adapter', "Illumina small RNA 3' adapter", "Illumina small RNA 5' adapter", 'Nextera transposase']
    assert P.source_of(b'A' * 9 + b'C') == 'poly-A' and P.source_of(b'A' * 8 + b'CC') is None and P.source_of(b'N' * 64) == 'poly-N'
    assert P.source_of(b'xxCTGTCTCTTATAxx') == 'Nextera transposase' == P.source_of(b'TATAAGAGACAG') and P.source_of(b'ccGATCGTCGGACT') == "Illumina small RNA 5' adapter"
    assert P.source_of(b'TGGAATTCTCGGG') == "Illumina small RNA 3' adapter"
    p.relabel()
    # equality looks at the header and at the rows
    q = P.profile_host(text, ['5'], [0, len(text)], overrepresented=True)
    assert p == q and not p != q
    q.over[OR.O_ROWS + 1] += 1; q.relabel()
    assert p != q
    q = P.profile_host(text, ['5'], [0, len(text)], overrepresented=True); q.over_info['keyed'] += 1
    assert p != q
    old = P.Profile(p.words, p.cutoffs)
    assert old != p and p != old and old.over is None and old.overrepresented is None and old.over_info is None
    # as_dict: one more key, and only when taken
    dd = p.as_dict()
    assert set(dd) == set(old.as_dict()) | {'overrepresented'} and old.as_dict() == {k: v for k, v in dd.items() if k != 'overrepresented'}
    assert dd['overrepresented']['rows'][2] == dict(sequence=keys[2].decode(), count=7, share=0.2, hash=RR.dup_hash(keys[2]), source='poly-G')
    assert dd['overrepresented']['listed'] == 5 and json.loads(json.dumps(dd))['overrepresented']['rows'][3]['source'] is None
    # the lines of the command line
    lines = p.overrepresented_lines()
    assert lines[0] == 'overrepresented: 5 sequences of 0.1 % and more among the 5 candidates of the first 262144 records (keyed=35 unkeyed=1 counted=35)'
    assert lines[1] == '%s 9 25.7143%% Illumina universal adapter' % keys[0].decode() and lines[4] == '%s 6 17.1429%% no known source' % keys[3].decode()
    assert len(lines) == 6
    for use in (old.overrepresented_lines, old.relabel):
        with pytest.raises(ValueError, match='overrepresented=True'):
            use()
    assert old.summary() == p.summary()
