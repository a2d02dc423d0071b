"""
The profile of the input without a GPU (include/kvarq_hip.h): ``kvq_profile_host``, the CPU twin of
``kvq_profile_records`` over the same definition, against its plain statement (tests/profile_ref.py) and -- for the
quality trim -- against the oracle's read-length histogram of a scan configured with the cutoff as ``Amin``; and the
arithmetic of ``kvarq_amd.profile.Profile``.
"""
import functools
import glob
import os

import numpy as np
import pytest

import kernel_matrix as KM
import profile_ref as R
import trim_matrix as TM
from kvarq_amd import profile as P
from kvarq_amd.fastq import Fastq, FastqFileFormatException, PhredScale
from oracle import oracle as O

CUTS = R.CUTOFFS8


@functools.lru_cache(maxsize=None)
def golden_texts():
    """name -> text of every golden .fastq that scans without a format error"""
    out = {}
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fastqs', '*.fastq'))):
        with open(path, 'rb') as f:
            text = f.read()
        try:
            O.scan_memory(text, [], Amin='!')
        except O.OracleFormatError:
            continue
        out[os.path.basename(path)] = text
    return out


def families_text():
    t = TM.Text(dict(KM.CONFIGS[8]), 4, seed=77)
    t.band(TM.FAMILIES, 150, nrec=len(TM.FAMILIES) * 40)
    return t.finish()


@functools.lru_cache(maxsize=None)
def matrix_texts():
    """name -> (text, chunk offsets or None): the texts of items 2 to 4"""
    redo, co = TM.redo_text(8)
    return {'amin_I': (TM.amin_text(ord('I')).data.tobytes(), None), 'redo': (redo.data.tobytes(), co),
            'families': (families_text().data.tobytes(), None)}


def check(text, chunk_off=None, cuts=CUTS):
    got = P.profile_host(text, cuts, chunk_off)
    co = got_co = chunk_off if chunk_off is not None else (O.chunk_offsets(text) if text else [0])
    want = R.profile(text, cuts, got_co)
    bad = np.nonzero(got.words != want)[0]
    assert bad.size == 0, (bad[:8], got.words[bad[:8]], want[bad[:8]])
    R.check_identities(got.words, len(cuts), R.long_counts(text, cuts, co))
    return got


def test_eight_golden_files_scan():
    assert len(golden_texts()) == 8


@pytest.mark.parametrize('name', ['L3_N1014_hits_500_1.fastq', 'L3_N1014_hits_500_2.fastq', 'L3_N1014_hits_5k.fastq', 'N0116_1_hits_1k.fastq',
                                  'test_analyser.fastq', 'test_engine.fastq', 'test_engine_1.fastq', 'test_engine_2.fastq'])
def test_twin_equals_the_plain_statement_on_the_golden_files(name):
    got = check(golden_texts()[name])
    assert got.records > 0


@pytest.mark.parametrize('name', ['amin_I', 'redo', 'families'])
def test_twin_equals_the_plain_statement_on_the_trim_matrix(name):
    text, co = matrix_texts()[name]
    got = check(text, co)
    if name == 'redo':
        # score lines of 1023 .. 9000 bytes, and the stretch of 16 .. 24-base records
        assert got.raw_lengths[1024] >= 18 and got.raw_lengths[1023] >= 2 and got.raw_lengths[16:25].min() > 0
        assert got.longest == 9000
    if name == 'families':
        assert got.raw_lengths[0] > 0 and got.raw_lengths[1] > 0 and got.raw_lengths[2] > 0      # the tiny family


@pytest.mark.parametrize('name', sorted(['L3_N1014_hits_500_1.fastq', 'L3_N1014_hits_500_2.fastq', 'L3_N1014_hits_5k.fastq', 'N0116_1_hits_1k.fastq',
                                         'test_analyser.fastq', 'test_engine.fastq', 'test_engine_1.fastq', 'test_engine_2.fastq', 'amin_I', 'redo']))
def test_readlengths_are_those_of_a_scan_with_that_amin(name):
    """the oracle is the pin: stats['readlengths'] of a scan with Amin = cutoff, an empty sequence list"""
    text, co = (golden_texts()[name], None) if name.endswith('.fastq') else matrix_texts()[name]
    cuts = [ord('!'), ord('.'), ord('I'), ord('~'), 0x05]
    got = P.profile_host(text, cuts, co)
    for c in cuts:
        want = O.scan_memory(text, [], Amin=bytes([c]))['stats']
        assert got.readlengths(c) == tuple(want['readlengths']), (name, c)
        assert got.records == want['records_parsed']


def rec(bases, scores, nl=b'\n', name=b'@r'):
    return name + nl + bases + nl + b'+' + nl + scores + nl


def test_edges_by_hand():
    # empty text
    p = P.profile_host(b'', CUTS, [0])
    assert p.records == 0 and not p.words.any() and p.longest == -1
    p = P.profile_host(b'', CUTS, [0, 0])
    assert not p.words.any()
    # a last record without its final newline is dropped
    one = rec(b'ACGT', b'IIII')
    p = check(one + one[:-1], [0, 2 * len(one) - 1])
    assert p.records == 1 and p.base_line_bytes == 4
    # CRLF: the '\r' is a byte of its line
    p = check(rec(b'ACGT', b'II#I', nl=b'\r\n'), [0, len(one) + 4], cuts=[ord('.')])
    assert p.records == 1 and p.base_bytes[13] == 1 and p.score_bytes[13] == 1 and p.raw_lengths[5] == 1 and p.mismatched == 0
    assert p.readlengths('.') == (0, 0, 1)                       # 'II' closed by '#'; 'I\r' is closed by the newline, as long, later
    assert p.score_range() == (2, 40)
    # a score line one byte longer and one byte shorter than its bases
    text = rec(b'ACGT', b'IIIII') + rec(b'ACGT', b'III') + rec(b'ACGT', b'IIII')
    p = check(text, [0, len(text)])
    assert p.records == 3 and p.mismatched == 2
    # bases lines of 1023 / 1024 / 1025 bytes
    text = b''.join(rec(b'A' * n, b'I' * n) for n in (1023, 1024, 1025))
    p = check(text, [0, len(text)])
    assert p.raw_lengths[1023] == 1 and p.raw_lengths[1024] == 2 and p.longest == 1025
    assert p.readlengths('I') == (0,) * 1023 + (1, 0, 0)        # 1024 and 1025 in no bin, but in the longest
    assert p.kept('I', 25) == 1.0
    # two chunks, the first ending in a partial record: its tail is dropped, the second chunk starts a fresh count
    a, b = rec(b'ACGT', b'IIII'), rec(b'GG', b'#I')
    text = a + b'@part\nAC\n' + b + b
    p = check(text, [0, len(a) + 9, len(text)])
    assert p.records == 3 and p.raw_lengths[4] == 1 and p.raw_lengths[2] == 2
    # calling twice adds (the maxima stay maxima)
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array([0, len(a) + 9, len(text)], dtype=np.int64)
    out = P.profile_host(text, CUTS, co).words.copy()
    import ctypes as C
    from kvarq_amd import _lib
    assert _lib.lib().kvq_profile_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 2, (C.c_uint8 * 8)(*CUTS), 8,
                                       out.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    want = R.profile(text, CUTS, co, into=R.profile(text, CUTS, co))
    assert (out == want).all() and out[R.RECORDS] == 6 and out[R.LONGEST] == 5
    # bad arguments
    assert _lib.lib().kvq_profile_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 2, (C.c_uint8 * 9)(), 9,
                                       out.ctypes.data_as(C.POINTER(C.c_int64))) == _lib.ERR_RUNTIME
    assert _lib.lib().kvq_profile_len(8) == R.profile_len(8) == len(out) and _lib.lib().kvq_profile_len(9) == 0


def _profile_of_scores(lines, cuts=('.',)):
    text = b''.join(rec(b'A' * len(s), s) for s in lines)
    return P.profile_host(text, cuts, [0, len(text)])


def test_profile_arithmetic():
    # Illumina 1.8+ / Sanger scores: '#' .. 'J'
    p = _profile_of_scores([b'##IIIIJJ', b'IIII', b'I#I#IIII#'])
    assert p.score_range() == (2, 41) and p.variants() == PhredScale.holding(2, 41) and p.dQ() == 0
    assert p.cutoffs == [ord('.')] and p.records == 3
    assert p.readlengths('.') == p.readlengths(b'.') == p.readlengths(46) == (0, 0, 0, 0, 2, 0, 1)
    assert p.kept('.', 5) == pytest.approx(1 / 3.) and p.kept('.', 4) == 1.0 and p.kept('.', 0) == 1.0
    n = 8 + 4 + 9
    assert p.mean_quality() == pytest.approx((5 * 2 + 14 * 40 + 2 * 41) / float(n))
    assert p.mean_quality(dQ=31) == pytest.approx(p.mean_quality() - 31)
    with pytest.raises(KeyError):
        p.readlengths('I')
    s = p.summary().splitlines()
    assert any(l.startswith('dQ=0') for l in s) and any(l.startswith('variants=') for l in s)
    assert sum(l.startswith('cutoff=') for l in s) == 1 and "cutoff='.'" in p.summary()
    # Illumina 1.3+ scores 'B' .. 'h' hold on the 64-offset scales only
    p = _profile_of_scores([b'BBBhhh'])
    assert p.dQ() == 31 and 'Illumina 1.3+' in p.variants() and 'Sanger' not in p.variants()
    # the Sanger / Illumina 1.3+ ambiguity is Fastq._scale's: scores that both hold give no dQ
    p = _profile_of_scores([b'@@@@IIII'])
    assert {PhredScale.offset(v) for v in p.variants()} == {0, 31}
    with pytest.raises(FastqFileFormatException, match='cannot determine dQ'):
        p.dQ()
    assert 'dQ=?' in p.summary()
    # no scale at all
    p = _profile_of_scores([b'!~'])
    assert p.variants() == []
    with pytest.raises(FastqFileFormatException, match='could not find'):
        p.dQ()
    # cutoffs: characters, bytes, ints, duplicates; nine are too many
    assert P.as_cutoffs(['.', b'I', 0x80, -1, '.']) == [46, 73, 0x80, 0xFF, 46]
    assert P.as_cutoffs('.I') == [46, 73] and P.as_cutoffs(True, amin='.') == [46]
    with pytest.raises(ValueError):
        P.as_cutoffs(range(9))
    assert P.profile_host(b'', []).cutoffs == []


def test_the_exact_dq_agrees_with_the_sampled_guess(fastqs):
    path = os.path.join(fastqs, 'test_analyser.fastq')
    fq = Fastq(path, quiet=True)
    with open(path, 'rb') as f:
        p = P.profile_host(f.read(), ['.'])
    assert p.dQ() == fq.dQ and p.variants() == fq.variants
