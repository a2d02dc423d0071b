"""
Adapter probes that tolerate mismatches, without a GPU (include/kvarq_hip.h): the plain statement of the rule
(tests/adapt_mm_ref.py) against the exact one where the two must agree, each wrong statement of the rule visible on the text
named for it, the CPU twins ``kvq_adapt_host_mm`` and ``kvq_clip_host_mm`` against the plain statement on every text -- each
asserts its census first --, ``per == 0`` against the old twins word for word, the refusals, what ``ScanOptions`` and the command
line hand on, and the twins as a program of their own under AddressSanitizer and UBSan.
"""
import contextlib
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapt_mm_ref as M
import adapt_ref as A
import clip_ref as CR
from kvarq_amd import _lib, profile as P
from kvarq_amd.options import ScanOptions

HERE = os.path.dirname(os.path.abspath(__file__))
RUNS = [(name, per) for name in sorted(M.texts()) for per in M.texts()[name][2]]


@pytest.mark.parametrize('name', sorted(A.texts()))
def test_the_rule_is_the_exact_rule_where_it_must_be(name):
    """per = 0 is section 18's rule on every text of adapt_ref; per = 10 changes nothing on them but on `aliases`, where it
    changes every record (their filler is C/T and their probes start with A or G: tolerance finds nothing by accident)"""
    text, probes = A.texts()[name]
    if name == 'edges':
        text = text[:60000]
        text = text[:text.rindex(b'\n@') + 1]
    co = [0, len(text)]
    exact = A.per_record(text, co, probes)
    assert [r[:6] for r in M.per_record(text, co, probes, 0)] == exact
    assert (M.adapt(text, co, probes, 0) == A.adapt(text, co, probes)).all()
    tolerant = [r[:6] for r in M.per_record(text, co, probes, 10)]
    if name == 'aliases':
        assert all(a != b for a, b in zip(tolerant, exact)) and len(exact) > 20
    else:
        assert tolerant == exact


@pytest.mark.parametrize('name', sorted(M.texts()))
def test_the_texts_reach_their_seams(name):
    M.check_census(name)


@pytest.mark.parametrize('wrong', sorted(M.MUTATIONS))
def test_every_wrong_statement_is_visible_on_its_text(wrong):
    name, words = M.MUTATIONS[wrong]
    text, probes, _, _ = M.texts()[name]
    co = [0, len(text)]
    right, mutant = M.adapt(text, co, probes, 10), M.adapt(text, co, probes, 10, wrong=wrong)
    assert (right != mutant).sum() == words > 0                                         # (the counts of profiles/adapt_mm_tests.txt)


@pytest.mark.parametrize('name,per', RUNS)
def test_twins_are_the_definition(name, per):
    M.check_census(name)
    text, probes, _, _ = M.texts()[name]
    co = [0, len(text)]
    want = M.adapt(text, co, probes, per)
    got = P.adapt_host(text, probes, co, adapter_mismatches=per)
    bad = np.nonzero(got.words != want)[0]
    assert bad.size == 0, (bad[:8], got.words[bad[:8]], want[bad[:8]])
    M.check_identities(got.words)
    assert got.mismatch_per == per and (got.first_mismatches.sum(axis=1) == got.found).all()
    masked, words = M.mask(text, co, probes, per)
    gm, gw = P.clip_host(text, probes, co, adapter_mismatches=per)
    assert bytes(gm) == masked and (gw == words).all() and gw[M.CLIP_PER] == per
    assert gw[M.C_CLIPPED] == got.with_adapter + got.tail_only
    twice, tw = P.clip_host(gm, probes, co, adapter_mismatches=per)                      # idempotent
    assert (twice == gm).all() and (tw == gw).all()
    # the twin ADDS over batches cut between records
    ends = CR.record_ends(text)
    cut = ends[len(ends) // 2 - 1]
    acc = np.zeros(M.C_LEN, dtype=np.int64)
    parts = [bytes(P.clip_host(text[x:y], probes, [0, y - x], into=acc, adapter_mismatches=per)[0]) for x, y in ((0, cut), (cut, len(text)))]
    assert b''.join(parts) == masked and (acc == words).all()


def call_mm(fn, text, probes, per, n=None, nwords=A.LEN):
    L = _lib.lib()
    arr = np.frombuffer(text, dtype=np.uint8).copy()
    co = np.array([0, len(text)], dtype=np.int64)
    out = np.zeros(nwords, dtype=np.int64)
    k = max(len(probes), 1)
    rc = getattr(L, fn)(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 1, (C.c_char_p * k)(*probes),
                        (C.c_int32 * k)(*([len(p) for p in probes] or [0])), len(probes) if n is None else n, per,
                        out.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, out, arr


@pytest.mark.parametrize('name', sorted(A.texts()) + ['stores'])
def test_per_zero_is_the_old_twins_word_for_word(name):
    text, probes = (CR.stores_text()[0], CR.PROBES[2]) if name == 'stores' else A.texts()[name]
    co = [0, len(text)]
    old = P.adapt_host(text, probes, co)
    rc, words, _ = call_mm('kvq_adapt_host_mm', text, probes, 0)
    assert rc == 0 and (words == old.words).all() and not words[4:8].any()
    om, ow = P.clip_host(text, probes, co)
    rc, words, arr = call_mm('kvq_clip_host_mm', text, probes, 0, nwords=M.C_LEN)
    assert rc == 0 and (words == ow).all() and (arr == om).all() and not words[5:].any()
    for off in (None, False, 0):
        assert P.adapt_host(text, probes, co, adapter_mismatches=off) == old


def test_by_hand():
    p = A.P12.decode()
    lines = ['CC' + p + 'TT',                     # exact at 2
             'CC' + p[:5] + 'N' + p[6:] + 'TT',   # one 'N': within the budget of a 12-base probe
             'CC' + p[:5] + 'NN' + p[7:] + 'TT',  # two: not
             'CCCC' + p[:11],                     # the last base missing: no window inside the line, a tail of 11
             'CCCC' + p[:5] + 'C' + p[6:10]]      # a tail of 10 with one mismatch
    text = ''.join('@r\n%s\n+\n%s\n' % (b, 'I' * len(b)) for b in lines).encode()
    recs = M.per_record(text, [0, len(text)], [A.P12], 10)
    assert [(r[2][0], r[6][0], r[3][0], r[4]) for r in recs] == [(2, 0, None, 2), (2, 1, None, 2), (None, None, None, 16), (None, None, 11, 4), (None, None, 10, 4)]
    a = P.adapt_host(text, [A.P12], [0, len(text)], adapter_mismatches=True)
    assert a.mismatch_per == 10 and a.first_mismatches.tolist() == [[1, 1, 0, 0]] and a.found[0] == 2 and a.tail[0, 11] == 1 and a.tail[0, 10] == 1
    assert (a.with_adapter, a.tail_only, a.records) == (2, 2, 5)
    exact = P.adapt_host(text, [A.P12], [0, len(text)])
    assert exact.mismatch_per == 0 and exact.found[0] == 1 and exact.tail[0, 11] == 1 and exact.tail_only == 1 and not exact.first_mismatches.any()
    got, w = P.clip_host(text, [A.P12], [0, len(text)], adapter_mismatches=10)
    assert bytes(got).split(b'\n')[3::4] == [b'II' + b'!' * 14, b'II' + b'!' * 14, b'I' * 16, b'IIII' + b'!' * 11, b'IIII' + b'!' * 10]
    assert w.tolist() == [1, 5, 4, 49, 49, 10, 0, 0]
    c = P.Clip(w, ['a'], [A.P12])
    assert c.mismatch_per == 10 and c.line().endswith('bases_cut=49 mismatches=1 per 10')
    ph = P.profile_host(text, 'I', [0, len(text)], adapters=[A.P12], clip=[A.P12], adapter_mismatches=10)
    assert ph.adapters == a and ph.clipped == c
    assert ph.adapter_lines()[-1].endswith('mismatches(1 per 10)=1/1/0/0') and ph.as_dict()['adapters']['probes'][0]['first_mismatches'] == [1, 1, 0, 0]
    assert 'mismatches' not in P.profile_host(text, 'I', [0, len(text)], adapters=[A.P12]).adapter_lines()[-1]


def test_refusals():
    text = A.rec(b'ACGT' * 10)
    for fn, nwords in (('kvq_adapt_host_mm', A.LEN), ('kvq_clip_host_mm', M.C_LEN)):
        for per in (0, 10, 17, 32):
            assert call_mm(fn, text, [A.P12], per, nwords=nwords)[0] == 0
        for per in (-1, 1, 9, 33, 1 << 20):
            rc, out, arr = call_mm(fn, text, [A.P12], per, nwords=nwords)
            assert rc == _lib.ERR_RUNTIME and 'mismatch' in _lib.last_error()[1] and not out.any() and bytes(arr) == text
        for probes, n in (([A.P12], 0), ([A.P12] * 9, 9), ([b'ACGTACG'], 1), ([b'A' * 33], 1), ([b'ACGTACGa'], 1), ([b'ACGTNCGT'], 1)):
            assert call_mm(fn, text, probes, 10, n, nwords=nwords)[0] == _lib.ERR_RUNTIME and 'upper-case A C G T' in _lib.last_error()[1]
    for bad in (1, 9, 33, -10, 10.0, '10'):
        with pytest.raises(ValueError):
            ScanOptions(clip=True, adapter_mismatches=bad)
    for on in (True, 10, 32):
        with pytest.raises(ValueError, match='adapters= or clip='):
            ScanOptions(adapter_mismatches=on)
        with pytest.raises(ValueError, match='adapters= or clip='):
            P.profile_host(text, (), [0, len(text)], adapter_mismatches=on)
    # the flag of kvq_findseqs_opts: refused without the probes' flags, and without the structure that holds the rate
    L = _lib.lib()
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)

    def refused(opts):
        assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.cast(C.byref(opts), C.POINTER(_lib.FindOpts)))
        assert _lib.last_error()[0] == _lib.ERR_RUNTIME
        return _lib.last_error()[1]
    assert 'KVQ_FIND_ADAPTERS or KVQ_FIND_CLIP' in refused(_lib.FindOpts(20, _lib.FIND_ADAPTER_MISMATCHES, 0, (C.c_uint8 * 8)()))
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_ADAPTER_MISMATCHES) and 'KVQ_FIND_ADAPTERS or KVQ_FIND_CLIP' in _lib.last_error()[1]
    fo = ScanOptions(clip=[A.P12]).find_opts(_lib.FIND_ADAPTER_MISMATCHES)               # the 288 bytes: no room for the rate
    assert C.sizeof(fo) == 288 and 'bad size' in refused(fo)
    for per in (9, 33, -1):
        fo = ScanOptions(clip=[A.P12], adapter_mismatches=10).find_opts()
        fo.mismatch_per = per
        assert 'mismatch' in refused(fo)
    assert C.sizeof(_lib.FindOptsAdaptersMm) == 292 and _lib.FIND_ADAPTER_MISMATCHES == 4096


def test_scan_options():
    for off in (None, False, 0):
        o = ScanOptions(clip=[A.P12], adapter_mismatches=off)
        fo = o.find_opts()
        assert o.mismatch_per == 0 and type(fo) is _lib.FindOptsAdapters and fo.base.size == 288 and fo.base.flags == _lib.FIND_CLIP
        assert [n for n, _ in o.setters()] == ['kvq_scan_set_clip']
    assert ScanOptions(adapter_mismatches=None).find_opts().size == 20 and ScanOptions().mismatch_per == 0
    assert ScanOptions(clip=True, adapter_mismatches=True).mismatch_per == 10
    per = ScanOptions(clip=True, adapter_mismatches=np.int64(12)).mismatch_per                  # any integer type
    assert per == 12 and type(per) is int and ScanOptions(clip=True, adapter_mismatches=np.uint8(0)).mismatch_per == 0
    for per in (10, 11, 32):
        o = ScanOptions(adapters=[A.P12, A.P32], clip=[A.P12, A.P32], adapter_mismatches=per, profile='I')
        fo = o.find_opts(1)
        assert type(fo) is _lib.FindOptsAdaptersMm and fo.mismatch_per == per == o.mismatch_per and fo.a.base.size == C.sizeof(fo) == 292
        assert fo.a.base.flags == 1 | _lib.FIND_PROFILE | _lib.FIND_ADAPTERS | _lib.FIND_CLIP | _lib.FIND_ADAPTER_MISMATCHES
        assert fo.a.n_probes == 2 and list(fo.a.lens)[:3] == [12, 32, 0] and bytes(fo.a.probes[1]) == A.P32
        calls = o.setters()
        assert [n for n, _ in calls] == ['kvq_scan_set_profile', 'kvq_scan_set_adapters', 'kvq_scan_set_clip', 'kvq_scan_set_adapter_mismatches']
        assert calls[-1][1] == (per,)
    o = ScanOptions(adapters=True, adapter_mismatches=True)
    assert o.profile == [] and [n for n, _ in o.setters()] == ['kvq_scan_set_profile', 'kvq_scan_set_adapters', 'kvq_scan_set_adapter_mismatches']


def test_command_line(tmp_path, monkeypatch):
    """``python -m kvarq_amd.profile FILE --adapters --clip --adapter-mismatches [PER]``, the scan replaced by the twins"""
    p = A.P12.decode()
    text = ''.join('@r\n%s\n+\n%s\n' % (b, 'I' * len(b)) for b in ('CC' + p + 'TT', 'CC' + p[:5] + 'N' + p[6:] + 'TT')).encode()
    (tmp_path / 't.fastq').write_bytes(text)
    seen = []

    def by_twin(fnames, cutoffs=True, inflate='host', **options):
        seen.append(options)
        with open(fnames[0], 'rb') as f:
            data = f.read()
        return P.profile_host(data, [ord('I')], [0, len(data)], adapters=options.get('adapters'), clip=options.get('clip'),
                              adapter_mismatches=options.get('adapter_mismatches'))
    monkeypatch.setattr(P, 'profile', by_twin)

    def run(*args):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            P.main([str(tmp_path / 't.fastq')] + list(args))
        return out.getvalue().strip().split('\n')
    said = run('--adapters', 'mine=' + p, '--clip', 'mine=' + p, '--adapter-mismatches')
    assert seen[-1]['adapter_mismatches'] == 10
    assert said[-2].startswith('mine ' + p + ': found=2') and said[-2].endswith(' mismatches(1 per 10)=1/1/0/0')
    assert said[-1] == 'clip: records=2 clipped=2 (1.0000) masked=28 bases_cut=28 mismatches=1 per 10'
    said = run('--adapters', 'mine=' + p, '--adapter-mismatches', '32')
    assert seen[-1]['adapter_mismatches'] == 32 and said[-1].endswith('found=1 (0.5000) first cycle=2 beyond=0 tails=0 mismatches(1 per 32)=1/0/0/0')
    said = run('--adapters', 'mine=' + p)
    assert 'adapter_mismatches' not in seen[-1] and 'mismatches' not in said[-1]
    for bad in (['--adapter-mismatches'], ['--clip', '--adapter-mismatches', '9'], ['--clip', '--adapter-mismatches', '33']):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            P.main([str(tmp_path / 't.fastq')] + bad)


def test_twins_under_the_sanitizers_as_a_program_of_their_own(tmp_path):
    """tests/adapt_mm_twin_main.cpp, built with -fsanitize=address,undefined, over `overhang` and `tails` in a heap block of exactly
    the text's size: the program's output is MASK_per(text), the adapters array and the eight words"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no C++ compiler'
    exe = str(tmp_path / 'adapt_mm_twin_main')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(HERE, 'adapt_mm_twin_main.cpp')], check=True, capture_output=True, timeout=300)
    for name in ('overhang', 'tails'):
        text, probes, _, _ = M.texts()[name]
        (tmp_path / 't.fastq').write_bytes(text)
        p = subprocess.run([exe, str(tmp_path / 't.fastq'), str(tmp_path / 'out.bin'), '10'] + [q.decode() for q in probes],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-2000:]
        got = (tmp_path / 'out.bin').read_bytes()
        co = [0, len(text)]
        want, words = M.mask(text, co, probes, 10)
        tail = np.frombuffer(got[len(text):], dtype=np.int64)
        assert got[:len(text)] == want and (tail[:A.LEN] == M.adapt(text, co, probes, 10)).all() and (tail[A.LEN:] == words).all()
