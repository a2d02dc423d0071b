"""
The adapter content without a GPU (include/kvarq_hip.h): the CPU twin ``kvq_adapt_host`` against the plain
statement of the definition (tests/adapt_ref.py) on every seam text and on random records, the identities of the array, the
refusals, what ``ScanOptions`` hands to the library, the ``Profile`` accessors and the command line's lines.
"""
import collections
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import adapt_ref as A
from kvarq_amd import _lib, profile as P
from kvarq_amd.options import ScanOptions


def twin(text, probes, co=None):
    return P.adapt_host(text, probes, [0, len(text)] if co is None else co)


@pytest.mark.parametrize('name', sorted(A.texts()))
def test_twin_is_the_definition_on_every_seam_text(name):
    A.check_census(name)
    text, probes = A.texts()[name]
    want = A.adapt(text, [0, len(text)], probes)
    got = twin(text, probes)
    bad = np.nonzero(got.words != want)[0]
    assert bad.size == 0, (bad[:8], got.words[bad[:8]], want[bad[:8]])
    A.check_identities(got.words, P.profile_host(text, (), [0, len(text)]).words)


def test_twin_is_the_definition_on_random_records():
    text, probes = A.random_text()
    want = A.adapt(text, [0, len(text)], probes)
    assert want[A.A_RECORDS] == 2000 and want[A.A_WITH_FULL] > 300 and want[A.A_TAIL_ONLY] > 20
    got = twin(text, probes)
    assert (got.words == want).all()
    A.check_identities(got.words)
    # chunks: only whole records of a chunk count, and the twin ADDS
    cut = text.index(b'\n@', len(text) // 3) + 1
    words = np.zeros(A.LEN, dtype=np.int64)
    L = _lib.lib()
    n = len(probes)
    for a, b in ((0, cut), (cut, len(text))):
        part = np.frombuffer(text[a:b], dtype=np.uint8)
        co = np.array([0, b - a], dtype=np.int64)
        assert L.kvq_adapt_host(part.ctypes.data, part.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 1, (C.c_char_p * n)(*probes),
                                (C.c_int32 * n)(*[len(p) for p in probes]), n, words.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert (words == want).all()


def test_none_text_is_the_raw_lengths():
    text, probes = A.texts()['none']
    prof = P.profile_host(text, (), [0, len(text)], adapters=probes)
    assert (prof.adapters.clip == prof.raw_lengths).all() and prof.adapters.records == prof.records
    assert prof.adapter_share() == 0.0 and prof.clipped_share() == 0.0 and not prof.adapter_content().any()


def test_by_hand():
    # one probe of twelve; T = 6
    p = A.P12
    text = b''.join(A.rec(b) for b in (b'CC' + p + b'TT', p[:6], b'CCCC' + p[:11], b'CT' * 10, p[:5], b'', b'TT' + p + b'C' + p))
    a = twin(text, [p])
    assert (a.records, a.with_adapter, a.tail_only) == (7, 2, 2) and a.lengths == [12] and a.names == ['probe 0'] and a.probes == [p]
    assert a.first[0, 2] == 2 and a.first.sum() == 2 and a.beyond[0] == 0 and a.found[0] == 2
    assert a.tail[0, 6] == 1 and a.tail[0, 11] == 1 and a.tail.sum() == 2 and a.tailed[0] == 2
    assert {int(i): int(a.clip[i]) for i in np.nonzero(a.clip)[0]} == {0: 2, 2: 2, 4: 1, 5: 1, 20: 1}
    # m = 32: the whole line is the probe; a tail of 31
    a = twin(A.rec(A.P32) + A.rec(A.P32[:31]) + A.rec(b'C' + A.P32[1:]), [A.P32])
    assert a.first[0, 0] == 1 and a.tail[0, 31] == 1 and a.clip[0] == 2 and a.clip[32] == 1


def test_refused_probes():
    text = A.rec(b'ACGT' * 10)
    for bad in ([], [A.P12] * 9, [b'ACGTACG'], [b'A' * 33], [b'ACGTACGa'], [b'ACGTNCGT'], [A.P12, b'ACGTACG.']):
        with pytest.raises(ValueError):
            P.as_adapters(bad)
    L = _lib.lib()
    arr = np.frombuffer(text, dtype=np.uint8)
    co = np.array([0, len(text)], dtype=np.int64)
    out = np.zeros(A.LEN, dtype=np.int64)

    def call(probes, n=None, lens=None):
        k = max(len(probes), 1)
        return L.kvq_adapt_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 1, (C.c_char_p * k)(*probes),
                                (C.c_int32 * k)(*(lens or [len(p) for p in probes] or [0])), len(probes) if n is None else n,
                                out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert call([A.P12]) == 0
    for probes, n in (([A.P12], 0), ([A.P12] * 9, 9), ([b'ACGTACG'], 1), ([b'A' * 33], 1), ([b'ACGTACGa'], 1), ([b'ACGTNCGT'], 1), ([A.P12, b'ACGTACG.'], 2)):
        assert call(probes, n) == _lib.ERR_RUNTIME and 'upper-case A C G T' in _lib.last_error()[1], probes
    assert out[A.A_RECORDS] == 1                                   # (a refused call adds nothing)


def test_scan_options():
    off = ScanOptions(profile=[ord('I')], cycles=True)
    fo = off.find_opts()
    assert type(fo) is _lib.FindOpts and C.sizeof(fo) == 20 and fo.size == 20 and fo.flags == _lib.FIND_PROFILE | _lib.FIND_CYCLES
    assert [name for name, _ in off.setters()] == ['kvq_scan_set_profile', 'kvq_scan_set_cycles'] and off.adapters is None
    for none in (None, False):
        assert ScanOptions(adapters=none).profile is None and ScanOptions(adapters=none).find_opts().size == 20
    on = ScanOptions(adapters=[A.P12, A.P32])
    assert on.profile == [] and on.adapters == [A.P12, A.P32] and on.adapter_names == ['probe 0', 'probe 1']
    fo = on.find_opts()
    assert type(fo) is _lib.FindOptsAdapters and fo.base.flags == 8 | 1024 and fo.base.size == C.sizeof(_lib.FindOptsAdapters) == 20 + 4 + 8 + 256
    assert fo.base.n_cutoffs == 0 and fo.n_probes == 2 and list(fo.lens) == [12, 32, 0, 0, 0, 0, 0, 0]
    assert bytes(fo.probes[0]) == A.P12 + bytes(20) and bytes(fo.probes[1]) == A.P32 and not any(bytes(fo.probes[k]).strip(b'\0') for k in range(2, 8))
    assert _lib.FindOptsAdapters.base.offset == 0 and _lib.FindOptsAdapters.n_probes.offset == 20
    calls = on.setters()
    assert [name for name, _ in calls] == ['kvq_scan_set_profile', 'kvq_scan_set_adapters']
    arr, lens, n = calls[1][1]
    assert n == 2 and list(lens) == [12, 32] and list(arr) == [A.P12, A.P32]
    # the three forms
    known = ScanOptions(adapters=True)
    assert known.adapter_names == [k for k, v in P.KNOWN_SOURCES.items() if isinstance(v, bytes)] and len(known.adapters) == 4
    assert known.adapters == [v for v in P.KNOWN_SOURCES.values() if isinstance(v, bytes)]
    named = ScanOptions(adapters=collections.OrderedDict([('mine', 'AGATCGGAAGAGC'), ('yours', A.P8)]), profile='I', duplication=True)
    assert named.adapter_names == ['mine', 'yours'] and named.adapters == [b'AGATCGGAAGAGC', A.P8]
    assert named.find_opts(1).base.flags == 1 | 8 | 256 | 1024
    assert [name for name, _ in named.setters()] == ['kvq_scan_set_profile', 'kvq_scan_set_read_stats', 'kvq_scan_set_adapters']
    with pytest.raises(ValueError):
        ScanOptions(adapters=[b'ACGT'])
    assert _lib.lib().kvq_adapt_len() == A.LEN == P.ADAPT_LEN == 9545


def test_profile_accessors_as_dict_and_eq():
    text, probes = A.texts()['several']
    named = collections.OrderedDict(zip(('a', 'b', 'poly-A', 'd'), probes))
    prof = P.profile_host(text, (), [0, len(text)], adapters=named)
    a = prof.adapters
    want = A.adapt(text, [0, len(text)], probes)
    assert (a.words == want).all() and a.names == list(named) and a.probes == probes and a.first.shape == (4, 1024) and a.tail.shape == (4, 32)
    assert a.clip.shape == (1025,) and a.beyond.shape == (4,) and a.records == 27 == prof.records
    assert prof.adapter_share() == a.with_adapter / 27.0 and prof.clipped_share() == (a.with_adapter + a.tail_only) / 27.0
    curve = prof.adapter_content('poly-A')
    assert curve.shape == (1024,) and curve[0] == 3 / 27.0 and curve[4] == 3 / 27.0 and curve[5] == 6 / 27.0 == curve[1023]
    assert (prof.adapter_content(2) == curve).all()
    assert np.allclose(prof.adapter_content(), sum(prof.adapter_content(k) for k in range(4)))
    lengths = sorted(c for _, _, _, _, c, _ in A.per_record(text, [0, len(text)], probes))
    assert prof.clip_quantile(0.0) == lengths[0] and prof.clip_quantile(1.0) == lengths[-1] and prof.clip_quantile(0.5) == lengths[13]
    with pytest.raises(ValueError):
        prof.clip_quantile(1.5)
    d = prof.as_dict()['adapters']
    assert d['records'] == 27 and [p['name'] for p in d['probes']] == list(named) and d['probes'][2]['first'] == {0: 3, 5: 3}
    assert d['probes'][2]['tail'] == {6: 3, 7: 3} and d['probes'][0]['sequence'] == 'AGATCGGAAGAG' and sum(d['clip'].values()) == 27
    lines = prof.adapter_lines()
    assert lines[0].startswith('adapters: records=27 with_adapter=21') and len(lines) == 2 + 4 and lines[4].startswith('poly-A AAAAAAAA: found=6')
    # __eq__: with and without, and other counts
    plain = P.profile_host(text, (), [0, len(text)])
    assert plain.adapters is None and 'adapters' not in plain.as_dict() and plain != prof and prof != plain
    assert prof == P.profile_host(text, (), [0, len(text)], adapters=named)
    assert prof != P.profile_host(text, (), [0, len(text)], adapters=probes[:3])
    for call in (plain.adapter_content, plain.adapter_share, plain.clipped_share, plain.adapter_lines, lambda: plain.clip_quantile(0.5)):
        with pytest.raises(ValueError):
            call()
    empty = P.profile_host(b'', (), [0], adapters=True)
    assert empty.adapters.records == 0 and np.isnan(empty.adapter_share()) and np.isnan(empty.clip_quantile(0.5)) and empty.adapters.lengths == [12] * 4


def test_command_line_on_a_small_file(tmp_path, monkeypatch):
    """the arguments and the lines of ``python -m kvarq_amd.profile FILE --adapters [NAME=SEQ ...]``, the scan replaced by the twin"""
    text, probes = A.texts()['tails']
    (tmp_path / 't.fastq').write_bytes(text)
    seen = []

    def by_twin(fnames, cutoffs=True, inflate='host', **options):
        seen.append(options)
        with open(fnames[0], 'rb') as f:
            data = f.read()
        return P.profile_host(data, [ord('I')], [0, len(data)], adapters=options.get('adapters'))
    monkeypatch.setattr(P, 'profile', by_twin)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--adapters', 'mine=' + A.P12.decode(), 'long=' + A.P32.decode(), 'periodic=' + A.PERIODIC.decode()])
    want = P.profile_host(text, [ord('I')], [0, len(text)], adapters=collections.OrderedDict([('mine', A.P12), ('long', A.P32), ('periodic', A.PERIODIC)]))
    assert (want.adapters.words == A.adapt(text, [0, len(text)], probes)).all()
    assert out.getvalue().strip() == '\n'.join([want.summary()] + want.adapter_lines())
    assert list(seen[-1]['adapters'].items()) == [('mine', A.P12), ('long', A.P32), ('periodic', A.PERIODIC)]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--adapters'])
    assert seen[-1]['adapters'] is True
    known = P.profile_host(text, [ord('I')], [0, len(text)], adapters=True)
    assert out.getvalue().strip().split('\n')[-6:] == known.adapter_lines() and 'Illumina universal adapter AGATCGGAAGAG: found=3 ' in out.getvalue()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq')])
    assert 'adapters' not in seen[-1] and 'adapters:' not in out.getvalue()
