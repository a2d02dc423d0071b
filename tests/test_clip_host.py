"""
The adapter clip without a GPU (include/kvarq_hip.h): the CPU twin ``kvq_clip_host`` against the plain statement
of the definition (tests/clip_ref.py) on every text -- each asserts its census first --, under chunk cuts and batch cuts, twice
(MASK is idempotent); the oracle on MASK(reveal), which gives exactly the predicted (file_pos, readlength) set, and on the text as
it lies, which does not; the refusals; what ``ScanOptions`` hands to the library; and the twin as a program of its own under
AddressSanitizer and UBSan, on a buffer that ends with the text's last byte.
"""
import collections
import contextlib
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import adapt_ref as A
import clip_ref as CR
from kvarq_amd import _lib, profile as P
from kvarq_amd.options import ScanOptions
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


def texts():
    """name -> (text, chunk offsets)"""
    redo = CR.redo_text()
    return {'stores': (CR.stores_text()[0], None), 'reveal': (CR.reveal_text()[0], None), 'redo': (redo[0], list(redo[3])),
            'quirk': (CR.quirk_text(), None), 'none': (CR.none_text(), None)}


def test_the_texts_reach_their_seams():
    CR.stores_census()
    c = CR.reveal_census('reveal')
    assert c['records'] > 700
    c = CR.reveal_census('redo')
    assert c['records'] > 800
    A.check_census('none')


@pytest.mark.parametrize('n', sorted(CR.PROBES))
@pytest.mark.parametrize('name', sorted(texts()))
def test_twin_is_the_definition(name, n):
    text, co = texts()[name]
    probes = CR.PROBES[n]
    co = [0, len(text)] if co is None else co
    want, words = CR.mask(text, co, probes)
    got, gw = P.clip_host(text, probes, co)
    bad = np.nonzero(got != np.frombuffer(want, dtype=np.uint8))[0]
    assert bad.size == 0, bad[:8]
    assert (gw == words).all(), (gw, words)
    assert gw[CR.C_N] == n and gw[CR.C_CLIPPED] <= gw[CR.C_RECORDS] and not gw[5:].any()
    # idempotent: the same bytes, the same words -- [3] counts positions, not changes
    twice, tw = P.clip_host(got, probes, co)
    assert (twice == got).all() and (tw == gw).all()
    again, aw = CR.mask(want, co, probes)
    assert again == want and (aw == words).all()
    if name == 'none':
        assert bytes(got) == text and gw[CR.C_CLIPPED] == 0 and gw[CR.C_RECORDS] == 47
    else:
        assert gw[CR.C_CLIPPED] > 0 and bytes(got) != text
    # only score bytes changed, and only to '!'
    changed = np.nonzero(got != np.frombuffer(text, dtype=np.uint8))[0]
    assert (got[changed] == 0x21).all() and changed.size <= gw[CR.C_MASKED]


@pytest.mark.parametrize('name', ['stores', 'redo'])
def test_chunk_cuts_and_batch_cuts(name):
    """only the whole records of a chunk are masked and counted; the twin ADDS over batches cut between records"""
    text, _ = texts()[name]
    probes = CR.PROBES[2]
    ends = CR.record_ends(text)
    want, words = CR.mask(text, [0, len(text)], probes)
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    got, gw = P.clip_host(text, probes, cuts)                                           # three chunks cut between records: the same
    assert bytes(got) == want and (gw == words).all()
    acc, parts = np.zeros(CR.LEN, dtype=np.int64), []
    for x, y in zip(cuts, cuts[1:]):                                                    # three batches
        part, _ = P.clip_host(text[x:y], probes, [0, y - x], into=acc)
        parts.append(bytes(part))
    assert b''.join(parts) == want and (acc == words).all()
    # a cut inside a record: every four newlines of a chunk are a record, whatever they are -- the python statement says the same
    mid = text.index(b'\n', ends[10]) + 3                                             # (inside a bases line: the chunk behind it counts its newlines from there)
    co = [0, mid, len(text)]
    want2, words2 = CR.mask(text, co, probes)
    got2, gw2 = P.clip_host(text, probes, co)
    assert bytes(got2) == want2 and (gw2 == words2).all() and want2 != want


def by_hand_text():
    p = A.P12.decode()
    lines = [('CC' + p + 'TT', 'IIIIIIIIIIIIIIII'),        # CLIP 2: fourteen positions
             ('CCCC' + p[:7], 'IIIIIIIIIII'),              # a tail of 7: CLIP 4
             ('CTCTCTCT', 'IIIIIIII'),                     # nothing
             ('C' + p, 'II'),                              # S = 2 > CLIP = 1: one position
             ('CT' + p, 'I')]                              # S = 1 <= CLIP = 2: clipped, nothing to mask
    return ''.join('@r\n%s\n+\n%s\n' % bq for bq in lines).encode()


def test_by_hand():
    text = by_hand_text()
    got, w = P.clip_host(text, [A.P12], [0, len(text)])
    assert bytes(got).split(b'\n')[3::4] == [b'II' + b'!' * 14, b'IIII' + b'!' * 7, b'IIIIIIII', b'I!', b'I']
    assert w.tolist() == [1, 5, 4, 14 + 7 + 1 + 0, 14 + 7 + 12 + 12, 0, 0, 0]
    c = P.Clip(w, ['a'], [A.P12])
    assert (c.records, c.clipped, c.masked, c.bases_cut) == (5, 4, 22, 45) and c['masked'] == 22 and (c['words'] == w).all()
    assert c.line() == 'clip: records=5 clipped=4 (0.8000) masked=22 bases_cut=45' and c == P.Clip(w.copy())
    # '\r' on both lines: neither is part of its line, neither is touched
    text = b'@r\r\nCC' + A.P12 + b'\r\n+\r\nIIIIIIIIIIIIII\r\n'
    got, w = P.clip_host(text, [A.P12], [0, len(text)])
    assert bytes(got) == b'@r\r\nCC' + A.P12 + b'\r\n+\r\nII!!!!!!!!!!!!\r\n' and w.tolist()[:5] == [1, 1, 1, 12, 12]


def test_profile_host_with_clip_is_the_profile_of_the_masked_text():
    text, _ = texts()['reveal']
    co = [0, len(text)]
    probes = CR.PROBES[2]
    masked, words = CR.mask(text, co, probes)
    p = P.profile_host(text, '.', co, cycles=True, adapters=probes, clip=probes)
    q = P.profile_host(masked, '.', co, cycles=True, adapters=probes)
    assert p == q and (p.clipped.words == words).all() and q.clipped is None
    assert p != P.profile_host(text, '.', co, cycles=True, adapters=probes)
    # the identities of the eight words against the adapter content of the same probes
    a = p.adapters
    assert words[CR.C_RECORDS] == a.records and words[CR.C_CLIPPED] == a.with_adapter + a.tail_only
    raw, clip = p.raw_lengths, a.clip
    assert raw[1024] == 0 and words[CR.C_BASES_CUT] == (np.arange(1025) * raw).sum() - (np.arange(1025) * clip).sum()


def test_the_oracle_on_the_masked_text_reveals_the_mask():
    """every record of `reveal` whose MASKED trim leaves minreadlength is a hit with (file_pos, readlength) of that trim: the oracle,
    unchanged, is the yardstick of everything behind the mask.  A mask that begins a byte early or late gives another set"""
    seqs = CR.TM.table()
    for which in ('reveal', 'redo'):
        if which == 'reveal':
            text, read_off, _ = CR.reveal_text(); co = [0, len(text)]
        else:
            text, read_off, _, co = CR.redo_text()
        want, _ = CR.revealed(text, read_off, co, CR.PROBES[2])
        masked, _ = P.clip_host(text, CR.PROBES[2], co)
        o = O.scan_memory(masked, seqs, **CR.CFG)
        assert {(h.file_pos, h.readlength) for h in o['hits']} == want and len(want) > 600
        plain = O.scan_memory(np.frombuffer(text, dtype=np.uint8), seqs, **CR.CFG)
        assert {(h.file_pos, h.readlength) for h in plain['hits']} != want
    # one byte off at the lower end, either way
    text, read_off, _ = CR.reveal_text()
    arr = np.frombuffer(text, dtype=np.uint8)
    for shift in (-1, 1):
        off = arr.copy()
        for n2, L, clip, S in CR.per_record(text, [0, len(text)], CR.PROBES[2]):
            lo = max(clip + shift, 0)
            off[n2 + 1 + lo:n2 + 1 + S] = 0x21
        o = O.scan_memory(off, seqs, **CR.CFG)
        assert {(h.file_pos, h.readlength) for h in o['hits']} != want


def test_refusals():
    text = A.rec(b'ACGT' * 10)
    L = _lib.lib()
    arr = np.frombuffer(text, dtype=np.uint8).copy()
    co = np.array([0, len(text)], dtype=np.int64)
    out = np.zeros(CR.LEN, dtype=np.int64)

    def call(probes, n=None):
        k = max(len(probes), 1)
        return L.kvq_clip_host(arr.ctypes.data, arr.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), 1, (C.c_char_p * k)(*probes),
                               (C.c_int32 * k)(*([len(p) for p in probes] or [0])), len(probes) if n is None else n,
                               out.ctypes.data_as(C.POINTER(C.c_int64)))
    assert call([A.P12]) == 0
    for probes, n in (([A.P12], 0), ([A.P12] * 9, 9), ([b'ACGTACG'], 1), ([b'A' * 33], 1), ([b'ACGTACGa'], 1), ([b'ACGTNCGT'], 1), ([A.P12, b'ACGTACG.'], 2)):
        assert call(probes, n) == _lib.ERR_RUNTIME and 'upper-case A C G T' in _lib.last_error()[1], probes
    assert out[CR.C_RECORDS] == 1 and bytes(arr) == text                  # (a refused call adds nothing and writes nothing)
    for bad in ([], [A.P12] * 9, [b'ACGTACG'], [b'A' * 33], [b'ACGTACGa'], [b'ACGTNCGT']):
        with pytest.raises(ValueError):
            ScanOptions(clip=bad)
    # adapters= and clip= name the same probes: one rule, because findseqs has one probe block
    with pytest.raises(ValueError, match='same probes'):
        ScanOptions(adapters=[A.P12], clip=[A.P32])
    with pytest.raises(ValueError, match='same probes'):
        ScanOptions(adapters=[A.P12, A.P32], clip=[A.P12])
    with pytest.raises(ValueError, match='same probes'):
        ScanOptions(adapters=True, clip=[A.P12])
    assert ScanOptions(adapters=True, clip=True).clip == ScanOptions(adapters=True).adapters
    # an Amin that '!' does not fall below, as a signed char: '!' itself, 0x05, 0x80 (refused where the table's Amin is known:
    # Scanner; the library refuses the same, tests/test_gpu_clip.py)
    for amin in (b'!', b'\x05', b'\x80'):
        with pytest.raises(ValueError, match="above '!'"):
            ScanOptions(clip=True, amin=amin)
    for amin in (b'"', b'.', b'\x7f'):
        assert ScanOptions(clip=True, amin=amin).clip


def test_scan_options():
    off = ScanOptions(profile=[ord('I')], cycles=True)
    fo = off.find_opts()
    assert type(fo) is _lib.FindOpts and C.sizeof(fo) == 20 and fo.size == 20 and off.clip is None       # the 20 bytes stay with the clip off
    for none in (None, False):
        o = ScanOptions(clip=none)
        assert o.clip is None and o.profile is None and o.find_opts().size == 20 and o.setters() == []
    on = ScanOptions(clip=[A.P12, A.P32])
    assert on.profile is None and on.adapters is None and on.clip == [A.P12, A.P32] and on.clip_names == ['probe 0', 'probe 1']     # no profile needed
    fo = on.find_opts(1)
    assert type(fo) is _lib.FindOptsAdapters and fo.base.flags == 1 | _lib.FIND_CLIP == 2049 and fo.base.size == C.sizeof(_lib.FindOptsAdapters)
    assert fo.n_probes == 2 and list(fo.lens) == [12, 32, 0, 0, 0, 0, 0, 0] and bytes(fo.probes[0]) == A.P12 + bytes(20) and bytes(fo.probes[1]) == A.P32
    (name, (arr, lens, n)), = on.setters()
    assert name == 'kvq_scan_set_clip' and n == 2 and list(lens) == [12, 32] and list(arr) == [A.P12, A.P32]
    both = ScanOptions(clip=collections.OrderedDict([('x', A.P12)]), adapters=[A.P12], profile='I', long_reads=True)
    assert both.find_opts().base.flags == _lib.FIND_PROFILE | _lib.FIND_ADAPTERS | _lib.FIND_CLIP | _lib.FIND_LONG_READS and both.clip_names == ['x']
    assert [name for name, _ in both.setters()] == ['kvq_scan_set_profile', 'kvq_scan_set_adapters', 'kvq_scan_set_clip', 'kvq_scan_set_long_reads']
    assert ScanOptions(clip=True).clip == [v for v in P.KNOWN_SOURCES.values() if isinstance(v, bytes)]
    assert _lib.lib().kvq_clip_len() == CR.LEN == P.CLIP_LEN == 8


def test_command_line(tmp_path, monkeypatch):
    """``python -m kvarq_amd.profile FILE --clip [NAME=SEQ ...]``, the scan replaced by the twin"""
    text = by_hand_text()
    (tmp_path / 't.fastq').write_bytes(text)
    seen = []

    def by_twin(fnames, cutoffs=True, inflate='host', **options):
        seen.append(options)
        with open(fnames[0], 'rb') as f:
            data = f.read()
        return P.profile_host(data, [ord('I')], [0, len(data)], clip=options.get('clip'))
    monkeypatch.setattr(P, 'profile', by_twin)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--clip', 'mine=' + A.P12.decode()])
    assert list(seen[-1]['clip'].items()) == [('mine', A.P12)] and 'adapters' not in seen[-1]
    assert out.getvalue().strip().split('\n')[-1] == 'clip: records=5 clipped=4 (0.8000) masked=22 bases_cut=45'
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--clip'])
    assert seen[-1]['clip'] is True and 'clip: records=5 clipped=4' in out.getvalue()      # (the universal adapter's probe is P12)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq')])
    assert 'clip' not in seen[-1] and 'clip:' not in out.getvalue()


def test_twin_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """tests/clip_twin_main.cpp, built with -fsanitize=address,undefined: the stores text in a heap block of exactly its size (its
    last record's newline is the block's last byte), masked twice; the program's output is MASK(text) and the eight words"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no C++ compiler'
    exe = str(tmp_path / 'clip_twin_main')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(HERE, 'clip_twin_main.cpp')], check=True, capture_output=True, timeout=300)
    text = CR.stores_text()[0]
    (tmp_path / 'stores.fastq').write_bytes(text)
    for n in (2, 8):
        probes = CR.PROBES[n]
        p = subprocess.run([exe, str(tmp_path / 'stores.fastq'), str(tmp_path / 'out.bin')] + [q.decode() for q in probes],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, p.stderr[-2000:]
        got = (tmp_path / 'out.bin').read_bytes()
        want, words = CR.mask(text, [0, len(text)], probes)
        assert got[:len(text)] == want and (np.frombuffer(got[len(text):], dtype=np.int64) == words).all()
