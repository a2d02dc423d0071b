"""
The emitted reads without a GPU (include/kvarq_hip.h): the CPU twin ``kvq_emit_host`` against the plain
statement of the definition (tests/emit_ref.py) on every text -- each asserts its census first --, under chunk cuts and batch
cuts; by hand; the contract with the clip, stated on the twins; the options, the structure of ``findseqs`` and the refusals; the
command line; and the twin as a program of its own under AddressSanitizer and UBSan, its input ending with the text's last byte
and its output exactly ``nbytes + nrec`` long.
"""
import contextlib
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import clip_ref as CR
import emit_ref as E
from kvarq_amd import _lib, profile as P
from kvarq_amd.options import ScanOptions, as_emit

HERE = os.path.dirname(os.path.abspath(__file__))


def texts():
    """name -> (text, chunk offsets, the min_lengths to emit it with)"""
    redo = CR.redo_text()
    empty = E.empty_chunk_case()
    return {'copies': (E.copies_text()[0], None, (0,)), 'trims': (E.trims_text()[0], None, (E.MINLEN, 0, 1)),
            'dropped': (E.dropped_text(), None, (E.MINLEN, 31)), 'empty-chunks': (empty[0], list(empty[1]), (E.MINLEN,)),
            'reveal': (CR.reveal_text()[0], None, (E.MINLEN, 0)), 'redo': (redo[0], list(redo[3]), (E.MINLEN,)),
            'quirk': (CR.quirk_text(), None, (E.MINLEN,))}


def test_the_texts_reach_their_seams():
    c = E.copies_census()
    assert c['cells'] == 16 * 16 * 146 and c['records'] < 14000
    c = E.trims_census()
    assert c['records'] == 44
    for n in E.COUNTS:
        E.counts_census(n)
    E.dropped_census()
    assert E.SCAN_BLOCK ** 2 + 1 in E.COUNTS and max(E.COUNTS) > 70000


@pytest.mark.parametrize('name', sorted(texts()))
def test_twin_is_the_definition(name):
    text, co, mins = texts()[name]
    co = [0, len(text)] if co is None else co
    for m in mins:
        want, words = E.emit(text, co, E.AMIN, m)
        got, gw = P.emit_host(text, E.AMIN, m, co)
        assert bytes(got) == want and (gw == words).all(), (name, m, gw, words)
        assert gw[E.N] == m
        E.check_identities(gw, len(got))
        if name == 'dropped':
            assert len(got) == 0 and gw[E.EMITTED] == 0 and gw[E.RECORDS] == 600
        else:
            assert gw[E.EMITTED] > 0
        # the emitted text is FastQ: four lines a record, a bare '+' the third, bases and scores of one length
        lines = want.split(b'\n')
        assert lines[-1] == b'' and len(lines) == 4 * gw[E.EMITTED] + 1
        assert set(lines[2:-1:4]) <= {b'+'} and all(len(b) == len(q) for b, q in zip(lines[1:-1:4], lines[3:-1:4]))


@pytest.mark.parametrize('n', E.COUNTS)
def test_twin_on_the_counts(n):
    text = E.counts_text(n)
    want, words = E.emit(text, [0, len(text)])
    got, gw = P.emit_host(text, E.AMIN, E.MINLEN, [0, len(text)])
    assert bytes(got) == want and (gw == words).all() and gw[E.RECORDS] == n


@pytest.mark.parametrize('amin', [ord('!'), ord('I'), 0x7E, 0x05, 0x0A, 0x0B, 0x80, 0xFF])
def test_twin_at_the_edges_of_the_signed_compare(amin):
    """cutoffs around the newline's byte (which closes the last run only when it is below the cutoff) and the sign bit"""
    text = E.trims_text()[0]
    want, words = E.emit(text, [0, len(text)], amin, 1)
    got, gw = P.emit_host(text, amin, 1, [0, len(text)])
    assert bytes(got) == want and (gw == words).all()
    if amin in (0x05, 0x0A, 0x80):
        assert gw[E.EMITTED] <= 2           # (no newline closes a run there: only a line that holds a lower byte has one)


def test_chunk_cuts_and_batch_cuts():
    """only the whole records of a chunk are emitted; the twin ADDS its words over batches cut between records; a cut inside a
    record makes the chunk behind it count its newlines from there -- and begin its first name there"""
    text = CR.reveal_text()[0]
    ends = E.record_ends(text)
    want, words = E.emit(text, [0, len(text)])
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    got, gw = P.emit_host(text, E.AMIN, E.MINLEN, cuts)
    assert bytes(got) == want and (gw == words).all()
    acc, parts = np.zeros(E.LEN, dtype=np.int64), []
    for x, y in zip(cuts, cuts[1:]):
        part, _ = P.emit_host(text[x:y], E.AMIN, E.MINLEN, [0, y - x], into=acc)
        parts.append(bytes(part))
    assert b''.join(parts) == want and (acc == words).all()
    mid = text.index(b'\n', ends[10]) + 3
    co = [0, mid, len(text)]
    want2, words2 = E.emit(text, co)
    got2, gw2 = P.emit_host(text, E.AMIN, E.MINLEN, co)
    assert bytes(got2) == want2 and (gw2 == words2).all() and want2 != want


def test_by_hand():
    text = (b'@a 1\r\nACGTACGTAC\r\n+a 1\r\nIIII#IIIII\r\n'      # runs of 4 and 5 ('\r' is a low score): the later, longer one
            b'@b\nACGT\n+\nII#\n'                                # bases and scores differ: dropped
            b'@c\nAC\n+\n##\n'                                   # nothing survives
            b'@d\nACGTA\n+\nII#II\n')                            # equal runs: the first
    out, w = P.emit_host(text, 'I', 2, [0, len(text)])
    assert bytes(out) == b'@a 1\nCGTAC\n+\nIIIII\n@d\nAC\n+\nII\n'
    assert w.tolist() == [2, 4, 2, 1, 1, 11 + 4 + 2 + 5, 7, 30]
    out, w = P.emit_host(text, 'I', 0, [0, len(text)])
    assert bytes(out) == b'@a 1\nCGTAC\n+\nIIIII\n@c\n\n+\n\n@d\nAC\n+\nII\n' and w.tolist() == [0, 4, 3, 0, 1, 22, 7, 37]
    e = P.Emit(w)
    assert (e.records, e.emitted, e.short, e.mismatched, e.bases_in, e.bases_out, e.bytes_out, e.min_length) == (4, 3, 0, 1, 22, 7, 37, 0)
    assert e['emitted'] == 3 and (e['words'] == w).all() and e == P.Emit(w.copy())
    with pytest.raises(KeyError):
        e['min_length']
    assert e.line() == 'emit: records=4 emitted=3 (0.7500) short=0 mismatched=1 bases 22 -> 7 bytes_out=37 min_length=0'
    # an emitted record is at most its input record plus one byte: a third line that is empty
    text = b'@e\nACGT\n\nIIII\n'
    out, w = P.emit_host(text, 'I', 0, [0, len(text)])
    assert bytes(out) == b'@e\nACGT\n+\nIIII\n' and len(out) == len(text) + 1


def test_the_contract_with_the_clip_on_the_twins():
    """EMIT(MASK(text)) differs from EMIT(text), never holds a mask byte, and every emitted read ends in front of its adapter"""
    text = CR.reveal_text()[0]
    co = [0, len(text)]
    masked, cw = P.clip_host(text, CR.PROBES[2], co)
    a, aw = P.emit_host(masked, E.AMIN, E.MINLEN, co)
    b, bw = P.emit_host(text, E.AMIN, E.MINLEN, co)
    want, words = E.emit(CR.mask(text, co, CR.PROBES[2])[0], co)
    assert bytes(a) == want and (aw == words).all() and bytes(a) != bytes(b) and aw[E.BASES_OUT] < bw[E.BASES_OUT]
    assert not any(b'!' in q for q in bytes(a).split(b'\n')[3::4])
    assert not any(CR.PROBES[2][0] in r for r in bytes(a).split(b'\n')[1::4]) and any(CR.PROBES[2][0] in r for r in bytes(b).split(b'\n')[1::4])


def test_refusals_of_the_twin():
    L = _lib.lib()
    text = np.frombuffer(b'@r\nACGT\n+\nIIII\n', dtype=np.uint8)
    co = np.array([0, text.nbytes], dtype=np.int64)
    out, words = np.zeros(64, dtype=np.uint8), np.zeros(E.LEN, dtype=np.int64)

    def call(min_length=0, cap=64, co=co, w=words):
        return L.kvq_emit_host(text.ctypes.data, text.nbytes, co.ctypes.data_as(C.POINTER(C.c_int64)), len(co) - 1, ord('I'), min_length,
                               out.ctypes.data, cap, w.ctypes.data_as(C.POINTER(C.c_int64)) if w is not None else None)
    assert call() == 15 and bytes(out[:15]) == bytes(text)
    assert call(min_length=-1) == -1 and 'bad arguments' in _lib.last_error()[1]
    assert call(w=None) == -1 and call(co=np.array([0, 99], dtype=np.int64)) == -1 and call(co=np.array([5, 2], dtype=np.int64)) == -1
    assert call(cap=14) == -1 and 'out_cap' in _lib.last_error()[1]
    assert call(cap=15) == 15                                             # nbytes + nrec = 16 always holds it; so does the exact length
    assert L.kvq_emit_len() == E.LEN == P.EMIT_LEN == 8


def test_scan_options():
    off = ScanOptions(profile=[ord('I')], cycles=True)
    fo = off.find_opts()
    assert type(fo) is _lib.FindOpts and C.sizeof(fo) == 20 and fo.size == 20 and off.emit is None and off.emit_min == -1      # the 20 bytes stay with the emit off
    for none in (None, False):
        o = ScanOptions(emit=none)
        assert o.emit is None and o.profile is None and o.find_opts().size == 20 and o.setters() == []
    with_probes = ScanOptions(clip=CR.PROBES[2], adapter_mismatches=12)
    assert type(with_probes.find_opts()) is _lib.FindOptsAdaptersMm and with_probes.find_opts().a.base.size == 292       # ... and so do the 288 and the 292
    on = ScanOptions(emit='out.fastq')
    assert on.emit == b'out.fastq' and on.emit_min == -1 and on.profile is None and on.clip is None                       # no profile needed
    fo = on.find_opts(1)
    assert type(fo) is _lib.FindOptsEmit and C.sizeof(fo) == 304 and fo.m.a.base.size == 304 and fo.m.a.base.flags == 1 | _lib.FIND_EMIT == 8193
    assert fo.min_length == -1 and fo.path == b'out.fastq' and fo.m.mismatch_per == 0 and fo.m.a.n_probes == 0
    assert _lib.FindOptsEmit.min_length.offset == 292 and _lib.FindOptsEmit.path.offset == 296
    assert on.setters() == [('kvq_scan_set_emit', (1, -1))]
    both = ScanOptions(emit=os.path.join('a', 'b.fq'), emit_min=0, clip=CR.PROBES[2], adapter_mismatches=True, profile='I', long_reads=True)
    fo = both.find_opts()
    assert type(fo) is _lib.FindOptsEmit and fo.min_length == 0 and fo.m.mismatch_per == 10 and fo.m.a.n_probes == 2
    assert fo.m.a.base.flags == _lib.FIND_PROFILE | _lib.FIND_CLIP | _lib.FIND_ADAPTER_MISMATCHES | _lib.FIND_LONG_READS | _lib.FIND_EMIT
    assert bytes(fo.m.a.probes[1]) == CR.PROBES[2][1].ljust(32, b'\0')
    assert [n for n, _ in both.setters()] == ['kvq_scan_set_profile', 'kvq_scan_set_clip', 'kvq_scan_set_adapter_mismatches', 'kvq_scan_set_long_reads', 'kvq_scan_set_emit']
    assert both.setters()[-1][1] == (1, 0)
    # True: handed back by Scanner; findseqs has nowhere to hand it to
    t = ScanOptions(emit=True, emit_min=np.int64(7))
    assert t.emit is True and t.emit_min == 7 and t.setters() == [('kvq_scan_set_emit', (1, 7))]
    with pytest.raises(ValueError, match='path'):
        t.find_opts()
    for bad in (-1, 1.5, '3', True, b'3', 1 << 31):
        with pytest.raises(ValueError, match='emit_min'):
            ScanOptions(emit=True, emit_min=bad)
    with pytest.raises(ValueError, match='emit='):
        ScanOptions(emit_min=3)
    for bad in (3, '', b'', [1]):
        with pytest.raises(ValueError, match='emit is'):
            ScanOptions(emit=bad)
    assert as_emit(None) == (None, -1) and as_emit('x', 0) == (b'x', 0)


def test_command_line(tmp_path, monkeypatch):
    """``python -m kvarq_amd.profile FILE --emit OUT [--emit-min N]``, the scan replaced by the twin"""
    text = b'@a\nACGTACGTAC\n+\nIIII#IIIII\n@b\nACGT\n+\nII#\n'
    (tmp_path / 't.fastq').write_bytes(text)
    seen = []

    def by_twin(fnames, cutoffs=True, inflate='host', **options):
        seen.append(options)
        with open(fnames[0], 'rb') as f:
            data = f.read()
        p = P.profile_host(data, [ord('I')], [0, len(data)])
        if options.get('emit'):
            out, w = P.emit_host(data, 'I', options.get('emit_min', 3), [0, len(data)])
            with open(options['emit'], 'wb') as f:
                f.write(bytes(out))
            p.emitted = P.Emit(w)
        return p
    monkeypatch.setattr(P, 'profile', by_twin)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--emit', str(tmp_path / 'o.fastq'), '--emit-min', '5'])
    assert seen[-1]['emit'] == str(tmp_path / 'o.fastq') and seen[-1]['emit_min'] == 5
    assert (tmp_path / 'o.fastq').read_bytes() == b'@a\nCGTAC\n+\nIIIII\n'
    assert out.getvalue().strip().split('\n')[-1] == 'emit: records=2 emitted=1 (0.5000) short=0 mismatched=1 bases 14 -> 5 bytes_out=17 min_length=5'
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq'), '--emit', str(tmp_path / 'o.fastq')])
    assert 'emit_min' not in seen[-1] and 'emit:' in out.getvalue()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        P.main([str(tmp_path / 't.fastq')])
    assert 'emit' not in seen[-1] and 'emit:' not in out.getvalue()
    for bad in (['--emit-min', '3'], ['--emit', 'x', '--emit-min', '-1']):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            P.main([str(tmp_path / 't.fastq')] + bad)


def test_twin_under_the_sanitizers_as_a_program_of_its_own(tmp_path):
    """tests/emit_twin_main.cpp, built with -fsanitize=address,undefined: the text in a heap block of exactly its size, the output
    in one of exactly nbytes + nrec bytes; the program's output is EMIT(text) and the eight words"""
    cxx = os.environ.get('CXX') or next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no C++ compiler'
    exe = str(tmp_path / 'emit_twin_main')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                    os.path.join(HERE, 'emit_twin_main.cpp')], check=True, capture_output=True, timeout=300)
    for name, text, amin, m in (('copies', E.copies_text()[0], E.AMIN, 0), ('trims', E.trims_text()[0], E.AMIN, E.MINLEN),
                                ('trims-low', E.trims_text()[0], 0x05, 0), ('dropped', E.dropped_text(), E.AMIN, E.MINLEN),
                                # every record as long as its input plus one byte: the output fills its block to the last byte
                                ('plus-one', b'@e\nACGT\n\nIIII\n' * 50, ord('I'), 0)):
        (tmp_path / 'in.fastq').write_bytes(text)
        p = subprocess.run([exe, str(tmp_path / 'in.fastq'), str(tmp_path / 'out.bin'), str(amin), str(m)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and 'Sanitizer' not in p.stderr and 'runtime error' not in p.stderr, (name, p.returncode, p.stderr[-2000:])
        got = (tmp_path / 'out.bin').read_bytes()
        want, words = E.emit(text, [0, len(text)], amin, m)
        assert got[:-64] == want and (np.frombuffer(got[-64:], dtype=np.int64) == words).all(), name
        if name == 'plus-one':
            assert len(want) == len(text) + 50
