"""
The emit's deflate on an MI355X (kernels_deflate.hip; include/kvarq_hip.h).  Byte for byte: what
kvq_deflate_bgzf_device makes of a text, and what a scan with ``emit_compress=True`` hands back or writes, is BGZF(text) as the CPU
twin makes it (tests/test_deflate_host.py ties the twin to zlib, to the project's own decoder and to the rule of the parse), batch
by batch, with one EOF member behind it; the eight emit words, the guards and the batch's text are what they are without the
option.  On the texts of tests/deflate_ref.py, on every way a batch can come again, beside the clip and the records, through
``findseqs``; and the round trip: the written file, read on the device-inflate route, gives the hits of the plain emitted text.
"""
import ctypes as C
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_writer as W
import clip_ref as CR
import deflate_ref as D
import emit_ref as E
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

PROBES = CR.PROBES[2]
HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0x5A


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv('KVQ_ARENA_CAP', raising=False)
    monkeypatch.delenv('KVQ_DEFLATE_ROUND', raising=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, chunk offsets, sequences, config) of a scan"""
    if name == 'trims':
        text = E.trims_text()[0]
    elif name == 'counts':
        text = E.counts_text(65537)
    else:
        text = CR.reveal_text()[0]
        return text, tuple(O.chunk_offsets(text)), tuple(CR.TM.table()), E.CFG
    return text, (0, len(text)), tuple(E.SEQ), E.CFG


@functools.lru_cache(maxsize=None)
def emitted(name, clip=False):
    """(EMIT(text) as bytes, the eight words) by the emit's twin"""
    text, co, _, cfg = case(name)
    if clip:
        text = P.clip_host(text, PROBES, list(co))[0]
    out, words = P.emit_host(text, E.AMIN, cfg['minreadlength'], list(co))
    words.flags.writeable = False
    return out.tobytes(), words


@functools.lru_cache(maxsize=None)
def twin(text):
    """(BGZF(text) without the EOF member, the eight words) by the CPU twin; computed once, left unchanged"""
    out, words = P.deflate_bgzf_host(text)
    words.flags.writeable = False
    return out, words


@functools.lru_cache(maxsize=None)
def oracle(name):
    text, _, seqs, cfg = case(name)
    return O.scan_memory(np.frombuffer(text, dtype=np.uint8), list(seqs), fold=True, **dict(cfg, nthreads=4))


def same_as_oracle(r, o):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], k


def device_deflate(text, shift=0, cap=None):
    """kvq_deflate_bgzf_device on the text, uploaded ``shift`` bytes into its buffer, into a buffer of kvq_deflate_bound bytes (or
    ``cap``) with 64 bytes of FILL behind it -> (length, words, the output buffer's bytes with what lies behind)"""
    arr = np.frombuffer(text, dtype=np.uint8)
    cap = _lib.lib().kvq_deflate_bound(len(text)) if cap is None else cap
    d_in, d_out = scan.DeviceBuffer(len(text) + shift), scan.DeviceBuffer(cap + 64)
    if len(text):
        d_in.upload(np.concatenate([np.zeros(shift, dtype=np.uint8), arr]))
    d_out.upload(np.full(cap + 64, FILL, dtype=np.uint8))
    try:
        n, words = scan.deflate_bgzf_device(d_in.ptr + shift, len(text), d_out.ptr, cap)
        return n, words, d_out.download(cap + 64)
    finally:
        d_in.free(); d_out.free()


# ---- the device entry on raw bytes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', D.NAMES)
def test_device_entry_byte_for_byte(name):
    D.text_census(name)
    text = D.text(name)
    want, words = twin(text)
    n, got_words, buf = device_deflate(text)
    assert n == len(want) and (got_words == words).all(), (n, len(want), got_words, words)
    bad = np.nonzero(buf[:n] != np.frombuffer(want, dtype=np.uint8))[0]
    assert bad.size == 0, bad[:8]
    assert (buf[n:] == FILL).all()                               # the bytes behind the output's end are untouched
    assert gzip.decompress(buf[:n].tobytes() + D.EOF) == text


@pytest.mark.parametrize('name,shift', [('block+1', 1), ('one-byte', 3), ('segment-end', 2)])
def test_device_entry_on_a_text_that_lies_on_no_word(name, shift):
    text = D.text(name)
    want, words = twin(text)
    n, got_words, buf = device_deflate(text, shift=shift)
    assert buf[:n].tobytes() == want and (got_words == words).all() and (buf[n:] == FILL).all()


@pytest.mark.parametrize('round_', [1, 2])
def test_device_entry_over_several_rounds(round_, monkeypatch):
    """the members of a text go through their slots a round at a time (2048 of them; fewer here): the rounds' bytes lie one behind
    the other"""
    monkeypatch.setenv('KVQ_DEFLATE_ROUND', str(round_))
    text = emitted('counts')[0]
    assert len(text) > 5 * D.BLOCK
    want, words = twin(text)
    n, got_words, buf = device_deflate(text)
    assert buf[:n].tobytes() == want and (got_words == words).all() and (buf[n:] == FILL).all()


def test_device_entry_refuses_a_short_buffer():
    text = D.text('two-blocks+1')
    want, _ = twin(text)
    d_in, d_out = scan.DeviceBuffer(len(text)), scan.DeviceBuffer(len(want) + 64)
    d_in.upload(np.frombuffer(text, dtype=np.uint8)); d_out.upload(np.full(len(want) + 64, FILL, dtype=np.uint8))
    with pytest.raises(RuntimeError):
        scan.deflate_bgzf_device(d_in.ptr, len(text), d_out.ptr, len(want) - 1)
    assert (d_out.download(65, len(want) - 1) == FILL).all()     # nothing at or behind the cap
    n, _ = scan.deflate_bgzf_device(d_in.ptr, len(text), d_out.ptr, len(want))
    assert d_out.download(n).tobytes() == want
    d_in.free(); d_out.free()


# ---- the scan ----------------------------------------------------------------------------------------------------------------------

def upload(arr, guard=64):
    d = scan.DeviceBuffer(arr.nbytes + guard - 64)
    d.upload(np.concatenate([arr, np.full(guard, 0xAA, dtype=np.uint8)]))
    return d


def scan_device(t, arr, co, **kw):
    """-> (result, the buffer's bytes after the scan); the guards of the emit's store are checked here"""
    d = upload(arr)
    s = scan.Scanner(t, **kw)
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    r = s.finish()
    if kw.get('emit'):
        assert _lib.lib().kvq_scan_emit_guard(s.h) == 0
    s.close()
    after = d.download(arr.nbytes + 64)
    d.free()
    return r, after


def check_compressed(r, batches, emit_words):
    """the stream is BGZF of every batch's emitted text, one behind the other, and one EOF member; the words are the twins' sums"""
    got = r['emitted'].tobytes()
    want = b''.join(twin(b)[0] for b in batches if b) + D.EOF
    assert len(got) == len(want) and got == want
    assert gzip.decompress(got) == b''.join(batches)
    z = r['emit_compress']
    tw = [twin(b)[1] for b in batches if b]
    sums = np.sum(tw, axis=0) if tw else np.zeros(8, dtype=np.int64)
    assert z['words'][:6].tolist() == sums[:6].tolist() and z['words'][6:].tolist() == (np.max(tw, axis=0)[6:].tolist() if tw else [0, 0])
    assert (r['emit'].words == emit_words).all()                 # the eight emit words are unchanged
    assert z['bytes_in'] == r['emit'].bytes_out == sum(map(len, batches)) and z['bytes_out'] + 28 == len(got)
    assert z['members'] == sum((len(b) + D.BLOCK - 1) // D.BLOCK for b in batches)
    assert r['emit_deflate_kernel_ms'] > 0 or not any(batches)


@pytest.mark.parametrize('name', ['trims', 'counts', 'reveal'])
def test_scan_byte_for_byte(name):
    text, co, seqs, cfg = case(name)
    want, words = emitted(name)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    plain, _ = scan_device(t, arr, co, emit=True)
    assert plain['emitted'].tobytes() == want and 'emit_compress' not in plain and 'emit_deflate_kernel_ms' not in plain
    r, after = scan_device(t, arr, co, emit=True, emit_compress=True)
    check_compressed(r, [want], words)
    assert gzip.decompress(r['emitted'].tobytes()) == plain['emitted'].tobytes()
    # the batch's text is only read, the scan is what it is without the option
    assert (after[:arr.nbytes] == arr).all() and (after[arr.nbytes:] == 0xAA).all()
    assert r['hits'] == plain['hits'] and r['hitseqs'] == plain['hitseqs'] and r['stats'] == plain['stats'] and (r['counters'] == plain['counters']).all()
    if name == 'counts':
        assert r['emit_compress']['members'] >= 3 and r['emit_compress']['stored'] == 0 and r['emit_compress']['ratio'] > 2
    t.close()


def test_a_scan_that_emits_nothing_yields_the_eof_member_alone():
    text = E.dropped_text()
    t = scan.Table(E.SEQ, **E.CFG)
    r, _ = scan_device(t, np.frombuffer(text, dtype=np.uint8), (0, len(text)), emit=True, emit_compress=True)
    assert r['emitted'].tobytes() == D.EOF and gzip.decompress(D.EOF) == b'' and r['emit_compress']['words'].tolist() == [0] * 8
    assert r['emit'].records == 600 and r['emit'].emitted == 0
    t.close()


def test_beside_the_clip_and_the_records():
    text, co, seqs, cfg = case('reveal')
    want, words = emitted('reveal', clip=True)
    assert want != emitted('reveal')[0]
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, after = scan_device(t, arr, co, emit=True, emit_compress=True, clip=PROBES, records=True)
    check_compressed(r, [want], words)
    plain, after2 = scan_device(t, arr, co, emit=True, clip=PROBES, records=True)
    assert r['records'] == plain['records'] and len(r['records']) == len(r['hits']) > 100 and (r['clip'].words == plain['clip'].words).all()
    assert (after == after2).all()
    t.close()


def batches_of(text, cuts, amin, m):
    return [P.emit_host(text[x:y], amin, m, [0, y - x])[0].tobytes() for x, y in zip(cuts, cuts[1:])]


def test_several_batches_under_chunk_cuts_and_a_reset():
    text, co, seqs, cfg = case('reveal')
    want, words = emitted('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    s = scan.Scanner(t, emit=True, emit_compress=True)
    ends = E.record_ends(text)
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    for i, (x, y) in enumerate(zip(cuts, cuts[1:])):
        mid = ends[len(ends) // 2] - x
        s.scan_host(arr[x:y], chunk_off=[0, mid, y - x] if i == 1 else [0, y - x], fpos_base=x)
    first = s.finish()
    parts = batches_of(text, cuts, E.AMIN, E.MINLEN)
    assert b''.join(parts) == want
    check_compressed(first, parts, words)                        # every batch its own members: the stream differs from BGZF of the whole
    assert first['emitted'].tobytes() != twin(want)[0] + D.EOF
    same_as_oracle(first, oracle('reveal'))
    # a reset carries nothing over: only the tail of the text, then all of it in one batch
    cut = ends[299]
    pw, pwords = P.emit_host(text[cut:], E.AMIN, E.MINLEN, [0, len(text) - cut])
    s.reset()
    s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut])
    check_compressed(s.finish(), [pw.tobytes()], pwords)
    s.reset()
    s.scan_host(arr, chunk_off=list(co))
    again = s.finish()
    check_compressed(again, [want], words)
    assert _lib.lib().kvq_scan_emit_guard(s.h) == 0 and again['hits'] == first['hits']
    s.close(); t.close()


@pytest.mark.parametrize('how', ['device', 'host', 'file'])
def test_a_rescan_after_an_arena_overflow_emits_once(how, monkeypatch, tmp_path):
    """an arena of 64 hits overflows and the batches run again: the sink was emptied with the arena (a file: truncated), the
    stream is there once, with one EOF member"""
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    text, co, seqs, cfg = case('reveal')
    want, words = emitted('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    out = str(tmp_path / 'out.fastq.gz')
    s = scan.Scanner(t, emit=out if how == 'file' else True, emit_compress=True)
    assert s.order_info()['arena_cap'] == 64
    d = upload(arr)
    if how == 'device':
        s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
        parts = [want]
    else:
        cut = E.record_ends(text)[300]
        s.scan_host(arr[:cut], chunk_off=[0, cut])
        s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut], fpos_base=cut)
        parts = batches_of(text, [0, cut, len(text)], E.AMIN, E.MINLEN)
    r = s.finish()
    assert s.order_info()['arena_cap'] > 64 and len(r['hits']) > 100
    same_as_oracle(r, oracle('reveal'))
    if how == 'file':
        assert 'emitted' not in r and (r['emit'].words == words).all() and _lib.lib().kvq_scan_emit_guard(s.h) == 0
        s.close()
        with open(out, 'rb') as f:
            got = f.read()
        assert got == b''.join(twin(b)[0] for b in parts) + D.EOF and got.count(D.EOF) == 1 and gzip.decompress(got) == want
    else:
        check_compressed(r, parts, words)
        assert r['emitted'].tobytes().count(D.EOF) == 1
        s.close()
    d.free(); t.close()


def test_where_one_workgroup_walks_all_the_tiles(tmp_path):
    """KVQ_GRID=1 is read once per process: a child scans `reveal` with the emit and its deflate on and hands back what it got"""
    text, co, seqs, cfg = case('reveal')
    want, words = emitted('reveal')
    (tmp_path / 'reveal.fastq').write_bytes(text)
    res = str(tmp_path / 'res.npz')
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, 'deflate_grid_child.py'), str(tmp_path / 'reveal.fastq'), res],
                           env=dict(os.environ, KVQ_GRID='1'), capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.exit('the deflate child under KVQ_GRID=1 did not end within 120 s\n%s\n%s' % (e.stdout, e.stderr), 1)
    said = p.stdout + p.stderr
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or 'illegal memory access' in said:
        pytest.exit('the deflate child under KVQ_GRID=1 ended with status %d\n%s' % (p.returncode, said), 1)
    assert p.returncode == 0 and 'deflate grid child ok' in p.stdout, said
    z = np.load(res)
    assert int(z['grid']) == 1 and bool(z['seeded']) and int(z['guard']) == 0
    assert z['emitted'].tobytes() == twin(want)[0] + D.EOF and (z['words'] == words).all() and (z['zwords'] == twin(want)[1]).all()
    assert z['file_pos'].tolist() == [h.file_pos for h in oracle('reveal')['hits']]


# ---- findseqs, and the round trip --------------------------------------------------------------------------------------------------

def test_findseqs_and_the_round_trip(tmp_path):
    text, _, seqs, cfg = case('reveal')
    want, words = emitted('reveal')
    saved = engine.get_config()
    engine.config(**cfg)
    try:
        (tmp_path / 'm.fastq').write_bytes(text)
        (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
        o = oracle('reveal')
        out = str(tmp_path / 'out.fastq')                         # (the suffix decides nothing)
        for name, kw, route in (('m.fastq', {}, 'host'), ('b.fastq.gz', {'inflate': 'device'}, 'device')):
            r = engine.findseqs(str(tmp_path / name), list(seqs), emit=out, emit_compress=True, **kw)
            assert engine.last_inflate() == route, (name, engine.last_inflate())
            assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs'], name
            assert (r['emit'].words == words).all() and (r['emit_compress']['words'] == twin(want)[1]).all() and r['emit_deflate_kernel_ms'] > 0, name
            with open(out, 'rb') as f:
                assert f.read() == twin(want)[0] + D.EOF, name
        # without the option the same path holds plain text, 'x.gz' or not
        gz = str(tmp_path / 'plain.gz')
        r = engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs), emit=gz)
        with open(gz, 'rb') as f:
            assert f.read() == want and 'emit_compress' not in r
        # BAM: its virtual FastQ text, trimmed and deflated
        data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
        vtext = bam.to_fastq_host(data)
        vw, vwords = P.emit_host(vtext, E.AMIN, E.MINLEN, [0, len(vtext)])
        r = engine.findseqs(str(tmp_path / 'm.bam'), list(seqs), emit=out, emit_compress=True)
        assert engine.last_inflate() == 'device_bam' and (r['emit'].words == vwords).all()
        with open(out, 'rb') as f:
            assert f.read() == twin(vw.tobytes())[0] + D.EOF
        # a profile-only call
        out = str(tmp_path / 'out.fastq.gz')                      # (for the round trip: the input's route goes by its name)
        p = P.profile(str(tmp_path / 'm.fastq'), cutoffs=[E.AMIN], emit=out, emit_compress=True)
        assert p.emit_compressed['bytes_in'] == len(want) == p.emitted.bytes_out
        with open(out, 'rb') as f:
            assert f.read() == twin(want)[0] + D.EOF
        with pytest.raises(ValueError):
            engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs), emit_compress=True)
        # the round trip: the written file on the device-inflate route gives the hits of the plain emitted text, in the same order
        (tmp_path / 'emitted.fastq').write_bytes(want)
        r1 = engine.findseqs(str(tmp_path / 'emitted.fastq'), list(seqs))
        r2 = engine.findseqs(out, list(seqs), inflate='device')
        assert engine.last_inflate() == 'device'
        key = lambda hits: [(h.seq_nr, h.seq_pos, h.length, h.readlength, h.file_pos) for h in hits]
        assert key(r1['hits']) == key(r2['hits']) and r1['hitseqs'] == r2['hitseqs'] and len(r1['hits']) > 100
        o2 = O.scan_memory(np.frombuffer(want, dtype=np.uint8), list(seqs), fold=True, **dict(cfg, nthreads=4))
        for r in (r1, r2):
            assert tuple(r['hits']) == tuple(o2['hits']) and r['hitseqs'] == o2['hitseqs']
            for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
                assert r['stats'][k] == o2['stats'][k], k
        assert [(h.seq_nr, h.seq_pos, h.length, h.readlength) for h in o2['hits']] == [(h.seq_nr, h.seq_pos, h.length, h.readlength) for h in o['hits']]
    finally:
        engine.config(**saved)


# ---- the option's rules ------------------------------------------------------------------------------------------------------------

def test_refusals():
    L = _lib.lib()
    arr = np.frombuffer(b'@r\nACGTACGT\n+\nIIII#III\n' * 2, dtype=np.uint8)
    t = scan.Table(E.SEQ, **E.CFG)
    s = scan.Scanner(t)
    assert L.kvq_scan_set_emit_compress(s.h, 1) == _lib.ERR_RUNTIME and 'kvq_scan_set_emit first' in _lib.last_error()[1]
    assert not L.kvq_scan_emit_compress(s.h) and L.kvq_scan_emit_deflate_kernel_ms(s.h) == 0
    assert L.kvq_scan_set_emit(s.h, 1, 3) == 0 and L.kvq_scan_set_emit_compress(s.h, 1) == 0
    s.scan_host(arr)
    assert L.kvq_scan_set_emit_compress(s.h, 0) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    s.finish()
    ptr, n = C.c_void_p(), C.c_int64()
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == 0
    got = C.string_at(ptr.value, n.value)
    assert gzip.decompress(got) == b'@r\nACGT\n+\nIIII\n' * 2 and got == twin(b'@r\nACGT\n+\nIIII\n' * 2)[0] + D.EOF
    zw = np.ctypeslib.as_array(L.kvq_scan_emit_compress(s.h), shape=(8,)).tolist()
    assert zw[:3] == [1, 30, len(got) - 28] and zw == twin(b'@r\nACGT\n+\nIIII\n' * 2)[1].tolist()
    # off again: the text as it was
    s.reset()
    assert L.kvq_scan_set_emit_compress(s.h, 0) == 0
    s.scan_host(arr); s.finish()
    assert L.kvq_scan_emitted(s.h, C.byref(ptr), C.byref(n)) == 0 and C.string_at(ptr.value, n.value) == b'@r\nACGT\n+\nIIII\n' * 2
    assert not L.kvq_scan_emit_compress(s.h) and L.kvq_scan_emit_deflate_kernel_ms(s.h) == 0
    s.close()
    with pytest.raises(ValueError):
        scan.Scanner(t, emit_compress=True)
    t.close()
