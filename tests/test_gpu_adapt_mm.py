"""
Adapter probes that tolerate mismatches on an MI355X (``kvq_adapt_records_mm``, ``kvq_clip_records_mm``; include/kvarq_hip.h,
DESIGN section 20).  The adapters array word for word against the plain statement of the rule (tests/adapt_mm_ref.py) on every
text -- each asserts its census first --, through ``Scanner`` under chunk and batch cuts of a few KB and through ``findseqs``;
what the clip leaves in a batch's buffer byte for byte against the CPU twin's text (tests/test_adapt_mm_host.py ties the twin to
the plain statement), with nothing written behind it; section 19's contract at per = 10 -- a scan with the clip on returns what
the oracle returns on MASK_per(text) -- on every route; the identities between the two arrays; and per == 0, set through the
new call, against a scan that never heard of it.
"""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import adapt_mm_ref as M
import adapt_ref as A
import bam_writer as W
import cases
import clip_ref as CR
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

SEQ = [b'ACGTACGTACGTACGTACGTACGTA']
PROBES = CR.PROBES[2]
RUNS = [(name, per) for name in sorted(M.texts()) for per in M.texts()[name][2]]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv('KVQ_ARENA_CAP', raising=False)


@functools.lru_cache(maxsize=None)
def want(name, per, co=None):
    """the plain statement's adapters array of a text; computed once, left unchanged"""
    text, probes, _, _ = M.texts()[name]
    w = M.adapt(text, list(co) if co is not None else [0, len(text)], probes, per)
    w.flags.writeable = False
    return w


def same_words(got, w):
    bad = np.nonzero(got != w)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], w[bad[:8]])


def cuts_of(text, step):
    """record ends at least ``step`` bytes apart, the text's end among them"""
    out = [0]
    for e in CR.record_ends(text):
        if e - out[-1] >= step or e == len(text):
            out.append(e)
    return out


@pytest.mark.parametrize('name,per', RUNS)
def test_adapters_array_under_chunk_and_batch_cuts(name, per):
    """one device batch whose buffer ends with the text's last byte and whose chunks are cut every few KB, then host batches of a
    few KB each; the clip beside it counts the same records"""
    M.check_census(name)
    text, probes, _, _ = M.texts()[name]
    arr = np.frombuffer(text, dtype=np.uint8)
    w = want(name, per)
    t = scan.Table(SEQ, **CR.CFG)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    s = scan.Scanner(t, adapters=probes, clip=probes, adapter_mismatches=per)
    assert _lib.lib().kvq_scan_adapter_mismatches(s.h) == per
    s.scan_device(d.ptr, arr.nbytes, np.array(cuts_of(text, 3000), dtype=np.int64))
    one = s.finish()
    a, c = one['profile'].adapters, one['clip']
    same_words(a.words, w)
    M.check_identities(a.words)
    assert a.mismatch_per == c.mismatch_per == per and (a.first_mismatches.sum(axis=1) == a.found).all()
    assert c.words[2] == a.with_adapter + a.tail_only and c.records == a.records == one['counters'][_lib.CTR_RECORDS]
    assert one['adapt_kernel_ms'] > 0 and one['clip_kernel_ms'] > 0
    s.reset()
    cuts = cuts_of(text, 4096)
    for x, y in zip(cuts, cuts[1:]):
        s.scan_host(arr[x:y], chunk_off=[0, y - x], fpos_base=x)
    many = s.finish()
    same_words(many['profile'].adapters.words, w)
    assert many['clip'] == c and many['hits'] == one['hits']
    s.close(); d.free(); t.close()


def test_findseqs_on_a_plain_file(tmp_path):
    engine.config(**cases.by_name()['multichunk'].config)
    seqs = cases.by_name()['multichunk'].seq_bytes()
    for name in sorted(M.texts()):
        text, probes, pers, _ = M.texts()[name]
        (tmp_path / 't.fastq').write_bytes(text)
        co = tuple(int(c) for c in O.chunk_offsets(text))
        for per in pers:
            r = engine.findseqs(str(tmp_path / 't.fastq'), seqs, adapters=probes, adapter_mismatches=per)
            same_words(r['profile'].adapters.words, want(name, per, co))
            assert r['profile'].adapters.probes == probes
    # the kept scan object gives the rate up with the option
    text, probes, _, _ = M.texts()['kinds']
    (tmp_path / 't.fastq').write_bytes(text)
    r = engine.findseqs(str(tmp_path / 't.fastq'), seqs, adapters=probes)
    assert r['profile'].adapters == P.adapt_host(text, probes, O.chunk_offsets(text)) and r['profile'].adapters.mismatch_per == 0


# ---- byte for byte -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stores_twin(n, per=10):
    """(MASK_per(stores) as an array, the eight words) by the CPU twin: ``clip_ref.stores_text`` -- every first address modulo 16
    with every length -- with a substitution in every other planted probe"""
    masked, words = P.clip_host(stores_mm_text(), CR.PROBES[n], [0, len(stores_mm_text())], adapter_mismatches=per)
    masked.flags.writeable = False; words.flags.writeable = False
    return masked, words


@functools.lru_cache(maxsize=None)
def stores_mm_text():
    CR.stores_census()
    text = bytearray(CR.stores_text()[0])
    at, n = text.find(A.P12), 0
    while at >= 0:
        if n % 2:
            text[at + n % 12] = M.wrong_byte(text[at + n % 12], ('base', 'N', 'lower', 'high')[(n // 2) % 4])
        n += 1
        at = text.find(A.P12, at + 12)
    assert n > 2000
    return bytes(text)


def upload(arr, guard=64):
    """a device buffer of exactly arr.nbytes + guard bytes (DeviceBuffer adds 64 of its own), `guard` bytes of 0xAA behind the text"""
    d = scan.DeviceBuffer(arr.nbytes + guard - 64)
    d.upload(np.concatenate([arr, np.full(guard, 0xAA, dtype=np.uint8)]))
    return d


@pytest.mark.parametrize('n', sorted(CR.PROBES))
def test_byte_for_byte(n):
    text = stores_mm_text()
    masked, words = stores_twin(n)
    exact, _ = P.clip_host(text, CR.PROBES[n], [0, len(text)])
    assert (exact != masked).sum() > 1000 and words[M.C_CLIPPED] > 2000                 # (the tolerant mask is another one)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **CR.CFG)
    d = upload(arr)
    s = scan.Scanner(t, clip=CR.PROBES[n], adapter_mismatches=10)
    s.scan_device(d.ptr, arr.nbytes, np.array([0, arr.nbytes], dtype=np.int64))
    r = s.finish()
    s.close()
    after = d.download(arr.nbytes + 64)
    d.free()
    bad = np.nonzero(after[:arr.nbytes] != masked)[0]
    assert bad.size == 0, (bad[:8], after[bad[:8]], masked[bad[:8]])
    assert (after[arr.nbytes:] == 0xAA).all()                                           # 64 guard bytes untouched behind the text
    assert (r['clip'].words == words).all() and r['clip'].mismatch_per == 10 and r['clip_kernel_ms'] > 0
    t.close()


# ---- the contract at per = 10 ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reveal():
    """(text, chunk offsets, MASK_10(text) by the twin, its words, the oracle's answer on it, the predicted (file_pos, readlength) set)"""
    M.reveal_census()
    text, read_off, _ = M.reveal_text()
    co = tuple(O.chunk_offsets(text))
    masked, words = P.clip_host(text, PROBES, list(co), adapter_mismatches=10)
    masked.flags.writeable = False; words.flags.writeable = False
    o = O.scan_memory(masked, list(CR.TM.table()), fold=True, **dict(CR.CFG, nthreads=4))
    src = masked.tobytes()
    trims = [CR.TM.trim(src[n2 + 1:n3], CR.AMIN) for _, _, n2, n3 in A.R.records_of(src, [0, len(src)])]
    predicted = set((off + s, ln) for off, (s, ln) in zip(read_off, trims) if ln >= CR.CFG['minreadlength'])
    return text, co, masked, words, o, predicted


def same_as_oracle(r, o):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], k
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations']
    assert int(r['counters'][_lib.CTR_HITS]) == len(o['hits'])


@pytest.mark.parametrize('route', ['seeded', 'exhaustive', 'long_reads'])
def test_scan_with_clip_is_the_oracle_on_the_masked_text(route):
    text, co, masked, words, o, predicted = reveal()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(CR.TM.table()), **CR.CFG)
    d = upload(arr)
    s = scan.Scanner(t, clip=PROBES, adapter_mismatches=10, **({'long_reads': True} if route == 'long_reads' else {}))
    if route == 'exhaustive':
        s.force_exhaustive()
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    r = s.finish()
    s.close()
    assert (d.download(arr.nbytes) == masked).all()
    d.free()
    assert (r['clip'].words == words).all()
    same_as_oracle(r, o)
    path = r['path']
    if route == 'seeded':
        assert path['seeded'] and not path['rescanned']
    elif route == 'exhaustive':
        assert path['exhaustive'] and not path['seeded']
    else:
        assert path['read_list'] and not path['seeded']
    assert {(h.file_pos, h.readlength) for h in r['hits']} == predicted and len(predicted) > 600
    # the exact rule gives another answer on this text
    s = scan.Scanner(t, clip=PROBES)
    s.scan_host(arr, chunk_off=list(co))
    assert tuple(s.finish()['hits']) != tuple(o['hits'])
    s.close(); t.close()


def test_the_records_of_the_hits_are_slices_of_the_masked_text():
    text, co, masked, words, o, _ = reveal()
    masked = masked.tobytes()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(CR.TM.table()), **CR.CFG)
    s = scan.Scanner(t, clip=PROBES, adapter_mismatches=10, records=True)
    s.scan_host(arr, chunk_off=list(co))
    r = s.finish()
    s.close()
    same_as_oracle(r, o)
    ends = CR.record_ends(text)
    assert len(r['records']) == len(r['hits']) > 600
    some_masked = 0
    for h, rec in zip(r['hits'], r['records']):
        i = bisect.bisect_right(ends, h.file_pos)
        start = ends[i - 1] if i else 0
        assert rec == masked[start:ends[i]]
        some_masked += rec != text[start:ends[i]]
    assert some_masked > 500
    t.close()


def test_bgzf_inflated_on_the_device_and_bam(tmp_path):
    text, _, masked, words, o, _ = reveal()
    seqs = list(CR.TM.table())
    engine.config(**CR.CFG)
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    r = engine.findseqs(str(tmp_path / 'b.fastq.gz'), seqs, clip=PROBES, adapter_mismatches=10, inflate='device')
    assert engine.last_inflate() == 'device'
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], k
    assert (r['clip'].words == words).all() and r['clip'].probes == PROBES
    # BAM: the clip of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    vmasked, vwords = P.clip_host(vtext, PROBES, O.chunk_offsets(vtext), adapter_mismatches=10)
    vo = O.scan_memory(vmasked, seqs, **dict(CR.CFG, nthreads=4))
    r = engine.findseqs(str(tmp_path / 'm.bam'), seqs, clip=PROBES, adapter_mismatches=10)
    assert engine.last_inflate() == 'device_bam' and tuple(r['hits']) == tuple(vo['hits']) and r['hitseqs'] == vo['hitseqs']
    assert r['stats']['readlengths'] == vo['stats']['readlengths'] and (r['clip'].words == vwords).all() and vwords[M.C_CLIPPED] > 700
    # the option off again: the kept scan object has given it up
    exact = engine.findseqs(str(tmp_path / 'm.bam'), seqs, clip=PROBES)
    assert exact['clip'].mismatch_per == 0 and (exact['clip'].words == P.clip_host(vtext, PROBES, O.chunk_offsets(vtext))[1]).all()


# ---- per == 0, and the call's rules ----------------------------------------------------------------------------------------------

def test_per_zero_through_the_new_call_is_a_scan_that_never_heard_of_it():
    L = _lib.lib()
    text, probes = A.texts()['aliases'][0] + A.texts()['tails'][0] + A.texts()['cr'][0], [A.P12, A.P32]
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(SEQ, **CR.CFG)
    res = []
    for zero in (False, True):
        s = scan.Scanner(t, adapters=probes, clip=probes)
        if zero:
            assert L.kvq_scan_set_adapter_mismatches(s.h, 10) == 0 and L.kvq_scan_set_adapter_mismatches(s.h, 0) == 0
        assert L.kvq_scan_adapter_mismatches(s.h) == 0
        d = upload(arr)
        s.scan_device(d.ptr, arr.nbytes, np.array([0, arr.nbytes], dtype=np.int64))
        r = s.finish()
        res.append((r['profile'].adapters.words, r['clip'].words, d.download(arr.nbytes + 64)))
        s.close(); d.free()
    for a, b in zip(*res):
        assert (a == b).all()
    assert not res[1][0][4:8].any() and not res[1][1][5:].any()
    A.check_identities(res[1][0])
    assert (res[1][0] == P.adapt_host(text, probes, [0, len(text)]).words).all()
    t.close()


def test_the_rules_of_the_call():
    L = _lib.lib()
    t = scan.Table(SEQ, **CR.CFG)
    arr = np.frombuffer(A.rec(b'CC' + M.subst(A.P12, [5]) + b'TTTT') * 2, dtype=np.uint8)
    one, len1 = (C.c_char_p * 1)(A.P12), (C.c_int32 * 1)(12)
    s = scan.Scanner(t)
    for bad in (-1, 1, 9, 33):
        assert L.kvq_scan_set_adapter_mismatches(s.h, bad) == _lib.ERR_RUNTIME and 'mismatch' in _lib.last_error()[1]
    assert L.kvq_scan_adapter_mismatches(s.h) == 0
    # order-free against the probes: the rate first, the clip behind it
    assert L.kvq_scan_set_adapter_mismatches(s.h, 12) == 0 and L.kvq_scan_set_clip(s.h, one, len1, 1) == 0
    s.scan_host(arr)
    assert L.kvq_scan_set_adapter_mismatches(s.h, 0) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    s.finish()
    assert np.ctypeslib.as_array(L.kvq_scan_clip(s.h), shape=(M.C_LEN,)).tolist() == [1, 2, 2, 32, 32, 12, 0, 0]
    # it stays while the probes go off and on, and goes only when told
    s.reset()
    assert L.kvq_scan_set_clip(s.h, None, None, 0) == 0 and L.kvq_scan_adapter_mismatches(s.h) == 12
    assert L.kvq_scan_set_clip(s.h, one, len1, 1) == 0 and L.kvq_scan_set_adapter_mismatches(s.h, 13) == 0
    s.scan_host(arr); s.finish()
    assert np.ctypeslib.as_array(L.kvq_scan_clip(s.h), shape=(M.C_LEN,)).tolist() == [1, 2, 0, 0, 0, 13, 0, 0]     # E(12) = 0 at per = 13
    s.reset()
    assert L.kvq_scan_set_adapter_mismatches(s.h, 0) == 0
    s.scan_host(arr); s.finish()
    assert np.ctypeslib.as_array(L.kvq_scan_clip(s.h), shape=(M.C_LEN,)).tolist() == [1, 2, 0, 0, 0, 0, 0, 0]
    s.close()
    with pytest.raises(ValueError):
        scan.Scanner(t, adapter_mismatches=10)
    t.close()
