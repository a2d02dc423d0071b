"""
The adapter clip on an MI355X (``kvq_clip_records``; include/kvarq_hip.h).  Byte for byte: what the kernel
leaves in a batch's buffer is MASK(text) as the CPU twin makes it (tests/test_clip_host.py ties the twin to the plain statement),
with nothing written behind the text, and the eight words are the twin's.  The contract: a scan with ``clip=`` returns what the
same scan without it returns on MASK(text), uploaded separately, and what the oracle returns on MASK(text) -- on the seeded path,
the exhaustive kernels, the read-list route, through the redo of skipped tiles, the redo of a whole batch, a rescan after an arena
overflow and a reset, with the records of the hits, beside the profile, and through every route of ``findseqs``.
"""
import bisect
import ctypes as C
import functools

import numpy as np
import pytest

import adapt_ref as A
import bam_writer as W
import clip_ref as CR
from kvarq_amd import _lib, bam, engine, profile as P, scan
from oracle import oracle as O
from test_host_logic import bgzf

pytestmark = pytest.mark.gpu

SEQ = [b'ACGTACGTACGTACGTACGTACGTA']
PROBES = CR.PROBES[2]


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    monkeypatch.delenv('KVQ_ARENA_CAP', raising=False)


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, chunk offsets, sequences, config) of a text of tests/clip_ref.py"""
    if name == 'stores':
        text = CR.stores_text()[0]
        return text, (0, len(text)), tuple(SEQ), CR.CFG
    if name == 'none':
        text = CR.none_text()
        return text, (0, len(text)), tuple(SEQ), CR.CFG
    if name == 'reveal':
        text = CR.reveal_text()[0]
        return text, tuple(O.chunk_offsets(text)), tuple(CR.TM.table()), CR.CFG
    if name == 'redo':
        text, _, _, co = CR.redo_text()
        return text, co, tuple(CR.TM.table()), CR.CFG
    text = CR.quirk_text()
    return text, tuple(O.chunk_offsets(text)), tuple(CR.quirk_seqs()), CR.QUIRK_CFG


@functools.lru_cache(maxsize=None)
def twin(name, n=2):
    """(MASK(text) as an array, the eight words) by the CPU twin; computed once, left unchanged"""
    text, co, _, _ = case(name)
    masked, words = P.clip_host(text, CR.PROBES[n], list(co))
    masked.flags.writeable = False; words.flags.writeable = False
    return masked, words


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's answer on MASK(text)"""
    _, _, seqs, cfg = case(name)
    return O.scan_memory(twin(name)[0], list(seqs), fold=True, **dict(cfg, nthreads=4))


def same_as_oracle(r, o):
    assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs']
    for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
        assert r['stats'][k] == o['stats'][k], k
    assert r['coverage'].tolist() == o['coverage'] and r['mutations'].tolist() == o['mutations']
    assert int(r['counters'][_lib.CTR_HITS]) == len(o['hits'])


def same_scan(a, b):
    assert b['hits'] == a['hits'] and b['hitseqs'] == a['hitseqs'] and b['stats'] == a['stats']
    assert (b['counters'] == a['counters']).all() and (b['coverage'] == a['coverage']).all() and (b['mutations'] == a['mutations']).all()


def check_clip(r, words):
    c = r['clip']
    assert (c.words == words).all(), (c.words, words)
    assert (c.records, c.clipped, c.masked, c.bases_cut) == tuple(int(v) for v in words[1:5]) and c['records'] == c.records
    assert c.clipped <= c.records == r['counters'][_lib.CTR_RECORDS] and (r['clip_kernel_ms'] > 0 or c.records == 0)


def upload(arr, guard=64):
    """a device buffer of exactly arr.nbytes + guard bytes (DeviceBuffer adds 64 of its own), `guard` bytes of 0xAA behind the text"""
    d = scan.DeviceBuffer(arr.nbytes + guard - 64)
    d.upload(np.concatenate([arr, np.full(guard, 0xAA, dtype=np.uint8)]))
    return d


def scan_device(t, arr, co, guard=64, **kw):
    """-> (result, the buffer's bytes after the scan)"""
    d = upload(arr, guard)
    s = scan.Scanner(t, **kw)
    s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    r = s.finish()
    s.close()
    after = d.download(arr.nbytes + guard)
    d.free()
    return r, after


# ---- byte for byte -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', sorted(CR.PROBES))
@pytest.mark.parametrize('name', ['stores', 'reveal', 'none'])
def test_byte_for_byte(name, n):
    if name == 'stores':
        CR.stores_census()
    elif name == 'reveal':
        CR.reveal_census()
    text, co, seqs, cfg = case(name)
    masked, words = twin(name, n)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    # 64 guard bytes of 0xAA behind the text
    r, after = scan_device(t, arr, co, clip=CR.PROBES[n])
    bad = np.nonzero(after[:arr.nbytes] != masked)[0]
    assert bad.size == 0, (bad[:8], after[bad[:8]], masked[bad[:8]])
    assert (after[arr.nbytes:] == 0xAA).all()
    check_clip(r, words)
    # a buffer that ends on the text's last byte
    r, after = scan_device(t, arr, co, guard=0, clip=CR.PROBES[n])
    assert (after == masked).all()
    check_clip(r, words)
    # three host batches cut between records
    ends = CR.record_ends(text)
    cuts = [0, ends[len(ends) // 3 - 1], ends[2 * len(ends) // 3 - 1], len(text)]
    s = scan.Scanner(t, clip=CR.PROBES[n])
    for x, y in zip(cuts, cuts[1:]):
        s.scan_host(arr[x:y], chunk_off=[0, y - x], fpos_base=x)
    three = s.finish()
    s.close()
    check_clip(three, words)
    same_scan(r, three)
    t.close()


def test_clip_off_writes_nothing_and_returns_nothing():
    text, co, seqs, cfg = case('stores')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, after = scan_device(t, arr, co)
    assert 'clip' not in r and 'clip_kernel_ms' not in r and (after[:arr.nbytes] == arr).all() and (after[arr.nbytes:] == 0xAA).all()
    s = scan.Scanner(t)
    assert not _lib.lib().kvq_scan_clip(s.h) and _lib.lib().kvq_scan_clip_kernel_ms(s.h) == 0
    s.close(); t.close()


# ---- the contract ----------------------------------------------------------------------------------------------------------------

def reveal_set(name):
    if name == 'reveal':
        text, read_off, _ = CR.reveal_text(); co = [0, len(text)]
    else:
        text, read_off, _, co = CR.redo_text()
    return CR.revealed(text, read_off, co, PROBES)[0]


@pytest.mark.parametrize('route', ['seeded', 'exhaustive', 'long_reads', 'tiles_rescanned', 'rescanned'])
def test_scan_with_clip_is_the_scan_of_the_masked_text(route):
    name = {'tiles_rescanned': 'redo', 'rescanned': 'quirk'}.get(route, 'reveal')
    if name != 'quirk':
        CR.reveal_census(name)
    text, co, seqs, cfg = case(name)
    masked, words = twin(name)
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    kw = {'long_reads': True} if route == 'long_reads' else {}
    res = []
    for data, more in ((arr, dict(clip=PROBES)), (masked, {})):
        d = upload(data)
        s = scan.Scanner(t, **dict(kw, **more))
        if route == 'exhaustive':
            s.force_exhaustive()
        if route == 'rescanned':
            s.scan_host(data, chunk_off=list(co))                    # (settled while its text is in the staging buffer, which the clip has masked)
        else:
            s.scan_device(d.ptr, data.nbytes, np.array(co, dtype=np.int64))
        res.append(s.finish())
        s.close()
        if more and route != 'rescanned':
            assert (d.download(data.nbytes) == masked).all()
        d.free()
    clipped, plain = res
    check_clip(clipped, words)
    same_scan(plain, clipped)
    same_as_oracle(clipped, oracle(name))
    path = clipped['path']
    assert path == plain['path']
    if route == 'seeded':
        assert path['seeded'] and not path['rescanned']
    elif route == 'exhaustive':
        assert path['exhaustive'] and not path['seeded']
    elif route == 'long_reads':
        assert path['read_list'] and not path['seeded']
    elif route == 'tiles_rescanned':
        assert path['seeded'] and path['tiles_rescanned'] and not path['rescanned']
    else:
        assert path['rescanned'] and len(oracle(name)['hits']) > 50      # (the redo has hits to get right: the oracle's count)
    if name != 'quirk':
        assert {(h.file_pos, h.readlength) for h in clipped['hits']} == reveal_set(name)
    t.close()


@pytest.mark.parametrize('how', ['device', 'host'])
def test_a_rescan_after_an_arena_overflow_masks_again_and_counts_anew(how, monkeypatch):
    """an arena of 64 hits overflows: the library replays a device batch -- whose text is already masked --, Scanner feeds host
    batches again; the results and the eight words are those of one scan"""
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    text, co, seqs, cfg = case('reveal')
    masked, words = twin('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    s = scan.Scanner(t, clip=PROBES)
    assert s.order_info()['arena_cap'] == 64
    d = upload(arr)
    if how == 'device':
        s.scan_device(d.ptr, arr.nbytes, np.array(co, dtype=np.int64))
    else:
        cut = CR.record_ends(text)[300]
        s.scan_host(arr[:cut], chunk_off=[0, cut])
        s.scan_host(arr[cut:], chunk_off=[0, len(text) - cut], fpos_base=cut)
    r = s.finish()
    assert s.order_info()['arena_cap'] > 64 and len(r['hits']) > 600
    check_clip(r, words)
    same_as_oracle(r, oracle('reveal'))
    if how == 'device':
        assert (d.download(arr.nbytes) == masked).all()
    s.close(); d.free(); t.close()


def test_a_reset_carries_nothing_over():
    text, co, seqs, cfg = case('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    s = scan.Scanner(t, clip=PROBES)
    s.scan_host(arr, chunk_off=list(co))
    first = s.finish()
    check_clip(first, twin('reveal')[1])
    cut = CR.record_ends(text)[299]
    part = text[cut:]
    pm, pw = P.clip_host(part, PROBES, [0, len(part)])
    s.reset()
    s.scan_host(arr[cut:], chunk_off=[0, len(part)])
    second = s.finish()
    check_clip(second, pw)
    assert second['clip'].records == first['clip'].records - 300
    o = O.scan_memory(pm, list(seqs), fold=True, **cfg)
    same_as_oracle(second, o)
    s.reset()
    s.scan_host(arr, chunk_off=list(co))
    again = s.finish()
    same_scan(first, again)
    assert again['clip'] == first['clip']
    s.close(); t.close()


def test_the_records_of_the_hits_are_slices_of_the_masked_text():
    text, co, seqs, cfg = case('reveal')
    masked = twin('reveal')[0].tobytes()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, arr, co, clip=PROBES, records=True)
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


def test_beside_the_profile():
    """profile, cycles and the adapter content of the same probes beside the clip: the profile is that of MASK(text), the adapter
    words are those of the text as it lay -- the bases are the same --, and the identities between the two hold"""
    text, co, seqs, cfg = case('reveal')
    masked, words = twin('reveal')
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table(list(seqs), **cfg)
    r, _ = scan_device(t, arr, co, profile=[CR.AMIN], cycles=True, adapters=PROBES, clip=PROBES)
    check_clip(r, words)
    want = P.profile_host(masked, [CR.AMIN], list(co), cycles=True, adapters=PROBES)
    unmasked = P.profile_host(text, [CR.AMIN], list(co), cycles=True, adapters=PROBES)
    p = r['profile']
    assert p == want and p != unmasked and p.adapters == unmasked.adapters
    a, c = p.adapters, r['clip']
    assert c.clipped <= c.records == a.records == p.records and c.clipped == a.with_adapter + a.tail_only
    assert p.raw_lengths[1024] == 0 and c.bases_cut == (np.arange(1025) * p.raw_lengths).sum() - (np.arange(1025) * a.clip).sum()
    assert p.readlengths(CR.AMIN) == r['stats']['readlengths']
    same_as_oracle(r, oracle('reveal'))
    t.close()


def test_every_route_of_findseqs(tmp_path):
    text, _, seqs, cfg = case('reveal')
    masked, words = twin('reveal')
    engine.config(**cfg)
    (tmp_path / 'm.fastq').write_bytes(text)
    (tmp_path / 'b.fastq.gz').write_bytes(bgzf(text))
    o = oracle('reveal')
    for name, kw, route in (('m.fastq', {}, 'host'), ('b.fastq.gz', {'inflate': 'device'}, 'device')):
        r = engine.findseqs(str(tmp_path / name), list(seqs), clip=PROBES, **kw)
        assert engine.last_inflate() == route
        assert tuple(r['hits']) == tuple(o['hits']) and r['hitseqs'] == o['hitseqs'], name
        for k in ('readlengths', 'nseqhits', 'nseqbasehits', 'records_parsed'):
            assert r['stats'][k] == o['stats'][k], (name, k)
        assert (r['clip'].words == words).all() and r['clip'].probes == PROBES and r['clip_kernel_ms'] > 0 and 'profile' not in r
    plain = engine.findseqs(str(tmp_path / 'm.fastq'), list(seqs))
    assert 'clip' not in plain and tuple(plain['hits']) != tuple(o['hits'])       # the kept scan object has given the option up
    # a profile-only call: the profile of the masked text, and what the clip did
    p = P.profile(str(tmp_path / 'm.fastq'), cutoffs=[CR.AMIN], clip=PROBES)
    assert p == P.profile_host(masked, [CR.AMIN]) and (p.clipped.words == words).all()
    # BAM: the clip of its virtual FastQ text
    data = W.write(str(tmp_path / 'm.bam'), W.header(), W.from_fastq(text))
    vtext = bam.to_fastq_host(data)
    vmasked, vwords = P.clip_host(vtext, PROBES, O.chunk_offsets(vtext))
    vo = O.scan_memory(vmasked, list(seqs), **dict(cfg, nthreads=4))
    r = engine.findseqs(str(tmp_path / 'm.bam'), list(seqs), clip=PROBES)
    assert engine.last_inflate() == 'device_bam' and tuple(r['hits']) == tuple(vo['hits']) and r['hitseqs'] == vo['hitseqs']
    assert r['stats']['readlengths'] == vo['stats']['readlengths'] and (r['clip'].words == vwords).all() and vwords[CR.C_CLIPPED] > 600


def test_refusals_and_with_a_communicator():
    L = _lib.lib()
    one = (C.c_char_p * 1)(A.P12)
    len1 = (C.c_int32 * 1)(12)
    arr = np.frombuffer(A.rec(b'CC' + A.P12 + b'TTTT') * 2, dtype=np.uint8)
    # an Amin that '!' does not fall below, as a signed char
    for amin in (b'!', b'\x05', b'\x80'):
        t = scan.Table(SEQ, **dict(CR.CFG, Amin=amin))
        with pytest.raises(ValueError):
            scan.Scanner(t, clip=[A.P12])
        s = scan.Scanner(t)
        assert L.kvq_scan_set_clip(s.h, one, len1, 1) == _lib.ERR_RUNTIME and "not above '!'" in _lib.last_error()[1]
        assert L.kvq_scan_set_clip(s.h, None, None, 0) == 0
        s.close(); t.close()
    t = scan.Table(SEQ, **dict(CR.CFG, Amin=b'"'))
    s = scan.Scanner(t)
    # the probe rules; a refused call leaves the option as it was: off
    for probe, n in ((b'ACGTACG', 1), (b'A' * 33, 1), (b'ACGTACGa', 1), (b'ACGTNCGT', 1), (A.P12, 9), (A.P12, -1)):
        k = max(n, 1)
        assert L.kvq_scan_set_clip(s.h, (C.c_char_p * k)(*[probe] * k), (C.c_int32 * k)(*[len(probe)] * k), n) == _lib.ERR_RUNTIME
        assert 'upper-case A C G T' in _lib.last_error()[1]
    # no profile needed; only before the first batch or after a reset
    assert L.kvq_scan_set_clip(s.h, one, len1, 1) == 0 and not L.kvq_scan_clip(s.h)
    s.scan_host(arr)
    assert L.kvq_scan_set_clip(s.h, None, None, 0) == _lib.ERR_RUNTIME and 'before the first batch' in _lib.last_error()[1]
    s.finish()
    words = np.ctypeslib.as_array(L.kvq_scan_clip(s.h), shape=(CR.LEN,))
    assert words.tolist() == [1, 2, 2, 32, 32, 0, 0, 0] and L.kvq_scan_clip_kernel_ms(s.h) > 0
    s.reset()
    assert L.kvq_scan_set_clip(s.h, None, None, 0) == 0
    s.scan_host(arr); s.finish()
    assert not L.kvq_scan_clip(s.h) and L.kvq_scan_clip_kernel_ms(s.h) == 0
    s.close()
    # with a communicator: allowed, the words are the rank's own
    comm = L.kvq_comm_create_local(1, 0, 0x636c6970)
    assert comm
    s = scan.Scanner(t, clip=[A.P12])
    assert L.kvq_scan_set_comm(s.h, comm) == 0
    s.scan_host(arr)
    assert L.kvq_scan_finish(s.h) == 0
    assert np.ctypeslib.as_array(L.kvq_scan_clip(s.h), shape=(CR.LEN,)).tolist() == [1, 2, 2, 32, 32, 0, 0, 0]
    assert L.kvq_scan_set_comm(s.h, None) == 0
    s.close()
    L.kvq_comm_destroy(comm)
    t.close()
    # the flag of kvq_findseqs_opts / kvq_findseqs_ex: not tied to the profile's, refused without the structure that holds the probes
    files = (C.c_char_p * 1)(b'/nonexistent.fastq')
    seq = (C.c_char_p * 1)(b'ACGTACGTACGT')
    lens = (C.c_int32 * 1)(12)
    opts = _lib.FindOpts(C.sizeof(_lib.FindOpts), _lib.FIND_CLIP, 0, (C.c_uint8 * 8)())
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.byref(opts))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    assert not L.kvq_findseqs_ex(files, 1, seq, lens, 1, _lib.FIND_CLIP)
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and 'bad size' in _lib.last_error()[1]
    big = _lib.FindOptsAdapters(_lib.FindOpts(C.sizeof(_lib.FindOptsAdapters), _lib.FIND_CLIP, 0, (C.c_uint8 * 8)()), 0)
    assert not L.kvq_findseqs_opts(files, 1, seq, lens, 1, C.cast(C.byref(big), C.POINTER(_lib.FindOpts)))
    assert _lib.last_error()[0] == _lib.ERR_RUNTIME and '1 to 8 probes' in _lib.last_error()[1]
