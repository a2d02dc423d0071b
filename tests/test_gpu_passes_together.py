"""
All the options of a scan ON ONE SCAN OBJECT on an MI355X: the records of the hits, the profile, the per-cycle counts, the
per-read distributions and the duplication together ("the lifecycle of an input pass").  Every pass against its
CPU twin over the whole text, the hits, stats and records against the same scan without the passes -- over two host batches, a
device batch the library replays into a larger arena, the same scan object reset and fed another text, and the scan object that
``engine.findseqs`` keeps from call to call while the options go on and off.
"""
import functools
import random

import numpy as np
import pytest

import cases
from kvarq_amd import _lib, engine, profile as P, scan

pytestmark = pytest.mark.gpu

CUTS = [ord('.'), ord('I')]
CONFIG = dict(cases.DEFAULTS, minreadlength=10)
ALL = dict(records=True, profile=CUTS, cycles=True, per_read=True, duplication=True)
MS = ('profile_kernel_ms', 'cycles_kernel_ms', 'reads_kernel_ms')


@functools.lru_cache(maxsize=None)
def texts():
    """(about 600 records, most of 150 bases with a handful of score values, a few with '\\r\\n' line ends, one of 1100 bases, one
    with an empty bases line; where its second half starts; a shorter text of other records)"""
    rng = random.Random(16)

    def read(i, n=150, nl='\n'):
        return cases.rec('r%d' % i, cases.randseq(rng, n, 'ACGTACGTACGTN'), ''.join(rng.choice('!.5FI') for _ in range(n)), nl=nl)
    recs = [read(i, nl='\r\n' if i % 97 == 5 else '\n') for i in range(600)]
    recs[77] = read(77, 1100)
    recs[401] = cases.rec('empty', '', '')
    recs[402] = recs[3]                                    # (a duplicate for the table)
    return b''.join(recs), len(b''.join(recs[:300])), b''.join(read(1000 + i, 90 + i % 7) for i in range(120))


@functools.lru_cache(maxsize=None)
def twin_of(text):
    return P.profile_host(text, CUTS, [0, len(text)], cycles=True, per_read=True, duplication=True)


def check(got, plain, text):
    """a result with every option against the twin of the text and the result of the same feeding with the records alone"""
    twin = twin_of(text)
    p = got['profile']
    assert p == twin and p.cycles is not None and p.reads is not None and p.duplication is not None
    assert p.records == int(p.reads[P.READS_RECORDS]) == got['stats']['records_parsed'] == text.count(b'\n') // 4
    assert got['hits'] == plain['hits'] and got['hitseqs'] == plain['hitseqs'] and got['stats'] == plain['stats']
    assert got['records'] == plain['records'] and len(got['hits']) > 64
    assert (got['counters'] == plain['counters']).all() and 'profile' not in plain
    assert all(got[k] > 0 for k in MS)


def test_two_host_batches():
    text, half, _ = texts()
    arr = np.frombuffer(text, dtype=np.uint8)
    t = scan.Table([b'ACG'], **CONFIG)
    res = []
    for kw in (dict(records=True), ALL):
        s = scan.Scanner(t, **kw)
        s.scan_host(arr[:half]); s.scan_host(arr[half:], fpos_base=half)
        res.append(s.finish())
        s.close()
    check(res[1], res[0], text)
    assert res[1]['profile'].longest == 1100 and res[1]['profile'].duplication['unkeyed'] == 1
    t.close()


def test_replayed_device_batch_then_reset_and_another_text(monkeypatch):
    monkeypatch.setenv('KVQ_ARENA_CAP', '64')
    L = _lib.lib()
    text, _, other = texts()
    arr, arr2 = np.frombuffer(text, dtype=np.uint8), np.frombuffer(other, dtype=np.uint8)
    t = scan.Table([b'ACG'], **CONFIG)
    d = scan.DeviceBuffer(arr.nbytes); d.upload(arr)
    co = np.array([0, arr.nbytes], dtype=np.int64)
    plain, s = scan.Scanner(t, records=True), scan.Scanner(t, **ALL)
    res = []
    for sc in (plain, s):
        sc.scan_device(d.ptr, arr.nbytes, co)
        res.append(sc.finish())
    check(res[1], res[0], text)                               # (the arena of 64 hits overflowed: every record counted once)
    # the same scan objects again, with a shorter text: nothing of the first remains
    for sc in (plain, s):
        sc.reset()
    assert all(f(s.h) == 0 for f in (L.kvq_scan_profile_kernel_ms, L.kvq_scan_cycles_kernel_ms, L.kvq_scan_reads_kernel_ms))
    assert not any(bool(f(s.h)) for f in (L.kvq_scan_profile, L.kvq_scan_cycles, L.kvq_scan_reads, L.kvq_scan_dup))
    res = []
    for sc in (plain, s):
        sc.scan_host(arr2, chunk_off=[0, arr2.nbytes])
        res.append(sc.finish())
        sc.close()
    check(res[1], res[0], other)
    assert res[1]['profile'].records == 120 and res[1]['profile'] != twin_of(text)
    d.free(); t.close()


def test_the_kept_scan_object_of_findseqs(tmp_path):
    text, _, _ = texts()
    path = str(tmp_path / 'all.fastq')
    with open(path, 'wb') as f:
        f.write(text)
    engine.config(**CONFIG)
    twin = twin_of(text)
    every, none, cyc = engine.findseqs(path, [b'ACG'], **ALL), engine.findseqs(path, [b'ACG']), engine.findseqs(path, [b'ACG'], cycles=True)
    assert every['profile'] == twin and len(every['records']) == len(every['hits']) > 64
    assert 'profile' not in none and 'records' not in none
    p = cyc['profile']
    assert p.cutoffs == [] and (p.cycles == twin.cycles).all() and p.reads is None and p.duplication is None
    assert (p.words == twin.words[:P.profile_len(0)]).all()
    assert every['hits'] == none['hits'] == cyc['hits'] and every['stats'] == none['stats'] == cyc['stats']
